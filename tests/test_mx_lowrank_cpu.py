"""CPU only: include/hv_mx_lowrank.h without a GPU - the documented refusals of its two entry points through the C ABI (made-up pointers:
skipped where a GPU is present), the bindings and the generated registration source, the factorisation identity, and the flags."""
import ctypes as C
import os

import pytest
import torch

from tests import mx_lowrank_ref as LR
from tests.test_gemm_mx4_cpu import ARG, LAUNCH, PTR, ROOT, _load_script, no_gpu
from hunyuanvideo_efficiency_amd import _abi, _lib

Q, G = "hv_quant_rows_mxfp4_lr", "hv_gemm_mxfp4_lr"


def _call(name, **ov):
    a = dict(x=PTR, ldx=1024, codes=PTR, ldq=512, scales=PTR, lds=32, Dn=PTR, ldd=1024, T=PTR, ldt=64, Up=PTR, ldu=64, R=64, M=5, K=1024,
             A_codes=PTR, lda=512, A_scales=PTR, ldas=32, W_codes=PTR, ldw=512, W_scales=PTR, ldws=32, bias=None, N=264, out0=PTR, ld0=264,
             act0=0, n_split=0, out1=None, ld1=0, act1=0, gate=None, res=None, ld_res=0, stream=None)
    a.update(ov)
    params = next(p for _, n, p in _abi.MX_LOWRANK_DECLS if n == name)
    return getattr(_lib.load(), name)(*[a[p] for _, p in params])


@no_gpu
def test_refusals():
    """the accepted call fails at the launch (-2: no device), each refusal before it (-1)"""
    for name in (Q, G):
        assert all(_call(name, R=r, ldt=r, ldu=r) == LAUNCH for r in (32, 64, 96, 128)) and _call(name, M=0) == 0
        for ov in (dict(R=0), dict(R=16), dict(R=48), dict(R=160), dict(R=-32), dict(T=None), dict(T=PTR + 8), dict(ldt=68), dict(ldt=56),
                   dict(ldt=(1 << 22) + 8), dict(M=-1)):
            assert _call(name, **ov) == ARG, (name, ov)
        assert _call(name, M=1, ldt=0) == LAUNCH                       # a single row has no pitch
    for ov in (dict(Dn=None), dict(Dn=PTR + 2), dict(ldd=1028), dict(ldd=512), dict(K=1056, ldx=1056, ldq=528, lds=33, ldd=1056),
               dict(K=0), dict(x=None), dict(x=PTR + 8), dict(ldx=1028), dict(ldq=520), dict(ldq=496), dict(lds=16), dict(codes=PTR + 4),
               dict(scales=None)):
        assert _call(Q, **ov) == ARG, ov
    for ov in (dict(Up=None), dict(Up=PTR + 4), dict(ldu=60), dict(ldu=32), dict(K=384, lda=192, ldw=192), dict(K=1056, lda=528, ldw=528),
               dict(N=260), dict(lda=520), dict(A_scales=PTR + 2), dict(ldws=30), dict(ld0=260), dict(act0=3), dict(gate=PTR),
               dict(n_split=128), dict(W_codes=None), dict(out0=None)):
        assert _call(G, **ov) == ARG, ov


def test_the_header_is_bound_and_the_generated_source_is_up_to_date():
    p, i, l = C.c_void_p, C.c_int, C.c_int64
    want = {Q: [p, l, p, l, p, l, p, l, p, l, l, i, i, p],
            G: [p, l, p, l, p, l, p, l, p, i, i, i, p, l, i, i, p, l, i, p, p, l, p, l, p, l, i, p]}
    lib = _lib.load()
    assert set(_lib.MX_LOWRANK_SIGNATURES) == set(want) and _abi.MX_LOWRANK_MACROS == {"HV_MX_LR_CHUNK": 32, "HV_MX_LR_MAX": 128}
    for name, args in want.items():
        assert getattr(lib, name).argtypes == args == _lib.MX_LOWRANK_SIGNATURES[name] and getattr(lib, name).restype is i
    g = _load_script("tools/gen_torch_ops.py")
    text = g.gen(_abi.MX_LOWRANK_DECLS, "hv_mx_lowrank.h")
    assert open(g.MX_LOWRANK_OUT).read() == text, "include/hv_mx_lowrank.h changed: run python tools/gen_torch_ops.py"
    assert "TORCH_LIBRARY_FRAGMENT(hv, m)" in text and text.count("m.def(") == 2
    assert all(hasattr(_lib.torch_ops(), n[3:]) for n in want)
    mk = open(os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "Makefile")).read()
    assert mk.count("hv_mx_lowrank_torch_ops.cpp") == 2 and mk.count("../../include/hv_mx_lowrank.h") == 2 and \
        "../lib/obj/hv_mx_lowrank.o: FLAGS += -Xclang -target-feature -Xclang -packed-fp32-ops" in mk


@pytest.mark.parametrize("rank", [32, 128])
def test_factorisation_identity(rank):
    """Up Dn + Res equals W to the bf16 rounding of Res (half an ulp: 2^-9 relative, 2^-8 allowed) plus the fp32 rounding of the
    rank-R product (1e-4 at these magnitudes); the R directions carry the weight's rank-4 part, so Res is well below W; the package's
    factorise is the restatement's"""
    from hunyuanvideo_efficiency_amd import mx_lowrank
    g = torch.Generator().manual_seed(7)
    w = (torch.randn(264, 512, generator=g) + 4.0 * torch.randn(264, 4, generator=g) @ torch.randn(4, 512, generator=g)).to(torch.bfloat16)
    up, dn, res = LR.factorise(w, rank)
    assert (up.shape, dn.shape, res.shape) == ((264, rank), (rank, 512), (264, 512))
    err = (up.double() @ dn.double() + res.double() - w.double()).abs()
    assert bool((err <= res.double().abs() * 2.0 ** -8 + 1e-4).all())
    assert float(res.float().pow(2).mean().sqrt()) < 0.5 * float(w.float().pow(2).mean().sqrt())
    for a, b in zip(mx_lowrank.factorise(w, rank), (up, dn, res)):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="rank must be"):
        mx_lowrank.factorise(w, 48)


def test_flags_and_conversion_refusals():
    mod = _load_script("sample_video.py")
    assert mod.parse_args([]).mxfp4_lowrank == 0 and mod.parse_args(["--mxfp4-linears", "--mxfp4-lowrank", "96"]).mxfp4_lowrank == 96
    for argv in (["--mxfp4-lowrank", "32"], ["--mxfp4-linears", "--mxfp4-lowrank", "48"], ["--mxfp6-linears", "--mxfp4-lowrank", "32"],
                 ["--mxfp4-linears", "--mxfp4-lowrank", "32", "--mxfp4-rotate", "64"], ["--mxfp4-linears", "--use-fp8", "--mxfp4-lowrank", "32"]):
        with pytest.raises(SystemExit):
            mod.parse_args(argv)
    from hunyuanvideo_efficiency_amd.modules import mxfp4_optimization as M4
    from hunyuanvideo_efficiency_amd.modules.layers import ParamLinear
    block = torch.nn.Module()                                   # what mxfp4_optimization._blocks takes for a single block
    block.hybrid_seq_parallel_attn, block.run = None, None
    block.linear1, block.linear2 = ParamLinear(512, 8, bias=False), ParamLinear(512, 8, bias=False)
    with pytest.raises(ValueError, match="lowrank must be"):
        M4.convert_mxfp4_linear(block, lowrank=48)
    with pytest.raises(ValueError, match="not built"):
        M4.convert_mxfp4_linear(block, rot=64, lowrank=32)
    assert block.linear1.weight.dtype != torch.uint8            # refused before the first layer was packed
