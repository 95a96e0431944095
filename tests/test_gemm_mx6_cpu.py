"""CPU only: include/hv_gemm_mx6.h without a GPU - the bindings and the generated registration source, the documented refusals of its
entry points through the C ABI (made-up pointers: skipped where a GPU is present), the restatement's own edge cases, and the flags."""
import ctypes as C
import importlib.util
import os
import types

import pytest
import torch

from tests import mxfp6_ref as MX
from hunyuanvideo_efficiency_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR, ARG, LAUNCH = 0x7f0000001000, -1, -2
no_gpu = pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present: calls with made-up pointers must not reach a device")


def _load_script(rel):
    spec = importlib.util.spec_from_file_location("hvmx6_" + os.path.basename(rel)[:-3], os.path.join(ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _call(name, **ov):
    a = dict(x=PTR, ldx=1024, codes=PTR, ldq=768, scales=PTR, lds=32, M=5, K=1024, D=1024, shift=None, scale=None, eps=1e-6,
             A_codes=PTR, lda=768, A_scales=PTR, ldas=32, W_codes=PTR, ldw=768, W_scales=PTR, ldws=32, bias=None, N=264, out0=PTR, ld0=264,
             act0=0, n_split=0, out1=None, ld1=0, act1=0, gate=None, res=None, ld_res=0, stream=None)
    a.update(ov)
    params = next(p for _, n, p in _abi.GEMM_MX6_DECLS if n == name)
    return getattr(_lib.load(), name)(*[a[p] for _, p in params])


@no_gpu
@pytest.mark.parametrize("ov", [dict(K=384), dict(K=1088), dict(N=260), dict(N=0), dict(lda=776), dict(ldw=8), dict(lda=(1 << 23) + 16),
                                dict(ldas=30), dict(ldws=2), dict(A_codes=None), dict(W_codes=None), dict(out0=None), dict(A_scales=None),
                                dict(W_scales=None), dict(A_codes=PTR + 8), dict(W_codes=PTR + 8), dict(W_scales=PTR + 2), dict(ld0=260),
                                dict(ld0=256), dict(n_split=128), dict(n_split=132, out1=PTR, ld1=136), dict(n_split=128, out1=PTR, ld1=132),
                                dict(gate=PTR), dict(res=PTR, ld_res=260), dict(act0=3), dict(act1=-1), dict(M=-1)],
                         ids=["K<512", "K%128", "N%8", "N<=0", "lda%16", "ldw%16", "lda>2^23", "ldas%4", "ldws%4", "no-A", "no-W", "no-out0",
                              "no-A-scales", "no-W-scales", "A-align", "W-align", "Ws-align", "ld0%8", "pitch", "split-no-out1", "split%8",
                              "ld1%8", "gate-no-res", "ld_res%8", "act0", "act1", "M<0"])
def test_gemm_refusals(ov):
    """the accepted call fails at the launch (-2: no device), each refusal before it (-1)"""
    assert _call("hv_gemm_mxfp6") == LAUNCH and _call("hv_gemm_mxfp6", **ov) == ARG
    assert _call("hv_gemm_mxfp6", M=0) == 0 and _call("hv_gemm_mxfp6", K=512, lda=384, ldw=384) == LAUNCH and _call("hv_gemm_mxfp6", K=15360, lda=11520, ldw=11520) == LAUNCH


@no_gpu
@pytest.mark.parametrize("name,kk", [("hv_quant_rows_mxfp6", "K"), ("hv_ln_modulate_mxfp6", "D")])
def test_quantiser_refusals(name, kk):
    assert _call(name) == LAUNCH and _call(name, M=0) == 0
    for ov in ({kk: 1040}, {kk: 0}, dict(ldx=1028), dict(ldq=772), dict(ldq=760), dict(lds=16), dict(scales=None), dict(codes=None),
               dict(codes=PTR + 4), dict(x=None), dict(M=-1), dict(M=2 ** 33 + 8)):
        assert _call(name, **ov) == ARG, ov
    assert _call(name, M=1, ldq=0, lds=0) == LAUNCH and _call(name, codes=PTR + 8) == LAUNCH          # a single row has no pitch; 8-byte alignment is enough
    assert _call("hv_ln_modulate_mxfp6", D=4128, ldq=3096, lds=256) == ARG


def test_the_header_is_bound_and_the_generated_source_is_up_to_date():
    p, i, l, f = C.c_void_p, C.c_int, C.c_int64, C.c_float
    want = {"hv_quant_rows_mxfp6": [p, l, p, l, p, l, l, i, p], "hv_ln_modulate_mxfp6": [p, p, p, p, l, p, l, l, i, l, f, p],
            "hv_gemm_mxfp6": [p, l, p, l, p, l, p, l, p, i, i, i, p, l, i, i, p, l, i, p, p, l, p]}
    lib = _lib.load()
    assert set(_lib.GEMM_MX6_SIGNATURES) == set(want)
    for name, args in want.items():
        assert getattr(lib, name).argtypes == args == _lib.GEMM_MX6_SIGNATURES[name] and getattr(lib, name).restype is i
        assert [t for t, _ in next(q for _, n, q in _abi.GEMM_MX6_DECLS if n == name)] == \
            [t for t, _ in next(q for _, n, q in _abi.GEMM_MX4_DECLS if n == name.replace("fp6", "fp4"))]        # the MXFP4 argument lists
    assert _abi.GEMM_MX6_MACROS == {"HV_MX6_BLOCK": 32, "HV_MX6_BLOCK_BYTES": 24, "HV_MX6_BM": 256, "HV_MX6_BN": 256, "HV_MX6_KSTAGE": 128,
                                    "HV_MX6_RING": 3, "HV_MX6_MIN_K": 512}
    g = _load_script("tools/gen_torch_ops.py")
    text = g.gen(_abi.GEMM_MX6_DECLS, "hv_gemm_mx6.h")
    assert open(g.GEMM_MX6_OUT).read() == text, "include/hv_gemm_mx6.h changed: run python tools/gen_torch_ops.py"
    assert "TORCH_LIBRARY_FRAGMENT(hv, m)" in text and text.count("m.def(") == 3
    assert all(hasattr(_lib.torch_ops(), n[3:]) for n in want)
    mk = open(os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "Makefile")).read()
    assert mk.count("hv_gemm_mx6_torch_ops.cpp") == 2 and mk.count("../../include/hv_gemm_mx6.h") == 2


def test_restatement_round_trips_every_code():
    """all 64 codes at several scales: dequant gives the header's value table, quantising the values gives the codes back (-0 -> +0)"""
    code = torch.arange(64).repeat(4)[None, :]                                  # 8 blocks
    s = torch.tensor([[127, 127, 0, 0, 252, 252, 125, 130]], dtype=torch.uint8)
    d = MX.dequant(MX.pack(code), s)
    i = torch.arange(32).double()
    table = torch.where(i < 8, i / 8, (1 + (i.long() & 7) / 8) * torch.exp2((i.long() >> 3).double() - 1))
    assert torch.equal(d[0, :64].double(), torch.cat([table, -table])) and float(table.max()) == 7.5
    assert torch.equal(MX.unpack(MX.pack(code)), code) and MX.pack(code).shape == (1, 192)
    blk = sum(int(c) << (6 * j) for j, c in enumerate(code[0, :32]))            # the header's rule, literally
    assert bytes(MX.pack(code)[0, :24].tolist()) == blk.to_bytes(24, "little")
    c2, s2 = MX.quant_rows(d)
    assert torch.equal(MX.unpack(c2), torch.where(code == 32, 0, code))
    assert s2.tolist() == [[127, 127, 0, 0, 252, 252, 125, 130]]           # every block holds a value in [4, 8): the scale comes back
    x = torch.zeros(1, 64)
    x[0, :8] = torch.tensor([1 / 16, 3 / 16, 1.9375, 2.125, 3.875, 7.25, 7.75, -7.9])
    assert MX.unpack(MX.quant_rows(x)[0])[0, :8].tolist() == [0, 2, 16, 16, 24, 30, 31, 63] and MX.quant_rows(x)[1].tolist() == [[127, 0]]


def test_flags_and_conflicts(capsys):
    mod = _load_script("sample_video.py")
    with pytest.raises(SystemExit):
        mod.parse_args(["--help"])
    assert "--mxfp6-linears" in capsys.readouterr().out
    assert mod.parse_args([]).mxfp6_linears is False and mod.parse_args(["--mxfp6-linears", "--fp8-attention"]).mxfp6_linears is True
    for other in ("--use-fp8", "--mxfp4-linears"):
        with pytest.raises(SystemExit):
            mod.parse_args(["--mxfp6-linears", other])
    from hunyuanvideo_efficiency_amd.modules import fp8_optimization as F8, mxfp4_optimization as M4, mxfp6_optimization as M6, models
    from hunyuanvideo_efficiency_amd.modules.layers import ParamLinear
    for flag in ("fp8_matmul_enabled", "mxfp4_linears_converted"):
        net = torch.nn.Module()
        setattr(net, flag, True)
        with pytest.raises(ValueError, match="one stored format"):
            M6.convert_mxfp6_linear(net)
    net = torch.nn.Module()
    net.mxfp6_linears_converted = True
    with pytest.raises(ValueError, match="one stored format"):
        F8.convert_fp8_linear(net, None, torch.bfloat16)
    with pytest.raises(ValueError, match="one stored format"):
        M4.convert_mxfp4_linear(net)
    lin = ParamLinear(512, 8, bias=False)
    lin.weight = torch.nn.Parameter(torch.zeros(8, 384, dtype=torch.uint8), requires_grad=False)
    lin.mx_format = 6
    with pytest.raises(RuntimeError, match="--mxfp6-linears"):
        lin.w()
    block = types.SimpleNamespace(mxfp6_linears=True)
    assert models._linear_mode(block, None, lin) == models.MX6
    with pytest.raises(NotImplementedError, match="sequence parallelism"):
        models._linear_mode(block, object(), lin)
    block.mxfp6_linears = False
    assert models._linear_mode(block, object(), lin) is False
