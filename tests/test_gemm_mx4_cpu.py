"""CPU only: include/hv_gemm_mx4.h without a GPU - the bindings and the generated registration source, the documented refusals of its
entry points through the C ABI (made-up pointers: skipped where a GPU is present), the restatement's own edge cases, and the flags."""
import ctypes as C
import importlib.util
import os
import types

import pytest
import torch

from tests import mxfp4_ref as MX
from hunyuanvideo_efficiency_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR, ARG, LAUNCH = 0x7f0000001000, -1, -2
no_gpu = pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present: calls with made-up pointers must not reach a device")


def _load_script(rel):
    spec = importlib.util.spec_from_file_location("hvmx_" + os.path.basename(rel)[:-3], os.path.join(ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _call(name, **ov):
    a = dict(x=PTR, ldx=1024, codes=PTR, ldq=512, scales=PTR, lds=32, M=5, K=1024, D=1024, shift=None, scale=None, eps=1e-6,
             A_codes=PTR, lda=512, A_scales=PTR, ldas=32, W_codes=PTR, ldw=512, W_scales=PTR, ldws=32, bias=None, N=264, out0=PTR, ld0=264,
             act0=0, n_split=0, out1=None, ld1=0, act1=0, gate=None, res=None, ld_res=0, stream=None)
    a.update(ov)
    params = next(p for _, n, p in _abi.GEMM_MX4_DECLS if n == name)
    return getattr(_lib.load(), name)(*[a[p] for _, p in params])


@no_gpu
@pytest.mark.parametrize("ov", [dict(K=384), dict(K=1088), dict(N=260), dict(lda=520), dict(ldw=8), dict(ldas=30), dict(ldws=2),
                                dict(A_scales=None), dict(W_scales=None), dict(A_codes=PTR + 8), dict(W_scales=PTR + 2), dict(ld0=260),
                                dict(ld0=256), dict(n_split=128), dict(gate=PTR), dict(act0=3), dict(M=-1)],
                         ids=["K<512", "K%128", "N%8", "lda%16", "ldw%16", "ldas%4", "ldws%4", "no-A-scales", "no-W-scales", "A-align",
                              "Ws-align", "ld0%8", "pitch", "split-no-out1", "gate-no-res", "act", "M<0"])
def test_gemm_refusals(ov):
    """the accepted call fails at the launch (-2: no device), each refusal before it (-1)"""
    assert _call("hv_gemm_mxfp4") == LAUNCH and _call("hv_gemm_mxfp4", **ov) == ARG
    assert _call("hv_gemm_mxfp4", M=0) == 0 and _call("hv_gemm_mxfp4", K=512) == LAUNCH and _call("hv_gemm_mxfp4", K=15360) == LAUNCH


@no_gpu
@pytest.mark.parametrize("name,kk", [("hv_quant_rows_mxfp4", "K"), ("hv_ln_modulate_mxfp4", "D")])
def test_quantiser_refusals(name, kk):
    assert _call(name) == LAUNCH and _call(name, M=0) == 0
    for ov in ({kk: 1040}, {kk: 0}, dict(ldx=1028), dict(ldq=520), dict(ldq=496), dict(lds=16), dict(scales=None), dict(codes=PTR + 4),
               dict(x=None), dict(M=-1)):
        assert _call(name, **ov) == ARG, ov
    assert _call(name, M=1, ldq=0, lds=0) == LAUNCH                       # a single row has no pitch
    assert _call("hv_ln_modulate_mxfp4", D=4128, ldq=4096, lds=256) == ARG


def test_the_header_is_bound_and_the_generated_source_is_up_to_date():
    p, i, l, f = C.c_void_p, C.c_int, C.c_int64, C.c_float
    want = {"hv_quant_rows_mxfp4": [p, l, p, l, p, l, l, i, p], "hv_ln_modulate_mxfp4": [p, p, p, p, l, p, l, l, i, l, f, p],
            "hv_gemm_mxfp4": [p, l, p, l, p, l, p, l, p, i, i, i, p, l, i, i, p, l, i, p, p, l, p]}
    lib = _lib.load()
    assert set(_lib.GEMM_MX4_SIGNATURES) == set(want)
    for name, args in want.items():
        assert getattr(lib, name).argtypes == args == _lib.GEMM_MX4_SIGNATURES[name] and getattr(lib, name).restype is i
    assert _abi.GEMM_MX4_MACROS == {"HV_MX4_BLOCK": 32, "HV_MX4_BM": 256, "HV_MX4_BN": 256, "HV_MX4_KSTAGE": 128, "HV_MX4_RING": 4,
                                    "HV_MX4_MIN_K": 512}
    g = _load_script("tools/gen_torch_ops.py")
    text = g.gen(_abi.GEMM_MX4_DECLS, "hv_gemm_mx4.h")
    assert open(g.GEMM_MX4_OUT).read() == text, "include/hv_gemm_mx4.h changed: run python tools/gen_torch_ops.py"
    assert "TORCH_LIBRARY_FRAGMENT(hv, m)" in text and text.count("m.def(") == 3
    assert open(g.OUT).read() == g.gen() and {n for _, n, _ in _abi.DECLS}.isdisjoint(want)          # hv_kernels.h is what it was
    assert all(hasattr(_lib.torch_ops(), n[3:]) for n in want)
    mk = open(os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "Makefile")).read()
    assert mk.count("hv_gemm_mx4_torch_ops.cpp") == 2 and mk.count("../../include/hv_gemm_mx4.h") == 2


def test_restatement_edges():
    """the restatement on the header's own examples: ties, saturation, the zero block, a subnormal block; dequant inverts exactly"""
    x = torch.zeros(1, 128)
    x[0, 32:46] = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 5.5, -0.25, -0.75, 6.0, 0.26, 0.74, -7.5])
    x[0, 64:66] = torch.tensor([2.0 ** -133, -127 * 2.0 ** -133])
    x[0, 96] = 3.984375
    c, s = MX.quant_rows(x)
    assert s.tolist() == [[0, 127, 0, 126]]
    code = torch.stack([c[0].int() & 15, c[0].int() >> 4], -1).reshape(-1)
    assert code[32:46].tolist() == [0, 2, 2, 4, 4, 6, 6, 7, 0, 10, 7, 1, 1, 15] and int(code[96]) == 7 and int(code[:32].max()) == 0
    d = MX.dequant(c, s)
    assert d[0, 32:40].tolist() == [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 6.0] and float(d[0, 96]) == 3.0         # 3.984375: E = 128, scale 2^-1, saturates at 6
    assert float(d[0, 65]) == -2.0 * 2.0 ** -127 and float(d[0, 64]) == 0.0          # 127 / 64 rounds to 2, 1 / 64 to 0, at scale 2^-127
    assert torch.equal(MX.quant_rows(d)[0], c)                                       # codes are a fixed point of the quantiser


def test_flags_and_conflicts(capsys):
    mod = _load_script("sample_video.py")
    with pytest.raises(SystemExit):
        mod.parse_args(["--help"])
    assert "--mxfp4-linears" in capsys.readouterr().out
    assert mod.parse_args([]).mxfp4_linears is False and mod.parse_args(["--mxfp4-linears"]).mxfp4_linears is True
    with pytest.raises(SystemExit):
        mod.parse_args(["--mxfp4-linears", "--use-fp8"])
    from hunyuanvideo_efficiency_amd.modules import fp8_optimization as F8, mxfp4_optimization as M4, models
    from hunyuanvideo_efficiency_amd.modules.layers import ParamLinear
    net = torch.nn.Module()
    net.fp8_matmul_enabled = True
    with pytest.raises(ValueError, match="one stored format"):
        M4.convert_mxfp4_linear(net)
    net = torch.nn.Module()
    net.mxfp4_linears_converted = True
    with pytest.raises(ValueError, match="one stored format"):
        F8.convert_fp8_linear(net, None, torch.bfloat16)
    lin = ParamLinear(512, 8, bias=False)
    lin.weight = torch.nn.Parameter(torch.zeros(8, 256, dtype=torch.uint8), requires_grad=False)
    with pytest.raises(RuntimeError, match="--mxfp4-linears"):
        lin.w()
    block = types.SimpleNamespace(mxfp4_linears=True)
    assert models._linear_mode(block, None, lin) == models.MX4
    with pytest.raises(NotImplementedError, match="sequence parallelism"):
        models._linear_mode(block, object(), lin)
    block.mxfp4_linears = False
    assert models._linear_mode(block, object(), lin) is False
