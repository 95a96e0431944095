"""CPU only: include/hv_mx_rot.h without a GPU - the documented refusals of its entry points through the C ABI (made-up pointers: skipped
where a GPU is present), the bindings and the generated registration source, the restatement's own algebra, and the flags."""
import ctypes as C
import os

import pytest
import torch

from tests import mx_rot_ref as RR
from tests.test_gemm_mx4_cpu import ARG, LAUNCH, PTR, ROOT, _load_script, no_gpu
from hunyuanvideo_efficiency_amd import _abi, _lib


def _call(name, **ov):
    a = dict(x=PTR, ldx=1024, codes=PTR, ldq=512, scales=PTR, lds=32, M=5, K=1024, D=1024, shift=None, scale=None, eps=1e-6, rot=64,
             stream=None)
    a.update(ov)
    params = next(p for _, n, p in _abi.MX_ROT_DECLS if n == name)
    return getattr(_lib.load(), name)(*[a[p] for _, p in params])


@no_gpu
@pytest.mark.parametrize("name,kk", [("hv_quant_rows_mxfp4_rot", "K"), ("hv_ln_modulate_mxfp4_rot", "D")])
def test_refusals(name, kk):
    """the accepted call fails at the launch (-2: no device), each refusal before it (-1)"""
    assert all(_call(name, rot=r) == LAUNCH for r in (16, 64, 256)) and _call(name, M=0) == 0
    odd = {kk: 1088, "ldx": 1088, "ldq": 544, "lds": 34}                  # 17 groups of 64: whole blocks, whole groups only for 16 and 64
    assert _call(name, **odd) == LAUNCH and _call(name, **odd, rot=16) == LAUNCH and _call(name, **odd, rot=256) == ARG
    for ov in (dict(rot=0), dict(rot=32), dict(rot=128), dict(rot=1024), dict(rot=-64), {kk: 0}, dict(ldx=1028), dict(ldq=520),
               dict(ldq=496), dict(lds=16), dict(scales=None), dict(codes=PTR + 4), dict(x=None), dict(M=-1)):
        assert _call(name, **ov) == ARG, ov
    assert _call(name, M=1, ldq=0, lds=0) == LAUNCH                       # a single row has no pitch
    assert _call("hv_ln_modulate_mxfp4_rot", D=4352, ldq=4096, lds=256, rot=256) == ARG


def test_the_header_is_bound_and_the_generated_source_is_up_to_date():
    p, i, l, f = C.c_void_p, C.c_int, C.c_int64, C.c_float
    want = {"hv_quant_rows_mxfp4_rot": [p, l, p, l, p, l, l, i, i, p], "hv_ln_modulate_mxfp4_rot": [p, p, p, p, l, p, l, l, i, l, f, i, p]}
    lib = _lib.load()
    assert set(_lib.MX_ROT_SIGNATURES) == set(want) and _abi.MX_ROT_MACROS == {"HV_MX_ROT_MIN": 16, "HV_MX_ROT_MAX": 256}
    for name, args in want.items():
        assert getattr(lib, name).argtypes == args == _lib.MX_ROT_SIGNATURES[name] and getattr(lib, name).restype is i
    g = _load_script("tools/gen_torch_ops.py")
    text = g.gen(_abi.MX_ROT_DECLS, "hv_mx_rot.h")
    assert open(g.MX_ROT_OUT).read() == text, "include/hv_mx_rot.h changed: run python tools/gen_torch_ops.py"
    assert "TORCH_LIBRARY_FRAGMENT(hv, m)" in text and text.count("m.def(") == 2
    assert all(hasattr(_lib.torch_ops(), n[3:]) for n in want)
    mk = open(os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "Makefile")).read()
    assert mk.count("hv_mx_rot_torch_ops.cpp") == 2 and mk.count("../../include/hv_mx_rot.h") == 2 and "hv_mx4_quant.hpp" in mk


@pytest.mark.parametrize("rot", [16, 64, 256])
def test_restatement_is_an_involution_and_sylvester(rot):
    """H is symmetric and orthonormal: applied twice it returns the input - exactly, on integers small enough that every partial sum
    fits 24 bits; and its entries carry the sign (-1)^popcount(i & j)"""
    x = torch.randint(-127, 128, (3, 2 * rot), generator=torch.Generator().manual_seed(rot)).to(torch.bfloat16)
    assert torch.equal(RR.wht(RR.wht(x, rot), rot), x.float())
    h = RR.wht(torch.eye(rot), rot) * 2.0 ** ((rot.bit_length() - 1) // 2)
    assert all(h[i, j] == (-1) ** bin(i & j).count("1") for i in (0, 1, 5, rot - 1) for j in range(rot))


def test_flags_and_conversion_refusals():
    mod = _load_script("sample_video.py")
    assert mod.parse_args([]).mxfp4_rotate == 0 and mod.parse_args(["--mxfp4-linears", "--mxfp4-rotate", "64"]).mxfp4_rotate == 64
    for argv in (["--mxfp4-rotate", "64"], ["--mxfp4-linears", "--mxfp4-rotate", "32"], ["--mxfp6-linears", "--mxfp4-rotate", "16"]):
        with pytest.raises(SystemExit):
            mod.parse_args(argv)
    from hunyuanvideo_efficiency_amd.modules import mxfp4_optimization as M4, models
    from hunyuanvideo_efficiency_amd.modules.layers import ParamLinear
    block = torch.nn.Module()                                   # what mxfp4_optimization._blocks takes for a single block
    block.hybrid_seq_parallel_attn, block.run = None, None
    block.linear1, block.linear2 = ParamLinear(512, 8, bias=False), ParamLinear(544, 8, bias=False)
    with pytest.raises(ValueError, match="rot must be"):
        M4.convert_mxfp4_linear(block, rot=32)
    with pytest.raises(ValueError, match="does not divide in_features = 544"):
        M4.convert_mxfp4_linear(block, rot=64)
    assert block.linear1.weight.dtype != torch.uint8            # refused before the first layer was packed
    block.linear1.mx_rot, block.linear2.mx_rot = 64, 16
    assert models._mx_rot(block.linear1) == 64 and models._mx_rot(ParamLinear(8, 8)) == 0
    with pytest.raises(ValueError, match="different rotations"):
        models._mx_rot(block.linear1, block.linear2)
