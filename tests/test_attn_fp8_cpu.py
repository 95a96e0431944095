"""CPU only: the contract of include/hv_attn_fp8.h without a GPU - the refusals of its entry points through the C ABI (made-up pointers:
skipped where a GPU is present, a missing guard must never launch on them), the workspace size against the header's layout paragraph,
the bindings, the generated registration source, the Makefile and the command-line flag."""
import ctypes as C
import importlib.util
import os

import pytest

from hunyuanvideo_efficiency_amd import _abi, _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR, ARG, LAUNCH = 0x7f0000001000, -1, -2
no_gpu = pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present: calls with made-up pointers must not reach a device")


def _load_script(rel):
    spec = importlib.util.spec_from_file_location("hvaf_" + os.path.basename(rel)[:-3], os.path.join(ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _call(name, **ov):
    lib = _lib.load()
    a = dict(q=PTR, k=PTR, v=PTR, o=PTR, stride_q=1152, stride_k=1152, stride_v=1152, stride_o=384, n_q=5, n_kv=70, n_heads=3, head_dim=128,
             scale=0.0884, workspace=PTR, workspace_bytes=None, stream=None)
    a.update(ov)
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = lib.hv_attn_fp8_workspace_bytes(5, 70, 3)
    params = next(p for _, n, p in _abi.ATTN_FP8_DECLS if n == name)
    return getattr(lib, name)(*[a[p] for _, p in params])


@no_gpu
@pytest.mark.parametrize("name", ["hv_attn_fp8_quantise", "hv_attn_fwd_fp8"])
@pytest.mark.parametrize("ov", [dict(workspace_bytes=106_000), dict(workspace=None), dict(workspace=PTR + 8), dict(head_dim=64),
                                dict(stride_q=1153, stride_o=386), dict(n_kv=0), dict(n_heads=0), dict(n_q=-1)],
                         ids=["short-workspace", "no-workspace", "workspace-align", "head_dim", "stride", "n_kv-0", "n_heads-0", "n_q<0"])
def test_refusals(name, ov):
    """the accepted call fails at the launch (-2: no device), each refusal before it (-1)"""
    assert _call(name) == LAUNCH and _call(name, **ov) == ARG
    assert _call(name, n_q=0) == 0 and _call(name, n_q=2, stride_o=0) == (ARG if name == "hv_attn_fwd_fp8" else LAUNCH)


def test_workspace_bytes_is_the_documented_layout():
    lib = _lib.load()
    # n_q 5, n_kv 70, 3 heads by hand: nt 2, nb 1; kmean 1536 | sv 1536 | sk 24 -> 256 | sq 60 -> 256 | part 3072 | q8 1920 -> 2048 | k8, v8 49152
    assert lib.hv_attn_fp8_workspace_bytes(5, 70, 3) == 1536 + 1536 + 256 + 256 + 3072 + 2048 + 2 * 49152 == 107008
    for shape in ((5, 70, 3), (1, 1, 1), (257, 1025, 24), (0, 64, 2), (119056, 119056, 24)):
        L = ops.attn_fp8_layout(*shape)
        assert lib.hv_attn_fp8_workspace_bytes(*shape) == L["total"] and all(L[k] % 256 == 0 for k in L if k not in ("nt", "nb")), shape
    for shape in ((-1, 64, 1), (5, 0, 1), (5, -1, 1), (5, 64, 0), (5, 2 ** 31 - 2048, 1)):
        assert lib.hv_attn_fp8_workspace_bytes(*shape) == 0, shape
    assert _abi.ATTN_FP8_MACROS == {"HV_ATTN_FP8_BM": 256, "HV_ATTN_FP8_RING": 3, "HV_ATTN_FP8_KVT": 64, "HV_ATTN_FP8_STAT_KEYS": 1024,
                                    "HV_ATTN_FP8_ALIGN": 256}


def test_the_header_is_bound_and_the_generated_source_is_up_to_date():
    p, i, l, f = C.c_void_p, C.c_int, C.c_int64, C.c_float
    want = {"hv_attn_fp8_workspace_bytes": ([i, i, i], l), "hv_attn_fp8_quantise": ([p, p, p, l, l, l, i, i, i, i, f, p, l, p], i),
            "hv_attn_fwd_fp8": ([p, l, p, l, i, i, i, i, p], i)}
    lib = _lib.load()
    assert set(_lib.ATTN_FP8_SIGNATURES) == set(want)
    for name, (args, ret) in want.items():
        assert getattr(lib, name).argtypes == args == _lib.ATTN_FP8_SIGNATURES[name] and getattr(lib, name).restype is ret
    g = _load_script("tools/gen_torch_ops.py")
    text = g.gen(_abi.ATTN_FP8_DECLS, "hv_attn_fp8.h")
    assert open(g.ATTN_FP8_OUT).read() == text, "include/hv_attn_fp8.h changed: run python tools/gen_torch_ops.py"
    assert "TORCH_LIBRARY_FRAGMENT(hv, m)" in text and text.count("m.def(") == 3
    assert open(g.OUT).read() == g.gen() and {n for _, n, _ in _abi.DECLS}.isdisjoint(want)          # hv_kernels.h is what it was
    hv = _lib.torch_ops()
    assert str(hv.attn_fwd_fp8.default._schema) == ("hv::attn_fwd_fp8(Tensor? workspace, int workspace_bytes, Tensor(a!)? o, int stride_o, "
                                                   "int n_q, int n_kv, int n_heads, int head_dim) -> ()")
    mk = open(os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "Makefile")).read()
    assert "$(wildcard *.hip)" in mk and mk.count("hv_attn_fp8_torch_ops.cpp") == 2 and mk.count("../../include/hv_attn_fp8.h") == 2
    assert os.path.exists(os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "hv_attn_fp8.hip"))


def test_sample_video_lists_the_flag(capsys):
    mod = _load_script("sample_video.py")
    with pytest.raises(SystemExit):
        mod.parse_args(["--help"])
    assert "--fp8-attention" in capsys.readouterr().out
    assert mod.parse_args([]).fp8_attention is False and mod.parse_args(["--fp8-attention"]).fp8_attention is True
