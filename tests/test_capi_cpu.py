"""CPU: the C-ABI library loads and exports exactly the symbols include/hv_kernels.h declares; the ctypes table derived from the
header equals hand-written pins and the recorded ABI of this version; the constants and the workspace sizing the Python side
shares with the kernels agree with the built library.  No compute calls (no GPU here)."""
import ctypes as C
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_decls():
    from hunyuanvideo_efficiency_amd import _abi
    return {name: len(params) for _, name, params in _abi.DECLS}


def test_header_matches_ctypes_table():
    """The table _lib derives from the header against signatures typed in here by hand from the C declarations: every C type class
    (device pointers, host arrays, int, int64_t, float, hipStream_t) and both return types, so the parser cannot merely agree with
    itself."""
    from hunyuanvideo_efficiency_amd import _lib
    p, i, l, f = C.c_void_p, C.c_int, C.c_int64, C.c_float
    pins = {
        "hv_gemm_bf16": ([p, l, p, l, p, i, i, i, p, l, i, i, p, l, i, p, p, l, p], i),
        "hv_vae_blend_f16": ([p, p, p, p, p, i, i, p], i),
        "hv_temporal_spectrum": ([p, l, l, l, i, i, i, i, i, i, i, i, i, i, i, i, p, l, p, p, p, l, p], i),
        "hv_attn_workspace_bytes": ([i, i, i], l),
        "hv_abi_version": ([], i),
    }
    for name, (argtypes, restype) in pins.items():
        assert _lib.SIGNATURES[name] == argtypes, name
        assert _lib.RESTYPES[name] is restype, name
    decls = _header_decls()
    assert set(decls) == set(_lib.SIGNATURES) == set(_lib.RESTYPES), (set(decls) ^ set(_lib.SIGNATURES))
    for name, n in decls.items():
        assert len(_lib.SIGNATURES[name]) == n, name
    lib = _lib.load()
    for name in decls:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name] and fn.restype is _lib.RESTYPES[name], name


def test_header_equals_recorded_abi():
    """tests/golden/abi_v<N>.json (written by `python tools/gen_torch_ops.py --record-abi`) holds name, return type and parameter C
    types of every declaration as of ABI version N: the header's rule "bumped on any signature change" as a test."""
    from hunyuanvideo_efficiency_amd import _abi, _lib
    path = os.path.join(ROOT, "tests", "golden", f"abi_v{_lib.ABI_VERSION}.json")
    hint = (f"include/hv_kernels.h no longer declares what {os.path.relpath(path, ROOT)} recorded for HV_ABI_VERSION {_lib.ABI_VERSION}: "
            "bump HV_ABI_VERSION (add the change to the list next to it) and record a new file with python tools/gen_torch_ops.py --record-abi")
    assert os.path.exists(path), hint
    with open(path) as fh:
        rec = json.load(fh)
    assert rec["abi_version"] == _lib.ABI_VERSION, hint
    now = [{"name": name, "returns": ret, "params": [t for t, _ in params]} for ret, name, params in _abi.DECLS]
    assert rec["declarations"] == now, hint


def test_constants_agree_with_built_library():
    import torch  # noqa: F401
    from hunyuanvideo_efficiency_amd import _abi, _lib, metrics, ops, vae_ops
    M = _abi.MACROS
    lib = _lib.load()
    assert lib.hv_abi_version() == M["HV_ABI_VERSION"] == _lib.ABI_VERSION
    assert ops.ATTN_MIN_WORKSPACE == M["HV_ATTN_MIN_WORKSPACE_BYTES"] == 256 == lib.hv_attn_workspace_bytes(0, 4096, 1)
    assert vae_ops.GN_FOLD_WS_FLOATS == M["HV_GN_FOLD_WS_FLOATS"] == 16384
    max_t, bk, bins = M["HV_SPECTRUM_MAX_T"], M["HV_SPECTRUM_BK"], M["HV_SPECTRUM_BINS"]
    assert (metrics.SPECTRUM_MAX_T, metrics.SPECTRUM_BK, metrics.SPECTRUM_BINS) == (max_t, bk, bins) == (1024, 32, 32)
    # the kernel's own limit on T is the header's: the workspace query returns 0 for a shape it refuses
    assert lib.hv_temporal_spectrum_workspace_bytes(1, 4, max_t, 8, 8) > 0
    assert lib.hv_temporal_spectrum_workspace_bytes(1, 4, max_t + 1, 8, 8) == 0
    with pytest.raises(_lib.HVKernelError):
        metrics.spectrum_twiddles(max_t + 1)
    # layout of the twiddle table the caller builds: k-chunks of BK frames, per column tile a cos and a sin block of BINS bins
    for T in (1, 33, 1024):
        ncol = max(1, -(-(T // 2) // bins))
        assert tuple(metrics.spectrum_twiddles(T).shape) == (-(-T // bk) * bk, 2 * bins * ncol), T


def test_attention_workspace_sizing_follows_the_kernels_split_rule():
    """ops._attn_workspace_bytes: nothing below HV_ATTN_BOUND_MIN_KV keys, the full split workspace exactly where the kernel's rule
    (hv_attn_suggest_splits) splits, the 256-byte key-norm bound elsewhere."""
    from hunyuanvideo_efficiency_amd import _abi, _lib, ops
    assert _abi.MACROS["HV_ATTN_BOUND_MIN_KV"] == 4096
    assert _lib.host("attn_suggest_splits", 118811, 118811, 3) == 2 and _lib.host("attn_suggest_splits", 118811, 118811, 24) == 1
    kinds = set()
    for n_q in (1, 255, 256, 257, 4133, 65537, 118811):
        for heads in (1, 2, 3, 6, 24, 62):
            for n_kv in (4095, 4096, 12345, 118811):
                got = ops._attn_workspace_bytes(n_q, n_kv, heads)
                if n_kv < 4096:
                    want = 0
                elif ops.attn_suggest_splits(n_q, n_kv, heads) == 2:
                    want = 256 + 2 * n_q * heads * 130 * 4
                    assert want == _lib.host("attn_workspace_bytes", n_q, n_kv, heads)
                else:
                    want = 256
                assert got == want, (n_q, n_kv, heads, got, want)
                kinds.add(min(want, 257))
    assert kinds == {0, 256, 257}            # the grid reaches all three answers


def test_library_loads_and_exports_every_symbol():
    from hunyuanvideo_efficiency_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} not built: run __graft_entry__.build()")
    lib = _lib.load()
    for name in _header_decls():
        assert hasattr(lib, name), name
    assert lib.hv_abi_version() == _lib.ABI_VERSION


def test_ops_refuse_cpu_tensors():
    import torch
    from hunyuanvideo_efficiency_amd import ops, _lib
    with pytest.raises(_lib.HVKernelError):
        ops.ln_modulate(torch.zeros(4, 256, dtype=torch.bfloat16))
    with pytest.raises(_lib.HVKernelError):
        ops.gemm(torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(8, 64, dtype=torch.bfloat16))


def test_torch_custom_ops_registered_for_every_entry_point():
    """SURVEY.md 8b last row: every C-ABI entry point is a PyTorch custom op torch.ops.hv.<name> (TORCH_LIBRARY(hv, m)); the
    kernels are registered for the CUDA(=HIP) dispatch key only - a CPU tensor is refused by the dispatcher (no CPU path)."""
    import torch
    from hunyuanvideo_efficiency_amd import _lib
    hv = _lib.torch_ops()
    for name in _header_decls():
        op = getattr(hv, name[len("hv_"):])
        assert op.default._schema.name == "hv::" + name[len("hv_"):]
    assert int(hv.abi_version()) == _lib.ABI_VERSION
    assert _lib.host("attn_suggest_splits", 118811, 118811, 3) == 2        # Ulysses-8 shape: shallow grid -> KV split
    assert _lib.host("attn_suggest_splits", 118811, 118811, 24) == 1
    # rows of the GroupNorm-statistics buffer a conv epilogue fills: one per 64 output rows, whole 256-row tiles; the sub-pixel
    # upsampler forms its tiles per output parity class (8 classes when T is upsampled: 4 with sT frames, 4 with sT - 1)
    assert _lib.host("gn_partial_rows", 65 * 256 * 256) == 66560 and _lib.host("gn_partial_rows", 90) == 4
    assert _lib.host("subpixel_gn_partial_rows", 17, 64, 64, 1) == 4 * (4 * 272 + 4 * 256)
    assert _lib.host("subpixel_gn_partial_rows", 1, 4, 4, 1) == 4 * 4 and _lib.host("subpixel_gn_partial_rows", 65, 128, 128, 0) == 4 * 4 * 4160
    with pytest.raises(_lib.HVKernelError):
        _lib.call("euler_step_f32", torch.zeros(4), torch.zeros(4, dtype=torch.bfloat16), 0.1, 4)


def test_generated_torch_ops_source_is_up_to_date():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_torch_ops", os.path.join(ROOT, "tools", "gen_torch_ops.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    assert open(g.OUT).read() == g.gen(), "include/hv_kernels.h changed: run python tools/gen_torch_ops.py"


def test_generated_attention_iteration_ignores_env_and_is_up_to_date_and_consistent(monkeypatch):
    """hv_attention_w4_loop.inc (the steady-state attention iteration as one asm statement) == what tools/gen_attn_w4_asm.py emits
    whatever the environment holds, and the schedule tables it is built from are self-consistent: every exponential is issued exactly
    once, every packed P word is written before the P.V MFMA that reads it (with at least one gap in between: VALU write -> MFMA
    operand wait states), every fragment read precedes its first MFMA by PF fragments and the counted lgkmcnt of that MFMA equals the
    LDS instructions issued in between."""
    import importlib.util
    import re
    # the generator emits the shipped schedule only: switches of retired timing experiments in the environment change nothing
    monkeypatch.setenv("HV_W4_ABL", "v")
    monkeypatch.setenv("HV_W4_STAMPS", "1")
    monkeypatch.setenv("HV_W4_ORDER", "emrdpa")
    spec = importlib.util.spec_from_file_location("gen_attn_w4_asm", os.path.join(ROOT, "tools", "gen_attn_w4_asm.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    assert open(g.OUT).read() == g.main(), "run python tools/gen_attn_w4_asm.py"
    # ... and the built library was compiled from exactly this file (not from a stale one, not from a timing experiment's)
    import ctypes
    from hunyuanvideo_efficiency_amd import _lib
    assert os.path.samefile(g.OUT, _lib.LOOP_INC)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert (lib.hv_attn_w4_loop_signature() & 0xFFFFFFFF) == _lib.loop_signature_in_tree(), "libhv_kernels.so is not built from the in-tree iteration: make -C hunyuanvideo_efficiency_amd/csrc"
    body = g.gen_iter(0)
    gaps, cur = [], None
    for ln in body:
        if ln.startswith("; ---- gap"):
            cur = []
            gaps.append(cur)
        else:
            cur.append(ln)
    assert len(gaps) == 64 and all(sum("v_mfma" in x for x in gp) == 1 for gp in gaps)
    exps = [ln for gp in gaps for ln in gp if ln.startswith("v_exp_f32")]
    assert len(exps) == 64 and len({ln.split(",")[1].strip() for ln in exps}) == 64            # every S'(t) register exactly once
    assert sum(ln.startswith("v_add_f32") for gp in gaps for ln in gp) == 64
    assert sum(ln.startswith("v_cvt_pk") for gp in gaps for ln in gp) == 32
    assert sum(ln.startswith("buffer_load") for gp in gaps for ln in gp) == 8
    # packed P words: written (v_cvt_pk dest) in a gap strictly before the MFMA that reads their tuple
    written = {}
    for gi, gp in enumerate(gaps):
        for ln in gp:
            if ln.startswith("v_cvt_pk"):
                written[int(re.match(r"v_cvt_pk_bf16_f32 v(\d+),", ln).group(1))] = gi
    for gi, gp in enumerate(gaps[32:], start=32):
        m = re.search(r"v_mfma_f32_32x32x16_bf16 a\[\d+:\d+\], a\[\d+:\d+\], v\[(\d+):(\d+)\]", [x for x in gp if "v_mfma" in x][0])
        lo, hi = int(m.group(1)), int(m.group(2))
        assert all(written[r] < gi for r in range(lo, hi + 1)), (gi, lo, hi)
    # fragment reads / counted waits: replay the LDS queue
    issued = []          # (fragment slot register, gap) in issue order
    for gi, gp in enumerate(gaps):
        for ln in gp:
            if ln.startswith("ds_read"):
                issued.append((int(re.search(r"a\[(\d+):", ln).group(1)), gi))
    assert len(issued) == 16 + 32
    # steady state: the stream of the previous iteration precedes this one; a wait lgkmcnt(N) at gap g leaves the N youngest of the reads
    # issued before it outstanding - the fragment registers of this gap's MFMA (and of the next fragment) must not be among them
    prev = [(r, gi - 64) for r, gi in issued]
    for gi, gp in enumerate(gaps):
        w = [x for x in gp if x.startswith("s_waitcnt lgkmcnt")]
        if not w:
            continue
        n = int(re.search(r"lgkmcnt\((\d+)\)", w[0]).group(1))
        before = [x for x in prev + issued if x[1] < gi]
        pending = {r for r, _ in before[len(before) - n:]} if n else set()
        mf = [x for x in gp if "v_mfma" in x][0]
        frag = int(re.findall(r"a\[(\d+):\d+\]", mf)[1 if gi >= 32 else 0])
        assert frag >= 192 and frag not in pending and not any(r in (frag, frag + 2) for r in pending), (gi, n, frag, pending)
        # one wait per PAIR of fragments: the MFMAs two gaps later (next fragment) issue without a wait of their own
        if gi + 2 < 64:
            mf2 = [x for x in gaps[gi + 2] if "v_mfma" in x][0]
            assert not [x for x in gaps[gi + 2] if x.startswith("s_waitcnt lgkmcnt")]
            frag2 = int(re.findall(r"a\[(\d+):\d+\]", mf2)[1 if gi + 2 >= 32 else 0])
            assert not any(r in (frag2, frag2 + 2) for r in pending), (gi, n, frag2, pending)


def test_attention_kernel_generated_code_audit(tmp_path):
    """hv_attention_w4.hip owns the accumulator half of the register file by literal names, so what hipcc does around the asm matters:
    compile it for gfx950 with -save-temps and require (cdna_hip_programming.md 5.7 item 4) no VGPR spills, no scratch, all 256
    accumulator registers allocated, and not one compiler-generated v_accvgpr_* outside ASMSTART/ASMEND (hipcc parks long-lived
    values in the accumulator half when it is short of registers - that would be a silent write into O)."""
    import re
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        import pytest
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "hv_attention_w4.hip")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wno-unused-result", "-save-temps=obj", "-c", src,
                    "-o", str(tmp_path / "w4.o")], check=True, cwd=str(tmp_path), capture_output=True)
    asm = open(tmp_path / "hv_attention_w4-hip-amdgcn-amd-amdhsa-gfx950.s").read()
    meta = {k: int(v) for k, v in re.findall(r"\.(vgpr_spill_count|private_segment_fixed_size|agpr_count|sgpr_spill_count):\s+(\d+)", asm)}
    assert meta["vgpr_spill_count"] == 0 and meta["private_segment_fixed_size"] == 0 and meta["agpr_count"] == 256, meta
    inside, bad = False, []
    for i, ln in enumerate(asm.split("\n")):
        if "#ASMSTART" in ln:
            inside = True
        elif "#ASMEND" in ln:
            inside = False
        elif not inside and "v_accvgpr" in ln:
            bad.append((i, ln.strip()))
    assert not bad, bad[:5]
    assert "scratch_" not in asm
