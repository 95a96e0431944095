"""AutoencoderKLCausal3D._mid_attention on device="cpu": the real host function over the fp32 doubles of its five kernels
(tests/cpu_kernel_doubles.py), recorded and checked by tests/mid_attention_bounds.py.  No GPU.

  * the faithful chain passes every check at every shape of the GPU table, in every data class, on both paths, for the decoder at
    C = 512 and C = 128 and for the encoder at C = 128;
  * every mutant - one changed line of a double, or one patched host argument - is rejected, and by the check named next to it;
  * the threshold between the two paths sits where the host says it does;
  * the figures behind the choice of the end-to-end bound's P-term (mid_attention_bounds.P_FORM) are measured here."""
import math

import pytest
import torch

from hunyuanvideo_efficiency_amd import vae_ops
from tests import cpu_kernel_doubles as KD
from tests import mid_attention_bounds as MB

F16 = torch.float16
CONFIGS = [("decoder", 512), ("decoder", 128), ("encoder", 128)]
E2E = {}            # (cls, p_form) -> largest e2e ratio of the faithful chain
RATIOS = {}         # (stage, path) -> largest ratio of the faithful chain


@pytest.fixture(scope="module")
def world():
    """one module per width (the 128-wide one holds both halves); prepared attention entries per (C, class); cases with their oracle"""
    class W:
        vae = {512: MB.make_vae(512, "cpu", False), 128: MB.make_vae(128, "cpu", True)}
        prep, cases = {}, {}

        def P(self, cls, C):
            if (cls, C) not in self.prep:
                self.prep[(cls, C)] = MB.prepared(self.vae[C], cls, C)
            return self.prep[(cls, C)]

        def case(self, cls, thw, C, pre):
            key = (cls, thw, C, pre)
            if key not in self.cases:
                case = MB.Case(cls, *thw, C, pre, MB.block_input(cls, *thw, C, pre), MB.attention_state(cls, C, pre))
                self.cases[key] = (case, MB.oracle_output(case), MB.oracle_tolerance(case))
            return self.cases[key]
    return W()


def pre_of(half):
    return MB.PRE_DEC if half == "decoder" else MB.PRE_ENC


def run(world, monkeypatch, cls, thw, C, half, path, softmax_mutant=None, patches=None, P=None, batch_bytes=None, p_form=MB.P_FORM):
    KD.install_vae_mid_attention(monkeypatch, softmax_mutant)
    pre = pre_of(half)
    case, o_ref, o_tol = world.case(cls, thw, C, pre)
    vae = world.vae[C]
    monkeypatch.setattr(vae, "mid_attention_batch_bytes", (4 << 30 if path == "batched" else 0) if batch_bytes is None else batch_bytes)
    rec = MB.Recorder(vae_ops)
    out = rec.run(vae, world.P(cls, C) if P is None else P, pre, case.x, thw[0], thw[1] * thw[2], host_patches=patches)
    ratios, failures = MB.check_recording(rec, case, out, o_ref, o_tol, p_form)
    return rec, case, out, ratios, failures


# ---------------------------------------------------------------------------------------------------- the faithful chain
DONE = set()


def faithful(world, thw, half, C):
    for cls in MB.CLASSES:
        for path in MB.PATHS:
            with pytest.MonkeyPatch.context() as mp:
                rec, case, out, ratios, failures = run(world, mp, cls, thw, C, half, path)
            assert not failures, (cls, path, failures)
            assert rec.path == path and set(MB.STAGES) <= set(ratios), (cls, path, rec.path, ratios)
            for s, r in ratios.items():
                RATIOS[(s, path)] = max(RATIOS.get((s, path), 0.0), r)
            qkv, a = rec.of("gemm_f16")[0].t["out"], rec.of("gemm_f16")[-1].t["a"]
            for form in ("worst", "stat"):
                a64, b = MB.e2e_ref(qkv, torch.arange(case.L), case.L, C, case.HW, form)
                E2E[(cls, form)] = max(E2E.get((cls, form), 0.0), float(MB._ratio(a, a64, b).max()))
    DONE.add((thw, half, C))


@pytest.mark.parametrize("half,C", CONFIGS)
@pytest.mark.parametrize("thw", MB.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_faithful_chain_passes_every_check(world, thw, half, C):
    faithful(world, thw, half, C)


def test_data_classes_are_what_they_claim(world):
    """on the fp64 chain of (3, 6, 6) at both widths: `random` scores of standard deviation ~2, `peaked` rows owned by their peak key,
    `flat` scores exactly zero, `phantom` scores ~-40"""
    thw = (3, 6, 6)
    for C in (512, 128):
        for cls in MB.CLASSES:
            with pytest.MonkeyPatch.context() as mp:
                rec, case, out, _, failures = run(world, mp, cls, thw, C, "decoder", "batched")
            assert not failures
            qkv = rec.of("gemm_f16")[0].t["out"].double()
            s = qkv[:, :C] @ qkv[:, C:2 * C].T / math.sqrt(C)
            ok = torch.arange(case.L)[None] < MB.valid_of(torch.arange(case.L), case.L, case.HW)[:, None]
            if cls == "random":
                assert 1.5 < float(s[ok].std()) < 2.6, float(s[ok].std())
            elif cls == "flat":
                assert float(s.abs().max()) == 0.0
            elif cls == "phantom":
                assert -48.0 < float(s[ok].mean()) < -34.0 and float(s[ok].max()) < -20.0, (float(s[ok].mean()), float(s[ok].max()))
            else:
                pk = MB.peak_key(3, 36)
                p = torch.softmax(s.masked_fill(~ok, -math.inf), -1)
                own = p[torch.arange(case.L), pk]
                assert float(own.median()) > 0.99 and float((own > 0.9).double().mean()) > 0.9, (float(own.median()), float(own.min()))
                gap = s[torch.arange(case.L), pk] - s.masked_fill(~ok, 0.0).sum(-1) / ok.sum(-1)
                assert 22.0 < float(gap.median()) < 40.0, float(gap.median())


# ---------------------------------------------------------------------------------------------------- mutants
def _softmax_args(**change):
    def make(fn):
        def wrapper(s, cols, cols_pad, scale, out=None, causal_block=0):
            a = dict(cols=cols, cols_pad=cols_pad, scale=scale, causal_block=causal_block)
            a.update({k: v(a) for k, v in change.items()})
            return fn(s, a["cols"], a["cols_pad"], a["scale"], out=out, causal_block=a["causal_block"])
        return wrapper
    return make


def _k_rows_shifted(fn):
    def wrapper(a, w, bias=None, out=None, out_f32=False, res=None, n=None, k=None):
        if out_f32:
            w = w.as_strided((w.shape[0] - 1, w.shape[1]), w.stride(), w.storage_offset() + w.stride(0))
        return fn(a, w, bias, out=out, out_f32=out_f32, res=res, n=n, k=k)
    return wrapper


def _vt_from_k(fn):
    def wrapper(src, dst):
        return fn(src.as_strided(src.shape, src.stride(), src.storage_offset() - src.shape[1]), dst)
    return wrapper


def _vt_pad_left(fn):
    def wrapper(src, dst):
        fn(src, dst)
        dst[:, src.shape[0]:] = 1.0
        return dst
    return wrapper


def _residual_is_n():
    seen = {}

    def apply(fn):
        def wrapper(x, affine, silu, out=None):
            seen["n"] = fn(x, affine, silu, out=out)
            return seen["n"]
        return wrapper

    def gemm(fn):
        def wrapper(a, w, bias=None, out=None, out_f32=False, res=None, n=None, k=None):
            return fn(a, w, bias, out=out, out_f32=out_f32, res=None if res is None else seen["n"], n=n, k=k)
        return wrapper
    return {"groupnorm_apply": apply, "gemm_f16": gemm}


# name: (class, path, softmax mutant of the double, host patches, checks that must fail, checks that must still pass)
MUTANTS = {
    "non-causal": ("random", "batched", None, {"softmax_rows": _softmax_args(causal_block=lambda a: 0)}, {"P.pad", "e2e"}, {"scores"}),
    "causal_block = HW + 1": ("random", "batched", None, {"softmax_rows": _softmax_args(causal_block=lambda a: a["causal_block"] + 1)},
                              {"P.pad", "e2e"}, {"scores"}),
    "frame index off by one": ("random", "batched", "frame_index", None, {"P.finite", "e2e"}, {"scores"}),
    "last valid key dropped": ("random", "batched", "drop_last_key", None, {"P", "e2e"}, {"scores"}),
    # under causal_block the kernel takes min(cols, frame end), so cols = round8(L) changes nothing on the batched path; the per-frame
    # path hands every frame its own cols
    "pad keys visible": ("random", "per-frame", None, {"softmax_rows": _softmax_args(cols=lambda a: MB.r_up(a["cols"], 8))}, {"P.pad", "e2e"},
                         {"scores"}),
    # exp(-46) is a normal fp32, so on the batched path (every column of S written) a maximum taken over the masked columns changes
    # nothing that a bound could see; it shows where the row of S holds cells no kernel wrote: the per-frame path
    "maximum over masked columns": ("phantom", "per-frame", "max_over_masked", None, {"P.finite", "e2e"}, {"scores"}),
    "scale (1 + 2^-6)": ("random", "batched", None, {"softmax_rows": _softmax_args(scale=lambda a: a["scale"] * (1.0 + 2.0 ** -6))},
                         {"P", "e2e"}, {"scores"}),
    "K rows shifted by one": ("random", "batched", None, {"gemm_f16": _k_rows_shifted}, {"e2e"}, {"scores", "P", "pv"}),
    "V^T from the k columns": ("random", "batched", None, {"transpose_16b": _vt_from_k}, {"vT", "e2e"}, {"scores", "P", "pv"}),
    "V^T pad columns non-zero": ("random", "batched", None, {"transpose_16b": _vt_pad_left}, {"vT.pad"}, {"scores", "P", "e2e"}),
    "P padded to round8(nk) only": ("random", "per-frame", None,
                                    {"softmax_rows": _softmax_args(cols_pad=lambda a: MB.r_up(a["cols"], 8))}, {"P.finite", "e2e"}, {"scores"}),
    # `flat` at (5, 3, 5): p = 1 / 15 .. 1 / 75.  (At (3, 5, 7) 1 / 35, 1 / 70 and 1 / 105 happen to have the same bf16 and fp16 values.)
    "P rounded to bf16": ("flat", "batched", "bf16_p", None, {"P", "e2e"}, {"scores"}, (5, 3, 5)),
    "row sum after the fp16 rounding": ("random", "batched", "sum_after_rounding", None, {"P"}, {"scores"}),
    "residual = n": ("random", "batched", None, _residual_is_n, {"out", "oracle"}, {"scores", "P", "pv", "e2e"}),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
@pytest.mark.parametrize("half,C", CONFIGS)
def test_mutant_is_rejected(world, monkeypatch, name, half, C):
    cls, path, sm, patches, must_fail, must_pass = MUTANTS[name][:6]
    thw = MUTANTS[name][6] if len(MUTANTS[name]) > 6 else (3, 5, 7)
    patches = patches() if callable(patches) else patches
    rec, case, out, ratios, failures = run(world, monkeypatch, cls, thw, C, half, path, softmax_mutant=sm, patches=patches)
    assert must_fail <= set(failures), (name, sorted(failures), ratios)
    assert not (must_pass & set(failures)), (name, failures)


def test_qkv_concatenated_as_q_v_k_is_rejected(world, monkeypatch):
    """the end-to-end check reads q, k, v from the same columns the chain does, so it cannot see this one: the weight check and the
    oracle do"""
    C, cls = 128, "random"
    P = dict(world.P(cls, C))
    w, b = P[MB.PRE_DEC + "qkv"]
    order = torch.cat([torch.arange(C), torch.arange(2 * C, 3 * C), torch.arange(C, 2 * C)])
    P[MB.PRE_DEC + "qkv"] = (w[order].contiguous(), b[order].contiguous())
    _, _, _, _, failures = run(world, monkeypatch, cls, (3, 5, 7), C, "decoder", "batched", P=P)
    assert {"glue", "oracle"} <= set(failures) and "e2e" not in failures, failures


def test_threshold_between_the_paths(world):
    """mid_attention_batch_bytes = L round8(L) 4 exactly: batched (one softmax launch, causal); one byte less: T launches"""
    T, H, W = 3, 5, 7
    L = T * H * W
    for nbytes, n_soft, path in ((L * MB.r_up(L, 8) * 4, 1, "batched"), (L * MB.r_up(L, 8) * 4 - 1, T, "per-frame")):
        with pytest.MonkeyPatch.context() as mp:
            rec, _, _, _, failures = run(world, mp, "random", (T, H, W), 128, "decoder", None, batch_bytes=nbytes)
        assert not failures
        assert len(rec.of("softmax_rows")) == n_soft and len(rec.of("gemm_f16")) == 2 + 2 * n_soft and rec.path == path
        assert rec.clones == (0 if path == "batched" else 2 * (T - 1))


def test_zz_p_form_decision(world):
    """The figures behind mid_attention_bounds.P_FORM (run after the faithful chain): the worst-case P-term stays if the faithful
    emulation reaches more than 0.05 of the end-to-end bound in every class."""
    for thw in MB.SHAPES:
        for half, C in CONFIGS:
            if (thw, half, C) not in DONE:
                faithful(world, thw, half, C)
    print("\nlargest e2e error-to-bound ratio of the faithful CPU chain, per class:\n" + "\n".join(
        f"  {cls:<8} worst-case P-term {E2E[(cls, 'worst')]:.3f}   statistical {E2E[(cls, 'stat')]:.3f}" for cls in MB.CLASSES))
    print("largest ratio per stage and path:\n" + "\n".join(f"  {s:<7} {p:<10} {RATIOS[(s, p)]:.3f}" for s, p in sorted(RATIOS)))
    assert MB.P_FORM == "worst"
    for cls in MB.CLASSES:
        assert 0.05 < E2E[(cls, "worst")] <= 1.0, (cls, E2E[(cls, "worst")])
