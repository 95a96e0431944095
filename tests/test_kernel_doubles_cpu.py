"""CPU: the kernel doubles (tests/cpu_kernel_doubles.py, tests/test_ulysses_gloo.py::CpuKernelDouble) held to the surface of the wrappers
they replace, the shared case table of tests/double_parity.py held to cover every double, the exactness of the "exact" class certified,
and the parity harness shown to reject each way a double can drift.  The kernel side of every case is tests/test_gpu_kernel_doubles.py.

  surface      inspect.signature of every double equals its wrapper's: names, order, defaults (EXTRA_HOOKS lists the trailing test hooks)
  coverage     every double has a case in double_parity.CASES; every public wrapper that launches a kernel has a double or a NO_DOUBLE reason
  exactness    every "exact" case evaluated in fp64 with the same rounding points, and with the K / channel order reversed, gives the bits
               of its fp32 evaluation: bit equality is then the right demand on the GPU
  teeth        compare_call with the pristine double as the kernel and a mutated copy as the double: each mutant rejected by the named check
  bounded      every double passes the check function and generator its kernel's GPU edge test uses (compare_call, double against itself)
  refusals     every illegal call of double_parity.REFUSALS raises on the double and writes nothing"""
import contextlib
import inspect

import pytest
import torch

from hunyuanvideo_efficiency_amd import ops, vae_ops
from hunyuanvideo_efficiency_amd.long_ctx_attention import _HipKernels
from tests import attention_bounds as AB
from tests import cpu_kernel_doubles as KD
from tests import double_parity as P
from tests.test_ulysses_gloo import CpuKernelDouble

BF16 = torch.bfloat16
EXTRA_HOOKS = {"vae_ops.softmax_rows": ["mutant"]}          # trailing parameters a double may have on top of its wrapper's
SP_METHODS = sorted(n for n, v in vars(CpuKernelDouble).items() if isinstance(v, staticmethod))


def pairs():
    """(op, wrapper, double) of every double"""
    out = [(f"ops.{n}", getattr(ops, n), getattr(KD, n)) for n in KD.NAMES + ["attn_partial", "attn_merge"]]
    out += [(f"vae_ops.{n}", getattr(vae_ops, n), getattr(KD, d)) for n, d in KD.VAE_TILE_CODER_NAMES.items()]
    out += [(f"vae_ops.{n}", getattr(vae_ops, n), getattr(KD, "vae_" + n)) for n in KD.VAE_MID_ATTENTION_NAMES]
    out += [(f"sp.{n}", getattr(_HipKernels, n), getattr(CpuKernelDouble, n)) for n in SP_METHODS]
    return out


def _params(f):
    return [(p.name, p.kind, p.default) for p in inspect.signature(f).parameters.values()]


@pytest.mark.parametrize("op,wrapper,double", pairs(), ids=[p[0] for p in pairs()])
def test_signature_equals_the_wrappers(op, wrapper, double):
    want, got = _params(wrapper), _params(double)
    extra = got[len(want):]
    assert got[:len(want)] == want, f"{op}: double {got} vs wrapper {want}"
    assert [n for n, _, _ in extra] == EXTRA_HOOKS.get(op, []), f"{op}: unlisted extra parameters {extra}"
    assert all(d is not inspect.Parameter.empty for _, _, d in extra), f"{op}: a test hook without a default"


def test_attn_partials_has_the_attributes_of_ops_attnpartials():
    assert _params(KD.AttnPartials.__init__) == _params(ops.AttnPartials.__init__)
    p = KD.AttnPartials(3, 5, 2, "cpu")
    assert (p.n_slots, p.n_q, p.n_heads, p.used) == (3, 5, 2, 0)
    assert tuple(p.o.shape) == (3, 5, 2, 128) and tuple(p.ml.shape) == (3, 5, 2, 2) and p.o.dtype == p.ml.dtype == torch.float32


# ------------------------------------------------------------------------------------------------------------ coverage
def test_every_double_has_a_case():
    have = {c.op for c in P.CASES}
    want = {op for op, _, _ in pairs()}
    deliberate = {k for k in P.DELIBERATE_DEVIATIONS if ":" not in k}          # a double that is MEANT to answer differently has its own test below
    missing = sorted(want - have - deliberate)
    assert not missing, f"doubles without a case in tests/double_parity.CASES: {missing}"
    assert not sorted(have - want), f"cases of no known double: {sorted(have - want)}"
    assert {c.cls for c in P.CASES} == {"copy", "exact", "bounded"}
    assert len({c.id for c in P.CASES}) == len(P.CASES), "duplicate case ids"


def test_every_launching_wrapper_has_a_double_or_a_reason():
    doubled = {op for op, _, _ in pairs()}
    launching = set()
    for mod, space in ((ops, "ops"), (vae_ops, "vae_ops")):
        for name, f in vars(mod).items():
            if inspect.isfunction(f) and f.__module__ == mod.__name__ and not name.startswith("_") and "_lib.call(" in inspect.getsource(f):
                launching.add(f"{space}.{name}")
    assert launching, "no launching wrapper found: the scan is broken"
    assert not sorted(launching - doubled - set(P.NO_DOUBLE)), f"wrappers with neither a double nor a NO_DOUBLE reason: {sorted(launching - doubled - set(P.NO_DOUBLE))}"
    assert not sorted(set(P.NO_DOUBLE) & doubled), "a NO_DOUBLE entry has a double by now"
    assert not sorted(set(P.NO_DOUBLE) - launching), "a NO_DOUBLE entry names no launching wrapper"
    assert all(len(r) > 20 for r in P.NO_DOUBLE.values())


def test_refusal_table_covers_the_ops_the_host_hands_views_to():
    need = {"ops.gemm", "ops.gemm_fp8", "ops.ln_modulate", "ops.ln_modulate_fp8", "ops.quant_rows_fp8", "ops.qknorm_rope_", "ops.attn_fwd",
            "ops.copy3d", "vae_ops.gemm_f16", "vae_ops.conv3d_causal", "vae_ops.groupnorm_apply", "vae_ops.softmax_rows"}
    assert need <= {r.op for r in P.REFUSALS}
    assert len({r.id for r in P.REFUSALS}) == len(P.REFUSALS)


# ------------------------------------------------------------------------------------------------------------ every case on the double
RATIOS = {}


@pytest.mark.parametrize("case", P.CASES, ids=[c.id for c in P.CASES])
def test_case_holds_on_the_double(case):
    """the harness on (double, double): the case builds, the double returns what it was given, and a bounded case passes the kernel's own
    check on the CPU - the DiT doubles included (ln_modulate, qknorm_rope_, the activation epilogues, linear_smallm, timestep_embedding,
    masked_mean), as tests/test_conv_bounds_cpu.py and tests/test_mid_attention_cpu.py do for the conv and mid-attention doubles"""
    f = P.double_fn(case.op)
    r = max(P.compare_call(f, f, case, "cpu", "cpu", P.double_peer, P.double_peer, real_is_double=True))
    if case.cls == "bounded":
        RATIOS[case.op] = max(RATIOS.get(case.op, 0.0), r)
        assert r <= 1.0


def test_zz_ratio_report(capsys):
    with capsys.disabled():
        for op in sorted(RATIOS):
            print(f"[kernel doubles, cpu] {op}: largest error-to-bound ratio of the double {RATIOS[op]:.3f}")


# ------------------------------------------------------------------------------------------------------------ exactness
@contextlib.contextmanager
def fp64_arithmetic():
    """the doubles' fp32 arithmetic in fp64: Tensor.float() yields fp64 and fresh accumulators are fp64; the roundings to bf16 / fp16 / fp32
    stores stay where they are"""
    orig, dflt = torch.Tensor.float, torch.get_default_dtype()
    torch.Tensor.float = lambda self, *a, **k: self.double()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.Tensor.float = orig
        torch.set_default_dtype(dflt)


OUTPUT_BUFFERS = ("out", "out1", "res", "sample", "part_o", "part_ml", "o32")


def _evaluate(case, flip=False, fp64=False):
    call = case.build("cpu", flip) if case.flippable else case.build("cpu")
    f = P.double_fn(case.op)
    with (fp64_arithmetic() if fp64 else contextlib.nullcontext()):
        ret = f(*call.args, **call.kwargs)
    got = {f"ret{i}": P.bits(t) for i, t in enumerate(P._flatten(ret)) if isinstance(t, torch.Tensor)}
    got.update({k: P.bits(v) for k, v in call.watch.items() if k in OUTPUT_BUFFERS})
    if call.post is not None:
        got.update({"derived." + k: P.bits(v) for k, v in call.post(ret, call, P.double_peer).items()})
    assert got, f"{case.id}: nothing to compare"
    return got


EXACT = P.cases_of("exact")


@pytest.mark.parametrize("case", EXACT, ids=[c.id for c in EXACT])
def test_exact_case_is_exact(case):
    base = _evaluate(case)
    variants = {"fp64": _evaluate(case, fp64=True)}
    if case.flippable:
        variants["K order reversed"] = _evaluate(case, flip=True)
        variants["K order reversed, fp64"] = _evaluate(case, flip=True, fp64=True)
    for nm, v in variants.items():
        assert v.keys() == base.keys()
        for k in base:
            assert torch.equal(base[k], v[k]), f"{case.id}: {k} differs in bits under '{nm}': the case is not exact in fp32 - replace it"


def test_every_reduction_case_is_flippable():
    red = ("gemm", "linear_smallm", "conv")
    assert all(c.flippable for c in EXACT if any(r in c.op for r in red))


# ------------------------------------------------------------------------------------------------------------ the harness has teeth
def _case(cid):
    return next(c for c in P.CASES if c.id == cid)


def m_unpatchify_ignores_out(y, c, t, h, w, out=None):
    return KD.unpatchify(y, c, t, h, w)


def m_attn_ignores_scale(q, k, v, out, n_heads, scale=None, kv_split_workspace=True):
    return KD.attn_fwd(q, k, v, out, n_heads)


def m_gemm_writes_pad_columns(a, w, bias=None, out=None, **kw):
    r = KD.gemm(a, w, bias, out, **kw)
    n = w.shape[0]
    torch.as_strided(out, (out.shape[0], 8), (out.stride(0), 1), out.storage_offset() + n).zero_()
    return r


def m_gemm_one_rounding_for_gate_and_res(a, w, bias=None, out=None, act=0, n_split=0, out1=None, act1=0, gate=None, res=None):
    y = P.E.r(a.float() @ w.float().T + bias.float())
    out.copy_((res.float() + y * gate.float()).to(BF16))
    return out


def m_conv_clamps_at_the_source_extent(*a, **kw):
    def up_rows(m, tap, oH, oW, src, up_t, up_hw):
        _, sH, sW = src
        t, h, w = m // (oH * oW), (m // oW) % oH, m % oW
        ti = (t + tap // 9 - 2).clamp(min=0)
        if up_t:
            ti = torch.where(ti == 0, ti, 1 + (ti - 1) // 2)
        hi = (h + (tap // 3) % 3 - 1).clamp(0, sH - 1) >> int(up_hw)
        wi = (w + tap % 3 - 1).clamp(0, sW - 1) >> int(up_hw)
        return (ti * sH + hi) * sW + wi
    orig, KD._up_rows = KD._up_rows, up_rows
    try:
        return KD.vae_conv3d_causal(*a, **kw)
    finally:
        KD._up_rows = orig


def m_quant_writes_scales_behind_m(x, out_q=None, out_scale=None):
    r = KD.quant_rows_fp8(x, out_q, out_scale)
    out_scale[x.shape[0]:] = 1.0
    return r


def m_copy3d_strides_swapped(src, dst, n_batch, rows, cols, src_bs, src_ld, dst_bs, dst_ld):
    return KD.copy3d(src, dst, n_batch, rows, cols, dst_bs, dst_ld, src_bs, src_ld)


def m_gemm_returns_a_fresh_tensor(*a, **kw):
    return KD.gemm(*a, **kw).clone()


MUTANTS = [      # (case id, mutant, the check that must catch it)
    ("ops.unpatchify:out-given", m_unpatchify_ignores_out, "written-set"),
    (f"ops.attn_fwd:random-321x449-scale={P.ATTN_SCALE}", m_attn_ignores_scale, "bounded"),
    ("ops.gemm:B3-wide-out", m_gemm_writes_pad_columns, "written-set"),
    ("ops.gemm:B3-gate", m_gemm_one_rounding_for_gate_and_res, "values"),
    ("vae_ops.conv3d_causal:up_hw", m_conv_clamps_at_the_source_extent, "values"),
    ("ops.quant_rows_fp8:given-outputs-long-scale", m_quant_writes_scales_behind_m, "written-set"),
    ("ops.copy3d:batched-strided", m_copy3d_strides_swapped, "written-set"),
    ("ops.gemm:B3-bias", m_gemm_returns_a_fresh_tensor, "return-identity"),
]


@pytest.mark.parametrize("cid,mutant,check", MUTANTS, ids=[m[1].__name__[2:] for m in MUTANTS])
def test_mutant_is_rejected_by_the_named_check(cid, mutant, check):
    """the conv mutant clamps at the SOURCE extent before halving: a clamp after the halving is, for the floor shifts of the gather, the
    same function as the clamp before it, so no test could tell that pair apart; the wrong extent is the mistake that order invites"""
    case = _case(cid)
    with pytest.raises(P.ParityError) as e:
        P.compare_call(P.double_fn(case.op), mutant, case, "cpu", "cpu", P.double_peer, P.double_peer, real_is_double=True)
    assert e.value.check == check and f"[{check}]" in str(e.value), str(e.value)


def test_unpatchify_mutant_also_fails_identity_when_the_written_set_is_not_looked_at():
    case = _case("ops.unpatchify:out-given")
    call = case.build("cpu")
    assert m_unpatchify_ignores_out(*call.args, **call.kwargs) is not call.kwargs["out"]
    call = case.build("cpu")
    assert KD.unpatchify(*call.args, **call.kwargs) is call.kwargs["out"]


# ------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("ref", P.REFUSALS, ids=[r.id for r in P.REFUSALS])
def test_double_refuses_what_the_wrapper_refuses(ref):
    P.check_refusal(P.double_fn(ref.op), ref, "cpu")


# ------------------------------------------------------------------------------------------------------------ deliberate deviations
def test_deviation_suggest_splits_is_still_real():
    from hunyuanvideo_efficiency_amd import _lib
    lib = _lib.load()
    assert CpuKernelDouble.attn_suggest_splits(4096, 128, 24) == 2 and CpuKernelDouble.attn_suggest_splits(1, 127, 1) == 1
    assert lib.hv_attn_suggest_splits(4096, 128, 24) == 1, "the kernel's rule now splits a full grid at 128 keys: the deviation is gone - remove it"


def test_deviation_unrounded_q_is_still_real():
    q, k, v = AB.make_case("random", 64, 449, 1, "dev.q")
    out = torch.empty(64, 128, dtype=BF16)
    KD.attn_fwd(q, k, v, out, 1)
    own, kern = AB.AttnRef(q, k, v, 1, rounded_q=False), AB.AttnRef(q, k, v, 1, rounded_q=True)
    assert own.check_o(out, "the double under its own contract") <= 1.0
    assert float((own.O - kern.O).abs().max()) > 0
    e_own, e_kern = (out.double().reshape(own.O.shape) - own.O).abs().mean(), (out.double().reshape(own.O.shape) - kern.O).abs().mean()
    assert float(e_own) < float(e_kern), "the double is no closer to the unrounded-q reference than to the kernel's: the deviation is gone"
    assert set(P.DELIBERATE_DEVIATIONS) == {"sp.attn_suggest_splits", "ops.attn_fwd:unrounded-q", "ops.attn_fwd:narrow-view"}


def test_deviation_narrow_view_is_still_real():
    q, k, v = AB.make_case("random", 3, 5, 2, "dev.narrow")
    out = torch.empty(3, 256, dtype=BF16)
    with pytest.raises(AssertionError, match="narrower"):
        KD.attn_fwd(q[:, :128], k, v, out, 2)
    assert "shape[1]" not in inspect.getsource(ops.attn_fwd), "ops.attn_fwd checks the view's width by now: the deviation is gone - remove it"


def test_every_refusal_names_its_error():
    assert set(P.REFUSAL_ERRORS) == {r.id for r in P.REFUSALS}
    assert set(P.REFUSAL_ERRORS.values()) == {"TypeError", "ValueError", "AssertionError", "HVKernelError"}
