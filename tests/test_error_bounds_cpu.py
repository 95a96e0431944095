"""CPU: the fp64 error bound of tests/error_bounds.py has teeth.  GEMM "mutants" - the ways a main loop can be subtly wrong - are
built on the CPU from bf16/fp16 operands and checked against the bound, and against the criterion the bf16 GEMM tests used so far
(assert_close to an oracle that rounds at the same points, rtol = 2^-7, atol = 2e-2):

  * fp32 accumulation in a shuffled k order                        -> within the bound (any order is a correct loop);
  * the running sum rounded to the output format once per K-tile   -> outside it, at every K the GPU tests use;
  * one K-tile dropped; one 16-row fragment of one K-tile read one row off -> outside it.

test_old_criterion_misses_what_the_bound_catches records which mutants the old criterion accepts while the bound rejects them."""
import math

import pytest
import torch

from hunyuanvideo_efficiency_amd import synthetic as syn
from tests import error_bounds as EB

BK = 64
KS = [64, 128, 192, 256, 320, 384, 448, 1024, 1728, 3072]     # K of the GPU GEMM / conv tests (1728 = 27 x 64: the conv)


def _operands(M, N, K, dtype, key, y_scale=1.0):
    """the data of the GPU tests: a ~ U(+-sqrt 3), w ~ U(+-sqrt(3/K)) * y_scale, b ~ U(+-0.1 sqrt 3)"""
    u = lambda shape, k, s: syn.hashed_uniform(shape, f"{key}.{k}", 5) * (s * math.sqrt(3.0))
    return (u((M, K), "a", 1.0).to(dtype), u((N, K), "w", y_scale / math.sqrt(K)).to(dtype), u((N,), "b", 0.1 * y_scale).to(dtype))


def _tiles(a, w):
    """exact per-K-tile sums (fp64) -> the fp32 value an MFMA chain over one tile produces (to within its own rounding)"""
    K = a.shape[1]
    a64, w64 = a.double(), w.double()
    return [(a64[:, k:k + BK] @ w64[:, k:k + BK].T).float() for k in range(0, K, BK)]


def _store(acc32, b, dtype):
    return (acc32 + b.float()).to(dtype)


def mutant_fp32_shuffled(a, w, b, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    af, wf = a.float(), w.float()
    for k in torch.randperm(a.shape[1], generator=g).tolist():
        acc += af[:, k:k + 1] * wf[:, k][None]          # bf16 / fp16 products are exact in fp32; one rounding per add
    return _store(acc, b, dtype)


def mutant_round_per_tile(a, w, b, dtype):
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    for t in _tiles(a, w):
        acc = (acc + t).to(dtype).float()                # running sum kept in the output format between K-tiles
    return _store(acc, b, dtype)


def mutant_drop_tile(a, w, b, dtype):
    ts = _tiles(a, w)
    ts.pop(len(ts) // 2)
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    for t in ts:
        acc += t
    return _store(acc, b, dtype)


def mutant_fragment_shift(a, w, b, dtype):
    """K-tile kt = last: A rows [16, 32) (one MFMA fragment) staged from rows [17, 33)"""
    ts = _tiles(a, w)
    k0 = (len(ts) - 1) * BK
    a2 = a.clone()
    a2[16:32, k0:] = a[17:33, k0:]
    ts[-1] = _tiles(a2[:, k0:], w[:, k0:])[0]
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    for t in ts:
        acc += t
    return _store(acc, b, dtype)


def old_criterion(got, a, w, b, dtype):
    """tests/test_gpu_ops.py::test_gemm_bias_and_act: assert_close(got, oracle, rtol=2**-7, atol=2e-2), the oracle rounding once"""
    ref = (a.float() @ w.float().T + b.float()).to(dtype).float()
    return bool(((got.float() - ref).abs() <= 2e-2 + 2 ** -7 * ref.abs()).all())


def new_bound(got, a, w, b, dtype, worst_case=False):
    return float(EB.ratio(got, EB.gemm_ref(a, w, b), dtype, worst_case).max())


DTYPES = [torch.bfloat16, torch.float16]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("K", [64, 192, 448, 3072])
def test_fp32_any_order_passes(K, dtype):
    a, w, b = _operands(64, 72, K, dtype, f"ok{K}")
    for seed in (0, 1):
        r = new_bound(mutant_fp32_shuffled(a, w, b, dtype, seed), a, w, b, dtype)
        assert r <= 1.0, r
    # the exact fp32 sum of the tiles (what a tile-ordered MFMA chain gives) too
    acc = torch.zeros(64, 72)
    for t in _tiles(a, w):
        acc += t
    assert new_bound(_store(acc, b, dtype), a, w, b, dtype) <= 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("K", KS)
def test_round_per_ktile_fails(K, dtype):
    a, w, b = _operands(256, 256, K, dtype, f"rt{K}")
    r = new_bound(mutant_round_per_tile(a, w, b, dtype), a, w, b, dtype)
    assert r > 1.0, f"K={K}: the running sum rounded per K-tile stays within the bound (ratio {r:.3g})"


@pytest.mark.parametrize("K", [384, 512, 640, 3072])
def test_worst_case_form_still_rejects(K):
    """the worst-case form (the fp8 path's, bf16 outputs, K of the fp8 tests) keeps its teeth"""
    a, w, b = _operands(256, 256, K, torch.bfloat16, f"wc{K}")
    for mut in (mutant_round_per_tile, mutant_drop_tile, mutant_fragment_shift):
        assert new_bound(mut(a, w, b, torch.bfloat16), a, w, b, torch.bfloat16, True) > 1.0, mut.__name__
    assert new_bound(mutant_fp32_shuffled(a, w, b, torch.bfloat16), a, w, b, torch.bfloat16, True) <= 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("K", [128, 448, 3072])
@pytest.mark.parametrize("mutant", [mutant_drop_tile, mutant_fragment_shift], ids=["drop_tile", "fragment_shift"])
def test_structural_mutants_fail(mutant, K, dtype):
    a, w, b = _operands(64, 72, K, dtype, f"st{K}")
    r = new_bound(mutant(a, w, b, dtype), a, w, b, dtype)
    assert r > 1.0, f"{mutant.__name__} K={K}: ratio {r:.3g}"


def test_fp32_output_bound_not_loose():
    """fp32 outputs (hv_gemm_f16 out_f32): no ulp term to hide behind - a correct order still uses a visible share of the bound"""
    a, w, _ = _operands(64, 72, 512, torch.float16, "f32")
    acc = torch.zeros(64, 72)
    for k in torch.randperm(512, generator=torch.Generator().manual_seed(3)).tolist():
        acc += a[:, k:k + 1].float() * w[:, k][None].float()
    r = float(EB.ratio(acc, EB.gemm_ref(a, w), torch.float32).max())
    assert 0.05 < r <= 1.0, r
    # one rounding of the running sum to fp16 per K-tile is far outside it
    acc = torch.zeros(64, 72)
    for t in _tiles(a, w):
        acc = (acc + t).half().float()
    assert float(EB.ratio(acc, EB.gemm_ref(a, w), torch.float32).max()) > 1.0


def test_old_criterion_misses_what_the_bound_catches(capsys):
    """gap 1 of the suite as a recorded fact: at the old tests' shapes and scales, which wrong main loops the old criterion accepts"""
    rows, missed = [], []
    for dtype in DTYPES:
        for K, y_scale in ((3072, 1.0), (3072, 0.1), (1728, 0.1), (448, 1.0)):
            a, w, b = _operands(256, 256, K, dtype, f"gap{K}", y_scale)
            for mut in (mutant_fp32_shuffled, mutant_round_per_tile, mutant_drop_tile, mutant_fragment_shift):
                got = mut(a, w, b, dtype)
                old, r = old_criterion(got, a, w, b, dtype), new_bound(got, a, w, b, dtype)
                name = f"{mut.__name__[7:]:<16} {str(dtype)[6:]:<8} K={K:<5} |y|~{y_scale}"
                rows.append(f"  {name}  old criterion: {'accepts' if old else 'rejects'}   new bound: ratio {r:8.3g} "
                            f"{'accepts' if r <= 1 else 'REJECTS'}")
                if mut is mutant_fp32_shuffled:
                    assert old and r <= 1.0, name
                elif old and r > 1.0:
                    missed.append(name)
    with capsys.disabled():
        print("\nmutant                                           old criterion vs fp64 bound\n" + "\n".join(rows))
        print("accepted by the old criterion, rejected by the bound:\n  " + "\n  ".join(missed))
    assert any(m.startswith("round_per_tile") for m in missed), missed
