"""CPU: the host half of the temporal spectra (metrics.temporal_spectrum / spectrum_report; csrc/hv_spectrum.hip) - band shares,
mirroring and cutoffs on hand-made spectra, refusals, the twiddle table against float64 - and the error bound of tests/spectrum_ref.py
against an fp32 double of the kernel (tests/spectrum_double.py): the double passes it per series, the mutants a wrong kernel or wrong host
rules would be do not.  No GPU.

Largest per-series error-to-bound ratio of the double (bins k >= 1, |X| and |X|^2 alike; noise, near-static 128 +- 1, ramp; gray and
raw data; the kernel's frame order / reversed / rotated by T / 2), as test_double_passes_the_bound_per_series_in_three_orders prints it:

    T       3      33     129    600    1024
    frames  0.20   0.18   0.18   0.17   0.19
    other   0.18   0.22   0.27   0.23   0.23

Under the bound's first form, ||d||_2 alone, the same double gave 0.22 / 0.31 / 0.42 / 0.74 / 0.65 in frame order and up to 1.10 (a
chain started in the middle of a ramp, T = 600) in the others: the largest-partial-sum term P_k of tests/spectrum_ref.py is what that
form missed.  Raw-mode bin 0: <= 0.73 (the ramp at T = 129)."""
import numpy as np
import pytest
import torch

from hunyuanvideo_efficiency_amd import _lib, metrics
from tests import spectrum_double as dbl
from tests import spectrum_ref as ref

ORDERS = ("frames", "reversed", "rotated")


# ---- host rules -----------------------------------------------------------------------------------------------------------------------
def test_mirror_odd_and_even_counts_the_nyquist_bin_once():
    assert metrics.mirror_spectrum([5.0, 1.0, 2.0], 4).tolist() == [5.0, 1.0, 2.0, 1.0]            # even T: bin 2 is the Nyquist bin
    assert metrics.mirror_spectrum([5.0, 1.0, 2.0], 5).tolist() == [5.0, 1.0, 2.0, 2.0, 1.0]
    assert metrics.mirror_spectrum([7.0], 1).tolist() == [7.0]
    assert metrics.mirror_spectrum([7.0, 3.0], 2).tolist() == [7.0, 3.0]
    assert metrics.mirror_spectrum(np.arange(6.0).reshape(2, 3), 4).tolist() == [[0, 1, 2, 1], [3, 4, 5, 4]]
    for T in (6, 7, 33, 64):                                    # against the FFT of a real series itself
        x = np.cos(np.arange(T) * 0.7) + np.arange(T) % 3
        full = np.abs(np.fft.fft(x))
        assert np.allclose(metrics.mirror_spectrum(full[:T // 2 + 1], T), full, rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        metrics.mirror_spectrum([1.0, 2.0, 3.0], 7)


def test_high_band_share_on_hand_made_spectra():
    even = np.array([100.0, 4.0, 2.0, 1.0, 8.0, 1.0, 2.0, 4.0])        # T = 8, Nyquist bin 4 once
    assert metrics.high_band_share(even, 1) == 1.0
    assert metrics.high_band_share(even, 2) == pytest.approx((2 + 1 + 8 + 1 + 2) / 22)
    assert metrics.high_band_share(even, 4) == pytest.approx(8 / 22)
    assert metrics.high_band_share(even, 5) == 0.0                      # empty band
    odd = np.array([100.0, 4.0, 2.0, 1.0, 1.0, 2.0, 4.0])              # T = 7
    assert metrics.high_band_share(odd, 2) == pytest.approx(6 / 14)
    assert metrics.high_band_share(odd, 3) == pytest.approx(2 / 14)
    assert metrics.high_band_share(np.array([9.0, 0.0, 0.0]), 1) == 0.0     # a static clip: no non-DC power
    assert metrics.high_band_share(np.array([9.0]), 1) == 0.0               # T = 1
    with pytest.raises(ValueError):
        metrics.high_band_share(even, 0)
    with pytest.raises(ValueError):
        metrics.high_band_share(even.reshape(2, 4), 1)


def test_report_cutoffs_are_the_latent_nyquist_bin():
    # 129 frames -> 33 latent samples: 1 / (2 * 129 / 33) cycles per frame; the first bin with k / 129 >= 33 / 258 is 17 (16.5 rounded up)
    assert metrics.latent_nyquist_bin(129, 129, 33) == 17
    assert metrics.latent_nyquist_bin(128, 128, 32) == 16               # k / 128 >= 1 / 8 exactly at 16
    assert metrics.latent_nyquist_bin(9, 9, 3) == 2
    assert metrics.latent_nyquist_bin(8, 9, 3) == 2                     # a reconstruction one frame short: 8 * 3 / 18 = 1.33 -> 2
    assert metrics.latent_nyquist_bin(5, 5, 5) == 3 and metrics.latent_nyquist_bin(4, 4, 1) == 1
    flat = lambda T: {"power": np.concatenate([[50.0], np.ones(T - 1)]), "magnitude": np.ones(T)}
    rep = metrics.add_high_band_shares({"input": flat(9), "latent": flat(3), "reconstruction": flat(9)})
    assert rep["input"]["cutoff_bin"] == 2 == rep["reconstruction"]["cutoff_bin"] and rep["latent"]["cutoff_bin"] == 1
    assert rep["input"]["high_band_share"] == pytest.approx(6 / 8)      # bins 2 .. 7 of 1 .. 8
    assert rep["latent"]["high_band_share"] == 1.0
    rep = metrics.add_high_band_shares({"input": flat(16), "latent": flat(4), "reconstruction": flat(16)})
    assert rep["input"]["cutoff_bin"] == 2 and rep["input"]["high_band_share"] == pytest.approx(13 / 15)
    batch = {"power": np.stack([flat(9)["power"], np.concatenate([[1.0], np.zeros(8)])]), "magnitude": np.ones((2, 9))}
    rep = metrics.add_high_band_shares({"input": batch, "latent": flat(3), "reconstruction": flat(9)})
    assert rep["input"]["high_band_share"].tolist() == pytest.approx([6 / 8, 0.0])
    js = metrics.spectrum_json(metrics.add_high_band_shares({"input": flat(9), "latent": flat(3), "reconstruction": flat(9)}))
    assert isinstance(js["input"]["power"], list) and isinstance(js["latent"]["high_band_share"], float)


def test_refusals_on_the_host():
    with pytest.raises(_lib.HVKernelError, match="GPU tensor"):
        metrics.temporal_spectrum(torch.zeros(3, 4, 8, 8))
    with pytest.raises(_lib.HVKernelError, match="GPU tensor"):
        metrics.temporal_spectrum(np.zeros((3, 4, 8, 8)))
    with pytest.raises(_lib.HVKernelError, match="GPU tensor"):
        metrics.spectrum_report(torch.zeros(3, 4, 8, 8), torch.zeros(16, 1, 1, 1), torch.zeros(3, 4, 8, 8))
    for T in (0, 1025):
        with pytest.raises(_lib.HVKernelError):
            metrics.spectrum_twiddles(T)


# ---- the twiddle table ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 3, 31, 32, 33, 64, 65, 129, 600, 1024])
def test_twiddle_table_against_float64(T):
    tab = metrics.spectrum_twiddles(T)
    assert tab.dtype == torch.float32 and tab.is_contiguous()
    tab = tab.numpy()
    nb = T // 2
    ncol = max(1, -(-nb // 32))
    assert tab.shape == (-(-T // 32) * 32, 64 * ncol)
    assert not tab[T:].any()                                    # rows behind T
    worst = 0.0
    for j in range(ncol):
        for c in range(64):
            k = 1 + 32 * j + (c & 31)
            col = tab[:T, 64 * j + c].astype(np.float64)
            if k > nb:
                assert not col.any(), (j, c)
                continue
            r = np.array([(k * t) % T for t in range(T)], dtype=np.float64)       # python integers: no overflow, no rounding
            want = (np.cos if c < 32 else np.sin)(2.0 * np.pi * r / T)
            # half an ulp of the fp32 value (spacing at |want|) plus float64's own error in the angle and the function
            half_ulp = 0.5 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            worst = max(worst, float(np.max((np.abs(col - want) - 1e-15) / half_ulp)))
    assert worst <= 1.0, worst
    cos, sin = dbl.table_columns(T)
    assert cos.shape == (T, nb) == sin.shape
    if nb:
        assert np.all(cos[0] == 1.0) and not sin[0].any()       # t = 0


# ---- the bound: what passes --------------------------------------------------------------------------------------------------------
def _signals(T, N, gray, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None]
    if gray:
        return {"noise": rng.integers(0, 256, (T, N)),
                "static": 128 + rng.integers(-1, 2, (T, N)) * (rng.random((T, N)) < 0.2),
                "ramp": np.clip(t * 255 // max(T - 1, 1) + rng.integers(0, 3, (1, N)), 0, 255)}
    f = lambda a: a.astype(np.float32).astype(np.float64)
    return {"noise": f(rng.standard_normal((T, N))), "static": f(3.0 + 1e-3 * rng.standard_normal((T, N))),
            "ramp": f(t / max(T - 1, 1) * 2 - 1 + 0.1 * rng.standard_normal((1, N)))}


def _series_ratio(sig, gray, **kw):
    r = ref.Spectrum(sig, gray)
    mag, pw = dbl.series_spectrum(sig, gray, **kw)
    K = sig.shape[0] // 2 + 1
    out = []
    for got, want, b in ((mag, r.series_mag[:K], r.series_mag_bound[:K]), (pw, r.series_pow[:K], r.series_pow_bound[:K])):
        err = np.abs(got - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            out.append(np.where(err == 0.0, 0.0, err / b))
    return np.maximum(out[0], out[1])                           # [K, N]


@pytest.mark.parametrize("gray", [True, False], ids=["gray", "raw"])
@pytest.mark.parametrize("T", [3, 33, 129, 600, 1024])
def test_double_passes_the_bound_per_series_in_three_orders(T, gray):
    N = 160 if T < 600 else 48 if T == 600 else 16
    worst = {}
    for name, sig in _signals(T, N, gray, T).items():
        for order in ORDERS:
            r = _series_ratio(sig, gray, order=order)
            worst[(name, order)] = (float(r[1:].max()), float(r[0].max()))
    print(f"T {T} {'gray' if gray else 'raw'}: " + ", ".join(f"{n}/{o} {a:.2f} dc {b:.2f}" for (n, o), (a, b) in worst.items()))
    assert max(a for a, _ in worst.values()) <= 1.0 and max(b for _, b in worst.values()) <= 1.0, worst
    if gray:
        assert max(b for _, b in worst.values()) == 0.0         # integer DC: exact


def test_double_static_series_give_exact_zeros():
    sig = np.full((33, 5), 128)
    mag, pw = dbl.series_spectrum(sig, True)
    assert not mag[1:].any() and not pw[1:].any() and np.all(mag[0] == 33 * 128)


# ---- the bound: what it rejects -----------------------------------------------------------------------------------------------------
def _video(T, H, W, kind, seed):
    """float32 [3, T, H, W] in [-1, 1] with distinct channels"""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        x = rng.random((3, T, H, W)) * 2 - 1
        x[2] *= 0.3                                             # R and B differ in level
    else:                                                       # near-static: grey level ~128, a +-1 flicker on a fifth of the samples
        q = 128 + rng.integers(-1, 2, (1, T, H, W)) * (rng.random((1, T, H, W)) < 0.2)
        x = np.repeat((q + 0.5) / 255.0 * 2 - 1, 3, axis=0)
    return x.astype(np.float32)


def _mean_ratio(x, mode="gray", **kw):
    sig = ref.gray_series(x) if mode == "gray" else ref.raw_series(x)
    got = dbl.temporal_spectrum(x, mode, **kw)
    return max(ref.Spectrum(sig, mode == "gray").ratios(got["magnitude"], got["power"]))


def test_mean_spectra_of_the_double_pass():
    for T, kind in ((8, "noise"), (9, "noise"), (33, "static"), (64, "static")):
        x = _video(T, 5, 7, kind, T)
        assert _mean_ratio(x) <= 1.0, (T, kind)
        assert _mean_ratio(x[:, :, :2, :3], "raw") <= 1.0, (T, kind)
    assert _mean_ratio(_video(600, 3, 4, "noise", 1)) <= 1.0


MUTANTS = [
    ("no pivot on near-static data", dict(pivot=False), 64, "static"),
    ("last frame dropped", dict(drop_last_frame=True), 9, "noise"),
    ("mean over the padded series count", dict(padded_count=True), 9, "noise"),
    ("R and B swapped", dict(swap_rb=True), 9, "noise"),
    ("luma truncated instead of rounded", dict(luma=ref.GRAY_LUMA[:3] + (0, 15)), 9, "noise"),
    ("magnitude from re alone", dict(re_only=True), 9, "noise"),
    ("mirror off by one", dict(mirror_off_by_one=True), 9, "noise"),
    ("mirror off by one, even T", dict(mirror_off_by_one=True), 8, "noise"),
    ("Nyquist bin doubled", dict(double_nyquist=True), 8, "noise"),
]


@pytest.mark.parametrize("what,kw,T,kind", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_bound_rejects_mutant(what, kw, T, kind):
    x = _video(T, 5, 7, kind, 3)
    assert _mean_ratio(x) <= 1.0
    r = _mean_ratio(x, **kw)
    print(f"{what}: ratio {r:.3g}")
    assert r > 1.0, what


def test_bound_rejects_twiddles_from_an_unreduced_fp32_angle_at_600_frames():
    x = _video(600, 3, 4, "noise", 1)
    r = _mean_ratio(x, twiddles=dbl.unreduced_fp32_twiddles(600))
    print(f"unreduced fp32 angle, T = 600: ratio {r:.3g}")
    assert r > 1.0
    sig = ref.raw_series(_video(600, 1, 2, "noise", 2)[:1])
    assert _series_ratio(sig, False, twiddles=dbl.unreduced_fp32_twiddles(600))[1:].max() > 1.0
