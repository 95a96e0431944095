"""GPU: the linear temporal interpolation (csrc/hv_temporal.hip) through torch.ops.hv.temporal_interp_f16 and through the ctypes entry
hv_temporal_interp_f16, against the fp64 reference and per-element bound of tests/tinterp_bounds.py (whose CPU test shows what the bound
accepts and rejects).  Operands sit in NaN-poisoned buffers with padded pitches, outputs in sentinel-filled ones
(tests/guarded_memory.py).  Checked: the bound on every element, the bits of the copies (lambda == 0, clamped ends, s == 1), the share of
outputs that differ from the correctly rounded fp64 value, run-to-run identity, the two entry paths bit for bit, the launch partitions
the host picks (a walk of 1, 2 and 8 source intervals per lane, a ragged last chunk, the second grid-stride trip above the grid cap) and
one refusal per rule of include/hv_temporal.h with the output left untouched."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from hunyuanvideo_efficiency_amd import synthetic as syn  # noqa: E402
from tests import tinterp_bounds as B  # noqa: E402
from tests.guarded_memory import Guarded, Poisoned, bits, same_bits  # noqa: E402

DEV = "cuda"
F16 = torch.float16
CAP = 8192 * 256                           # lanes of the capped grid (csrc/hv_temporal.hip: kMaxBlocks * kThreads)


@pytest.fixture(scope="module")
def L():
    from hunyuanvideo_efficiency_amd import _lib
    _lib.torch_ops()
    return _lib


def walk_of(T_in, HW, C):
    """the host's choice of source intervals per lane (hv_temporal_interp_f16), mirrored"""
    plane, walk = HW * (C // 8), 1
    while walk < 8 and -(-T_in // (2 * walk)) >= -(-CAP // plane):
        walk *= 2
    return walk


def via_torch(L, X, o, T_in, HW, C, s):
    L.call("temporal_interp_f16", X, X.stride(0), o, o.stride(0), T_in, HW, C, s)


def via_ctypes(L, X, o, T_in, HW, C, s):
    torch.cuda.synchronize()
    rc = L.load().hv_temporal_interp_f16(X.data_ptr(), X.stride(0), o.data_ptr(), o.stride(0), T_in, HW, C, s, None)
    torch.cuda.synchronize()
    assert rc == 0, rc


def _case(L, T_in, HW, C, s):
    what = f"temporal_interp T_in={T_in} HW={HW} C={C} s={s}"
    x = B.activations(T_in, HW, C, "gpu")
    X = Poisoned(x.to(DEV), 3, 5, 8)
    outs = []
    for run in (via_torch, via_ctypes, via_torch):
        o = Guarded(T_in * s * HW, C, F16, pad=16)
        run(L, X.view, o.view, T_in, HW, C, s)
        assert o.intact() and X.intact(), f"{what}: a store outside the output"
        outs.append(o.view.cpu())
    assert same_bits(outs[0], outs[1]), f"{what}: torch.ops.hv and the ctypes entry differ"
    assert same_bits(outs[0], outs[2]), f"{what}: two runs differ"
    got = outs[0]
    y64, bound = B.tinterp_ref(x, T_in, HW, s)
    r = B.check(got, y64, bound, what)
    cp = B.copies(T_in, s).repeat_interleave(HW)
    t0 = B.frames(T_in, s)[0]
    src = x.reshape(T_in, HW, C)[t0].reshape(T_in * s * HW, C)
    assert same_bits(got[cp], src[cp]), f"{what}: a copy frame does not have the input's bits"
    if s == 1:
        assert same_bits(got, x), what
    return r, got, y64


@pytest.mark.parametrize("s", B.SCALES)
@pytest.mark.parametrize("T_in", B.T_INS)
def test_interp_grid(L, T_in, s):
    worst, n_bad, n = 0.0, 0, 0
    for HW in B.HWS:
        for C in B.CS:
            assert walk_of(T_in, HW, C) == 1
            r, got, y64 = _case(L, T_in, HW, C, s)
            worst = max(worst, r)
            n_bad += int(round(B.mismatch_share(got, y64, F16) * got.numel()))
            n += got.numel()
    print(f"T_in={T_in} s={s}: worst error / bound {worst:.3f}, bits differ from RNE(fp64) on {n_bad} of {n}")
    assert n_bad / n <= B.mismatch_cap(n), (n_bad, n)


def test_copies_carry_nan_payloads_and_signed_zeros(L):
    """a copy is a copy of bits: the kernel must not pass the clamped frames or the lambda == 0 frames through its arithmetic"""
    T_in, HW, C, s = 3, 2, 8, 3
    x = B.activations(T_in, HW, C, "nan").to(DEV)
    xb = bits(x).clone()
    xb[0, 0], xb[1, 1], xb[2, 2], xb[5, 3] = 0x7E01, -0x8000, 0x7C00, -0x1FF          # a NaN payload, -0, +inf, another NaN (0xFE01)
    x = xb.view(F16)
    o = Guarded(T_in * s * HW, C, F16)
    via_torch(L, x, o.view, T_in, HW, C, s)
    cp = B.copies(T_in, s).repeat_interleave(HW)
    t0 = B.frames(T_in, s)[0]
    src = x.cpu().reshape(T_in, HW, C)[t0].reshape(-1, C)
    assert same_bits(o.view.cpu()[cp], src[cp]) and o.intact()


def _big(L, T_in, HW, C, s, walk, trips):
    """a launch too large for the CPU reference in one piece: checked frame by frame on the device, same reference, same bound"""
    plane = HW * (C // 8)
    assert walk_of(T_in, HW, C) == walk and (-(-T_in // walk) * plane > CAP) == (trips > 1)
    x = (syn.hashed_uniform((T_in * HW, C), f"tinterp.big.{T_in}.{HW}.{C}", 47, DEV) * 3.0 ** 0.5).to(F16)
    X = Poisoned(x, 3, 5, 8)
    del x
    o = Guarded(T_in * s * HW, C, F16, pad=8)
    via_torch(L, X.view, o.view, T_in, HW, C, s)
    assert o.intact() and X.intact()
    t0, t1, r = B.frames(T_in, s)
    cp = B.copies(T_in, s)
    worst, n_bad = 0.0, 0
    for t in range(T_in * s):
        x0, x1 = (X.view[int(k) * HW:(int(k) + 1) * HW] for k in (t0[t], t1[t]))
        got = o.view[t * HW:(t + 1) * HW]
        if cp[t]:
            assert same_bits(got, x0), t
            continue
        lam = float(r[t]) / (2 * s)
        y64 = (1.0 - lam) * x0.double() + lam * x1.double()
        bound = B.ulp_out(y64, F16) + B.E32 * (x0.double().abs() + x1.double().abs()) + \
            float(B.dlambda(torch.tensor(float(t0[t]) + lam))) * (x1.double() - x0.double()).abs()
        worst = max(worst, B.check(got, y64, bound, f"T_in={T_in} HW={HW} C={C} s={s} frame {t}"))
        n_bad += int(round(B.mismatch_share(got, y64, F16) * got.numel()))
    n = T_in * s * HW * C
    print(f"T_in={T_in} HW={HW} C={C} s={s} walk={walk}: worst error / bound {worst:.3f}, bits differ on {n_bad} of {n}")
    assert n_bad / n <= B.mismatch_cap(n)
    o2 = Guarded(T_in * s * HW, C, F16, pad=8)
    via_torch(L, X.view, o2.view, T_in, HW, C, s)
    assert torch.equal(o.buf, o2.buf)


def test_second_grid_stride_trip(L):
    _big(L, 3, (1 << 20) + 3, 16, 2, walk=8, trips=2)          # one chunk of 3 intervals per lane; 2 * (2^20 + 3) lanes > 8192 * 256


def test_walk_of_two_with_a_ragged_last_chunk(L):
    _big(L, 9, (1 << 18) + 1, 16, 3, walk=2, trips=2)          # chunks of 2, 2, 2, 2, 1 intervals


def test_walk_of_eight_over_three_chunks(L):
    _big(L, 17, (1 << 17) + 5, 64, 2, walk=8, trips=2)         # chunks of 8, 8, 1 intervals; the shape class of a decoder activation


REFUSALS = [("C % 8 == 0", dict(C=12)), ("C > 0", dict(C=0)), ("ldx % 8 == 0", dict(ldx=68)), ("ldo % 8 == 0", dict(ldo=84)),
            ("T_in > 0", dict(T_in=0)), ("HW > 0", dict(HW=0)), ("s >= 1", dict(s=0)), ("T_in * s fits an int", dict(T_in=1 << 16, s=1 << 15)),
            ("T_out * HW * C/8 fits an int64", dict(HW=1 << 61)), ("output pitch: ldo >= C", dict(ldo=8)), ("x not NULL", dict(x=None)),
            ("out not NULL", dict(out=None)), ("x 16-byte aligned", dict(x_off=4)), ("out 16-byte aligned", dict(out_off=4))]


@pytest.mark.parametrize("rule,ov", REFUSALS, ids=[r for r, _ in REFUSALS])
def test_refusal_leaves_the_output_untouched(L, rule, ov):
    T_in, HW, C, s = 2, 3, 64, 2
    X = Poisoned(B.activations(T_in, HW, C, "refuse").to(DEV), 3, 5, 8)
    o = Guarded(T_in * s * HW, C, F16, pad=16)
    a = dict(x=X.view, ldx=X.view.stride(0), out=o.view, ldo=o.view.stride(0), T_in=T_in, HW=HW, C=C, s=s)
    assert a["ldx"] == 72 and a["ldo"] == 80
    a.update({k: v for k, v in ov.items() if k in a})
    if "x_off" in ov:
        a["x"] = X.buf.view(F16).reshape(-1)[3 * 72 + ov["x_off"]:]          # 8 bytes behind the first row of the operand
    if "out_off" in ov:
        a["out"] = o.buf.view(F16).reshape(-1)[2 * 80 + ov["out_off"]:]
    order = ("x", "ldx", "out", "ldo", "T_in", "HW", "C", "s")
    with pytest.raises(L.HVKernelError, match="bad argument"):
        L.call("temporal_interp_f16", *[a[k] for k in order])
    torch.cuda.synchronize()
    ptr = [a[k].data_ptr() if isinstance(a[k], torch.Tensor) else a[k] for k in order]
    assert L.load().hv_temporal_interp_f16(*ptr, None) == -1
    torch.cuda.synchronize()
    assert bool((o.buf == o.sent).all()) and X.intact(), rule
    # the accepted neighbour: the same call without the override runs
    via_torch(L, X.view, o.view, T_in, HW, C, s)
    assert o.intact() and not bool((bits(o.view) == o.sent).any())


def test_wrapper(L):
    from hunyuanvideo_efficiency_amd import vae_ops as V
    x = B.activations(5, 7, 72, "wrap")
    out, T = V.temporal_linear_up(x.to(DEV), 5, 7, 3)
    assert T == 15 and tuple(out.shape) == (15 * 7, 72)
    y64, bound = B.tinterp_ref(x, 5, 7, 3)
    B.check(out.cpu(), y64, bound, "temporal_linear_up")
    near, _ = V.temporal_nearest_up(x.to(DEV), 5, 7, 3)
    assert not same_bits(near, out)
