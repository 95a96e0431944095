"""GPU: hv_conv3d_cout4_f16 (GroupNorm affine [+ SiLU] + conv_out: an MFMA planes pass and a 27-plane gather) against the fp64 reference
and per-element bound of tests/conv_bounds.py, with x embedded in NaN-poisoned memory (rows before and after, columns [Cin, ldx)), the
affine and the bias followed by NaNs, the output in a sentinel-filled buffer, and a second launch that must give the same bits.

Shapes (conv_bounds.cout4_cases; tests/test_conv_bounds_cpu.py runs the same operands through fp32 emulations on the CPU):
    Cin in {32, 64, 96, 128}, each at 1x1x1, 3x5x7 (105 voxels: a ragged 16-voxel group), 2x4x6 (M % 16 == 0), and at T = 1, H = 1 and
    W = 1 (every tap along one axis clamps);  Cout in {1, 2, 3};  ldx = Cin + 40;
    ldo = 3 (the scalar-store path: columns Cout..2 and the rows around keep their bits), 8 and 16 (one 16-byte store: columns Cout..7
    zero, columns 8.. untouched);  affine with silu 1 and 0, and no affine.
    Grid cap (2048 blocks x 4 waves x 16 voxels = 131,072 voxels per grid-stride trip), Cin 128: 3 x 209 x 210 = 131,670 voxels (a second
    trip for some waves only) and 5 x 229 x 230 = 263,350 (a third trip: the prefetched `nxt` becomes `cur` twice), with silu 1 and 0; the
    fp64 reference is computed on the GPU in row chunks.

Every case asserts that at most 1 % of its activations are ambiguous (conv_bounds).  test_zz_ratio_report prints the largest
error-to-bound ratio per class (mode; ldo 3 / 8 / 16; the grid-cap cases); each must be above 0.05.  The same logic run against the
CPU doubles (tests/cpu_kernel_doubles.py) reaches 0.48 - 0.49 in every class."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import conv_bounds as CB  # noqa: E402
from tests import rowwise_bounds as RB  # noqa: E402
from tests.guarded_memory import INT, SENT, Poisoned, poisoned_vec, same_bits  # noqa: E402

DEV = "cuda"
F16 = torch.float16
RATIOS = {}
CASES = CB.cout4_cases()


@pytest.fixture(scope="module")
def V():
    from hunyuanvideo_efficiency_amd import vae_ops, _lib
    _lib.load()
    return vae_ops


def _record(cls, r):
    RATIOS[cls] = max(RATIOS.get(cls, 0.0), r)


class GuardedRows:
    """an output [M, ldo] with row stride exactly ldo (ldo = 3: the scalar-store path), 16-byte aligned, between sentinel rows; `cols`
    leading columns of each row belong to the output, the rest are guard cells"""

    def __init__(self, M, ldo, cols, front_rows=16, after_rows=16):
        self.buf = torch.full((front_rows + M + after_rows, ldo), SENT[2], dtype=INT[2], device=DEV)     # 16 rows of ldo fp16: a multiple of 16 B
        self.view = self.buf.view(F16)[front_rows:front_rows + M]
        self.mask = torch.ones_like(self.buf, dtype=torch.bool)
        self.mask[front_rows:front_rows + M, :cols] = False

    def intact(self):
        return bool((self.buf[self.mask] == SENT[2]).all())


def _output(M, ldo, cout):
    if ldo < 8:
        return GuardedRows(M, ldo, cout)
    return GuardedRows(M, ldo, 8)


def _launch_and_check(V, T, H, W, cin, cout, ldo, mode, chunk=None):
    M = T * H * W
    what = f"cout4 {T}x{H}x{W} {cin}->{cout} ldo {ldo} {mode}"
    with_aff, silu = CB.COUT4_MODES[mode]
    x, aff, w, b = CB.cout4_operands(M, cin, cout, CB.cout4_key(T, H, W, cin, cout), DEV)
    aff = aff if with_aff else None
    X = Poisoned(x, 2, 6, 40)                                   # ldx = Cin + 40 > Cin
    affp = poisoned_vec(aff.reshape(-1)).reshape(cin, 2) if with_aff else None
    bias = poisoned_vec(b)
    wf = V.cout4_weight_fragments(w)
    o = _output(M, ldo, cout)
    V.conv_cout4(X.view, affp, silu, wf, bias, T, H, W, cin, cout, out=o.view)
    assert o.intact(), f"{what}: a store outside the output"
    got = o.view.clone()
    if ldo >= 8:
        assert not bool(got[:, cout:8].any()), f"{what}: columns Cout..7 are not zero"
    V.conv_cout4(X.view, affp, silu, wf, bias, T, H, W, cin, cout, out=o.view)
    assert o.intact() and same_bits(o.view, got), f"{what}: a second launch differs"
    assert X.intact()
    h, au, share = CB.cout4_act(x, aff, silu)
    assert share <= CB.AMBIGUOUS_SHARE_LIMIT, f"{what}: {share:.4f} of the activations are ambiguous"
    worst = 0.0
    step = M if chunk is None else chunk
    for r0 in range(0, M, step):
        r1 = min(M, r0 + step)
        y, bound = CB.cout4_ref(h, au, w, b, T, H, W, r0, r1)
        worst = max(worst, RB.check(got[r0:r1, :cout], y, bound, f"{what} rows [{r0}, {r1})"))
    print(f"\n{what}: largest |got - y64| / bound {worst:.3f}, ambiguous share {share:.4f}")
    return worst


@pytest.mark.parametrize("T,H,W,cin,cout,ldo,mode", CASES, ids=[f"{'x'.join(map(str, c[:3]))}-{c[3]}to{c[4]}-ldo{c[5]}-{c[6]}" for c in CASES])
def test_conv_out_edges(V, T, H, W, cin, cout, ldo, mode):
    r = _launch_and_check(V, T, H, W, cin, cout, ldo, mode)
    _record(mode, r)
    _record(f"ldo {ldo}", r)


@pytest.mark.parametrize("T,H,W", CB.COUT4_CAP, ids=["x".join(map(str, c)) for c in CB.COUT4_CAP])
@pytest.mark.parametrize("mode,ldo", [("affine+silu", 8), ("affine", 3)])
def test_conv_out_grid_cap(V, T, H, W, mode, ldo):
    """beyond the planes kernel's grid cap: its second and third grid-stride trips, every output against the bound"""
    _record(f"grid cap {T * H * W}", _launch_and_check(V, T, H, W, 128, 3, ldo, mode, chunk=32768))


def test_bad_arguments_leave_the_output_alone(V):
    """Cin = 48 (not a multiple of 32), Cout = 4 and ldo = 12 (>= 8, not a multiple of 8) are refused before anything is launched"""
    from hunyuanvideo_efficiency_amd._lib import HVKernelError
    x, aff, w, b = CB.cout4_operands(30, 64, 3, "c4.bad", DEV)
    wf = V.cout4_weight_fragments(w)
    for cin, cout, ldo in [(48, 3, 8), (64, 4, 8), (64, 3, 12)]:
        o = GuardedRows(30, ldo, 0)
        with pytest.raises(HVKernelError, match="bad argument"):
            V.conv_cout4(x, aff, True, wf, b, 2, 3, 5, cin, cout, out=o.view)
        torch.cuda.synchronize()
        assert o.intact(), (cin, cout, ldo)


def test_zz_ratio_report():
    """largest error-to-bound ratio per class over this module's cases (run after them); each must use a visible share of the bound"""
    lines = [f"  {p:<20} {RATIOS[p]:.3f}" for p in sorted(RATIOS)]
    print("\nlargest |got - y64| / bound per class:\n" + "\n".join(lines))
    assert set(CB.COUT4_MODES) <= set(RATIOS) and {"ldo 3", "ldo 8"} <= set(RATIOS)
    low = {p: r for p, r in RATIOS.items() if r < 0.05}
    assert not low, f"bound too loose on {low}"
