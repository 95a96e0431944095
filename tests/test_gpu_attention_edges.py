"""GPU: the attention kernel (csrc/hv_attention_w4.hip + the generated hv_attention_w4_loop.inc) at every loop tail, against the fp64
contract and per-element bound of tests/attention_bounds.py, with q / k / v embedded in NaN-poisoned memory, every output in a
sentinel-filled buffer, and an exact key census.

Which loop iteration a key count reaches (ntiles = ceil(n_kv / 64); the steady-state statement runs in groups of four while
t + 6 < ntiles, then 0-5 compiler-scheduled tail iterations, then the last tile, masked when n_kv % 64 != 0):

    ntiles  1        prologue + last tile only                    ntiles  7 .. 10   one group  + 2, 3, 4, 5 tail iterations
    ntiles  2 .. 6   no steady state, 1 .. 5 tail iterations      ntiles 11, 12     two groups + 2, 3 tail iterations
    n_kv 4096 / 4097, 4159 / 4224 / 4288 = 64 / 65 / 66 / 67 tiles: 15 groups (static or online statement) + 3 / 4 / 5 groups' tail, 16 groups + 2
    KV split of those (hv_attn_fwd_bf16, halves of ceil(ntiles / 2) tiles): 32 + 32, 33 + 32 (4097: the second half ends in ONE key;
      4159: in 63), 33 + 33, 34 + 33 tiles
    hv_attn_partial_bf16 splits = 2: n_kv 65 = 64 + 1 key, 128 = 64 + 64, 129 = 128 + 1, 191 = 128 + 63

test_loop_tails / test_key_census run ntiles 1 .. 12 x remainder {1, 31, 32, 33, 63, 64} (the mask on both 32-key halves of the tile)
with n_q = 321: the second workgroup has one full wave, one wave with a single row and two waves past the end.

Data classes (attention_bounds.make_case): random, peaked (rescale for some rows of a query block only; peak in tile 0 / the last
full tile / the last valid key), flat, phantom (a key read behind n_kv would own the row).  Census (q = 0: p = 1 exactly): the
partials must hold the integer column sums of v, l = n_kv and m = 0 bit-exactly - a dropped, duplicated or phantom key changes
an integer - and the normalised output is within 1 bf16 ulp of sum v / n_kv.

Memory: q, k, v are column blocks of ONE buffer with ld = 3 H 128 + 8 (a row stride that is no multiple of 256 bytes), NaN in the
rows before / after, in columns [3 H 128, ld) and in the rows of q behind n_q and of k, v behind n_kv; test_strides gives k and v
buffers and strides of their own.  Outputs: stride H 128 + 16, sentinel rows after n_q.  No NaN may reach an output, every sentinel
and every poisoned cell keeps its bits, a repeated launch gives the same bits.

Largest error-to-bound ratio per path (test_zz_ratio_report requires 0.05 < ratio <= 1 on each), measured on an MI355X:
    online 0.619, static 0.707, fwd-split 0.725, partial 0.846, merge 0.624"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import attention_bounds as AB  # noqa: E402
from tests import error_bounds as EB  # noqa: E402

DEV = "cuda"
D, KVT = AB.D, AB.KVT
BF16 = torch.bfloat16
NAN16, SENT16, SENT32 = 0x7FFF, 0x7E5A, 0x7F5A5A5A
REMS = (1, 31, 32, 33, 63, 64)
LONG_KV = (4096, 4097, 4159, 4224, 4288)
PATHS = ("online", "static", "fwd-split", "partial", "merge")
RATIOS = {}
SCALE = D ** -0.5


@pytest.fixture(scope="module")
def ops():
    from hunyuanvideo_efficiency_amd import ops as _ops, _lib
    _lib.torch_ops()
    return _ops


def _record(path, r):
    RATIOS[path] = max(RATIOS.get(path, 0.0), r)


# ------------------------------------------------------------------------------------------------------ poisoned / guarded memory
class Operands:
    """q [n_q, H*128], k, v [n_kv, H*128] inside NaN-filled memory.  fused: column blocks of one [3 + rows + 5, 3 H 128 + 8] buffer;
    else three buffers with row strides H 128 + 8 (q), + 8 (k), + 24 (v)."""

    def __init__(self, q, k, v, fused=True, before=3, after=5):
        n_q, n_kv, hd = q.shape[0], k.shape[0], q.shape[1]
        self.bufs, self.masks = [], []

        def place(buf, mask, t, c0):
            view = buf.view(BF16)[before:before + t.shape[0], c0:c0 + hd]
            view.copy_(t)
            mask[before:before + t.shape[0], c0:c0 + hd] = False
            return view

        def alloc(rows, ld):
            buf = torch.full((before + rows + after, ld), NAN16, dtype=torch.int16, device=DEV)
            self.bufs.append(buf)
            self.masks.append(torch.ones_like(buf, dtype=torch.bool))
            return buf, self.masks[-1]

        if fused:
            buf, mask = alloc(max(n_q, n_kv), 3 * hd + 8)
            self.q, self.k, self.v = place(buf, mask, q, 0), place(buf, mask, k, hd), place(buf, mask, v, 2 * hd)
        else:
            self.q = place(*alloc(n_q, hd + 8), q, 0)
            self.k = place(*alloc(n_kv, hd + 8), k, 0)
            self.v = place(*alloc(n_kv, hd + 24), v, 0)

    def intact(self):
        return all(bool((b[m] == NAN16).all()) for b, m in zip(self.bufs, self.masks))


class GuardedOut:
    """bf16 output [n_q, H*128] at rows [2, 2 + n_q), columns [0, H*128) of a sentinel-filled [2 + n_q + 3, H*128 + 16] buffer"""

    def __init__(self, n_q, hd):
        self.buf = torch.full((2 + n_q + 3, hd + 16), SENT16, dtype=torch.int16, device=DEV)
        self.view = self.buf.view(BF16)[2:2 + n_q, :hd]
        self.mask = torch.ones_like(self.buf, dtype=torch.bool)
        self.mask[2:2 + n_q, :hd] = False

    def intact(self):
        return bool((self.buf[self.mask] == SENT16).all())


def guarded_partials(ops, n_slots, n_q, H):
    """AttnPartials whose slots are followed by one sentinel slot"""
    parts = ops.AttnPartials(n_slots, n_q, H, torch.device(DEV))
    parts.o_buf = torch.full((n_slots + 1, n_q, H, D), SENT32, dtype=torch.int32, device=DEV)
    parts.ml_buf = torch.full((n_slots + 1, n_q, H, 2), SENT32, dtype=torch.int32, device=DEV)
    parts.o, parts.ml = parts.o_buf.view(torch.float32)[:n_slots], parts.ml_buf.view(torch.float32)[:n_slots]
    return parts


def partials_intact(parts):
    return bool((parts.o_buf[-1] == SENT32).all()) and bool((parts.ml_buf[-1] == SENT32).all())


def fwd(x, out, H, ws=None):
    """hv_attn_fwd_bf16 with an explicit workspace (None: online maximum, single pass; 256 bytes: the key-norm bound only)"""
    from hunyuanvideo_efficiency_amd import _lib
    _lib.call("attn_fwd_bf16", x.q, x.k, x.v, out, x.q.stride(0), x.k.stride(0), x.v.stride(0), out.stride(0), x.q.shape[0], x.k.shape[0],
              H, D, SCALE, ws, 0 if ws is None else ws.numel())


def modes(ws):
    """(some wave ran against the static row bound, some wave kept the online maximum): words 62 and 63 of the workspace"""
    torch.cuda.synchronize()
    w = ws[:256].view(torch.int32).cpu()
    return bool(w[62]), bool(w[63])


def run_fwd(x, H, ws=None, what=""):
    """two launches into guarded outputs: same bits, no NaN, sentinels and poison intact -> the output"""
    outs = []
    for _ in range(2):
        g = GuardedOut(x.q.shape[0], H * D)
        fwd(x, g.view, H, ws)
        assert g.intact(), f"{what}: a sentinel around the output was overwritten"
        outs.append(g.view.clone())
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), f"{what}: two launches differ"
    assert bool(torch.isfinite(outs[0]).all()), f"{what}: non-finite output"
    assert x.intact(), f"{what}: an operand buffer was written"
    return outs[0]


def run_partial(ops, x, H, splits, what=""):
    parts = guarded_partials(ops, splits, x.q.shape[0], H)
    ops.attn_partial(x.q, x.k, x.v, parts, H, splits)
    first = (parts.o.clone(), parts.ml.clone())
    parts.used = 0
    ops.attn_partial(x.q, x.k, x.v, parts, H, splits)
    assert torch.equal(first[0].view(torch.int32), parts.o.view(torch.int32)) and torch.equal(first[1].view(torch.int32), parts.ml.view(torch.int32)), \
        f"{what}: two launches differ"
    assert partials_intact(parts) and x.intact(), f"{what}: wrote outside its slots"
    assert bool(torch.isfinite(parts.o).all()) and bool(torch.isfinite(parts.ml).all()), f"{what}: non-finite partials"
    return parts


def split_cut(n_kv):
    return ((((n_kv + KVT - 1) // KVT) + 1) // 2) * KVT


def check_online_and_partial(ops, cls, n_q, n_kv, H, key, fused=True):
    q, k, v = AB.make_case(cls, n_q, n_kv, H, key, DEV)
    x = Operands(q, k, v, fused)
    ref = AB.AttnRef(q, k, v, H)
    what = f"{cls} n_q={n_q} n_kv={n_kv}"
    _record("online", ref.check_o(run_fwd(x, H, None, what), what + " online"))
    parts = run_partial(ops, x, H, 1, what)
    _record("partial", ref.check_partial(parts.o[0], parts.ml[0], what + " partial"))


# ------------------------------------------------------------------------------------------------------ loop tails, n_q edges, strides
@pytest.mark.parametrize("ntiles", range(1, 13))
def test_loop_tails(ops, ntiles):
    for r in REMS:
        for cls in AB.CLASSES:
            check_online_and_partial(ops, cls, 321, KVT * (ntiles - 1) + r, 2, "tails")


@pytest.mark.parametrize("n_q", [1, 31, 32, 33, 63, 64, 65, 255, 256, 257])
def test_n_q_edges(ops, n_q):
    for cls in AB.CLASSES:
        check_online_and_partial(ops, cls, n_q, 449, 2, "nq")


@pytest.mark.parametrize("n_q,n_kv", [(321, 449), (33, 64 * 7 + 33), (257, 129)])
def test_strides(ops, n_q, n_kv):
    """k and v in buffers of their own with different row strides (neither a multiple of 256 bytes)"""
    for cls in ("random", "phantom"):
        check_online_and_partial(ops, cls, n_q, n_kv, 2, "strides", fused=False)


# ------------------------------------------------------------------------------------------------------ key census
def census_v(n_kv, case):
    j, d = torch.arange(n_kv, device=DEV)[:, None], torch.arange(D, device=DEV)[None]
    return (j % 128 == d).float() if case == "A" else ((7 * j + 3 * d) % 11 - 5).float()


@pytest.mark.parametrize("ntiles", range(1, 13))
def test_key_census(ops, ntiles):
    n_q, H = 321, 2
    for r in REMS:
        n_kv = KVT * (ntiles - 1) + r
        for case in "AB":
            v1 = census_v(n_kv, case)
            v = torch.cat([v1, -v1.flip(1)], 1).to(BF16)                      # head 1: another pattern, exact integers too
            k = AB.make_case("flat", n_q, n_kv, H, "census", DEV)[1]
            x = Operands(torch.zeros(n_q, H * D, dtype=BF16, device=DEV), k, v)
            what = f"census {case} n_kv={n_kv}"
            parts = run_partial(ops, x, H, 1, what)
            sums = v.float().sum(dim=0).reshape(1, H, D).expand(n_q, H, D)
            assert torch.equal(parts.ml[0, ..., 0], torch.zeros(n_q, H, device=DEV)), f"{what}: m != 0"
            assert torch.equal(parts.ml[0, ..., 1], torch.full((n_q, H), float(n_kv), device=DEV)), \
                f"{what}: l != n_kv (l in [{float(parts.ml[0, ..., 1].min())}, {float(parts.ml[0, ..., 1].max())}])"
            assert torch.equal(parts.o[0], sums), f"{what}: {int((parts.o[0] != sums).sum())} column sums differ (max {float((parts.o[0] - sums).abs().max())})"
            out = run_fwd(x, H, None, what)
            want = (sums.double() / n_kv).reshape(n_q, H * D)
            err = (out.double() - want).abs()
            assert bool((err <= EB.ulp_out(want, BF16)).all()), f"{what}: normalised output off by {float((err / EB.ulp_out(want, BF16)).max()):.3g} ulp"


# ------------------------------------------------------------------------------------------------------ long key ranges: static / online / KV split
_LONG = {}


def long_case(cls, n_q, n_kv, H):
    """operands, the reference (its gap covers the static bound and the halves of a KV split), and the predicted mode, computed once"""
    key = (cls, n_q, n_kv, H)
    if key not in _LONG:
        q, k, v = AB.make_case(cls, n_q, n_kv, H, "long", DEV)
        gap = AB.kernel_gap(q, k, H, cuts=(split_cut(n_kv),), static=True)
        # bound - row max of tile 0, per row and head: the kernel's static-mode decision (<= 90 for every row of a wave)
        margin = torch.stack([AB.static_row_bound(q[:, h * D:(h + 1) * D], k[:, h * D:(h + 1) * D]) -
                              (AB.q_prime(q[:, h * D:(h + 1) * D]).double() @ k[:KVT, h * D:(h + 1) * D].double().T).max(dim=1).values for h in range(H)], 1)
        _LONG[key] = (Operands(q, k, v), AB.AttnRef(q, k, v, H, gap=gap), float(margin.min()), float(margin.max()))
    return _LONG[key]


def expect_mode(ws, lo, hi, what):
    got = modes(ws)
    if hi < 89.0:
        assert got == (True, False), f"{what}: bound - max in [{lo:.1f}, {hi:.1f}] but modes (static, online) = {got}"
    elif lo > 91.0:
        assert got == (False, True), f"{what}: bound - max in [{lo:.1f}, {hi:.1f}] but modes (static, online) = {got}"
    else:
        assert got[0] or got[1]
    return "static" if got == (True, False) else "online"


@pytest.mark.parametrize("n_kv", LONG_KV)
def test_static_and_online_maximum_long(ops, n_kv):
    """a 256-byte workspace (the key-norm bound alone, no KV split) -> the static maximum where the data allow it (random, peaked,
    flat; phantom's bound sits ~130 above its scores -> online); no workspace -> the online maximum over the same 64-67 tiles"""
    n_q, H = 300, 2
    seen = set()
    for cls in AB.CLASSES:
        x, ref, lo, hi = long_case(cls, n_q, n_kv, H)
        what = f"{cls} n_q={n_q} n_kv={n_kv}"
        ws = torch.zeros(256, dtype=torch.uint8, device=DEV)
        out = run_fwd(x, H, ws, what + " ws256")
        path = expect_mode(ws, lo, hi, what)
        seen.add(path)
        _record(path, ref.check_o(out, f"{what} {path} (256-byte workspace)"))
        _record("online", ref.check_o(run_fwd(x, H, None, what), what + " online (no workspace)"))
    assert seen == {"static", "online"}


@pytest.mark.parametrize("n_q", [200, 300])
@pytest.mark.parametrize("n_kv", LONG_KV)
def test_kv_split_inside_fwd(ops, n_kv, n_q):
    """a full workspace and a grid of one / two workgroups: hv_attn_fwd_bf16 halves the key range and merges; the result is held
    to the single pass's fp64 bound (not to the single pass)"""
    H = 1
    assert ops.attn_suggest_splits(n_q, n_kv, H) == 2              # the same rule hv_attn_fwd_bf16 applies
    for cls in AB.CLASSES:
        x, ref, lo, hi = long_case(cls, n_q, n_kv, H)
        ws = torch.zeros(int(ops._lib.host("attn_workspace_bytes", n_q, n_kv, H)), dtype=torch.uint8, device=DEV)
        what = f"{cls} n_q={n_q} n_kv={n_kv} kv-split"
        out = run_fwd(x, H, ws, what)
        got = modes(ws)
        assert got[0] or got[1]
        if cls == "phantom":
            assert got == (False, True), got
        _record("fwd-split", ref.check_o(out, what))


# ------------------------------------------------------------------------------------------------------ partials and merge
@pytest.mark.parametrize("n_kv", [65, 128, 129, 191])
def test_partial_two_slots_and_merge(ops, n_kv):
    n_q, H = 321, 2
    cut = split_cut(n_kv)
    for cls in AB.CLASSES:
        q, k, v = AB.make_case(cls, n_q, n_kv, H, "p2", DEV)
        x = Operands(q, k, v)
        what = f"{cls} n_kv={n_kv} splits=2"
        parts = run_partial(ops, x, H, 2, what)
        for s, (a, b) in enumerate(((0, cut), (cut, n_kv))):
            _record("partial", AB.AttnRef(q, k[a:b], v[a:b], H).check_partial(parts.o[s], parts.ml[s], f"{what} slot {s}"))
        g = GuardedOut(n_q, H * D)
        ops.attn_merge(parts, g.view)
        assert g.intact() and bool(torch.isfinite(g.view).all()), what
        ref = AB.AttnRef(q, k, v, H, gap=AB.kernel_gap(q, k, H, cuts=(cut,)))
        _record("merge", ref.check_o(g.view, what + " merged"))
        r = float(AB.merge_ratio(g.view, parts.o, parts.ml).max())
        assert r <= 1.0, f"{what}: merge of its own partials off by {r:.3g} x the bound"


@pytest.mark.parametrize("n_slots", [1, 2, 3, 4])
def test_merge_slots(ops, n_slots):
    """ring chunks of 65, 128, 191 and 129 keys -> 1 .. 4 slots, merged: against attention over the concatenated keys (fp64 bound) and
    against the fp64 merge of the same partials; then one slot's m raised by 160: every other weight underflows to 0 exactly"""
    n_q, H = 321, 2
    chunks = (65, 128, 191, 129)[:n_slots]
    edges = [sum(chunks[:i]) for i in range(n_slots + 1)]
    for cls in ("random", "peaked", "phantom"):
        q, k, v = AB.make_case(cls, n_q, edges[-1], H, "ring", DEV)
        x = Operands(q, k, v)
        parts = guarded_partials(ops, n_slots, n_q, H)
        for a, b in zip(edges[:-1], edges[1:]):
            ops.attn_partial(x.q, x.k[a:b], x.v[a:b], parts, H, 1)
        g = GuardedOut(n_q, H * D)
        ops.attn_merge(parts, g.view)
        what = f"{cls} {n_slots} slots"
        assert g.intact() and partials_intact(parts) and x.intact() and bool(torch.isfinite(g.view).all()), what
        ref = AB.AttnRef(q, k, v, H, gap=AB.kernel_gap(q, k, H, cuts=edges[1:-1]))
        _record("merge", ref.check_o(g.view, what + " merged"))
        assert float(AB.merge_ratio(g.view, parts.o, parts.ml).max()) <= 1.0, what
        # one slot far above the others
        parts.ml[n_slots - 1, ..., 0] += 160.0
        g2 = GuardedOut(n_q, H * D)
        ops.attn_merge(parts, g2.view)
        assert g2.intact() and bool(torch.isfinite(g2.view).all()), what
        r = float(AB.merge_ratio(g2.view, parts.o, parts.ml).max())
        assert r <= 1.0, f"{what}: merge with one slot 160 above off by {r:.3g} x the bound"
        alone = parts.o[n_slots - 1].double() / parts.ml[n_slots - 1, ..., 1:2].double()
        assert bool(((g2.view.double().reshape(n_q, H, D) - alone).abs() <= EB.ulp_out(alone, BF16)).all()), what


# ------------------------------------------------------------------------------------------------------ report
def test_zz_ratio_report(capsys):
    with capsys.disabled():
        print("\nattention: largest error / fp64 bound per path: " + ", ".join(f"{p} {RATIOS.get(p, float('nan')):.3f}" for p in PATHS))
    for p in PATHS:
        assert p in RATIOS, f"path {p} was never measured (run the whole file)"
        assert 0.05 < RATIOS[p] <= 1.0, f"{p}: ratio {RATIOS[p]:.3g} (a bound looser than 0.05 catches nothing)"
