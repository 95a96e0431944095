"""GPU: the sliding-tile kernel of include/hv_attn_tile.h on HAND-BUILT plans - what the header promises for any valid plan and
ops.tile_plan never produces (tests/test_gpu_attn_tile.py runs its plans): neighbour lists of lengths 0, 1, 2, 3 and 5 in one launch, the
65-token tile (a one-key last chunk) and the 1-token tile first, last and in the middle of a list, a tile listed twice, a dense range over
image rows, a dense range anywhere in [0, n_kv) with n_kv > n_q, an arbitrary permutation, one list per head of different lengths, tiles
without keys, other softmax scales, n_q = 0.

The plans are tests/attn_tile_plans.PLANS; the reference gathers the key rows WITH multiplicity, list order then dense order, from the
hand-written lists (attn_tile_plans.key_rows), never from the plan tensors, and hands them per (tile, head) to AB.AttnRef(.., 1,
gap=AB.THR, scale=..): the bound is the dense kernel's (tests/attention_bounds.py), unchanged, as in test_gpu_attn_tile.check_case.  q, k, v
are views into one fused buffer; the output is a sentinel-filled buffer with 64 guard columns and guard rows behind the image rows.
A tile without keys must get rows of zero BITS.  Keys outside a key set are NaN in `poison`: every output stays finite and in the bound.

MI355X, worst error / bound per group over the classes and head counts (printed per case): ragged 0.485 (dense 0) / 0.459 (1) / 0.489
(65), tiles without keys 0.552, multiplicity 0.531 (the reference that counts every key once is off by 78.5 x the bound on `peaked`),
shuffled perm 0.471, dense range elsewhere 0.469 / empty 0.501, poison 0.546, one list per head 0.479 / 0.470, scale 0.2 0.570 / scale
0.03 0.317.  All against the fp64 references above, none against the kernel itself."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import attention_bounds as AB  # noqa: E402
from tests import attn_tile_plans as TP  # noqa: E402

DEV = "cuda"
D = 128
N = TP.N
CLASSES = ["random", "peaked", "phantom"]


@pytest.fixture(scope="module")
def ops():
    from hunyuanvideo_efficiency_amd import ops as _ops, _lib
    _lib.torch_ops()
    return _ops


def run_plan(ops, name, n_kv, dense, H, cls, scale=None, poison=False, once_ratio=None):
    """one launch on PLANS[name] with k, v of n_kv rows; returns the worst error / bound.  once_ratio: a list that receives the worst
    ratio against the reference that counts every key row once."""
    perm, sizes, lists = TP.PLANS[name]
    TP.validate(perm, sizes, lists, H)
    assert n_kv >= N and 0 <= dense[0] <= dense[1] <= n_kv
    rows_total = n_kv + 3                                      # three rows behind k and v: never a key
    q, k, v = AB.make_case(cls, rows_total, rows_total, H, f"plan.{name}.{n_kv}.{dense}.{H}", device=DEV)
    buf = torch.cat([q, k, v], 1)                              # q, k, v as views into one fused buffer
    qv, kv, vv = buf[:N, :H * D], buf[:n_kv, H * D:2 * H * D], buf[:n_kv, 2 * H * D:]
    if poison:                                                 # every k / v row that is in no key set
        used = {r for per_tile in lists for lst in per_tile for r in TP.key_rows(perm, sizes, lst, dense)}
        dead = torch.tensor(sorted(set(range(rows_total)) - used), device=DEV)
        assert len(dead) > sizes[2] + sizes[4]
        buf[dead, H * D:] = float("nan")
        assert bool(torch.isfinite(qv).all())
    out = torch.full((rows_total, H * D + 64), 7.0, dtype=torch.bfloat16, device=DEV)
    kw = {} if scale is None else {"scale": scale}
    ret = ops.attn_fwd_tile(qv, kv, vv, out[:N, :H * D], H, TP.hand_plan(perm, sizes, lists, DEV), dense=dense, **kw)
    assert ret.data_ptr() == out.data_ptr()
    assert bool((out[N:] == 7.0).all()) and bool((out[:, H * D:] == 7.0).all()), "rows or columns outside the image output were written"
    worst = 0.0
    for h in range(H):
        cols = slice(h * D, (h + 1) * D)
        for t in range(len(sizes)):
            lst = lists[h % len(lists)][t]
            rows = torch.tensor([perm[s] for s in TP.slots(sizes, t)], device=DEV)
            keys = TP.key_rows(perm, sizes, lst, dense)
            what = f"{name} {cls} dense {dense} head {h}/{H} tile {t} list {lst}"
            got = out[rows][:, cols]
            if not keys:
                assert bool((got.view(torch.int16) == 0).all()), f"{what}: a tile without keys must get rows of zero bits"
                continue
            kt = torch.tensor(keys, device=DEV)
            worst = max(worst, AB.AttnRef(qv[rows][:, cols], kv[kt][:, cols], vv[kt][:, cols], 1, gap=AB.THR, scale=scale).check_o(got, what))
            if once_ratio is not None and len(set(keys)) < len(keys):
                ko = torch.tensor(TP.key_rows(perm, sizes, lst, dense, once=True), device=DEV)
                once = AB.AttnRef(qv[rows][:, cols], kv[ko][:, cols], vv[ko][:, cols], 1, gap=AB.THR, scale=scale)
                once_ratio.append(float(once.ratio_o(got).max()))
    print(f"tile attention, hand-built plan {name} {cls} n_kv {n_kv} dense {dense} x {H} scale {scale}: worst error / bound {worst:.3f}")
    return worst


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("n_dense", [0, 1, 65])
def test_ragged_csr(ops, n_dense, H, cls):
    """list lengths 0, 1, 2, 3 and 5 in one launch; with a dense range the tile with the empty list reads the dense range alone, without
    one its rows are zero"""
    run_plan(ops, "ragged", N + n_dense, (N, N + n_dense), H, cls)


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("H", [1, 3])
def test_tiles_without_keys_get_zero_rows(ops, H, cls):
    run_plan(ops, "empty", N, (N, N), H, cls)


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("H", [1, 3])
def test_multiplicity(ops, H, cls):
    """a tile twice in one list and a dense range (0, 70) over image rows: those keys count twice"""
    once = []
    run_plan(ops, "twice", N, (0, 70), H, cls, once_ratio=once)
    assert once
    if cls == "peaked" and H == 1:
        print(f"tile attention, multiplicity: the reference that counts every key once is off by {max(once):.3g} x the bound")
        assert max(once) > 1.0, "counting the doubled keys once is inside the bound: the case cannot tell the two readings apart"


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("H", [1, 3])
def test_arbitrary_permutation(ops, H, cls):
    run_plan(ops, "shuffled", N + 65, (N, N + 65), H, cls)


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("dense", [(N + 3, N + 68), (N, N)], ids=["65-keys-from-n_img+3", "empty"])
def test_dense_range_elsewhere_and_more_keys_than_queries(ops, dense, H, cls):
    run_plan(ops, "shuffled", N + 70, dense, H, cls)


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("H", [1, 3])
def test_keys_outside_the_key_set_leave_no_trace(ops, H, cls):
    """NaN in the k / v rows of the tiles in nobody's list, between n_img and dense_lo and behind dense_hi"""
    run_plan(ops, "unlisted", N + 70, (N + 3, N + 68), H, cls, poison=True)


@pytest.mark.parametrize("cls", CLASSES)
def test_one_list_per_head_of_different_lengths(ops, cls):
    run_plan(ops, "per-head", N + 65, (N, N + 65), 3, cls)
    run_plan(ops, "per-head", N, (N, N), 3, cls)               # head 1 of tile 3 and head 2 of tile 0: zero rows, the other heads not


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("scale", [0.2, 0.03])
def test_scale(ops, scale, cls):
    run_plan(ops, "ragged", N + 65, (N, N + 65), 3, cls, scale=scale)


def test_no_queries_with_a_plan_that_is_not_null(ops):
    """n_q = 0 at the C ABI: HV_OK, nothing done.  A zero-row view has a null data pointer, which the ABI refuses before it looks at n_q, so
    the call hands over the whole buffers and says n_q = 0 (the host never launches for s_img = 0)"""
    from hunyuanvideo_efficiency_amd import _lib
    buf = torch.ones(70, 3 * D, dtype=torch.bfloat16, device=DEV)
    out = torch.full((8, D + 64), 7.0, dtype=torch.bfloat16, device=DEV)
    plan = TP.empty_plan(DEV)
    _lib.call("attn_fwd_tile_bf16", buf[:, :D], buf[:, D:2 * D], buf[:, 2 * D:], out[:, :D], buf.stride(0), buf.stride(0), buf.stride(0),
              out.stride(0), 0, 70, 1, 128, 128 ** -0.5, plan.perm, plan.tile_start, plan.n_tiles, plan.nb_ptr, plan.nb_idx, plan.n_lists, 0, 70)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
