"""TEST INFRASTRUCTURE: tile plans for the sliding-tile attention of include/hv_attn_tile.h that do NOT come from ops.tile_plan, and the
key sets they stand for, restated from the hand-written lists (never read back from the plan tensors the kernel consumes).

  allowed(grid, tile, window)                the window of ops.tile_plan restated from index arithmetic: may query i see key j
  hand_plan(perm, sizes, lists, device)      explicit perm, tile sizes and neighbour lists -> ops.TilePlan, held to the header's rules first
  key_rows(perm, sizes, lst, dense)          the key rows of one tile's list WITH multiplicity, list order then dense order
  PLANS                                      the hand-built plans of tests/test_gpu_attn_tile_plans.py and tests/double_parity.py"""
import torch

from hunyuanvideo_efficiency_amd import synthetic as syn
from hunyuanvideo_efficiency_amd.attn_tile import ATTN_TILE, TilePlan


def allowed(grid, tile, window):
    """-> ([n_img, n_img] bool: may query i see key j, [n_img] tile id of each token), tokens in (t, h, w) raster order"""
    g, tl, w = torch.tensor(grid), torch.tensor(tile), torch.tensor(window)
    tc = torch.stack(torch.meshgrid(*[torch.arange(x) for x in grid], indexing="ij"), -1).reshape(-1, 3) // tl
    nt = -(-g // tl)
    n = torch.minimum(w, nt)                                   # tiles per axis actually attended
    lo = torch.minimum((tc - w // 2).clamp(min=0), nt - n)     # the window starts w // 2 before the tile, pushed back inside the grid
    ok = ((tc[None] >= lo[:, None]) & (tc[None] < (lo + n)[:, None])).all(-1)
    return ok, (tc[:, 0] * nt[1] + tc[:, 1]) * nt[2] + tc[:, 2]


def hashed_perm(n, key):
    """a permutation of [0, n) from hashed uniforms: the tokens of a tile scattered over the sequence, not increasing within a tile"""
    return torch.argsort(syn.hashed_uniform((n,), "tileplan." + key, 31), stable=True).tolist()


def slots(sizes, t):
    lo = sum(sizes[:t])
    return range(lo, lo + sizes[t])


def key_rows(perm, sizes, lst, dense, once=False):
    """rows of k / v the queries of a tile with neighbour list `lst` attend: the rows of each listed tile in slot order, in list order,
    then the dense range in natural order - a tile listed twice and a dense row that is also an image row appear twice.  once=True is
    the WRONG reading (every row at most once), kept to show that a case can tell the two apart."""
    rows = [perm[s] for t in lst for s in slots(sizes, t)] + list(range(dense[0], dense[1]))
    return list(dict.fromkeys(rows)) if once else rows


def validate(perm, sizes, lists, n_heads=None):
    """the rules of include/hv_attn_tile.h a producer owes the kernel (which trusts the arrays like pointers)"""
    n_q, n_tiles = len(perm), len(sizes)
    assert sorted(perm) == list(range(n_q)), "perm is not a permutation of [0, n_q)"
    assert n_tiles >= 1 and sum(sizes) == n_q and all(1 <= c <= ATTN_TILE["HV_ATTN_TILE_BM"] for c in sizes), sizes
    assert len(lists) >= 1 and (n_heads is None or len(lists) in (1, n_heads)), len(lists)
    for per_tile in lists:
        assert len(per_tile) == n_tiles, "one neighbour list per tile"
        assert all(0 <= t < n_tiles for lst in per_tile for t in lst), "a list names a tile that does not exist"
    assert sum(len(lst) for per_tile in lists for lst in per_tile) < 2 ** 31


def hand_plan(perm, sizes, lists, device) -> TilePlan:
    """perm [n_q], sizes [n_tiles], lists [n_lists][n_tiles] -> list of tile ids (n_lists = 1: shared by the heads)"""
    validate(perm, sizes, lists)
    n_q, n_tiles = len(perm), len(sizes)
    start, ptrs, idx = [0], [], []
    for c in sizes:
        start.append(start[-1] + c)
    for per_tile in lists:
        row = [len(idx)]
        for lst in per_tile:
            idx += lst
            row.append(len(idx))
        ptrs.append(row)
    pairs = sum(sizes[i] * sizes[t] for per_tile in lists for i, lst in enumerate(per_tile) for t in lst)
    dev = lambda x: torch.tensor(x, dtype=torch.int32).to(device)
    return TilePlan(dev(perm), dev(start), dev(ptrs), dev(idx + [0]), n_q, n_tiles, len(lists),       # one unreferenced entry: nb_idx is never null
                    pairs / (len(lists) * float(n_q) ** 2), (0, 0, 0), (0, 0, 0), ())


def empty_plan(device) -> TilePlan:
    """a plan for n_q = 0 whose four pointers are not null (an empty tensor has a null data pointer: perm keeps one unread entry)"""
    z = lambda n: torch.zeros(n, dtype=torch.int32, device=device)
    return TilePlan(z(1), z(2), z(2).view(1, 2), z(1), 0, 1, 1, 0.0, (0, 0, 0), (0, 0, 0), ())


# tile ids:  0 = 65 tokens (a one-key last chunk), 1 = one token, 2 = 63, 3 = 64, 4 = 256
SIZES = [65, 1, 63, 64, 256]
N = sum(SIZES)
IDENT = list(range(N))
# list lengths 0, 1, 2, 3, 5: the 65-token tile alone, last, first and in the middle of a list; the 1-token tile first, in the middle and last
RAGGED = [[[], [0], [1, 0], [0, 1, 2], [3, 0, 4, 2, 1]]]
PLANS = {
    "ragged": (IDENT, SIZES, RAGGED),
    # tiles 0, 2 and 4 (65, 63 and 256 queries: one, one and four waves) attend nothing
    "empty": (IDENT, SIZES, [[[], [1], [], [0, 2], []]]),
    # a tile twice in one list, next to a tile listed once (doubling EVERY key of a row would change nothing)
    "twice": (IDENT, SIZES, [[[1, 0, 1], [0, 0, 3], [2, 3, 3], [4, 1, 4], [0, 2, 2, 1]]]),
    "shuffled": (hashed_perm(N, "shuffled"), SIZES, RAGGED),
    # tiles 2 and 4 are in nobody's list
    "unlisted": (hashed_perm(N, "unlisted"), SIZES, [[[0], [3, 1], [1, 0, 3], [], [3, 0, 1]]]),
    # one list per head, of different lengths per head; head 1 of tile 3 and head 2 of tile 0 attend no tile
    "per-head": (hashed_perm(N, "per-head"), SIZES, [RAGGED[0], [[4], [1, 1, 0], [2], [], [0, 3]], [[], [4, 2, 0, 3], [1], [3, 1, 2], [4]]]),
}
