"""TEST INFRASTRUCTURE: the rule of include/hv_attn_select.h restated in float64 from the bf16 inputs, written from the header - the
ranking, the cut, and for every score the fp32 error bound from absolute sums (in the manner of tests/error_bounds.py), carried through
exp2 and the mass sums to every comparison at the cut.  With u = 2^-24 and A_ij = |sl2| * (mean|q|_i . mean|k|_j):
  |ds_ij| <= u * ((c_i + c_j + 136) * A_ij + 4 * (|s_ij| + log2 c_j))   c_i + c_j roundings in the two means (sums and the division), 128
                                                                        in the dot product, the final fma, an approximate log2 (2 ulp)
  rho_ij  =  ln 2 * (ds_ij + max_j ds_ij + u * |s_ij - max|) + 4 u      relative error of exp2(s - max) up to a factor common to the row:
                                                                        its own score, the row maximum's, the subtraction, exp2 (2 ulp)
  a mass over a set: sum p rho + 24 u * mass                            16 sequential adds per lane and a 6-step butterfly, terms >= 0
A comparison is decided when the float64 values differ by more than the bounds of both sides."""
import functools

import numpy as np
import torch

from hunyuanvideo_efficiency_amd.attn_tile import tile_plan

U = 2.0 ** -24
D = 128


def make_inputs(grid, tile, H, extra_rows=0, spread=1.5):
    """q, k (and v) as views into one fused bf16 buffer with padded strides: tile centres * spread + unit noise, so that the pooled scores
    spread over several units; `extra_rows` plain random rows behind the image (a dense range).  Deterministic."""
    base = tile_plan(grid, tile, (1, 1, 1), "cpu")
    g = torch.Generator().manual_seed(1000 * base.n_tiles + 10 * H + extra_rows)
    tile_of = torch.empty(base.n_img, dtype=torch.long)
    tile_of[base.perm.long()] = torch.repeat_interleave(torch.arange(base.n_tiles), base.tile_start.diff().long())
    buf = torch.randn(base.n_img + extra_rows, 3 * H * D + 24, generator=g)
    buf[:base.n_img, :2 * H * D] += spread * torch.randn(2, base.n_tiles, H * D, generator=g)[:, tile_of].permute(1, 0, 2).reshape(base.n_img, -1)
    return base, buf.to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def pooled(grid, tile, H, scale=None):
    """-> base plan, fused buffer, and per head the float64 p [nt, nt], rho [nt, nt], counts c - shared by every (cdf, k_min, k_max) case"""
    base, buf = make_inputs(grid, tile, H)
    sl2 = float(np.float32(np.float32(D ** -0.5 if scale is None else scale) * np.float32(1.4426950408889634)))
    c = base.tile_start.diff().double().numpy()
    rows = [base.perm[a:b].long() for a, b in zip(base.tile_start[:-1], base.tile_start[1:])]
    heads = []
    for h in range(H):
        q, k = (buf[:base.n_img, o + h * D:o + (h + 1) * D].double() for o in (0, H * D))
        qm, km, qa, ka = (np.stack([x[r].mean(0).numpy() for r in rows]) for x in (q, k, q.abs(), k.abs()))
        s = sl2 * (qm @ km.T) + np.log2(c)[None, :]
        ds = U * ((c[:, None] + c[None, :] + 136) * abs(sl2) * (qa @ ka.T) + 4 * (np.abs(s) + np.log2(c)[None, :]))
        mx = s.max(1, keepdims=True)
        p = np.exp2(s - mx)
        rho = np.log(2.0) * (ds + ds.max(1, keepdims=True) + U * np.abs(s - mx)) + 4 * U
        heads.append((p / p.sum(1, keepdims=True), rho))
    return base, buf, heads, c


def cut(p, rho, i, cdf, k_min, k_max):
    """row i of one head (p, rho: its nt entries) -> (list, decided, ranking, clamps): the rule, and whether fp32 could have decided otherwise"""
    nt = p.shape[0]
    key = p.copy()
    key[i] = np.inf
    order = np.argsort(-key, kind="stable")                    # p descending, tile index ascending, own tile first
    po, ro = p[order], rho[order]
    cum, err_l = np.cumsum(po), float((p * rho).sum()) + 24 * U
    err = np.cumsum(po * ro) + 24 * U * cum + cum * err_l + 8 * U   # bound of (mass of the first n) / (sum of all) as the kernel forms it
    lo_c, hi_c = min(k_min, nt), min(nt if k_max is None else k_max, nt)
    if cdf >= 1.0:
        n_lo = n_hi = n = nt
    else:
        first = lambda ok: int(np.argmax(ok)) + 1 if ok.any() else nt
        n, n_lo, n_hi = first(cum >= cdf), first(cum + err >= cdf), first(cum - err >= cdf)
    clamp = lambda x: min(max(x, lo_c), hi_c)
    n, decided = clamp(n), clamp(n_lo) == clamp(n_hi)
    if decided and 2 <= n < nt:                                # the last kept against the first dropped (the own tile is never compared)
        decided = po[n - 1] * (1 - ro[n - 1]) > po[n] * (1 + ro[n])
    return sorted(order[:n].tolist()), bool(decided), order, (lo_c, hi_c)


def mass_and_bound(p, rho, lst):
    """row-wise: the float64 pooled mass of a list and the bound of the kernel's kept_mass for it"""
    lst = np.asarray(lst)
    m = float(p[lst].sum())
    return m, float((p[lst] * rho[lst]).sum()) + 24 * U * m + m * (float((p * rho).sum()) + 24 * U) + 8 * U
