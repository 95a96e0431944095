"""fp64 reference of the attention kernel's arithmetic contract (csrc/hv_attention_w4.hip, one head of 128 dims at a time) and a
per-element error bound for its bf16 output, its fp32 partials (part_o, m, l) and the merge of partials.  The companion of
tests/error_bounds.py (its C, EPS32, ulp_out and Ref are reused).

Contract: the kernel multiplies q' = bf16(fp32(q) * fp32(scale * log2 e)) - ONE fp32 multiply, then round-to-nearest-even - with k,
so the reference uses q', not q and not the oracle's rounding points (log2 domain throughout):

    s_j = q' . k_j        w_j = 2^(s_j - M) / sum_j 2^(s_j - M)  (M = max_j s_j)        O64 = sum_j w_j v_j       L64 = M + log2 sum_j 2^(s_j - M)

Bound on the bf16 output, element d of a row - every term from what the kernel does, none fitted to its output:

    |O - O64|_d <= ulp_bf16(O64_d)                          the final rounding (EB.ulp_out)
                 + P-term                                   P = 2^(s - m) is rounded to bf16 for P.V, the row sum l is not
                 + sum_j eta_j w_j |v_jd - O64_d|           a relative error of p_j that numerator and row sum share
                 + C sqrt(n_kv) 2^-24 (||(w_j v_jd)_j||_2 + 2 |O64_d|)      fp32 accumulation of P.V and of l, any key order

  * eta_j = ln 2 * bs_j + 2^-22: bs_j is the EB.Ref bound of the 128-term fp32 score chain, C sqrt(128) 2^-24 (||(q'_c k_jc)_c||_2 +
    |s_j - m| + |m|) - the maximum m sits in the C operand of the chain, so its partial sums are of size |m| + |s|; |m - M| <= gap
    (8 = the deferred-max threshold THR; the static row bound can sit up to 90 above M, a KV split's halves have their own maxima:
    the caller passes the gap).  2^-22 covers v_exp_f32.
  * P-term: 2^-8 sum_j w_j |v_jd|, the worst case over the bf16 roundings (half an ulp of every p_j, all aligned).  Decided on the
    CPU emulation of tests/test_attention_bounds_cpu.py alone: with it a faithful kernel sits at 0.3-0.4 of the bound on `random`,
    `peaked` and `phantom` data (scores of standard deviation 2 leave ~100 effective keys of 737, so the roundings' sqrt(n)
    cancellation is worth only ~2x) and every mutant there is rejected, so the worst case stays.  p_form="stat" is the statistical
    alternative min(worst, C 2^-8 / sqrt 3 * ||(w_j v_jd)_j||_2) (C = 4 as in error_bounds.py), kept for that comparison only.

Partials (hv_attn_partial_bf16: part_o fp32 unnormalised, m, l):  part_o / l within the same bound without the final rounding;
m + log2 l within sum_j w_j bs_j + (2^-22 + C sqrt(n_kv) 2^-24) / ln 2 of L64;  M - 8 - eps <= m <= M + eps with eps = 2 max_j bs_j +
2^-23 |M| (m is tile 0's row max plus the increments d = fp32 score - m of the rescales: within two score errors of a true score).

Data classes (make_case; deterministic, syn.hashed_uniform): `random` (log2-domain scores of standard deviation ~2), `peaked` (one
dominant key per row, ~2^14 above the rest, in tile 0 / in the last full tile / at the last valid key, by row % 3), `flat` (q = 0:
every p is exactly 1) and `phantom` (q and k carry opposite common components: every real score ~ -60, so a key read as zeros
behind n_kv - score 0 - would own the row)."""
from __future__ import annotations

import math

import torch

from hunyuanvideo_efficiency_amd import synthetic as syn
from tests import error_bounds as EB

D = 128
KVT = 64
THR = 8.0
LN2 = math.log(2.0)
BF16 = torch.bfloat16
CLASSES = ("random", "peaked", "flat", "phantom")


def scale_log2e(scale=None) -> float:
    """fp32(scale) * fp32(log2 e) in fp32: AttnArgs::scale_log2e"""
    s = torch.tensor(D ** -0.5 if scale is None else scale, dtype=torch.float32)
    return float(s * torch.tensor(1.4426950408889634, dtype=torch.float32))


def q_prime(q: torch.Tensor, scale=None) -> torch.Tensor:
    """bf16(fp32(q) * scale_log2e): one fp32 multiply (the factor is an fp32 value: exact as a Python float), then RNE to bf16"""
    return (q.float() * scale_log2e(scale)).to(BF16)


def static_row_bound(q: torch.Tensor, k: torch.Tensor, scale=None) -> torch.Tensor:
    """the kernel's static maximum per row of one head: |q'| max_j |k_j| * 1.001 + 1e-3 (fp64 here: an upper bound of its |m|)"""
    qn = q_prime(q, scale).double().norm(dim=1)
    return qn * k.double().norm(dim=1).max() * 1.001 + 1e-3


def peak_positions(n_kv: int):
    """keys of the `peaked` class: one in tile 0, one in the last FULL tile, the last valid key (distinct, ascending)"""
    full = n_kv // KVT                         # number of full tiles
    pos = {min(5, n_kv - 1), n_kv - 1}
    if full >= 1:
        pos.add(min(KVT * (full - 1) + 37, n_kv - 1))
    return sorted(pos)


def make_case(cls: str, n_q: int, n_kv: int, H: int, key: str, device="cpu"):
    """q [n_q, H*128], k, v [n_kv, H*128] bf16 of one data class"""
    u = lambda shape, name, s=1.0: syn.hashed_uniform(shape, f"ab.{key}.{cls}.{name}", 29, device) * (s * math.sqrt(3.0))
    q, k, v = u((n_q, H, D), "q", 1.39), u((n_kv, H, D), "k"), u((n_kv, H, D), "v")
    if cls == "flat":
        q = torch.zeros_like(q)
    elif cls == "peaked":
        pos = peak_positions(n_kv)
        rows = torch.arange(n_q, device=device)
        for i, p in enumerate(pos):
            dirn = torch.zeros(D, device=device)
            dirn[32 * i:32 * i + 32] = 1.0 / math.sqrt(32.0)
            k[p] = 16.0 * dirn                                       # score of an assigned row: 16 * 11.76 * 0.1275 = 24 (log2 domain)
            q[rows % len(pos) == i] += 11.76 * dirn
    elif cls == "phantom":
        u0 = torch.full((D,), 1.0 / math.sqrt(D), device=device)
        q = q + 21.7 * u0                                            # common score -21.7^2 * 0.1275 = -60
        k = k - 21.7 * u0
    elif cls != "random":
        raise ValueError(cls)
    return q.reshape(n_q, H * D).to(BF16), k.reshape(n_kv, H * D).to(BF16), v.reshape(n_kv, H * D).to(BF16)


def kernel_gap(q, k, H, cuts=(), static=False, scale=None) -> torch.Tensor:
    """[n_q, H]: an upper bound of |m - M| over every pass the kernel makes.  The key range is cut at `cuts` (the halves of a KV split,
    the chunks of a ring); a pass over range R keeps m in [M_R - 8, M_R] (online) or at the static row bound, which lies in
    [M_R, M_R + 90]; M_R <= M.  So |m - M| <= max_R (M - M_R) + 8 (+ 90 where the static mode can run)."""
    edges = [0] + [c for c in cuts if 0 < c < k.shape[0]] + [k.shape[0]]
    gaps = []
    for h in range(H):
        s = q_prime(q[:, h * D:(h + 1) * D], scale).double() @ k[:, h * D:(h + 1) * D].double().T
        m_r = torch.stack([s[:, a:b].max(dim=1).values for a, b in zip(edges[:-1], edges[1:])])
        gaps.append(s.max(dim=1).values - m_r.min(dim=0).values + THR + (90.0 if static else 0.0))
    return torch.stack(gaps, 1)


def _eta_term(we: torch.Tensor, v: torch.Tensor, o: torch.Tensor) -> torch.Tensor:
    """sum_j we[i, j] |v[j, d] - o[i, d]|, a block of rows at a time"""
    out = torch.empty_like(o)
    step = max(1, (1 << 23) // (v.shape[0] * D))
    for r0 in range(0, o.shape[0], step):
        dev = (v[None] - o[r0:r0 + step, None]).abs()
        out[r0:r0 + step] = torch.bmm(we[r0:r0 + step, None], dev)[:, 0]
    return out


class HeadRef:
    """one head: q [n_q, 128], k, v [n_kv, 128] (bf16 values, any device).  gap: upper bound of |m - M| per row (scalar or [n_q])."""

    def __init__(self, q, k, v, scale=None, gap=THR, rounded_q=True, p_form="worst"):
        qd = q_prime(q, scale).double() if rounded_q else q.double() * scale_log2e(scale)
        kd, vd = k.double(), v.double()
        n_kv = k.shape[0]
        sref = EB.Ref().add(qd, kd)
        s = sref.y
        self.M = s.max(dim=1).values
        e = torch.exp2(s - self.M[:, None])
        z = e.sum(dim=1)
        w = e / z[:, None]
        self.O = w @ vd
        self.L = self.M + torch.log2(z)
        gap = torch.as_tensor(gap, dtype=torch.float64, device=s.device).expand(s.shape[0])
        bs = EB.C * math.sqrt(D) * EB.EPS32 * (sref.sq.sqrt() + (s - self.M[:, None]).abs() + (self.M.abs() + 2.0 * gap)[:, None])
        eta = LN2 * bs + 2.0 ** -22
        l2 = ((w * w) @ (vd * vd)).sqrt()
        worst = 2.0 ** -8 * (w @ vd.abs())
        stat = EB.C * 2.0 ** -8 / math.sqrt(3.0) * l2
        self.p_term = {"worst": worst, "stat": torch.minimum(worst, stat)}[p_form]
        self.eta_term = _eta_term(eta * w, vd, self.O)
        self.acc_term = EB.C * math.sqrt(n_kv) * EB.EPS32 * (l2 + 2.0 * self.O.abs())
        self.tol_L = (w * bs).sum(dim=1) + (2.0 ** -22 + EB.C * math.sqrt(n_kv) * EB.EPS32) / LN2
        self.eps_m = 2.0 * bs.max(dim=1).values + 2.0 ** -23 * self.M.abs()

    def bound(self, final=True):
        b = self.p_term + self.eta_term + self.acc_term
        return b + EB.ulp_out(self.O, BF16) if final else b


class AttnRef:
    """H heads: q [n_q, >= H*128] (head h at columns h*128 ..), k, v [n_kv, ..]; gap scalar or [n_q, H]"""

    def __init__(self, q, k, v, H, scale=None, gap=THR, rounded_q=True, p_form="worst"):
        self.H = H
        g = torch.as_tensor(gap, dtype=torch.float64, device=q.device)
        self.heads = [HeadRef(q[:, h * D:(h + 1) * D], k[:, h * D:(h + 1) * D], v[:, h * D:(h + 1) * D], scale,
                              g[:, h] if g.dim() == 2 else g, rounded_q, p_form) for h in range(H)]
        self.O = torch.stack([r.O for r in self.heads], 1)               # [n_q, H, 128]
        self.L = torch.stack([r.L for r in self.heads], 1)               # [n_q, H]
        self.M = torch.stack([r.M for r in self.heads], 1)
        self.tol_L = torch.stack([r.tol_L for r in self.heads], 1)
        self.eps_m = torch.stack([r.eps_m for r in self.heads], 1)

    def bound(self, final=True):
        return torch.stack([r.bound(final) for r in self.heads], 1)

    def ratio_o(self, got, final=True):
        """|got - O64| / bound per element, got [n_q, H*128] or [n_q, H, 128] (inf where got is not finite)"""
        g = got.double().reshape(self.O.shape).to(self.O.device)
        err = (g - self.O).abs()
        r = torch.where(err == 0, torch.zeros_like(err), err / self.bound(final))
        return torch.where(torch.isfinite(g), r, torch.full_like(r, math.inf))

    def check_o(self, got, what="", final=True) -> float:
        r = self.ratio_o(got, final)
        worst = float(r.max())
        if not worst <= 1.0:
            bad = (r > 1.0).nonzero()
            i, h, d = (int(x) for x in bad[r[r > 1.0].argmax()])
            raise AssertionError(f"{what}: {bad.shape[0]} of {r.numel()} elements outside the fp64 error bound (worst ratio {worst:.3g} at "
                                 f"row {i} head {h} dim {d}: got {float(got.reshape(self.O.shape)[i, h, d])}, O64 {float(self.O[i, h, d]):.9g}); "
                                 f"rows [{int(bad[:, 0].min())}, {int(bad[:, 0].max())}]")
        return worst

    def check_partial(self, part_o, ml, what="") -> float:
        """part_o [n_q, H, 128] fp32 unnormalised, ml [n_q, H, 2] = (m, l): the three checks of the module docstring"""
        m, l = ml[..., 0].double().to(self.O.device), ml[..., 1].double().to(self.O.device)
        assert bool(torch.isfinite(m).all()) and bool((l > 0).all()) and bool(torch.isfinite(l).all()), f"{what}: (m, l) not finite / positive"
        lo, hi = self.M - THR - self.eps_m, self.M + self.eps_m
        ok = (m >= lo) & (m <= hi)
        if not bool(ok.all()):
            i, h = (int(x) for x in (~ok).nonzero()[0])
            raise AssertionError(f"{what}: m outside [rowmax - 8, rowmax] for {int((~ok).sum())} rows, e.g. row {i} head {h}: m {float(m[i, h])}, "
                                 f"rowmax {float(self.M[i, h]):.9g}")
        rl = ((m + torch.log2(l)) - self.L).abs() / self.tol_L
        if not float(rl.max()) <= 1.0:
            i, h = divmod(int(rl.reshape(-1).argmax()), self.H)
            raise AssertionError(f"{what}: m + log2 l off by {float(rl.max()):.3g} x its tolerance at row {i} head {h}: "
                                 f"{float(m[i, h] + torch.log2(l[i, h])):.9g} vs L64 {float(self.L[i, h]):.9g}")
        return self.check_o(part_o.double().to(self.O.device) / l[..., None], what + " part_o / l", final=False)


def merge_ref(part_o, ml):
    """fp64 merge of slots part_o [S, n_q, H, 128], ml [S, n_q, H, 2] and the bound of attn_combine_kernel's fp32 arithmetic on THESE
    partials: the final rounding + the v_exp_f32 error of each weight and a few fp32 roundings per term (2^-21 of the terms' size)"""
    o, m, l = part_o.double(), ml[..., 0].double(), ml[..., 1].double()
    w = torch.exp2(m - m.max(dim=0).values)
    den = (l * w).sum(dim=0)
    y = (o * w[..., None]).sum(dim=0) / den[..., None]
    size = (o.abs() * w[..., None]).sum(dim=0) / den[..., None]
    return y, EB.ulp_out(y, BF16) + 2.0 ** -21 * size


def merge_ratio(got, part_o, ml):
    y, b = merge_ref(part_o, ml)
    g = got.double().reshape(y.shape).to(y.device)
    r = (g - y).abs() / b
    return torch.where(torch.isfinite(g), r, torch.full_like(r, math.inf))
