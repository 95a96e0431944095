"""TEST INFRASTRUCTURE: the sequence-parallel path as a COMPOSITION - cases, device-agnostic checks and mutants for the host layer
that moves tokens and heads between ranks (long_ctx_attention.UlyssesLongContextAttention, _sp_chunked_qkv and the segment loops of
modules/models.py, inference.parallelize_transformer_module).  The same rank worker runs on the CPU kernel doubles under gloo
(tests/test_sp_wiring_gloo.py, where every mutant below must be rejected by the check named for it) and on the HIP kernels with the
ranks sharing one card (tests/test_gpu_sp_wiring.py).  The exchange is pure data movement, so almost everything is asserted bit for bit.

Part 1 - the attention object against a single-rank replay.  q, k, v [s_img + n_j, H*128] are built identically on every rank
(attention_bounds.make_case); a rank's operands are the column blocks of ONE fused buffer (row stride 3 H 128 + 8) inside NaN-filled
memory, its output a [s_loc + n_j, H*128] view of a wider sentinel-filled buffer.  The replay is plain torch indexing - the tokens of
the rank's Ulysses group in rank order, joint rows at the rear, the columns of one head group - followed by the SAME kernel calls on
buffers of the same shape and stride: attn_fwd, or for a ring attn_partial per chunk in the order the rank sees them (local chunk
with the joint keys, then ring ranks rr-1, rr-2, ... without) with the splits attn_suggest_splits gives, then attn_merge.
  A1 run        the object returns (no exception)
  A1 operands   qf / kf / vf of the object == the replay's, bit for bit
  A1 partials   ring: every partial slot (o, ml) == the replay's, bit for bit
  A1 output     the output rows (local image rows, text rows, every head group) == the replays of the group's ranks, bit for bit; no
                NaN in it, every sentinel around it and every NaN around the operands keeps its bits
  A1 segments   attend_async: the returned row ranges tile [0, s_loc + n_j) and, right after a segment's finish(), its rows are final
  A2 fp64       the replay within the per-element fp64 bound of attention_bounds.AttnRef over the concatenated keys in the rank's
                order (cuts at the chunk and split boundaries)
  A3 census     ring, q = 0 and integer v: every slot holds the integer column sums of its chunk, m = 0, l = the chunk's key count,
                and over a rank's slots sum l = s_img + n_j - each key once, the joint keys only with the local chunk
The `flat` data class (q = 0) is left to A3: with it every query row is the same, so A1 could not see a mis-placed row.

Part 2 - the sharded model, stage by stage (d = 512, 4 heads, 1 + 2 blocks), traced with dit_wiring.traced on every rank.
  B1  every block's output (the rank's image rows and its text rows) against the oracle block on that block's own input - the image
      rows of all ranks gathered into the unsharded token order, the rank's own text rows - at dit_wiring's block tolerance; the
      gathered output against the oracle's final layer on the gathered input
  B2  after every block the text rows of the residual stream are bit-equal on the ranks of a Ulysses group.  Across ring ranks they
      need not be: the text queries of ring rank rr meet the key chunks in the order rr, rr-1, ..., another summation order in the
      merge, so across ring ranks the text rows are only held to B1
  B3  other content in the padding text rows changes no bit of the sharded output
A check records its failure and the rank goes on: it takes part in every remaining collective, so a failure cannot hang its peers."""
from __future__ import annotations

import contextlib
import dataclasses
import datetime
import json
import os
import sys
import traceback
import types
from typing import Optional

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16
D = 128
NAN16, SENT16 = 0x7FFF, 0x7E5A
TIMEOUT = datetime.timedelta(seconds=60)


# ------------------------------------------------------------------------------------------------------------------ kernels
class Kit:
    """the kernel set of one device: the HIP kernels, or the CPU doubles of tests/"""

    def __init__(self, device: str):
        self.dev = torch.device(device)
        self.gpu = self.dev.type == "cuda"
        if self.gpu:
            from hunyuanvideo_efficiency_amd import ops
            from hunyuanvideo_efficiency_amd.long_ctx_attention import _HipKernels
            self.K, self.qknorm_rope_, self.ops = _HipKernels, ops.qknorm_rope_, ops
        else:
            from tests import cpu_kernel_doubles as KD
            from tests.test_ulysses_gloo import CpuKernelDouble
            self.K, self.qknorm_rope_, self.ops = CpuKernelDouble, KD.qknorm_rope_, None


class Log:
    """failures of one rank, by check name; ratios error / bound by path"""

    def __init__(self):
        self.failures = []
        self.ratios = {}

    def check(self, name: str, where: str, fn):
        try:
            fn()
            return True
        except AssertionError as e:
            self.failures.append(f"{name}: {where}: {e}")
        except Exception as e:  # noqa: BLE001 - a check that cannot even run has failed
            self.failures.append(f"{name}: {where}: raised {type(e).__name__}: {e}")
        return False

    def ratio(self, path: str, r: float):
        self.ratios[path] = max(self.ratios.get(path, 0.0), float(r))


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def n_bits_differ(a: torch.Tensor, b: torch.Tensor) -> str:
    if a.shape != b.shape:
        return f"shapes {tuple(a.shape)} / {tuple(b.shape)}"
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    ne = a.contiguous().view(it) != b.contiguous().view(it)
    rows = ne.reshape(ne.shape[0], -1).any(1).nonzero().reshape(-1)
    return f"{int(ne.sum())} of {ne.numel()} elements differ, rows [{int(rows.min())}, {int(rows.max())}]" if rows.numel() else "equal"


def make_groups(U: int, R: int):
    """(ulysses group, ring group) of this rank in the layout of inference.set_sequence_parallel_groups; every rank creates every
    group in the same order.  R = 1: (None, None) - the WORLD group is the Ulysses group."""
    if R == 1:
        return None, None
    rank, ug, rg = dist.get_rank(), None, None
    for i in range(R):
        ranks = list(range(i * U, (i + 1) * U))
        g = dist.new_group(ranks, timeout=TIMEOUT)
        ug = g if rank in ranks else ug
    for j in range(U):
        ranks = list(range(j, U * R, U))
        g = dist.new_group(ranks, timeout=TIMEOUT)
        rg = g if rank in ranks else rg
    return ug, rg


# ================================================================================================================== Part 1
@dataclasses.dataclass(frozen=True)
class Run:
    """one way of driving the object: surface "call" | "fused" | "async"; for "async" the exchange variant, and how pack_dst is
    filled when scatter_pack is on ("copy": plain torch; "qknorm": qknorm_rope_(out=pack_dst) for q and k)"""
    surface: str
    nseg: int = 1
    out_exchange: str = "a2a"
    scatter_pack: bool = False
    fill: str = "copy"

    @property
    def name(self) -> str:
        if self.surface != "async":
            return self.surface
        return f"async-nseg{self.nseg}-{self.out_exchange}" + (f"-pack.{self.fill}" if self.scatter_pack else "")


CALL, FUSED = Run("call"), Run("fused")
ASYNC = Run("async")
ALL_RUNS = (CALL, FUSED, ASYNC, Run("async", 2, "a2a"), Run("async", 3, "a2a"), Run("async", 2, "p2p"), Run("async", 3, "p2p"),
            Run("async", 2, "a2a", True, "copy"), Run("async", 3, "p2p", True, "qknorm"))


@dataclasses.dataclass(frozen=True)
class Geo:
    U: int
    R: int
    H: int
    s_loc: int
    n_j: int
    cls: str = "random"
    runs: tuple = (CALL, FUSED, ASYNC)
    long: bool = False              # HIP kernels only: the chunks are long enough for the KV split

    @property
    def world(self) -> int:
        return self.U * self.R

    @property
    def s_img(self) -> int:
        return self.world * self.s_loc

    @property
    def s_u(self) -> int:
        return self.U * self.s_loc

    @property
    def hp(self) -> int:
        return self.H // self.U

    @property
    def w(self) -> int:
        return self.hp * D

    @property
    def name(self) -> str:
        return f"U{self.U}xR{self.R}-H{self.H}-sloc{self.s_loc}-nj{self.n_j}-{self.cls}"


# one value of each edge, not their product: s_loc 1 / 63 / 64 / 65; n_j 0 / 1 / 11 / 64 (U s_loc + n_j below, on and above a 64-key
# tile: 127, 128, 129, ...); P 2 / 3 / 4 / 8 (H = 24 at 8: 3 heads per rank); hp odd and even; an odd H through run_fused; nseg 1 / 2 /
# 3 with s_loc not divisible, a2a and p2p; pack_dst filled by a copy and by qknorm_rope_; hybrid (1,2), (1,3), (2,2); two long cases
GEOS = [
    Geo(2, 1, 2, 1, 0, "random"),
    Geo(2, 1, 4, 63, 1, "peaked", ALL_RUNS),
    Geo(2, 1, 2, 64, 0, "phantom", (CALL, FUSED, Run("async", 3, "p2p"))),
    Geo(2, 1, 6, 65, 11, "random", (CALL, FUSED, Run("async", 2, "a2a", True, "qknorm"), Run("async", 3, "p2p", True, "copy"))),
    Geo(1, 2, 2, 65, 11, "peaked", (CALL, FUSED, ASYNC)),
    Geo(1, 2, 1, 64, 64, "random", (CALL, FUSED)),
    Geo(1, 2, 2, 63, 0, "phantom", (CALL, ASYNC)),
    Geo(2, 1, 2, 2048, 11, "random", (FUSED, Run("async", 2, "p2p", True, "copy")), long=True),
    Geo(1, 2, 1, 4096, 11, "random", (FUSED,), long=True),
    Geo(3, 1, 3, 64, 1, "phantom", (CALL, FUSED)),
    Geo(3, 1, 6, 65, 64, "random", (FUSED, Run("async", 3, "a2a"), Run("async", 2, "p2p", True, "qknorm"))),
    Geo(1, 3, 2, 63, 11, "random", (CALL, FUSED, ASYNC)),
    Geo(4, 1, 4, 63, 11, "peaked", ALL_RUNS),
    Geo(4, 1, 8, 1, 64, "random", (CALL, FUSED, Run("async", 2, "p2p"))),
    Geo(2, 2, 2, 64, 1, "phantom", (CALL, FUSED, Run("async", 2, "a2a"))),
    Geo(2, 2, 4, 65, 0, "peaked", (FUSED, Run("async", 3, "p2p", True, "copy"), Run("async", 2, "a2a", True, "qknorm"))),
    Geo(8, 1, 24, 65, 11, "random", (CALL, FUSED, Run("async", 3, "p2p", True, "qknorm"), Run("async", 2, "a2a"))),
]
WORLDS = sorted({g.world for g in GEOS})


def geos_of(world: int, gpu: bool):
    return [g for g in GEOS if g.world == world and (gpu or not g.long)]


class Local:
    """this rank's rows [local image | joint] of q | k | v as column blocks of one fused buffer, row stride 3 H 128 + 8, inside
    NaN-filled memory (3 rows before, 5 after, 8 columns at the right)"""

    def __init__(self, q, k, v, geo: Geo, g: int, dev, before=3, after=5):
        hd, rows = geo.H * D, geo.s_loc + geo.n_j
        self.ld = 3 * hd + 8
        self.buf = torch.full((before + rows + after, self.ld), NAN16, dtype=torch.int16, device=dev)
        self.mask = torch.ones_like(self.buf, dtype=torch.bool)
        view = self.buf.view(BF16)
        for i, t in enumerate((q, k, v)):
            view[before:before + geo.s_loc, i * hd:(i + 1) * hd] = t[g * geo.s_loc:(g + 1) * geo.s_loc]
            view[before + geo.s_loc:before + rows, i * hd:(i + 1) * hd] = t[geo.s_img:]
        self.mask[before:before + rows, :3 * hd] = False
        self.fused = view[before:before + rows, :3 * hd]
        self.poison = self.buf.clone()

    def chunk(self, c: int, geo: Geo):
        hd = geo.H * D
        return self.fused[:geo.s_loc, c * hd:(c + 1) * hd], self.fused[geo.s_loc:, c * hd:(c + 1) * hd]

    def intact(self) -> bool:
        return bool((self.buf[self.mask] == NAN16).all())


class GuardedOut:
    """bf16 output [rows, hd] at rows [2, 2 + rows), columns [0, hd) of a sentinel-filled [2 + rows + 3, hd + 16] buffer"""

    def __init__(self, rows: int, hd: int, dev):
        self.buf = torch.full((2 + rows + 3, hd + 16), SENT16, dtype=torch.int16, device=dev)
        self.view = self.buf.view(BF16)[2:2 + rows, :hd]
        self.mask = torch.ones_like(self.buf, dtype=torch.bool)
        self.mask[2:2 + rows, :hd] = False

    def intact(self) -> bool:
        return bool((self.buf[self.mask] == SENT16).all())


def group_rows(t: torch.Tensor, geo: Geo, rr: int, joint: bool) -> torch.Tensor:
    """rows of t [s_img + n_j, ..]: the tokens of Ulysses group rr in rank order (its ranks hold consecutive shards), + the joint rows"""
    parts = [t[rr * geo.s_u:(rr + 1) * geo.s_u]] + ([t[geo.s_img:]] if joint else [])
    return torch.cat(parts, 0)


def split_cut(n_kv: int) -> int:
    return (((n_kv + 63) // 64 + 1) // 2) * 64


def replay(kit: Kit, q, k, v, geo: Geo, rr: int, p: int) -> dict:
    """what rank (ring rr, Ulysses p) computes, on one rank: operands by torch indexing, then the same kernel calls"""
    K, dev, hp, w, s_u, n_j = kit.K, q.device, geo.hp, geo.w, geo.s_u, geo.n_j
    n_tot = s_u + n_j
    cols = slice(p * w, (p + 1) * w)
    qf = torch.empty(n_tot, w, dtype=BF16, device=dev)
    kv = torch.empty(2, n_tot, w, dtype=BF16, device=dev)              # K and V share one allocation, as in the object
    of = torch.empty(n_tot, w, dtype=BF16, device=dev)
    qf.copy_(group_rows(q, geo, rr, True)[:, cols])
    kv[0].copy_(group_rows(k, geo, rr, True)[:, cols])
    kv[1].copy_(group_rows(v, geo, rr, True)[:, cols])
    rep = dict(qf=qf, kf=kv[0], vf=kv[1], of=of, parts=None, keys=[kv[0]], vals=[kv[1]], cuts=[], splits=[], static=False)
    if geo.R == 1:
        K.attn_fwd(qf, kv[0], kv[1], of, hp)
        if kit.gpu:
            ws = kit.ops._attn_workspace_bytes(n_tot, n_tot, hp)
            rep["static"] = ws > 0
            rep["cuts"] = [split_cut(n_tot)] if ws > kit.ops.ATTN_MIN_WORKSPACE else []
        return rep
    sp0, sp = K.attn_suggest_splits(n_tot, s_u + n_j, hp), K.attn_suggest_splits(n_tot, s_u, hp)
    parts = K.attn_partials(sp0 + (geo.R - 1) * sp, n_tot, hp, dev)
    parts.used = 0
    K.attn_partial(qf, kv[0], kv[1], parts, hp, sp0)
    rep["splits"] = [sp0]
    for t in range(1, geo.R):
        ring = torch.empty(2, s_u, w, dtype=BF16, device=dev)
        src = (rr - t) % geo.R
        ring[0].copy_(group_rows(k, geo, src, False)[:, cols])
        ring[1].copy_(group_rows(v, geo, src, False)[:, cols])
        K.attn_partial(qf, ring[0], ring[1], parts, hp, sp)
        rep["keys"].append(ring[0]), rep["vals"].append(ring[1]), rep["splits"].append(sp)
    K.attn_merge(parts, of)
    lo = 0
    for kc, s in zip(rep["keys"], rep["splits"]):
        if s == 2:
            rep["cuts"].append(lo + split_cut(kc.shape[0]))
        lo += kc.shape[0]
        rep["cuts"].append(lo)
    rep["parts"] = parts
    return rep


def expected_output(reps: list, geo: Geo, ur: int) -> torch.Tensor:
    """out[r][p w + c] = of_p[ur s_loc + r][c] (image rows), out[s_loc + j][p w + c] = of_p[s_u + j][c] (text rows)"""
    img = torch.cat([r["of"][ur * geo.s_loc:(ur + 1) * geo.s_loc] for r in reps], 1)
    txt = torch.cat([r["of"][geo.s_u:] for r in reps], 1)
    return torch.cat([img, txt], 0)


def _as4(t2: torch.Tensor, H: int) -> torch.Tensor:
    """[rows, H*128] view (any row stride) -> the [1, rows, H, 128] view the reference hook takes"""
    return t2.as_strided((1, t2.shape[0], H, D), (0, t2.stride(0), D, 1), t2.storage_offset())


def norm_weights(dev):
    from hunyuanvideo_efficiency_amd import synthetic as syn
    return tuple((1.0 + 0.25 * syn.hashed_uniform((D,), f"spw.norm.{n}", 3)).to(BF16).to(dev) for n in "qk")


def drive(kit: Kit, sp, geo: Geo, loc: Local, run: Run, ctx: dict):
    """one run of the object through `run.surface` -> (output [s_loc + n_j, H*128], guard or None, consumed or None, problems)"""
    H, hd, s_loc, n_j = geo.H, geo.H * D, geo.s_loc, geo.n_j
    rows = s_loc + n_j
    if run.surface == "call":
        (q_i, q_j), (k_i, k_j), (v_i, v_j) = (loc.chunk(c, geo) for c in range(3))
        kw = {}
        if n_j:
            kw = dict(joint_tensor_query=_as4(q_j, H), joint_tensor_key=_as4(k_j, H), joint_tensor_value=_as4(v_j, H), joint_strategy="rear")
        out = sp(None, _as4(q_i, H), _as4(k_i, H), _as4(v_i, H), dropout_p=0.0, causal=False, **kw)
        assert out.shape == (1, rows, H, D), out.shape
        return out.reshape(rows, hd), None, None, []
    g = GuardedOut(rows, hd, loc.buf.device)
    ctx["out"] = g.view
    if run.surface == "fused":
        sp.run_fused(loc.fused, g.view, s_loc, rows, H, hd)
        return g.view, g, None, []
    sp.begin(s_loc, n_j, H, loc.buf.device)
    P = geo.U
    for c, which in enumerate("qkv"):
        chunk, joint = loc.chunk(c, geo)
        dst = sp.chunk_dst(which)
        if dst is not None:
            dst.copy_(chunk)                        # one rank: the producer writes the operand rows themselves
            chunk = dst
        packed = sp.pack_dst(which) if dst is None else None
        if packed is not None and (run.fill == "copy" or which != "v"):
            assert tuple(packed.shape) == (s_loc, P, geo.w), packed.shape
            if run.fill == "copy":
                packed.copy_(chunk.unflatten(1, (P, geo.w)))
            else:
                wq, wk = ctx["norm_w"]
                nw = wq if which == "q" else wk
                kit.qknorm_rope_(chunk, nw, nw, None, None, 0, H // 2, (H // 2) * D, out=packed)
            sp.send_packed(which, joint, loc.ld)
            continue
        sp.send(which, chunk, chunk.stride(0), joint, loc.ld)
    segs = sp.attend_async(g.view, g.view.stride(0))
    consumed = torch.full((rows, hd), SENT16, dtype=torch.int16, device=loc.buf.device).view(BF16)
    problems, at = [], 0
    for r0, r1, finish in segs:
        if r0 != at or r1 <= r0:
            problems.append(f"segment [{r0}, {r1}) follows row {at}")
        finish()
        consumed[r0:r1] = g.view[r0:r1]             # the consumer (the out-projection GEMM) reads these rows NOW
        at = r1
    if at != rows:
        problems.append(f"the segments end at row {at}, not at s_loc + n_j = {rows}")
    return g.view, g, consumed, problems


def census_v(n: int, hd: int, dev) -> torch.Tensor:
    j, d = torch.arange(n, device=dev)[:, None], torch.arange(hd, device=dev)[None]
    return ((7 * j + 3 * d) % 11 - 5).to(BF16)             # |v| <= 5: every column sum is an integer below 2^24, exact in fp32


def check_census(kit: Kit, sp, geo: Geo, g: int, q, k, v, what: str):
    """A3 on the partial slots the object left"""
    rr, ur = g // geo.U, g % geo.U
    cols = slice(ur * geo.w, (ur + 1) * geo.w)
    n_tot = geo.s_u + geo.n_j
    sp0, sp1 = kit.K.attn_suggest_splits(n_tot, geo.s_u + geo.n_j, geo.hp), kit.K.attn_suggest_splits(n_tot, geo.s_u, geo.hp)
    parts = sp._parts
    want = []
    for t in range(geo.R):
        vc = group_rows(v, geo, (rr - t) % geo.R, t == 0)[:, cols].float()
        edges = [0, vc.shape[0]] if (sp0 if t == 0 else sp1) == 1 else [0, split_cut(vc.shape[0]), vc.shape[0]]
        want += [vc[a:b] for a, b in zip(edges[:-1], edges[1:])]
    assert parts is not None and parts.used == len(want), f"{what}: {getattr(parts, 'used', None)} slots used, {len(want)} expected"
    total = 0.0
    for s, vc in enumerate(want):
        o, m, l = parts.o[s], parts.ml[s, ..., 0], parts.ml[s, ..., 1]
        assert bool((m == 0).all()), f"{what}: slot {s}: m != 0"
        assert bool((l == float(vc.shape[0])).all()), \
            f"{what}: slot {s}: l in [{float(l.min())}, {float(l.max())}], the chunk has {vc.shape[0]} keys"
        sums = vc.sum(0).reshape(1, geo.hp, D).expand(n_tot, geo.hp, D).to(o.device)
        assert torch.equal(o.float(), sums), f"{what}: slot {s}: {int((o.float() != sums).sum())} column sums differ"
        total += float(l[0, 0])
    assert total == geo.s_img + geo.n_j, f"{what}: sum of l over the slots {total}, s_img + n_j = {geo.s_img + geo.n_j}"


def new_object(kit: Kit, groups, run: Run, mutant, ctx):
    from hunyuanvideo_efficiency_amd.long_ctx_attention import UlyssesLongContextAttention
    ug, rg = groups
    sp = UlyssesLongContextAttention(ug, kit.K, rg, nseg=run.nseg, out_exchange=run.out_exchange, scatter_pack=run.scatter_pack)
    sp.min_seg_rows = 1
    if mutant is not None:
        ATTN_MUTANTS[mutant][0](sp, ctx)
    return sp


def check_geo(kit: Kit, log: Log, geo: Geo, g: int, groups, mutant: Optional[str] = None, runs=None, census: bool = True, a2: bool = True):
    """all checks of Part 1 at one geometry, on rank g.  Every collective is inside the object's own calls, and every rank makes the
    same calls whatever its checks say."""
    dev = kit.dev
    rr, ur = g // geo.U, g % geo.U
    n = geo.s_img + geo.n_j
    from tests import attention_bounds as AB
    q, k, v = AB.make_case(geo.cls, n, n, geo.H, "spw." + geo.name, dev)
    ctx = dict(geo=geo, g=g, rr=rr, ur=ur, ld=3 * geo.H * D + 8, norm_w=norm_weights(dev))
    runs = geo.runs if runs is None else runs
    if geo.long and kit.gpu:
        def long_rules():
            n_tot = geo.s_u + geo.n_j
            assert geo.s_u == 4096 and geo.hp == 1
            for n_kv in {n_tot, geo.s_u} if geo.R > 1 else {n_tot}:
                assert kit.K.attn_suggest_splits(n_tot, n_kv, 1) == 2, f"attn_suggest_splits({n_tot}, {n_kv}, 1) != 2"
            if geo.R == 1:
                assert kit.ops._attn_workspace_bytes(n_tot, n_tot, 1) > kit.ops.ATTN_MIN_WORKSPACE, "attn_fwd would not take the KV split"
        log.check("A2 fp64", geo.name + " (dispatch)", long_rules)
    # the operands a run with the qknorm fill sees: q and k normalised per head (no RoPE), computed out of place in ONE head block
    qn = kn = None
    if any(r.scatter_pack and r.fill == "qknorm" for r in runs):
        hd = geo.H * D
        both = torch.empty(n, 1, 2 * hd, dtype=BF16, device=dev)
        kit.qknorm_rope_(torch.cat([q, k], 1), *ctx["norm_w"], None, None, 0, geo.H, hd, out=both)
        qn, kn = both[:, 0, :hd].contiguous(), both[:, 0, hd:].contiguous()
    reps = {}

    def replays(normed: bool):
        if normed not in reps:
            qq, kk = (qn, kn) if normed else (q, k)
            reps[normed] = [replay(kit, qq, kk, v, geo, rr, p) for p in range(geo.U)]
        return reps[normed]

    for run in runs:
        normed = run.surface == "async" and run.scatter_pack and run.fill == "qknorm" and geo.U > 1
        what = f"{geo.name} {run.name} rank {g}"
        mine = replays(normed)
        # raw local rows; with the qknorm fill the joint rows are final already (the block normalises the text rows first)
        loc = Local(q, k, v, geo, g, dev)
        if normed:
            hd = geo.H * D
            loc.fused[geo.s_loc:, :hd] = qn[geo.s_img:]
            loc.fused[geo.s_loc:, hd:2 * hd] = kn[geo.s_img:]
        sp = new_object(kit, groups, run, mutant, ctx)
        res = {}

        def go():
            res["r"] = drive(kit, sp, geo, loc, run, ctx)
        if not log.check("A1 run", what, go):
            continue
        out, guard, consumed, problems = res["r"]
        me = mine[ur]

        def operands():
            for nm in ("qf", "kf", "vf"):
                got = sp._bufs[nm]
                assert bits_equal(got, me[nm]), f"{nm}: {n_bits_differ(got, me[nm])}"
        log.check("A1 operands", what, operands)
        if geo.R > 1:
            def partials():
                p, e = sp._parts, me["parts"]
                assert p.used == e.used, (p.used, e.used)
                assert bits_equal(p.o[:p.used], e.o[:e.used]), "o: " + n_bits_differ(p.o[:p.used].flatten(0, 1), e.o[:e.used].flatten(0, 1))
                assert bits_equal(p.ml[:p.used], e.ml[:e.used]), "ml: " + n_bits_differ(p.ml[:p.used].flatten(0, 1), e.ml[:e.used].flatten(0, 1))
            log.check("A1 partials", what, partials)
        exp = expected_output(mine, geo, ur)

        def output():
            assert not bool(torch.isnan(out).any()), "NaN in the output"
            assert bits_equal(out, exp), n_bits_differ(out, exp)
            assert guard is None or guard.intact(), "a sentinel around the output was overwritten"
            assert loc.intact(), "the memory around the operands was written"
        log.check("A1 output", what, output)
        if consumed is not None:
            def segments():
                assert not problems, "; ".join(problems)
                assert bits_equal(consumed, exp), "rows as read after their segment's finish(): " + n_bits_differ(consumed, exp)
            log.check("A1 segments", what, segments)
    if a2:
        me = replays(False)[ur]
        path = ("ring" if geo.R > 1 else "attn_fwd") + (" long" if geo.long else "")

        def fp64():
            kc, vc = torch.cat(me["keys"], 0), torch.cat(me["vals"], 0)
            # the HIP kernels multiply q' = bf16(q * scale * log2 e) with k; the CPU doubles (the oracle's sdpa) do not round q: each is
            # held to the bound of its own contract (tests/test_attention_bounds_cpu.py::test_unrounded_q_fails_the_contract_and_passes_its_own)
            ref = AB.AttnRef(me["qf"], kc, vc, geo.hp, gap=AB.kernel_gap(me["qf"], kc, geo.hp, cuts=sorted(set(me["cuts"])), static=me["static"]),
                             rounded_q=kit.gpu)
            log.ratio(path, ref.check_o(me["of"], f"replay of rank {g}"))
        log.check("A2 fp64", f"{geo.name} rank {g}", fp64)
    if census and geo.R > 1:
        zq = torch.zeros_like(q)
        kf = AB.make_case("flat", n, n, geo.H, "spw.census", dev)[1]
        cv = census_v(n, geo.H * D, dev)
        what = f"{geo.name} census rank {g}"
        sp = new_object(kit, groups, CALL, mutant, ctx)
        loc = Local(zq, kf, cv, geo, g, dev)
        if log.check("A1 run", what, lambda: drive(kit, sp, geo, loc, CALL, ctx)):
            log.check("A3 census", what, lambda: check_census(kit, sp, geo, g, zq, kf, cv, what))


# ------------------------------------------------------------------------------------------------------------------ mutants, Part 1
def _kernels(K, **over):
    names = ("copy3d", "attn_fwd", "attn_partials", "attn_suggest_splits", "attn_partial", "attn_merge")
    ns = types.SimpleNamespace(**{n: getattr(K, n) for n in names})
    ns.__dict__.update(over)
    return ns


def _shift(t: torch.Tensor, elements: int) -> torch.Tensor:
    return torch.as_strided(t, t.shape, t.stride(), t.storage_offset() + elements)


def _m_copy3d(edit):
    """a mutant of one copy3d call: edit(sp, ctx, args dict) changes the arguments of the call it recognises (or returns False: skip)"""
    def install(sp, ctx):
        inner = sp.k.copy3d

        def copy3d(src, dst, n_batch, rows, cols, src_bs, src_ld, dst_bs, dst_ld):
            a = dict(src=src, dst=dst, n_batch=n_batch, rows=rows, cols=cols, src_bs=src_bs, src_ld=src_ld, dst_bs=dst_bs, dst_ld=dst_ld)
            if edit(sp, ctx, a) is False:
                return dst
            return inner(**a)
        sp.k = _kernels(sp.k, copy3d=copy3d)
    return install


def _edit_pack_swapped(sp, c, a):
    geo = c["geo"]
    if a["n_batch"] == geo.U and a["src_bs"] == geo.w and a["dst_bs"] == geo.s_loc * geo.w and a["dst_ld"] == geo.w:
        a["dst_bs"], a["dst_ld"] = geo.w, geo.U * geo.w            # send[r][p] in place of send[p][r]


def _edit_joint_group0(sp, c, a):
    geo = c["geo"]
    if a["n_batch"] == 1 and a["rows"] == geo.n_j and a["src_ld"] == c["ld"] and a["dst_ld"] == geo.w:
        a["src"] = _shift(a["src"], -c["ur"] * geo.w)               # j[:, 0:w] on every rank


def _edit_txt_batch_stride(sp, c, a):
    geo = c["geo"]
    if a["n_batch"] == geo.U and a["rows"] == geo.n_j and a["src_bs"] == geo.n_j * geo.w and a["dst_bs"] == geo.w:
        a["src_bs"] = geo.s_loc * geo.w


def _edit_segment_no_r0(sp, c, a):
    geo, out = c["geo"], c["out"]
    if (a["n_batch"] == geo.U and a["dst_bs"] == geo.w and a["dst_ld"] == out.stride(0) and a["rows"] < geo.s_loc
            and a["src_bs"] == a["rows"] * geo.w and a["src"].data_ptr() != sp._bufs.get("recv_t", a["dst"]).data_ptr()):
        a["dst"] = _shift(a["dst"], out.storage_offset() - a["dst"].storage_offset())


def _edit_p2p_no_own(sp, c, a):
    geo, out = c["geo"], c["out"]
    if (a["n_batch"] == 1 and a["src_ld"] == geo.w and a["dst_ld"] == out.stride(0)
            and a["src"].untyped_storage().data_ptr() == sp._bufs["of"].untyped_storage().data_ptr()):
        return False


def _m_joint_keys(every: bool):
    def install(sp, ctx):
        inner, geo, st = sp.k.attn_partial, ctx["geo"], {}

        def attn_partial(q, k, v, parts, heads, splits):
            if parts.used == 0:
                st["k"], st["v"] = k[geo.s_u:], v[geo.s_u:]
                if not every:
                    k, v = k[:geo.s_u], v[:geo.s_u]
            elif every:
                k, v = torch.cat([k, st["k"]], 0), torch.cat([v, st["v"]], 0)
            return inner(q, k, v, parts, heads, splits)
        sp.k = _kernels(sp.k, attn_partial=attn_partial)
    return install


def _m_n_slots_from_sp(sp, ctx):
    inner, geo, K = sp.k.attn_partials, ctx["geo"], sp.k
    sp.k = _kernels(sp.k, attn_partials=lambda n_slots, n_q, heads, dev: inner(geo.R * K.attn_suggest_splits(n_q, geo.s_u, heads), n_q, heads, dev))


def _m_last_segment_without_text(sp, ctx):
    inner, geo = sp.attend_async, ctx["geo"]

    def attend_async(out, ld_out, nseg=None):
        segs = inner(out, ld_out, nseg)
        r0, r1, finish = segs[-1]
        segs[-1] = (r0, r1 - geo.n_j, finish)
        return segs
    sp.attend_async = attend_async


_MID = dict(U=2, R=1, H=4, s_loc=63, n_j=11)
# name -> (installer on the object, the check that rejects it, the geometry, the run).  Geometries chosen so that the slip moves data:
# s_loc != n_j, s_loc < n_j for the text unpack (its wrong stride stays inside recv_t), sp0 != sp for the slot count (on the doubles
# attn_suggest_splits is 2 from 128 keys on: s_u = 120 < 128 <= s_u + n_j)
ATTN_MUTANTS = {
    "pack strides swapped": (_m_copy3d(_edit_pack_swapped), "A1 operands", Geo(**_MID), ASYNC),
    "joint rows from head group 0": (_m_copy3d(_edit_joint_group0), "A1 operands", Geo(**_MID), FUSED),
    "joint keys with every ring chunk": (_m_joint_keys(True), "A3 census", Geo(1, 2, 2, 65, 11), CALL),
    "joint keys with no ring chunk": (_m_joint_keys(False), "A3 census", Geo(1, 2, 2, 65, 11), CALL),
    "text all-gather unpacked with batch stride s_loc w": (_m_copy3d(_edit_txt_batch_stride), "A1 output", Geo(2, 1, 4, 5, 11), CALL),
    "segment unpacked without r0": (_m_copy3d(_edit_segment_no_r0), "A1 output", Geo(**_MID), Run("async", 2, "a2a")),
    "last segment does not cover the text rows": (_m_last_segment_without_text, "A1 segments", Geo(**_MID), Run("async", 2, "a2a")),
    "p2p own-slice copy omitted": (_m_copy3d(_edit_p2p_no_own), "A1 output", Geo(**_MID), Run("async", 2, "p2p")),
    "n_slots from sp alone": (_m_n_slots_from_sp, "A1 run", Geo(1, 2, 2, 120, 11), CALL),
}


# ================================================================================================================== Part 2
@dataclasses.dataclass(frozen=True)
class ModelCase:
    U: int
    R: int
    thw: tuple
    n_valid: int
    variant: int
    s_txt: int = 32

    @property
    def world(self) -> int:
        return self.U * self.R

    @property
    def name(self) -> str:
        return f"U{self.U}xR{self.R}-thw{'x'.join(map(str, self.thw))}-v{self.n_valid}-variant{self.variant}"


VARIANTS = [dict(nseg=1, out_exchange="a2a", scatter_pack=False), dict(nseg=2, out_exchange="a2a", scatter_pack=True),
            dict(nseg=2, out_exchange="p2p", scatter_pack=True)]
# H-split: (H/2) % P == 0; W-split: (H/2) % P != 0 and (W/2) % P == 0.  n_valid 0 / 11 / s_txt, cycling over the three variants
H2, W2, H4, W4 = (3, 12, 12), (3, 10, 16), (3, 8, 12), (3, 12, 16)
MODEL_CASES = [
    ModelCase(2, 1, H2, 11, 0), ModelCase(2, 1, W2, 0, 1), ModelCase(2, 1, H2, 32, 2),
    ModelCase(4, 1, W4, 11, 1), ModelCase(4, 1, H4, 0, 2), ModelCase(4, 1, W4, 32, 0),
    ModelCase(2, 2, H4, 11, 2), ModelCase(2, 2, W4, 32, 1), ModelCase(2, 2, H4, 0, 0),
]
MODEL_WORLDS = sorted({c.world for c in MODEL_CASES})


def sp_object(model):
    """the attention object parallelize_transformer_module holds for this model"""
    from hunyuanvideo_efficiency_amd.long_ctx_attention import UlyssesLongContextAttention
    hits = [c.cell_contents for c in model.forward.__closure__ if isinstance(c.cell_contents, UlyssesLongContextAttention)]
    assert len(hits) == 1
    return hits[0]


def token_order(thw, P: int):
    """(split axis of the latent, per rank the unsharded indices of its tokens): the same torch.chunk on an index tensor"""
    t, h, w = thw[0], thw[1] // 2, thw[2] // 2
    axis = 1 if h % P == 0 else 2
    idx = torch.arange(t * h * w).reshape(t, h, w)
    return axis, [c.reshape(-1) for c in torch.chunk(idx, P, dim=axis)]


def _gather(t: torch.Tensor, world: int):
    parts = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(parts, t.contiguous())
    return [p.cpu() for p in parts]


def check_model_case(kit: Kit, log: Log, h, model, case: ModelCase, rank: int):
    """B1, B2, B3 at one case.  The collectives (the two forwards, two all-gathers) are outside the recorded checks."""
    from oracle import dit_ref as Rf
    from tests import dit_wiring as W
    world = case.world
    wc = W.Case(case.thw, case.s_txt, case.n_valid)
    sp = sp_object(model)
    for kk, vv in VARIANTS[case.variant].items():
        setattr(sp, kk, vv)
    sp.min_seg_rows = 8
    inp = h.inputs(wc, "fp8")
    out, rec = h.run_traced(model, inp)
    _, order = token_order(case.thw, world)
    mine, s_loc, s_img = order[rank], order[rank].numel(), wc.s_img
    blocks = [r for r in rec if "block" in r["name"]] + [rec[-1]]
    # one all-gather of the image rows around every block (+ the final layer's input), one of the text rows after every block
    img = torch.stack([t for r in blocks for t in (r["x_in"][:s_loc], r["x_out"][:s_loc])])
    txt = torch.stack([r["x_out"][s_loc:] for r in blocks[:-1]])
    img_all, txt_all = _gather(img, world), _gather(txt, world)
    perm = torch.cat(order)
    full = torch.empty(img.shape[0], s_img, img.shape[2], dtype=img.dtype)
    full[:, perm] = torch.cat(img_all, 1)
    what = f"{case.name} rank {rank}"
    cfg = W.config("fp8")
    sd, _ = h.oracle_weights(model)
    c = W._cpu(inp)
    cos, sin, heads = c["freqs_cos"], c["freqs_sin"], cfg.heads_num
    cu = torch.tensor([0, s_img + case.n_valid, s_img + case.s_txt], dtype=torch.int32)
    text_rows = case.n_valid > 0
    ratios = {}

    def b1():
        assert [r["name"] for r in blocks] == ["double_block.0", "single_block.0", "single_block.1", "final_layer"]
        assert all(r["args"][4] == s_loc + case.n_valid for r in blocks[:-1]), [r["args"][4] for r in blocks[:-1]]
        for r in blocks[:-1]:
            # the tables a block is handed are the rows of the unsharded tables at this rank's tokens, bit for bit
            assert bits_equal(r["args"][5].cpu(), cos[mine]) and bits_equal(r["args"][6].cpu(), sin[mine]), \
                f"{r['name']}: the RoPE tables are not rows {mine[:3].tolist()}.. of the unsharded tables"
        for i, r in enumerate(blocks):
            name, vec = r["name"], r["args"][2 if i == len(blocks) - 1 else 3].float().cpu()
            x_in = torch.cat([full[2 * i].float(), r["x_in"][s_loc:].float().cpu()], 0)         # gathered image rows | this rank's text rows
            x_out = r["x_out"].float().cpu()
            if name.startswith("double"):
                rio, rto = Rf.double_block(sd, "double_blocks.0.", x_in[None, :s_img], x_in[None, s_img:], vec, cu, cos, sin, heads, W.E)
                ratios[name + ".img"] = W._ratio(x_out[:s_loc], rio[0, mine], name + ".img")
                if text_rows:
                    ratios[name + ".txt"] = W._ratio(x_out[s_loc:], rto[0], name + ".txt")
            elif name.startswith("single"):
                ref = Rf.single_block(sd, name.replace("_block", "_blocks") + ".", x_in[None], vec, case.s_txt, cu, cos, sin, heads, W.E)
                ratios[name + ".img"] = W._ratio(x_out[:s_loc], ref[0, mine], name + ".img")
                if text_rows:
                    ratios[name + ".txt"] = W._ratio(x_out[s_loc:], ref[0, s_img:], name + ".txt")
            else:
                t, hh, w = case.thw
                ref = Rf.unpatchify(Rf.final_layer(sd, x_in[None, :s_img], vec, W.E), t, hh // 2, w // 2, cfg.out_channels, cfg.patch_size)
                ratios["final_layer+gather"] = W._ratio(out, ref, "the gathered output")
        bad = {k_: v_ for k_, v_ in ratios.items() if not v_ <= 1.0}
        assert not bad, f"stages beyond rtol 2^-6 / atol 6e-2 (error / tolerance): {bad}"
    log.check("B1 stages", what, b1)
    for k_, v_ in ratios.items():
        log.ratio("B1 " + k_, v_)

    def b2():
        me = txt_all[rank].view(torch.int16)
        for peer in range((rank // case.U) * case.U, (rank // case.U + 1) * case.U):
            other = txt_all[peer].view(torch.int16)
            same = (me == other) | (torch.isnan(txt_all[rank]) & torch.isnan(txt_all[peer]))      # a NaN row (n_valid = 0) has no value
            for i in range(me.shape[0]):
                assert bool(same[i].all()), f"text rows after {blocks[i]['name']} differ from rank {peer}'s in {int((~same[i]).sum())} elements"
    log.check("B2 text rows", what, b2)
    if case.n_valid < case.s_txt:
        from hunyuanvideo_efficiency_amd import synthetic as syn
        inp2 = W.clone_inputs(inp)
        pad = inp2["text_states"][0, case.n_valid:]
        junk = syn.hashed_uniform(tuple(pad.shape), "spw.padding", 5) * 3.0
        junk.view(-1)[::7] *= 1000.0
        pad.copy_(junk.to(BF16))
        out2 = h.run(model, inp2)

        def b3():
            assert bits_equal(out, out2), "padding text content changed the output: " + n_bits_differ(out.flatten(0, 3), out2.flatten(0, 3))
        log.check("B3 padding content", what, b3)


class _TorchProxy:
    """`torch` as inference.py sees it, with some functions replaced"""

    def __init__(self, **over):
        self._over = over

    def __getattr__(self, name):
        return self._over[name] if name in self._over else getattr(torch, name)


@contextlib.contextmanager
def _patched_inference_torch(**over):
    from hunyuanvideo_efficiency_amd import inference
    inference.torch = _TorchProxy(**over)
    try:
        yield
    finally:
        inference.torch = torch


def _mutant_rope_other_axis():
    def chunk(t, n, dim=0):
        return torch.chunk(t, n, dim={-3: -2, -2: -3}[dim] if t.dim() == 4 else dim)
    return _patched_inference_torch(chunk=chunk)


def _mutant_gather_other_axis():
    def cat(ts, dim=0):
        return torch.cat(ts, dim={-2: -1, -1: -2}[dim] if ts[0].dim() == 5 else dim)
    return _patched_inference_torch(cat=cat)


# name -> (context manager factory, the check that rejects it, the case).  H2: both H/2 and W/2 are 6, so the tables sharded along W
# have the right number of rows
MODEL_MUTANTS = {
    "RoPE tables sharded along the other axis": (_mutant_rope_other_axis, "B1 stages", ModelCase(2, 1, H2, 11, 0)),
    "output gather concatenated along the other axis": (_mutant_gather_other_axis, "B1 stages", ModelCase(2, 1, H2, 11, 1)),
}
MUTANTS = {**{k: v[1:] for k, v in ATTN_MUTANTS.items()}, **{k: v[1:] for k, v in MODEL_MUTANTS.items()}}


# ================================================================================================================== rank worker
def rank_main(rank: int, world: int, port: int, outdir: str, device: str, part: str, mutant: Optional[str] = None):
    """one rank: part "attention" (all geometries of this world size) | "model" (all model cases of this world size) | "mutant" (the
    one case of `mutant`).  Writes {failures, ratios} to outdir/rank<r>.json."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    log = Log()
    try:
        torch.set_num_threads(2)            # `world` processes share the host
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=TIMEOUT)
        if device == "cuda":
            torch.cuda.set_device(0)
            from tests.sp_gpu_helpers import stage_collectives_through_host
            stage_collectives_through_host()
        kit = Kit(device)
        if part == "attention" or mutant in ATTN_MUTANTS:
            if mutant is not None:
                _, _, geo, run = ATTN_MUTANTS[mutant]
                groups, clean = make_groups(geo.U, geo.R), Log()
                check_geo(kit, clean, geo, rank, groups, None, runs=(run,), a2=False)      # the faithful object passes the very same calls
                log.failures += ["faithful: " + f for f in clean.failures]
                check_geo(kit, log, geo, rank, groups, mutant, runs=(run,), a2=False)
            else:
                geos = geos_of(world, kit.gpu)
                groups = {ur: make_groups(*ur) for ur in sorted({(g.U, g.R) for g in geos})}
                for geo in geos:
                    check_geo(kit, log, geo, rank, groups[(geo.U, geo.R)])
        else:
            _model_part(kit, log, rank, world, mutant)
        if device == "cuda":
            torch.cuda.synchronize()
    except Exception:  # noqa: BLE001
        log.failures.append("worker raised: " + traceback.format_exc())
    finally:
        with open(os.path.join(outdir, f"rank{rank}.json"), "w") as f:
            json.dump(dict(failures=log.failures, ratios=log.ratios), f)
        if dist.is_initialized():
            dist.destroy_process_group()


def _model_part(kit: Kit, log: Log, rank: int, world: int, mutant: Optional[str]):
    from hunyuanvideo_efficiency_amd.builders import build_model
    from hunyuanvideo_efficiency_amd.inference import parallelize_transformer_module
    from tests import dit_wiring as W
    if not kit.gpu:
        from tests import cpu_kernel_doubles as KD
        KD.install()
    cases = [MODEL_MUTANTS[mutant][2]] if mutant is not None else [c for c in MODEL_CASES if c.world == world]
    h = W.Harness(str(kit.dev))
    models = {}
    for ur in sorted({(c.U, c.R) for c in cases}):
        ug, rg = make_groups(*ur)
        model = build_model(W.config("fp8"), kit.dev)
        model.wiring_kind = "sp"
        parallelize_transformer_module(model, None, None if kit.gpu else kit.K, ulysses_group=ug, ring_group=rg)
        models[ur] = model
    if mutant is not None:
        clean = Log()
        check_model_case(kit, clean, h, models[(cases[0].U, cases[0].R)], cases[0], rank)
        log.failures += ["faithful: " + f for f in clean.failures]
    with (MODEL_MUTANTS[mutant][0]() if mutant is not None else contextlib.nullcontext()):
        for case in cases:
            check_model_case(kit, log, h, models[(case.U, case.R)], case, rank)


def read_results(outdir: str, world: int):
    """([failure strings of all ranks], {path: largest ratio}); a rank that left no file has failed"""
    failures, ratios = [], {}
    for r in range(world):
        path = os.path.join(outdir, f"rank{r}.json")
        if not os.path.exists(path):
            failures.append(f"rank {r} left no result")
            continue
        with open(path) as f:
            res = json.load(f)
        failures += res["failures"]
        for k, v in res["ratios"].items():
            ratios[k] = max(ratios.get(k, 0.0), v)
    return failures, ratios
