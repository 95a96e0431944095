"""TEST INFRASTRUCTURE: the VAE tile coder as a COMPOSITION - cases, a recorder, device-agnostic checks and mutants for the host layer
that wires the VAE kernels into AutoencoderKLCausal3D._decode_tile / _encode_tile (_mid_block, _resnet, _mid_attention, _conv, _gn and the
weight packing of _prepare).  The same functions run on the CPU kernel doubles (tests/test_vae_wiring_cpu.py, where every mutant below
must be rejected) and on the HIP kernels (tests/test_gpu_vae_wiring.py).  The companion of tests/dit_wiring.py.

Recorder (`recording`): wraps the fifteen vae_ops entry points the tile coder calls and the methods _resnet, _mid_attention, _mid_block
and _gn of ONE model instance; every call keeps its stage name (the _prepare key of the weight it was given), clones of its tensor
operands as the device held them, its scalar arguments, a clone of its output and - for GroupNorm statistics - the very call that
produced the GNStats object.  Before a conv runs the recorder asserts that its source has exactly the rows the geometry arguments
describe (an output grid that does not fit its source would make the kernel gather outside it).

  A  stage by stage, each stage on its OWN input, so no error accumulates:
     single kernels against their fp64 restatement with the bound the project already has for that kernel (error_bounds.Ref tap by tap
     for GEMMs and convs, rowwise_bounds for GroupNorm apply / softmax / the average pool, tinterp_bounds, conv_bounds for the planes tail),
     bit equality for latent_tile, transpose, nearest-up, copy4d_ and every zero padding;
     composite stages (resnet, mid_attention, upsampler, downsampler, tail, post_quant_conv, quant_conv) against oracle/vae_ref.py /
     vae_enc_ref.py in the fp16-emulated contract, in max norm, with the tolerance 4 x |oracle fp16 contract - oracle fp64| on that same
     input (reference against reference), floored at 2 fp16 ulps of the stage's largest |y|.
  B  statistics hand-off: at every site that consumes a GNStats (i) its producer is the tensor being normalised, by recorder identity,
     (ii) the affine agrees with the fp64 affine of that tensor within 2e-4 (1 + |y|) (tests/test_gpu_groupnorm_conditioning.py), (iii) the
     same GroupNorm without the hand-off, on the same tensor, agrees within twice that; and the set of sites that hand off is the one the
     case table states by hand.
  C  trace: the ordered list of (stage, conv form, geometry, flags) equals the one generated here from vae_ref.decoder_config /
     vae_enc_ref.encoder_config and the t_ops dict; the final (T', H', W') is the oracle's output shape.
  D  nothing skipped: every recorded call is matched by exactly one check.
A check raises AssertionError whose message starts with the check's letter; Harness.ratios collects error / tolerance per stage kind."""
from __future__ import annotations

import contextlib
import dataclasses
import math
import os
import types
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

from hunyuanvideo_efficiency_amd import synthetic as syn
from oracle import vae_enc_ref as VE
from oracle import vae_ref as VR
from tests import conv_bounds as CB
from tests import error_bounds as EB
from tests import rowwise_bounds as RB
from tests import tinterp_bounds as TB

F16, F32, F64 = torch.float16, torch.float32, torch.float64
E = VR.Prec(True)
from tests.test_gpu_groupnorm_conditioning import AFFINE_TOL as GN_AFFINE_TOL  # noqa: E402  2e-4 (1 + |y|), every affine path
COMPOSITE_FACTOR = 4.0          # composite tolerance = 4 x the distance of the two oracles, floored at ...
COMPOSITE_FLOOR_ULPS = 2.0      # ... 2 fp16 ulps of the stage's largest |y|
TOPO_A = (64, 128, 256, 256)    # all three conv forms, both shortcut resnets, the epilogue hand-off everywhere (C % 64 == 0)
TOPO_B = (32, 64, 128, 128)     # the goldens' reduced model: 32 channels -> one channel per group, no hand-off, _pad_channels

KERNELS = {  # vae_ops name -> its positional argument names
    "latent_tile": ("z", "cpad"),
    "gemm_f16": ("a", "w", "bias", "out", "out_f32", "res", "n", "k"),
    "conv3d_causal": ("x", "w", "bias", "T", "H", "W", "cin", "cout", "up_t", "up_hw", "res", "out", "gn_stats"),
    "conv3d_upsampled_subpixel": ("x", "w", "table", "ntap", "bias", "sT", "sH", "sW", "cin", "cout", "up_t", "out", "gn_stats"),
    "conv3d_causal_strided": ("x", "w", "bias", "sT", "sH", "sW", "cin", "cout", "stride", "out"),
    "conv_cout4": ("x", "affine", "silu", "w", "bias", "T", "H", "W", "cin", "cout", "out"),
    "groupnorm_affine": ("x", "weight", "bias", "groups", "eps"),
    "groupnorm_affine_from_stats": ("st", "weight", "bias", "groups", "eps"),
    "groupnorm_apply": ("x", "affine", "silu", "out"),
    "softmax_rows": ("S", "cols", "cols_pad", "scale", "out", "causal_block"),
    "transpose_16b": ("src", "dst"),
    "temporal_avg_pool": ("x", "T", "HW", "k", "s"),
    "temporal_nearest_up": ("x", "T", "HW", "s"),
    "temporal_linear_up": ("x", "T", "HW", "s"),
    "copy4d_": ("src", "dst"),
}
DEFAULTS = {"gemm_f16": dict(bias=None, out=None, out_f32=False, res=None, n=None, k=None),
            "conv3d_causal": dict(up_t=False, up_hw=False, res=None, out=None, gn_stats=False),
            "conv3d_upsampled_subpixel": dict(out=None, gn_stats=False), "conv3d_causal_strided": dict(stride=(1, 1, 1), out=None),
            "conv_cout4": dict(out=None), "groupnorm_affine": dict(groups=32, eps=1e-6),
            "groupnorm_affine_from_stats": dict(groups=32, eps=1e-6), "groupnorm_apply": dict(out=None),
            "softmax_rows": dict(out=None, causal_block=0)}
WEIGHT_ROLE = {"gemm_f16": "w", "conv3d_causal": "w", "conv3d_upsampled_subpixel": "w", "conv3d_causal_strided": "w", "conv_cout4": "w",
               "groupnorm_affine": "weight", "groupnorm_affine_from_stats": "weight"}
METHODS = ("_resnet", "_mid_attention", "_mid_block", "_gn")


def _r(x: int, m: int) -> int:
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass(eq=False)
class Case:
    name: str
    half: str                           # "decoder": shape is the latent (T, H, W); "encoder": the video (T, H, W)
    boc: tuple
    shape: tuple
    handoff: frozenset                  # the GroupNorm sites that consume epilogue statistics, written by hand (see HANDOFF_*)
    t_ops: Optional[dict] = None
    subpixel: str = "fast"              # HV_VAE_SUBPIXEL
    conv_out: str = "planes"            # HV_VAE_CONV_OUT
    batch_bytes: Optional[int] = None   # mid_attention_batch_bytes (None: the product's default)

    def __repr__(self):
        return self.name


def _sites(half, what, blocks, resnets):
    return [f"{half}.{what}.{i}.resnets.{j}" for i in blocks for j in resnets]


# The expected hand-off sets, from the REFERENCE topology alone: a GroupNorm takes the statistics of a conv epilogue where the tensor it
# normalises was stored by a conv (conv1 of its own resnet, conv2 of the resnet before it, or the upsampler conv before its block) with
# nothing in between, and has an even number of channels per group.  The mid block and the encoder hand off inside a resnet only (conv1 ->
# norm2): their resnets are called without the statistics of their input.
_DEC_NORM2 = [n + ".norm2" for n in ["decoder.mid_block.resnets.0", "decoder.mid_block.resnets.1"] + _sites("decoder", "up_blocks", range(4), range(3))]
_DEC_NORM1 = [n + ".norm1" for n in _sites("decoder", "up_blocks", range(4), range(3))]
# up_blocks.0.resnets.0.norm1 normalises the mid block's output: never handed off
HANDOFF_A = frozenset(_DEC_NORM2 + _DEC_NORM1 + ["decoder.conv_norm_out"]) - {"decoder.up_blocks.0.resnets.0.norm1"}
# TOPO_B, decoder widths 128, 128, 64, 32: exactly the sites whose tensor has 64 or 128 channels
HANDOFF_B = frozenset(
    ["decoder.mid_block.resnets.0.norm2", "decoder.mid_block.resnets.1.norm2"]
    + [n + ".norm2" for n in _sites("decoder", "up_blocks", (0, 1, 2), range(3))]                   # conv1 outputs of 128, 128, 64 channels
    + ["decoder.up_blocks.0.resnets.1.norm1", "decoder.up_blocks.0.resnets.2.norm1"]                # 128
    + [n + ".norm1" for n in _sites("decoder", "up_blocks", (1, 2), range(3))]                      # 128 | 128, 64, 64
    + ["decoder.up_blocks.3.resnets.0.norm1"])                                                      # the 64-channel upsampler output
# TOPO_B, encoder widths 32, 64, 128, 128: norm2 of the 64- and 128-channel resnets
HANDOFF_B_ENC = frozenset([n + ".norm2" for n in _sites("encoder", "down_blocks", (1, 2, 3), range(2))
                           + ["encoder.mid_block.resnets.0", "encoder.mid_block.resnets.1"]])


def _up(i, before=(False,) * 3, after=(False,) * 3, scale=None, mode=None):
    d = {"block_index": i, "enable_t_interp_before_block": list(before), "enable_t_interp_after_block": list(after)}
    if scale is not None:
        d["interp_t_scale_factor"] = scale
    if mode is not None:
        d["interp_mode"] = mode
    return d


def _pool(before, after, k=None, s=None, **extra):
    d = {"enable_t_pool_before_block": list(before), "enable_t_pool_after_block": list(after)}
    if k is not None:
        d["pool_t_kernel"] = k
    if s is not None:
        d["pool_t_stride"] = s
    d.update(extra)
    return d


T_, F_ = True, False
CASES = [
    # ---- topology A: the three conv forms and both conv_out modes, at T = 1, an odd ragged tile and a 3-frame tile
    Case("A-1x2x2-off-gemm", "decoder", TOPO_A, (1, 2, 2), HANDOFF_A, subpixel="off", conv_out="gemm"),
    Case("A-2x3x5-fast-planes", "decoder", TOPO_A, (2, 3, 5), HANDOFF_A),                             # L = 30: batched attention
    Case("A-3x4x4-exact-gemm", "decoder", TOPO_A, (3, 4, 4), HANDOFF_A, subpixel="exact", conv_out="gemm"),
    Case("A-3x3x5-perframe", "decoder", TOPO_A, (3, 3, 5), HANDOFF_A, batch_bytes=0),                 # L = 45, 15 keys per frame
    # ---- decoder t_ops on topology A
    # block 1 interpolates before its first resnet: the upsampler of block 0 must not hand off; T = 1 input, nearest, scale 2
    Case("A-tops-eib-first", "decoder", TOPO_A, (1, 2, 2), HANDOFF_A - {"decoder.up_blocks.1.resnets.0.norm1"},
         t_ops={"decoder": {"up_blocks": [_up(1, before=(T_, F_, F_), scale=2, mode="nearest")]}}),
    # the last block interpolates after its first and its last resnet: trilinear, scale 3; conv_norm_out reads an interpolated tensor
    Case("A-tops-eia-last", "decoder", TOPO_A, (2, 2, 2),
         HANDOFF_A - {"decoder.up_blocks.3.resnets.1.norm1", "decoder.conv_norm_out"},
         t_ops={"decoder": {"up_blocks": [_up(3, after=(T_, F_, T_), scale=3, mode="trilinear")]}}),
    # block 2: before the first and the last resnet, after the middle one (the scale and the mode at their defaults, 2 and nearest)
    Case("A-tops-both", "decoder", TOPO_A, (1, 2, 2),
         HANDOFF_A - {"decoder.up_blocks.2.resnets.0.norm1", "decoder.up_blocks.2.resnets.2.norm1"},
         t_ops={"decoder": {"up_blocks": [_up(2, before=(T_, F_, T_), after=(F_, T_, F_))]}}),
    # ---- topology B: one channel per group in the 32-channel block (statistics None), _pad_channels; the goldens' latent
    Case("B-3x4x4", "decoder", TOPO_B, (3, 4, 4), HANDOFF_B),
    # ---- mid-block pools, decoder: before / after / both; (k, s) default (2, 2), (3, 2), (3, 1); T = 5, 2, 1
    Case("B-midpool-before-k2s2-T5", "decoder", TOPO_B, (5, 2, 2), HANDOFF_B, t_ops={"decoder": {"mid_block": _pool((T_, F_), (F_, F_))}}),
    Case("B-midpool-mixed-k3s2-T2", "decoder", TOPO_B, (2, 2, 2), HANDOFF_B, t_ops={"decoder": {"mid_block": _pool((F_, T_), (T_, F_), 3, 2)}}),
    Case("B-midpool-both-k3s1-T1", "decoder", TOPO_B, (1, 2, 2), HANDOFF_B, t_ops={"decoder": {"mid_block": _pool((T_, T_), (T_, T_), 3, 1)}}),
    # ---- encoder: the plain 884 schedule, pools around down-block resnets, one downsample_stride override on a temporal block, mid pools
    Case("B-enc-5x16x16", "encoder", TOPO_B, (5, 16, 16), HANDOFF_B_ENC),
    Case("B-enc-1x16x16", "encoder", TOPO_B, (1, 16, 16), HANDOFF_B_ENC),
    Case("B-enc-tops", "encoder", TOPO_B, (5, 16, 16), HANDOFF_B_ENC,
         t_ops={"encoder": {"down_blocks": [dict(_pool((F_, T_), (T_, F_)), block_index=0),
                                            dict(_pool((F_, F_), (F_, F_)), block_index=2, downsample_stride=[1, 2, 2])],
                            "mid_block": _pool((F_, T_), (T_, F_), 3, 2)}}),
    Case("B-enc-midpool-k2s2-T2", "encoder", TOPO_B, (5, 16, 16), HANDOFF_B_ENC, t_ops={"encoder": {"mid_block": _pool((T_, F_), (F_, T_))}}),  # 2 frames reach it
    Case("B-enc-midpool-k3s1-T1", "encoder", TOPO_B, (1, 16, 16), HANDOFF_B_ENC, t_ops={"encoder": {"mid_block": _pool((T_, F_), (F_, T_), 3, 1)}}),
]
CASE = {c.name: c for c in CASES}


# ------------------------------------------------------------------------------------------------------------------ recorder
class Call:
    """one kernel launch: t = cloned tensor operands by role, kw = scalars, out = clone of the result, ref = the live operand / result
    tensors (identity), stats = the GNStats it returned, producer = for groupnorm_affine_from_stats the Call that made its GNStats"""

    def __init__(self, idx, name):
        self.idx, self.name, self.stage = idx, name, None
        self.t, self.kw, self.ref = {}, {}, {}
        self.out = self.out_ref = self.stats = self.producer = None
        self.inside = ()            # names of the model methods the call ran under, outermost first
        self.checked = 0

    def __repr__(self):
        return f"<{self.idx} {self.name} {self.stage}>"


class Stage:
    """one call of a wrapped model method: args as given (tensors cloned), out (clone; a tuple stays a tuple), first/last kernel index"""

    def __init__(self, name, pre):
        self.name, self.pre = name, pre
        self.args, self.kw = (), {}
        self.ref_in = self.out = self.out_ref = None       # ref_in / out_ref: the live tensors (identity along the data path)
        self.first = self.last = 0
        self.checked = 0

    def __repr__(self):
        return f"<{self.name} {self.pre} [{self.first}, {self.last})>"


class Recording:
    def __init__(self):
        self.calls: List[Call] = []
        self.stages: List[Stage] = []
        self.stats_producer = {}        # data_ptr of GNStats.partial -> Call (the buffer is kept alive by call.stats)
        self.open: List[Stage] = []

    def of(self, name):
        return [c for c in self.calls if c.name == name]

    def stages_of(self, name):
        return [s for s in self.stages if s.name == name]


def _same(a, b) -> bool:
    return a is not None and b is not None and a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride()


def weight_names(P) -> Dict[int, str]:
    """data_ptr of the first tensor of every _prepare entry -> its key: the stage name of a kernel call"""
    return {v[0].data_ptr(): k for k, v in P.items()}


def _conv_geometry(name, b):
    """C, before the launch: the source rows a conv is about to gather from are exactly those its geometry arguments describe"""
    if name == "conv3d_causal":
        src = ((b["T"] + 1) // 2 if b["up_t"] else b["T"], b["H"] >> int(b["up_hw"]), b["W"] >> int(b["up_hw"]))
        ok = (not b["up_t"] or b["T"] % 2 == 1) and (not b["up_hw"] or (b["H"] % 2 == 0 and b["W"] % 2 == 0))
    elif name in ("conv3d_upsampled_subpixel", "conv3d_causal_strided"):
        src, ok = (b["sT"], b["sH"], b["sW"]), True
    elif name == "conv_cout4":
        src, ok = (b["T"], b["H"], b["W"]), True
    else:
        return
    rows = src[0] * src[1] * src[2]
    assert ok and b["x"].shape[0] == rows and b["x"].shape[1] >= b["cin"], \
        f"C geometry: {name} is given a source of {tuple(b['x'].shape)} for the grid {src} x {b['cin']} channels (up_t {b.get('up_t')}, up_hw {b.get('up_hw')})"


@contextlib.contextmanager
def recording(vae, V=None):
    """Install the wrappers on vae_ops (module attributes, looked up by the host at call time) and on the instance `vae`."""
    from hunyuanvideo_efficiency_amd import vae_ops
    V = V or vae_ops
    rec = Recording()
    names = weight_names(vae._prepare())
    saved = {n: getattr(V, n) for n in KERNELS}

    def clone(v):
        return v.clone() if torch.is_tensor(v) else v

    def wrap_kernel(name, fn):
        def wrapper(*args, **kwargs):
            b = dict(DEFAULTS.get(name, {}))
            b.update(zip(KERNELS[name], args))
            b.update(kwargs)
            _conv_geometry(name, b)
            c = Call(len(rec.calls), name)
            c.inside = tuple(s.name for s in rec.open)
            for k, v in b.items():
                if torch.is_tensor(v):
                    c.ref[k] = v
                    if k not in ("out", "dst"):
                        c.t[k] = v.clone()
                elif k == "st":
                    c.producer = rec.stats_producer.get(v.partial.data_ptr())
                    c.kw["st_M"], c.kw["st_C"] = v.M, v.C
                    c.stats = v
                else:
                    c.kw[k] = v
            role = WEIGHT_ROLE.get(name)
            if role is not None:
                c.stage = names.get(b[role].data_ptr())
            if c.stage is None:
                c.stage = (rec.open[-1].pre if rec.open else "") + name
            ret = fn(*args, **kwargs)
            out = ret[0] if isinstance(ret, tuple) else ret
            if name in ("transpose_16b", "copy4d_"):
                out = b["dst"]
            c.out_ref, c.out = out, out.clone()
            if isinstance(ret, tuple) and name in ("conv3d_causal", "conv3d_upsampled_subpixel") and ret[1] is not None:
                c.stats = ret[1]
                rec.stats_producer[ret[1].partial.data_ptr()] = c
            if isinstance(ret, tuple) and name in ("conv3d_causal_strided", "temporal_avg_pool", "temporal_nearest_up", "temporal_linear_up"):
                c.kw["ret_geom"] = tuple(ret[1:])
            rec.calls.append(c)
            return ret
        return wrapper

    def wrap_method(name):
        inner = getattr(vae, name)

        def method(P, pre, *args, **kwargs):
            s = Stage(name, pre)
            s.args, s.kw = tuple(clone(a) for a in args), {k: clone(v) for k, v in kwargs.items()}
            s.ref_in = args[0]
            s.first = len(rec.calls)
            rec.open.append(s)
            try:
                ret = inner(P, pre, *args, **kwargs)
            finally:
                rec.open.pop()
            s.last = len(rec.calls)
            s.out_ref = ret
            s.out = tuple(clone(r) for r in ret) if isinstance(ret, tuple) else clone(ret)
            rec.stages.append(s)
            return ret
        setattr(vae, name, method)

    try:
        for n in KERNELS:
            setattr(V, n, wrap_kernel(n, saved[n]))
        for n in METHODS:
            wrap_method(n)
        yield rec
    finally:
        for n in KERNELS:
            setattr(V, n, saved[n])
        for n in METHODS:
            vae.__dict__.pop(n, None)


# ------------------------------------------------------------------------------------------------------------------ harness
class Harness:
    """Models, inputs and oracle weights for one device.  On "cpu" the caller has installed the doubles on vae_ops."""

    def __init__(self, device):
        self.dev = device
        self._models = {}
        self.ratios = {}            # stage kind -> (largest error / tolerance, case name)
        self.dists = {}             # composite stage kind -> (largest oracle-to-oracle distance / largest |y|, case name)
        self.ran = set()
        self._sd = {}

    def model(self, case: Case, fresh: bool = False):
        key = (case.boc, case.subpixel, case.conv_out, case.half)
        if not fresh and key in self._models:
            return self._models[key]
        from hunyuanvideo_efficiency_amd.vae import AutoencoderKLCausal3D
        enc = case.half == "encoder"
        vae = AutoencoderKLCausal3D(block_out_channels=case.boc, device=self.dev, with_encoder=enc)
        sd = syn.synth_vae_state_dict(case.boc, seed=0, encoder=enc)
        vae.load_state_dict({k: v.to(F16) for k, v in sd.items()}, strict=True)
        old = {k: os.environ.get(k) for k in ("HV_VAE_SUBPIXEL", "HV_VAE_CONV_OUT")}
        os.environ["HV_VAE_SUBPIXEL"], os.environ["HV_VAE_CONV_OUT"] = case.subpixel, case.conv_out
        try:
            vae._prepare()              # the two modes are read here, once
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        if not fresh:
            self._models[key] = vae
        return vae

    def sd(self, case: Case, dtype=F32):
        """the oracle's state dict: the fp16 weights the module holds, as fp32 / fp64, on the CPU"""
        key = (case.boc, case.half, dtype)
        if key not in self._sd:
            sd = syn.synth_vae_state_dict(case.boc, seed=0, encoder=case.half == "encoder")
            self._sd[key] = {k: v.to(F16).to(dtype) for k, v in sd.items()}
        return self._sd[key]

    def input(self, case: Case) -> torch.Tensor:
        """decoder: an fp32 latent [16, T, H, W] of unit scale; encoder: an fp32 video [3, T, H, W] in [-1, 1]"""
        c = 16 if case.half == "decoder" else 3
        x = syn.hashed_uniform((c, *case.shape), f"vae_wiring.{case.half}.{case.shape}", 11)
        return (x * (math.sqrt(3.0) if case.half == "decoder" else 1.0)).to(self.dev)

    def run(self, case: Case, vae=None, mutant=None):
        """(output rows, T', H', W', Recording) of the tile coder under the recorder (and under `mutant`, laid OVER the recorder)"""
        vae = vae or self.model(case)
        vae.apply_t_ops_config(case.t_ops)
        old = vae.mid_attention_batch_bytes
        if case.batch_bytes is not None:
            vae.mid_attention_batch_bytes = case.batch_bytes
        x = self.input(case)
        try:
            with torch.no_grad(), recording(vae) as rec:
                with (mutant(vae) if mutant is not None else contextlib.nullcontext()):
                    out, T, H, W = vae._decode_tile(x) if case.half == "decoder" else vae._encode_tile(x)
                out = out.clone()
        finally:
            vae.mid_attention_batch_bytes = old
            vae.apply_t_ops_config(None)
        return out, (T, H, W), rec

    def note(self, kind: str, ratio: float, case: Case):
        if ratio > self.ratios.get(kind, (-1.0, ""))[0]:
            self.ratios[kind] = (ratio, case.name)

    def note_dist(self, kind: str, dist: float, case: Case):
        if dist > self.dists.get(kind, (-1.0, ""))[0]:
            self.dists[kind] = (dist, case.name)


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _cl5(rows, T, H, W, c=None):
    """channels-last rows [T H W, >= c] -> the oracle's [1, c, T, H, W] fp32 on the CPU"""
    c = rows.shape[1] if c is None else c
    return rows[:, :c].float().cpu().reshape(T, H, W, c).permute(3, 0, 1, 2)[None].contiguous()


def _rows(y5):
    """[1, C, T, H, W] -> rows [T H W, C]"""
    return y5[0].permute(1, 2, 3, 0).reshape(-1, y5.shape[1])


# ------------------------------------------------------------------------------------------------------------------ _prepare
def check_prepare(vae, sd16):
    """The weight packing of _prepare against the state dict (fp16 values): conv [Cout][27][Cin] zero-padded to (8, 64) multiples, 1x1x1
    convs as [N pad 8][K pad 64] GEMM weights, q | k | v concatenated, the sub-pixel and planes forms from their own builders."""
    from hunyuanvideo_efficiency_amd import vae_ops as V
    P = vae._prepare()
    dev = vae.device
    for k, w in sd16.items():
        if not k.endswith(".weight"):
            continue
        name, b = k[:-7], sd16[k[:-7] + ".bias"].to(dev)
        w = w.to(dev)
        if w.dim() == 5 and w.shape[-1] == 3:
            wt, bp, cip, cop = P[name]
            co, ci = w.shape[:2]
            assert (cip, cop) == (_r(ci, 64), _r(co, 8)) and tuple(wt.shape) == (cop, 27, cip), f"A prepare: {name} padded to {(cop, cip)}"
            want = torch.zeros(cop, 27, cip, dtype=F16, device=dev)
            want[:co, :, :ci] = w.permute(0, 2, 3, 4, 1).reshape(co, 27, ci)
            assert bits_equal(wt, want) and bits_equal(bp[:co], b) and not bool(bp[co:].any()), f"A prepare: {name} is not [Cout][27][Cin] of the state dict"
        elif w.dim() == 5:
            wp, bp = P[name]
            n, kk = w.shape[:2]
            want = torch.zeros(_r(n, 8), _r(kk, 64), dtype=F16, device=dev)
            want[:n, :kk] = w.reshape(n, kk)
            assert bits_equal(wp, want) and bits_equal(bp[:n], b) and not bool(bp[n:].any()), f"A prepare: {name} is not the zero-padded 1x1x1 weight"
        elif w.dim() == 1:
            assert bits_equal(P[name][0], w) and bits_equal(P[name][1], b), f"A prepare: {name}"
    for half in (("decoder", "encoder") if vae.with_encoder else ("decoder",)):
        a = half + ".mid_block.attentions.0."
        wq = torch.cat([sd16[a + n + ".weight"] for n in ("to_q", "to_k", "to_v")], 0).to(dev)
        bq = torch.cat([sd16[a + n + ".bias"] for n in ("to_q", "to_k", "to_v")], 0).to(dev)
        assert bits_equal(P[a + "qkv"][0], wq) and bits_equal(P[a + "qkv"][1], bq), "A prepare: qkv is not to_q | to_k | to_v"
        assert bits_equal(P[a + "to_out.0"][0], sd16[a + "to_out.0.weight"].to(dev)), "A prepare: to_out.0"
    for k in P:
        if k.endswith("#subpixel"):
            w_sub, table, ntap, bp, cip, cop = P[k]
            i = int(k.split("up_blocks.")[1].split(".")[0])
            tm = vae._resample_schedule()[i][1]
            mode = "exact" if ntap > (8 if tm else 12) else "fast"
            w2, t2, n2 = V.subpixel_weights(sd16[k[:-9] + ".weight"].to(dev), tm, mode, cip, cop)
            assert n2 == ntap and bits_equal(w_sub, w2) and torch.equal(table, t2), f"A prepare: {k}"
        if k.endswith("#cout4"):
            assert bits_equal(P[k][0], V.cout4_weight_fragments(sd16[k[:-6] + ".weight"].to(dev))), f"A prepare: {k}"


# ------------------------------------------------------------------------------------------------------------------ check A, single kernels
def _true_k(sd16, stage):
    """the channels of a stage's input that carry data (the rest of a K-padded operand must be zero)"""
    name = stage.split("#")[0]
    if name.endswith("attentions.0.qkv"):
        name = name[:-3] + "to_q"
    w = sd16.get(name + ".weight")
    return None if w is None or w.dim() < 2 else int(w.shape[1])


def _zero_pad_ok(x, k_true, k):
    return k_true is None or k_true >= k or not bool((x[:, k_true:k].contiguous().view(torch.int16) != 0).any())


def affine_error(x, aff, w, b, groups, eps) -> float:
    """the affine comparison of tests/test_gpu_groupnorm_conditioning.py over every row, with the launch's own groups and eps (that these
    are 32 and 1e-6 is the trace's business)"""
    from tests.test_gpu_groupnorm_conditioning import affine_error as shared
    assert bool(torch.isfinite(aff).all()), "non-finite affine"
    return float(shared(x, aff, w, b, None, groups, eps)[0])


def _within(got, y64, bound, what) -> float:
    """RB.check, with an exact result counting as ratio 0 where the bound itself is 0 (the zero rows and columns of a padded operand)"""
    exact = got.double().to(y64.device) == y64
    return RB.check(got, y64, torch.where(exact & (bound == 0), torch.ones_like(bound), bound), what)


def _eb(got, ref: EB.Ref, dtype, what, res=None):
    """res: out = fp16(res + fp16(y)) - the bound of y, plus one fp16 ulp of the sum"""
    if res is None:
        return _within(got, ref.y, ref.bound(dtype), what)
    y = ref.y + res.double()
    return _within(got, y, ref.bound(dtype) + EB.ulp_out(y, dtype), what)


def check_call(c: Call, sd16) -> tuple:
    """One recorded kernel launch against its fp64 restatement on its own operands.  Returns (kind, error / bound)."""
    t, kw, name, out = c.t, c.kw, c.name, c.out
    what = f"A {name} [{c.stage}] (call {c.idx})"
    if name == "latent_tile":
        z = t["z"]
        ch = z.shape[0]
        want = z.permute(1, 2, 3, 0).reshape(-1, ch).to(F16)
        assert out.shape == (want.shape[0], kw["cpad"]) and bits_equal(out[:, :ch], want), f"{what}: not fp16 of the fp32 value, channels-last"
        assert not bool((out[:, ch:].contiguous().view(torch.int16) != 0).any()), f"{what}: padding columns not zero"
        return "latent_tile (bits)", 0.0
    if name == "gemm_f16":
        k = t["a"].shape[1] if kw["k"] is None else kw["k"]
        n = t["w"].shape[0] if kw["n"] is None else kw["n"]
        assert _zero_pad_ok(t["a"], _true_k(sd16, c.stage), k), f"{what}: the K padding of the operand is not zero"
        ref = EB.gemm_ref(t["a"][:, :k], t["w"][:n, :k], None if t.get("bias") is None else t["bias"][:n])
        if kw["out_f32"]:
            return "gemm_f16 (fp32 out)", _eb(out[:, :n], ref, F32, what)
        if t.get("res") is not None:
            return "gemm_f16 (+ res)", _eb(out[:, :n], ref, F16, what, t["res"][:, :n])
        return "gemm_f16", _eb(out[:, :n], ref, F16, what)
    if name in ("conv3d_causal", "conv3d_causal_strided", "conv3d_upsampled_subpixel"):
        cin, cout = kw["cin"], kw["cout"]
        assert _zero_pad_ok(t["x"], _true_k(sd16, c.stage), cin), f"{what}: the channel padding of the source is not zero"
        if name == "conv3d_causal":
            ref = CB.conv_ref(t["x"], t["w"], t["bias"], kw["T"], kw["H"], kw["W"], cin, cout, kw["up_t"], kw["up_hw"])
            kind = "conv3d_causal" + (" (upsample)" if kw["up_t"] or kw["up_hw"] else "") + (" (+ res)" if t.get("res") is not None else "")
            if t.get("res") is not None:
                return kind, _eb(out, ref, F16, what, t["res"][:, :cout])
        elif name == "conv3d_causal_strided":
            stride = tuple(int(v) for v in kw["stride"])
            src = (kw["sT"], kw["sH"], kw["sW"])
            T, H, W = CB.out_grid(src, stride)
            assert kw["ret_geom"] == (T, H, W), f"{what}: returns the grid {kw['ret_geom']}"
            ref = CB.conv_ref(t["x"], t["w"], t["bias"], T, H, W, cin, cout, stride=stride, src=src)
            kind = "conv3d_causal_strided"
        else:
            from tests.test_gpu_gemm_conv_edges import subpixel_ref
            ref = subpixel_ref(t["x"], t["w"], t["table"], kw["ntap"], t["bias"], kw["sT"], kw["sH"], kw["sW"], cin, cout, kw["up_t"])
            kind = "conv3d_upsampled_subpixel"
        assert out.shape == ref.y.shape, f"{what}: output {tuple(out.shape)}, expected {tuple(ref.y.shape)}"
        return kind, _eb(out, ref, F16, what)
    if name == "conv_cout4":
        w = sd16[c.stage.split("#")[0] + ".weight"].to(out.device)
        b = sd16[c.stage.split("#")[0] + ".bias"].to(out.device)
        h, au, share = CB.cout4_act(t["x"][:, :kw["cin"]], t.get("affine"), bool(kw["silu"]))
        assert share <= CB.AMBIGUOUS_SHARE_LIMIT, f"{what}: {share:.4f} of the activations are ambiguous"
        c.kw["ambiguous_share"] = share
        y, bound = CB.cout4_ref(h, au, w, b, kw["T"], kw["H"], kw["W"])
        assert not bool((out[:, kw["cout"]:].contiguous().view(torch.int16) != 0).any()), f"{what}: columns [Cout, 8) not zero"
        return "conv_cout4", RB.check(out[:, :kw["cout"]], y, bound, what)
    if name == "groupnorm_affine":
        err = affine_error(t["x"], out, t["weight"], t["bias"], kw["groups"], kw["eps"])
        assert err <= GN_AFFINE_TOL, f"{what}: affine error {err:.3e} (bound 2e-4 (1 + |y|))"
        return "groupnorm_affine", err / GN_AFFINE_TOL
    if name == "groupnorm_affine_from_stats":
        assert c.producer is not None, f"B(i) {what}: statistics that no recorded conv produced"
        err = affine_error(c.producer.out, out, t["weight"], t["bias"], kw["groups"], kw["eps"])
        assert err <= GN_AFFINE_TOL, f"B(ii) {what}: affine error {err:.3e} against the fp64 affine of the producing conv's output (bound 2e-4 (1 + |y|))"
        return "groupnorm_affine_from_stats", err / GN_AFFINE_TOL
    if name == "groupnorm_apply":
        y, bound = RB.gn_apply_ref(t["x"], t["affine"], bool(kw["silu"]))
        return "groupnorm_apply", RB.check(out, y, bound, what)
    if name == "softmax_rows":
        S, cols, pad, cb = t["S"], kw["cols"], kw["cols_pad"], kw["causal_block"]
        r = torch.arange(S.shape[0], device=S.device)
        valid = torch.clamp((r // cb + 1) * cb, max=cols) if cb > 0 else torch.full_like(r, cols)
        p, bound = RB.softmax_ref(S[:, :cols], valid, kw["scale"])
        behind = torch.arange(pad, device=S.device)[None] >= valid[:, None]
        assert not bool(((out[:, :pad].contiguous().view(torch.int16) != 0) & behind).any()), f"{what}: cells behind the valid keys are not +0"
        return "softmax_rows", RB.check(out[:, :cols], p, bound, what)
    if name == "transpose_16b":
        rr, cc = t["src"].shape
        assert bits_equal(out[:cc, :rr], t["src"].T), f"{what}: not the bit-equal transpose"
        assert not bool((out[:, rr:].contiguous().view(torch.int16) != 0).any()), f"{what}: columns behind the rows are not zero"
        return "transpose_16b (bits)", 0.0
    if name == "copy4d_":
        assert bits_equal(out, t["src"]), f"{what}: not a bit copy"
        return "copy4d_ (bits)", 0.0
    if name == "temporal_nearest_up":
        T, HW, s = kw["T"], kw["HW"], kw["s"]
        x = t["x"]
        want = x.reshape(T, 1, HW, x.shape[1]).expand(T, s, HW, x.shape[1]).reshape(T * s * HW, x.shape[1])
        assert kw["ret_geom"] == (T * s,) and bits_equal(out, want), f"{what}: not every frame repeated {s} times"
        return "temporal_nearest_up (bits)", 0.0
    if name == "temporal_linear_up":
        T, HW, s = kw["T"], kw["HW"], kw["s"]
        y, bound = TB.tinterp_ref(t["x"], T, HW, s)
        cp = TB.copies(T, s).to(out.device)
        t0 = TB.frames(T, s)[0].to(out.device)
        x3, o3 = t["x"].reshape(T, HW, -1), out.reshape(T * s, HW, -1)
        assert kw["ret_geom"] == (T * s,) and bits_equal(o3[cp], x3[t0[cp]]), f"{what}: a frame with lambda = 0 or t0 = t1 is not a bit copy"
        return "temporal_linear_up", RB.check(out, y, bound, what)
    if name == "temporal_avg_pool":
        T, HW, k, s = kw["T"], kw["HW"], kw["k"], kw["s"]
        y, bound = RB.temporal_avg_ref(t["x"], T, HW, k, s)
        assert kw["ret_geom"] == ((T - 1) // s + 1,) and out.shape == y.shape, f"{what}: {tuple(out.shape)} rows for T_out {(T - 1) // s + 1}"
        share = RB.mismatch_share(out, y, F16)
        assert share <= TB.mismatch_cap(out.numel()), f"{what}: {share:.4f} of the outputs are not the correctly rounded fp16 mean"
        return "temporal_avg_pool", RB.check(out, y, bound, what)
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------------------------ check A, composites
def _composite(h: Harness, case: Case, kind: str, what: str, got_rows, fn, assert_ok=True) -> float:
    """fn(precision, dtype) -> the oracle's rows of the stage on the stage's own input.  Tolerance: 4 x max |oracle(fp16 contract) -
    oracle(fp64)|, floored at 2 fp16 ulps of the largest |y|; the code under test does not enter it."""
    y16, y64 = fn(E, F32).double(), fn(VR.FP32, F64).double()
    got = got_rows.double().cpu()
    assert got.shape == y16.shape, f"A {what}: output {tuple(got.shape)}, the oracle's {tuple(y16.shape)}"
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(y16).all()), f"A {what}: not finite"
    dist = float((y16 - y64).abs().max())
    ymax = float(y64.abs().max())
    floor = COMPOSITE_FLOOR_ULPS * float(EB.ulp_out(torch.tensor(ymax, dtype=F64), F16))
    tol = max(COMPOSITE_FACTOR * dist, floor)
    ratio = float((got - y16).abs().max()) / tol
    if assert_ok:
        h.note_dist(kind, dist / max(ymax, 1e-30), case)
        h.note("composite " + kind, ratio, case)
        assert ratio <= 1.0, (f"A {what}: max |stage - oracle| = {ratio * tol:.4e} is {ratio:.2f} x the tolerance {tol:.4e} "
                              f"(oracle fp16 contract to fp64: {dist:.4e}, largest |y| {ymax:.3f})")
    return ratio


def check_composites(h: Harness, case: Case, rec: Recording, assert_ok=True) -> Dict[str, float]:
    """resnet, mid_attention, upsampler, downsampler, tail, post_quant_conv / quant_conv: each on its own recorded input."""
    sd32 = h.sd(case)
    sd64 = h.sd(case, F64)
    pick = lambda dt: sd32 if dt == F32 else sd64
    ratios = {}
    rec.composites = {}             # kind -> how many ran: check_case compares it with expected_composites

    def put(kind, r):
        ratios[kind] = max(ratios.get(kind, 0.0), r)
        rec.composites[kind] = rec.composites.get(kind, 0) + 1

    # geometry of every method stage from the kernels under it: the T, H, W arguments the host passed
    for s in rec.stages:
        if s.name == "_resnet":
            x, T, H, W = s.args[0], s.args[1], s.args[2], s.args[3]
            cin = sd32[s.pre + "norm1.weight"].shape[0]
            x5 = _cl5(x, T, H, W, cin)
            got = s.out[0] if isinstance(s.out, tuple) else s.out
            fn = lambda p, dt, x5=x5, pre=s.pre: _rows(VR.resnet_block(pick(dt), pre, x5.to(dt), p))
            put("resnet", _composite(h, case, "resnet", f"resnet {s.pre}", got, fn, assert_ok))
            s.checked += 1
        elif s.name == "_mid_attention":
            x, T, HW = s.args
            x5 = _cl5(x, T, HW, 1)
            fn = lambda p, dt, x5=x5, pre=s.pre: _rows(VR.mid_attention(pick(dt), pre, x5.to(dt), p))
            path = "batched" if any(c.kw["causal_block"] > 0 for c in rec.calls[s.first:s.last] if c.name == "softmax_rows") else "per-frame"
            put("mid_attention " + path, _composite(h, case, "mid_attention " + path, f"mid_attention {s.pre} ({path})", s.out, fn, assert_ok))
            s.checked += 1
    for c in rec.calls:
        t, kw, st = c.t, c.kw, c.stage
        if "upsamplers" in st and c.name in ("conv3d_causal", "conv3d_upsampled_subpixel"):
            name = st.split("#")[0]
            if c.name == "conv3d_causal":
                src = ((kw["T"] + 1) // 2 if kw["up_t"] else kw["T"], kw["H"] >> int(kw["up_hw"]), kw["W"] >> int(kw["up_hw"]))
                fac = (2 if kw["up_t"] else 1, 2 if kw["up_hw"] else 1, 2 if kw["up_hw"] else 1)
                form = "27-tap"
            else:
                src, fac, form = (kw["sT"], kw["sH"], kw["sW"]), (2 if kw["up_t"] else 1, 2, 2), "sub-pixel " + case.subpixel
            cin = sd32[name + ".weight"].shape[1]
            x5 = _cl5(t["x"], *src, cin)
            fn = lambda p, dt, x5=x5, name=name, fac=fac: _rows(VR.causal_conv3d(VR.upsample_causal(x5.to(dt), fac), pick(dt)[name + ".weight"],
                                                                                 pick(dt)[name + ".bias"], p))
            put("upsampler " + form, _composite(h, case, "upsampler " + form, f"upsampler {name} ({form})", c.out, fn, assert_ok))
        elif c.name == "conv3d_causal_strided":
            cin = sd32[st + ".weight"].shape[1]
            x5 = _cl5(t["x"], kw["sT"], kw["sH"], kw["sW"], cin)
            stride = tuple(int(v) for v in kw["stride"])
            fn = lambda p, dt, x5=x5, st=st, stride=stride: _rows(VE.causal_conv3d_strided(x5.to(dt), pick(dt)[st + ".weight"],
                                                                                          pick(dt)[st + ".bias"], stride, p))
            put("downsampler", _composite(h, case, "downsampler", f"downsampler {st} stride {stride}", c.out, fn, assert_ok))
        elif c.name == "gemm_f16" and st in ("post_quant_conv", "quant_conv"):
            n, k = sd32[st + ".weight"].shape[:2]
            a5 = t["a"][:, :k].float().cpu().T.reshape(1, k, -1, 1, 1)
            fn = lambda p, dt, a5=a5, st=st: _rows(p.r(F.conv3d(p.r(a5.to(dt)), p.r(pick(dt)[st + ".weight"]), p.r(pick(dt)[st + ".bias"]))))
            put(st, _composite(h, case, st, st, c.out[:, :n], fn, assert_ok))
        elif c.name == "conv_cout4":
            pre = st.split("conv_out")[0]
            x5 = _cl5(t["x"], kw["T"], kw["H"], kw["W"], kw["cin"])
            put("tail planes", _composite(h, case, "tail planes", "tail (planes)", c.out[:, :kw["cout"]], _tail_fn(pick, pre, x5), assert_ok))
    # the tail in its GEMM form: _gn(conv_norm_out) followed by the conv_out conv
    for tail_gn in [s for s in rec.stages_of("_gn") if s.pre == "decoder.conv_norm_out"]:
        conv = [c for c in rec.calls if c.stage == "decoder.conv_out.conv" and c.name == "conv3d_causal"]
        assert len(conv) == 1 and _same(conv[0].ref["x"], tail_gn.out_ref), "C the conv_out conv does not read the output of conv_norm_out"
        kw = conv[0].kw
        cin = sd32["decoder.conv_norm_out.weight"].shape[0]
        x5 = _cl5(tail_gn.args[0], kw["T"], kw["H"], kw["W"], cin)
        put("tail gemm", _composite(h, case, "tail gemm", "tail (GroupNorm apply + conv)", conv[0].out[:, :3], _tail_fn(pick, "decoder.", x5), assert_ok))
    return ratios


def _tail_fn(pick, pre, x5):
    def fn(p, dt):
        sd = pick(dt)
        hh = VR.group_norm_silu(x5.to(dt), sd[pre + "conv_norm_out.weight"], sd[pre + "conv_norm_out.bias"])
        return _rows(VR.causal_conv3d(hh, sd[pre + "conv_out.conv.weight"], sd[pre + "conv_out.conv.bias"], p))
    return fn


# ------------------------------------------------------------------------------------------------------------------ check B
def consumer_of(rec: Recording, aff_call: Call) -> Optional[Call]:
    """the groupnorm_apply / conv_cout4 launch that was given the affine `aff_call` returned"""
    for c in rec.calls[aff_call.idx + 1:]:
        if c.name in ("groupnorm_apply", "conv_cout4") and c.ref.get("affine") is aff_call.out_ref:
            return c
    return None


def check_handoff(h: Harness, case: Case, vae, rec: Recording):
    """B (i) identity, (iii) the same GroupNorm without the hand-off on the same tensor, and the hand-written site set.  (ii) is the
    single-kernel check of groupnorm_affine_from_stats in check_call."""
    from hunyuanvideo_efficiency_amd import vae_ops as V
    sites = set()
    for c in rec.of("groupnorm_affine_from_stats"):
        what = f"[{c.stage}] (call {c.idx})"
        sites.add(c.stage)
        user = consumer_of(rec, c)
        assert user is not None, f"B {what}: the affine from statistics is never applied"
        prod = c.producer
        assert prod is not None, f"B(i) {what}: statistics that no recorded conv produced"
        assert _same(prod.out_ref, user.ref["x"]) and bits_equal(prod.out, user.t["x"]), \
            f"B(i) {what}: the statistics come from {prod!r}, whose output is not the tensor being normalised"
        assert (c.kw["st_M"], c.kw["st_C"]) == tuple(user.t["x"].shape), f"B(i) {what}: statistics of {(c.kw['st_M'], c.kw['st_C'])} for {tuple(user.t['x'].shape)}"
        # (iii): the product's own pass over the tensor (hand-off disabled) gives the same normalised values within the same bound
        plain = V.groupnorm_affine(user.t["x"], c.t["weight"], c.t["bias"], 32, 1e-6)
        x64 = user.t["x"].double()
        y_s = x64 * c.out[:, 0].double() + c.out[:, 1].double()
        y_p = x64 * plain[:, 0].double() + plain[:, 1].double()
        err = float(((y_s - y_p).abs() / (1.0 + y_p.abs())).max())
        h.note("hand-off vs own pass / 2e-4", err / GN_AFFINE_TOL, case)
        assert err <= GN_AFFINE_TOL, f"B(iii) {what}: hand-off and own pass differ by {err:.3e} (1 + |y|)"
    for c in rec.of("groupnorm_affine"):
        assert c.stage not in sites, f"B [{c.stage}]: both paths at one site"
    want = set(case.handoff)
    assert sites == want, f"B hand-off sites: unexpected {sorted(sites - want)}, missing {sorted(want - sites)}"
    # every statistics buffer a conv took is consumed (none taken for nothing), and only by one site
    taken = [c for c in rec.calls if c.name in ("conv3d_causal", "conv3d_upsampled_subpixel") and c.kw["gn_stats"]]
    used = [c.producer for c in rec.of("groupnorm_affine_from_stats")]
    assert {id(c) for c in taken} == {id(c) for c in used} and len(used) == len(set(map(id, used))), \
        f"B hand-off: statistics taken by {sorted(c.stage for c in taken if c not in used)} are never consumed"


def check_handoff_disabled(h: Harness, case: Case, out, rec: Recording):
    """B(iii), whole run: with _conv patched to drop gn_stats no site hands off, the trace is otherwise the same and every stage output
    stays within the composite tolerance of ITS OWN input - so the output of the two runs is the same function, stage by stage."""
    def no_stats(vae):
        inner = vae._conv

        def _conv(P, name, x, T, H, W, up_t=False, up_hw=False, res=None, gn_stats=False):
            y = inner(P, name, x, T, H, W, up_t, up_hw, res, False)
            return (y, None) if gn_stats else y

        V = _V()                        # the sub-pixel upsampler is not called through _conv
        sub_inner = V.conv3d_upsampled_subpixel

        def conv3d_upsampled_subpixel(*args, **kwargs):
            b = dict(DEFAULTS["conv3d_upsampled_subpixel"])
            b.update(zip(KERNELS["conv3d_upsampled_subpixel"], args))
            b.update(kwargs)
            wanted, b["gn_stats"] = b["gn_stats"], False
            y = sub_inner(*[b[k] for k in KERNELS["conv3d_upsampled_subpixel"]])
            return (y, None) if wanted else y
        return _both(_patch(vae, "_conv", _conv), _patch(V, "conv3d_upsampled_subpixel", conv3d_upsampled_subpixel))
    out2, thw2, rec2 = h.run(case, mutant=no_stats)
    left = [c.stage for c in rec2.of("groupnorm_affine_from_stats")]
    assert not left, f"B(iii): hand-offs although no conv takes statistics: {left}"

    def strip(tr):      # all but the statistics: the conv's own flag (the fourth) and the GroupNorm's source (its first)
        return [(st, form, geom, fl[:3] if form in ("27tap", "subpixel") else fl[1:] if form == "gn" else fl) for st, form, geom, fl in tr]
    assert strip(trace_of(rec)) == strip(trace_of(rec2)), "B(iii): the run without hand-off takes another path"
    for a, b in zip(rec.stages_of("_gn"), rec2.stages_of("_gn")):
        if bits_equal(a.args[0], b.args[0]):            # the same input in both runs: outputs within the GroupNorm apply bound of each other
            aff = [c for c in rec2.calls[b.first:b.last] if c.name.startswith("groupnorm_affine")][0]
            y, bound = RB.gn_apply_ref(a.args[0], aff.out, bool(a.kw.get("silu", True)))
            slack = GN_AFFINE_TOL * (1.0 + y.abs())
            RB.check(a.out, y, bound + slack, f"B(iii) [{a.pre}] hand-off output against the affine of the own pass")
    check_composites(h, case, rec2)
    return out2


# ------------------------------------------------------------------------------------------------------------------ check C
def conv_form(case: Case, name: str, cin: int, cout: int, sp: bool) -> str:
    """the documented rule of _prepare: sub-pixel for a spatial upsampler with Cin (padded to 64) a power of two >= 256 and Cout > 128 unless
    HV_VAE_SUBPIXEL=off; planes for conv_out with Cout <= 3, Cin <= 128 and Cin % 32 == 0 unless HV_VAE_CONV_OUT=gemm"""
    cip, cop = _r(cin, 64), _r(cout, 8)
    if "upsamplers" in name and case.subpixel != "off" and sp and cip >= 256 and (cip & (cip - 1)) == 0 and cop > 128:
        return "subpixel"
    if name.endswith("conv_out.conv") and name.startswith("decoder") and case.conv_out == "planes" and cout <= 3 and cin <= 128 and cin % 32 == 0:
        return "planes"
    return "27tap"


def trace_of(rec: Recording) -> list:
    """(stage, form, geometry, flags) of every launch outside the attention; the attention as one entry"""
    tr = []
    att = {s.first: s for s in rec.stages_of("_mid_attention")}
    for c in rec.calls:
        kw = c.kw
        if c.idx in att:
            s = att[c.idx]
            path = "batched" if any(x.kw["causal_block"] > 0 for x in rec.calls[s.first:s.last] if x.name == "softmax_rows") else "per-frame"
            tr.append((s.pre, "attention", (s.args[1], s.args[2]), (path,)))
        if "_mid_attention" in c.inside or c.name in ("copy4d_", "groupnorm_apply"):
            continue
        if c.name == "latent_tile":
            tr.append(("latent_tile", "latent_tile", tuple(c.t["z"].shape[1:]), (kw["cpad"],)))
        elif c.name == "gemm_f16":
            tr.append((c.stage, "gemm", (c.t["a"].shape[0],), (c.t.get("res") is not None,)))
        elif c.name == "conv3d_causal":
            tr.append((c.stage, "27tap", (kw["T"], kw["H"], kw["W"]), (bool(kw["up_t"]), bool(kw["up_hw"]), c.t.get("res") is not None, bool(kw["gn_stats"]))))
        elif c.name == "conv3d_upsampled_subpixel":
            T2 = 2 * kw["sT"] - 1 if kw["up_t"] else kw["sT"]
            tr.append((c.stage.split("#")[0], "subpixel", (T2, 2 * kw["sH"], 2 * kw["sW"]), (bool(kw["up_t"]), True, False, bool(kw["gn_stats"]))))
        elif c.name == "conv3d_causal_strided":
            tr.append((c.stage, "strided", kw["ret_geom"], tuple(int(v) for v in kw["stride"])))
        elif c.name == "conv_cout4":
            tr.append((c.stage.split("#")[0], "planes", (kw["T"], kw["H"], kw["W"]), (bool(kw["silu"]), c.t.get("affine") is not None)))
        elif c.name in ("groupnorm_affine", "groupnorm_affine_from_stats"):
            user = consumer_of(rec, c)
            rows = kw["st_M"] if c.name.endswith("stats") else c.t["x"].shape[0]
            tr.append((c.stage, "gn", (rows,), ("stats" if c.name.endswith("stats") else "pass", kw["groups"], kw["eps"],
                                               None if user is None else bool(user.kw["silu"]))))
        elif c.name == "temporal_avg_pool":
            tr.append(("t_pool", "pool", (kw["T"], kw["HW"]), (kw["k"], kw["s"])))
        elif c.name in ("temporal_nearest_up", "temporal_linear_up"):
            tr.append(("t_interp", "nearest" if c.name == "temporal_nearest_up" else "trilinear", (kw["T"], kw["HW"]), (kw["s"],)))
        else:
            raise KeyError(c.name)
    return tr


class _Walk:
    """the expected trace, built from the oracle's topology; T, H, W move as the reference moves them"""

    def __init__(self, case: Case, sd, vae):
        self.case, self.sd, self.tr = case, sd, []
        self.bytes = vae.mid_attention_batch_bytes if case.batch_bytes is None else case.batch_bytes

    def gn(self, name, M, silu=True):
        src = "stats" if name in self.case.handoff else "pass"
        if src == "stats":      # the launch right before a GroupNorm that takes statistics is the conv that stored its tensor
            st, form, geom, fl = self.tr[-1]
            assert form in ("27tap", "subpixel"), (name, self.tr[-1])
            self.tr[-1] = (st, form, geom, fl[:3] + (True,))
        self.tr.append((name, "gn", (M,), (src, 32, 1e-6, silu)))

    def conv(self, name, T, H, W, up_t=False, up_hw=False, res=False):
        co, ci = self.sd[name + ".weight"].shape[:2]
        form = conv_form(self.case, name, ci, co, up_hw)
        self.tr.append((name, form, (T, H, W), (up_t, up_hw, res, False)))

    def resnet(self, pre, T, H, W):
        M = T * H * W
        self.gn(pre + "norm1", M)
        self.conv(pre + "conv1.conv", T, H, W)
        self.gn(pre + "norm2", M)
        if pre + "conv_shortcut.conv.weight" in self.sd:
            self.tr.append((pre + "conv_shortcut.conv", "gemm", (M,), (False,)))
        self.conv(pre + "conv2.conv", T, H, W, res=True)

    def pool(self, T, HW, k, s):
        self.tr.append(("t_pool", "pool", (T, HW), (k, s)))
        return (T - 1) // s + 1

    def mid_block(self, pre, T, H, W, cfg):
        self.mid_in = T
        conf = VE._pool_conf(cfg if (cfg and "enable_t_pool_before_block" in cfg) else None, 2)
        for i in range(2):
            if i > 0:
                L = T * H * W
                self.tr.append((pre + "attentions.0.", "attention", (T, H * W), ("batched" if L * _r(L, 8) * 4 <= self.bytes else "per-frame",)))
            before, after, k, s = conf[i]
            if before:
                T = self.pool(T, H * W, k, s)
            self.resnet(f"{pre}resnets.{i}.", T, H, W)
            if after:
                T = self.pool(T, H * W, k, s)
        self.mid_out = T
        return T


def expected_trace(case: Case, sd, vae) -> tuple:
    """(trace, (T', H', W')) from vae_ref.decoder_config / vae_enc_ref.encoder_config and the t_ops dict"""
    w = _Walk(case, sd, vae)
    T, H, W = case.shape
    ops = (case.t_ops or {}).get(case.half, {})
    w.tr.append(("latent_tile", "latent_tile", (T, H, W), (64,)))
    if case.half == "decoder":
        w.tr.append(("post_quant_conv", "gemm", (T * H * W,), (False,)))
        pre = "decoder."
        w.conv(pre + "conv_in.conv", T, H, W)
        T = w.mid_block(pre + "mid_block.", T, H, W, ops.get("mid_block"))
        for i, (_, _, n_res, fac) in enumerate(VR.decoder_config(case.boc)):
            bc = VE._by_index(ops.get("up_blocks"), i) or {}
            eib = bc.get("enable_t_interp_before_block", [False] * n_res)
            eia = bc.get("enable_t_interp_after_block", [False] * n_res)
            sc, mode = bc.get("interp_t_scale_factor", 2), bc.get("interp_mode", "nearest")
            for j in range(n_res):
                if eib[j]:
                    w.tr.append(("t_interp", mode, (T, H * W), (sc,)))
                    T *= sc
                w.resnet(f"{pre}up_blocks.{i}.resnets.{j}.", T, H, W)
                if eia[j]:
                    w.tr.append(("t_interp", mode, (T, H * W), (sc,)))
                    T *= sc
            if fac is not None:
                ft, fh, fw = fac
                T, H, W = 1 + ft * (T - 1), H * fh, W * fw
                w.conv(f"{pre}up_blocks.{i}.upsamplers.0.conv.conv", T, H, W, up_t=ft == 2, up_hw=fh == 2)
        co, ci = sd[pre + "conv_out.conv.weight"].shape[:2]
        if conv_form(case, pre + "conv_out.conv", ci, co, False) == "planes":
            name = pre + "conv_norm_out"
            src = "stats" if name in case.handoff else "pass"
            if src == "stats":
                st, form, geom, fl = w.tr[-1]
                w.tr[-1] = (st, form, geom, fl[:3] + (True,))
            w.tr.append((name, "gn", (T * H * W,), (src, 32, 1e-6, True)))
            w.tr.append((pre + "conv_out.conv", "planes", (T, H, W), (True, True)))
        else:
            w.gn(pre + "conv_norm_out", T * H * W)
            w.conv(pre + "conv_out.conv", T, H, W)
    else:
        pre = "encoder."
        w.conv(pre + "conv_in.conv", T, H, W)
        for i, (_, _, stride) in enumerate(VE.encoder_config(case.boc)):
            bc = VE._by_index(ops.get("down_blocks"), i)
            conf = VE._pool_conf(bc if (bc and "enable_t_pool_before_block" in bc) else None, 2)
            for j in range(2):
                before, after, k, s = conf[j]
                if before:
                    T = w.pool(T, H * W, k, s)
                w.resnet(f"{pre}down_blocks.{i}.resnets.{j}.", T, H, W)
                if after:
                    T = w.pool(T, H * W, k, s)
            if stride is not None:
                if bc and "downsample_stride" in bc:
                    stride = tuple(bc["downsample_stride"])
                T, H, W = ((v - 1) // s + 1 for v, s in zip((T, H, W), stride))
                w.tr.append((f"{pre}down_blocks.{i}.downsamplers.0.conv.conv", "strided", (T, H, W), tuple(stride)))
        T = w.mid_block(pre + "mid_block.", T, H, W, ops.get("mid_block"))
        w.gn(pre + "conv_norm_out", T * H * W)
        w.conv(pre + "conv_out.conv", T, H, W)
        w.tr.append(("quant_conv", "gemm", (T * H * W,), (False,)))
    return w.tr, (T, H, W), (w.mid_in, w.mid_out)


def oracle_whole(h: Harness, case: Case) -> torch.Tensor:
    x = h.input(case).float().cpu()[None]
    sd = h.sd(case)
    if case.half == "decoder":
        return VE.decode_tile_tops(sd, x, case.boc, E, case.t_ops)
    return VE.encode_tile(sd, x, case.boc, E, case.t_ops)


def check_trace(h: Harness, case: Case, vae, out, thw, rec: Recording):
    want, thw_walk, (mid_in, mid_out) = expected_trace(case, h.sd(case), vae)
    got = trace_of(rec)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"C trace of {case.name}: launch {i} is {a}, the reference topology gives {b}"
    assert len(got) == len(want), f"C trace of {case.name}: {len(got)} launches, the reference topology gives {len(want)}"
    ref = oracle_whole(h, case)
    assert tuple(ref.shape[2:]) == tuple(thw) == tuple(thw_walk), f"C {case.name}: returns {thw}, the oracle's output is {tuple(ref.shape[2:])}"
    c_out = ref.shape[1]
    assert out.shape[0] == thw[0] * thw[1] * thw[2] and out.shape[1] >= c_out, f"C {case.name}: output {tuple(out.shape)}"
    err = float((out[:, :c_out].float().cpu() - _rows(ref)).abs().max() / ref.abs().max())
    print(f"[vae wiring] {case.name}: whole output vs oracle {err:.3e} of range (information; the stage checks carry the assertions)")
    # the data path: every stage reads what the stage before it returned
    mids = rec.stages_of("_mid_block")
    assert len(mids) == 1, f"C {case.name}: {len(mids)} mid blocks"
    for s in mids:          # takes mid_in frames, returns the frames the reference's pools leave, and the tensor its last launch stored
        assert (s.args[1], s.out[1]) == (mid_in, mid_out), f"C {s.pre}: T {s.args[1]} -> {s.out[1]}, the reference topology gives {mid_in} -> {mid_out}"
        assert bits_equal(s.out[0], rec.calls[s.last - 1].out), f"C {s.pre}: does not return what its last launch stored"
        s.checked += 1
    for s in rec.stages_of("_gn"):
        app = [c for c in rec.calls[s.first:s.last] if c.name == "groupnorm_apply"]
        assert len(app) == 1 and bits_equal(app[0].out, s.out) and bits_equal(app[0].t["x"], s.args[0]), f"C _gn {s.pre}: not one apply of its input"
        assert (s.kw.get("stats") is not None) == (s.pre in case.handoff), f"B _gn {s.pre}: statistics {'given' if s.kw.get('stats') is not None else 'not given'}"
        s.checked += 1
    check_data_path(case, rec)
    return want


def check_data_path(case: Case, rec: Recording):
    """C, identity along the chain: every unit of the tile coder - a resnet, the attention, a GroupNorm outside both, or a launch outside
    all three (latent_tile, the 1x1x1 GEMMs, conv_in, pools, interpolations, up- and downsamplers, the channel padding, the tail) - reads
    the very tensor the unit before it returned (the recorder keeps every tensor alive, so an address names one tensor)."""
    outer = [s for s in rec.stages if s.name in ("_resnet", "_mid_attention")]
    units = {s.first: s for s in outer}
    for g in rec.stages_of("_gn"):
        if not any(s.first <= g.first and g.last <= s.last for s in outer):
            units[g.first] = g
    role = {"latent_tile": "z", "gemm_f16": "a", "copy4d_": "src"}
    cur, cur_name, i = None, None, 0
    while i < len(rec.calls):
        u = units.get(i)
        if u is not None:
            inp, outp, name, i = u.ref_in, (u.out_ref[0] if isinstance(u.out_ref, tuple) else u.out_ref), f"{u.name} {u.pre}", u.last
        else:
            c = rec.calls[i]
            i += 1
            if c.name == "groupnorm_affine_from_stats":         # reads no tensor: B(i) ties it to its producer
                continue
            inp, outp, name = c.ref[role.get(c.name, "x")], (None if c.name == "groupnorm_affine" else c.out_ref), repr(c)
        if cur is not None:
            assert inp.data_ptr() == cur.data_ptr() and inp.shape[-2] == cur.shape[-2], \
                f"C data path of {case.name}: {name} does not read what {cur_name} returned"
        if outp is not None:
            cur, cur_name = outp, name


def expected_composites(case: Case, want: list) -> Dict[str, int]:
    """how many composite stages of each kind the reference topology has, from the expected trace"""
    n: Dict[str, int] = {}
    for st, form, _, fl in want:
        kind = None
        if form == "gn" and st.endswith(".norm1"):
            kind = "resnet"
        elif form == "attention":
            kind = "mid_attention " + fl[0]
        elif "upsamplers" in st:
            kind = "upsampler 27-tap" if form == "27tap" else "upsampler sub-pixel " + case.subpixel
        elif form == "strided":
            kind = "downsampler"
        elif st in ("post_quant_conv", "quant_conv"):
            kind = st
        elif st == "decoder.conv_out.conv":
            kind = "tail planes" if form == "planes" else "tail gemm"
        if kind is not None:
            n[kind] = n.get(kind, 0) + 1
    return n


# ------------------------------------------------------------------------------------------------------------------ the whole case
def check_case(h: Harness, case: Case, verbose=True):
    """A, B, C and D on one case."""
    vae = h.model(case)
    sd16 = {k: v.to(F16) for k, v in h.sd(case).items()}
    key = ("prepare", case.boc, case.subpixel, case.conv_out, case.half)
    if key not in h.ran:
        check_prepare(vae, sd16)
        h.ran.add(key)
    out, thw, rec = h.run(case)
    want = check_trace(h, case, vae, out, thw, rec)
    per_kind = {}
    for c in rec.calls:
        kind, r = check_call(c, sd16)
        c.checked += 1
        per_kind[kind] = max(per_kind.get(kind, 0.0), r)
    for k, v in per_kind.items():
        h.note(k, v, case)
    for c in rec.of("conv_cout4"):
        h.note("conv_cout4: ambiguous activations / 1 %", c.kw["ambiguous_share"] / CB.AMBIGUOUS_SHARE_LIMIT, case)
    check_handoff(h, case, vae, rec)
    comp = check_composites(h, case, rec)
    assert rec.composites == expected_composites(case, want), \
        f"D {case.name}: composite stages checked {rec.composites}, the reference topology has {expected_composites(case, want)}"
    unchecked = [c for c in rec.calls if c.checked != 1] + [s for s in rec.stages if s.checked != 1]
    assert not unchecked, f"D {case.name}: {len(unchecked)} recorded calls without exactly one check: {unchecked[:8]}"
    h.ran.add(case.name)
    if verbose:
        print(f"[vae wiring] {case.name}: {len(rec.calls)} launches, {len(rec.stages)} stages; error / tolerance: "
              + ", ".join(f"{k} {v:.3f}" for k, v in {**per_kind, **{'composite ' + k: v for k, v in comp.items()}}.items()))
    return out, thw, rec


def check_second_call(h: Harness, case: Case):
    """a model that ran `case` (with t_ops), then apply_t_ops_config(None): the cached _prep and workspaces give the bits of a fresh model"""
    plain = dataclasses.replace(case, t_ops=None, name=case.name + "-cleared")
    used = h.model(case, fresh=True)
    h.run(case, vae=used)
    a, thw_a, _ = h.run(plain, vae=used)
    b, thw_b, _ = h.run(plain, vae=h.model(case, fresh=True))
    assert thw_a == thw_b and bits_equal(a, b), f"{case.name}: a second call after apply_t_ops_config(None) differs from a fresh model"


def report(h: Harness) -> str:
    lines = ["[vae wiring] largest error / tolerance per stage kind:"]
    for k in sorted(h.ratios):
        v, where = h.ratios[k]
        lines.append(f"[vae wiring]   {k:<44s} {v:.3f}  at {where}")
    lines.append("[vae wiring] composite stages: largest |oracle fp16 contract - oracle fp64| / largest |y| (the tolerance is 4 x the distance):")
    for k in sorted(h.dists):
        v, where = h.dists[k]
        lines.append(f"[vae wiring]   {k:<44s} {v:.3e}  at {where}")
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------------------------ mutants
# Each is a context manager factory taking the model; it mis-wires the host code the way a slip of the pen would, and is laid OVER the
# recorder, so a changed kernel argument is recorded as the kernel received it.
@contextlib.contextmanager
def _patch(obj, name, value):
    had = isinstance(obj, types.ModuleType) or name in vars(obj)       # an instance attribute laid over a method is deleted again
    old = getattr(obj, name)
    setattr(obj, name, value)
    try:
        yield
    finally:
        if had:
            setattr(obj, name, old)
        else:
            delattr(obj, name)


def _V():
    from hunyuanvideo_efficiency_amd import vae_ops
    return vae_ops


def _m_residual_from_normalised(vae):
    inner = vae._conv

    def _conv(P, name, x, T, H, W, up_t=False, up_hw=False, res=None, gn_stats=False):
        if res is not None and res.shape == x.shape:
            res = x                                                     # the normalised tensor instead of the block's input
        return inner(P, name, x, T, H, W, up_t, up_hw, res, gn_stats)
    return _patch(vae, "_conv", _conv)


def _m_stats_of_input(vae):
    inner = vae._resnet

    def _resnet(P, pre, x, T, H, W, x_stats=None, out_stats=False):
        ret = inner(P, pre, x, T, H, W, x_stats=x_stats, out_stats=out_stats)
        if out_stats and ret[1] is not None and ret[0].shape == x.shape:
            from tests.cpu_kernel_doubles import gn_stats_of            # (the mutants run on the CPU doubles only)
            return ret[0], gn_stats_of(x)                               # same shape: the assert in _gn cannot tell
        return ret
    return _patch(vae, "_resnet", _resnet)


def _m_stats_kept_across_t_up(vae):
    """In the product as it stands `st` is already None wherever a t_up runs: feeds_gn is False for the conv in front of one.  So the slip
    is taken together with its twin - the conv in front of the interpolation takes the statistics, and they survive it (M follows the
    tensor, which sidesteps the shape assert of _gn)."""
    from hunyuanvideo_efficiency_amd.vae_ops import GNStats
    inner = vae._resnet
    last = {}

    def _resnet(P, pre, x, T, H, W, x_stats=None, out_stats=False):
        st = last.get("st")
        if x_stats is None and st is not None and st.C == x.shape[1] and st.M != x.shape[0]:
            x_stats = GNStats(st.partial, st.rows, x.shape[0], st.C)
        y, st_out = inner(P, pre, x, T, H, W, x_stats=x_stats, out_stats=True)
        last["st"] = st_out if "up_blocks" in pre else None
        return (y, st_out) if out_stats else y
    return _patch(vae, "_resnet", _resnet)


def _m_feeds_gn_before_upsampler(vae):
    inner = vae._resnet

    def _resnet(P, pre, x, T, H, W, x_stats=None, out_stats=False):
        if pre.endswith("resnets.2.") and "up_blocks.1." in pre and not out_stats:
            return inner(P, pre, x, T, H, W, x_stats=x_stats, out_stats=True)[0]
        return inner(P, pre, x, T, H, W, x_stats=x_stats, out_stats=out_stats)
    return _patch(vae, "_resnet", _resnet)


def _m_mid_block(attention_after_pool=False, swap=False):
    def make(vae):
        V = _V()

        def _mid_block(P, pre, h, T, H, W, cfg=None):
            conf = vae._pool_conf(cfg, 2, "UNetMidBlockCausal3D")
            for i in range(2):
                before, after, k, s = conf[i]
                if swap:
                    before, after = after, before
                if i > 0 and not attention_after_pool:
                    h = vae._mid_attention(P, pre + "attentions.0.", h, T, H * W)
                if before:
                    h, T = V.temporal_avg_pool(h, T, H * W, k, s)
                if i > 0 and attention_after_pool:
                    h = vae._mid_attention(P, pre + "attentions.0.", h, T, H * W)
                h = vae._resnet(P, f"{pre}resnets.{i}.", h, T, H, W)
                if after:
                    h, T = V.temporal_avg_pool(h, T, H * W, k, s)
            return h, T
        return _patch(vae, "_mid_block", _mid_block)
    return make


def _m_mid_block_output_dropped(vae):
    inner = vae._mid_block

    def _mid_block(P, pre, h, T, H, W, cfg=None):
        inner(P, pre, h, T, H, W, cfg)
        return h, T                                                     # same shape: the next block reads the mid block's INPUT
    return _patch(vae, "_mid_block", _mid_block)


def _m_pool_defaults(vae):
    inner = type(vae)._pool_conf

    def _pool_conf(cfg, n_res, who):
        if cfg and "enable_t_pool_before_block" in cfg:
            cfg = dict({"pool_t_kernel": 3, "pool_t_stride": 1}, **cfg)
        return inner(cfg, n_res, who)
    return _patch(vae, "_pool_conf", _pool_conf)


def _m_tm_two_t(vae):
    inner = vae._conv

    def _conv(P, name, x, T, H, W, up_t=False, up_hw=False, res=None, gn_stats=False):
        if up_t:
            T = 2 * ((T + 1) // 2)                                      # T2 = 2 T instead of 1 + 2 (T - 1)
        return inner(P, name, x, T, H, W, up_t, up_hw, res, gn_stats)
    return _patch(vae, "_conv", _conv)


def _m_up_swapped(vae):
    inner = vae._conv

    def _conv(P, name, x, T, H, W, up_t=False, up_hw=False, res=None, gn_stats=False):
        if up_t != up_hw:
            up_t, up_hw = up_hw, up_t
        return inner(P, name, x, T, H, W, up_t, up_hw, res, gn_stats)
    return _patch(vae, "_conv", _conv)


def _m_block_cfg(edit):
    def make(vae):
        inner = type(vae)._block_cfg

        def _block_cfg(cfgs, i):
            c = inner(cfgs, i)
            return None if c is None else edit(dict(c))
        return _patch(vae, "_block_cfg", _block_cfg)
    return make


def _eib_after(c):
    if "enable_t_interp_before_block" in c:
        b, a = c["enable_t_interp_before_block"], c.get("enable_t_interp_after_block", [False] * 3)
        c["enable_t_interp_after_block"] = [x or y for x, y in zip(a, b)]
        c["enable_t_interp_before_block"] = [False] * len(b)
    return c


def _no_stride(c):
    c.pop("downsample_stride", None)
    return c


def _m_trilinear_by_nearest(vae):
    return _patch(vae, "_interp_op", lambda mode: _V().temporal_nearest_up)


def _m_kernel(name, edit):
    """the vae_ops entry point `name` called with arguments changed by edit(vae, bound arguments)"""
    def make(vae):
        V = _V()
        inner = getattr(V, name)

        def fn(*args, **kwargs):
            b = dict(DEFAULTS.get(name, {}))
            b.update(zip(KERNELS[name], args))
            b.update(kwargs)
            edit(vae, b)
            return inner(*[b[k] for k in KERNELS[name]])
        return _patch(V, name, fn)
    return make


def _no_silu(vae, b):
    b["silu"] = False


def _eps_of_norm_out(vae, b):
    if b["weight"].data_ptr() == vae._prepare()["decoder.conv_norm_out"][0].data_ptr():
        b["eps"] = 1e-5


def _no_pq_bias(vae, b):
    if b["w"].data_ptr() == vae._prepare()["post_quant_conv"][0].data_ptr():
        b["bias"] = None


def _previous_frame_keys(vae, b):
    hw = b["S"].shape[0]
    if not b.get("causal_block") and b["cols"] > hw:
        b["cols"] -= hw                                                 # nk of the previous frame


@contextlib.contextmanager
def _both(a, b):
    with a, b:
        yield


# name -> (factory, case, the check letters of which at least one must reject it)
MUTANTS = {
    "conv2 residual from the normalised tensor": (_m_residual_from_normalised, "A-1x2x2-off-gemm", "A"),
    "statistics of the resnet's input for the GroupNorm after its output": (_m_stats_of_input, "A-1x2x2-off-gemm", "B"),
    "st kept across a t_up": (_m_stats_kept_across_t_up, "A-tops-both", "B"),     # run_mutant: the hand-off check runs first for "B"
    "feeds_gn forced True before an upsampler": (_m_feeds_gn_before_upsampler, "A-1x2x2-off-gemm", "BC"),
    "mid attention after resnet 1's before-pool": (_m_mid_block(attention_after_pool=True), "B-midpool-mixed-k3s2-T2", "C"),
    "up_blocks.0 reads the mid block's input": (_m_mid_block_output_dropped, "A-1x2x2-off-gemm", "C"),
    "pool before/after swapped": (_m_mid_block(swap=True), "B-midpool-before-k2s2-T5", "C"),
    "pool defaults k, s = 3, 1": (_m_pool_defaults, "B-midpool-before-k2s2-T5", "C"),
    "tm upsample producing 2T frames": (_m_tm_two_t, "A-3x4x4-exact-gemm", "C"),
    "up_t / up_hw swapped": (_m_up_swapped, "A-1x2x2-off-gemm", "C"),
    "eib applied after the resnet": (_m_block_cfg(_eib_after), "A-tops-both", "BC"),
    "trilinear served by the nearest kernel": (_m_trilinear_by_nearest, "A-tops-eia-last", "C"),
    "tail without SiLU (planes)": (_m_kernel("conv_cout4", _no_silu), "A-2x3x5-fast-planes", "AC"),
    "tail without SiLU (gemm form)": (lambda vae: _patch(vae, "_gn", lambda P, name, x, silu=True, stats=None, _g=vae._gn: _g(
        P, name, x, silu=silu and name != "decoder.conv_norm_out", stats=stats)), "A-1x2x2-off-gemm", "AC"),
    "conv_norm_out eps 1e-5": (lambda vae: _both(_m_kernel("groupnorm_affine_from_stats", _eps_of_norm_out)(vae),
                                                 _m_kernel("groupnorm_affine", _eps_of_norm_out)(vae)), "A-1x2x2-off-gemm", "C"),
    "post_quant_conv bias dropped": (_m_kernel("gemm_f16", _no_pq_bias), "A-1x2x2-off-gemm", "A"),
    "downsample_stride override ignored": (_m_block_cfg(_no_stride), "B-enc-tops", "C"),
    "per-frame attention with nk of the previous frame": (_m_kernel("softmax_rows", _previous_frame_keys), "A-3x3x5-perframe", "A"),
}


def run_mutant(h: Harness, name: str) -> str:
    """Runs the mutant's case under the mutant through the checks of check_case; returns the message of the check that rejected it
    (AssertionError whose text starts with the check's letter), or raises if every check passed."""
    make, case_name, letters = MUTANTS[name]
    case = CASE[case_name]
    vae = h.model(case)
    sd16 = {k: v.to(F16) for k, v in h.sd(case).items()}
    try:
        out, thw, rec = h.run(case, mutant=make)
        if letters[0] == "B":           # B and C both see a hand-off that should not be: let the identity check speak first
            check_handoff(h, case, vae, rec)
        check_trace(h, case, vae, out, thw, rec)
        for c in rec.calls:
            check_call(c, sd16)
        check_handoff(h, case, vae, rec)
        ratios = check_composites(h, case, rec, assert_ok=False)
        bad = {k: v for k, v in ratios.items() if not v <= 1.0}
        assert not bad, f"A composite stages beyond the tolerance (error / tolerance): {bad}"
    except AssertionError as e:
        msg = str(e)
        assert msg[:1] in letters, f"mutant {name!r} was rejected, but by another check than {letters}: {msg}"
        return msg
    raise RuntimeError(f"mutant {name!r} survived every check at {case.name}")
