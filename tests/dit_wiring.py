"""TEST INFRASTRUCTURE: the DiT forward as a COMPOSITION - cases, device-agnostic checks and mutants for the host layer that wires the
kernels into the model (modules/models.py, token_refiner.py, attenion.py, layers.py: workspace row ranges [lo, hi), cu1 = s_img +
n_valid, n_rope, the per-prompt refiner cache, workspace re-keying).  The same functions run on the CPU kernel doubles
(tests/test_dit_wiring_cpu.py, where every mutant below must be rejected) and on the HIP kernels (tests/test_gpu_dit_wiring.py).

Two kinds of check:
  A  tolerance, stage by stage: every stage's OWN input (as the device held it) goes through the oracle stage in the bf16-emulated
     contract and is compared with the stage's output at the block tolerance of test_gpu_model.py::test_block_call_surfaces_vs_oracle
     (rtol 2^-6, atol 6e-2), plus the whole output at 3e-2 of its range.  No error accumulates across stages, so a mis-wired
     modulation chunk shows at full size.
  B  exact, bitwise: what a prefix mask promises.  Padding text content cannot change one bit of the image rows; the token on each
     side of cu1 is inside / outside the image's attention; table rows past n_rope are never read; repeats, re-keyed workspaces,
     the refiner cache and batch rows give the bits of a fresh single-sample run.
A check raises AssertionError; `ratios` collects error / tolerance per stage for the report."""
from __future__ import annotations

import contextlib
import dataclasses
from typing import Optional

import torch

from hunyuanvideo_efficiency_amd import synthetic as syn
from oracle import dit_ref as R

E = R.Prec(True)
BF16 = torch.bfloat16
RTOL, ATOL = 2 ** -6, 6e-2      # test_block_call_surfaces_vs_oracle: 2 bf16 ulps of |x| <= ~6
RANGE_TOL = 3e-2                # whole output, of its range (test_gpu_model.py, oracle_checks.py)


# ------------------------------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass(frozen=True)
class Case:
    thw: tuple                      # latent (T, H, W) -> s_img = T * H/2 * W/2
    s_txt: int
    n_valid: int
    mask: bool = True               # False: text_mask=None
    use_attention_mask: bool = True
    rope: bool = True               # False: freqs_cos = freqs_sin = None (n_rope = 0)
    guidance_embed: bool = True

    @property
    def s_img(self) -> int:
        t, h, w = self.thw
        return t * (h // 2) * (w // 2)

    @property
    def cu1(self) -> int:
        return self.s_img + (self.n_valid if self.mask else self.s_txt)

    @property
    def name(self) -> str:
        flags = "".join(f"-{n}" for n, on in (("nomask", not self.mask), ("noattnmask", not self.use_attention_mask),
                                             ("norope", not self.rope), ("noguidance", not self.guidance_embed)) if on)
        return f"img{self.s_img}-txt{self.s_txt}v{self.n_valid}{flags}"

    @property
    def model_kind(self) -> str:
        return "tiny" + ("" if self.guidance_embed else "-noguidance") + ("" if self.use_attention_mask else "-noattnmask")


# every s_img edge and every (s_txt, n_valid) edge once, not their product
CASES = [
    Case((1, 2, 2), 32, 11),        # image mode, one image token
    Case((3, 6, 10), 32, 31),       # under one 64-key tile, odd; a one-row padding segment
    Case((1, 16, 16), 32, 0),       # exactly one tile, n_kv = 64; no valid text: the refiner's masked mean is 0/0 (image only)
    Case((1, 16, 16), 32, 1),       # n_kv = 65
    Case((5, 16, 16), 32, 32),      # five full tiles; no padding segment
    Case((1, 2, 510), 1, 1),        # one below the 256-row GEMM tile; a single text token, valid
    Case((1, 2, 514), 1, 0),        # one above it; a single text token, padding
    Case((3, 6, 10), 9, 4),
    Case((1, 16, 16), 256, 77),     # the shipped text length and a CLIP-length prompt
    Case((3, 6, 10), 32, 32, mask=False),
    Case((3, 6, 10), 32, 11, use_attention_mask=False),
    Case((3, 6, 10), 32, 11, rope=False),
    Case((3, 6, 10), 32, 11, guidance_embed=False),
]
# the FP8-MFMA configuration (d = 512, 4 heads, 1 + 2 blocks): s_img 1, 45 and 257; n_valid 0 and s_txt
FP8_CASES = [Case((1, 2, 2), 32, 11), Case((3, 6, 10), 32, 0), Case((1, 2, 514), 32, 32), Case((3, 6, 10), 9, 4)]


def config(kind: str) -> syn.DiTConfig:
    if kind.startswith("fp8"):
        return syn.DiTConfig(hidden_size=512, heads_num=4, mm_double_blocks_depth=1, mm_single_blocks_depth=2)
    cfg = syn.tiny_config()
    cfg.guidance_embed = "-noguidance" not in kind
    return cfg


# ------------------------------------------------------------------------------------------------------------------ harness
class Harness:
    """Models, inputs and oracle weights for one device.  On "cpu" the caller has installed tests/cpu_kernel_doubles.py on ops."""

    def __init__(self, device):
        self.dev = device
        self._models = {}
        self.ratios = {}            # stage -> (largest error / tolerance, case name)

    def model(self, kind: str = "tiny", fresh: bool = False):
        if not fresh and kind in self._models:
            return self._models[kind]
        from hunyuanvideo_efficiency_amd.builders import build_model
        model = build_model(config(kind), self.dev)
        model.use_attention_mask = "-noattnmask" not in kind
        if kind.startswith("fp8"):
            from hunyuanvideo_efficiency_amd.modules.fp8_optimization import convert_fp8_linear, enable_fp8_mfma
            convert_fp8_linear(model, None, BF16)
            assert enable_fp8_mfma(model) == 3
        model.wiring_kind = kind
        if not fresh:
            self._models[kind] = model
        return model

    def oracle_weights(self, model):
        """(state dict for the oracle, its Prec): bf16 weights as fp32; FP8 layers registered with the quantisation-aware Prec"""
        hit = getattr(model, "_wiring_sd", None)
        if hit is None:
            sd = {k: p.float().cpu() for k, p in model.state_dict().items()}
            prec = E
            if model.wiring_kind.startswith("fp8"):
                prec = R.Fp8MfmaPrec()
                for name, layer in model.named_modules():
                    if hasattr(layer, "fp8_scale"):
                        sd[name + ".weight"] = prec.fp8(layer.weight.cpu(), layer.fp8_scale.cpu())
            hit = model._wiring_sd = (sd, prec)
        return hit

    def inputs(self, case: Case, kind: Optional[str] = None, seed: int = 0) -> dict:
        """Forward arguments on the device: fresh tensor objects on every call (the refiner cache hangs on text_states)."""
        cfg = config(kind or case.model_kind)
        x, ts, tm, ts2 = syn.synth_dit_inputs(cfg, case.thw, case.s_txt, case.n_valid, seed=seed)
        t, h, w = case.thw
        cos, sin = R.rope_tables([t, h // 2, w // 2], cfg.rope_dim_list, 256.0) if case.rope else (None, None)
        inp = dict(x=x, t=torch.tensor([997.093]), text_states=ts.to(BF16), text_mask=tm if case.mask else None, text_states_2=ts2,
                   freqs_cos=cos, freqs_sin=sin, guidance=torch.tensor([6016.0]) if cfg.guidance_embed else None)
        return {k: None if v is None else v.clone().to(self.dev) for k, v in inp.items()}

    def run(self, model, inp: dict) -> torch.Tensor:
        with torch.no_grad():
            out = model(inp["x"], inp["t"], text_states=inp["text_states"], text_mask=inp["text_mask"],
                        text_states_2=inp["text_states_2"], freqs_cos=inp["freqs_cos"], freqs_sin=inp["freqs_sin"],
                        guidance=inp["guidance"], return_dict=False)
        return out.clone()

    def run_traced(self, model, inp: dict):
        with traced(model) as rec:
            out = self.run(model, inp)
        return out, rec

    def note(self, stage: str, ratio: float, case: Case):
        if ratio > self.ratios.get(stage, (-1.0, ""))[0]:
            self.ratios[stage] = (ratio, case.name)


def clone_inputs(inp: dict) -> dict:
    return {k: None if v is None else v.clone() for k, v in inp.items()}


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """same shape and the same bf16 bit patterns (NaN payloads included)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


@contextlib.contextmanager
def traced(model):
    """Wrap img_in.run, txt_in.run, every block's run and final_layer.run ON THE INSTANCES; each call appends
    {name, args, x_in, x_out}: the residual stream ws.x cloned around the call (vec, cu1 and the tables are in args)."""
    rec = []
    stages = [("patch_embed", model.img_in), ("token_refiner", model.txt_in)]
    stages += [(f"double_block.{i}", b) for i, b in enumerate(model.double_blocks)]
    stages += [(f"single_block.{i}", b) for i, b in enumerate(model.single_blocks)]
    stages += [("final_layer", model.final_layer)]

    def wrap(name, obj):
        inner = obj.run

        def run(*args, **kwargs):
            x_in = model._ws.x.clone()
            ret = inner(*args, **kwargs)
            rec.append(dict(name=name, args=tuple(a.clone() if torch.is_tensor(a) else a for a in args), x_in=x_in,
                            x_out=model._ws.x.clone()))
            return ret
        obj.run = run

    for name, obj in stages:
        wrap(name, obj)
    try:
        yield rec
    finally:
        for _, obj in stages:
            del obj.run


# ------------------------------------------------------------------------------------------------------------------ oracle
def _cu(case: Case) -> torch.Tensor:
    return torch.tensor([0, case.cu1, case.s_img + case.s_txt], dtype=torch.int32)


def _refiner_mask(case: Case, inp: dict):
    return inp["text_mask"].cpu() if (case.mask and case.use_attention_mask) else None


def _cpu(inp: dict) -> dict:
    return {k: None if v is None else v.float().cpu() if v.is_floating_point() else v.cpu() for k, v in inp.items()}


def oracle_forward(sd, cfg, case: Case, inp: dict, prec) -> torch.Tensor:
    """R.dit_forward with the two switches it does not have: text_mask=None (one segment, unmasked refiner) and
    use_attention_mask=False (unmasked refiner, cu_seqlens still from the mask: models.py:637-648 of the reference)."""
    c = _cpu(inp)
    t, h, w = case.thw
    vec = R.dit_vec(sd, c["t"], c["text_states_2"], c["guidance"], prec)
    img = R.patch_embed(sd, c["x"], prec)
    txt = R.token_refiner(sd, "txt_in.", c["text_states"], c["t"], _refiner_mask(case, inp), cfg.heads_num, prec, cfg.refiner_depth)
    cu, cos, sin = _cu(case), c["freqs_cos"], c["freqs_sin"]
    for i in range(cfg.mm_double_blocks_depth):
        img, txt = R.double_block(sd, f"double_blocks.{i}.", img, txt, vec, cu, cos, sin, cfg.heads_num, prec)
    xs = torch.cat([img, txt], 1)
    for i in range(cfg.mm_single_blocks_depth):
        xs = R.single_block(sd, f"single_blocks.{i}.", xs, vec, case.s_txt, cu, cos, sin, cfg.heads_num, prec)
    out = R.final_layer(sd, xs[:, :case.s_img], vec, prec)
    return R.unpatchify(out, t, h // 2, w // 2, cfg.out_channels, cfg.patch_size)


def _ratio(got: torch.Tensor, ref: torch.Tensor, what: str) -> float:
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(ref).all()), f"{what}: the oracle is not finite"
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    return float(((got - ref).abs() / (ATOL + RTOL * ref.abs())).max())


def range_error(out: torch.Tensor, ref: torch.Tensor) -> float:
    out, ref = out.float().cpu(), ref.float().cpu()
    assert bool(torch.isfinite(out).all()), "the image output is not finite"
    return float((out - ref).abs().max() / ref.abs().max())


# ------------------------------------------------------------------------------------------------------------------ check A
def check_stages(h: Harness, model, case: Case, inp: dict, out: torch.Tensor, rec: list, verbose: bool = True,
                 assert_ok: bool = True) -> dict:
    """Every stage on the device's own input against the oracle stage (Prec(True)); returns {stage: error / tolerance}.
    assert_ok=False (the mutant tests, which ask by how much a stage is off) only returns them."""
    cfg = config(case.model_kind)
    sd, _ = h.oracle_weights(model)
    c = _cpu(inp)
    s_img, heads = case.s_img, cfg.heads_num
    t, hh, w = case.thw
    text_rows = case.n_valid > 0 or not case.mask       # n_valid = 0: the text rows are NaN (0/0), as in the reference; image only
    cu, cos, sin = _cu(case), c["freqs_cos"], c["freqs_sin"]
    names = [r["name"] for r in rec]
    want = (["patch_embed", "token_refiner"] + [f"double_block.{i}" for i in range(cfg.mm_double_blocks_depth)]
            + [f"single_block.{i}" for i in range(cfg.mm_single_blocks_depth)] + ["final_layer"])
    assert names == want, names
    ratios = {}
    blocks = [r for r in rec if "block" in r["name"]]
    vec = blocks[0]["args"][3]
    assert all(bits_equal(r["args"][3], vec) for r in blocks) and bits_equal(rec[-1]["args"][2], vec), "vec differs between stages"
    assert all(r["args"][4] == case.cu1 for r in blocks), ([r["args"][4] for r in blocks], case.cu1)
    ratios["dit_vec"] = _ratio(vec, R.dit_vec(sd, c["t"], c["text_states_2"], c["guidance"], E), "dit_vec")
    vec = vec.float().cpu()
    for r in rec:
        name, x_in, x_out = r["name"], r["x_in"].float().cpu(), r["x_out"].float().cpu()
        kind = name.split(".")[0]
        if kind == "patch_embed":
            ratios[kind] = _ratio(x_out[:s_img], R.patch_embed(sd, c["x"], E)[0], name)
        elif kind == "token_refiner":
            if text_rows:
                ref = R.token_refiner(sd, "txt_in.", c["text_states"], c["t"], _refiner_mask(case, inp), heads, E, cfg.refiner_depth)
                ratios[kind] = _ratio(x_out[s_img:], ref[0], name)
        elif kind == "double_block":
            rio, rto = R.double_block(sd, name.replace("_block", "_blocks") + ".", x_in[None, :s_img], x_in[None, s_img:], vec, cu,
                                      cos, sin, heads, E)
            ratios[name + ".img"] = _ratio(x_out[:s_img], rio[0], name + ".img")
            if text_rows:
                ratios[name + ".txt"] = _ratio(x_out[s_img:], rto[0], name + ".txt")
        elif kind == "single_block":
            ref = R.single_block(sd, name.replace("_block", "_blocks") + ".", x_in[None], vec, case.s_txt, cu, cos, sin, heads, E)
            rows = slice(None) if text_rows else slice(0, s_img)
            ratios[name] = _ratio(x_out[rows], ref[0, rows], name)
        else:
            ref = R.unpatchify(R.final_layer(sd, x_in[None, :s_img], vec, E), t, hh // 2, w // 2, cfg.out_channels, cfg.patch_size)
            ratios[kind] = _ratio(out, ref, name)
    if not assert_ok:
        return ratios
    for k, v in ratios.items():
        h.note(k, v, case)
    if verbose:
        print(f"[dit wiring] {case.name}: error / tolerance per stage: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f"{case.name}: stages beyond rtol 2^-6 / atol 6e-2 (error / tolerance): {bad}"
    return ratios


def check_whole_output(h: Harness, model, case: Case, inp: dict, out: torch.Tensor, kind: Optional[str] = None) -> float:
    sd, prec = h.oracle_weights(model)
    err = range_error(out, oracle_forward(sd, config(kind or case.model_kind), case, inp, prec))
    h.note("whole output / 3e-2" + (" (fp8)" if (kind or "").startswith("fp8") else ""), err / RANGE_TOL, case)
    print(f"[dit wiring] {case.name}: whole output vs oracle {err:.3e} of range")
    assert err < RANGE_TOL, f"{case.name}: whole output {err:.3e} of range"
    return err


# ------------------------------------------------------------------------------------------------------------------ checks B
def padding_applies(case: Case) -> bool:
    """a prefix mask with at least one padding row that the refiner honours (use_attention_mask=False lets the refiner see them)"""
    return case.mask and case.use_attention_mask and case.n_valid < case.s_txt


def check_padding_content(h: Harness, model, case: Case, inp: dict, out: torch.Tensor, rec: list):
    """B1: other finite content (large values included) in text rows [n_valid, s_txt) leaves the image output and, after every
    stage, rows [0, cu1) of the residual stream bit-equal."""
    assert padding_applies(case)
    inp2 = clone_inputs(inp)
    pad = inp2["text_states"][0, case.n_valid:]
    junk = syn.hashed_uniform(tuple(pad.shape), "wiring.padding", 5) * 3.0
    junk.view(-1)[::7] *= 1000.0                       # |x| up to 3e3: a leak of any weight shows
    pad.copy_(junk.to(BF16))
    out2, rec2 = h.run_traced(model, inp2)
    for a, b in zip(rec, rec2):
        hi = case.s_img if a["name"] == "patch_embed" else case.cu1
        assert bits_equal(a["x_out"][:hi], b["x_out"][:hi]), f"{case.name}: padding text content changed rows [0, {hi}) after {a['name']}"
    assert bits_equal(out, out2), f"{case.name}: padding text content changed the image output"
    if case.n_valid > 0:
        # the other side: the last valid token is not padding
        inp3 = clone_inputs(inp)
        inp3["text_states"][0, case.n_valid - 1] = junk[0, :].to(BF16) * 1e-3
        assert not bits_equal(out, h.run(model, inp3)), f"{case.name}: the last valid text token does not reach the image output"


def check_rope_table_edge(h: Harness, model, case: Case, inp: dict, out: torch.Tensor):
    """B3: the tables as the first s_img rows of a buffer whose later rows are NaN: no NaN, bit-equal; row s_img - 1 is read."""
    assert case.rope
    inp2 = dict(inp)
    for k in ("freqs_cos", "freqs_sin"):
        buf = torch.full((case.s_img + 3, inp[k].shape[1]), float("nan"), dtype=inp[k].dtype, device=inp[k].device)
        buf[:case.s_img] = inp[k]
        inp2[k] = buf[:case.s_img]
    out2 = h.run(model, inp2)
    assert not bool(torch.isnan(out2).any()), f"{case.name}: a table row past s_img reached the output"
    assert bits_equal(out, out2), f"{case.name}: output differs with the tables inside a larger buffer"
    inp3 = dict(inp)
    for k, f in (("freqs_cos", 0.5), ("freqs_sin", -0.25)):
        inp3[k] = inp[k].clone()
        inp3[k][case.s_img - 1] = inp3[k][case.s_img - 1] * f + 0.3
    assert not bits_equal(out, h.run(model, inp3)), f"{case.name}: table row s_img - 1 is not read"


def check_repeat(h: Harness, model, case: Case, inp: dict, out: torch.Tensor):
    """B4"""
    assert bits_equal(out, h.run(model, inp)), f"{case.name}: a second call gives other bits"


SURFACE_VEC = 1.5       # half-width of the uniform `vec` of check_block_call_surfaces (test_block_call_surfaces_vs_oracle: 0.5)


def check_block_call_surfaces(h: Harness, model, case: Case, assert_ok: bool = True):
    """double_blocks[0].forward / single_blocks[0].forward on inputs made here.  B2, both sides of cu1: attention is a block's only
    path from a text row to the image rows, so stream row n_valid (the first padding row) must leave img_out and the valid text rows
    bit-equal and change the padding rows; row n_valid - 1 must change img_out.  Then A on the same calls (as
    test_block_call_surfaces_vs_oracle, at every case and with a wide vec); assert_ok=False returns those ratios unasserted."""
    cfg = config(case.model_kind)
    d, s_img, s_txt, nv = cfg.hidden_size, case.s_img, case.s_txt, (case.n_valid if case.mask else case.s_txt)
    S = s_img + s_txt
    dev = h.dev
    u = lambda shape, key, scale: (syn.hashed_uniform(shape, key, 7) * scale).to(BF16).to(dev)
    img, txt, vec = u((1, s_img, d), "wiring.img", 1.7), u((1, s_txt, d), "wiring.txt", 1.7), u((1, d), "wiring.vec", SURFACE_VEC)
    other = u((d,), "wiring.other", 1.7)
    cu = _cu(case)
    t, hh, w = case.thw
    freqs = None
    if case.rope:
        freqs = tuple(f.to(dev) for f in R.rope_tables([t, hh // 2, w // 2], cfg.rope_dim_list, 256.0))
    dbl, sgl = model.double_blocks[0], model.single_blocks[0]

    def double(txt_):
        with torch.no_grad():
            io, to = dbl(img, txt_, vec, cu, cu, S, S, freqs)
        return io[0].clone(), to[0].clone()

    def single(txt_):
        with torch.no_grad():
            return sgl(torch.cat([img, txt_], 1), vec, s_txt, cu, cu, S, S, freqs)[0].clone()

    def edited(row):
        e = txt.clone()
        e[0, row] = other
        return e

    io, to = double(txt)
    so = single(txt)
    if nv < s_txt:
        io2, to2 = double(edited(nv))
        assert bits_equal(io, io2), f"{case.name}: double block: the first padding row reaches img_out"
        assert bits_equal(to[:nv], to2[:nv]), f"{case.name}: double block: the first padding row reaches the valid text rows"
        assert not bits_equal(to[nv:], to2[nv:]), f"{case.name}: double block: the first padding row does not change the padding rows"
        so2 = single(edited(nv))
        assert bits_equal(so[:s_img + nv], so2[:s_img + nv]), f"{case.name}: single block: the first padding row reaches rows [0, cu1)"
        assert not bits_equal(so[s_img + nv:], so2[s_img + nv:]), f"{case.name}: single block: the first padding row changes nothing"
    if nv > 0:
        io2, _ = double(edited(nv - 1))
        assert not bits_equal(io, io2), f"{case.name}: double block: the last valid text row does not reach img_out"
        so2 = single(edited(nv - 1))
        assert not bits_equal(so[:s_img], so2[:s_img]), f"{case.name}: single block: the last valid text row does not reach the image rows"
    # A on these inputs: the modulation is SURFACE_VEC wide here, so a swapped chunk is far outside the tolerance
    sd, _ = h.oracle_weights(model)
    f = lambda t_: t_.float().cpu()
    ofreqs = (None, None) if freqs is None else tuple(f(t_) for t_ in freqs)
    rio, rto = R.double_block(sd, "double_blocks.0.", f(img), f(txt), f(vec), cu, *ofreqs, cfg.heads_num, E)
    rso = R.single_block(sd, "single_blocks.0.", torch.cat([f(img), f(txt)], 1), f(vec), s_txt, cu, *ofreqs, cfg.heads_num, E)
    ratios = {"surface.double.img": _ratio(io, rio[0], "double img_out"), "surface.double.txt": _ratio(to, rto[0], "double txt_out"),
              "surface.single": _ratio(so, rso[0], "single out")}
    if not assert_ok:
        return ratios
    for k, v in ratios.items():
        h.note(k, v, case)
    print(f"[dit wiring] {case.name}: block call surfaces, error / tolerance: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f"{case.name}: block call surfaces beyond rtol 2^-6 / atol 6e-2 (error / tolerance): {bad}"


def check_rekey(h: Harness, model, case_a: Case, case_b: Case, kind: Optional[str] = None):
    """B5: shapes A, B, A on one model (the workspace and the refiner buffers are re-keyed twice): the third output has the bits
    of the first."""
    inp_a, inp_b = h.inputs(case_a, kind), h.inputs(case_b, kind)
    first = h.run(model, inp_a)
    ws_a = model._ws
    h.run(model, inp_b)
    assert model._ws is not ws_a and model._ws.key[:2] == (case_b.s_img, case_b.s_txt)
    assert bits_equal(first, h.run(model, inp_a)), f"A = {case_a.name}, B = {case_b.name}: A after B differs from A"
    assert model._ws.key[:2] == (case_a.s_img, case_a.s_txt)


def check_cache(h: Harness, kind: str = "tiny"):
    """B6: the SAME text_states / text_mask objects across calls, edited in place, then a new mask object; after every step the
    output has the bits of a freshly built model on cloned inputs."""
    case = Case((3, 6, 10), 32, 11)
    model = h.model(kind, fresh=True)
    inp = h.inputs(case)

    def same_as_fresh(step):
        got = h.run(model, inp)
        want = h.run(h.model(kind, fresh=True), clone_inputs(inp))
        assert bits_equal(got, want), f"refiner cache / valid-count cache: stale output after: {step}"
        return got

    base = same_as_fresh("first call")
    same_as_fresh("second call, nothing changed")
    inp["text_states"][0, 3] = inp["text_states"][0, 3] * -0.5 + 0.25
    edited = same_as_fresh("in-place edit of valid text token 3")
    assert not bits_equal(base, edited)
    inp["text_mask"][0, 5:11] = 0
    short = same_as_fresh("in-place edit of the mask, n_valid 11 -> 5")
    assert not bits_equal(edited, short)
    inp["text_mask"][0, 5:11] = 1
    assert bits_equal(edited, same_as_fresh("in-place edit of the mask, n_valid 5 -> 11"))
    mask7 = torch.zeros_like(inp["text_mask"])
    mask7[0, :7] = 1
    inp["text_mask"] = mask7
    assert not bits_equal(edited, same_as_fresh("a new mask object with n_valid 7"))


def check_batch(h: Harness, kind: str = "tiny"):
    """B7: B = 2 at latent (3, 6, 10), n_valid (1, 31) per row or one shared [1, L] mask, t and guidance with 1 or 2 elements:
    every row has the bits of its single-sample run."""
    model = h.model(kind)
    rows = [h.inputs(Case((3, 6, 10), 32, nv), seed=s) for s, nv in ((0, 1), (1, 31))]
    cat = lambda k: torch.cat([r[k] for r in rows], 0)
    t2, g2 = torch.tensor([997.093, 412.5], device=h.dev), torch.tensor([6016.0, 1000.0], device=h.dev)
    shared = torch.zeros_like(rows[0]["text_mask"])
    shared[0, :11] = 1
    for n_t, n_g, per_row in ((1, 1, True), (2, 2, True), (2, 1, False), (1, 2, False)):
        batch = dict(rows[0], x=cat("x"), text_states=cat("text_states"), text_states_2=cat("text_states_2"),
                     text_mask=cat("text_mask") if per_row else shared.clone(), t=t2[:n_t].clone(), guidance=g2[:n_g].clone())
        out = h.run(model, batch)
        assert out.shape[0] == 2
        for b in range(2):
            one = dict(clone_inputs(rows[b]), t=t2[b if n_t == 2 else 0].reshape(1).clone(), guidance=g2[b if n_g == 2 else 0].reshape(1).clone())
            if not per_row:
                one["text_mask"] = shared.clone()
            assert bits_equal(out[b:b + 1], h.run(model, one)), \
                f"batch row {b} (t x{n_t}, guidance x{n_g}, {'per-row' if per_row else 'shared'} mask) differs from its single-sample run"


def check_mask_none_equals_ones(h: Harness):
    """text_mask=None is an all-ones mask, bit for bit"""
    none, ones = Case((3, 6, 10), 32, 32, mask=False), Case((3, 6, 10), 32, 32)
    model = h.model("tiny")
    assert bits_equal(h.run(model, h.inputs(none)), h.run(model, h.inputs(ones)))


def check_case(h: Harness, case: Case):
    """A and the per-case exact checks (B1, B3, B4) that apply to the case"""
    model = h.model(case.model_kind)
    inp = h.inputs(case)
    out, rec = h.run_traced(model, inp)
    check_stages(h, model, case, inp, out, rec)
    check_whole_output(h, model, case, inp, out)
    check_repeat(h, model, case, inp, out)
    if padding_applies(case):
        check_padding_content(h, model, case, inp, out, rec)
    if case.rope:
        check_rope_table_edge(h, model, case, inp, out)


def check_fp8_case(h: Harness, case: Case, other: Case):
    """the FP8-MFMA configuration: whole output against the quantisation-aware oracle, B1 and B5"""
    model = h.model("fp8")
    inp = h.inputs(case, "fp8")
    out, rec = h.run_traced(model, inp)
    assert model._ws.xq is not None, "the FP8-MFMA path did not run"
    check_whole_output(h, model, case, inp, out, "fp8")
    if padding_applies(case):
        check_padding_content(h, model, case, inp, out, rec)
    check_rekey(h, model, case, other, "fp8")
    assert model._ws.xq is not None


# ------------------------------------------------------------------------------------------------------------------ mutants
# Each is a context manager that mis-wires the host code (or the double it calls) the way a slip of the pen would; `check` names the
# check that must reject it and `case` where.  "A" = check_stages, "A block call surfaces" = the tolerance part of
# check_block_call_surfaces (a tolerance: the mutant must exceed it at least 2x on the CPU, in the stage named last).
def _patch_attr(obj, name, value):
    @contextlib.contextmanager
    def cm():
        old = getattr(obj, name)
        setattr(obj, name, value)
        try:
            yield
        finally:
            setattr(obj, name, old)
    return cm()


def _mutant_cu1(delta):
    from hunyuanvideo_efficiency_amd.modules import models
    inner = models.segment_attention_
    return _patch_attr(models, "segment_attention_", lambda sp, qkv, cat, s_img, cu1, heads, d: inner(sp, qkv, cat, s_img, cu1 + delta, heads, d))


def _mutant_refiner_n_valid(delta):
    """token_refiner.run looks n_valid_text up in attenion at call time; models.py holds its own name for cu1 (unchanged)"""
    from hunyuanvideo_efficiency_amd.modules import attenion
    inner = attenion.n_valid_text
    return _patch_attr(attenion, "n_valid_text", lambda mask: max(0, min(mask.shape[1], inner(mask) + delta)))


def _mutant_n_rope(delta):
    from hunyuanvideo_efficiency_amd import ops
    inner = ops.qknorm_rope_

    def qknorm_rope_(qkv, qw, kw, cos, sin, n_rope, *a, **k):
        if n_rope > 0:
            n_rope = min(n_rope + delta, qkv.shape[0])          # the kernel rotates row r where r < n_rows and r < n_rope
            if n_rope > cos.shape[0]:                           # ... and reads the memory behind a table that is too short
                room = (cos.untyped_storage().nbytes() // cos.element_size() - cos.storage_offset()) // cos.stride(0)
                n_rope = min(n_rope, room)                      # (where the allocation ends with the table, nothing to emulate)
                cos, sin = (torch.as_strided(t, (n_rope, t.shape[1]), t.stride(), t.storage_offset()) for t in (cos, sin))
        return inner(qkv, qw, kw, cos, sin, n_rope, *a, **k)
    return _patch_attr(ops, "qknorm_rope_", qknorm_rope_)


def _mutant_mod_chunks(swaps):
    """the 6 chunks (shift1, scale1, gate1, shift2, scale2, gate2) of a double block's modulation read from swapped slots"""
    from hunyuanvideo_efficiency_amd import ops
    inner = ops.linear_smallm

    def linear_smallm(x, w, bias=None, silu_in=False, **k):
        y = inner(x, w, bias, silu_in=silu_in, **k)
        d = x.shape[-1]
        if silu_in and w.shape[0] == 6 * d:
            c = list(y.reshape(6, d).unbind(0))
            for i, j in swaps:
                c[i], c[j] = c[j], c[i]
            y = torch.stack(c, 0).reshape(1, 6 * d)
        return y
    return _patch_attr(ops, "linear_smallm", linear_smallm)


@contextlib.contextmanager
def _mutant_img_txt_mod(model):
    blk = model.double_blocks[0]
    blk.img_mod, blk.txt_mod = blk.txt_mod, blk.img_mod
    try:
        yield
    finally:
        blk.img_mod, blk.txt_mod = blk.txt_mod, blk.img_mod


def _mutant_cache_ignores_version():
    """the refiner cache key without the _version of text_states and of the mask: the stored key is made current before every call"""
    from hunyuanvideo_efficiency_amd.modules.models import HYVideoDiffusionTransformer as M
    inner = M._forward_one

    def _forward_one(self, x, t, text_states, text_mask, *a):
        tc = getattr(text_states, "_hv_txt_cache", None)
        mask_all = text_mask if self.use_attention_mask else None
        if tc is not None and tc.get("mask") is mask_all:
            tc["key"] = (text_states._version, None if mask_all is None else mask_all._version, id(self.txt_in),
                         tuple(p._version for p in self.txt_in.parameters()))
        return inner(self, x, t, text_states, text_mask, *a)
    return _patch_attr(M, "_forward_one", _forward_one)


def _mutant_batch_row0_mask():
    from hunyuanvideo_efficiency_amd.modules.models import HYVideoDiffusionTransformer as M
    inner = M._forward_one

    def _forward_one(self, x, t, text_states, text_mask, *a):
        if text_mask is not None and text_mask.shape[0] > 1:
            text_mask = text_mask[0:1]
        return inner(self, x, t, text_states, text_mask, *a)
    return _patch_attr(M, "_forward_one", _forward_one)


_MID = Case((3, 6, 10), 32, 11)
_ONE_TILE = Case((1, 16, 16), 32, 1)
# name -> (context manager factory taking the model, the check that rejects it, the case, for "A": the stage)
MUTANTS = {
    "cu1+1": (lambda m: _mutant_cu1(+1), "B2 block call surfaces", _ONE_TILE, None),
    "cu1-1": (lambda m: _mutant_cu1(-1), "B2 block call surfaces", _ONE_TILE, None),
    "cu1+1 (forward)": (lambda m: _mutant_cu1(+1), "B1 padding content", _MID, None),
    "refiner n_valid+1": (lambda m: _mutant_refiner_n_valid(+1), "B1 padding content", _MID, None),
    "refiner n_valid-1": (lambda m: _mutant_refiner_n_valid(-1), "A", Case((3, 6, 10), 9, 4), "token_refiner"),
    "n_rope+1": (lambda m: _mutant_n_rope(+1), "B3 rope table edge", _MID, None),
    "n_rope-1": (lambda m: _mutant_n_rope(-1), "B3 rope table edge", _MID, None),
    "gate1<->gate2": (lambda m: _mutant_mod_chunks([(2, 5)]), "A block call surfaces", _MID, "surface.double.img"),
    "img_mod<->txt_mod": (_mutant_img_txt_mod, "A block call surfaces", _MID, "surface.double.img"),
    "shift<->scale": (lambda m: _mutant_mod_chunks([(0, 1), (3, 4)]), "A block call surfaces", _MID, "surface.double.img"),
    "refiner cache ignores _version": (lambda m: _mutant_cache_ignores_version(), "B6 cache", None, None),
    "batch row b reads row 0's mask": (lambda m: _mutant_batch_row0_mask(), "B7 batch", None, None),
}


def run_named_check(h: Harness, check: str, case: Optional[Case]):
    """the one check a mutant is assigned to, as check_case / the scenario tests run it"""
    if check == "B6 cache":
        return check_cache(h)
    if check == "B7 batch":
        return check_batch(h)
    model = h.model(case.model_kind)
    if check == "B2 block call surfaces":
        return check_block_call_surfaces(h, model, case)
    if check == "A block call surfaces":
        return check_block_call_surfaces(h, model, case, assert_ok=False)
    inp = h.inputs(case)
    out, rec = h.run_traced(model, inp)
    if check == "A":
        return check_stages(h, model, case, inp, out, rec, verbose=False, assert_ok=False)
    if check == "B1 padding content":
        return check_padding_content(h, model, case, inp, out, rec)
    if check == "B3 rope table edge":
        return check_rope_table_edge(h, model, case, inp, out)
    raise KeyError(check)


def report(h: Harness) -> str:
    lines = ["[dit wiring] largest error / tolerance per stage (rtol 2^-6, atol 6e-2; whole output: of 3e-2 of range):"]
    for k in sorted(h.ratios):
        v, where = h.ratios[k]
        lines.append(f"[dit wiring]   {k:<28s} {v:.3f}  at {where}")
    return "\n".join(lines)
