"""TEST INFRASTRUCTURE: CPU stand-ins for the C-ABI kernels (hunyuanvideo_efficiency_amd.ops.*), built on the oracle's
arithmetic, so that the HOST logic of the product (module wiring, workspaces, strided views, sequence-parallel sharding)
can run under gloo on CPU with world_size > 1.  Never imported by the product; installed by tests via `install()`.

Each double has the signature, the return value, the written cells, the rounding points and the refusals of the wrapper it replaces:
tests/test_kernel_doubles_cpu.py and tests/test_gpu_kernel_doubles.py make the same call on both (tests/double_parity.py) and compare."""
import math

import torch
import torch.nn.functional as F

from oracle import dit_ref as R

E = R.Prec(True)
BF16 = torch.bfloat16
F16 = torch.float16


def _bf(x):
    return x.to(BF16)


# ---- the refusals of the wrappers and of the C ABI behind them, restated (not imported): a host bug that hands a kernel an illegal view
# must fail on the CPU tier as it would on the GPU.  _chk / _rows are what ops._chk / ops._rows refuse (minus "not a GPU tensor"); a rule
# the C ABI checks (HV_ERR_ARG: row strides in multiples of 8 elements = 16 bytes, the output pitch, the K / N granularity of a main
# loop) raises HVKernelError as the product does.  tests/double_parity.REFUSALS asserts each of them on both sides.
from hunyuanvideo_efficiency_amd._abi import HVKernelError  # noqa: E402


def _chk(t, dtype, name, last_contig=True):
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if last_contig and t.dim() > 0 and t.stride(-1) != 1:
        raise ValueError(f"{name}: innermost dimension must be contiguous")


def _rows(t, name):
    """(n_rows, D, row_stride) of a [.., D] tensor whose leading dimensions collapse to uniformly strided rows"""
    if t.dim() == 1:
        return 1, t.shape[0], t.shape[0]
    d = t.shape[-1]
    ld = exp = t.stride(-2)
    for i in range(t.dim() - 2, -1, -1):
        if t.shape[i] != 1 and t.stride(i) != exp:
            raise ValueError(f"{name}: rows are not uniformly strided {tuple(t.shape)} {t.stride()}")
        exp *= t.shape[i]
    return t.numel() // d, d, ld


def _abi(ok, what):
    """a condition the C ABI answers with HV_ERR_ARG"""
    if not ok:
        raise HVKernelError(f"{what}: bad argument")


def _pitch_ok(rows, pitch, width):
    return rows <= 1 or pitch >= width


def _rows_of(t, m, width):
    """the [m, width] row view of a [.., >= width] tensor with uniformly strided rows (what a kernel addresses through ld)"""
    _, _, ld = _rows(t, "rows")
    return torch.as_strided(t, (m, width), (ld, 1), t.storage_offset())


def _chk_mod_vectors(shift, scale, d):
    for t, n in ((shift, "shift"), (scale, "scale")):
        if t is not None:
            _chk(t, BF16, n)
            assert t.numel() == d and t.is_contiguous(), f"{n} must be a contiguous [{d}] vector (batch 1)"


def ln_modulate(x, shift=None, scale=None, out=None, eps=1e-6, affine=False):
    _chk(x, BF16, "x")
    m, d, ldx = _rows(x, "x")
    if out is not None:
        _chk(out, BF16, "out")
        mo, do, ldo = _rows(out, "out")
        assert (mo, do) == (m, d)
        _abi(ldo % 8 == 0 and _pitch_ok(m, ldo, d), "ln_modulate out")
    _chk_mod_vectors(shift, scale, d)
    _abi(d % 8 == 0 and d <= 4096 and ldx % 8 == 0, "ln_modulate")
    xf = x.float()
    y = F.layer_norm(xf, (x.shape[-1],), None, None, eps)
    if affine:
        y = y * scale.float() + shift.float()
    else:
        if scale is not None:
            y = y * E.r(1.0 + scale.float())
        if shift is not None:
            y = y + shift.float()
    r = _bf(y)
    if out is None:
        return r
    out.copy_(r)
    return out


def qknorm_rope_(qkv, q_weight, k_weight, cos, sin, n_rope, n_heads, k_offset, eps=1e-6, out=None):
    _chk(qkv, BF16, "qkv")
    n, _, ld = _rows(qkv, "qkv")
    _chk(q_weight, BF16, "q_weight"), _chk(k_weight, BF16, "k_weight")
    if n_rope > 0:
        _chk(cos, torch.float32, "cos"), _chk(sin, torch.float32, "sin")
        assert cos.is_contiguous() and sin.is_contiguous() and cos.shape[-1] == 128 and cos.shape[0] >= n_rope
    d = n_heads * 128
    _abi(n_heads > 0 and 0 <= n_rope <= n and ld % 8 == 0 and k_offset % 8 == 0, "qknorm_rope")
    if out is not None:
        _chk(out, BF16, "out", False)
        assert out.dim() == 3 and out.shape[0] == n and out.stride(2) == 1 and out.shape[2] % 128 == 0
        assert out.shape[1] * out.shape[2] == 2 * n_heads * 128, (out.shape, n_heads)
        _abi(out.stride(0) % 8 == 0 and out.stride(1) % 8 == 0 and _pitch_ok(n, out.stride(0), out.shape[2]), "qknorm_rope out")
    else:
        _abi(k_offset >= d and _pitch_ok(n, ld, k_offset + d), "qknorm_rope k_offset")
    res = []
    for off, w in ((0, q_weight), (k_offset, k_weight)):
        x = qkv[:, off:off + d].float().reshape(1, n, n_heads, 128)
        y = R.rms_norm(x, w.float(), E, eps)
        if n_rope:
            y = torch.cat([R.apply_rope(y[:, :n_rope], cos[:n_rope].float(), sin[:n_rope].float(), E), y[:, n_rope:]], 1)
        if out is None:
            qkv[:, off:off + d] = _bf(y.reshape(n, d))
        res.append(_bf(y.reshape(n, d)))
    if out is not None:      # out of place, scattered by head block: out [n, blocks, heads_per_block*128] (source untouched)
        out.copy_(torch.cat(res, 1).reshape(n, out.shape[1], out.shape[2]))
        return out
    return qkv


def _act(y, act):
    if act == 1:
        return R.gelu_tanh(y, E)
    if act == 2:
        return E.r(F.silu(y))
    return y


def _gemm_epilogue(out_shape, m, n, n_split, out, out1, bias, gate, res, act, act1):
    """what ops._gemm_epilogue and fill_common (csrc/hv_gemm.hip) refuse; allocates a missing out as out_shape + (n0,)"""
    n0 = n_split if 0 < n_split < n else n
    if out is None:
        out = torch.empty(*out_shape, n0, dtype=BF16)
    _chk(out, BF16, "out")
    mo, no, ld0 = _rows(out, "out")
    assert mo == m and no >= n0
    _abi(n % 8 == 0 and ld0 % 8 == 0 and _pitch_ok(m, ld0, n0), "gemm out")
    if n0 < n:
        _abi(out1 is not None, "gemm out1")
        _chk(out1, BF16, "out1")
        m1, n1, ld1 = _rows(out1, "out1")
        assert m1 == m and n1 >= n - n0
        _abi(n0 % 8 == 0 and ld1 % 8 == 0 and _pitch_ok(m, ld1, n - n0), "gemm n_split / out1")
    for t, nm in ((bias, "bias"), (gate, "gate")):
        if t is not None:
            _chk(t, BF16, nm)
            assert t.numel() == n and t.is_contiguous()
    if res is not None:
        _chk(res, BF16, "res")
        mr, nr, ld_res = _rows(res, "res")
        assert mr == m and nr == n
        _abi(ld_res % 8 == 0, "gemm res")
    _abi(not (gate is not None and res is None) and act in (0, 1, 2) and act1 in (0, 1, 2), "gemm epilogue")
    return out, n0


def _gemm_store(y, out, n0, act, out1, act1, gate, res):
    """the epilogues shared by gemm and gemm_fp8, on the rounded product y [M, N]: out[:, :n0] (columns behind n0 keep their bits),
    out1[:, :N - n0]; with a gate bf16(res + bf16(act(y) * gate)), two roundings; with res alone bf16(res + act(y))"""
    m, n = y.shape
    z = torch.cat([_act(y[:, :n0], act), _act(y[:, n0:], act1)], 1)
    if res is not None:          # res and gate span all N columns: the columns of out1 take them too (csrc/hv_gemm.hip, epilogue)
        z = _rows_of(res, m, n).float() + (E.r(z * gate.float()) if gate is not None else z)
    z = _bf(z)
    _rows_of(out, m, n0).copy_(z[:, :n0])
    if n0 < n:
        _rows_of(out1, m, n - n0).copy_(z[:, n0:])
    return out


def gemm(a, w, bias=None, out=None, act=0, n_split=0, out1=None, act1=0, gate=None, res=None):
    _chk(a, BF16, "a"), _chk(w, BF16, "w")
    m, k, lda = _rows(a, "a")
    n, kw, ldw = _rows(w, "w")
    assert k == kw, (a.shape, w.shape)
    out, n0 = _gemm_epilogue(a.shape[:-1], m, n, n_split, out, out1, bias, gate, res, act, act1)
    _abi(k >= 64 and k % 64 == 0 and lda % 8 == 0 and ldw % 8 == 0, "gemm K / lda / ldw")
    y = E.r(_rows_of(a, m, k).float() @ _rows_of(w, n, k).float().T + (0 if bias is None else bias.float()))
    return _gemm_store(y, out, n0, act, out1, act1, gate, res)


# ---- the opt-in FP8-MFMA path (ops.fp8_dequant, quant_rows_fp8, ln_modulate_fp8, gemm_fp8): the contract of oracle/dit_ref.py
# (fp8_quant_rows, Fp8MfmaPrec) on CPU float8_e4m3fn tensors
FP8 = torch.float8_e4m3fn


def fp8_dequant(w8, scale_bf16, out_bf16):
    if w8.dtype != FP8:
        raise HVKernelError("fp8_dequant: expected a float8_e4m3fn tensor")
    _chk(scale_bf16, BF16, "scale"), _chk(out_bf16, BF16, "out")
    assert w8.is_contiguous() and out_bf16.is_contiguous() and out_bf16.numel() == w8.numel()
    _abi(w8.numel() > 0 and w8.numel() % 8 == 0, "fp8_dequant n")
    out_bf16.copy_(_bf(w8.to(BF16).float() * scale_bf16.float()).reshape(out_bf16.shape))
    return out_bf16


def _quant_outputs(x, out_q, out_scale, what):
    _chk(x, BF16, "x")
    m, k, ldx = _rows(x, "x")
    if out_q is None:
        out_q = torch.empty(m, k, dtype=FP8)
    if out_scale is None:
        out_scale = torch.empty(m, dtype=torch.float32)
    assert out_q.dtype == FP8 and out_q.shape[-1] == k and out_q.stride(-1) == 1 and out_scale.numel() >= m
    ldq = out_q.stride(-2) if out_q.dim() > 1 else k
    _abi(k % 8 == 0 and ldx % 8 == 0 and ldq % 16 == 0 and _pitch_ok(m, ldq, k), what)
    return m, k, out_q, out_scale


def _quant_store(y, m, k, out_q, out_scale):
    q, s = R.fp8_quant_rows(y.reshape(m, k).float())
    torch.as_strided(out_q, (m, k), (out_q.stride(-2) if out_q.dim() > 1 else k, 1), out_q.storage_offset()).copy_(q.to(FP8))
    out_scale.reshape(-1)[:m] = s[:, 0]
    return out_q, out_scale


def quant_rows_fp8(x, out_q=None, out_scale=None):
    m, k, out_q, out_scale = _quant_outputs(x, out_q, out_scale, "quant_rows_fp8")
    return _quant_store(x, m, k, out_q, out_scale)


def ln_modulate_fp8(x, shift=None, scale=None, out_q=None, out_scale=None, eps=1e-6):
    m, d, out_q, out_scale = _quant_outputs(x, out_q, out_scale, "ln_modulate_fp8")
    _chk_mod_vectors(shift, scale, d)
    _abi(d <= 4096, "ln_modulate_fp8 D")
    return _quant_store(ln_modulate(x, shift, scale, eps=eps), m, d, out_q, out_scale)


def gemm_fp8(a_q, a_scale, w_q, w_scale, bias=None, out=None, act=0, n_split=0, out1=None, act1=0, gate=None, res=None):
    for t, nm in ((a_q, "a_q"), (w_q, "w_q")):
        if t.dtype != FP8:
            raise HVKernelError(f"gemm_fp8: {nm} must be a float8_e4m3fn tensor")
    _chk(a_scale, torch.float32, "a_scale"), _chk(w_scale, BF16, "w_scale")
    m, k, lda = _rows(a_q, "a_q")
    n, kw, ldw = _rows(w_q, "w_q")
    assert k == kw and a_scale.numel() >= m and w_scale.numel() == 1
    out, n0 = _gemm_epilogue((m,), m, n, n_split, out, out1, bias, gate, res, act, act1)
    _abi(k >= 384 and k % 128 == 0 and lda % 16 == 0 and ldw % 16 == 0, "gemm_fp8 K / lda / ldw")
    y = (_rows_of(a_q, m, k).float() @ (_rows_of(w_q, n, k).float() * w_scale.float()).T) * a_scale.reshape(-1)[:m, None]
    y = E.r(y + (0 if bias is None else bias.float()))
    return _gemm_store(y, out, n0, act, out1, act1, gate, res)


def linear_smallm(x, w, bias=None, silu_in=False, silu_out=False, out=None, addend=None):
    _chk(x, BF16, "x"), _chk(w, BF16, "w")
    m, k, ldx = _rows(x, "x")
    n, kw, ldw = _rows(w, "w")
    assert k == kw and ldw == k and m <= 4
    if bias is not None:
        _chk(bias, BF16, "bias")
    if out is not None:
        _abi(_pitch_ok(m, _rows(out, "out")[2], n), "linear_smallm out")
    if addend is not None:
        _chk(addend, BF16, "addend")
        assert out is None or (addend.shape == out.shape and addend.stride() == out.stride())
        assert out is not None or (tuple(addend.shape) == (*x.shape[:-1], n) and addend.is_contiguous())
    _abi(m >= 1 and k >= 8 and k % 8 == 0 and ldx % 8 == 0, "linear_smallm")
    xf = x.float()
    if silu_in:
        xf = E.r(F.silu(xf))
    y = E.r(xf @ w.float().T + (0 if bias is None else bias.float()))
    if silu_out:
        y = E.r(F.silu(y))
    if addend is not None:
        y = E.r(y + addend.float())
    r = _bf(y)
    if out is None:
        return r
    out.copy_(r)
    return out


def _attn_views(q, k, v, out, n_heads, what):
    """the refusals shared by attn_fwd and attn_partial; returns the [n, H, 128] head views of q, k, v (columns behind H * 128 unread)"""
    for t, nm in ((q, "q"), (k, "k"), (v, "v")) + (() if out is None else ((out, "out"),)):
        _chk(t, BF16, nm)
        assert t.dim() == 2
    n_q, n_kv, d = q.shape[0], k.shape[0], n_heads * 128
    assert v.shape[0] == n_kv and (out is None or out.shape[0] == n_q)
    _abi(n_heads > 0 and n_kv > 0 and all(t.stride(0) % 8 == 0 for t in (q, k, v)), what + " strides")
    assert all(t.shape[1] >= d for t in (q, k, v)), f"{what}: a view narrower than n_heads * 128 columns"
    return tuple(t[:, :d].float().reshape(t.shape[0], n_heads, 128) for t in (q, k, v))


def attn_fwd(q, k, v, out, n_heads, scale=None, kv_split_workspace=True):
    """the oracle's attention (oracle.dit_ref.sdpa: fp32 scores, p rounded to bf16 for P.V, the unrounded row sum) of the first
    n_heads * 128 columns of each view, with the softmax scale the caller gives; kv_split_workspace only chooses between two kernels
    that compute the same function.  q is NOT rounded after the scale (DELIBERATE_DEVIATIONS in tests/double_parity.py)."""
    qh, kh, vh = _attn_views(q, k, v, out, n_heads, "attn_fwd")
    n_q, d = q.shape[0], n_heads * 128
    _abi(out.stride(0) % 4 == 0 and _pitch_ok(n_q, out.stride(0), d), "attn_fwd out")
    assert out.shape[1] >= d
    if n_q == 0:
        return out
    s = torch.matmul(qh.permute(1, 0, 2), kh.permute(1, 2, 0)) * (1.0 / math.sqrt(128) if scale is None else float(scale))
    e = torch.exp(s - s.amax(dim=-1, keepdim=True))
    o = torch.matmul(e.to(BF16).float(), vh.permute(1, 0, 2)) / e.sum(dim=-1, keepdim=True)
    out[:, :d] = _bf(o.permute(1, 0, 2).reshape(n_q, d))
    return out


# ---- ring attention: the partial format of hv_attn_partial_bf16 / hv_attn_merge_bf16 (log2-domain max m, unnormalised fp32 o and row sum l)
class AttnPartials:
    """ops.AttnPartials on the CPU: the same attributes, shapes and dtypes"""

    def __init__(self, n_slots, n_q, n_heads, device):
        self.n_slots, self.n_q, self.n_heads = n_slots, n_q, n_heads
        self.o = torch.zeros(n_slots, n_q, n_heads, 128, dtype=torch.float32)
        self.ml = torch.zeros(n_slots, n_q, n_heads, 2, dtype=torch.float32)
        self.used = 0


def split_cut(n_kv):
    """the first key of the second half of a 2-way KV split: half the 64-key tiles, rounded up (include/hv_kernels.h)"""
    return ((n_kv + 63) // 64 + 1) // 2 * 64


def attn_partial(q, k, v, parts, n_heads, splits=1, scale=None):
    qh, kh, vh = _attn_views(q, k, v, None, n_heads, "attn_partial")
    n_q, n_kv = q.shape[0], k.shape[0]
    assert n_q == parts.n_q and n_heads == parts.n_heads and parts.used + splits <= parts.n_slots
    _abi(splits in (1, 2) and not (splits == 2 and (n_kv + 63) // 64 < 2), "attn_partial splits")
    sc = torch.tensor(128 ** -0.5 if scale is None else scale, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    qh = qh.transpose(0, 1)
    bounds = [0, n_kv] if splits == 1 else [0, split_cut(n_kv), n_kv]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        s = qh @ kh[lo:hi].transpose(0, 1).transpose(1, 2) * sc
        m = s.max(-1, keepdim=True).values
        pr = torch.exp2(s - m)
        parts.o[parts.used] = (pr.to(BF16).float() @ vh[lo:hi].transpose(0, 1)).transpose(0, 1)
        parts.ml[parts.used, :, :, 0] = m[..., 0].transpose(0, 1)
        parts.ml[parts.used, :, :, 1] = pr.sum(-1).transpose(0, 1)
        parts.used += 1


def attn_merge(parts, out):
    _chk(out, BF16, "out")
    assert out.dim() == 2 and out.shape[0] == parts.n_q and parts.used >= 1
    d = parts.n_heads * 128
    _abi(out.stride(0) % 4 == 0 and _pitch_ok(parts.n_q, out.stride(0), d), "attn_merge out")
    o, ml = parts.o[:parts.used], parts.ml[:parts.used]
    m = ml[..., 0].max(0).values
    wgt = torch.exp2(ml[..., 0] - m)
    acc = (o * wgt[..., None]).sum(0) / (ml[..., 1] * wgt).sum(0)[..., None]
    out[:, :d] = acc.reshape(parts.n_q, -1).to(BF16)
    return out


def patchify(x_f32, out=None):
    _chk(x_f32, torch.float32, "x")
    assert x_f32.is_contiguous() and x_f32.dim() == 4
    c, t, h, w = x_f32.shape
    _abi(h % 2 == 0 and w % 2 == 0, "patchify H / W")
    r = _bf(x_f32.reshape(c, t, h // 2, 2, w // 2, 2).permute(1, 2, 4, 0, 3, 5).reshape(t * (h // 2) * (w // 2), c * 4))
    if out is None:
        return r
    out.copy_(r)
    return out


def unpatchify(y, c, t, h, w, out=None):
    _chk(y, BF16, "y")
    assert y.dim() == 2
    _abi(h % 2 == 0 and w % 2 == 0 and y.stride(0) % 4 == 0, "unpatchify H / W / ldy")
    n = t * (h // 2) * (w // 2)
    r = R.unpatchify(y[:n, :c * 4][None], t, h // 2, w // 2, c, [1, 2, 2])[0]        # a bit copy: no arithmetic
    if out is None:
        return r.contiguous()
    torch.as_strided(out, (r.numel(),), (1,), out.storage_offset()).copy_(r.reshape(-1))      # the c t h w elements behind out's first
    return out


def euler_step_(sample_f32, model_out_bf16, dt):
    _chk(sample_f32, torch.float32, "sample"), _chk(model_out_bf16, BF16, "model_out")
    assert sample_f32.is_contiguous() and model_out_bf16.is_contiguous() and sample_f32.numel() == model_out_bf16.numel()
    sample_f32.add_(model_out_bf16.float() * dt)
    return sample_f32


def masked_mean(x, mask_i32=None):
    _chk(x, BF16, "x")
    assert x.dim() == 2 and x.is_contiguous()
    if mask_i32 is not None:
        _chk(mask_i32, torch.int32, "mask")
    if mask_i32 is None:
        return _bf(x.float().mean(0))
    m = mask_i32.float()[:, None]
    return _bf((x.float() * m).sum(0) / m.sum())


def broadcast_row_(src, dst):
    _chk(src, BF16, "src"), _chk(dst, BF16, "dst")
    assert dst.dim() == 2 and src.numel() == dst.shape[1]
    _abi(_pitch_ok(dst.shape[0], dst.stride(0), dst.shape[1]), "broadcast_row dst")
    dst.copy_(src.reshape(1, -1).expand_as(dst))
    return dst


def timestep_embedding(t_f32, dim=256, max_period=10000.0):
    if t_f32.dtype != torch.float32 or (t_f32.dim() > 0 and t_f32.stride(-1) != 1):     # what ops._chk refuses
        raise ValueError("t: expected fp32 with a contiguous innermost dimension")
    return _bf(R.timestep_embedding(t_f32.reshape(-1), dim, max_period))


def copy3d(src, dst, n_batch, rows, cols, src_bs, src_ld, dst_bs, dst_ld):
    _chk(src, BF16, "src", False), _chk(dst, BF16, "dst", False)
    _abi(n_batch >= 0 and rows >= 0 and cols > 0 and cols % 8 == 0 and src_ld % 8 == 0 and dst_ld % 8 == 0 and src_bs % 8 == 0
         and dst_bs % 8 == 0 and n_batch <= 65535 and _pitch_ok(rows, dst_ld, cols), "copy3d")
    if n_batch == 0 or rows == 0:
        return dst
    s = torch.as_strided(src, (n_batch, rows, cols), (src_bs, src_ld, 1), src.storage_offset())
    d = torch.as_strided(dst, (n_batch, rows, cols), (dst_bs, dst_ld, 1), dst.storage_offset())
    d.copy_(s)
    return dst


# ---- VAE conv entry points (hunyuanvideo_efficiency_amd.vae_ops.*): fp32 emulations in the kernels' own operation order, so that the
# reference-and-bound logic of the GPU edge tests (tests/conv_bounds.py) runs against them on the CPU (tests/test_conv_bounds_cpu.py)
def _gather_rows(m, tap, oH, oW, src, stride):
    _, sH, sW = src
    t, h, w = m // (oH * oW), (m // oW) % oH, m % oW
    ti = (t * stride[0] + tap // 9 - 2).clamp(min=0)
    hi = (h * stride[1] + (tap // 3) % 3 - 1).clamp(0, sH - 1)
    wi = (w * stride[2] + tap % 3 - 1).clamp(0, sW - 1)
    return (ti * sH + hi) * sW + wi


def conv3d_causal_strided(x, w_taps, bias, sT, sH, sW, cin, cout, stride=(1, 1, 1), out=None):
    """K-tile by K-tile (64 channels of one tap) into one fp32 accumulator, bias added last, one rounding to fp16"""
    _chk(x, F16, "x"), _chk(w_taps, F16, "w_taps")
    assert w_taps.is_contiguous() and w_taps.numel() == cout * 27 * cin, (w_taps.shape, cout, cin)
    T, H, W = ((s - 1) // m + 1 for s, m in zip((sT, sH, sW), stride))
    if out is not None:
        _chk(out, F16, "out")
        assert tuple(out.shape) == (T * H * W, cout), (tuple(out.shape), T, H, W, cout)
        _abi(out.stride(0) % 8 == 0 and _pitch_ok(T * H * W, out.stride(0), cout), "conv3d_causal_strided out")
    _abi(min(sT, sH, sW) > 0 and cin >= 64 and cin % 64 == 0 and cout > 0 and cout % 8 == 0 and x.stride(0) % 8 == 0
         and all(v in (1, 2) for v in stride), "conv3d_causal_strided")
    m = torch.arange(T * H * W)
    wt = w_taps.float().reshape(cout, 27, cin)
    acc = torch.zeros(T * H * W, cout)
    for tap in range(27):
        a = x[_gather_rows(m, tap, H, W, (sT, sH, sW), stride)][:, :cin].float()
        for k0 in range(0, cin, 64):
            acc = acc + a[:, k0:k0 + 64] @ wt[:, tap, k0:k0 + 64].T
    if bias is not None:
        acc = acc + bias.float()[None]
    r = acc.to(torch.float16)
    if out is None:
        return r, T, H, W
    out.copy_(r)
    return out, T, H, W


def cout4_weights_from_fragments(w_frag):
    """the inverse of vae_ops.cout4_weight_fragments: fp16 [7, 4, 64, 8] -> [tap 28][c 4][channel 128]"""
    return w_frag.reshape(7, 4, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(28, 4, 128)


def conv_cout4(x, affine, silu, w_frag, bias, T, H, W, cin, cout, out=None):
    """planes[tap][voxel][c] in fp32 (32-channel steps into one accumulator, as the MFMA chain), then bias + the 27 planes at the
    tap-shifted voxels in the order tap = 0..26, one rounding to fp16; columns cout..7 zero (written only where the row stride is >= 8)"""
    _chk(x, F16, "x"), _chk(w_frag, F16, "w_frag"), _chk(bias, F16, "bias")
    if affine is not None:
        _chk(affine, torch.float32, "affine")
    M = T * H * W
    assert x.shape[0] == M and x.shape[1] >= cin and tuple(w_frag.shape) == (7, 4, 64, 8), (x.shape, M, cin, w_frag.shape)
    ldo = 8 if out is None else out.stride(0)
    _abi(M > 0 and 0 < cin <= 128 and cin % 32 == 0 and 0 < cout <= 3 and x.stride(0) >= cin and x.stride(0) % 8 == 0 and ldo >= cout
         and (ldo < 8 or ldo % 8 == 0) and x.data_ptr() % 16 == 0 and (out is None or out.data_ptr() % 16 == 0), "conv_cout4")
    h = x[:, :cin].float()
    if affine is not None:
        t = h * affine[:, 0][None] + affine[:, 1][None]
        h = (t / (1.0 + torch.exp(-t)) if silu else t)
    h = h.to(torch.float16).float()
    wn = cout4_weights_from_fragments(w_frag).float()
    planes = torch.zeros(27, M, 3)
    for tap in range(27):
        for k0 in range(0, cin, 32):
            planes[tap] = planes[tap] + h[:, k0:k0 + 32] @ wn[tap, :3, k0:k0 + 32].T
    acc = torch.zeros(M, 3)
    acc[:, :cout] = bias[:cout].float()[None]
    m = torch.arange(M)
    for tap in range(27):
        acc = acc + planes[tap][_gather_rows(m, tap, H, W, (T, H, W), (1, 1, 1))]
    r = torch.zeros(M, 8, dtype=torch.float16)
    r[:, :3] = acc.to(torch.float16)
    if out is None:
        return r
    n = 8 if out.stride(0) >= 8 else cout          # ldo >= 8: one 16-byte store; below: Cout scalar stores
    out[:, :n] = r[:, :n]
    return out


# ---- VAE mid-block attention entry points (vae_ops.gemm_f16, softmax_rows, transpose_16b, groupnorm_affine, groupnorm_apply): fp32
# emulations in the kernels' own operation order and with the wrappers' argument meaning (n, k, `out` views with their row strides,
# cols_pad, causal_block, out_f32, res), so that AutoencoderKLCausal3D._mid_attention itself runs on device="cpu"
# (tests/test_mid_attention_cpu.py).  `mutant` selects one changed line of the softmax (the ways such a kernel can be subtly wrong).
def vae_gemm_f16(a, w, bias=None, out=None, out_f32=False, res=None, n=None, k=None):
    """64-wide K-tiles into one fp32 accumulator, bias added last; fp32 store, or one rounding to fp16 and then fp16(res + y)"""
    _chk(a, F16, "a"), _chk(w, F16, "w")
    m = a.shape[0]
    k = a.shape[1] if k is None else k
    n = w.shape[0] if n is None else n
    if out is not None:
        _chk(out, torch.float32 if out_f32 else F16, "out")
        _abi(out.stride(0) % 8 == 0 and _pitch_ok(m, out.stride(0), n), "gemm_f16 out")
    if bias is not None:
        _chk(bias, F16, "bias")
    if res is not None:
        _chk(res, F16, "res")
        _abi(res.stride(0) % 8 == 0, "gemm_f16 res")
    _abi(k >= 64 and k % 64 == 0 and n > 0 and n % 8 == 0 and a.stride(0) % 8 == 0 and w.stride(0) % 8 == 0
         and not (out_f32 and res is not None), "gemm_f16")
    acc = torch.zeros(m, n)
    for k0 in range(0, k, 64):
        acc = acc + a[:, k0:k0 + 64].float() @ w[:n, k0:k0 + 64].float().T
    if bias is not None:
        acc = acc + bias[:n].float()[None]
    if out is None:
        out = torch.empty(m, n, dtype=torch.float32 if out_f32 else F16)
    if out_f32:
        out[:, :n] = acc
    elif res is not None:
        out[:, :n] = (res[:, :n].float() + acc.to(F16).float()).to(F16)
    else:
        out[:, :n] = acc.to(F16)
    return out


def vae_softmax_rows(s_f32, cols, cols_pad, scale, out=None, causal_block=0, mutant=None):
    """valid(r) = cols, or min(cols, (r / causal_block + 1) * causal_block); m = max over the valid columns * scale; p = fp16(exp(s *
    scale - m) * (1 / sum)); +0 in [valid, cols_pad)"""
    _chk(s_f32, torch.float32, "S")
    rows = s_f32.shape[0]
    if out is None:
        out = torch.empty(rows, cols_pad, dtype=F16)
    _abi(rows > 0 and 0 < cols <= cols_pad and causal_block >= 0 and _pitch_ok(rows, out.stride(0), cols_pad), "softmax_rows")
    r = torch.arange(rows)
    valid = torch.full((rows,), cols)
    if causal_block > 0:
        frames = r // causal_block if mutant == "frame_index" else r // causal_block + 1
        valid = torch.clamp(frames * causal_block, max=cols)
    if mutant == "drop_last_key":
        valid = valid - 1
    ok = torch.arange(cols_pad)[None] < valid[:, None]
    sc = torch.tensor(scale, dtype=torch.float32)
    width = min(cols_pad, s_f32.shape[1])
    s = torch.full((rows, cols_pad), -math.inf)
    s[:, :width] = s_f32[:, :width]
    seen = s_f32 if mutant == "max_over_masked" else torch.where(ok, s, torch.tensor(-math.inf))
    m = seen.max(-1, keepdim=True).values * sc
    e = torch.where(ok, torch.exp(s * sc - m), torch.zeros(()))
    if mutant == "sum_after_rounding":
        e = e.to(F16).float()
    p = e * (1.0 / e.sum(-1, keepdim=True))
    out[:, :cols_pad] = p.to(torch.bfloat16).to(F16) if mutant == "bf16_p" else p.to(F16)
    return out


def vae_transpose_16b(src, dst):
    assert src.element_size() == 2 and dst.element_size() == 2
    r, c = src.shape
    _abi(r > 0 and c > 0 and _pitch_ok(c, dst.stride(0), r), "transpose_16b")
    dst[:c, :r] = src.T
    return dst


def _gn_abi(m, c, groups, what):
    """the extents hv_groupnorm_affine_f16 / hv_groupnorm_finalize_f16 accept"""
    _abi(m > 0 and c >= 8 and c % 8 == 0 and c <= 2048 and 0 < groups <= 64 and groups & (groups - 1) == 0 and c % groups == 0, what)


def vae_groupnorm_affine(x, weight, bias, groups=32, eps=1e-6):
    """sums of d = x - pivot (the group's first value of row 0) and of d^2 in fp32, folded in fp64; sc = fp32(rstd w),
    sh = fp32(b - mean sc) (gn_affine_out)"""
    _chk(x, F16, "x"), _chk(weight, F16, "weight"), _chk(bias, F16, "bias")
    m, c = x.shape
    _gn_abi(m, c, groups, "groupnorm_affine")
    _abi(x.stride(0) % 8 == 0 and 256 % (c // 8) == 0, "groupnorm_affine ldx / C")
    cpg = c // groups
    xf = x[:, :c].float().reshape(m, groups, cpg)
    pivot = xf[0, :, 0]
    d = xf - pivot[None, :, None]
    s, q = d.sum(0).double().sum(-1), (d * d).sum(0).double().sum(-1)
    n = float(m * cpg)
    md = s / n
    mean, var = pivot.double() + md, (q / n - md * md).clamp(min=0.0)
    rstd = 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))
    sc = (rstd.repeat_interleave(cpg) * weight.double()).float()
    sh = (bias.double() - mean.repeat_interleave(cpg) * sc.double()).float()
    return torch.stack([sc, sh], 1).contiguous()


def vae_groupnorm_apply(x, affine, silu, out=None):
    _chk(x, F16, "x"), _chk(affine, torch.float32, "affine")
    m, c = x.shape
    ldy = c if out is None else out.stride(0)
    _abi(m > 0 and c >= 8 and c % 8 == 0 and c <= 2048 and x.stride(0) % 8 == 0 and ldy % 8 == 0 and _pitch_ok(m, ldy, c), "groupnorm_apply")
    t = x.float() * affine[:, 0][None] + affine[:, 1][None]
    y = (t / (1.0 + torch.exp(-t)) if silu else t).to(F16)
    if out is None:
        return y
    out.copy_(y)
    return out


VAE_MID_ATTENTION_NAMES = ["gemm_f16", "softmax_rows", "transpose_16b", "groupnorm_affine", "groupnorm_apply"]


def install_vae_mid_attention(monkeypatch, softmax_mutant=None):
    """Install the five doubles on hunyuanvideo_efficiency_amd.vae_ops for the length of a test (pytest's monkeypatch undoes it)."""
    import functools
    from hunyuanvideo_efficiency_amd import vae_ops
    g = globals()
    for n in VAE_MID_ATTENTION_NAMES:
        f = g["vae_" + n]
        if n == "softmax_rows" and softmax_mutant is not None:
            f = functools.partial(f, mutant=softmax_mutant)
        monkeypatch.setattr(vae_ops, n, f)
    return vae_ops


# ---- the rest of the VAE tile coder (AutoencoderKLCausal3D._decode_tile / _encode_tile): the unit-stride conv with its fused nearest
# upsample, residual and GroupNorm statistics, the sub-pixel upsampler conv, the temporal ops, latent_tile and copy4d_, with the rounding
# points include/hv_kernels.h documents, so that the whole tile coder runs on device="cpu" (tests/test_vae_wiring_cpu.py)
def gn_stats_of(y):
    """the statistics a conv epilogue leaves for the fp16 tensor y [M, C] it stored, as ONE partial row in the documented entry format
    (include/hv_kernels.h, gn_partial): per pair of adjacent columns (c, c + 1), c even, over the k = 2 M values: [c] = (S = sum, C2 = sum
    of (x - S / k)^2), [c + 1] = (0, k) - a vae_ops.GNStats with rows = 1, which vae_groupnorm_affine_from_stats folds"""
    from hunyuanvideo_efficiency_amd.vae_ops import GNStats
    m, c = y.shape
    pair = y.double().reshape(m, c // 2, 2)
    k = 2.0 * m
    s = pair.sum((0, 2))
    c2 = ((pair - (s / k)[None, :, None]) ** 2).sum((0, 2))
    partial = torch.zeros(1, c, 2, dtype=torch.float32)
    partial[0, 0::2, 0], partial[0, 0::2, 1], partial[0, 1::2, 1] = s.float(), c2.float(), k
    return GNStats(partial, 1, m, c)


def vae_groupnorm_affine_from_stats(st, weight, bias, groups=32, eps=1e-6):
    """hv_groupnorm_finalize_f16: sum x^2 of an entry = C2 + S^2 / k, folded in fp64; sc = fp32(rstd w), sh = fp32(b - mean sc)"""
    _chk(weight, F16, "weight"), _chk(bias, F16, "bias")
    c = st.C
    _gn_abi(st.M, c, groups, "groupnorm_affine_from_stats")
    cpg = c // groups
    _abi(st.rows > 0 and cpg % 2 == 0, "groupnorm_affine_from_stats: the epilogue credits each pair of adjacent channels to the even one")
    p = st.partial.reshape(st.rows, c, 2).double()
    s, c2, k = p[:, 0::2, 0], p[:, 0::2, 1], p[:, 1::2, 1]
    q = c2 + torch.where(k > 0, s * s / k.clamp(min=1.0), torch.zeros_like(s))
    n = float(st.M * cpg)
    sg, qg = s.sum(0).reshape(groups, cpg // 2).sum(-1), q.sum(0).reshape(groups, cpg // 2).sum(-1)
    mean = sg / n
    var = (qg / n - mean * mean).clamp(min=0.0)
    rstd = 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))
    sc = (rstd.repeat_interleave(cpg) * weight.double()).float()
    sh = (bias.double() - mean.repeat_interleave(cpg) * sc.double()).float()
    return torch.stack([sc, sh], 1).contiguous()


def _up_rows(m, tap, oH, oW, src, up_t, up_hw):
    """_gather_rows at unit stride with the nearest upsample folded into the gather: clamp on the UPSAMPLED extents, then halve"""
    _, sH, sW = src
    bH, bW = sH << int(up_hw), sW << int(up_hw)
    t, h, w = m // (oH * oW), (m // oW) % oH, m % oW
    ti = (t + tap // 9 - 2).clamp(min=0)
    if up_t:
        ti = torch.where(ti == 0, ti, 1 + (ti - 1) // 2)
    hi = (h + (tap // 3) % 3 - 1).clamp(0, bH - 1) >> int(up_hw)
    wi = (w + tap % 3 - 1).clamp(0, bW - 1) >> int(up_hw)
    return (ti * sH + hi) * sW + wi


def _conv_store(acc, bias, res, out, gn_stats):
    """bias added last, one rounding to fp16, then fp16(res + y); the statistics are those of the stored tensor"""
    if bias is not None:
        acc = acc + bias.float()[None]
    r = acc.to(F16)
    if res is not None:
        r = (res[:, :r.shape[1]].float() + r.float()).to(F16)
    if out is None:
        out = r
    else:
        out.copy_(r)
    return (out, gn_stats_of(r)) if gn_stats else out


def vae_conv3d_causal(x, w_taps, bias, T, H, W, cin, cout, up_t=False, up_hw=False, res=None, out=None, gn_stats=False):
    """K-tile by K-tile (64 channels of one tap) into one fp32 accumulator over the OUTPUT grid T x H x W"""
    _chk(x, F16, "x"), _chk(w_taps, F16, "w_taps")
    assert w_taps.is_contiguous() and w_taps.numel() == cout * 27 * cin, (w_taps.shape, cout, cin)
    if res is not None:
        _chk(res, F16, "res")
        _abi(res.stride(0) % 8 == 0, "conv3d_causal res")
    _abi(T > 0 and H > 0 and W > 0 and cin >= 64 and cin % 64 == 0 and cout > 0 and cout % 8 == 0 and x.stride(0) % 8 == 0
         and (out is None or (out.stride(0) % 8 == 0 and _pitch_ok(T * H * W, out.stride(0), cout))), "conv3d_causal")
    _abi((not up_t or T % 2 == 1) and (not up_hw or (H % 2 == 0 and W % 2 == 0)), "conv3d_causal up_t / up_hw")
    src = ((T + 1) // 2 if up_t else T, H >> int(up_hw), W >> int(up_hw))
    assert x.shape[0] >= src[0] * src[1] * src[2], (tuple(x.shape), src)
    m = torch.arange(T * H * W)
    wt = w_taps.float().reshape(cout, 27, cin)
    acc = torch.zeros(T * H * W, cout)
    for tap in range(27):
        a = x[_up_rows(m, tap, H, W, src, up_t, up_hw)][:, :cin].float()
        for k0 in range(0, cin, 64):
            acc = acc + a[:, k0:k0 + 64] @ wt[:, tap, k0:k0 + 64].T
    return _conv_store(acc, bias, res, out, gn_stats)


def vae_conv3d_upsampled_subpixel(x, w_sub, table, ntap, bias, sT, sH, sW, cin, cout, up_t, out=None, gn_stats=False):
    """per parity class (pt, ph, pw) a conv over the source grid: tap j reads source voxel (max(kt + pt + ot, 0), clamp(kh + oh),
    clamp(kw + ow)) with w_sub[class][:, j cin : (j + 1) cin]; class voxel (kt, kh, kw) is output (2 kt + pt | kt, 2 kh + ph, 2 kw + pw)"""
    _chk(x, F16, "x"), _chk(w_sub, F16, "w_sub"), _chk(table, torch.int32, "tap_table")
    ncls = 8 if up_t else 4
    assert w_sub.is_contiguous() and tuple(w_sub.shape) == (ncls, cout, ntap * cin), (w_sub.shape, ncls, cout, ntap, cin)
    assert table.is_contiguous() and tuple(table.shape) == (ncls, ntap)
    T2, H2, W2 = (2 * sT - 1 if up_t else sT), 2 * sH, 2 * sW
    _abi(min(sT, sH, sW) > 0 and 1 <= ntap <= 27 and cin >= 256 and cin % 64 == 0 and cout > 128 and cout % 8 == 0 and x.stride(0) % 8 == 0
         and (out is None or (out.stride(0) % 8 == 0 and out.stride(0) >= cout)), "conv3d_upsampled_subpixel")
    acc = torch.zeros(T2 * H2 * W2, cout)
    tab = table.tolist()
    for c in range(8 if up_t else 4):
        pt, ph, pw = (c >> 2 if up_t else 0), (c >> 1) & 1, c & 1
        frames = sT - 1 if (up_t and pt) else sT
        if frames == 0:
            continue
        m = torch.arange(frames * sH * sW)
        kt, kh, kw = m // (sH * sW), (m // sW) % sH, m % sW
        a_c = torch.zeros(m.numel(), cout)
        for j in range(ntap):
            e = tab[c][j]
            ot, oh, ow = (e & 15) - 8, ((e >> 4) & 15) - 8, ((e >> 8) & 15) - 8
            rows = ((kt + pt + ot).clamp(min=0) * sH + (kh + oh).clamp(0, sH - 1)) * sW + (kw + ow).clamp(0, sW - 1)
            a = x[rows][:, :cin].float()
            wj = w_sub[c][:, j * cin:(j + 1) * cin].float()
            for k0 in range(0, cin, 64):
                a_c = a_c + a[:, k0:k0 + 64] @ wj[:, k0:k0 + 64].T
        acc[((2 * kt + pt if up_t else kt) * H2 + 2 * kh + ph) * W2 + 2 * kw + pw] = a_c
    return _conv_store(acc, bias, None, out, gn_stats)


def _temporal_abi(x, T, HW, s, k=1):
    _chk(x, F16, "x")
    _abi(T > 0 and HW > 0 and x.shape[1] > 0 and x.shape[1] % 8 == 0 and x.stride(0) % 8 == 0 and s >= 1 and k >= 1, "temporal resample")


def vae_temporal_avg_pool(x, T, HW, k, s):
    """frames t s + i - (k - 1), clamped at 0, summed in fp32 in the order i = 0 .. k - 1, times fp32(1 / k), one rounding to fp16"""
    _temporal_abi(x, T, HW, s, k)
    t_out = (T - 1) // s + 1
    xf = x.float().reshape(T, HW, x.shape[1])
    idx = (torch.arange(t_out)[:, None] * s + torch.arange(k)[None] - (k - 1)).clamp(min=0)
    acc = torch.zeros(t_out, HW, x.shape[1])
    for i in range(k):
        acc = acc + xf[idx[:, i]]
    return (acc * torch.tensor(1.0 / k, dtype=torch.float32)).to(F16).reshape(t_out * HW, x.shape[1]), t_out


def vae_temporal_nearest_up(x, T, HW, s):
    _temporal_abi(x, T, HW, s)
    return x.reshape(T, 1, HW, x.shape[1]).expand(T, s, HW, x.shape[1]).reshape(T * s * HW, x.shape[1]).clone(), T * s


def vae_temporal_linear_up(x, T, HW, s):
    """output frame t: num = max(2 t + 1 - s, 0), t0 = num // 2 s, t1 = min(t0 + 1, T - 1), lambda = fp32((num mod 2 s) / 2 s);
    y = fp16(x0 + lambda (x1 - x0)) in fp32; a bit copy of x0 where lambda = 0 or t0 = t1"""
    _temporal_abi(x, T, HW, s)
    t = torch.arange(T * s)
    num = (2 * t + 1 - s).clamp(min=0)
    t0 = num // (2 * s)
    t1 = (t0 + 1).clamp(max=T - 1)
    lam = ((num % (2 * s)).float() / float(2 * s))[:, None, None]
    xf = x.float().reshape(T, HW, x.shape[1])
    y = xf[t0] + lam * (xf[t1] - xf[t0])
    return y.to(F16).reshape(T * s * HW, x.shape[1]), T * s


def vae_latent_tile(z_f32_view, cpad):
    """[C, T, H, W] fp32 (any strides) -> channels-last fp16 [T H W, cpad]: one rounding, zero in the columns [C, cpad)"""
    _chk(z_f32_view, torch.float32, "z", False)
    c, t, h, w = z_f32_view.shape
    _abi(min(c, t, h, w) > 0 and cpad >= c, "latent_tile")
    out = torch.zeros(t * h * w, cpad, dtype=F16)
    out[:, :c] = z_f32_view.permute(1, 2, 3, 0).reshape(t * h * w, c).to(F16)
    return out


def vae_copy4d_(src_view, dst_view):
    assert src_view.shape == dst_view.shape and src_view.dim() == 4 and src_view.element_size() == 2 and dst_view.element_size() == 2
    dst_view.copy_(src_view)
    return dst_view


# vae_ops name -> the double's name in this module
VAE_TILE_CODER_NAMES = {"latent_tile": "vae_latent_tile", "gemm_f16": "vae_gemm_f16", "conv3d_causal": "vae_conv3d_causal",
                        "conv3d_upsampled_subpixel": "vae_conv3d_upsampled_subpixel", "conv3d_causal_strided": "conv3d_causal_strided",
                        "conv_cout4": "conv_cout4", "groupnorm_affine": "vae_groupnorm_affine",
                        "groupnorm_affine_from_stats": "vae_groupnorm_affine_from_stats", "groupnorm_apply": "vae_groupnorm_apply",
                        "softmax_rows": "vae_softmax_rows", "transpose_16b": "vae_transpose_16b",
                        "temporal_avg_pool": "vae_temporal_avg_pool", "temporal_nearest_up": "vae_temporal_nearest_up",
                        "temporal_linear_up": "vae_temporal_linear_up", "copy4d_": "vae_copy4d_"}


def install_vae_tile_coder(monkeypatch):
    """Install the doubles of every vae_ops entry point the tile coder calls, for the length of a test or module (monkeypatch undoes it)."""
    from hunyuanvideo_efficiency_amd import vae_ops
    g = globals()
    for n, double in VAE_TILE_CODER_NAMES.items():
        monkeypatch.setattr(vae_ops, n, g[double])
    return vae_ops


NAMES = ["ln_modulate", "qknorm_rope_", "gemm", "linear_smallm", "attn_fwd", "patchify", "unpatchify", "euler_step_",
         "masked_mean", "broadcast_row_", "timestep_embedding", "copy3d",
         "fp8_dequant", "quant_rows_fp8", "ln_modulate_fp8", "gemm_fp8"]


def install():
    """Replace the kernel wrappers of hunyuanvideo_efficiency_amd.ops with the CPU doubles (test processes only)."""
    from hunyuanvideo_efficiency_amd import ops
    g = globals()
    for n in NAMES:
        setattr(ops, n, g[n])
    return ops
