"""TEST INFRASTRUCTURE: CPU stand-ins for the C-ABI kernels (hunyuanvideo_efficiency_amd.ops.*), built on the oracle's
arithmetic, so that the HOST logic of the product (module wiring, workspaces, strided views, sequence-parallel sharding)
can run under gloo on CPU with world_size > 1.  Never imported by the product; installed by tests via `install()`."""
import math

import torch
import torch.nn.functional as F

from oracle import dit_ref as R

E = R.Prec(True)
BF16 = torch.bfloat16


def _bf(x):
    return x.to(BF16)


def ln_modulate(x, shift=None, scale=None, out=None, eps=1e-6, affine=False):
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
    n = qkv.shape[0]
    d = n_heads * 128
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


def _gemm_store(y, a_rows, out, act, n_split, out1, act1, gate, res):
    """the epilogues shared by gemm and gemm_fp8, on the rounded product y [M, N]"""
    n = y.shape[1]
    n0 = n_split if 0 < n_split < n else n
    if gate is not None:
        r = _bf(res.float() + E.r(_act(y, act) * gate.float()))
    else:
        r = _bf(_act(y[:, :n0], act))
    if out is None:
        out = torch.empty(a_rows, n0, dtype=BF16)
    out[:, :n0] = r[:, :n0]
    if n0 < n:
        out1[:, :n - n0] = _bf(_act(y[:, n0:], act1))
    return out


def gemm(a, w, bias=None, out=None, act=0, n_split=0, out1=None, act1=0, gate=None, res=None):
    y = E.r(a.float() @ w.float().T + (0 if bias is None else bias.float()))
    return _gemm_store(y, a.shape[0], out, act, n_split, out1, act1, gate, res)


# ---- the opt-in FP8-MFMA path (ops.fp8_dequant, quant_rows_fp8, ln_modulate_fp8, gemm_fp8): the contract of oracle/dit_ref.py
# (fp8_quant_rows, Fp8MfmaPrec) on CPU float8_e4m3fn tensors
FP8 = torch.float8_e4m3fn


def fp8_dequant(w8, scale_bf16, out_bf16):
    out_bf16.copy_(_bf(w8.to(BF16).float() * scale_bf16.float()).reshape(out_bf16.shape))
    return out_bf16


def quant_rows_fp8(x, out_q=None, out_scale=None):
    q, s = R.fp8_quant_rows(x.float())
    m = x.shape[0]
    if out_q is None:
        out_q = torch.empty(m, x.shape[1], dtype=FP8)
    if out_scale is None:
        out_scale = torch.empty(m, dtype=torch.float32)
    out_q.copy_(q.to(FP8))
    out_scale[:m] = s[:, 0]
    return out_q, out_scale


def ln_modulate_fp8(x, shift=None, scale=None, out_q=None, out_scale=None, eps=1e-6):
    return quant_rows_fp8(ln_modulate(x, shift, scale, eps=eps), out_q, out_scale)


def gemm_fp8(a_q, a_scale, w_q, w_scale, bias=None, out=None, act=0, n_split=0, out1=None, act1=0, gate=None, res=None):
    m = a_q.shape[0]
    y = (a_q.float() @ (w_q.float() * w_scale.float()).T) * a_scale[:m, None]
    y = E.r(y + (0 if bias is None else bias.float()))
    return _gemm_store(y, m, out, act, n_split, out1, act1, gate, res)


def linear_smallm(x, w, bias=None, silu_in=False, silu_out=False, out=None, addend=None):
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


def attn_fwd(q, k, v, out, n_heads, scale=None):
    o = R.sdpa(q.float().reshape(1, q.shape[0], n_heads, 128), k.float().reshape(1, k.shape[0], n_heads, 128),
               v.float().reshape(1, v.shape[0], n_heads, 128), E)
    out.copy_(_bf(o.reshape(q.shape[0], n_heads * 128)))
    return out


def patchify(x_f32, out=None):
    c, t, h, w = x_f32.shape
    r = _bf(x_f32.reshape(c, t, h // 2, 2, w // 2, 2).permute(1, 2, 4, 0, 3, 5).reshape(t * (h // 2) * (w // 2), c * 4))
    if out is None:
        return r
    out.copy_(r)
    return out


def unpatchify(y, c, t, h, w, out=None):
    return _bf(R.unpatchify(y.float()[None], t, h // 2, w // 2, c, [1, 2, 2])[0])


def euler_step_(sample_f32, model_out_bf16, dt):
    sample_f32.add_(model_out_bf16.float() * dt)
    return sample_f32


def masked_mean(x, mask_i32=None):
    if mask_i32 is None:
        return _bf(x.float().mean(0))
    m = mask_i32.float()[:, None]
    return _bf((x.float() * m).sum(0) / m.sum())


def broadcast_row_(src, dst):
    dst.copy_(src[None].expand_as(dst))
    return dst


def timestep_embedding(t_f32, dim=256, max_period=10000.0):
    if t_f32.dtype != torch.float32 or (t_f32.dim() > 0 and t_f32.stride(-1) != 1):     # what ops._chk refuses
        raise ValueError("t: expected fp32 with a contiguous innermost dimension")
    return _bf(R.timestep_embedding(t_f32.reshape(-1), dim, max_period))


def copy3d(src, dst, n_batch, rows, cols, src_bs, src_ld, dst_bs, dst_ld):
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
    T, H, W = ((s - 1) // m + 1 for s, m in zip((sT, sH, sW), stride))
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
    M = T * H * W
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
F16 = torch.float16


def vae_gemm_f16(a, w, bias=None, out=None, out_f32=False, res=None, n=None, k=None):
    """64-wide K-tiles into one fp32 accumulator, bias added last; fp32 store, or one rounding to fp16 and then fp16(res + y)"""
    m = a.shape[0]
    k = a.shape[1] if k is None else k
    n = w.shape[0] if n is None else n
    assert k >= 64 and k % 64 == 0 and n % 8 == 0 and not (out_f32 and res is not None), (m, n, k)
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
    rows = s_f32.shape[0]
    assert 0 < cols <= cols_pad and causal_block >= 0
    if out is None:
        out = torch.empty(rows, cols_pad, dtype=F16)
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
    r, c = src.shape
    dst[:c, :r] = src.T
    return dst


def vae_groupnorm_affine(x, weight, bias, groups=32, eps=1e-6):
    """sums of d = x - pivot (the group's first value of row 0) and of d^2 in fp32, folded in fp64; sc = fp32(rstd w),
    sh = fp32(b - mean sc) (gn_affine_out)"""
    m, c = x.shape
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
    c = st.C
    cpg = c // groups
    assert cpg % 2 == 0, "the epilogue credits each pair of adjacent channels to the even one"
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
    assert (not up_t or T % 2 == 1) and (not up_hw or (H % 2 == 0 and W % 2 == 0)), (T, H, W, up_t, up_hw)
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
    T2, H2, W2 = (2 * sT - 1 if up_t else sT), 2 * sH, 2 * sW
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


def vae_temporal_avg_pool(x, T, HW, k, s):
    """frames t s + i - (k - 1), clamped at 0, summed in fp32 in the order i = 0 .. k - 1, times fp32(1 / k), one rounding to fp16"""
    t_out = (T - 1) // s + 1
    xf = x.float().reshape(T, HW, x.shape[1])
    idx = (torch.arange(t_out)[:, None] * s + torch.arange(k)[None] - (k - 1)).clamp(min=0)
    acc = torch.zeros(t_out, HW, x.shape[1])
    for i in range(k):
        acc = acc + xf[idx[:, i]]
    return (acc * torch.tensor(1.0 / k, dtype=torch.float32)).to(F16).reshape(t_out * HW, x.shape[1]), t_out


def vae_temporal_nearest_up(x, T, HW, s):
    return x.reshape(T, 1, HW, x.shape[1]).expand(T, s, HW, x.shape[1]).reshape(T * s * HW, x.shape[1]).clone(), T * s


def vae_temporal_linear_up(x, T, HW, s):
    """output frame t: num = max(2 t + 1 - s, 0), t0 = num // 2 s, t1 = min(t0 + 1, T - 1), lambda = fp32((num mod 2 s) / 2 s);
    y = fp16(x0 + lambda (x1 - x0)) in fp32; a bit copy of x0 where lambda = 0 or t0 = t1"""
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
    c, t, h, w = z_f32_view.shape
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
