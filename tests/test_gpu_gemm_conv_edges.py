"""GPU: every GEMM / conv main loop at its tile and dispatch edges, against an fp64 reference with a per-element error bound
(tests/error_bounds.py), with every operand embedded in NaN-poisoned memory and every output in a sentinel-filled buffer.

Path table - a Python mirror of the dispatch in csrc/hv_gemm.hip (launch, launch_tiles, hv_gemm_fp8, hv_conv3d_causal_f16,
hv_conv3d_upsampled_subpixel_f16); test_path_table_matches_launched_kernels confirms it with the profiler:

    B1 gemm_kernel<BF16T,false,128>   hv_gemm_bf16, N <= 128          F1-F3: the same three for hv_gemm_f16
    B2 gemm_kernel<BF16T,false,256>   hv_gemm_bf16, N > 128, K < 192         (plain fp16 output, out_f32, res)
    B3 gemm8_kernel<BF16T>            hv_gemm_bf16, N > 128, K >= 192  Q  gemm8_kernel<FP8T>: hv_gemm_fp8, every N
    C1 gemm_kernel<F16T,true,128>     conv, Cout <= 128, Cin not a power of two >= 128
    C2 conv128_kernel                 conv, Cout <= 128, Cin a power of two >= 128, W not in {4, 8, .., 256} (or not dividing 256)
    C3 conv128s_kernel                conv, 32 < Cout <= 128, Cin a power of two >= 128, W divides 256 and W % 4 == 0
    C4 conv128s_narrow_kernel         as C3 with Cout <= 32
    C5 gemm8_kernel<F16T,true>        conv, Cout > 128, Cin a power of two >= 256
    C6 gemm_kernel<F16T,true,256>     conv, Cout > 128, otherwise
    SP gemm8_kernel<F16T,true,true>   the sub-pixel upsampling conv
In launch()'s own terms (conv_path): the pipelined loops C2 - C5 need packed coordinates, cT * mt < 256 and clamp extents bH, bW <= 4096
(conv_fits_packing), else C1 / C6; the W-shift-reuse kernels C3 / C4 need mw == 1 and bW == cW on top of the W conditions.  The strided
entry point (hv_conv3d_causal_strided_f16: mt / mh / mw of 1 or 2, bH / bW the SOURCE extents) goes through the same launch(), so a
stride of 2 along W always leaves C3 / C4 for C2.

Shapes: M in {1, 255, 257}; tiles_m in {5, 6, 7, 9} with tiles_n >= 2 and a grid that is not a multiple of 8 (a short last band
of GROUP_M = 4 M-tiles, and the XCD remap with a remainder); N = 256 k + 8 and N = BN - 8; the smallest K of each main loop and
an odd K-tile count; convs at T = H = W = 1, M % 256 in {1, 255}, Cout from 8 to 264 across the narrow / 128 / 256 boundaries.
Strided convs (STRIDED_CASES, source grid and stride): every path with a stride of 2 on each axis it admits (C5: all seven strides that
are not all ones); 1x1x1 and 2x2x2 sources at stride (2,2,2) (M = 1, every tap clamped); odd and even source extents on each strided
axis (the odd one makes the last output read one past the source and clamp at the SOURCE extent); several M tiles with M % 256 in
{1, 255} on C1, C2, C5, C6 and in {4, 252} on C3 / C4, whose W % 4 == 0 makes M a multiple of 4; stride (1,1,1) bit-equal to
hv_conv3d_causal_f16.  Both sides of the packing guard (PACK_CASES, STRIDED_PACK_CASES, SP_PACK_CASES): T = 255 | 256, H and W = 4096 |
4097 at unit stride; sT = 254 | 255 with stride_t 2 (cT mt = 254 | 256), source H and W = 4096 | 4097 with a stride of 2 (largest packed
coordinate 4094); the sub-pixel form at sT = 254 (accepted) and 255 (refused as a bad argument, the output untouched).

Checks per case: the plain output within the fp64 bound; GELU / SiLU within 1 ulp of the oracle's formula on the kernel's own y (random
y of size 0.5; the whole 16-bit domain, with the tail where that sentence does not hold, is tests/test_gpu_activation_domain.py);
gate + residual (in place and not) and res bit-equal to the oracle's formula; column splits bit-equal to the unsplit launch;
poison (NaN rows before / after the operand, columns in [K, ld)) never reaches an output; sentinel cells around every output
keep their bits; a dense-operand launch and a repeated launch give the same bits.  The largest error-to-bound ratio of each
path is printed at the end (test_zz_ratio_report) and must be above 0.05 - a bound that loose would catch nothing."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from hunyuanvideo_efficiency_amd import synthetic as syn  # noqa: E402
from oracle import dit_ref as R  # noqa: E402
from oracle import vae_enc_ref as VE  # noqa: E402
from oracle import vae_ref as VR  # noqa: E402
from tests import conv_bounds as CB  # noqa: E402
from tests import error_bounds as EB  # noqa: E402
from tests.guarded_memory import INT, NAN_BITS, SENT, Guarded, Poisoned, bits, poisoned_vec, same_bits  # noqa: E402,F401

DEV = "cuda"
E = R.Prec(True)
BF16, F16, F32, FP8 = torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn
RATIOS = {}


@pytest.fixture(scope="module")
def ops():
    from hunyuanvideo_efficiency_amd import ops as _ops, _lib
    _lib.load()
    return _ops


@pytest.fixture(scope="module")
def V():
    from hunyuanvideo_efficiency_amd import vae_ops, _lib
    _lib.load()
    return vae_ops


def U(shape, key, scale=1.0):
    return syn.hashed_uniform(shape, key, 17, DEV) * (scale * math.sqrt(3.0))


def _record(path, r):
    RATIOS[path] = max(RATIOS.get(path, 0.0), r)


# ------------------------------------------------------------------------------------------------------ the dispatcher's mirror
def gemm_path(kind, N, K):
    if kind == "fp8":
        return "Q"                                   # hv_gemm_fp8 -> gemm8_kernel<FP8T> for every N
    p = "B" if kind == "bf16" else "F"
    if N <= 128:
        return p + "1"                               # launch(): N <= 128 -> gemm_kernel<.., 128>
    return p + ("3" if K >= 3 * 64 else "2")       # K >= 3 BK -> gemm8_kernel (HV_GEMM_2STAGE unset)


def conv_path(T, H, W, cin, cout, stride=(1, 1, 1), src=None):
    """launch<F16T, true>: T x H x W is the OUTPUT grid (cT, cH, cW), stride = (mt, mh, mw), src the source extents (sT, sH, sW) of the
    strided entry point, whose clamp extents bH / bW are the source's; hv_conv3d_causal_f16 (src None) has bH = cH, bW = cW, upsampled or not"""
    mt, mh, mw = stride
    bH, bW = (H, W) if src is None else src[1:]
    pow2, fits = cin & (cin - 1) == 0, T * mt < 256 and bH <= 4096 and bW <= 4096
    if cout <= 128:
        if pow2 and cin >= 128 and (27 * cin // 64) % 3 == 0 and 27 * cin // 64 >= 6 and fits:
            if mw == 1 and bW == W and W <= 256 and 256 % W == 0 and W % 4 == 0:
                return "C4" if cout <= 32 else "C3"
            return "C2"
        return "C1"
    return "C5" if pow2 and cin >= 256 and fits else "C6"


KERNELS = {        # path -> (demangled name without "(anonymous namespace)::", mangled fragment)
    "B1": ("gemm_kernel<BF16T, false, 128>", "11gemm_kernelINS_5BF16TELb0ELi128E"),
    "B2": ("gemm_kernel<BF16T, false, 256>", "11gemm_kernelINS_5BF16TELb0ELi256E"),
    "B3": ("gemm8_kernel<BF16T, false, false>", "12gemm8_kernelINS_5BF16TELb0ELb0E"),
    "F1": ("gemm_kernel<F16T, false, 128>", "11gemm_kernelINS_4F16TELb0ELi128E"),
    "F2": ("gemm_kernel<F16T, false, 256>", "11gemm_kernelINS_4F16TELb0ELi256E"),
    "F3": ("gemm8_kernel<F16T, false, false>", "12gemm8_kernelINS_4F16TELb0ELb0E"),
    "Q": ("gemm8_kernel<FP8T, false, false>", "12gemm8_kernelINS_4FP8TELb0ELb0E"),
    "C1": ("gemm_kernel<F16T, true, 128>", "11gemm_kernelINS_4F16TELb1ELi128E"),
    "C2": ("conv128_kernel(", "14conv128_kernelE"),
    "C3": ("conv128s_kernel(", "15conv128s_kernelE"),
    "C4": ("conv128s_narrow_kernel(", "22conv128s_narrow_kernelE"),
    "C5": ("gemm8_kernel<F16T, true, false>", "12gemm8_kernelINS_4F16TELb1ELb0E"),
    "C6": ("gemm_kernel<F16T, true, 256>", "11gemm_kernelINS_4F16TELb1ELi256E"),
    "SP": ("gemm8_kernel<F16T, true, true>", "12gemm8_kernelINS_4F16TELb1ELb1E"),
}


def kernel_path(name):
    plain = name.replace("(anonymous namespace)::", "")
    hits = [p for p, (dem, mang) in KERNELS.items() if plain.startswith(dem) or (" " + dem) in plain or mang in name]
    return hits[0] if len(hits) == 1 else None


def within_ulp(got, ref, dtype):
    g, r = got.double(), ref.double()
    tol = torch.maximum(EB.ulp_out(g, dtype), EB.ulp_out(r, dtype))
    return float(((g - r).abs() / tol).max())


# ------------------------------------------------------------------------------------------------------ GEMM rows
def _gemm_cases():
    c = []
    # B1 / F1: N <= 128 (tiles_n = 1: the short band with tiles_m 5, 6, 7, 9 is the whole grid)
    for M, N, K in [(1, 8, 64), (255, 64, 192), (257, 120, 64), (1100, 8, 64), (1281, 120, 128), (1700, 64, 64), (2049, 120, 192)]:
        c += [("bf16", M, N, K), ("f16", M, N, K)]
    # B2 / F2: N > 128, K < 192 (K-tile counts 1 and 2)
    for M, N, K in [(1, 264, 64), (255, 248, 128), (257, 264, 64), (1100, 264, 128), (1281, 520, 64), (1700, 520, 128),
                    (2049, 264, 64)]:
        c += [("bf16", M, N, K), ("f16", M, N, K)]
    # B3 / F3: the pipelined loop: K = 192 (3 K-tiles: its smallest), 320 / 448 (odd counts), 256 (even)
    for M, N, K in [(1, 264, 192), (255, 248, 320), (257, 520, 192), (1100, 264, 320), (1281, 520, 256), (1700, 264, 448),
                    (2049, 520, 192)]:
        c += [("bf16", M, N, K), ("f16", M, N, K)]
    # Q: fp8 with 128-byte K-tiles: K = 384 (3 tiles: smallest), 640 (5: odd), 512; N from 8 (one column group) up
    for M, N, K in [(1, 8, 384), (255, 64, 640), (257, 248, 384), (1100, 264, 512), (1281, 520, 384), (1700, 8, 640),
                    (2049, 264, 384), (300, 120, 384)]:
        c.append(("fp8", M, N, K))
    return c


GEMM_CASES = _gemm_cases()


def _gemm_operands(kind, M, N, K):
    """the exact operand values the kernel sees (on the GPU), and the fp64 reference"""
    key = f"{kind}.{M}.{N}.{K}"
    if kind == "fp8":
        a = U((M, K), key + ".a", 0.5)
        w = U((N, K), key + ".w", 1.0 / math.sqrt(K))
        b = U((N,), key + ".b", 0.05).to(BF16)
        ws = (w.abs().max() / 448.0).to(BF16)
        w8 = (w / ws.float()).clamp(-448, 448).to(FP8)
        a8 = torch.empty(M, K, dtype=FP8, device=DEV)
        asc = torch.empty(M, dtype=F32, device=DEV)
        amax = a.abs().amax(1).clamp(min=1e-12)
        asc.copy_(amax / 448.0)
        a8.copy_((a / asc[:, None]).clamp(-448, 448).to(FP8))
        ref = EB.gemm_ref(a8.double() * asc.double()[:, None], w8.double() * ws.double(), b)
        return dict(a=a8, w=w8, b=b, asc=asc, ws=ws.reshape(1)), ref, BF16
    dt = BF16 if kind == "bf16" else F16
    a = U((M, K), key + ".a").to(dt)
    w = U((N, K), key + ".w", 0.5 / math.sqrt(K)).to(dt)       # y ~ 0.5: GELU / SiLU stay where 1 ulp is a fair test
    b = U((N,), key + ".b", 0.05).to(dt)
    return dict(a=a, w=w, b=b), EB.gemm_ref(a, w, b), dt


def _launcher(ops, V, kind, opnd):
    if kind == "fp8":
        return lambda a, w, b, **kw: ops.gemm_fp8(a, opnd["asc_p"], w, opnd["ws"], b, **kw)
    if kind == "bf16":
        return lambda a, w, b, **kw: ops.gemm(a, w, b, **kw)
    return lambda a, w, b, **kw: V.gemm_f16(a, w, b, **kw)


@pytest.mark.parametrize("kind,M,N,K", GEMM_CASES, ids=[f"{gemm_path(k, n, kk)}-{k}-{m}x{n}x{kk}" for k, m, n, kk in GEMM_CASES])
def test_gemm_edges(ops, V, kind, M, N, K):
    path = gemm_path(kind, N, K)
    opnd, ref, dt = _gemm_operands(kind, M, N, K)
    pad = 32 if kind == "fp8" else 24                                    # keeps the row strides legal (16 B / 8 elements)
    A, W = Poisoned(opnd["a"], 3, 5, pad), Poisoned(opnd["w"], 2, 7, pad + 16)
    bias = poisoned_vec(opnd["b"])
    if kind == "fp8":
        opnd["asc_p"] = poisoned_vec(opnd["asc"])
    run = _launcher(ops, V, kind, opnd)
    what = f"{path} {kind} {M}x{N}x{K}"

    # 1. accumulation: the plain output against the fp64 bound; guard cells and poison untouched
    o = Guarded(M, N, dt, c0=8)
    run(A.view, W.view, bias, out=o.view)
    assert o.intact(), f"{what}: a store outside the output"
    y = o.view.clone()
    _record(path, EB.check(y, ref, dt, what, worst_case=kind == "fp8"))     # fp8 MFMA: see tests/error_bounds.py
    # 5. run-to-run identity, and the same bits from dense operands
    run(A.view, W.view, bias, out=o.view)
    assert same_bits(o.view, y), f"{what}: a second launch differs"
    dense = run(opnd["a"].contiguous(), opnd["w"].contiguous(), opnd["b"].contiguous())
    assert same_bits(dense, y), f"{what}: strided NaN-padded operands give other bits than dense ones"

    yf = y.float()
    res = U((M, N), f"{what}.res").to(dt)
    Rs = Poisoned(res, 1, 4, 16)
    if kind == "f16":
        # fp32 output (the attention scores' out_f32): its own bound, a guarded fp32 buffer
        o32 = Guarded(M, N, F32, c0=8)
        run(A.view, W.view, bias, out=o32.view, out_f32=True)
        assert o32.intact(), f"{what}: out_f32 store outside the output"
        _record(path + ".f32", EB.check(o32.view, ref, F32, what + " out_f32"))
        # residual: out = fp16(res + y), bit-equal
        o2 = Guarded(M, N, dt, c0=16)
        run(A.view, W.view, bias, out=o2.view, res=Rs.view)
        assert o2.intact() and Rs.intact()
        assert same_bits(o2.view, (res.float() + yf).to(dt)), f"{what}: residual epilogue"
    else:
        # 2. epilogues on the kernel's own y
        for act, f in ((ops.ACT_GELU_TANH, lambda v: R.gelu_tanh(v, E)), (ops.ACT_SILU, lambda v: E.r(torch.nn.functional.silu(v)))):
            og = Guarded(M, N, dt, c0=8)
            run(A.view, W.view, bias, out=og.view, act=act)
            assert og.intact()
            r = within_ulp(og.view, f(yf), dt)
            assert r <= 1.0, f"{what}: activation {act} is {r:.3g} ulp from the oracle's formula on the kernel's y"
        gate = poisoned_vec(U((N,), f"{what}.g", 0.5).to(dt))
        want = R.gate_residual(res.float()[None], yf[None], gate.float()[None], E)[0]
        og = Guarded(M, N, dt, c0=8)
        run(A.view, W.view, bias, out=og.view, gate=gate, res=Rs.view)
        assert og.intact() and Rs.intact() and same_bits(og.view, want.to(dt)), f"{what}: gate + residual out of place"
        run(A.view, W.view, bias, out=Rs.view, gate=gate, res=Rs.view)                # in place: out is res
        assert Rs.intact() and same_bits(Rs.view, want.to(dt)), f"{what}: gate + residual in place"
        # column splits: at 8, at 264 (inside a 256-wide tile, not a multiple of 64), at N - 8
        for ns in sorted({s for s in (8, 264, N - 8) if 8 <= s < N}):
            o0, o1 = Guarded(M, ns, dt, c0=0), Guarded(M, N - ns, dt, c0=24)
            run(A.view, W.view, bias, out=o0.view, n_split=ns, out1=o1.view)
            assert o0.intact() and o1.intact(), f"{what}: split {ns} stores outside out0 / out1"
            assert same_bits(o0.view, y[:, :ns]) and same_bits(o1.view, y[:, ns:]), f"{what}: split at {ns}"
    assert A.intact() and W.intact()


# ------------------------------------------------------------------------------------------------------ conv rows
conv_ref = CB.conv_ref        # the fp64 im2col reference, strided or upsampled (tests/conv_bounds.py)


def subpixel_ref(x, w_sub, table, ntap, b, sT, sH, sW, cin, cout, up_t):
    """fp64 reference of hv_conv3d_upsampled_subpixel_f16 from its own operands: class c = (pt, ph, pw) is a conv over the source
    grid (frame coordinate kt + pt), tap j reading source voxel (max(k_t + ot, 0), clamp(kh + oh), clamp(kw + ow)) with weights
    w_sub[c][:, j*cin:(j+1)*cin]; class voxel (kt, kh, kw) is output (2 kt + pt | kt, 2 kh + ph, 2 kw + pw)"""
    dev = x.device
    T2, H2, W2 = (2 * sT - 1 if up_t else sT), 2 * sH, 2 * sW
    ncls = 8 if up_t else 4
    y = torch.zeros(T2 * H2 * W2, cout, dtype=torch.float64, device=dev)
    sq, sa, seen = torch.zeros_like(y), torch.zeros_like(y), torch.zeros(T2 * H2 * W2, dtype=torch.int32, device=dev)
    tab = table.cpu().tolist()
    for c in range(ncls):
        pt, ph, pw = (c >> 2 if up_t else 0), (c >> 1) & 1, c & 1
        frames = sT - 1 if (up_t and pt) else sT
        if frames == 0:
            continue
        m = torch.arange(frames * sH * sW, device=dev)
        kt, kh, kw = m // (sH * sW), (m // sW) % sH, m % sW
        r = EB.Ref()
        for j in range(ntap):
            e = tab[c][j]
            ot, oh, ow = (e & 15) - 8, ((e >> 4) & 15) - 8, ((e >> 8) & 15) - 8
            src = ((kt + pt + ot).clamp(min=0) * sH + (kh + oh).clamp(0, sH - 1)) * sW + (kw + ow).clamp(0, sW - 1)
            r.add(x[src], w_sub[c][:, j * cin:(j + 1) * cin])
        rows = ((2 * kt + pt if up_t else kt) * H2 + 2 * kh + ph) * W2 + 2 * kw + pw
        y[rows], sq[rows], sa[rows] = r.y, r.sq, r.s
        seen[rows] += 1
    assert bool((seen == 1).all())
    ref = EB.Ref()
    ref.y, ref.sq, ref.s, ref.k = y, sq, sa, ntap * cin
    return ref.bias(b)


CONV_CASES = [   # T, H, W, cin, cout, up_t, up_hw  (output grid)
    # C1: Cin 64 (2-stage 256 x 128 tile)
    (1, 1, 1, 64, 8, 0, 0), (3, 5, 17, 64, 40, 0, 0), (1, 1, 257, 64, 120, 0, 0), (5, 9, 29, 64, 128, 0, 0), (2, 4, 6, 64, 32, 0, 1),
    # C2: conv128 (per-tap pipelined 256 x 128): W = 1 (all clamps), W = 17 / 257 (not dividing 256), an upsampled W = 10
    (1, 1, 1, 128, 128, 0, 0), (3, 5, 17, 128, 120, 0, 0), (1, 1, 257, 128, 40, 0, 0), (3, 6, 10, 128, 128, 1, 1), (1, 3, 6, 256, 32, 0, 0),
    # C3 / C4: the W-shift-reuse kernel at W = 4 (admitted, never tested before), both sides of the narrow boundary (32 / 40)
    (1, 3, 4, 128, 40, 0, 0), (1, 3, 4, 128, 32, 0, 0), (2, 5, 64, 128, 40, 0, 0), (2, 5, 64, 128, 32, 0, 0), (2, 5, 256, 128, 120, 0, 0),
    (3, 4, 32, 256, 8, 0, 0), (2, 6, 16, 128, 128, 0, 1), (4, 9, 32, 256, 128, 0, 0),
    # C5: pipelined 256 x 256 (Cin 256 / 512): clamps, M % 256 = 255 / 1, a short band (tiles_m 6, 7) with an 8-column N tail
    (1, 1, 1, 256, 136, 0, 0), (3, 5, 17, 256, 264, 0, 0), (1, 1, 257, 512, 136, 0, 0), (5, 9, 29, 256, 264, 0, 0),
    (5, 11, 29, 256, 136, 0, 0), (3, 7, 13, 256, 256, 0, 0),
    # C6: 2-stage 256 x 256 (Cin 64 / 128)
    (1, 1, 1, 64, 136, 0, 0), (3, 5, 17, 64, 264, 0, 0), (5, 9, 29, 64, 136, 0, 0), (5, 11, 29, 64, 264, 0, 0), (1, 3, 5, 128, 256, 0, 0),
]
# both sides of conv_fits_packing() at unit stride: (T, H, W, cin, cout, the path conv_path must predict)
PACK_CASES = [
    (255, 1, 2, 128, 40, "C2"), (256, 1, 2, 128, 40, "C1"), (255, 1, 2, 256, 136, "C5"), (256, 1, 2, 256, 136, "C6"),
    (255, 1, 4, 128, 40, "C3"), (256, 1, 4, 128, 40, "C1"),
    (1, 1, 4096, 128, 8, "C2"), (1, 1, 4097, 128, 8, "C1"), (1, 1, 4096, 256, 136, "C5"), (1, 1, 4097, 256, 136, "C6"),
    (1, 4096, 1, 128, 8, "C2"), (1, 4097, 1, 128, 8, "C1"), (1, 4096, 1, 256, 136, "C5"), (1, 4097, 1, 256, 136, "C6"),
]


def _strided_cases():
    c = [  # source T, H, W, cin, cout, stride
        # C1: Cin 64
        (1, 1, 1, 64, 8, (2, 2, 2)), (2, 2, 2, 64, 40, (2, 2, 2)), (5, 37, 17, 64, 128, (2, 2, 2)), (3, 10, 34, 64, 120, (1, 2, 2)),
        (7, 6, 17, 64, 40, (2, 1, 1)), (6, 62, 22, 64, 32, (2, 2, 2)),
        # C2: Cin 128, a stride of 2 along W (never the W-shift-reuse kernel); source W 17 -> 9 (513 rows), 22 -> 11 (1023 rows)
        (1, 1, 1, 128, 128, (2, 2, 2)), (2, 2, 2, 128, 40, (2, 2, 2)), (5, 37, 17, 128, 120, (2, 2, 2)), (6, 62, 22, 128, 40, (2, 2, 2)),
        # C5: Cin 256 / 512, the seven strides; 513 / 1023 / 255 rows
        (1, 1, 1, 256, 136, (2, 2, 2)), (2, 2, 2, 512, 264, (2, 2, 2)), (5, 37, 17, 256, 264, (2, 2, 2)), (6, 62, 22, 512, 136, (2, 2, 2)),
        (3, 10, 34, 256, 136, (1, 2, 2)), (6, 5, 33, 512, 264, (2, 1, 2)), (5, 10, 17, 256, 264, (2, 2, 1)), (3, 19, 18, 256, 136, (1, 1, 2)),
        (3, 37, 9, 512, 136, (1, 2, 1)), (5, 19, 9, 256, 264, (2, 1, 1)),
        # C6: Cin 64 / 128, Cout 136
        (2, 2, 2, 64, 136, (2, 2, 2)), (1, 1, 1, 128, 136, (2, 2, 2)), (5, 37, 17, 64, 136, (2, 2, 2)), (6, 62, 22, 128, 136, (2, 2, 2)),
    ]
    # C3 (Cout 40 / 128) and C4 (Cout 8 / 32): unit stride along W, source W in {4, 16, 64}; odd and even sT / sH; 260, 1020 rows (M % 256
    # = 4 / 252), 816, 960, 96
    for co_a, co_b in ((40, 128), (8, 32)):
        c += [(9, 13, 4, 128, co_a, (2, 1, 1)), (10, 13, 4, 128, co_b, (2, 1, 1)), (3, 170, 4, 128, co_a, (1, 2, 1)),
              (3, 33, 16, 128, co_b, (1, 2, 1)), (5, 9, 64, 128, co_a, (2, 2, 1)), (4, 6, 16, 128, co_b, (2, 2, 1))]
    return c


STRIDED_CASES = _strided_cases()
STRIDED_PACK_CASES = [   # source T, H, W, cin, cout, stride, the path: cT mt = 254 | 256; source H, W = 4096 (largest packed 4094) | 4097
    (254, 1, 2, 128, 40, (2, 1, 1), "C2"), (255, 1, 2, 128, 40, (2, 1, 1), "C1"), (254, 2, 1, 256, 136, (2, 1, 1), "C5"),
    (255, 2, 1, 256, 136, (2, 1, 1), "C6"), (1, 4096, 1, 128, 8, (1, 2, 1), "C2"), (1, 4097, 1, 128, 8, (1, 2, 1), "C1"),
    (1, 4096, 2, 256, 136, (1, 2, 1), "C5"), (1, 4097, 2, 256, 136, (1, 2, 1), "C6"), (1, 1, 4096, 128, 8, (1, 1, 2), "C2"),
    (1, 1, 4097, 128, 8, (1, 1, 2), "C1"),
]
UNIT_STRIDE_CASES = [(2, 3, 5, 64, 40), (2, 3, 12, 128, 128), (2, 3, 8, 128, 40), (2, 3, 8, 128, 32), (2, 3, 5, 256, 136), (2, 3, 5, 64, 136)]
SP_PACK_CASES = [(254, 1, 1, 256, 136, 0), (254, 1, 1, 256, 136, 1)]        # sT + 1 = 255 < 256: accepted; sT = 255 is refused
SP_CASES = [(1, 1, 1, 256, 136, 1), (2, 3, 5, 256, 264, 1), (3, 5, 7, 256, 136, 0), (3, 9, 13, 256, 264, 1), (2, 5, 6, 512, 256, 0)]


def _conv_check(V, path, what, run, ref, M, cout, gn_ok, label=None):
    """run(x_sel, w_sel, out=..., res=..., gn_stats=...) -> out [, st]; x_sel / w_sel: 'poisoned' or 'dense'"""
    o = Guarded(M, cout, F16, c0=8)
    run("poisoned", out=o.view)
    assert o.intact(), f"{what}: a store outside the output"
    y = o.view.clone()
    _record(label or path, EB.check(y, ref, F16, what))
    run("poisoned", out=o.view)
    assert same_bits(o.view, y), f"{what}: a second launch differs"
    assert same_bits(run("dense"), y), f"{what}: strided NaN-padded operands give other bits than dense ones"
    if gn_ok:
        gw, gb = (1 + U((cout,), what + ".gw", 0.1)).to(F16), U((cout,), what + ".gb", 0.1).to(F16)
        og = Guarded(M, cout, F16, c0=8)
        out, st = run("poisoned", out=og.view, gn_stats=True)
        assert og.intact() and same_bits(og.view, y)
        torch.testing.assert_close(V.groupnorm_affine_from_stats(st, gw, gb), V.groupnorm_affine(og.view, gw, gb), rtol=2e-5, atol=2e-6)
    return y


def _conv_case(V, T, H, W, cin, cout, up_t, up_hw, label=None):
    path = conv_path(T, H, W, cin, cout)
    what = f"{path} conv {T}x{H}x{W} {cin}->{cout} up {up_t}{up_hw}"
    sT, sH, sW = ((T + 1) // 2 if up_t else T), H >> up_hw, W >> up_hw
    M = T * H * W
    x = U((sT * sH * sW, cin), what + ".x").to(F16)
    w = U((cout, 27 * cin), what + ".w", 1.0 / math.sqrt(27 * cin)).to(F16)
    b = U((cout,), what + ".b", 0.1).to(F16)
    X, Wp = Poisoned(x, 2, 6, 40), Poisoned(w, 0, 5, 0)        # weights: rows >= Cout (ldw is 27 Cin by the ABI)
    bias = poisoned_vec(b)
    ops_x = {"poisoned": (X.view, Wp.view, bias), "dense": (x, w, b)}

    def run(sel, **kw):
        xs, ws, bs = ops_x[sel]
        return V.conv3d_causal(xs, ws, bs, T, H, W, cin, cout, up_t=bool(up_t), up_hw=bool(up_hw), **kw)

    ref = conv_ref(x, w, b, T, H, W, cin, cout, up_t, up_hw)
    if M * cout * cin <= 1 << 24:      # the gather above against the oracle's own padding / upsampling (fp64, no rounding)
        x5 = x.cpu().double().reshape(sT, sH, sW, cin).permute(3, 0, 1, 2)[None]
        if up_t or up_hw:
            x5 = VR.upsample_causal(x5, (2 if up_t else 1, 2 if up_hw else 1, 2 if up_hw else 1))
        w5 = w.cpu().double().reshape(cout, 3, 3, 3, cin).permute(0, 4, 1, 2, 3)
        o5 = VR.causal_conv3d(x5, w5, b.cpu().double(), VR.FP32)[0].permute(1, 2, 3, 0).reshape(M, cout)
        torch.testing.assert_close(ref.y.cpu(), o5, rtol=1e-12, atol=1e-12)
    y = _conv_check(V, path, what, run, ref, M, cout, cout % 64 == 0, label)
    # residual epilogue: fp16(res + y), bit-equal; poison around res untouched
    res = U((M, cout), what + ".res").to(F16)
    Rs = Poisoned(res, 1, 3, 16)
    o = Guarded(M, cout, F16, c0=8)
    run("poisoned", out=o.view, res=Rs.view)
    assert o.intact() and Rs.intact() and same_bits(o.view, (res.float() + y.float()).to(F16)), f"{what}: residual epilogue"
    assert X.intact() and Wp.intact()


@pytest.mark.parametrize("T,H,W,cin,cout,up_t,up_hw", CONV_CASES,
                         ids=[f"{conv_path(*c[:5])}-{'x'.join(map(str, c[:3]))}-{c[3]}to{c[4]}{'-up' if c[5] or c[6] else ''}" for c in CONV_CASES])
def test_conv_edges(V, T, H, W, cin, cout, up_t, up_hw):
    _conv_case(V, T, H, W, cin, cout, up_t, up_hw)


@pytest.mark.parametrize("T,H,W,cin,cout,path", PACK_CASES, ids=[f"{c[5]}-{'x'.join(map(str, c[:3]))}-{c[3]}to{c[4]}" for c in PACK_CASES])
def test_conv_packing_guard(V, T, H, W, cin, cout, path):
    """T = 255 | 256 and H, W = 4096 | 4097: the last coordinates the 8 + 12 + 12 bit packing holds, and the first the 2-stage loops take"""
    assert conv_path(T, H, W, cin, cout) == path
    _conv_case(V, T, H, W, cin, cout, 0, 0, label=path + ".pack")


def _strided_case(V, sT, sH, sW, cin, cout, stride, label):
    src = (sT, sH, sW)
    T, H, W = CB.out_grid(src, stride)
    path = conv_path(T, H, W, cin, cout, stride, src)
    what = f"{path} strided conv {sT}x{sH}x{sW} / {stride} {cin}->{cout}"
    M = T * H * W
    x = U((sT * sH * sW, cin), what + ".x").to(F16)
    w = U((cout, 27 * cin), what + ".w", 1.0 / math.sqrt(27 * cin)).to(F16)
    b = U((cout,), what + ".b", 0.1).to(F16)
    X, Wp = Poisoned(x, 2, 6, 40), Poisoned(w, 0, 5, 0)
    bias = poisoned_vec(b)
    ops_x = {"poisoned": (X.view, Wp.view, bias), "dense": (x, w, b)}

    def run(sel, **kw):
        xs, ws, bs = ops_x[sel]
        out, T_, H_, W_ = V.conv3d_causal_strided(xs, ws, bs, sT, sH, sW, cin, cout, stride, **kw)
        assert (T_, H_, W_) == (T, H, W)
        return out

    ref = conv_ref(x, w, b, T, H, W, cin, cout, stride=stride, src=src)
    if M * cout * cin <= 1 << 22:      # against the oracle's own replicate padding + strided Conv3d (fp64, no rounding)
        x5 = x.cpu().double().reshape(sT, sH, sW, cin).permute(3, 0, 1, 2)[None]
        w5 = w.cpu().double().reshape(cout, 3, 3, 3, cin).permute(0, 4, 1, 2, 3)
        o5 = VE.causal_conv3d_strided(x5, w5, b.cpu().double(), stride, VR.FP32)[0].permute(1, 2, 3, 0).reshape(M, cout)
        torch.testing.assert_close(ref.y.cpu(), o5, rtol=1e-12, atol=1e-12)
    _conv_check(V, path, what, run, ref, M, cout, False, label=path + label)
    assert X.intact() and Wp.intact()
    return path


def _sid(c):
    src, stride = c[:3], c[5]
    return f"{conv_path(*CB.out_grid(src, stride), c[3], c[4], stride, src)}-{'x'.join(map(str, src))}-s{''.join(map(str, stride))}-{c[3]}to{c[4]}"


@pytest.mark.parametrize("sT,sH,sW,cin,cout,stride", STRIDED_CASES, ids=[_sid(c) for c in STRIDED_CASES])
def test_strided_conv_edges(V, sT, sH, sW, cin, cout, stride):
    _strided_case(V, sT, sH, sW, cin, cout, stride, ".strided")


def test_strided_cases_cover_every_path_and_stride():
    """the table of the cases, checked: every path with a stride of 2 on each axis it admits, C5 with all seven strides, ragged tiles"""
    seen = {}
    for sT, sH, sW, cin, cout, stride in STRIDED_CASES:
        T, H, W = CB.out_grid((sT, sH, sW), stride)
        seen.setdefault(conv_path(T, H, W, cin, cout, stride, (sT, sH, sW)), []).append((stride, T * H * W))
    assert sorted(seen) == ["C1", "C2", "C3", "C4", "C5", "C6"]
    for path, rows in seen.items():
        axes = (0, 1) if path in ("C3", "C4") else (0, 1, 2)
        assert all(any(s[a] == 2 for s, _ in rows) for a in axes), path
        assert any(m > 256 and m % 256 in ((4, 252) if path in ("C3", "C4") else (1, 255)) for _, m in rows), path
        assert any(m == 1 for _, m in rows) or path in ("C3", "C4"), path
    assert len({s for s, _ in seen["C5"]}) == 7


@pytest.mark.parametrize("sT,sH,sW,cin,cout,stride,path", STRIDED_PACK_CASES,
                         ids=[f"{c[6]}-{'x'.join(map(str, c[:3]))}-s{''.join(map(str, c[5]))}-{c[3]}to{c[4]}" for c in STRIDED_PACK_CASES])
def test_strided_conv_packing_guard(V, sT, sH, sW, cin, cout, stride, path):
    assert _strided_case(V, sT, sH, sW, cin, cout, stride, ".spack") == path


@pytest.mark.parametrize("T,H,W,cin,cout", UNIT_STRIDE_CASES, ids=[f"{conv_path(*c)}-{'x'.join(map(str, c[:3]))}-{c[3]}to{c[4]}" for c in UNIT_STRIDE_CASES])
def test_strided_entry_at_unit_stride_is_the_plain_conv(V, T, H, W, cin, cout):
    what = f"unit stride {T}x{H}x{W} {cin}->{cout}"
    x = U((T * H * W, cin), what + ".x").to(F16)
    w = U((cout, 27 * cin), what + ".w", 1.0 / math.sqrt(27 * cin)).to(F16)
    b = U((cout,), what + ".b", 0.1).to(F16)
    got, T_, H_, W_ = V.conv3d_causal_strided(x, w, b, T, H, W, cin, cout, (1, 1, 1))
    assert (T_, H_, W_) == (T, H, W) and same_bits(got, V.conv3d_causal(x, w, b, T, H, W, cin, cout)), what


def _subpixel_operands(sT, sH, sW, cin, cout, up_t, what, V):
    x = U((sT * sH * sW, cin), what + ".x").to(F16)
    w = U((cout, cin, 3, 3, 3), what + ".w", 1.0 / math.sqrt(27 * cin)).to(F16)
    b = U((cout,), what + ".b", 0.1).to(F16)
    return (x, b) + tuple(V.subpixel_weights(w, bool(up_t), "fast"))


def _subpixel_case(V, sT, sH, sW, cin, cout, up_t, label="SP"):
    what = f"SP {sT}x{sH}x{sW} {cin}->{cout} up_t {up_t}"
    x, b, w_sub, table, ntap = _subpixel_operands(sT, sH, sW, cin, cout, up_t, what, V)
    ncls = w_sub.shape[0]
    T2 = 2 * sT - 1 if up_t else sT
    M = T2 * 4 * sH * sW
    X = Poisoned(x, 2, 6, 40)
    Wb = Poisoned(w_sub.reshape(ncls * cout, -1), 0, 4, 0)        # rows after the last class's Cout
    bias = poisoned_vec(b)
    ops_x = {"poisoned": (X.view, Wb.view.reshape(ncls, cout, -1), bias), "dense": (x, w_sub, b)}

    def run(sel, **kw):
        xs, ws, bs = ops_x[sel]
        return V.conv3d_upsampled_subpixel(xs, ws, table, ntap, bs, sT, sH, sW, cin, cout, bool(up_t), **kw)

    ref = subpixel_ref(x, w_sub, table, ntap, b, sT, sH, sW, cin, cout, up_t)
    _conv_check(V, "SP", what, run, ref, M, cout, cout % 64 == 0, label)
    assert X.intact() and Wb.intact()


@pytest.mark.parametrize("sT,sH,sW,cin,cout,up_t", SP_CASES, ids=[f"SP-{'x'.join(map(str, c[:3]))}-{c[3]}to{c[4]}-t{c[5]}" for c in SP_CASES])
def test_subpixel_edges(V, sT, sH, sW, cin, cout, up_t):
    _subpixel_case(V, sT, sH, sW, cin, cout, up_t)


@pytest.mark.parametrize("sT,sH,sW,cin,cout,up_t", SP_PACK_CASES, ids=[f"SP-{'x'.join(map(str, c[:3]))}-{c[3]}to{c[4]}-t{c[5]}" for c in SP_PACK_CASES])
def test_subpixel_packing_guard_accepts(V, sT, sH, sW, cin, cout, up_t):
    """sT = 254: the packed frame coordinate goes up to sT (k = kt + 1 for the odd output frames), 254 + 1 < 256"""
    _subpixel_case(V, sT, sH, sW, cin, cout, up_t, label="SP.pack")


@pytest.mark.parametrize("up_t", [0, 1])
def test_subpixel_packing_guard_refuses(V, up_t):
    """sT = 255 would need the frame coordinate 256: refused as a bad argument before anything is launched, the output keeps every bit"""
    from hunyuanvideo_efficiency_amd._lib import HVKernelError
    sT, cin, cout = 255, 256, 136
    x, b, w_sub, table, ntap = _subpixel_operands(sT, 1, 1, cin, cout, up_t, f"SP refuse {up_t}", V)
    M = (2 * sT - 1 if up_t else sT) * 4
    o = Guarded(M, cout, F16, c0=8)
    with pytest.raises(HVKernelError, match="bad argument"):
        V.conv3d_upsampled_subpixel(x, w_sub, table, ntap, b, sT, 1, 1, cin, cout, bool(up_t), out=o.view)
    torch.cuda.synchronize()
    assert bool((o.buf == o.sent).all()), "a refused call wrote to its output"


# ------------------------------------------------------------------------------------------------------ production shape
def test_final_layer_full_tensor(ops):
    """FinalLayer's linear (modules/models.py): M = 118,800 tokens, N = 64, K = 3072 on gemm_kernel<BF16T,false,128>, every
    element against the fp64 bound (reference computed on the GPU in row chunks)"""
    M, N, K = 118800, 64, 3072
    a = U((M, K), "fl.a").to(BF16)
    w, b = U((N, K), "fl.w", 1.0 / math.sqrt(K)).to(BF16), U((N,), "fl.b", 0.1).to(BF16)
    got = ops.gemm(a, w, b)
    worst = 0.0
    for r0 in range(0, M, 16384):
        r1 = min(M, r0 + 16384)
        worst = max(worst, EB.check(got[r0:r1], EB.gemm_ref(a[r0:r1], w, b), BF16, f"FinalLayer rows [{r0}, {r1})"))
    _record("B1", worst)


# ------------------------------------------------------------------------------------------------------ the path table, confirmed
def test_path_table_matches_launched_kernels(ops, V):
    """one launch per row of the table under torch.profiler: the kernel the device ran is the one the mirror predicts"""
    from torch.profiler import ProfilerActivity, profile
    launches = []
    for kind, M, N, K in [("bf16", 300, 64, 64), ("bf16", 300, 264, 64), ("bf16", 300, 264, 192), ("f16", 300, 64, 64),
                          ("f16", 300, 264, 128), ("f16", 300, 264, 192), ("fp8", 300, 8, 384)]:
        opnd, _, _ = _gemm_operands(kind, M, N, K)
        opnd["asc_p"] = opnd.get("asc")
        run = _launcher(ops, V, kind, opnd)
        launches.append((gemm_path(kind, N, K), lambda run=run, o=opnd: run(o["a"], o["w"], o["b"])))
    for T, H, W, cin, cout in [(1, 3, 5, 64, 40), (1, 3, 12, 128, 128), (1, 3, 8, 128, 40), (1, 3, 8, 128, 32), (1, 3, 5, 256, 136),
                               (1, 3, 5, 64, 136)]:
        x = U((T * H * W, cin), "pt.x").to(F16)
        w = U((cout, 27 * cin), "pt.w", 0.01).to(F16)
        launches.append((conv_path(T, H, W, cin, cout),
                         lambda x=x, w=w, a=(T, H, W, cin, cout): V.conv3d_causal(x, w, None, *a)))
    # both sides of the packing guard: T = 255 on the pipelined loop, T = 256 on the 2-stage one
    for T, H, W, cin, cout, want in [(255, 1, 2, 128, 40, "C2"), (256, 1, 2, 128, 40, "C1")]:
        assert conv_path(T, H, W, cin, cout) == want
        x = U((T * H * W, cin), "pt.px").to(F16)
        w = U((cout, 27 * cin), "pt.pw", 0.01).to(F16)
        launches.append((want, lambda x=x, w=w, a=(T, H, W, cin, cout): V.conv3d_causal(x, w, None, *a)))
    # one strided launch per conv path
    strided = [((3, 6, 10), 64, 40, (2, 2, 2)), ((3, 6, 10), 128, 40, (2, 2, 2)), ((4, 3, 8), 128, 40, (2, 1, 1)), ((4, 3, 8), 128, 32, (2, 1, 1)),
               ((3, 6, 10), 256, 136, (2, 2, 2)), ((3, 6, 10), 64, 136, (2, 2, 2))]
    for src, cin, cout, stride in strided:
        x = U((src[0] * src[1] * src[2], cin), "pt.sx").to(F16)
        w = U((cout, 27 * cin), "pt.sw", 0.01).to(F16)
        launches.append((conv_path(*CB.out_grid(src, stride), cin, cout, stride, src),
                         lambda x=x, w=w, a=(*src, cin, cout, stride): V.conv3d_causal_strided(x, w, None, *a)))
    assert [p for p, _ in launches[-6:]] == ["C1", "C2", "C3", "C4", "C5", "C6"]
    xs = U((2 * 3 * 5, 256), "pt.sx").to(F16)
    w_sub, table, ntap = V.subpixel_weights(U((136, 256, 3, 3, 3), "pt.sw", 0.01).to(F16), True, "fast")
    launches.append(("SP", lambda: V.conv3d_upsampled_subpixel(xs, w_sub, table, ntap, None, 2, 3, 5, 256, 136, True)))
    assert sorted({p for p, _ in launches}) == sorted(KERNELS)
    for want, fn in launches:
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if kernel_path(e.name)]
        assert names and {kernel_path(n) for n in names} == {want}, f"{want}: launched {names}"


def test_zz_ratio_report():
    """largest error-to-bound ratio per path over this module's cases (run after them); each must use a visible share of the
    bound: below 0.05 the bound would be too loose there to catch anything"""
    lines = [f"  {p:<8} {RATIOS[p]:.3f}" for p in sorted(RATIOS)]
    print("\nlargest |got - y64| / bound per path:\n" + "\n".join(lines))
    low = {p: r for p, r in RATIOS.items() if r < 0.05}
    assert not low, f"bound too loose on {low}"
