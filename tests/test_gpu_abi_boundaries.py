"""GPU: the accepted side of the argument contract of include/hv_kernels.h (the refused side runs without a GPU:
tests/test_capi_refusals_cpu.py).  Only accepted calls are made here, through the ctypes handle with data_ptr() of real buffers.

  early-outs            the zero-row calls return 0 and leave every byte of sentinel-filled buffers intact
  single-row exemption  every entry point with the output-pitch rule: ONE row whose pitch is below its width agrees bit for bit with
                        the same call at a tight pitch, and nothing outside the row is written
  tight pitch           the smallest two-row shape with pitch == width against the project's fp64 reference / double for that
                        operation, under the bound tests/rowwise_bounds.py, error_bounds.py, conv_bounds.py and attention_bounds.py state"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from hunyuanvideo_efficiency_amd import _abi  # noqa: E402
from hunyuanvideo_efficiency_amd import synthetic as syn  # noqa: E402
from oracle import dit_ref as R  # noqa: E402
from tests import attention_bounds as AB  # noqa: E402
from tests import conv_bounds as CB  # noqa: E402
from tests import error_bounds as EB  # noqa: E402
from tests import rowwise_bounds as RB  # noqa: E402
from tests.guarded_memory import GuardedFlat, same_bits  # noqa: E402

DEV = "cuda"
BF16, F16, F32, FP8 = torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn
PARAMS = {name: params for _, name, params in _abi.DECLS}


@pytest.fixture(scope="module")
def lib():
    from hunyuanvideo_efficiency_amd import _lib
    return _lib.load()


def U(shape, key, scale=1.0):
    return syn.hashed_uniform(shape, key, 53, DEV) * (scale * math.sqrt(3.0))


def call(lib, name, **kw):
    """hv_<name> on the default stream: tensors as data_ptr(), None as NULL; returns the code after the work has finished"""
    args = []
    for ctype, p in PARAMS["hv_" + name]:
        v = None if ctype == "hipStream_t" else kw.pop(p)
        args.append(v.data_ptr() if isinstance(v, torch.Tensor) else v)
    assert not kw, kw
    rc = getattr(lib, "hv_" + name)(*args)
    torch.cuda.synchronize()
    return rc


def exact(want, what):
    def chk(y):
        assert same_bits(y, want), what
    return chk


def out_buf(rows, width, dtype):
    """a tight [rows, width] output between sentinels"""
    return GuardedFlat(rows * width, dtype)


def pitch_case(lib, name, make, out, pitch, width, dtype, under, check, row0=True):
    """make(rows) -> the other arguments for `rows` output rows.  Two rows at pitch == width are checked against the reference;
    one row at pitch `under` (< width) equals one row at the tight pitch, bit for bit, with the sentinels around it intact."""
    g = out_buf(2, width, dtype)
    assert call(lib, name, **make(2), **{out: g.view, pitch: width}) == 0, f"{name}: two rows at a tight pitch refused"
    assert g.intact(), f"{name}: a store outside the two tight rows"
    check(g.view.reshape(2, width).clone())
    t, u = out_buf(1, width, dtype), out_buf(1, width, dtype)
    assert call(lib, name, **make(1), **{out: t.view, pitch: width}) == 0
    assert call(lib, name, **make(1), **{out: u.view, pitch: under}) == 0, f"{name}: a single row with pitch {under} < {width} refused"
    assert t.intact() and u.intact(), f"{name}: a store outside the single row"
    assert same_bits(u.view, t.view), f"{name}: the single row depends on its pitch"
    if row0:        # (not for a conv: the neighbour is inside the window of voxel 0)
        assert same_bits(t.view, g.view[:width]), f"{name}: row 0 differs between the one-row and the two-row call"


# ---------------------------------------------------------------------------------------------------- early-outs
def test_zero_row_calls_return_ok_and_touch_nothing(lib):
    s16, s8, s32 = GuardedFlat(4096, BF16), GuardedFlat(4096, FP8), GuardedFlat(4096, F32)
    src = U((4096,), "early.src").to(BF16)
    src32, src8 = src.float(), src.to(FP8)
    o, o8, o32 = s16.view, s8.view, s32.view
    gemm = dict(bias=src, M=0, N=8, out0=o, ld0=8, act0=0, n_split=0, out1=None, ld1=0, act1=0, gate=None, res=None, ld_res=0)
    attn = dict(q=src, k=src, v=src, stride_q=128, stride_k=128, stride_v=128, n_q=0, n_kv=64, n_heads=1, head_dim=128, scale=0.088)
    qk = dict(q_weight=src, k_weight=src, cos_tab=src32, sin_tab=src32, n_rows=0, n_rope=0, n_heads=1, head_dim=128, ld=384, k_offset=128, eps=1e-6)
    calls = [
        ("ln_modulate_bf16", dict(x=src, shift_or_bias=src, scale_or_weight=src, out=o, M=0, D=256, ldx=256, ldo=256, eps=1e-6, mode=0)),
        ("ln_modulate_fp8", dict(x=src, shift=src, scale=src, out_q=o8, out_row_scale=o32, M=0, D=256, ldx=256, ldq=256, eps=1e-6)),
        ("quant_rows_fp8", dict(x=src, ldx=256, out_q=o8, ldq=256, out_row_scale=o32, M=0, K=256)),
        ("qknorm_rope_bf16", dict(qk, qkv=o)),
        ("qknorm_rope_scatter_bf16", dict(qk, qkv=src, dst=o, dst_ld=128, heads_per_block=1, dst_block_stride=256)),
        ("gemm_bf16", dict(gemm, A=src, lda=64, W=src, ldw=64, K=64)),
        ("gemm_fp8", dict(gemm, A_q=src8, lda=384, a_row_scale=src32, W_q=src8, ldw=384, w_scale_bf16=src, K=384)),
        ("gemm_f16", dict(A=src, lda=64, W=src, ldw=64, bias=src, M=0, N=8, K=64, out=o, ldo=8, out_is_f32=0, res=None, ld_res=0)),
        ("attn_fwd_bf16", dict(attn, o=o, stride_o=128, workspace=o32, workspace_bytes=4096 * 4)),
        ("attn_partial_bf16", dict(attn, part_o=o32, part_ml=o32, n_slots=1, slot=0, splits=1)),
        ("attn_merge_bf16", dict(part_o=src32, part_ml=src32, o=o, stride_o=128, n_q=0, n_heads=1, n_slots=1)),
        ("euler_step_f32", dict(sample=o32, model_out_bf16=src, dt=0.5, n=0)),
        ("euler_step_f32_f32", dict(sample=o32, model_out_f32=src32, dt=0.5, n=0)),
        ("broadcast_row_bf16", dict(src=src, dst=o, n_rows=0, D=256, ld=256)),
        ("copy3d_bf16", dict(src=src, dst=o, n_batch=0, rows=2, cols=8, src_batch_stride=16, src_ld=8, dst_batch_stride=16, dst_ld=8)),
        ("copy3d_bf16", dict(src=src, dst=o, n_batch=1, rows=0, cols=8, src_batch_stride=16, src_ld=8, dst_batch_stride=16, dst_ld=8)),
    ]
    for name, kw in calls:
        assert call(lib, name, **kw) == 0, name
        for g in (s16, s8, s32):
            assert bool((g.buf == g.sent).all()), f"{name}: a zero-row call wrote to a buffer"


# ---------------------------------------------------------------------------------------------------- row-wise kernels, M = 2, D = 256
D_ = 256


def test_ln_modulate_bf16_and_fp8(lib):
    x = RB.data_rows("control", 2, D_, "abi.ln").to(DEV)
    shift, scale = U((D_,), "abi.ln.shift", 0.5).to(BF16), U((D_,), "abi.ln.scale", 0.5).to(BF16)
    y64, bound = RB.ln_ref(x, shift, scale)
    kept = {}

    def make(rows):
        return dict(x=x, shift_or_bias=shift, scale_or_weight=scale, M=rows, D=D_, ldx=D_, eps=1e-6, mode=0)

    def check(y):
        RB.check(y, y64, bound, "ln_modulate_bf16 2 x 256, ldo = D")
        kept["y"] = y

    pitch_case(lib, "ln_modulate_bf16", make, "out", "ldo", D_, BF16, 8, check)
    q_ref, s_ref = R.fp8_quant_rows(kept["y"].cpu())
    for rows in (2, 1):
        sc = GuardedFlat(rows, F32)

        def make8(r, sc=sc):
            return dict(x=x, shift=shift, scale=scale, out_row_scale=sc.view, M=r, D=D_, ldx=D_, eps=1e-6)

        if rows == 2:
            q = out_buf(2, D_, FP8)
            assert call(lib, "ln_modulate_fp8", **make8(2), out_q=q.view, ldq=D_) == 0
            assert q.intact() and sc.intact()
            assert same_bits(sc.view.cpu(), s_ref.reshape(-1)) and same_bits(q.view.reshape(2, D_).cpu(), q_ref.to(FP8)), "ln_modulate_fp8, ldq = D"
        else:
            t, u = out_buf(1, D_, FP8), out_buf(1, D_, FP8)
            assert call(lib, "ln_modulate_fp8", **make8(1), out_q=t.view, ldq=D_) == 0
            assert call(lib, "ln_modulate_fp8", **make8(1), out_q=u.view, ldq=16) == 0, "ln_modulate_fp8: a single row with ldq < D refused"
            assert t.intact() and u.intact() and sc.intact() and same_bits(t.view, u.view)
            assert same_bits(t.view.cpu(), q_ref[0].to(FP8))


def test_quant_rows_fp8(lib):
    x = RB.data_rows("control", 2, D_, "abi.quant").to(DEV)
    q_ref, s_ref = R.fp8_quant_rows(x.cpu())
    sc = GuardedFlat(2, F32)

    def make(rows):
        return dict(x=x, ldx=D_, out_row_scale=sc.view, M=rows, K=D_)

    def check(q):
        assert same_bits(q.cpu(), q_ref.to(FP8)) and same_bits(sc.view.cpu(), s_ref.reshape(-1)), "quant_rows_fp8, ldq = K"

    pitch_case(lib, "quant_rows_fp8", make, "out_q", "ldq", D_, FP8, 16, check)
    assert sc.intact()


def _qk(n_rows):
    row, x, w, qw, kw = RB.qk_case("control", 1, n_rows, "abi.qk")
    cos, sin = RB.rope_tables_independent(n_rows, "abi.qk")
    tight = torch.cat([row[:, :128], row[:, 256:384]], 1).contiguous().to(DEV)      # [q | k], ld = k_offset + 128 = 256
    return x.to(DEV), w.to(DEV), qw.to(DEV), kw.to(DEV), cos.to(DEV), sin.to(DEV), tight


def _qk_check(got, x, w, cos, sin, n_rope, what):
    y64, bound, amb, amb_bound = RB.qknorm_ref(x, w, cos, sin, n_rope)
    assert bool(torch.isfinite(got.float()).all()), what
    RB.check(got.reshape(-1, 128), y64.reshape(-1, 128), bound.reshape(-1, 128), what, skip=amb.reshape(-1, 128))
    RB.check(got.reshape(-1, 128), y64.reshape(-1, 128), amb_bound.reshape(-1, 128), what + " (ambiguous)", skip=~amb.reshape(-1, 128))


def test_qknorm_rope_in_place_and_scatter(lib):
    x, w, qw, kw, cos, sin, tight = _qk(2)
    common = dict(q_weight=qw, k_weight=kw, cos_tab=cos, sin_tab=sin, n_rope=1, n_heads=1, head_dim=128, k_offset=128, eps=1e-6)
    # in place, two rows, ld == k_offset + n_heads * 128
    g = out_buf(2, 256, BF16)
    g.view.copy_(tight.reshape(-1))
    assert call(lib, "qknorm_rope_bf16", qkv=g.view, n_rows=2, ld=256, **common) == 0 and g.intact()
    y2 = g.view.reshape(2, 2, 128).clone()
    _qk_check(y2, x, w, cos, sin, 1, "qknorm_rope_bf16 2 rows, ld = 256")
    # one row: ld below the columns it rewrites
    outs = []
    for ld in (256, 128, 0):
        g1 = out_buf(1, 256, BF16)
        g1.view.copy_(tight[0])
        assert call(lib, "qknorm_rope_bf16", qkv=g1.view, n_rows=1, ld=ld, **common) == 0, f"single row with ld = {ld} refused"
        assert g1.intact()
        outs.append(g1.view.clone())
    assert same_bits(outs[0], outs[1]) and same_bits(outs[0], outs[2]) and same_bits(outs[0], y2[0].reshape(-1))
    # scatter: dst [block][row][128], dst_ld == heads_per_block * 128
    d = out_buf(4, 128, BF16)
    sc = dict(common, qkv=tight, ld=256, heads_per_block=1)
    assert call(lib, "qknorm_rope_scatter_bf16", n_rows=2, dst=d.view, dst_ld=128, dst_block_stride=256, **sc) == 0 and d.intact()
    got = d.view.reshape(2, 2, 128).transpose(0, 1)                # [row][head]
    assert same_bits(got, y2), "scatter differs from the in-place result"
    outs = []
    for dst_ld in (128, 0):
        d1 = out_buf(2, 128, BF16)
        assert call(lib, "qknorm_rope_scatter_bf16", n_rows=1, dst=d1.view, dst_ld=dst_ld, dst_block_stride=128, **sc) == 0, dst_ld
        assert d1.intact()
        outs.append(d1.view.clone())
    assert same_bits(outs[0], outs[1]) and same_bits(outs[0].reshape(2, 128), y2[0])


def test_linear_smallm(lib):
    N, K = 16, 64
    x, w, b = (t.to(DEV) for t in RB.gemv_operands(2, N, K, "abi.gemv"))
    ref = EB.gemm_ref(x, w, b)
    pitch_case(lib, "linear_smallm_bf16", lambda rows: dict(x=x, W=w, bias=b, addend=None, M=rows, N=N, K=K, ldx=K, act=0),
               "out", "ldo", N, BF16, 8, lambda y: EB.check(y, ref, BF16, "linear_smallm 2 x 16 x 64, ldo = N"))


def test_broadcast_row_and_copy3d(lib):
    src = U((2, D_), "abi.copy").to(BF16)
    pitch_case(lib, "broadcast_row_bf16", lambda rows: dict(src=src, n_rows=rows, D=D_), "dst", "ld", D_, BF16, 8,
               exact(src[0].expand(2, D_), "broadcast_row, ld = D"))
    pitch_case(lib, "copy3d_bf16", lambda rows: dict(src=src, n_batch=1, rows=rows, cols=D_, src_batch_stride=2 * D_, src_ld=D_,
                                                      dst_batch_stride=2 * D_), "dst", "dst_ld", D_, BF16, 8,
               exact(src, "copy3d, dst_ld = cols"))


# ---------------------------------------------------------------------------------------------------- GEMMs: M = 2, N = 8, K = 64 (fp8: 384)
def _epilogue(b, rows):
    return dict(bias=b, M=rows, N=8, act0=0, n_split=0, out1=None, ld1=0, act1=0, gate=None, res=None, ld_res=0)


def test_gemm_bf16_fp8_f16(lib):
    a, w, b = U((2, 64), "abi.g.a").to(BF16), U((8, 64), "abi.g.w", 0.5 / 8).to(BF16), U((8,), "abi.g.b", 0.05).to(BF16)
    ref = EB.gemm_ref(a, w, b)
    pitch_case(lib, "gemm_bf16", lambda rows: dict(_epilogue(b, rows), A=a, lda=64, W=w, ldw=64, K=64), "out0", "ld0", 8, BF16, 0,
               lambda y: EB.check(y, ref, BF16, "gemm_bf16 2 x 8 x 64, ld0 = N"))
    af, wf, bf = a.to(F16), w.to(F16), b.to(F16)
    reff = EB.gemm_ref(af, wf, bf)
    for f32 in (0, 1):
        pitch_case(lib, "gemm_f16", lambda rows: dict(A=af, lda=64, W=wf, ldw=64, bias=bf, M=rows, N=8, K=64, out_is_f32=f32, res=None, ld_res=0),
                   "out", "ldo", 8, F32 if f32 else F16, 0,
                   lambda y: EB.check(y, reff, F32 if f32 else F16, f"gemm_f16 2 x 8 x 64 out_is_f32 = {f32}, ldo = N"))
    # fp8: the operands of tests/test_gpu_gemm_conv_edges.py (per-row activation scales, one weight scale), its worst-case bound
    K = 384
    a32, w32 = U((2, K), "abi.q.a", 0.5), U((8, K), "abi.q.w", 1.0 / math.sqrt(K))
    ws = (w32.abs().max() / 448.0).to(BF16).reshape(1)
    w8 = (w32 / ws.float()).clamp(-448, 448).to(FP8)
    asc = (a32.abs().amax(1).clamp(min=1e-12) / 448.0).contiguous()
    a8 = (a32 / asc[:, None]).clamp(-448, 448).to(FP8)
    ref8 = EB.gemm_ref(a8.double() * asc.double()[:, None], w8.double() * ws.double(), b)
    pitch_case(lib, "gemm_fp8", lambda rows: dict(_epilogue(b, rows), A_q=a8, lda=K, a_row_scale=asc, W_q=w8, ldw=K, w_scale_bf16=ws, K=K),
               "out0", "ld0", 8, BF16, 0, lambda y: EB.check(y, ref8, BF16, "gemm_fp8 2 x 8 x 384, ld0 = N", worst_case=True))


def test_gemm_split_outputs_at_tight_pitches(lib):
    """columns [0, 8) to out0 and [8, 16) to out1, both rows at ld0 = ld1 = 8; one row with ld1 below the width"""
    a, w, b = U((2, 64), "abi.s.a").to(BF16), U((16, 64), "abi.s.w", 0.5 / 8).to(BF16), U((16,), "abi.s.b", 0.05).to(BF16)
    ref = EB.gemm_ref(a, w, b)
    kw = dict(A=a, lda=64, W=w, ldw=64, bias=b, N=16, K=64, act0=0, n_split=8, act1=0, gate=None, res=None, ld_res=0)
    g0, g1 = out_buf(2, 8, BF16), out_buf(2, 8, BF16)
    assert call(lib, "gemm_bf16", M=2, out0=g0.view, ld0=8, out1=g1.view, ld1=8, **kw) == 0 and g0.intact() and g1.intact()
    y = torch.cat([g0.view.reshape(2, 8), g1.view.reshape(2, 8)], 1)
    EB.check(y, ref, BF16, "gemm_bf16 split, ld0 = ld1 = 8")
    u0, u1 = out_buf(1, 8, BF16), out_buf(1, 8, BF16)
    assert call(lib, "gemm_bf16", M=1, out0=u0.view, ld0=0, out1=u1.view, ld1=0, **kw) == 0 and u0.intact() and u1.intact()
    assert same_bits(torch.cat([u0.view, u1.view]), y[0])


# ---------------------------------------------------------------------------------------------------- convs: 1 x 1 x 2, Cin 64, Cout 8
def _conv_operands(key):
    x = U((3, 64), key + ".x").to(F16)
    w = U((8, 27 * 64), key + ".w", 1.0 / math.sqrt(27 * 64)).to(F16)
    return x, w, U((8,), key + ".b", 0.1).to(F16)


def test_conv3d_causal_and_strided(lib):
    x, w, b = _conv_operands("abi.conv")
    ref = CB.conv_ref(x[:2], w, b, 1, 1, 2, 64, 8)
    pitch_case(lib, "conv3d_causal_f16",
               lambda rows: dict(x=x, ldx=64, w_taps=w, bias=b, T=1, H=1, W=rows, Cin=64, Cout=8, up_t=0, up_hw=0, res=None, ld_res=0,
                                 gn_partial=None, gn_partial_floats=0),
               "out", "ldo", 8, F16, 0, lambda y: EB.check(y, ref, F16, "conv3d_causal 1x1x2 64->8, ldo = Cout"), row0=False)
    # stride 2 along W: source widths 3 (two outputs) and 1 (one output)
    refs = CB.conv_ref(x, w, b, 1, 1, 2, 64, 8, stride=(1, 1, 2), src=(1, 1, 3))
    g = out_buf(2, 8, F16)
    kw = dict(x=x, ldx=64, w_taps=w, bias=b, sT=1, sH=1, Cin=64, Cout=8, stride_t=1, stride_h=1, stride_w=2)
    assert call(lib, "conv3d_causal_strided_f16", sW=3, out=g.view, ldo=8, **kw) == 0 and g.intact()
    EB.check(g.view.reshape(2, 8), refs, F16, "conv3d_causal_strided 1x1x3 / 2 64->8, ldo = Cout")
    t, u = out_buf(1, 8, F16), out_buf(1, 8, F16)
    assert call(lib, "conv3d_causal_strided_f16", sW=1, out=t.view, ldo=8, **kw) == 0
    assert call(lib, "conv3d_causal_strided_f16", sW=1, out=u.view, ldo=0, **kw) == 0, "a single voxel with ldo < Cout refused"
    assert t.intact() and u.intact() and same_bits(t.view, u.view)
    EB.check(t.view.reshape(1, 8), CB.conv_ref(x[:1], w, b, 1, 1, 1, 64, 8), F16, "conv3d_causal_strided single voxel")


def test_conv3d_upsampled_subpixel_at_a_tight_pitch(lib):
    """the smallest shape the entry point takes (one source voxel, Cin 256, Cout 136: four output voxels), ldo == Cout"""
    from hunyuanvideo_efficiency_amd import vae_ops as V
    from tests.test_gpu_gemm_conv_edges import subpixel_ref
    cin, cout = 256, 136
    x = U((1, cin), "abi.sp.x").to(F16)
    w5 = U((cout, cin, 3, 3, 3), "abi.sp.w", 1.0 / math.sqrt(27 * cin)).to(F16)
    b = U((cout,), "abi.sp.b", 0.1).to(F16)
    w_sub, table, ntap = V.subpixel_weights(w5, False, "fast")
    g = out_buf(4, cout, F16)
    rc = call(lib, "conv3d_upsampled_subpixel_f16", x=x, ldx=cin, w_sub=w_sub, tap_table=table, ntap=ntap, bias=b, out=g.view, ldo=cout, sT=1,
              sH=1, sW=1, Cin=cin, Cout=cout, up_t=0, gn_partial=None, gn_partial_floats=0)
    assert rc == 0 and g.intact()
    EB.check(g.view.reshape(4, cout), subpixel_ref(x, w_sub, table, ntap, b, 1, 1, 1, cin, cout, 0), F16, "subpixel 1x1x1 256->136, ldo = Cout")


# ---------------------------------------------------------------------------------------------------- attention: n_q = 2, n_kv = 64, one head
def test_attention_forward_and_merge(lib):
    q, k, v = AB.make_case("random", 2, 64, 1, "abi", DEV)
    ref = AB.AttnRef(q, k, v, 1)

    def make(rows):
        return dict(q=q, k=k, v=v, stride_q=128, stride_k=128, stride_v=128, n_q=rows, n_kv=64, n_heads=1, head_dim=128, scale=128 ** -0.5,
                    workspace=None, workspace_bytes=0)

    pitch_case(lib, "attn_fwd_bf16", make, "o", "stride_o", 128, BF16, 64, lambda y: ref.check_o(y, "attn_fwd 2 x 64, stride_o = 128"))
    parts = {}
    for rows in (2, 1):
        po, pml = GuardedFlat(rows * 128, F32), GuardedFlat(rows * 2, F32)
        kw = make(rows)
        del kw["workspace"], kw["workspace_bytes"]
        assert call(lib, "attn_partial_bf16", part_o=po.view, part_ml=pml.view, n_slots=1, slot=0, splits=1, **kw) == 0
        assert po.intact() and pml.intact()
        parts[rows] = (po.view, pml.view)
    pitch_case(lib, "attn_merge_bf16", lambda rows: dict(part_o=parts[rows][0], part_ml=parts[rows][1], n_q=rows, n_heads=1, n_slots=1),
               "o", "stride_o", 128, BF16, 64, lambda y: ref.check_o(y, "attn_merge 2 rows, stride_o = 128"))


# ---------------------------------------------------------------------------------------------------- VAE streaming kernels
def test_groupnorm_apply_softmax_transpose_resample(lib):
    C = D_
    x = U((2, C), "abi.gn.x", 2.0).to(F16)
    aff = torch.stack([1.0 + U((C,), "abi.gn.sc", 0.3), U((C,), "abi.gn.sh", 0.5)], 1).contiguous()
    for silu in (0, 1):
        y64, bound = RB.gn_apply_ref(x, aff, bool(silu))
        pitch_case(lib, "groupnorm_apply_f16", lambda rows: dict(x=x, ldx=C, M=rows, C=C, affine=aff, silu=silu), "y", "ldy", C, F16, 8,
                   lambda y: RB.check(y, y64, bound, f"groupnorm_apply 2 x 256 silu = {silu}, ldy = C"))
    # softmax: 2 rows of 60 scores padded to 64 columns
    cols, pad = 60, 64
    s = RB.softmax_scores("spread", 2, cols, "abi.sm").to(DEV)
    p64, pb = RB.softmax_ref(s, RB.valid_of(2, cols, 0).to(DEV), 0.25)

    def check_p(p):
        RB.check(p[:, :cols], p64, pb, "softmax_rows 2 x 60 (64), ld_p = cols_pad")
        assert not bool(p[:, cols:].any()), "softmax_rows: the padding columns are not zero"

    pitch_case(lib, "softmax_rows_f32_f16", lambda rows: dict(S=s, ld_s=cols, rows=rows, cols=cols, cols_pad=pad, scale=0.25, causal_block=0),
               "P", "ld_p", pad, F16, 4, check_p)
    # transpose: src [R = 40][C] -> dst [C][R]; two output rows (C = 2) at ld_dst = R, one (C = 1) at ld_dst = 1
    src = U((40, 2), "abi.tr").to(F16)
    pitch_case(lib, "transpose_16b", lambda rows: dict(src=src, ld_src=2, R=40, C=rows), "dst", "ld_dst", 40, F16, 1,
               exact(src.T, "transpose_16b, ld_dst = R"))
    # temporal average k = 2, s = 1 over T_in frames of one pixel: T_in output rows
    xt = U((2, C), "abi.tr.x").to(F16)
    y64, bound = RB.temporal_avg_ref(xt, 2, 1, 2, 1)
    pitch_case(lib, "temporal_resample_f16", lambda rows: dict(x=xt, ldx=C, T_in=rows, HW=1, C=C, mode=0, k=2, s=1), "out", "ldo", C, F16, 8,
               lambda y: RB.check(y, y64, bound, "temporal_resample 2 frames, ldo = C"))
