"""The argument contract of include/hv_kernels.h as a table: for every entry point that takes a hipStream_t one accepted baseline call,
the class of every pointer, one row per refusal the header states (or the code makes), the last accepted value of every numeric limit,
and the early-outs; for the pure host queries the shapes they answer with 0 and the size rule that ties each to its kernel.

Data and small helpers only; tests/test_capi_refusals_cpu.py drives it through ctypes on a machine WITHOUT a GPU: there a call that
passes every guard reaches the launch and returns -2 (LAUNCH), a refused one returns -1 (ARG) before any launch, an early-out 0.
"Device" pointers are made-up aligned integers - the host half of an entry point never dereferences them; the host arrays of
hv_vae_blend_f16 / hv_copy4d_16b (strides, dims) are real ctypes arrays.

A row is (rule, overrides): exactly the named arguments differ from the baseline, so the answer is attributable to the rule.  A value
may be a callable taking the ctypes library (a size that only the library's own query knows)."""
import ctypes as C
import itertools

from hunyuanvideo_efficiency_amd import _abi

OK, ARG, LAUNCH = 0, -1, -2
PTR = 0x7F0000001000            # 4 KiB aligned
I31 = 0x7FFFFFFF
I63 = (1 << 63) - 1
M = _abi.MACROS


def i64s(*v):
    return (C.c_int64 * len(v))(*v)


def i32s(*v):
    return (C.c_int * len(v))(*v)


class Entry:
    def __init__(self, base, required=(), nullable=()):
        self.base, self.required, self.nullable = dict(base), tuple(required), tuple(nullable)
        self.refuse, self.accept, self.early = [], [], []
        self.limits = []        # (rule, macro names, accepted overrides, refused overrides or None)

    def no(self, rule, **ov):
        self.refuse.append((rule, ov))
        return self

    def yes(self, rule, **ov):
        self.accept.append((rule, ov))
        return self

    def out(self, rule, **ov):
        self.early.append((rule, ov))
        return self

    def limit(self, rule, last_ok, first_bad=None, macros=()):
        self.limits.append((rule, tuple(macros), last_ok, first_bad))
        return self


E = {}

# ------------------------------------------------------------------------------------------------ row-wise kernels (hv_rowwise.hip)
E["hv_ln_modulate_bf16"] = (
    Entry(dict(x=PTR, shift_or_bias=PTR, scale_or_weight=PTR, out=PTR, M=2, D=16, ldx=64, ldo=64, eps=1e-6, mode=0),
          required=("x", "out"), nullable=("shift_or_bias", "scale_or_weight"))
    .no("D % 8 == 0", D=12).no("D > 0", D=0).no("M >= 0", M=-1).no("ldx % 8 == 0", ldx=68).no("ldo % 8 == 0", ldo=68)
    .no("mode 0 | 1", mode=2).no("mode 0 | 1", mode=-1)
    .no("output pitch: ldo >= D when M > 1", ldo=8).yes("tight pitch ldo == D", ldo=16).yes("single row exempt from the pitch rule", M=1, ldo=8)
    .yes("input pitch is free (overlapping reads)", ldx=0)
    .limit("D <= 4096", dict(D=4096, ldx=4096, ldo=4096), dict(D=4104, ldx=4104, ldo=4104))
    .limit("(M + 3) / 4 workgroups fit grid.x", dict(M=4 * I31), dict(M=4 * I31 + 1))
    .out("M == 0", M=0))

_QK = dict(qkv=PTR, q_weight=PTR, k_weight=PTR, cos_tab=PTR, sin_tab=PTR, n_rows=2, n_rope=1, n_heads=1, head_dim=128, ld=384,
           k_offset=128, eps=1e-6)
E["hv_qknorm_rope_bf16"] = (
    Entry(_QK, required=("qkv", "q_weight", "k_weight", "cos_tab", "sin_tab"))
    .yes("cos / sin tables may be NULL when n_rope == 0", n_rope=0, cos_tab=None, sin_tab=None)
    .no("head_dim == 128", head_dim=64).no("n_heads > 0", n_heads=0).no("n_rows >= 0", n_rows=-1).no("n_rope >= 0", n_rope=-1)
    .no("n_rope <= n_rows", n_rope=3).no("ld % 8 == 0", ld=388).no("k_offset % 8 == 0", k_offset=132)
    .no("q and k heads on different columns: k_offset >= n_heads * 128", k_offset=0)
    .no("q and k heads on different columns: k_offset >= n_heads * 128", k_offset=120)
    .no("output pitch: ld >= k_offset + n_heads * 128 when n_rows > 1", ld=128)
    .yes("tight pitch ld == k_offset + n_heads * 128", ld=256).yes("single row exempt from the pitch rule", n_rows=1, ld=128)
    .limit("n_rows workgroups fit grid.x", dict(n_rows=I31), dict(n_rows=I31 + 1))
    .out("n_rows == 0", n_rows=0, n_rope=0))
E["hv_qknorm_rope_scatter_bf16"] = (
    Entry(dict(_QK, dst=PTR, dst_ld=128, heads_per_block=1, dst_block_stride=256),
          required=("qkv", "q_weight", "k_weight", "cos_tab", "sin_tab", "dst"))
    .yes("cos / sin tables may be NULL when n_rope == 0", n_rope=0, cos_tab=None, sin_tab=None)
    .no("head_dim == 128", head_dim=64).no("n_heads > 0", n_heads=0).no("n_rows >= 0", n_rows=-1).no("n_rope >= 0", n_rope=-1)
    .no("n_rope <= n_rows", n_rope=3).no("ld % 8 == 0", ld=388).no("k_offset % 8 == 0", k_offset=132)
    .no("dst_ld % 8 == 0", dst_ld=132).no("dst_block_stride % 8 == 0", dst_block_stride=260).no("heads_per_block > 0", heads_per_block=0)
    .no("output pitch: dst_ld >= heads_per_block * 128 when n_rows > 1", dst_ld=0)
    .yes("single row exempt from the pitch rule", n_rows=1, dst_ld=0)
    .yes("the source row is only read: k_offset and ld are free", k_offset=0, ld=128)
    .limit("n_rows workgroups fit grid.x", dict(n_rows=I31), dict(n_rows=I31 + 1))
    .out("n_rows == 0", n_rows=0, n_rope=0))

E["hv_linear_smallm_bf16"] = (
    Entry(dict(x=PTR, W=PTR, bias=PTR, addend=PTR, out=PTR, M=2, N=8, K=8, ldx=8, ldo=8, act=0),
          required=("x", "W", "out"), nullable=("bias", "addend"))
    .no("M >= 1", M=0).no("N >= 1", N=0).no("K >= 8", K=0).no("K % 8 == 0", K=12).no("ldx % 8 == 0", ldx=12)
    .no("act bits 0 | 1 only", act=4).no("act bits 0 | 1 only", act=-1).yes("act = both bits", act=3)
    .no("output pitch: ldo >= N when M > 1", ldo=0).yes("single row exempt from the pitch rule", M=1, ldo=0)
    .limit("M <= 4", dict(M=4), dict(M=5)))

E["hv_timestep_embedding_bf16"] = (
    Entry(dict(t=PTR, out=PTR, n_t=1, dim=2, max_period=10000.0), required=("t", "out"))
    .no("n_t > 0", n_t=0).no("dim > 0", dim=0).no("dim even", dim=3)
    .no("n_t * dim fits an int", n_t=1 << 20, dim=1 << 12)
    .limit("n_t * dim <= 2^31 - 1", dict(n_t=0x3FFFFFFF), dict(n_t=0x40000000)))

_TOK = 256 * I31                # elements of the widest one-thread-per-(token, channel) grid
E["hv_patchify_f32_bf16"] = (
    Entry(dict(x=PTR, A=PTR, C=1, T=1, H=2, W=2), required=("x", "A"))
    .no("C > 0", C=0).no("T > 0", T=0).no("H > 0", H=0).no("W > 0", W=0).no("H > 0", H=-2).no("H even", H=3).no("W even", W=3)
    .limit("T * H/2 * W/2 * C threads fit grid.x", dict(T=I31, W=512), dict(T=I31, W=514)))
E["hv_unpatchify_bf16"] = (
    Entry(dict(y=PTR, out=PTR, C=1, T=1, H=2, W=2, ldy=4), required=("y", "out"))
    .no("C > 0", C=0).no("T > 0", T=0).no("H > 0", H=0).no("H > 0", H=-2).no("W > 0", W=0).no("W > 0", W=-2).no("H even", H=3)
    .no("W even", W=3).no("ldy % 4 == 0", ldy=6).yes("input pitch is free", ldy=0)
    .limit("T * H/2 * W/2 * C threads fit grid.x", dict(T=I31, W=512), dict(T=I31, W=514)))

for _n, _v in (("hv_euler_step_f32", "model_out_bf16"), ("hv_euler_step_f32_f32", "model_out_f32")):
    E[_n] = (Entry({"sample": PTR, _v: PTR, "dt": 0.5, "n": 1}, required=("sample", _v))
             .no("n >= 0", n=-1).out("n == 0", n=0)
             .limit("n / 4 threads fit grid.x", dict(n=(1 << 41) - 1025), dict(n=(1 << 41) - 1024)))

E["hv_masked_mean_bf16"] = (Entry(dict(x=PTR, mask=PTR, out=PTR, L=1, D=1), required=("x", "out"), nullable=("mask",))
                            .no("L > 0", L=0).no("D > 0", D=0))

E["hv_broadcast_row_bf16"] = (
    Entry(dict(src=PTR, dst=PTR, n_rows=2, D=8, ld=8), required=("src", "dst"))
    .no("n_rows >= 0", n_rows=-1).no("D > 0", D=0).no("output pitch: ld >= D when n_rows > 1", ld=0)
    .yes("single row exempt from the pitch rule", n_rows=1, ld=0)
    .limit("n_rows * D threads fit grid.x", dict(n_rows=I31, D=256, ld=256), dict(n_rows=I31 + 1, D=256, ld=256))
    .out("n_rows == 0", n_rows=0))

E["hv_copy3d_bf16"] = (
    Entry(dict(src=PTR, dst=PTR, n_batch=1, rows=2, cols=8, src_batch_stride=16, src_ld=8, dst_batch_stride=16, dst_ld=8),
          required=("src", "dst"))
    .no("n_batch >= 0", n_batch=-1).no("rows >= 0", rows=-1).no("cols > 0", cols=0).no("cols % 8 == 0", cols=12)
    .no("src_ld % 8 == 0", src_ld=12).no("dst_ld % 8 == 0", dst_ld=12).no("src_batch_stride % 8 == 0", src_batch_stride=12)
    .no("dst_batch_stride % 8 == 0", dst_batch_stride=12)
    .no("output pitch: dst_ld >= cols when rows > 1", dst_ld=0).yes("single row exempt from the pitch rule", rows=1, dst_ld=0)
    .yes("input pitch is free", src_ld=0)
    .yes("a batch stride below a row is the unpack layout out[r][p * w + c]", n_batch=2, dst_batch_stride=8, dst_ld=16)
    .limit("rows <= 2^31 - 1", dict(rows=I31), dict(rows=I31 + 1))
    .limit("n_batch <= 65535 (grid.z)", dict(n_batch=65535), dict(n_batch=65536))
    .out("n_batch == 0", n_batch=0).out("rows == 0", rows=0))

E["hv_fp8_dequant_bf16"] = (Entry(dict(w_e4m3fn=PTR, scale_bf16=PTR, out_bf16=PTR, n=8), required=("w_e4m3fn", "scale_bf16", "out_bf16"))
                            .no("n > 0", n=0).no("n > 0", n=-8).no("n % 8 == 0", n=12))

E["hv_ln_modulate_fp8"] = (
    Entry(dict(x=PTR, shift=PTR, scale=PTR, out_q=PTR, out_row_scale=PTR, M=2, D=16, ldx=64, ldq=64, eps=1e-6),
          required=("x", "out_q", "out_row_scale"), nullable=("shift", "scale"))
    .no("D % 8 == 0", D=12).no("D > 0", D=0).no("M >= 0", M=-1).no("ldx % 8 == 0", ldx=68).no("ldq % 16 == 0", ldq=72)
    .no("output pitch: ldq >= D when M > 1", ldq=0).yes("tight pitch ldq == D", ldq=16).yes("single row exempt from the pitch rule", M=1, ldq=0)
    .limit("D <= 4096", dict(D=4096, ldx=4096, ldq=4096), dict(D=4104, ldx=4104, ldq=4112))
    .limit("(M + 3) / 4 workgroups fit grid.x", dict(M=4 * I31), dict(M=4 * I31 + 1))
    .out("M == 0", M=0))

E["hv_quant_rows_fp8"] = (
    Entry(dict(x=PTR, ldx=16, out_q=PTR, ldq=16, out_row_scale=PTR, M=2, K=16), required=("x", "out_q", "out_row_scale"))
    .no("K > 0", K=0).no("K % 8 == 0", K=12).no("M >= 0", M=-1).no("ldx % 8 == 0", ldx=20).no("ldq % 16 == 0", ldq=24)
    .no("output pitch: ldq >= K when M > 1", ldq=0).yes("single row exempt from the pitch rule", M=1, ldq=0).yes("input pitch is free", ldx=0)
    .limit("(M + 3) / 4 workgroups fit grid.x", dict(M=4 * I31), dict(M=4 * I31 + 1))
    .out("M == 0", M=0))

# ------------------------------------------------------------------------------------------------ GEMMs and convs (hv_gemm.hip)
_EPI = dict(out0=PTR, ld0=16, act0=0, n_split=0, out1=PTR, ld1=16, act1=0, gate=None, res=PTR, ld_res=16)


def _gemm_rows(e, k0):
    """the rules hv_gemm_bf16 and hv_gemm_fp8 share (fill_common and the epilogue operands); k0 = the baseline's K"""
    return (e.no("N > 0", N=0).no("N % 8 == 0", N=12).no("M >= 0", M=-1).no("ld0 % 8 == 0", ld0=20)
            .no("act0 in 0..2", act0=3).no("act0 in 0..2", act0=-1).no("act1 in 0..2", act1=3).no("act1 in 0..2", act1=-1)
            .no("a split needs out1", n_split=8, out1=None).no("n_split % 8 == 0", n_split=4).no("ld1 % 8 == 0 with a split", n_split=8, ld1=12)
            .no("gate needs res", gate=PTR, res=None).no("ld_res % 8 == 0", ld_res=20)
            .yes("gate with res", gate=PTR).yes("split at column 8", n_split=8).yes("n_split >= N: no split, out1 unused", n_split=16, out1=None)
            .no("output pitch: ld0 >= columns of out0 when M > 1", ld0=8)
            .no("output pitch: ld1 >= N - n_split when M > 1", n_split=8, ld1=0)
            .yes("tight pitches of a split: ld0 == n_split, ld1 == N - n_split", n_split=8, ld0=8, ld1=8)
            .yes("single row exempt from the pitch rule", M=1, ld0=8).yes("single row exempt from the pitch rule", M=1, n_split=8, ld1=0)
            .yes("ld_res is an input pitch", ld_res=0)
            .limit("tiles_m * tiles_n workgroups fit grid.x", dict(M=I31, N=65280, ld0=65280), dict(M=I31, N=65536, ld0=65536))
            .out("M == 0", M=0))


E["hv_gemm_bf16"] = _gemm_rows(
    Entry(dict(A=PTR, lda=64, W=PTR, ldw=64, bias=PTR, M=2, N=16, K=64, **_EPI),
          required=("A", "W", "out0"), nullable=("bias", "out1", "gate", "res"))
    .no("K >= 64", K=0).no("K % 64 == 0", K=96).no("lda % 8 == 0", lda=68).no("ldw % 8 == 0", ldw=68), 64)
E["hv_gemm_fp8"] = _gemm_rows(
    Entry(dict(A_q=PTR, lda=384, a_row_scale=PTR, W_q=PTR, ldw=384, w_scale_bf16=PTR, bias=PTR, M=2, N=16, K=384, **_EPI),
          required=("A_q", "a_row_scale", "W_q", "w_scale_bf16", "out0"), nullable=("bias", "out1", "gate", "res"))
    .no("K % 128 == 0", K=448).no("lda % 16 == 0", lda=392).no("ldw % 16 == 0", ldw=392)
    .limit("K >= 384", dict(K=384), dict(K=256)), 384)

E["hv_gemm_f16"] = (
    Entry(dict(A=PTR, lda=64, W=PTR, ldw=64, bias=PTR, M=2, N=16, K=64, out=PTR, ldo=16, out_is_f32=0, res=PTR, ld_res=16),
          required=("A", "W", "out"), nullable=("bias", "res"))
    .no("K >= 64", K=0).no("K % 64 == 0", K=96).no("N % 8 == 0", N=12).no("N > 0", N=0).no("M >= 0", M=-1).no("lda % 8 == 0", lda=68)
    .no("ldw % 8 == 0", ldw=68).no("ldo % 8 == 0", ldo=20).no("ld_res % 8 == 0", ld_res=20)
    .no("out_is_f32 0 | 1", out_is_f32=2, res=None).no("out_is_f32 0 | 1", out_is_f32=-1, res=None)
    .no("no residual with an fp32 result", out_is_f32=1)
    .yes("fp32 result", out_is_f32=1, res=None)
    .no("output pitch: ldo >= N when M > 1", ldo=8).no("output pitch: ldo >= N when M > 1 (fp32 result)", out_is_f32=1, res=None, ldo=8)
    .yes("single row exempt from the pitch rule", M=1, ldo=8)
    .limit("tiles_m * tiles_n workgroups fit grid.x", dict(M=I31, N=65280, ldo=65280), dict(M=I31, N=65536, ldo=65536))
    .out("M == 0", M=0))


def _rows_floats(query, qargs, cout):
    return lambda lib: getattr(lib, query)(*qargs) * cout * 2


E["hv_conv3d_causal_f16"] = (
    Entry(dict(x=PTR, ldx=64, w_taps=PTR, bias=PTR, out=PTR, ldo=8, T=1, H=1, W=2, Cin=64, Cout=8, up_t=0, up_hw=0, res=PTR, ld_res=8,
               gn_partial=PTR, gn_partial_floats=_rows_floats("hv_gn_partial_rows", (2,), 8)),
          required=("x", "w_taps", "out"), nullable=("bias", "res", "gn_partial"))
    .no("T > 0", T=0).no("H > 0", H=0).no("W > 0", W=0).no("Cin >= 64", Cin=32).no("Cin % 64 == 0", Cin=96).no("Cout > 0", Cout=0)
    .no("Cout % 8 == 0", Cout=12, ldo=16, ld_res=16, gn_partial=None).no("up_t 0 | 1", up_t=2).no("up_hw 0 | 1", up_hw=2)
    .no("up_t needs an odd T", up_t=1, T=2).yes("up_t with T = 3", up_t=1, T=3)
    .no("up_hw needs even H, W", up_hw=1).yes("up_hw with H = W = 2", up_hw=1, H=2)
    .no("ldx % 8 == 0", ldx=68).no("ldo % 8 == 0", ldo=12).no("ld_res % 8 == 0", ld_res=12)
    .no("output pitch: ldo >= Cout when more than one voxel", ldo=0).yes("single voxel exempt from the pitch rule", W=1, ldo=0)
    .limit("gn_partial_floats >= hv_gn_partial_rows(T*H*W) * Cout * 2", dict(), dict(gn_partial_floats=63))
    .limit("source below 4 GiB: sT*sH*sW*ldx*2 < 2^32", dict(ldx=(1 << 30) - 8), dict(ldx=1 << 30))
    .limit("T*H*W <= 2^31 - 1", dict(ldx=0, H=32768, W=65535, gn_partial=None), dict(ldx=0, H=32768, W=65536, gn_partial=None)))

_SP_FLOATS = _rows_floats("hv_subpixel_gn_partial_rows", (1, 1, 1, 0), 136)
E["hv_conv3d_upsampled_subpixel_f16"] = (
    Entry(dict(x=PTR, ldx=256, w_sub=PTR, tap_table=PTR, ntap=12, bias=PTR, out=PTR, ldo=136, sT=1, sH=1, sW=1, Cin=256, Cout=136, up_t=0,
               gn_partial=PTR, gn_partial_floats=_SP_FLOATS),
          required=("x", "w_sub", "tap_table", "out"), nullable=("bias", "gn_partial"))
    .no("sT > 0", sT=0).no("sH > 0", sH=0).no("sW > 0", sW=0).no("ntap >= 1", ntap=0).no("up_t 0 | 1", up_t=2)
    .yes("up_t = 1 with a single source frame (the odd-frame classes are empty)", up_t=1)
    .no("Cin a power of two", Cin=384, ldx=384).no("Cout % 8 == 0", Cout=140, ldo=144, gn_partial=None).no("ldx % 8 == 0", ldx=260)
    .no("ldo % 8 == 0", ldo=140).no("output pitch: ldo >= Cout", ldo=128)
    .limit("ntap <= 27", dict(ntap=27), dict(ntap=28))
    .limit("Cin >= 256", dict(Cin=256), dict(Cin=128))
    .limit("Cout > 128", dict(Cout=136), dict(Cout=128))
    .limit("sT + 1 < 256 (packed frame coordinate)", dict(sT=254), dict(sT=255))
    .limit("sH <= 4096 (packed coordinate)", dict(sH=4096, gn_partial=None), dict(sH=4097, gn_partial=None))
    .limit("sW <= 4096 (packed coordinate)", dict(sW=4096, gn_partial=None), dict(sW=4097, gn_partial=None))
    .limit("gn_partial_floats >= hv_subpixel_gn_partial_rows(...) * Cout * 2", dict(), dict(gn_partial_floats=lambda lib: _SP_FLOATS(lib) - 1))
    .limit("source below 4 GiB: sT*sH*sW*ldx*2 < 2^32", dict(ldx=(1 << 31) - 8), dict(ldx=1 << 31)))

E["hv_conv3d_cout4_f16"] = (
    Entry(dict(x=PTR, ldx=32, affine=PTR, silu=0, w_frag=PTR, bias=PTR, out=PTR, ldo=8, T=1, H=1, W=2, Cin=32, Cout=3, planes=PTR,
               planes_floats=lambda lib: lib.hv_conv3d_cout4_planes_floats(2)),
          required=("x", "w_frag", "bias", "out", "planes"), nullable=("affine",))
    .no("silu 0 | 1", silu=2).no("silu 0 | 1", silu=-1).yes("silu = 1", silu=1)
    .no("T > 0", T=0).no("H > 0", H=0).no("W > 0", W=0).no("Cin > 0", Cin=0).no("Cin % 32 == 0", Cin=48, ldx=48).no("Cout > 0", Cout=0)
    .no("ldx >= Cin", ldx=24).no("ldx % 8 == 0", ldx=36).no("ldo >= Cout", ldo=2).no("ldo % 8 == 0 from 8 on", ldo=12)
    .yes("ldo below 8: Cout columns alone are written", ldo=3)
    .no("x 16-byte aligned", x=PTR + 8).no("out 16-byte aligned", out=PTR + 8).no("w_frag 16-byte aligned", w_frag=PTR + 8)
    .limit("Cin <= 128", dict(Cin=128, ldx=128), dict(Cin=160, ldx=160))
    .limit("Cout <= 3", dict(Cout=3), dict(Cout=4))
    .limit("planes_floats >= hv_conv3d_cout4_planes_floats(T*H*W)", dict(), dict(planes_floats=161))
    .limit("T*H*W / 256 workgroups fit grid.x", dict(T=I31, H=256, W=1, planes_floats=I63), dict(T=I31, H=257, W=1, planes_floats=I63)))

E["hv_conv3d_causal_strided_f16"] = (
    Entry(dict(x=PTR, ldx=64, w_taps=PTR, bias=PTR, out=PTR, ldo=8, sT=1, sH=1, sW=3, Cin=64, Cout=8, stride_t=1, stride_h=1, stride_w=2),
          required=("x", "w_taps", "out"), nullable=("bias",))
    .no("sT > 0", sT=0).no("sH > 0", sH=0).no("sW > 0", sW=0).no("Cin >= 64", Cin=32).no("Cin % 64 == 0", Cin=96).no("Cout > 0", Cout=0)
    .no("Cout % 8 == 0", Cout=12, ldo=16).no("stride_t 1 | 2", stride_t=0).no("stride_t 1 | 2", stride_t=3).no("stride_h 1 | 2", stride_h=0)
    .no("stride_h 1 | 2", stride_h=3).no("stride_w 1 | 2", stride_w=0).no("stride_w 1 | 2", stride_w=3)
    .no("ldx % 8 == 0", ldx=68).no("ldo % 8 == 0", ldo=12)
    .no("output pitch: ldo >= Cout when more than one voxel", ldo=0).yes("single voxel exempt from the pitch rule", sW=1, ldo=0)
    .limit("source below 4 GiB: sT*sH*sW*ldx*2 < 2^32", dict(ldx=715827880), dict(ldx=715827888))
    .limit("sT*sH*sW <= 2^31 - 1", dict(ldx=0, sH=32768, sW=65535), dict(ldx=0, sH=32768, sW=65536)))

# ------------------------------------------------------------------------------------------------ attention (hv_attention.hip)
_ATT = dict(q=PTR, k=PTR, v=PTR, stride_q=128, stride_k=128, stride_v=128, n_q=2, n_kv=64, n_heads=1, head_dim=128, scale=0.088)
_KV_MAX = I31 - 2048
E["hv_attn_fwd_bf16"] = (
    Entry(dict(_ATT, o=PTR, stride_o=128, workspace=None, workspace_bytes=0), required=("q", "k", "v", "o"), nullable=("workspace",))
    .no("head_dim == 128", head_dim=64).no("n_heads > 0", n_heads=0).no("n_q >= 0", n_q=-1).no("n_kv >= 0", n_kv=-1)
    .no("n_kv > 0 when there are queries", n_kv=0)
    .no("stride_q % 8 == 0", stride_q=132).no("stride_k % 8 == 0", stride_k=132).no("stride_v % 8 == 0", stride_v=132)
    .no("stride_o % 4 == 0", stride_o=130)
    .no("output pitch: stride_o >= n_heads * 128 when n_q > 1", stride_o=64).yes("single row exempt from the pitch rule", n_q=1, stride_o=64)
    .yes("input pitches are free", stride_q=0, stride_k=0, stride_v=0)
    .limit("the key-norm bound serves up to 62 heads from HV_ATTN_BOUND_MIN_KV keys with HV_ATTN_MIN_WORKSPACE_BYTES; beyond, the call "
           "runs without it (no refusal)", dict(n_heads=62, stride_o=62 * 128, n_kv=M["HV_ATTN_BOUND_MIN_KV"], workspace=PTR,
                                                workspace_bytes=M["HV_ATTN_MIN_WORKSPACE_BYTES"]), None,
           macros=("HV_ATTN_BOUND_MIN_KV", "HV_ATTN_MIN_WORKSPACE_BYTES"))
    .yes("63 heads with the bound workspace: the bound is skipped", n_heads=63, stride_o=63 * 128, n_kv=4096, workspace=PTR, workspace_bytes=256)
    .yes("a workspace below HV_ATTN_MIN_WORKSPACE_BYTES is ignored", n_kv=4096, workspace=PTR, workspace_bytes=255)
    .limit("n_kv <= 2^31 - 2049", dict(n_kv=_KV_MAX), dict(n_kv=_KV_MAX + 1))
    .limit("n_q / 256 * n_heads workgroups fit grid.x", dict(n_q=I31, n_heads=255, stride_o=256 * 128), dict(n_q=I31, n_heads=256, stride_o=256 * 128))
    .out("n_q == 0", n_q=0).out("n_q == 0 (also without keys)", n_q=0, n_kv=0))
E["hv_attn_partial_bf16"] = (
    Entry(dict(_ATT, part_o=PTR, part_ml=PTR, n_slots=1, slot=0, splits=1), required=("q", "k", "v", "part_o", "part_ml"))
    .no("head_dim == 128", head_dim=64).no("n_heads > 0", n_heads=0).no("n_q >= 0", n_q=-1).no("n_kv > 0", n_kv=0).no("n_kv > 0", n_kv=-1)
    .no("stride_q % 8 == 0", stride_q=132).no("stride_k % 8 == 0", stride_k=132).no("stride_v % 8 == 0", stride_v=132)
    .no("splits 1 | 2", splits=0).no("splits 1 | 2", splits=3).no("slot >= 0", slot=-1).no("slot + splits <= n_slots", slot=1)
    .no("slot + splits <= n_slots", splits=2, n_kv=128)
    .limit("splits = 2 needs two key tiles", dict(splits=2, n_slots=2, n_kv=65), dict(splits=2, n_slots=2, n_kv=64))
    .limit("n_kv <= 2^31 - 2049", dict(n_kv=_KV_MAX), dict(n_kv=_KV_MAX + 1))
    .limit("n_q / 256 * n_heads workgroups fit grid.x", dict(n_q=I31, n_heads=255), dict(n_q=I31, n_heads=256))
    .out("n_q == 0", n_q=0))
E["hv_attn_merge_bf16"] = (
    Entry(dict(part_o=PTR, part_ml=PTR, o=PTR, stride_o=128, n_q=2, n_heads=1, n_slots=1), required=("part_o", "part_ml", "o"))
    .no("n_heads > 0", n_heads=0).no("n_q >= 0", n_q=-1).no("n_slots > 0", n_slots=0).no("stride_o % 4 == 0", stride_o=130)
    .no("output pitch: stride_o >= n_heads * 128 when n_q > 1", stride_o=64).yes("single row exempt from the pitch rule", n_q=1, stride_o=64)
    .limit("n_q * n_heads * 32 threads fit grid.x", dict(n_q=I31, n_heads=8, stride_o=9 * 128), dict(n_q=I31, n_heads=9, stride_o=9 * 128))
    .out("n_q == 0", n_q=0))

# ------------------------------------------------------------------------------------------------ VAE streaming kernels (hv_vae.hip)
E["hv_temporal_resample_f16"] = (
    Entry(dict(x=PTR, ldx=8, out=PTR, ldo=8, T_in=2, HW=1, C=8, mode=0, k=1, s=1), required=("x", "out"))
    .no("T_in > 0", T_in=0).no("HW > 0", HW=0).no("C > 0", C=0).no("C % 8 == 0", C=12).no("ldx % 8 == 0", ldx=12).no("ldo % 8 == 0", ldo=12)
    .no("s >= 1", s=0).no("mode 0 | 1", mode=2).no("mode 0 | 1", mode=-1).no("k >= 1 in mode 0", k=0).yes("k unused in mode 1", mode=1, k=0)
    .no("output pitch: ldo >= C when more than one row", ldo=0).yes("single row exempt from the pitch rule", T_in=1, ldo=0)
    .yes("input pitch is free", ldx=0)
    .limit("T_in * s fits an int (mode 1)", dict(mode=1, T_in=1 << 16, s=(1 << 15) - 1), dict(mode=1, T_in=1 << 16, s=1 << 15))
    .limit("T_out * HW * C/8 fits an int64", dict(HW=(1 << 62) - 1), dict(HW=1 << 62)))

_GN = dict(C=8, groups=1, eps=1e-6, weight=PTR, bias=PTR, affine_out=PTR)
E["hv_groupnorm_affine_f16"] = (
    Entry(dict(_GN, x=PTR, ldx=8, M=1, partial_ws=PTR, partial_ws_floats=16), required=("x", "weight", "bias", "partial_ws", "affine_out"))
    .no("M > 0", M=0).no("C >= 8", C=0).no("C % 8 == 0", C=12).no("groups > 0", groups=0).no("groups a power of two dividing C", groups=3, C=24)
    .no("C % groups == 0", groups=16).no("ldx % 8 == 0", ldx=12).no("C / 8 divides 256", C=24, partial_ws_floats=48)
    .limit("C <= 2048", dict(C=2048, ldx=2048, partial_ws_floats=4096), dict(C=2056, ldx=2056, partial_ws_floats=4112))
    .limit("groups <= 64", dict(C=1024, groups=64, ldx=1024, partial_ws_floats=2048), dict(C=1024, groups=128, ldx=1024, partial_ws_floats=2048))
    .limit("partial_ws_floats >= 2 * C", dict(), dict(partial_ws_floats=15)))
_FOLD = M["HV_GN_FOLD_WS_FLOATS"]
E["hv_groupnorm_finalize_f16"] = (
    Entry(dict(_GN, partial=PTR, partial_floats=16 + _FOLD, nrow=1, M=1), required=("partial", "weight", "bias", "affine_out"))
    .no("nrow > 0", nrow=0).no("M > 0", M=0).no("C >= 8", C=0).no("C % 8 == 0", C=12, partial_floats=24 + _FOLD).no("groups > 0", groups=0)
    .no("groups a power of two", groups=3, C=24, partial_floats=48 + _FOLD).no("C % groups == 0", groups=16)
    .no("C / groups even (whole column pairs)", groups=8)
    .limit("C <= 2048", dict(C=2048, partial_floats=4096 + _FOLD), dict(C=2056, partial_floats=4112 + _FOLD))
    .limit("groups <= 64", dict(C=1024, groups=64, partial_floats=2048 + _FOLD), dict(C=1024, groups=128, partial_floats=2048 + _FOLD))
    .limit("partial_floats >= align2(nrow*C*2) + HV_GN_FOLD_WS_FLOATS", dict(), dict(partial_floats=15 + _FOLD), macros=("HV_GN_FOLD_WS_FLOATS",))
    .limit("a buffer sized for the conv alone is refused", dict(), dict(partial_floats=16)))
E["hv_groupnorm_apply_f16"] = (
    Entry(dict(x=PTR, ldx=8, y=PTR, ldy=8, M=2, C=8, affine=PTR, silu=0), required=("x", "y", "affine"))
    .no("M > 0", M=0).no("C >= 8", C=0).no("C % 8 == 0", C=12, ldx=16, ldy=16).no("ldx % 8 == 0", ldx=12).no("ldy % 8 == 0", ldy=12)
    .no("silu 0 | 1", silu=2).no("silu 0 | 1", silu=-1).yes("silu = 1", silu=1)
    .no("output pitch: ldy >= C when M > 1", ldy=0).yes("single row exempt from the pitch rule", M=1, ldy=0).yes("input pitch is free", ldx=0)
    .limit("C <= 2048", dict(C=2048, ldx=2048, ldy=2048), dict(C=2056, ldx=2056, ldy=2056))
    .limit("row blocks fit grid.x", dict(C=2048, ldx=2048, ldy=2048, M=4 * I31), dict(C=2048, ldx=2048, ldy=2048, M=4 * I31 + 1)))

E["hv_softmax_rows_f32_f16"] = (
    Entry(dict(S=PTR, ld_s=1, P=PTR, ld_p=1, rows=2, cols=1, cols_pad=1, scale=1.0, causal_block=0), required=("S", "P"))
    .no("rows > 0", rows=0).no("cols > 0", cols=0).no("cols_pad >= cols", cols_pad=0).no("causal_block >= 0", causal_block=-1)
    .no("output pitch: ld_p >= cols_pad when rows > 1", ld_p=0).yes("single row exempt from the pitch rule", rows=1, ld_p=0)
    .no("output pitch covers the zero-filled padding", cols_pad=4, ld_p=2).yes("input pitch is free", ld_s=0))

E["hv_transpose_16b"] = (
    Entry(dict(src=PTR, ld_src=2, dst=PTR, ld_dst=1, R=1, C=2), required=("src", "dst"))
    .no("R > 0", R=0).no("C > 0", C=0).no("output pitch: ld_dst >= R when C > 1", ld_dst=0)
    .yes("single output row exempt from the pitch rule", C=1, ld_dst=0).yes("input pitch is free", ld_src=0)
    .limit("R / 32 tile rows fit grid.y", dict(R=65535 * 32, ld_dst=65535 * 32), dict(R=65535 * 32 + 1, ld_dst=65535 * 32 + 1)))

E["hv_vae_latent_tile_f16"] = (
    Entry(dict(z=PTR, sc=1, st=1, sh=1, sw=1, C=1, T=1, H=1, W=1, Cpad=1, out=PTR), required=("z", "out"))
    .no("C > 0", C=0).no("T > 0", T=0).no("H > 0", H=0).no("W > 0", W=0).no("Cpad >= C", Cpad=0)
    .yes("the source strides are free", sc=0, st=-1, sh=0, sw=0)
    .limit("T*H*W*Cpad fits an int64", dict(T=I31, H=I31, W=1, Cpad=2), dict(T=I31, H=I31, W=2, Cpad=2)))

_ONES, _D1 = i64s(1, 1, 1, 1), i32s(1, 1, 1, 1)
E["hv_vae_blend_f16"] = (
    Entry(dict(a=PTR, a_strides=_ONES, b=PTR, b_strides=_ONES, dims=_D1, axis=0, extent=1),
          required=("a", "a_strides", "b", "b_strides", "dims"))
    .no("axis in 0..3", axis=-1).no("extent > 0", extent=0).no("dims[axis] <= extent", dims=i32s(2, 1, 1, 1)).no("dims > 0", dims=i32s(1, 0, 1, 1))
    .no("the element count fits an int64", dims=i32s(I31, I31, I31, I31), extent=I31)
    .limit("axis <= 3", dict(axis=3), dict(axis=4)))
E["hv_copy4d_16b"] = (
    Entry(dict(src=PTR, src_strides=_ONES, dst=PTR, dst_strides=_ONES, dims=_D1), required=("src", "src_strides", "dst", "dst_strides", "dims"))
    .no("dims > 0", dims=i32s(1, 0, 1, 1)).no("dims > 0", dims=i32s(1, 1, 1, -1))
    .no("the element count fits an int64", dims=i32s(I31, I31, I31, I31)).yes("three full int extents", dims=i32s(I31, I31, 1, 1)))

E["hv_vae_postprocess_f16_f32"] = Entry(dict(x=PTR, out=PTR, n=1), required=("x", "out")).no("n > 0", n=0).no("n > 0", n=-1)

# ------------------------------------------------------------------------------------------------ scoring kernels
_VID = dict(a=PTR, a_sc=49, a_st=49, a_sh=7, b=PTR, b_sc=49, b_st=49, b_sh=7, dtype=0)


def _metrics_ws(*shape):
    return lambda lib: lib.hv_video_metrics_workspace_bytes(*shape)


E["hv_video_metrics"] = (
    Entry(dict(_VID, C=1, T=1, H=7, W=7, rescale=0, passes=3, sse=PTR, minmax=PTR, ssim_sum=PTR, workspace=PTR,
               workspace_bytes=_metrics_ws(1, 1, 7, 7)), required=("a", "b", "sse", "minmax", "ssim_sum", "workspace"))
    .no("C 1 | 3", C=2).no("C 1 | 3", C=0).yes("C = 3", C=3, workspace_bytes=_metrics_ws(3, 1, 7, 7)).no("T >= 1", T=0)
    .no("dtype 0 | 1", dtype=2).no("rescale 0 | 1", rescale=2).no("passes 1..3", passes=0).no("passes 1..3", passes=4)
    .no("overlapping strides: a_sh >= W", a_sh=6).no("overlapping strides: b_sh >= W", b_sh=6).no("negative stride", a_sc=-1)
    .no("negative stride", a_st=-1).no("negative stride", b_sc=-1).no("negative stride", b_st=-1)
    .no("workspace 16-byte aligned", workspace=PTR + 8)
    .limit("H >= 7", dict(), dict(H=6)).limit("W >= 7", dict(), dict(W=6))
    .limit("T <= 65535", dict(T=65535, workspace_bytes=_metrics_ws(1, 65535, 7, 7)), dict(T=65536, workspace_bytes=I63))
    .limit("H <= 65536", dict(H=65536, workspace_bytes=_metrics_ws(1, 1, 65536, 7)), dict(H=65537, workspace_bytes=I63))
    .limit("W <= 65536", dict(W=65536, a_sh=65536, b_sh=65536, workspace_bytes=_metrics_ws(1, 1, 7, 65536)),
           dict(W=65537, a_sh=65537, b_sh=65537, workspace_bytes=I63))
    .limit("workspace_bytes >= hv_video_metrics_workspace_bytes(C, T, H, W)", dict(),
           dict(workspace_bytes=lambda lib: lib.hv_video_metrics_workspace_bytes(1, 1, 7, 7) - 1)))

_V31 = dict(a=PTR, a_sc=961, a_st=961, a_sh=31, b=PTR, b_sc=961, b_st=961, b_sh=31, dtype=0)
E["hv_lpips_conv1_f32"] = (
    Entry(dict(_V31, T=1, H=31, W=31, rescale=0, lut=PTR, w=PTR, bias=PTR, y=PTR), required=("a", "b", "lut", "w", "bias", "y"))
    .no("dtype 0 | 1", dtype=2).no("rescale 0 | 1", rescale=2).no("T >= 1", T=0)
    .no("overlapping strides: a_sh >= W", a_sh=30).no("overlapping strides: b_sh >= W", b_sh=30).no("negative stride", a_sc=-1)
    .no("negative stride", a_st=-1).no("negative stride", b_sc=-1).no("negative stride", b_st=-1).no("w 16-byte aligned", w=PTR + 4)
    .limit("H >= 31", dict(), dict(H=30)).limit("W >= 31", dict(), dict(W=30))
    .limit("T <= 32767", dict(T=32767), dict(T=32768))
    .limit("H <= 65536", dict(H=65536), dict(H=65537))
    .limit("W <= 65536", dict(W=65536, a_sh=65536, b_sh=65536), dict(W=65537, a_sh=65537, b_sh=65537)))
E["hv_lpips_conv2d_f32"] = (
    Entry(dict(x=PTR, w=PTR, bias=PTR, y=PTR, N=1, H=1, W=1, Cin=32, Cout=64, ksize=1, pad=0), required=("x", "w", "bias", "y"))
    .no("N >= 1", N=0).no("H >= 1", H=0).no("W >= 1", W=0).no("Cin % 32 == 0", Cin=48).no("Cin >= 32", Cin=0).no("Cout % 64 == 0", Cout=96)
    .no("Cout >= 64", Cout=0).no("ksize >= 1", ksize=0).no("pad >= 0", pad=-1).no("pad < ksize", pad=1)
    .no("the output has at least one pixel", ksize=3).no("x 16-byte aligned", x=PTR + 4).no("w 16-byte aligned", w=PTR + 4)
    .limit("H <= 65536", dict(H=65536), dict(H=65537)).limit("W <= 65536", dict(W=65536), dict(W=65537))
    .limit("Cin <= 4096", dict(Cin=4096), dict(Cin=4128)).limit("Cout <= 4096", dict(Cout=4096), dict(Cout=4160))
    .limit("ksize <= 11", dict(ksize=11, pad=5), dict(ksize=12, pad=6))
    .limit("N*H*W <= 2^31 - 1", dict(N=I31), dict(N=I31, H=2)))
E["hv_lpips_maxpool_f32"] = (
    Entry(dict(x=PTR, y=PTR, N=1, H=3, W=3, C=4), required=("x", "y"))
    .no("N >= 1", N=0).no("C >= 4", C=0).no("C % 4 == 0", C=6).no("x 16-byte aligned", x=PTR + 4).no("y 16-byte aligned", y=PTR + 4)
    .limit("H >= 3", dict(), dict(H=2)).limit("W >= 3", dict(), dict(W=2))
    .limit("H <= 65536", dict(H=65536), dict(H=65537)).limit("W <= 65536", dict(W=65536), dict(W=65537))
    .limit("C <= 4096", dict(C=4096), dict(C=4100))
    .limit("one thread per 4 channels: the workgroups fit grid.x", dict(N=I31, C=1024), dict(N=I31, C=1028)))


def _lpips_ws(t, p):
    return lambda lib: lib.hv_lpips_distance_workspace_bytes(t, p)


E["hv_lpips_distance_f32"] = (
    Entry(dict(f=PTR, lin=PTR, T=1, P=1, C=1, layer=0, out=PTR, workspace=PTR, workspace_bytes=_lpips_ws(1, 1)),
          required=("f", "lin", "out", "workspace"))
    .no("T >= 1", T=0).no("P >= 1", P=0).no("C >= 1", C=0).no("layer >= 0", layer=-1).no("workspace 8-byte aligned", workspace=PTR + 4)
    .limit("T <= 65535", dict(T=65535, workspace_bytes=_lpips_ws(65535, 1)), dict(T=65536, workspace_bytes=I63))
    .limit("C <= 384", dict(C=384), dict(C=385)).limit("layer <= 4", dict(layer=4), dict(layer=5))
    .limit("workspace_bytes >= hv_lpips_distance_workspace_bytes(T, P)", dict(),
           dict(workspace_bytes=lambda lib: lib.hv_lpips_distance_workspace_bytes(1, 1) - 1)))

_BK, _BINS, _MAXT = M["HV_SPECTRUM_BK"], M["HV_SPECTRUM_BINS"], M["HV_SPECTRUM_MAX_T"]


def twiddle_floats(t):
    """the header's rule: Tpad * 64 * ncol with Tpad = T rounded up to HV_SPECTRUM_BK and HV_SPECTRUM_BINS bins per column tile"""
    return -(-t // _BK) * _BK * 2 * _BINS * max(1, -(-(t // 2) // _BINS))


def _spec_ws(*a):
    return lambda lib: lib.hv_temporal_spectrum_workspace_bytes(*a)


_SPEC = dict(x=PTR, sc=1, st=1, sh=1, dtype=1, mode=1, C=1, T=1, H=1, W=1, rescale=0, wr=0, wg=0, wb=0, round=0, shift=0, twiddle=PTR,
             twiddle_floats=twiddle_floats(1), mag_sum=PTR, pow_sum=PTR, workspace=PTR, workspace_bytes=_spec_ws(1, 1, 1, 1, 1))
_GRAY = dict(mode=0, C=3, wr=1, workspace_bytes=_spec_ws(0, 3, 1, 1, 1))
E["hv_temporal_spectrum"] = (
    Entry(_SPEC, required=("x", "twiddle", "mag_sum", "pow_sum", "workspace"))
    .no("dtype 0 | 1", dtype=2).no("rescale 0 | 1", rescale=2).no("mode 0 | 1", mode=2).no("T >= 1", T=0).no("C >= 1", C=0)
    .no("H >= 1", H=0).no("W >= 1", W=0).no("overlapping strides: sh >= W", sh=0).no("negative stride", sc=-1).no("negative stride", st=-1)
    .no("C == 3 in mode 0", mode=0, wr=1)
    .yes("mode 0 (gray8) with a byte luma", **_GRAY)
    .no("mode 0: weights >= 0", **dict(_GRAY, wr=-1)).no("mode 0: round >= 0", **dict(_GRAY, round=-1))
    .no("mode 0: shift >= 0", **dict(_GRAY, shift=-1)).no("mode 0: the luma stays a byte", **dict(_GRAY, wr=2))
    .no("mode 0: the luma stays a byte", **dict(_GRAY, round=1)).no("mode 0: weights <= 2^22", **dict(_GRAY, wr=(1 << 22) + 1, shift=22))
    .limit("mode 0: shift <= 22", dict(_GRAY, wr=1 << 22, shift=22), dict(_GRAY, wr=1 << 22, shift=23))
    .no("twiddle 16-byte aligned", twiddle=PTR + 4).no("workspace 8-byte aligned", workspace=PTR + 4)
    .limit("T <= HV_SPECTRUM_MAX_T", dict(T=_MAXT, twiddle_floats=twiddle_floats(_MAXT), workspace_bytes=_spec_ws(1, 1, _MAXT, 1, 1)),
           dict(T=_MAXT + 1, twiddle_floats=I63, workspace_bytes=I63), macros=("HV_SPECTRUM_MAX_T",))
    .limit("twiddle_floats >= Tpad * 64 * ncol (Tpad from HV_SPECTRUM_BK, ncol from HV_SPECTRUM_BINS), one column tile",
           dict(T=_BK + 1, twiddle_floats=twiddle_floats(_BK + 1), workspace_bytes=_spec_ws(1, 1, _BK + 1, 1, 1)),
           dict(T=_BK + 1, twiddle_floats=twiddle_floats(_BK + 1) - 1, workspace_bytes=_spec_ws(1, 1, _BK + 1, 1, 1)), macros=("HV_SPECTRUM_BK",))
    .limit("twiddle_floats: a second column tile from T / 2 = HV_SPECTRUM_BINS + 1 on",
           dict(T=2 * _BINS + 2, twiddle_floats=twiddle_floats(2 * _BINS + 2), workspace_bytes=_spec_ws(1, 1, 2 * _BINS + 2, 1, 1)),
           dict(T=2 * _BINS + 2, twiddle_floats=twiddle_floats(2 * _BINS + 2) - 1, workspace_bytes=_spec_ws(1, 1, 2 * _BINS + 2, 1, 1)),
           macros=("HV_SPECTRUM_BINS",))
    .limit("C <= 65536", dict(C=65536, workspace_bytes=_spec_ws(1, 65536, 1, 1, 1)), dict(C=65537, workspace_bytes=I63))
    .limit("H <= 65536", dict(H=65536, workspace_bytes=_spec_ws(1, 1, 1, 65536, 1)), dict(H=65537, workspace_bytes=I63))
    .limit("W <= 65536", dict(W=65536, sh=65536, workspace_bytes=_spec_ws(1, 1, 1, 1, 65536)), dict(W=65537, sh=65537, workspace_bytes=I63))
    .limit("H * W <= 2^31 - 1", dict(H=65536, W=32767, sh=32767, workspace_bytes=_spec_ws(1, 1, 1, 65536, 32767)),
           dict(H=65536, W=32768, sh=32768, workspace_bytes=I63))
    .limit("workspace_bytes >= hv_temporal_spectrum_workspace_bytes(...)", dict(),
           dict(workspace_bytes=lambda lib: lib.hv_temporal_spectrum_workspace_bytes(1, 1, 1, 1, 1) - 1)))

E["hv_i3d_preprocess"] = (
    Entry(dict(x=PTR, x_sc=1, x_st=1, x_sh=1, dtype=0, T=1, H=1, W=1, RH=224, RW=224, rescale=0, y=PTR), required=("x", "y"))
    .no("dtype 0 | 1", dtype=2).no("rescale 0 | 1", rescale=2).no("T >= 1", T=0).no("H >= 1", H=0).no("W >= 1", W=0)
    .no("overlapping strides: x_sh >= W", x_sh=0).no("negative stride", x_sc=-1).no("negative stride", x_st=-1).no("y 16-byte aligned", y=PTR + 8)
    .no("one side's extent is 224", RH=225, RW=225).no("the shorter side's extent is 224", W=2, x_sh=2, RH=225)
    .yes("the longer side may exceed 224", W=2, x_sh=2, RW=448).yes("a square clip may come as 225 x 224", RH=225)
    .limit("RH >= 224", dict(), dict(RH=223)).limit("RW >= 224", dict(), dict(RW=223))
    .limit("RH <= 2^20", dict(RH=1 << 20), dict(RH=(1 << 20) + 1))
    .limit("T <= 65536", dict(T=65536), dict(T=65537)).limit("H <= 65536", dict(H=65536), dict(H=65537))
    .limit("W <= 65536", dict(W=65536, x_sh=65536), dict(W=65537, x_sh=65537)))

_KSP = dict(kt=1, kh=1, kw=1, stride_t=1, stride_h=1, stride_w=1, pad_t=0, pad_h=0, pad_w=0)
E["hv_i3d_conv3d_f32"] = (
    Entry(dict(x=PTR, ldx=4, w=PTR, sc=PTR, sh=PTR, y=PTR, ldy=4, T=1, H=1, W=2, Cin=4, Cout=4, relu=0, **_KSP),
          required=("x", "w", "sc", "sh", "y"))
    .no("relu 0 | 1", relu=2).no("T >= 1", T=0).no("H >= 1", H=0).no("W >= 1", W=0).no("Cin >= 4", Cin=0).no("Cin % 4 == 0", Cin=6, ldx=8)
    .no("Cout >= 4", Cout=0).no("Cout % 4 == 0", Cout=6, ldy=8).no("kernel extent 1 | 3 | 7", kt=2).no("kernel extent 1 | 3 | 7", kh=5)
    .no("kernel extent 1 | 3 | 7", kw=0).no("stride 1 | 2", stride_t=0).no("stride 1 | 2", stride_h=3).no("stride 1 | 2", stride_w=3)
    .no("pad >= 0", pad_t=-1).no("pad < kernel extent", pad_h=1).no("pad < kernel extent", pad_w=1)
    .yes("7-tap kernel, stride 2, pad 3", kt=7, stride_t=2, pad_t=3)
    .no("ldx >= Cin", ldx=0).no("ldx % 4 == 0", ldx=6).no("output pitch: ldy >= Cout", ldy=0)
    .no("x 16-byte aligned", x=PTR + 4).no("w 16-byte aligned", w=PTR + 4)
    .limit("T <= 65536", dict(T=65536, W=1), dict(T=65537, W=1)).limit("H <= 65536", dict(H=65536, W=1), dict(H=65537, W=1))
    .limit("W <= 65536", dict(W=65536), dict(W=65537))
    .limit("T*H*W <= 2^31 - 1", dict(T=32767, H=65536, W=1), dict(T=32768, H=65536, W=1))
    .limit("Cin <= 4096", dict(Cin=4096, ldx=4096), dict(Cin=4100, ldx=4100))
    .limit("Cout <= 4096", dict(Cout=4096, ldy=4096), dict(Cout=4100, ldy=4100)))
E["hv_i3d_maxpool3d_f32"] = (
    Entry(dict(x=PTR, ldx=4, y=PTR, ldy=4, T=1, H=1, W=2, C=4, **_KSP), required=("x", "y"))
    .no("T >= 1", T=0).no("H >= 1", H=0).no("W >= 1", W=0).no("C >= 4", C=0).no("C % 4 == 0", C=6, ldx=8, ldy=8)
    .no("ldx >= C", ldx=0).no("ldx % 4 == 0", ldx=6).no("output pitch: ldy >= C", ldy=0).no("ldy % 4 == 0", ldy=6)
    .no("kernel extent >= 1", kt=0).no("stride 1 | 2", stride_h=0).no("stride 1 | 2", stride_w=3).no("pad >= 0", pad_t=-1)
    .no("pad < kernel extent", pad_w=1).no("x 16-byte aligned", x=PTR + 4).no("y 16-byte aligned", y=PTR + 4)
    .limit("kernel extent <= 3", dict(kh=3, pad_h=2), dict(kh=4, pad_h=2))
    .limit("T <= 65536", dict(T=65536, W=1), dict(T=65537, W=1)).limit("W <= 65536", dict(W=65536), dict(W=65537))
    .limit("T*H*W <= 2^31 - 1", dict(T=32767, H=65536, W=1), dict(T=32768, H=65536, W=1))
    .limit("C <= 4096", dict(C=4096, ldx=4096, ldy=4096), dict(C=4100, ldx=4100, ldy=4100)))
_HT = M["HV_I3D_HEAD_MAX_T"]
E["hv_i3d_head_f32"] = (
    Entry(dict(x=PTR, ldx=1024, w=PTR, bias=PTR, out=PTR, T=2, H=7, W=7, C=1024, workspace=PTR, workspace_floats=1024),
          required=("x", "w", "bias", "out", "workspace"))
    .no("H == 7", H=6).no("W == 7", W=8).no("C == 1024", C=512).no("ldx >= C", ldx=1020).no("ldx % 4 == 0", ldx=1026)
    .no("x 16-byte aligned", x=PTR + 4).no("workspace 16-byte aligned", workspace=PTR + 4)
    .limit("T >= 2", dict(), dict(T=1))
    .limit("T <= HV_I3D_HEAD_MAX_T", dict(T=_HT, workspace_floats=(_HT - 1) * 1024), dict(T=_HT + 1, workspace_floats=_HT * 1024),
           macros=("HV_I3D_HEAD_MAX_T",))
    .limit("workspace_floats >= (T - 1) * 1024", dict(), dict(workspace_floats=1023)))

_SIDE = M["HV_YUV_MAX_SIDE"]
E["hv_yuv420_to_clip"] = (
    Entry(dict(raw=PTR, T=1, layout=M["HV_YUV_I420"], W=2, H=2, out=PTR, dtype=0, sc=4, st=4, sh=2, OH=2, OW=2, ytab=PTR, xtab=PTR, vtab=PTR),
          required=("raw", "out", "vtab"), nullable=("ytab", "xtab"))
    .no("T >= 1", T=0).no("dtype 0 | 1", dtype=2).no("W positive", W=0).no("W even", W=3).no("H positive", H=0).no("H even", H=3)
    .no("OH >= 1", OH=0).no("OW >= 1", OW=0)
    .no("differing sizes need both tables", OH=4, sc=8, st=8, ytab=None).no("differing sizes need both tables", OH=4, sc=8, st=8, xtab=None)
    .yes("resize with both tables", OH=4, sc=8, st=8)
    .no("vtab aligned to the output dtype", vtab=PTR + 1).no("out aligned to the output dtype", out=PTR + 1)
    .no("negative stride", sc=-4).no("negative stride", st=-4, T=2).no("two cells share an address: sh < OW", sh=1)
    .no("two cells share an address: channels inside a frame's rows", sc=2)
    .limit("layout >= HV_YUV_I420", dict(layout=M["HV_YUV_I420"]), dict(layout=M["HV_YUV_I420"] - 1), macros=("HV_YUV_I420",))
    .limit("layout HV_YUV_YV12", dict(layout=M["HV_YUV_YV12"]), None, macros=("HV_YUV_YV12",))
    .limit("layout <= HV_YUV_NV12", dict(layout=M["HV_YUV_NV12"]), dict(layout=M["HV_YUV_NV12"] + 1), macros=("HV_YUV_NV12",))
    .limit("W <= HV_YUV_MAX_SIDE", dict(W=_SIDE), dict(W=_SIDE + 2), macros=("HV_YUV_MAX_SIDE",))
    .limit("H <= HV_YUV_MAX_SIDE", dict(H=_SIDE), dict(H=_SIDE + 2), macros=("HV_YUV_MAX_SIDE",))
    .limit("OH <= HV_YUV_MAX_SIDE", dict(OH=_SIDE, sc=2 * _SIDE, st=2 * _SIDE), dict(OH=_SIDE + 1, sc=2 * _SIDE + 2, st=2 * _SIDE + 2),
           macros=("HV_YUV_MAX_SIDE",))
    .limit("OW <= HV_YUV_MAX_SIDE", dict(OW=_SIDE, sh=_SIDE, sc=2 * _SIDE, st=2 * _SIDE),
           dict(OW=_SIDE + 1, sh=_SIDE + 1, sc=2 * _SIDE + 2, st=2 * _SIDE + 2), macros=("HV_YUV_MAX_SIDE",)))

# Macros that are no argument limit (with the reason), and conditions the host side cannot be driven to (at most five).
MACROS_NOT_LIMITS = {
    "HV_ABI_VERSION": "the version of the header (tests/test_capi_cpu.py pins it against the library and the recorded ABI)",
    "HV_YUV_COEF_BITS": "precision of the caller-built resize tables; the kernel clamps an entry into range, the host checks nothing",
}
NOT_DRIVEN = [
    ("hv_attn_fwd_bf16", "workspace_bytes below hv_attn_workspace_bytes(...) is no refusal: the header documents that the call then runs "
                         "without the KV split (and below HV_ATTN_MIN_WORKSPACE_BYTES without the key bound), so the query has no "
                         "size / size - 1 pair"),
    ("hv_yuv420_to_clip", "table entries outside [0, 2^HV_YUV_COEF_BITS] live in device memory; the kernel clamps them"),
]

# ------------------------------------------------------------------------------------------------ pure host queries (no stream)
# name -> [(arguments, expected value or None for "positive")]; the refused shapes answer 0, and no argument makes one negative.
QUERIES = {
    "hv_attn_workspace_bytes": [((2, 64, 1), 256 + 2 * 2 * 130 * 4), ((0, 4096, 1), 256), ((-1, 4096, 1), 0), ((2, -1, 1), 0), ((2, 0, 1), 0),
                                ((2, 64, 0), 0), ((2, 64, -3), 0), ((2, _KV_MAX + 1, 1), 0), ((I31, 64, 256), 0)],
    "hv_attn_suggest_splits": [((118811, 118811, 3), 2), ((118811, 118811, 24), 1), ((0, 64, 1), 1), ((-1, 64, 1), 0), ((2, 0, 1), 0),
                               ((2, -64, 1), 0), ((2, 64, 0), 0), ((I31, 64, 256), 0)],
    "hv_gn_partial_rows": [((90,), 4), ((256,), 4), ((257,), 8), ((0,), 0), ((-5,), 0), ((I31 + 1,), 0)],
    "hv_subpixel_gn_partial_rows": [((1, 4, 4, 1), 16), ((17, 64, 64, 1), 4 * (4 * 272 + 4 * 256)), ((0, 4, 4, 1), 0), ((1, 0, 4, 0), 0),
                                    ((1, 4, -4, 0), 0), ((1, 4, 4, 2), 0), ((255, 4, 4, 0), 0), ((1, 4097, 4, 0), 0), ((254, 4096, 4096, 1), 0)],
    "hv_conv3d_cout4_planes_floats": [((2,), 162), ((0,), 0), ((-1,), 0), ((256 * I31,), 81 * 256 * I31), ((256 * I31 + 1,), 0)],
    "hv_video_metrics_workspace_bytes": [((1, 1, 7, 7), None), ((3, 65535, 7, 7), None), ((2, 1, 7, 7), 0), ((1, 0, 7, 7), 0), ((1, 65536, 7, 7), 0),
                                         ((1, 1, 6, 7), 0), ((1, 1, 7, 6), 0), ((1, 1, 65537, 7), 0), ((1, 1, -7, 7), 0)],
    "hv_lpips_distance_workspace_bytes": [((1, 1), None), ((65535, 1 << 40), None), ((0, 1), 0), ((65536, 1), 0), ((1, 0), 0), ((1, -1), 0)],
    "hv_temporal_spectrum_workspace_bytes": [((1, 1, 1, 1, 1), None), ((0, 3, _MAXT, 8, 8), None), ((0, 1, 8, 8, 8), 0), ((2, 1, 8, 8, 8), 0),
                                             ((1, 1, _MAXT + 1, 8, 8), 0), ((1, 0, 8, 8, 8), 0), ((1, 1, 0, 8, 8), 0), ((1, 1, 8, 65537, 8), 0),
                                             ((1, 1, 8, 65536, 65536), 0), ((1, -1, 8, 8, 8), 0)],
}
SWEEP = (-(1 << 31), -1, 0, 1, 7, 4096, I31)      # every query is also called on the full product of these: never negative

# (query, its arguments, kernel, the size argument, scale from the query's answer to the size): the size is accepted by the kernel at
# its baseline shape, the size minus one refused.
SIZE_RULES = [
    ("hv_gn_partial_rows", (2,), "hv_conv3d_causal_f16", "gn_partial_floats", 8 * 2),
    ("hv_subpixel_gn_partial_rows", (1, 1, 1, 0), "hv_conv3d_upsampled_subpixel_f16", "gn_partial_floats", 136 * 2),
    ("hv_conv3d_cout4_planes_floats", (2,), "hv_conv3d_cout4_f16", "planes_floats", 1),
    ("hv_video_metrics_workspace_bytes", (1, 1, 7, 7), "hv_video_metrics", "workspace_bytes", 1),
    ("hv_lpips_distance_workspace_bytes", (1, 1), "hv_lpips_distance_f32", "workspace_bytes", 1),
    ("hv_temporal_spectrum_workspace_bytes", (1, 1, 1, 1, 1), "hv_temporal_spectrum", "workspace_bytes", 1),
]


# ------------------------------------------------------------------------------------------------ helpers
def stream_decls():
    """name -> [(C type, parameter)] of the declarations that take a hipStream_t"""
    return {name: params for _, name, params in _abi.DECLS if any(t == "hipStream_t" for t, _ in params)}


def pointer_params(params):
    return [p for t, p in params if t.endswith("*")]


def call(lib, name, overrides=None):
    """the entry point at its baseline with `overrides` applied, NULL stream -> return code"""
    e = E[name]
    vals = dict(e.base)
    unknown = set(overrides or ()) - set(vals)
    assert not unknown, f"{name}: overrides {sorted(unknown)} name no parameter of the baseline"
    vals.update(overrides or {})
    args = []
    for ctype, p in stream_decls()[name]:
        if ctype == "hipStream_t":
            args.append(None)
            continue
        v = vals[p]
        if callable(v):
            v = v(lib)
        if isinstance(v, C.Array):
            v = C.cast(v, C.c_void_p)
        args.append(v)
    return getattr(lib, name)(*args)


def rows():
    """every parametrised case: (id, entry point, overrides, expected code or "base")"""
    out = []
    for name, e in E.items():
        out.append((f"{name}-baseline", name, {}, LAUNCH))
        for p in e.required:
            out.append((f"{name}-NULL-{p}", name, {p: None}, ARG))
        for p in e.nullable:
            out.append((f"{name}-NULL-ok-{p}", name, {p: None}, LAUNCH))
            out.append((f"{name}-set-ok-{p}", name, {p: PTR}, LAUNCH))
        for kind, lst, want in (("refuse", e.refuse, ARG), ("accept", e.accept, LAUNCH), ("early", e.early, OK)):
            for i, (rule, ov) in enumerate(lst):
                out.append((f"{name}-{kind}{i}-{rule}", name, ov, want))
        for i, (rule, _, ok, bad) in enumerate(e.limits):
            out.append((f"{name}-limit{i}-ok-{rule}", name, ok, LAUNCH))
            if bad is not None:
                out.append((f"{name}-limit{i}-refuse-{rule}", name, bad, ARG))
    return out


def sweep(nargs):
    return itertools.product(SWEEP, repeat=nargs)
