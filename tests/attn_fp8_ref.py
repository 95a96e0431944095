"""TEST INFRASTRUCTURE: the FP8 attention of include/hv_attn_fp8.h restated in torch - the quantisation rules (`restate`), the workspace
layout in both directions (`unpack`, `pack`), the dequantised operands (`dequantised`) and the fp64 reference with its bound (`fp8_bound`).
Shared by tests/test_gpu_attn_fp8.py (the kernel), tests/cpu_kernel_doubles.py (the CPU doubles) and tests/double_parity.py.

The bound per output element d, with w_j the fp64 softmax weights over the DEQUANTISED operands (sq Q8, sk K8, sv V8, log2 domain),
l = sum_j 2^(s_j - M) >= 1 and v~ the dequantised V:

    ulp_bf16(O64_d)                                                   the final rounding (EB.ulp_out)
  + sum_j max(2^-4 w_j, 2^-18 / l) |v~_jd|                            e4m3(p 2^8): half an ulp relative (3 mantissa bits) down to
                                                                      p 2^8 = 2^-6, half the subnormal spacing 2^-10 below; a p rounded
                                                                      against an earlier, smaller running maximum is scaled down after
  + sum_j eta_j w_j |v~_jd - O64_d|,  eta_j = ln 2 bs_j + 2^-22        a relative error of p_j shared by numerator and row sum (the form of
                                                                      attention_bounds.py); bs_j = C sqrt(128) 2^-24 S_j + 2^-22 (|s_j| +
                                                                      |M|): the 128-term reduction of the fp8 MFMA in the worst-case form
                                                                      error_bounds.py prescribes for it (S_j = sum_c |q'_c k_jc|), then the
                                                                      two scale multiplies and the subtraction of m; 2^-22 for v_exp_f32
  + C sqrt(n_kv) 2^-24 (sum_j w_j |v~_jd| + 2 |O64_d|)                fp32 accumulation of P.V and l, the per-tile rescales and the epilogue,
                                                                      worst-case form as well.
No term is fitted to the kernel."""
import math

import torch

from hunyuanvideo_efficiency_amd.attn_fp8 import attn_fp8_layout
from tests import attention_bounds as AB
from tests import error_bounds as EB

FP8 = torch.float8_e4m3fn
D, KVT = 128, 64
_P = torch.arange(KVT)
V_KEY = 32 * ((_P >> 4) & 1) + 8 * ((_P >> 2) & 3) + 4 * (_P >> 5) + (_P & 3)      # the header's key(p)
AREAS = ("kmean", "sv", "sk", "sq", "q8", "k8", "v8")                              # what a caller may read; `part` is scratch


def _area(ws, L, name, n, dtype):
    return ws[L[name]:L[name] + n * torch.empty(0, dtype=dtype).element_size()].view(dtype)


def unpack(ws, n_q, n_kv, H):
    """the workspace areas in natural order: kmean, sv [H, 128], sk [H, nt], sq [n_q, H] fp32; q8 [n_q, H, 128], k8, v8 [H, nt 64, 128] e4m3"""
    L = attn_fp8_layout(n_q, n_kv, H)
    nt = L["nt"]
    v8 = _area(ws, L, "v8", H * nt * 8192, FP8).view(H, nt, D, KVT)
    v_nat = torch.empty(H, nt, KVT, D, dtype=FP8, device=ws.device)
    v_nat.view(torch.uint8)[:, :, V_KEY.to(ws.device)] = v8.view(torch.uint8).transpose(2, 3)
    return dict(kmean=_area(ws, L, "kmean", H * D, torch.float32).view(H, D), sv=_area(ws, L, "sv", H * D, torch.float32).view(H, D),
                sk=_area(ws, L, "sk", H * nt, torch.float32).view(H, nt), sq=_area(ws, L, "sq", n_q * H, torch.float32).view(n_q, H),
                q8=_area(ws, L, "q8", n_q * H * D, FP8).view(n_q, H, D), k8=_area(ws, L, "k8", H * nt * 8192, FP8).view(H, nt * KVT, D),
                v8=v_nat.view(H, nt * KVT, D))


def pack(areas, ws, n_q, n_kv, H):
    """the inverse of unpack: natural-order areas (the dict `restate` returns) into the workspace bytes; `part`, the alignment gaps and
    the bytes behind the layout's total are not touched"""
    L = attn_fp8_layout(n_q, n_kv, H)
    nt = L["nt"]
    _area(ws, L, "kmean", H * D, torch.float32).copy_(areas["kmean"].reshape(-1))
    _area(ws, L, "sv", H * D, torch.float32).copy_(areas["sv"].reshape(-1))
    _area(ws, L, "sk", H * nt, torch.float32).copy_(areas["sk"].reshape(-1))
    _area(ws, L, "sq", n_q * H, torch.float32).copy_(areas["sq"].reshape(-1))
    _area(ws, L, "q8", n_q * H * D, torch.uint8).copy_(areas["q8"].contiguous().view(torch.uint8).reshape(-1))
    _area(ws, L, "k8", H * nt * 8192, torch.uint8).copy_(areas["k8"].contiguous().view(torch.uint8).reshape(-1))
    v_nat = areas["v8"].contiguous().view(torch.uint8).view(H, nt, KVT, D)
    v8 = v_nat[:, :, V_KEY.to(ws.device)].transpose(2, 3)                          # byte p of row d holds key V_KEY[p]
    _area(ws, L, "v8", H * nt * 8192, torch.uint8).copy_(v8.reshape(-1))
    return ws


def restate(q, k, v, H, blk, scale=None):
    """the header's quantisation rules in fp32 torch, natural order (q [n_q, H 128], k, v [n_kv, H 128] bf16 on the CPU)"""
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)
    scale_of = lambda a: torch.where(a > 0, torch.clamp(a * (f32(1.0) / f32(448.0)), min=2.0 ** -126), torch.ones_like(a))
    code = lambda x, s: (x * (f32(1.0) / s)).clamp(-448.0, 448.0).to(FP8)
    n_q, n_kv, nt = q.shape[0], k.shape[0], -(-k.shape[0] // KVT)
    kf, vf = k.float().view(n_kv, H, D), v.float().view(n_kv, H, D)
    total, vmax = torch.zeros(H, D), torch.zeros(H, D)
    for b0 in range(0, n_kv, blk):
        sums, maxs = [], []
        for c in range(4):
            s, m = torch.zeros(H, D), torch.zeros(H, D)
            for j in range(b0 + c, min(b0 + blk, n_kv), 4):
                s, m = s + kf[j], torch.maximum(m, vf[j].abs())
            sums.append(s), maxs.append(m)
        total = total + ((sums[0] + sums[1]) + (sums[2] + sums[3]))
        vmax = torch.maximum(vmax, torch.stack(maxs).max(dim=0).values)
    kmean, sv = total / f32(float(n_kv)), scale_of(vmax)
    qp = q.float().view(n_q, H, D) * AB.scale_log2e(scale)
    sq = scale_of(qp.abs().amax(dim=2))
    kc = torch.zeros(nt * KVT, H, D)
    kc[:n_kv] = kf - kmean
    sk = scale_of(kc.view(nt, KVT, H, D).abs().amax(dim=(1, 3))).T.contiguous()                    # [H, nt]
    v_pad = torch.zeros(nt * KVT, H, D)
    v_pad[:n_kv] = vf
    return dict(kmean=kmean, sv=sv, sk=sk, sq=sq, q8=code(qp, sq[:, :, None]),
                k8=code(kc.view(nt, KVT, H, D), sk.T[:, None, :, None]).view(nt * KVT, H, D).transpose(0, 1),
                v8=code(v_pad, sv[None]).transpose(0, 1))


def dequantised(u, h, n_kv):
    """fp64 (q' [n_q, 128], k, v [n_kv, 128]) of head h from the unpacked areas `u`"""
    qd = u["q8"][:, h].float().double() * u["sq"][:, h, None].double()
    kd = (u["k8"][h].float().double() * u["sk"][h].double().repeat_interleave(KVT)[:, None])[:n_kv]
    vd = (u["v8"][h].float().double() * u["sv"][h].double())[:n_kv]
    return qd, kd, vd


def fp8_bound(qd, kd, vd, n_kv):
    """one head, fp64: dequantised q' [n_q, 128], k, v [n_kv, 128] -> (O64, bound); the module docstring's terms"""
    ref = EB.Ref().add(qd, kd)
    s = ref.y
    M = s.max(dim=1, keepdim=True).values
    e = torch.exp2(s - M)
    l = e.sum(dim=1, keepdim=True)
    w = e / l
    O = w @ vd
    p8 = torch.maximum(2.0 ** -4 * w, 2.0 ** -18 / l.expand_as(w)) @ vd.abs()
    bs = EB.C * math.sqrt(D) * EB.EPS32 * ref.s + 2.0 ** -22 * (s.abs() + M.abs())
    eta = AB._eta_term((AB.LN2 * bs + 2.0 ** -22) * w, vd, O)
    acc = EB.C * math.sqrt(n_kv) * EB.EPS32 * (w @ vd.abs() + 2.0 * O.abs())
    return O, EB.ulp_out(O, torch.bfloat16) + p8 + eta + acc


def check_fwd(out, ws, n_q, n_kv, H, what):
    """the bf16 output [n_q, >= H 128] of the forward against fp64 attention over the workspace it read; returns the worst error / bound"""
    u = unpack(ws, n_q, n_kv, H)
    worst = 0.0
    for h in range(H):
        O, bound = fp8_bound(*dequantised(u, h, n_kv), n_kv)
        got = out[:, h * D:(h + 1) * D].double().to(O.device)
        assert bool(torch.isfinite(got).all()), f"{what}: head {h} is not finite"
        ratio = (got - O).abs() / bound
        worst = max(worst, float(ratio.max()))
        i, d = divmod(int(ratio.argmax()), D)
        assert float(ratio.max()) <= 1.0, (f"{what} head {h}/{H}: {int((ratio > 1).sum())} elements outside the bound, worst "
                                           f"{float(ratio.max()):.3g} at row {i} dim {d}: got {float(got[i, d])}, O64 {float(O[i, d]):.6g}")
    return worst
