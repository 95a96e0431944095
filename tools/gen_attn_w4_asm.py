#!/usr/bin/env python3
"""Generate hunyuanvideo_efficiency_amd/csrc/hv_attention_w4_loop.inc: the steady-state iteration of the 4-wave x 64-row attention
kernel (hv_attention_w4.hip) as ONE inline-asm statement with every register named literally.

Why one statement: hipcc pads an `s_nop` in front of every instruction that reads a VGPR the previous asm statement wrote (it
does not count the instructions inside asm as wait states), so a loop built from one asm statement per instruction carries ~1.5
s_nop per MFMA gap - and a wave that is alone on its SIMD pays ~4 issue cycles for each (MI355X_MICROARCH.md, 'vector-instruction
ISSUE cost').  Inside one statement nothing is padded; the wait states below are met by placement and stated where they matter.

Register map (arch VGPRs pinned by "{v[..]}" constraints, accumulator registers owned by literal names):
  v[0:63]   S_A  tile (qb, kb) at 16 (2 qb + kb)        v[64:127] S_B           (roles swap every iteration: AB / BA statements)
  v[128:159] -m, the C operand of the S chains (qb 0 | 1)
  v[160:191] packed P: (qb, k-step kk) at 160 + 4 (4 qb + kk)
  v[192:199] ring of the last 8 exponentials     v200 v201 row sums l[qb]     v202 v203 row max of S'(t+1) [qb] (lane-local)
  v[206:209] V fragment addresses (db 0..3) and v[236:243] K fragment addresses (ks 0..7): STATIC per kernel - the four-deep K / V tile
  rings are walked by a x4 unrolled loop, so every ring buffer is a compile-time immediate of the ds_read / the DMA's M0
  v[212:215] K DMA offsets (piece 0..3)   v[216:219] V DMA offsets
  a[0:127] O   a[128:191] Q'   a[192:223] K fragment ring (8 x 4)   a[224:255] V fragment ring (8 x 4)
Schedule per iteration t (64 MFMA gaps): see hv_attention_w4.hip header; the tables here are the single source of it.
"""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "hv_attention_w4_loop.inc")

A_O, A_Q, A_KF, A_VF = 0, 128, 192, 224
RING = 8
PF = 4          # fragments of LDS read-ahead (must match hv_attention_w4.hip)
WGRP = 2        # one counted lgkmcnt wait per WGRP fragments (must match hv_attention_w4.hip)
ORDER = "rdpaem"    # order of a gap's fillers behind its MFMA: fragment reads, DMA piece, packs, adds, exps, row max (memory first: +2.9 % over VALU first, profiles/r03/attn_filler_order.txt)
DMAPH = 3       # the DMA pieces go to gaps = DMAPH (mod 4) of the S phase
LAG = 1         # gaps between a v_exp_f32 and the pack / row-sum add that read it
EXR = 12                                          # ring of the last exponentials (>= 2 per gap x (LAG + 1) + the pair partner)
V_NEGM, V_PW, V_EX, V_L, V_MX, V_VV, V_KOFF, V_VOFF, V_VKS = 128, 160, 222, 200, 202, 206, 212, 216, 236
NBUF, TILE_BYTES = 4, 16384
LDS_KOFF, LDS_VOFF = 0, NBUF * TILE_BYTES      # LDS bytes: [K0 K1 K2 K3 | V0 V1 V2 V3]
V_L2 = 234      # second partial row sum per query block (v234, v235): consecutive adds never hit the same accumulator


def l_reg(qb, odd):
    return (V_L2 if odd else V_L) + qb


def exps_before(g):
    """exponentials issued before gap g: 5 per 4 gaps through the S phase (gaps 0..31: 40), then one per gap, the last at gap 54 (two in
    gap 32), so that with the consumers up to 2 gaps behind, the pack of the last pair (gap <= 56) precedes its MFMA (gap 57)."""
    if g <= 32:
        return g + (g + 3) // 4
    return min(64, 41 + (g - 32))


def frag_insts(f):      # LDS instructions per fragment: K one ds_read_b128, V two ds_read_b64_tr_b16
    return 2 if 16 <= f < 32 else 1


def wait_for(f):    # first MFMA of fragment f (f % WGRP == 0): f .. f+WGRP-1 landed = all but the reads of f+WGRP .. f+PF-1 outstanding
    return sum(frag_insts(f + i) for i in range(WGRP, PF))


def gen_iter(j, static=False):
    """iteration t with t = j (mod 4): S'(t) in S_A for even j; K(t+1) in ring buffer (j+1)&3, V(t) in j&3, K(t+2) (its first PF
    fragments are read at the end) in (j+2)&3; DMA targets K(t+3) -> (j+3)&3, V(t+2) -> (j+2)&3"""
    SC, SN = (0, 64) if j % 2 == 0 else (64, 0)
    KB1, KB2, VB = ((j + 1) & 3) * TILE_BYTES, ((j + 2) & 3) * TILE_BYTES, (j & 3) * TILE_BYTES
    KD, VD = LDS_KOFF + ((j + 3) & 3) * TILE_BYTES, LDS_VOFF + ((j + 2) & 3) * TILE_BYTES
    L = []
    A = L.append

    def s_reg(base, qb, kb, r):
        return f"v{base + 16 * (2 * qb + kb) + r}"

    def s_tile(base, qb, kb):
        b = base + 16 * (2 * qb + kb)
        return f"v[{b}:{b + 15}]"

    def ex_reg(e):
        return f"v{V_EX + (e % EXR)}"

    for g in range(64):
        A(f"; ---- gap {g}")
        dma = g < 32 and (g & 3) == DMAPH
        if dma and ((g >> 2) & 3) == 0:      # M0 once per tensor: piece i adds i * 1024 through its immediate offset
            A(f"s_add_u32 m0, %[ldsw], {KD if g < 16 else VD}")
        # ---- MFMA
        if g < 32:
            f, qb = g >> 1, g & 1
            kb, ks = f >> 3, f & 7
            kf, qf = A_KF + 4 * (f % RING), A_Q + 4 * (qb * 8 + ks)
            if qb == 0 and f % WGRP == 0:
                A(f"s_waitcnt lgkmcnt({wait_for(f)})")
            c = f"v[{V_NEGM + 16 * qb}:{V_NEGM + 16 * qb + 15}]" if ks == 0 else s_tile(SN, qb, kb)
            A(f"v_mfma_f32_32x32x16_bf16 {s_tile(SN, qb, kb)}, a[{kf}:{kf + 3}], a[{qf}:{qf + 3}], {c}")
        else:
            j = g - 32
            kk, db, qb, f = j >> 3, (j & 7) >> 1, j & 1, 16 + (j >> 1)
            vf, ot = A_VF + 4 * (f % RING), A_O + 16 * (qb * 4 + db)
            if qb == 0 and f % WGRP == 0:
                A(f"s_waitcnt lgkmcnt({wait_for(f)})")
            pw = V_PW + 4 * (4 * qb + kk)
            A(f"v_mfma_f32_32x32x16_bf16 a[{ot}:{ot + 15}], a[{vf}:{vf + 3}], v[{pw}:{pw + 3}], a[{ot}:{ot + 15}]")
        # ---- barrier: this wave's pieces of K(t+2) / V(t+1) by the counted vmcnt (the 8 youngest = this iteration's), everyone's by the barrier
        if g == 2 * (32 - PF):
            A("s_waitcnt vmcnt(8)")
            A("s_barrier")
        # ---- the gap's fillers, collected by kind and emitted in ORDER (p packs, a adds, r fragment reads, e exponentials, m row max, d DMA)
        packs, adds, reads, exps, maxs, dmas = [], [], [], [], [], []
        # packs and row-sum adds of the exponentials issued LAG gaps ago (the MFMAs in between separate them from their v_exp_f32)
        if g >= LAG:
            for e in range(exps_before(g - LAG), exps_before(g - LAG + 1)):
                kk, qb, j = e >> 4, (e >> 3) & 1, e & 7
                if j & 1:
                    packs.append(f"v_cvt_pk_bf16_f32 v{V_PW + 4 * (4 * qb + kk) + (j >> 1)}, {ex_reg(e - 1)}, {ex_reg(e)}")
            for e in range(exps_before(g - LAG), exps_before(g - LAG + 1)):
                qb = (e >> 3) & 1
                acc = l_reg(qb, e & 1)
                adds.append(f"v_add_f32 v{acc}, v{acc}, {ex_reg(e)}")
        # fragment reads, PF fragments ahead
        if g % 2 == 0:
            f2 = g // 2 + PF
            if f2 < 16 or f2 >= 32:
                fk = f2 if f2 < 16 else f2 - 32
                slot = A_KF + 4 * (f2 % RING)
                ks, kb = fk & 7, fk >> 3
                reads.append(f"ds_read_b128 a[{slot}:{slot + 3}], v{V_VKS + ks} offset:{(KB1 if f2 < 16 else KB2) + kb * 8192}")
            else:
                j2 = f2 - 16
                kk2, db2 = j2 >> 2, j2 & 3
                slot = A_VF + 4 * (f2 % RING)
                reads.append(f"ds_read_b64_tr_b16 a[{slot}:{slot + 1}], v{V_VV + db2} offset:{VB + kk2 * 4096}")
                reads.append(f"ds_read_b64_tr_b16 a[{slot + 2}:{slot + 3}], v{V_VV + db2} offset:{VB + kk2 * 4096 + 2048}")
        # exponentials of P(t)
        for e in range(exps_before(g), exps_before(g + 1)):
            kk, qb, j = e >> 4, (e >> 3) & 1, e & 7
            exps.append(f"v_exp_f32 {ex_reg(e)}, {s_reg(SC, qb, kk >> 1, 8 * (kk & 1) + j)}")
        # row max of S'(t+1): two values per gap, chain-complete order
        if g >= 32 and not static:
            mi = g - 32
            c = mi >> 3
            qb, kb, r = c & 1, c >> 1, 2 * (mi & 7)
            if kb == 0 and r == 0:
                maxs.append(f"v_max_f32 v{V_MX + qb}, {s_reg(SN, qb, kb, r)}, {s_reg(SN, qb, kb, r + 1)}")
            else:
                maxs.append(f"v_max3_f32 v{V_MX + qb}, v{V_MX + qb}, {s_reg(SN, qb, kb, r)}, {s_reg(SN, qb, kb, r + 1)}")
        # ---- DMA piece (K(t+3) at gaps 3..15, V(t+2) at gaps 19..31); M0 was written at the top of the gap
        if dma:
            i = (g >> 2) & 3
            if g < 16:
                dmas.append(f"buffer_load_dwordx4 v{V_KOFF + i}, %[krs], 0 offen{f' offset:{i * 1024}' if i else ''} lds")
            else:
                dmas.append(f"buffer_load_dwordx4 v{V_VOFF + i}, %[vrs], 0 offen{f' offset:{i * 1024}' if i else ''} lds")
        kinds = {"p": packs, "a": adds, "r": reads, "e": exps, "m": maxs, "d": dmas}
        for kind in ORDER:
            L += kinds[kind]
    return L


def emit_fn(name, j, static=False):
    body = gen_iter(j, static)
    SC, SN = (0, 64) if j % 2 == 0 else (64, 0)
    text = "\n".join(f'        "{ln}\\n\\t"' for ln in body)
    sc = "sA" if SC == 0 else "sB"
    sn = "sB" if SC == 0 else "sA"

    def tiles(var, base, pre):
        return ", ".join(f'"{pre}{{v[{base + 16 * (2 * qb + kb)}:{base + 16 * (2 * qb + kb) + 15}]}}"({var}[{qb}][{kb}])' for qb in range(2) for kb in range(2))
    clob = [f'"v{i}"' for i in list(range(V_PW, V_PW + 32)) + list(range(V_EX, V_EX + EXR))]
    mx_arg = "" if static else "float (&mx)[2], "
    mx_out = "" if static else f', "={{v{V_MX}}}"(mx[0]), "={{v{V_MX + 1}}}"(mx[1])'
    kind = "static row bound in -m: no row max of S'(t+1), never a rescale" if static else "online (deferred) running max: row max of S'(t+1) in mx"
    return f'''// iteration t = {j} (mod 4): S'(t) in {sc}, S'(t+1) produced in {sn}; K(t+1) in ring buffer {(j + 1) & 3}, V(t) in {j & 3}; {kind}
__device__ __forceinline__ void {name}(f32x16 (&sA)[2][2], f32x16 (&sB)[2][2], const f32x16 (&negm)[2], float (&l)[2], float (&l2)[2], {mx_arg}
                                       u32x4 vks_lo, u32x4 vks_hi, u32x4 vv, u32x4 koff, u32x4 voff, u32x4 krs, u32x4 vrs, uint32_t ldsw) {{
    asm volatile(
{text}
        : {tiles(sn, SN, "=")}, "+{{v{l_reg(0, 0)}}}"(l[0]), "+{{v{l_reg(1, 0)}}}"(l[1]), "+{{v{l_reg(0, 1)}}}"(l2[0]), "+{{v{l_reg(1, 1)}}}"(l2[1]){mx_out}
        : {tiles(sc, SC, "")}, "{{v[{V_NEGM}:{V_NEGM + 15}]}}"(negm[0]), "{{v[{V_NEGM + 16}:{V_NEGM + 31}]}}"(negm[1]),
          "{{v[{V_VKS}:{V_VKS + 3}]}}"(vks_lo), "{{v[{V_VKS + 4}:{V_VKS + 7}]}}"(vks_hi), "{{v[{V_VV}:{V_VV + 3}]}}"(vv),
          "{{v[{V_KOFF}:{V_KOFF + 3}]}}"(koff), "{{v[{V_VOFF}:{V_VOFF + 3}]}}"(voff), [krs] "s"(krs), [vrs] "s"(vrs), [ldsw] "s"(ldsw)
        : {", ".join(clob)}, "scc", "memory", HV_CLOBBER_ALL_AGPRS);
}}
'''


def main():
    hdr = ("// GENERATED by tools/gen_attn_w4_asm.py - do not edit by hand (tests/test_capi_cpu.py checks it is up to date).\n"
           "// The steady-state iteration of attn_fwd_kernel_w4 as one inline-asm statement per position in the x4 unrolled loop (S-buffer role and\n"
           "// ring buffers are compile-time), in two kinds (online running max / static row bound); register map and schedule:\n"
           "// the generator's docstring and the header of hv_attention_w4.hip.\n")
    body = "\n".join(emit_fn(f"w4_iter_{j}", j) for j in range(4))
    body += "\n" + "\n".join(emit_fn(f"w4_iter_{j}_static", j, True) for j in range(4))
    # the library reports this number (hv_attn_w4_loop_signature): tests compare it with the in-tree file, so a library built from an
    # experiment's iteration (or from a stale one) cannot pass for the product
    import zlib
    sig = zlib.crc32(body.encode()) & 0xFFFFFFFF
    return hdr + f"#define HV_W4_LOOP_SIGNATURE 0x{sig:08x}u\n" + body


if __name__ == "__main__":
    t = main()
    with open(OUT, "w") as f:
        f.write(t)
    print(f"wrote {OUT}: {t.count(chr(10))} lines")
