"""numpy int64 restatement of the baseline JPEG coder of include/hv_mjpeg.h, written from its statement and from ITU-T T.81 (Annex K
tables, Annex F coding procedures), not from the kernel: the quantiser of frames_uint8, JFIF BT.601 colour in 16 fractional bits, MCU
padding by replication, 4:2:0 chroma from 2 x 2 sums, the integer 8 x 8 DCT, IJG-scaled quantisation tables, the four typical Huffman
tables, one restart interval per MCU row, and the frame around them.  Everything behind the quantiser is integer arithmetic, so the
kernel's bytes must equal these.  `encode` also returns a census of what the entropy coder met."""
import math

import numpy as np
import torch

from tests.yuv_write_ref import quantise

# T.81 Annex K.1 / K.2, in natural (row-major) order
K1 = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
K2 = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
# T.81 Annex K.3 - K.6: (BITS, HUFFVAL) of the DC luminance, DC chrominance, AC luminance and AC chrominance tables
DC_L = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_C = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_L = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
        [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
         0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A,
         0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53,
         0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
         0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5,
         0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9,
         0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2,
         0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])
AC_C = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
        [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
         0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17,
         0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A,
         0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
         0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3,
         0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7,
         0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2,
         0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])


# what Pillow's decode of these bytes may lose against Pillow's own 4:2:0 non-optimised encode at the same quality (tests/test_mjpeg_cpu.py
# test_psnr_and_size_against_pillows_own_encode measures 0.011 dB and 0.8 % at the most and says what the margins cover)
PSNR_MARGIN_DB = 0.05
SIZE_MARGIN = 0.015


def zigzag():
    """natural index of every zigzag position (T.81 Figure A.6), walked along the anti-diagonals"""
    out = []
    for s in range(15):
        ys = range(max(0, s - 7), min(7, s) + 1)
        out += [(y, s - y) for y in (ys if s % 2 else reversed(ys))]
    return [y * 8 + x for y, x in out]


ZIG = zigzag()
M = np.array([[int(round(8192 * (math.sqrt(1 / 8) if u == 0 else 0.5) * math.cos((2 * x + 1) * u * math.pi / 16))) for x in range(8)]
              for u in range(8)], dtype=np.int64)


def quant_tables(quality: int):
    """(luma, chroma) int64 [64] in natural order: Annex K scaled by the IJG quality rule"""
    assert 1 <= quality <= 100
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((np.array(k, dtype=np.int64) * s + 50) // 100, 1, 255) for k in (K1, K2))


def huff_codes(bits, vals, n):
    """T.81 Annex C: symbol -> (code, length), as two int64 arrays of n entries (length 0: no code)"""
    code, length, c, k = np.zeros(n, np.int64), np.zeros(n, np.int64), 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            code[vals[k]], length[vals[k]] = c, l
            c, k = c + 1, k + 1
        c <<= 1
    return code, length


def ycc_planes(q: np.ndarray):
    """q int64 [C, H, W] of bytes -> Y [16 R, 16 M], Cb, Cr [8 R, 8 M] int64 of the padded frame (R MCU rows of M MCUs)"""
    C, H, W = q.shape
    R, Mc = (H + 15) // 16, (W + 15) // 16
    q = np.pad(q, ((0, 0), (0, 16 * R - H), (0, 16 * Mc - W)), mode="edge")
    r, g, b = (q[0], q[0], q[0]) if C == 1 else (q[0], q[1], q[2])
    Y = np.clip((19595 * r + 38470 * g + 7471 * b + 32768) >> 16, 0, 255)
    s = lambda p: p[::2, ::2] + p[::2, 1::2] + p[1::2, ::2] + p[1::2, 1::2]
    rs, gs, bs = s(r), s(g), s(b)
    Cb = np.clip((-11059 * rs - 21709 * gs + 32768 * bs + (128 << 18) + (1 << 17)) >> 18, 0, 255)
    Cr = np.clip((32768 * rs - 27439 * gs - 5329 * bs + (128 << 18) + (1 << 17)) >> 18, 0, 255)
    return Y, Cb, Cr


def fdct(blocks: np.ndarray) -> np.ndarray:
    """samples int64 [N, 8, 8] (0 .. 255) -> r int64 [N, 8, 8] at scale 2^18, r[v][u]: row pass, (t + 128) >> 8, column pass"""
    s = blocks - 128
    t = np.einsum("ux,nyx->nyu", M, s)
    t1 = (t + 128) >> 8
    r = np.einsum("vy,nyu->nvu", M, t1)
    assert np.abs(r).max(initial=0) < 2 ** 31
    return r


def quantise_coefs(r: np.ndarray, Q: np.ndarray) -> np.ndarray:
    """r [N, 8, 8], Q [64] natural -> c [N, 64] natural: sign(r) * ((|r| + (Q << 17)) / (Q << 18))"""
    r = r.reshape(-1, 64)
    return np.sign(r) * ((np.abs(r) + (Q << 17)) // (Q << 18))


def _blocks(plane, n):
    """plane [8 a, 8 b] -> [a, b, 8, 8]"""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def frame_coefs(q: np.ndarray, quality: int) -> np.ndarray:
    """q int64 [C, H, W] bytes -> zigzag coefficients int64 [R, M, 6, 64] in coding order (Y00 Y01 Y10 Y11 Cb Cr of every MCU)"""
    Y, Cb, Cr = ycc_planes(q)
    QL, QC = quant_tables(quality)
    R, Mc = Y.shape[0] // 16, Y.shape[1] // 16
    yb = _blocks(Y, 8).reshape(R, 2, Mc, 2, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(R, Mc, 4, 8, 8)
    out = np.zeros((R, Mc, 6, 64), np.int64)
    out[:, :, :4] = quantise_coefs(fdct(yb.reshape(-1, 8, 8)), QL).reshape(R, Mc, 4, 64)
    out[:, :, 4] = quantise_coefs(fdct(_blocks(Cb, 8).reshape(-1, 8, 8)), QC).reshape(R, Mc, 64)
    out[:, :, 5] = quantise_coefs(fdct(_blocks(Cr, 8).reshape(-1, 8, 8)), QC).reshape(R, Mc, 64)
    return out[..., ZIG]


def _category(v):
    """number of bits of |v| (T.81 F.1.2.1: SSSS)"""
    a = np.abs(v)
    return np.where(a == 0, 0, np.floor(np.log2(np.maximum(a, 1))).astype(np.int64) + 1)


def _value_bits(v, n):
    """the n low bits that follow a code: v for v > 0, v - 1 (two's complement) for v < 0"""
    return np.where(v < 0, v - 1, v) & ((1 << n) - 1)


def new_census():
    return dict(dc_cat=set(), ac_cat=set(), runs=set(), zrl=0, eob=0, last63=0, stuffed=0, pad_bits=set(), rst=set(), rst_wrap=False)


def merge_census(a, b):
    for k, v in b.items():
        if isinstance(v, set):
            a[k] |= v
        elif isinstance(v, bool):
            a[k] = a[k] or v
        else:
            a[k] += v
    return a


def entropy_code(Z: np.ndarray, census=None):
    """Z int64 [R, M, 6, 64] zigzag coefficients of one frame -> list of R byte strings, one per restart interval: stuffed, padded with
    1-bits, followed by RSTm (m = row mod 8) except after the last"""
    census = new_census() if census is None else census
    R, Mc = Z.shape[:2]
    N = R * Mc * 6
    Zf = Z.reshape(N, 64)
    assert np.abs(Zf[:, 1:]).max(initial=0) <= 1023
    k6 = np.arange(N) % 6
    chroma = k6 >= 4
    # DC differences: the predictor is the previous block of the same component in the interval, 0 at its start
    dc = Z[..., 0]                                                  # [R, M, 6]
    diff = np.zeros_like(dc)
    yd = dc[:, :, :4].reshape(R, Mc * 4)
    diff[:, :, :4] = (yd - np.concatenate([np.zeros((R, 1), np.int64), yd[:, :-1]], axis=1)).reshape(R, Mc, 4)
    for c in (4, 5):
        diff[:, :, c] = dc[:, :, c] - np.concatenate([np.zeros((R, 1), np.int64), dc[:, :-1, c]], axis=1)
    diff = diff.reshape(N)
    dcat = _category(diff)
    assert dcat.max(initial=0) <= 11
    tabs = {name: huff_codes(*t, n) for name, t, n in (("dl", DC_L, 12), ("dc", DC_C, 12), ("al", AC_L, 256), ("ac", AC_C, 256))}
    dcode = np.where(chroma, tabs["dc"][0][dcat], tabs["dl"][0][dcat])
    dlen = np.where(chroma, tabs["dc"][1][dcat], tabs["dl"][1][dcat])
    keys = [np.arange(N) * 1024]
    codes = [(dcode << dcat) | _value_bits(diff, dcat)]
    lens = [dlen + dcat]
    # AC: every non-zero coefficient with the run of zeros before it
    b, k = np.nonzero(Zf[:, 1:])
    k = k + 1
    first = np.concatenate([[True], b[1:] != b[:-1]]) if b.size else np.zeros(0, bool)
    prev = np.where(first, 0, np.concatenate([[0], k[:-1]]))
    run = k - prev - 1
    v = Zf[b, k]
    cat = _category(v)
    assert cat.max(initial=0) <= 10
    sym = ((run % 16) << 4) | cat
    ch = chroma[b]
    acode = np.where(ch, tabs["ac"][0][sym], tabs["al"][0][sym])
    alen = np.where(ch, tabs["ac"][1][sym], tabs["al"][1][sym])
    assert (alen > 0).all()
    keys.append(b * 1024 + k * 4 + 3)
    codes.append((acode << cat) | _value_bits(v, cat))
    lens.append(alen + cat)
    for z in (1, 2, 3):                                             # ZRL: one per 16 zeros of a longer run
        m = run // 16 >= z
        keys.append(b[m] * 1024 + k[m] * 4 + (z - 1))
        codes.append(np.where(ch[m], tabs["ac"][0][0xF0], tabs["al"][0][0xF0]))
        lens.append(np.where(ch[m], tabs["ac"][1][0xF0], tabs["al"][1][0xF0]))
        census["zrl"] += int(m.sum())
    last = np.zeros(N, np.int64)
    np.maximum.at(last, b, k)
    eob = np.nonzero(last < 63)[0]
    keys.append(eob * 1024 + 64 * 4)
    codes.append(np.where(chroma[eob], tabs["ac"][0][0], tabs["al"][0][0]))
    lens.append(np.where(chroma[eob], tabs["ac"][1][0], tabs["al"][1][0]))
    census["dc_cat"] |= set(dcat.tolist())
    census["ac_cat"] |= set(cat.tolist())
    census["runs"] |= set((run % 16).tolist())
    census["eob"] += int(eob.size)
    census["last63"] += int((last == 63).sum())
    keys, codes, lens = np.concatenate(keys), np.concatenate(codes), np.concatenate(lens)
    order = np.argsort(keys, kind="stable")
    keys, codes, lens = keys[order], codes[order], lens[order]
    total = int(lens.sum())
    tok = np.repeat(np.arange(lens.size), lens)
    j = np.arange(total) - np.repeat(np.cumsum(lens) - lens, lens)
    bits = ((codes[tok] >> (lens[tok] - 1 - j)) & 1).astype(np.uint8)
    per_block = np.bincount(keys // 1024, weights=lens, minlength=N).astype(np.int64)
    ends = np.cumsum(per_block.reshape(R, Mc * 6).sum(axis=1))
    out = []
    for r in range(R):
        seg = bits[(ends[r - 1] if r else 0):ends[r]]
        pad = (-seg.size) % 8
        census["pad_bits"].add(pad)
        data = np.packbits(np.concatenate([seg, np.ones(pad, np.uint8)]))
        ff = np.nonzero(data == 0xFF)[0]
        census["stuffed"] += int(ff.size)
        data = np.insert(data, ff + 1, 0)
        tail = b""
        if r < R - 1:
            tail = bytes([0xFF, 0xD0 + r % 8])
            census["rst"].add(r % 8)
            census["rst_wrap"] = census["rst_wrap"] or r >= 8
        out.append(data.tobytes() + tail)
    return out


def header(W: int, H: int, quality: int) -> bytes:
    """SOI, APP0 JFIF 1.01, DQT x 2, SOF0, DHT x 4, DRI, SOS"""
    be = lambda v: bytes([v >> 8, v & 0xFF])
    seg = lambda m, body: bytes([0xFF, m]) + be(len(body) + 2) + body
    out = b"\xFF\xD8" + seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i, Q in enumerate(quant_tables(quality)):
        out += seg(0xDB, bytes([i]) + bytes(int(Q[n]) for n in ZIG))
    out += seg(0xC0, bytes([8]) + be(H) + be(W) + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc, (bits, vals) in ((0x00, DC_L), (0x10, AC_L), (0x01, DC_C), (0x11, AC_C)):
        out += seg(0xC4, bytes([tc]) + bytes(bits) + bytes(vals))
    out += seg(0xDD, be((W + 15) // 16))
    return out + seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def encode(x: torch.Tensor, quality: int = 90, rescale: bool = False, census=None):
    """x [C, T, H, W] host tensor -> (intervals: list over frames of lists of byte strings, header bytes, census)"""
    census = new_census() if census is None else census
    q = quantise(x, rescale)
    C, T, H, W = q.shape
    intervals = [entropy_code(frame_coefs(q[:, t], quality), census) for t in range(T)]
    return intervals, header(W, H, quality), census


def frames(x: torch.Tensor, quality: int = 90, rescale: bool = False, census=None):
    """x [C, T, H, W] -> list of T complete JPEG files (bytes)"""
    intervals, head, _ = encode(x, quality, rescale, census)
    return [head + b"".join(iv) + b"\xFF\xD9" for iv in intervals]


# ---- inputs that make the census complete (tests/test_mjpeg_cpu.py asserts it; tests/test_gpu_mjpeg.py codes the same inputs) ----

def idct_block(c: np.ndarray) -> np.ndarray:
    """float64 inverse DCT of natural-order coefficients [8, 8] (unquantised scale) -> samples, 128 added, not clamped"""
    A = np.array([[(math.sqrt(1 / 8) if u == 0 else 0.5) * math.cos((2 * x + 1) * u * math.pi / 16) for x in range(8)] for u in range(8)])
    return A.T @ c @ A + 128


def census_inputs():
    """name -> (x [C, T, H, W] fp32 in [0, 1], quality).  Sizes stay small: the GPU tests code every one through two routes."""
    g = torch.Generator().manual_seed(1234)
    out = {}
    out["noise_q100"] = (torch.rand(3, 1, 40, 56, generator=g), 100)
    out["constant"] = (torch.full((3, 2, 16, 160), 0.5), 90)                   # all-zero differences, EOB only
    tall = torch.rand(1, 1, 160, 16, generator=g)                             # 16 x 160: ten MCU rows, RST0 .. RST7 and RST0 again
    out["tall_noise"] = (tall, 75)
    # gray blocks that hold one coefficient each at zigzag position p (p = 1 .. 63) with an amplitude that lands in a chosen category:
    # the run before it is p - 1 (ZRL for p > 16), p = 63 ends the block without an EOB
    Hs, Ws = 64, 128
    img = np.full((Hs, Ws), 128.0)
    n = 0
    for by in range(Hs // 8):
        for bx in range(Ws // 8):
            p = 1 + n % 63
            c = np.zeros(64)
            amp = (3.0, 9.0, 30.0, 90.0, 200.0, 420.0)[n % 6] * (1 if n % 2 else -1)
            c[ZIG[p]] = amp
            if n % 5 == 0 and p + 17 <= 63:
                c[ZIG[p + 17]] = 40.0                                         # a second coefficient after a run of 16: one ZRL + run 0
            img[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = idct_block(c.reshape(8, 8))
            n += 1
    gray = torch.from_numpy(np.clip(np.round(img), 0, 255) / 255.0 + 0.001).float()
    out["single_coefficients"] = (gray[None, None], 100)
    # adjacent 8 x 8 blocks swinging between 0 and 255 (DC differences of category 11), and checkerboards inside blocks (AC category 10)
    sw = torch.zeros(1, 1, 32, 64)
    for by in range(4):
        for bx in range(8):
            sw[0, 0, by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = float((by + bx) % 2)
    yy, xx = torch.meshgrid(torch.arange(32), torch.arange(64), indexing="ij")
    ck = ((yy + xx) % 2).float()
    stripes_h = (xx % 2).float()
    stripes_v = (yy % 2).float()
    half = ((xx % 8) < 4).float()
    out["swing"] = (torch.cat([sw, ck[None, None], stripes_h[None, None], stripes_v[None, None], half[None, None]], dim=1), 100)
    # ramps of DC steps: every DC category 0 .. 11 in both directions
    steps = [0, 0, 1, 3, 6, 12, 24, 48, 96, 160, 255, 0, 255, 128, 127, 125, 121, 113, 97, 65, 1, 255, 2, 0]
    ramp = torch.zeros(1, 1, 16, 8 * len(steps))
    for i, s in enumerate(steps):
        ramp[0, 0, :, 8 * i:8 * i + 8] = (s + 0.5) / 255.0
    out["dc_steps"] = (ramp, 100)
    # a stream rich in 1-bits: stuffed bytes
    out["noise_q100_gray"] = (torch.rand(1, 2, 24, 24, generator=g), 100)
    return out


def census_complete(c):
    """the list of census conditions of the issue that `c` does not meet (empty: complete)"""
    miss = []
    if not set(range(12)) <= c["dc_cat"]:
        miss.append(("dc_cat", sorted(set(range(12)) - c["dc_cat"])))
    if not set(range(1, 11)) <= c["ac_cat"]:
        miss.append(("ac_cat", sorted(set(range(1, 11)) - c["ac_cat"])))
    if not set(range(16)) <= c["runs"]:
        miss.append(("runs", sorted(set(range(16)) - c["runs"])))
    for k in ("zrl", "eob", "last63", "stuffed"):
        if c[k] < 1:
            miss.append((k, c[k]))
    if not set(range(8)) <= c["pad_bits"]:
        miss.append(("pad_bits", sorted(set(range(8)) - c["pad_bits"])))
    if not set(range(8)) <= c["rst"] or not c["rst_wrap"]:
        miss.append(("rst", sorted(c["rst"]), c["rst_wrap"]))
    return miss
