"""numpy / plain Python restatement of the baseline JPEG decoder of include/hv_mjpeg_read.h, written from its statement and from ITU-T
T.81 (B.2 segment syntax, Annex C code assignment, F.2.2 decoding procedures), not from the kernel: the frame parser, restart-marker
search, a table-driven Huffman decoder for arbitrary DHT tables working on a list of bits, the status rules, then dequantisation, the
two-pass integer inverse DCT, the triangle chroma filter on the real chroma plane, and JFIF colour.  Everything is integer arithmetic,
so the kernel's bytes must equal these, and tests/test_mjpeg_read_cpu.py holds these against Pillow's decode byte for byte.  `decode`
also fills a census of what the decoder met."""
import numpy as np

from tests.mjpeg_ref import AC_C, AC_L, DC_C, DC_L, ZIG

OK, NO_BYTES, NO_CODE, INDEX, MARKER = 0, 1, 2, 3, 4
RST_ORDER = 1 << 30
ANNEX_K = (DC_L, AC_L, DC_C, AC_C)                 # the order of the header: DC 0, AC 0, DC 1, AC 1
LOOK_BITS = 9


def new_census():
    return dict(dc_cat=set(), ac_cat=set(), runs=set(), zrl=0, eob=0, last63=0, stuffed=0, pad_bits=set(), rst=set(), rst_wrap=False,
                code_paths=set(), upsample=set(), edges=set(), clamps=set())


def census_complete(c):
    """the conditions of the census that `c` does not meet (empty: complete)"""
    miss = []
    for key, want in (("dc_cat", set(range(12))), ("ac_cat", set(range(1, 11))), ("runs", set(range(16))), ("pad_bits", set(range(8))),
                      ("rst", set(range(8))), ("code_paths", {"lookup", "long"}), ("upsample", {"repeat", "filter"}),
                      ("edges", {(e, p) for e in ("top", "bottom", "left", "right") for p in (0, 1)}),
                      ("clamps", {(ch, end) for ch in "RGB" for end in ("low", "high")})):
        if not want <= c[key]:
            miss.append((key, sorted(want - c[key])))
    for k in ("zrl", "eob", "last63", "stuffed"):
        if c[k] < 1:
            miss.append((k, c[k]))
    if not c["rst_wrap"]:
        miss.append(("rst_wrap", False))
    return miss


# ------------------------------------------------------------------------------------------------ the frame (T.81 Annex B)

class Refused(ValueError):
    pass


def parse(d: bytes):
    """-> dict(W, H, quant (Y, chroma) int64 [64] natural, huff [(BITS, HUFFVAL)] x 4, Ri, begin, end); Refused outside the scope"""
    assert d[:2] == b"\xFF\xD8"
    qt, ht, sof, Ri, pos = {}, {}, None, 0, 2
    while True:
        assert d[pos] == 0xFF
        while d[pos] == 0xFF:
            pos += 1
        m = d[pos]
        pos += 1
        if m in (0xD8, 0x01) or 0xD0 <= m <= 0xD7:
            continue
        L = d[pos] * 256 + d[pos + 1]
        body, pos = d[pos + 2:pos + L], pos + L
        if 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8):
            raise Refused(f"marker {m:02X}")
        if m == 0xDC:
            raise Refused("DNL")
        if m == 0xDB:
            while body:
                if body[0] >> 4:
                    raise Refused("16-bit DQT")
                q = np.zeros(64, np.int64)
                q[ZIG] = list(body[1:65])
                qt[body[0] & 15], body = q, body[65:]
        elif m == 0xC4:
            while body:
                bits = list(body[1:17])
                ht[(body[0] >> 4, body[0] & 15)] = (bits, list(body[17:17 + sum(bits)]))
                body = body[17 + sum(bits):]
        elif m == 0xDD:
            Ri = body[0] * 256 + body[1]
        elif m == 0xC0:
            if body[0] != 8:
                raise Refused("precision")
            H, W, nc = body[1] * 256 + body[2], body[3] * 256 + body[4], body[5]
            comps = [tuple(body[6 + 3 * c:9 + 3 * c]) for c in range(nc)]
            if nc != 3 or [c[1] for c in comps] != [0x22, 0x11, 0x11] or comps[1][2] != comps[2][2]:
                raise Refused("components")
            sof = (W, H, comps)
        elif m == 0xDA:
            W, H, comps = sof
            if body[0] != 3 or tuple(body[7:10]) != (0, 63, 0) or body[4] != body[6]:
                raise Refused("scan")
            huff = []
            for t in (body[2], body[4]):
                for key in ((0, t >> 4), (1, t & 15)):
                    huff.append(ht[key] if ht else ANNEX_K[2 * key[1] + key[0]])
            end = pos
            while end < len(d) and not (d[end] == 0xFF and end + 1 < len(d) and d[end + 1] not in (0, 0xFF) and not 0xD0 <= d[end + 1] <= 0xD7):
                end += 1
            if end + 1 < len(d) and d[end + 1] != 0xD9:
                raise Refused(f"marker {d[end + 1]:02X} behind the scan")
            return dict(W=W, H=H, quant=(qt[comps[0][2]], qt[comps[1][2]]), huff=huff, Ri=Ri, begin=pos, end=end)


def geometry(W, H, Ri):
    """(mcus, mcu_rows, mpf, ipf)"""
    mcus, rows = (W + 15) // 16, (H + 15) // 16
    mpf = mcus * rows
    return mcus, rows, mpf, 1 if Ri == 0 else (mpf + Ri - 1) // Ri


def huff_bytes(huff):
    """the 1088 table bytes of hv_mjpeg_decode_coefs"""
    out = []
    for bits, vals in huff:
        out += list(bits) + list(vals) + [0] * (256 - len(vals))
    return out


def table_ok(bits, vals, ac):
    """the refusals of the header: more than 256 symbols, over-subscribed lengths, a DC symbol above 11, an AC size above 10"""
    code = 0
    for l in range(1, 17):
        code += bits[l - 1]
        if code > (1 << l):
            return False
        code <<= 1
    n = sum(bits)
    return n <= 256 and all((v & 15) <= 10 if ac else v <= 11 for v in vals[:n])


# ------------------------------------------------------------------------------------------------ stage A

def find_restarts(d: bytes, begin: int, end: int, ipf: int):
    """-> (interval_begin [ipf], interval_end [ipf], found word)"""
    marks = [j for j in range(begin, end - 1) if d[j] == 0xFF and 0xD0 <= d[j + 1] <= 0xD7]
    ib, ie = [begin] + [end] * (ipf - 1), [end] * ipf
    bad = False
    for j, p in enumerate(marks[:ipf - 1]):
        ie[j], ib[j + 1] = p, p + 2
        bad = bad or d[p + 1] != 0xD0 + j % 8
    return ib, ie, len(marks) | (RST_ORDER if bad else 0)


# ------------------------------------------------------------------------------------------------ stage B (T.81 F.2.2)

def code_book(bits, vals):
    """Annex C: {(length, code): symbol}"""
    book, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            book[(l, code)] = vals[k]
            code, k = code + 1, k + 1
        code <<= 1
    return book


class Bits:
    """the bits of d[begin:end) up to the first 0xFF not followed by 0x00, stuffing removed; zeros behind them"""

    def __init__(self, d, begin, end, census):
        raw, p, self.marker = bytearray(), begin, -1
        while p < end:
            if d[p] != 0xFF:
                raw.append(d[p])
                p += 1
            elif p + 1 < end and d[p + 1] == 0:
                raw.append(0xFF)
                p += 2
                census["stuffed"] += 1
            else:
                self.marker = d[p + 1] if p + 1 < end else -1
                break
        self.bits = np.unpackbits(np.frombuffer(bytes(raw), np.uint8)).tolist()
        self.pos = 0

    def take(self, n):
        v = 0
        for i in range(self.pos, self.pos + n):
            v = v * 2 + (self.bits[i] if i < len(self.bits) else 0)
        self.pos += n
        return v

    def over(self):
        return self.pos > len(self.bits)


def decode_interval(d, begin, end, expect, huff, n_mcus, census=None):
    """-> (coefficients int16 [n_mcus, 6, 64] natural order, status).  expect: the marker byte that may end the data, 0 for none."""
    census = new_census() if census is None else census
    books = [code_book(*h) for h in huff]
    out = np.zeros((n_mcus, 6, 64), np.int16)
    r = Bits(d, max(begin, 0), max(end, begin, 0), census)
    fail = lambda: MARKER if r.marker > 0 and r.marker != expect else NO_BYTES

    def symbol(book):
        code = 0
        for l in range(1, 17):
            code = code * 2 + r.take(1)
            if (l, code) in book:
                census["code_paths"].add("lookup" if l <= LOOK_BITS else "long")
                return book[(l, code)]
        return None

    def value(s):
        v = r.take(s)
        return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v

    pred = [0, 0, 0]
    for m in range(n_mcus):
        for b in range(6):
            comp = 0 if b < 4 else b - 3
            t = symbol(books[2 if comp else 0])
            if t is None:
                return out, NO_CODE
            diff = value(t)
            if r.over():
                return out, fail()
            census["dc_cat"].add(t)
            pred[comp] = (pred[comp] + diff + 32768) % 65536 - 32768
            out[m, b, 0] = pred[comp]
            k = 1
            while k < 64:
                rs = symbol(books[3 if comp else 1])
                if rs is None:
                    return out, NO_CODE
                run, s = rs >> 4, rs & 15
                v = value(s)
                if r.over():
                    return out, fail()
                if s == 0:
                    if run != 15:
                        census["eob"] += 1
                        break
                    census["zrl"] += 1
                    k += 16
                    if k > 63:
                        return out, INDEX
                else:
                    k += run
                    if k > 63:
                        return out, INDEX
                    out[m, b, ZIG[k]] = v
                    census["ac_cat"].add(s)
                    census["runs"].add(run)
                    k += 1
                    if k == 64:
                        census["last63"] += 1
    left = len(r.bits) - r.pos
    if left < 8:
        census["pad_bits"].add(left)
    return out, OK


def decode_coefs(d: bytes, p, census=None, intervals=None):
    """one frame -> (coefs int16 [mcu_rows, mcus, 6, 64], status [ipf], found word).  intervals: (begin list, end list) to use instead
    of the restart search (the coder's own offsets, which include each RSTm in its interval)."""
    census = new_census() if census is None else census
    mcus, rows, mpf, ipf = geometry(p["W"], p["H"], p["Ri"])
    if intervals is None:
        ib, ie, found = find_restarts(d, p["begin"], p["end"], ipf)
    else:
        (ib, ie), found = intervals, ipf - 1
    coefs, status = np.zeros((mpf, 6, 64), np.int16), []
    for k in range(ipf):
        m0 = k * p["Ri"]
        n = mpf - m0 if p["Ri"] == 0 else min(p["Ri"], mpf - m0)
        expect = 0xD0 + k % 8 if k < ipf - 1 else 0
        coefs[m0:m0 + n], st = decode_interval(d, ib[k], ie[k], expect, p["huff"], n, census)
        status.append(st)
        if k < ipf - 1 and k < (found & (RST_ORDER - 1)):
            census["rst"].add(k % 8)
            census["rst_wrap"] = census["rst_wrap"] or k >= 8
    return coefs.reshape(rows, mcus, 6, 64), status, found


# ------------------------------------------------------------------------------------------------ stage C

def idct_1d(d):
    """the 1-D pass of the header on axis 0 of d [8, ...] int64 -> y [8, ...], unscaled"""
    z1 = (d[2] + d[6]) * 4433
    t2, t3 = z1 - d[6] * 15137, z1 + d[2] * 6270
    t0, t1 = (d[0] + d[4]) << 13, (d[0] - d[4]) << 13
    e0, e3, e1, e2 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    z1, z2, z3, z4 = d[7] + d[1], d[5] + d[3], d[7] + d[3], d[5] + d[1]
    z5 = (z3 + z4) * 9633
    o0, o1, o2, o3 = d[7] * 2446, d[5] * 16819, d[3] * 25172, d[1] * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    return np.stack([e0 + o3, e1 + o2, e2 + o1, e3 + o0, e3 - o0, e2 - o1, e1 - o2, e0 - o3])


def samples(blocks, Q):
    """quantised blocks int [N, 64] natural, Q [64] -> (bytes [N, 8, 8], whether every sample stayed where clamping and the wrap-around
    range table of libjpeg agree: |sample - 128| < 384)"""
    d = (blocks.astype(np.int64) * Q).reshape(-1, 8, 8)
    w = (idct_1d(d.transpose(1, 0, 2)) + (1 << 10)) >> 11                     # down the columns: axis 0 = row index
    y = (idct_1d(w.transpose(2, 1, 0)) + (1 << 17)) >> 18                      # along the rows: axis 0 = column index -> [x, N, y]
    s = y.transpose(1, 2, 0) + 128
    return np.clip(s, 0, 255), bool((np.abs(s - 128) < 384).all())


def planes(coefs, quant, W, H):
    """coefs [rows, mcus, 6, 64] -> Y [H, W], Cb, Cr [ch, cw] (the real planes), in-range flag"""
    rows, mcus = coefs.shape[:2]
    yb, ok1 = samples(coefs[:, :, :4].reshape(-1, 64), quant[0])
    Y = yb.reshape(rows, mcus, 2, 2, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(rows * 16, mcus * 16)
    out, ok = [Y[:H, :W]], ok1
    for c in (4, 5):
        cb, okc = samples(coefs[:, :, c].reshape(-1, 64), quant[1])
        ok = ok and okc
        out.append(cb.reshape(rows, mcus, 8, 8).transpose(0, 2, 1, 3).reshape(rows * 8, mcus * 8)[:(H + 1) // 2, :(W + 1) // 2])
    return out[0], out[1], out[2], ok


def upsample(p, W, H, census):
    """chroma plane [ch, cw] -> [H, W]"""
    ch, cw = p.shape
    if cw <= 2:
        census["upsample"].add("repeat")
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)[:H, :W]
    census["upsample"].add("filter")
    for e, par in (("top", H % 2), ("bottom", H % 2), ("left", W % 2), ("right", W % 2)):
        census["edges"].add((e, par))
    up, down = np.concatenate([p[:1], p[:-1]]), np.concatenate([p[1:], p[-1:]])
    s = np.empty((2 * ch, cw), np.int64)
    s[0::2], s[1::2] = 3 * p + up, 3 * p + down
    left, right = np.concatenate([s[:, :1], s[:, :-1]], axis=1), np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    out = np.empty((2 * ch, 2 * cw), np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * s + left + 8) >> 4, (3 * s + right + 7) >> 4
    return out[:H, :W]


def pixels(coefs, quant, W, H, census=None):
    """-> (uint8 [H, W, 3] R G B, in-range flag)"""
    census = new_census() if census is None else census
    Y, Cb, Cr, ok = planes(coefs, quant, W, H)
    cb, cr = upsample(Cb, W, H, census) - 128, upsample(Cr, W, H, census) - 128
    rgb = [Y + ((91881 * cr + 32768) >> 16), Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), Y + ((116130 * cb + 32768) >> 16)]
    for name, v in zip("RGB", rgb):
        if (v < 0).any():
            census["clamps"].add((name, "low"))
        if (v > 255).any():
            census["clamps"].add((name, "high"))
    return np.clip(np.stack(rgb, axis=-1), 0, 255).astype(np.uint8), ok


def decode(d: bytes, census=None):
    """a whole JPEG file -> (uint8 [H, W, 3], status list, found word, in-range flag)"""
    p = parse(d)
    coefs, status, found = decode_coefs(d, p, census)
    img, ok = pixels(coefs, p["quant"], p["W"], p["H"], census)
    return img, status, found, ok


def decode_clip(frames, census=None):
    """list of JPEG files of one size -> uint8 [3, T, H, W], asserting that every one decodes cleanly"""
    out = []
    for d in frames:
        img, status, found, _ = decode(d, census)
        p = parse(d)
        assert not any(status) and found == geometry(p["W"], p["H"], p["Ri"])[3] - 1, (status, found)
        out.append(img)
    return np.stack(out).transpose(3, 0, 1, 2)
