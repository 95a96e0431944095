// The entropy decoder of include/hv_mjpeg_read.h (stage B) as plain __host__ __device__ functions: table validation, the lookup tables of
// one Huffman table, the bit reader, one restart interval.  csrc/hv_mjpeg_read.hip runs it with one lane per interval;
// tools/mjpeg_decode_fuzz.cpp compiles the same text for the host under sanitizers.  No HIP header is needed here.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HV_HD __host__ __device__
#else
#define HV_HD
#endif

#define HV_MJD_OK 0
#define HV_MJD_NO_BYTES 1
#define HV_MJD_NO_CODE 2
#define HV_MJD_INDEX 3
#define HV_MJD_MARKER 4

constexpr int kMjdLookBits = 9;                 // first-level lookup: codes up to 9 bits
constexpr int kMjdTableBytes = 16 + 256;        // BITS, HUFFVAL

// natural index of every zigzag position (T.81 Figure A.6)
HV_HD inline int hv_mjd_natural(int k) {
    constexpr uint8_t nat[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return nat[k & 63];
}

struct HvHuffTab {
    uint16_t look[1 << kMjdLookBits];           // (length << 8) | symbol of the code the next 9 bits begin with; 0: longer than 9 bits
    int32_t maxcode[17];                        // [l]: the largest code of length l, -1 if there is none
    int32_t valoff[17];                         // [l]: index into val of the first code of length l, minus that code
    uint8_t val[256];
};

// one table (BITS[16], HUFFVAL[256]): at most 256 symbols, code lengths not over-subscribed, symbols inside what a baseline block holds
HV_HD inline bool hv_mjd_table_ok(const uint8_t* t, bool ac) {
    int n = 0;
    uint32_t code = 0;
    for (int l = 1; l <= 16; ++l) {
        n += t[l - 1];
        code += t[l - 1];
        if (code > (1u << l)) return false;
        code <<= 1;
    }
    if (n > 256) return false;
    for (int i = 0; i < n; ++i)
        if (ac ? (t[16 + i] & 15) > 10 : t[16 + i] > 11) return false;
    return true;
}

// the four tables of a scan, DC 0, AC 0, DC 1, AC 1
HV_HD inline bool hv_mjd_tables_ok(const uint8_t* t) {
    for (int i = 0; i < 4; ++i)
        if (!hv_mjd_table_ok(t + i * kMjdTableBytes, (i & 1) != 0)) return false;
    return true;
}

// T.81 Annex C + F.2.2.3 for a table hv_mjd_table_ok accepted
HV_HD inline void hv_mjd_build(const uint8_t* t, HvHuffTab* h) {
    for (int i = 0; i < (1 << kMjdLookBits); ++i) h->look[i] = 0;
    for (int i = 0; i < 256; ++i) h->val[i] = t[16 + i];
    uint32_t code = 0;
    int k = 0;
    h->maxcode[0] = -1, h->valoff[0] = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = t[l - 1];
        h->valoff[l] = k - (int32_t)code;
        if (l <= kMjdLookBits)
            for (int i = 0; i < n; ++i) {
                const uint32_t first = (code + i) << (kMjdLookBits - l);
                for (uint32_t j = 0; j < (1u << (kMjdLookBits - l)); ++j)
                    h->look[(first + j) & ((1u << kMjdLookBits) - 1)] = (uint16_t)((l << 8) | t[16 + ((k + i) & 255)]);
            }
        code += n, k += n;
        h->maxcode[l] = n ? (int32_t)code - 1 : -1;
        code <<= 1;
    }
}

// the bits of data[p .. end): 0xFF 0x00 is the byte 0xFF, any other byte behind 0xFF (or none) ends the data; zeros follow the end.
// Bytes come from memory four at a time (one unaligned 32-bit load while four are left, single bytes for the tail: nothing at or past
// `end` is read) into a small queue, so a lane waits for memory once per four bytes and not once per byte.
struct HvBits {
    const uint8_t* d;
    int64_t p, end;                             // p: the next byte to load
    uint64_t q;                                 // the queue: qn loaded bytes, the next one lowest
    int qn;
    uint64_t acc;                               // the low n bits are unread
    int n, virt;                                // virt: how many of the n bits are zeros from behind the end
    int marker;                                 // 0: data go on; -1: ended at `end` or a lone 0xFF; else the byte behind the 0xFF
};

HV_HD inline void hv_mjd_fill(HvBits& r) {
    while (r.n <= 56) {
        uint32_t b = 0;
        if (r.marker == 0) {
            if (r.qn < 2 && r.p < r.end) {
                if (r.p + 4 <= r.end) {
                    uint32_t v;
                    __builtin_memcpy(&v, r.d + r.p, 4);
                    r.q |= (uint64_t)v << (8 * r.qn);
                    r.qn += 4, r.p += 4;
                } else {
                    for (; r.p < r.end; ++r.p, ++r.qn) r.q |= (uint64_t)r.d[r.p] << (8 * r.qn);
                }
            }
            if (r.qn == 0) {
                r.marker = -1;
            } else {
                b = (uint32_t)(r.q & 0xFFu);
                const uint32_t next = (uint32_t)(r.q >> 8) & 0xFFu;
                if (b != 0xFFu) {
                    r.q >>= 8, r.qn -= 1;
                } else if (r.qn >= 2 && next == 0) {
                    r.q >>= 16, r.qn -= 2;
                } else {
                    r.marker = r.qn >= 2 ? (int)next : -1;
                    b = 0;
                }
            }
        }
        if (r.marker != 0) r.virt += 8;
        r.acc = (r.acc << 8) | b;
        r.n += 8;
    }
}

HV_HD inline uint32_t hv_mjd_peek(const HvBits& r, int k) { return (uint32_t)(r.acc >> (r.n - k)) & ((1u << k) - 1u); }

// T.81 F.2.2.3 DECODE: the next symbol of table h, -1 if no code matches; at least 16 bits are in the reader
HV_HD inline int hv_mjd_symbol(HvBits& r, const HvHuffTab& h) {
    const uint32_t v = hv_mjd_peek(r, 16);
    const uint32_t e = h.look[v >> (16 - kMjdLookBits)];
    if (e) {
        r.n -= (int)(e >> 8);
        return (int)(e & 0xFFu);
    }
    for (int l = kMjdLookBits + 1; l <= 16; ++l) {
        const int32_t code = (int32_t)(v >> (16 - l));
        if (code <= h.maxcode[l]) {
            r.n -= l;
            return h.val[(uint32_t)(h.valoff[l] + code) & 255u];
        }
    }
    return -1;
}

// T.81 F.2.2.1 RECEIVE + EXTEND: a value of s bits, 0 <= s <= 15
HV_HD inline int hv_mjd_value(HvBits& r, int s) {
    if (s == 0) return 0;
    const int v = (int)hv_mjd_peek(r, s);
    r.n -= s;
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

HV_HD inline int hv_mjd_overrun(const HvBits& r, int expect) {
    if (r.n >= r.virt) return HV_MJD_OK;
    return r.marker > 0 && r.marker != expect ? HV_MJD_MARKER : HV_MJD_NO_BYTES;
}

// One restart interval: n_mcus MCUs of 6 blocks from data[begin .. end) into out (n_mcus * 6 * 64 int16, natural order, 16-byte
// aligned), every block stored once and whole through `stage` (64 int16, 16-byte aligned, the caller's scratch).  tabs: DC 0, AC 0, DC 1,
// AC 1.  nat: the 64 entries of hv_mjd_natural where the caller reads them fastest.  expect: the marker byte that may end the data
// (0xD0 + m), 0 for none.  Returns the status of include/hv_mjpeg_read.h.
HV_HD inline int hv_mjd_interval(const uint8_t* data, int64_t begin, int64_t end, int expect, const HvHuffTab* tabs, const uint8_t* nat,
                                 int64_t n_mcus, int16_t* stage, int16_t* out) {
    HvBits r{data, begin, end < begin ? begin : end, 0, 0, 0, 0, 0, 0};
    int status = HV_MJD_OK;
    int pred[3] = {0, 0, 0};
    for (int64_t blk = 0; blk < n_mcus * 6; ++blk) {
        __builtin_memset(__builtin_assume_aligned(stage, 16), 0, 128);
        if (status == HV_MJD_OK) {
            const int b = (int)(blk % 6), comp = b < 4 ? 0 : b - 3;
            const HvHuffTab& dc = tabs[comp ? 2 : 0];
            const HvHuffTab& ac = tabs[comp ? 3 : 1];
            hv_mjd_fill(r);
            const int t = hv_mjd_symbol(r, dc);
            if (t < 0) {
                status = HV_MJD_NO_CODE;
            } else {
                const int diff = hv_mjd_value(r, t & 15);
                status = hv_mjd_overrun(r, expect);
                if (status == HV_MJD_OK) {
                    pred[comp] = (int)(int16_t)(uint16_t)(pred[comp] + diff);
                    stage[0] = (int16_t)pred[comp];
                }
            }
            int k = 1;
            while (status == HV_MJD_OK && k < 64) {
                hv_mjd_fill(r);
                const int rs = hv_mjd_symbol(r, ac);
                if (rs < 0) {
                    status = HV_MJD_NO_CODE;
                    break;
                }
                const int run = rs >> 4, s = rs & 15;
                const int v = hv_mjd_value(r, s);
                status = hv_mjd_overrun(r, expect);
                if (status != HV_MJD_OK) break;
                if (s == 0) {
                    if (run != 15) break;                          // EOB
                    k += 16;                                       // ZRL
                    if (k > 63) status = HV_MJD_INDEX;
                } else {
                    k += run;
                    if (k > 63) {
                        status = HV_MJD_INDEX;
                    } else {
                        stage[nat[k]] = (int16_t)v;
                        ++k;
                    }
                }
            }
        }
        __builtin_memcpy(__builtin_assume_aligned(out + blk * 64, 16), __builtin_assume_aligned(stage, 16), 128);
    }
    return status;
}
