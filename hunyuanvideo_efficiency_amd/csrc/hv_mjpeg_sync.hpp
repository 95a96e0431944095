// The self-synchronising entropy decoder of include/hv_mjpeg_sync.h as plain __host__ __device__ functions on top of
// csrc/hv_mjpeg_decode.hpp (whose tables, symbol decoder and serial interval decoder it uses unchanged): a decoder state, the bit reader
// that also knows its raw position, the guess a lane starts from, and the decode of one subsequence from one entry state.
// csrc/hv_mjpeg_sync.hip runs a lane per thread; tools/mjpeg_sync_check.cpp runs the lanes one after the other on the host under
// sanitizers.  No HIP header is needed here.
#pragma once
#include "hv_mjpeg_decode.hpp"

// between two symbols: pos = raw bit position counted from the interval's begin (-1: dead, see the header), b = block in MCU, k = zigzag
// index of the coefficient the next symbol is about (0: a DC symbol comes next)
struct HvSyncState {
    int64_t pos;
    int32_t b, k;
};

HV_HD inline bool hv_mjs_same(const HvSyncState& x, const HvSyncState& y) { return x.pos == y.pos && x.b == y.b && x.k == y.k; }
HV_HD inline HvSyncState hv_mjs_dead() { return HvSyncState{-1, 0, 0}; }

// HvBits plus one flag per byte of the accumulator (the byte loaded last lowest): it was a 0xFF with a stuffed 0x00 behind it
struct HvSyncBits {
    HvBits r;
    uint32_t stuff;
};

// hv_mjd_fill, which also keeps the flags
HV_HD inline void hv_mjs_fill(HvSyncBits& s) {
    HvBits& r = s.r;
    while (r.n <= 56) {
        uint32_t b = 0, stuffed = 0;
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
                    stuffed = 1;
                } else {
                    r.marker = r.qn >= 2 ? (int)next : -1;
                    b = 0;
                }
            }
        }
        if (r.marker != 0) r.virt += 8;
        r.acc = (r.acc << 8) | b;
        r.n += 8;
        s.stuff = (s.stuff << 1) | stuffed;
    }
}

// the raw bit position of the next unread bit, for a reader that has not overrun (n >= virt): the bytes handed to the accumulator end
// at p - qn; in front of that lie the unread real bits and the stuffing of every byte that still has an unread bit
HV_HD inline int64_t hv_mjs_pos(const HvSyncBits& s) {
    const int real = s.r.n - s.r.virt;
    const int bytes = (real + 7) >> 3;                                             // <= 8
    const uint32_t m = (s.stuff >> (s.r.virt >> 3)) & ((1u << bytes) - 1u);
    return (s.r.p - s.r.qn) * 8 - real - 8 * (int64_t)__builtin_popcount(m);
}

// the state lane j > 0 guesses: the start of its subsequence (byte `at` of d[0 .. len)), a DC symbol of block 0 next
HV_HD inline HvSyncState hv_mjs_guess(const uint8_t* d, int64_t len, int64_t at) {
    if (at >= 1 && at < len && d[at] == 0 && d[at - 1] == 0xFF) ++at;              // stuffing, not data
    return HvSyncState{at * 8, 0, 0};
}

// The symbols of d[0 .. len) that begin in [e.pos, sub_end) (bit positions), decoded from the entry state e.  *exit: the first state
// at or behind sub_end, or dead when a symbol met one of the conditions 1 .. 4 of include/hv_mjpeg_read.h (checked as hv_mjd_interval
// checks them); *blocks: how many blocks were completed before that.  kStore: the coefficients go to out, the block in
// progress at e being `blk`: non-zero coefficients at [block][nat[k]], the DC difference at [block][0], only for blocks below n_blocks
// (the decode ends there).  tabs: DC 0, AC 0, DC 1, AC 1.
template <bool kStore>
HV_HD inline void hv_mjs_lane(const uint8_t* d, int64_t len, const HvHuffTab* tabs, const uint8_t* nat, HvSyncState e, int64_t sub_end,
                              int64_t blk, int64_t n_blocks, int16_t* out, HvSyncState* exit, int32_t* blocks) {
    *blocks = 0;
    *exit = e;
    if (e.pos < 0 || e.pos >= sub_end) return;                                     // e.pos < 0: no caller feeds a dead entry; nothing is decoded
    HvSyncBits s{{d, e.pos >> 3, len, 0, 0, 0, 0, 0, 0}, 0};
    hv_mjs_fill(s);
    s.r.n -= (int)(e.pos & 7);
    int b = e.b, k = e.k & 63;
    int32_t done = 0;
    int64_t pos = e.pos;
    // every symbol uses at least one bit: at most sub_end - e.pos of them begin in front of sub_end
    for (int64_t left = sub_end - e.pos; left > 0 && pos < sub_end; --left) {
        if (kStore && blk >= n_blocks) break;
        bool block_done = false;
        hv_mjs_fill(s);
        if (k == 0) {
            const int t = hv_mjd_symbol(s.r, tabs[b < 4 ? 0 : 2]);
            if (t < 0) pos = -1;
            if (pos >= 0) {
                const int diff = hv_mjd_value(s.r, t & 15);
                if (hv_mjd_overrun(s.r, 0) != HV_MJD_OK) {
                    pos = -1;
                } else {
                    if (kStore && diff != 0) out[blk * 64] = (int16_t)diff;
                    k = 1;
                }
            }
        } else {
            const int rs = hv_mjd_symbol(s.r, tabs[b < 4 ? 1 : 3]);
            if (rs < 0) pos = -1;
            if (pos >= 0) {
                const int run = rs >> 4, sz = rs & 15;
                const int v = hv_mjd_value(s.r, sz);
                if (hv_mjd_overrun(s.r, 0) != HV_MJD_OK) {
                    pos = -1;
                } else if (sz == 0) {
                    if (run != 15) {
                        block_done = true;                                         // EOB
                    } else {
                        k += 16;                                                   // ZRL
                        if (k > 63) pos = -1;
                    }
                } else {
                    k += run;
                    if (k > 63) {
                        pos = -1;
                    } else {
                        if (kStore) out[blk * 64 + nat[k]] = (int16_t)v;
                        ++k;
                        block_done = k == 64;
                    }
                }
            }
        }
        if (pos < 0) break;
        if (block_done) {
            k = 0, b = b == 5 ? 0 : b + 1;
            ++done, ++blk;
        }
        pos = hv_mjs_pos(s);
    }
    *blocks = done;
    *exit = pos < 0 ? hv_mjs_dead() : HvSyncState{pos, b, k};
}

// the block of the unit that holds value i of component comp (0: Y, 1: Cb, 2: Cr) in interval order
HV_HD inline int64_t hv_mjs_dc_block(int comp, int64_t i) { return comp == 0 ? (i >> 2) * 6 + (i & 3) : i * 6 + 3 + comp; }
