// Host check program of the self-synchronising entropy decoder csrc/hv_mjpeg_sync.hpp: the text the GPU kernel compiles
// (csrc/hv_mjpeg_sync.hip), here for the CPU under -fsanitize=address,undefined, with its own main and nothing preloaded.  It runs the
// lanes of a workgroup one after the other in lane order, with the rounds and iterations of the kernel, and compares the coefficients and
// the status of every restart interval with the serial decoder hv_mjd_interval, each side against heap buffers of exactly the size the
// contract names (the interval's bytes, its n_mcus * 768 bytes of coefficients, 128 bytes of staging).  Inputs: every JPEG file on the
// command line at sub_bytes 16 .. 64, 128, 1024 and 4096 (files with restart markers a second time with every RSTm inside its interval,
// as the package's own coder hands them over), then mutations of each from a fixed seed at sub_bytes 16 and 128 (bit flips, truncations,
// all-ones, all-zeros, random bytes, random tails, markers, changed tables).  Exit 0 only if nothing differs; a sanitizer report aborts
// with its own exit code.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I hunyuanvideo_efficiency_amd/csrc -I include \
//       tools/mjpeg_sync_check.cpp -o /tmp/mjpeg_sync_check && /tmp/mjpeg_sync_check tests/golden/mjpeg_read/*.jpg tests/golden/mjpeg_sync/*.jpg
// Options: --mutations=N per file and sub_bytes (default 400); --dump=DIR writes <file name>.coefs (int16, the frame's workspace) and
// <file name>.status (one number per line) of every unmutated file at --dump-sub=S (default 16); every unmutated run prints one `census`
// line, which tests/test_mjpeg_sync_cpu.py reads.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hv_mjpeg_sync.hpp"
#include "hv_mjpeg_sync.h"

namespace {

constexpr int kLanes = HV_MJPEG_SYNC_LANES;

struct Frame {
    int W = 0, H = 0, Ri = 0;
    uint8_t huff[4 * kMjdTableBytes] = {};
    bool have_huff = false;
    size_t begin = 0, end = 0;
};

// the headers of a baseline 4:2:0 file the fixtures' makers wrote (no refusals here: mjpeg_io.parse_jpeg owns those)
bool parse(const std::vector<uint8_t>& d, Frame& f) {
    uint8_t dht[2][4][kMjdTableBytes] = {};
    int td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
    size_t pos = 2;
    while (pos + 4 <= d.size()) {
        if (d[pos] != 0xFF) return false;
        const int m = d[pos + 1];
        const size_t L = (size_t)d[pos + 2] * 256 + d[pos + 3];
        if (L < 2 || pos + 2 + L > d.size()) return false;
        const uint8_t* b = &d[pos + 4];
        const size_t n = L - 2;
        if (m == 0xC0 && n >= 6) {
            f.H = b[1] * 256 + b[2], f.W = b[3] * 256 + b[4];
        } else if (m == 0xDD && n == 2) {
            f.Ri = b[0] * 256 + b[1];
        } else if (m == 0xC4) {
            size_t i = 0;
            while (i + 17 <= n) {
                int cnt = 0;
                for (int k = 0; k < 16; ++k) cnt += b[i + 1 + k];
                if (cnt > 256 || i + 17 + cnt > n || (b[i] >> 4) > 1 || (b[i] & 15) > 3) return false;
                uint8_t* t = dht[b[i] >> 4][b[i] & 15];
                memset(t, 0, kMjdTableBytes);
                memcpy(t, b + i + 1, 16);
                memcpy(t + 16, b + i + 17, cnt);
                f.have_huff = true;
                i += 17 + cnt;
            }
        } else if (m == 0xDA && n >= 10) {
            for (int c = 0; c < 3; ++c) td[c] = b[2 + 2 * c] >> 4, ta[c] = b[2 + 2 * c] & 15;
            memcpy(f.huff + 0 * kMjdTableBytes, dht[0][td[0] & 3], kMjdTableBytes);
            memcpy(f.huff + 1 * kMjdTableBytes, dht[1][ta[0] & 3], kMjdTableBytes);
            memcpy(f.huff + 2 * kMjdTableBytes, dht[0][td[1] & 3], kMjdTableBytes);
            memcpy(f.huff + 3 * kMjdTableBytes, dht[1][ta[1] & 3], kMjdTableBytes);
            f.begin = pos + 2 + L;
            f.end = d.size() >= 2 ? d.size() - 2 : d.size();                       // EOI
            return f.W > 0 && f.H > 0 && f.have_huff && f.begin <= f.end;
        }
        pos += 2 + L;
    }
    return false;
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

// what the algorithm distinguishes, over the units of one run
struct Census {
    long units = 0, fallback = 0, straddle = 0, value_cross = 0, rst_end = 0, short_units = 0;
    long span = 0, blocks = 0, code = 0, rounds = 0, iters = 0;                     // maxima
    void add(const Census& c) {
        units += c.units, fallback += c.fallback, straddle += c.straddle, value_cross += c.value_cross, rst_end += c.rst_end;
        short_units += c.short_units;
        span = c.span > span ? c.span : span, blocks = c.blocks > blocks ? c.blocks : blocks, code = c.code > code ? c.code : code;
        rounds = c.rounds > rounds ? c.rounds : rounds, iters = c.iters > iters ? c.iters : iters;
    }
};

long g_units = 0, g_status[5] = {0, 0, 0, 0, 0};
Census g_all;

// the symbols of a clean unit, one reader from its begin: value bits across an edge, the subsequences of a block, the longest code
void walk(const uint8_t* d, int64_t len, const HvHuffTab* tabs, int64_t n_blocks, int sub, Census& c) {
    HvSyncBits s{{d, 0, len, 0, 0, 0, 0, 0, 0}, 0};
    const int64_t edge = (int64_t)sub * 8;
    int b = 0, k = 0;
    int64_t first_sub = 0;
    for (int64_t blk = 0; blk < n_blocks;) {
        hv_mjs_fill(s);
        const int64_t p0 = hv_mjs_pos(s);
        if (k == 0) first_sub = p0 / edge;
        const int n0 = s.r.n;
        const int sym = hv_mjd_symbol(s.r, tabs[(b < 4 ? 0 : 2) + (k ? 1 : 0)]);
        if (sym < 0) return;
        if (n0 - s.r.n > c.code) c.code = n0 - s.r.n;
        if (hv_mjd_overrun(s.r, 0) != HV_MJD_OK) return;
        const int64_t p1 = hv_mjs_pos(s);
        const int sz = sym & 15;
        hv_mjd_value(s.r, sz);
        if (hv_mjd_overrun(s.r, 0) != HV_MJD_OK) return;
        if (sz > 0 && p1 / edge != (p1 + sz - 1) / edge) ++c.value_cross;          // stuffing only moves the last bit further
        bool done = false;
        if (k == 0) {
            k = 1;
        } else if (sz == 0) {
            if ((sym >> 4) != 15) done = true;
            else k += 16;
        } else {
            k += (sym >> 4) + 1;
            done = k == 64;
        }
        if (k > 64) return;
        if (done) {
            if (p0 / edge - first_sub + 1 > c.span) c.span = p0 / edge - first_sub + 1;
            k = 0, b = b == 5 ? 0 : b + 1, ++blk;
        }
    }
}

// One unit as a workgroup decodes it, the lanes one after the other: data[0 .. len) (a heap copy of exactly the interval), n MCUs into
// out (n * 768 bytes).  Returns the status; *iters as the kernel reports it.
int sync_unit(const uint8_t* d, int64_t len, int expect, const HvHuffTab* tabs, const uint8_t* nat, int64_t n, int sub, int16_t* out,
              int32_t* iters, Census& c) {
    const int64_t n_blocks = n * 6;
    memset(out, 0, (size_t)n * 768);
    const int64_t subs = (len + sub - 1) / sub, rounds = (subs + kLanes - 1) / kLanes;
    HvSyncState entry{0, 0, 0};
    int64_t total = 0;
    int its = 0;
    std::vector<HvSyncState> used(kLanes), exits(kLanes), e(kLanes);
    std::vector<int32_t> cnt(kLanes);
    std::vector<char> changed(kLanes);
    if (rounds > c.rounds) c.rounds = rounds;
    if (len < sub) ++c.short_units;
    for (int64_t j = sub; j < len; j += sub) c.straddle += d[j] == 0 && d[j - 1] == 0xFF;
    for (int64_t r = 0; r < rounds && entry.pos >= 0 && total < n_blocks; ++r) {
        auto sub_begin = [&](int j) { return r * kLanes + j < subs ? (r * kLanes + j) * sub : len; };
        auto sub_end = [&](int j) { return (len - sub_begin(j) < sub ? len : sub_begin(j) + sub) * 8; };
        for (int j = 0; j < kLanes; ++j) used[j] = HvSyncState{-2, 0, 0}, exits[j] = hv_mjs_dead(), cnt[j] = 0;
        int round_its = 0;
        for (int it = 0; it < kLanes + 1; ++it) {
            bool any = false;
            for (int j = 0; j < kLanes; ++j) {                                     // every exit is read before one is replaced
                e[j] = j == 0 ? entry : it == 0 ? hv_mjs_guess(d, len, sub_begin(j)) : exits[j - 1];
                if (e[j].pos < 0) e[j] = used[j];                                  // a dead exit says nothing: the entry in use stands
                changed[j] = r * kLanes + j < subs && !hv_mjs_same(e[j], used[j]);
            }
            for (int j = 0; j < kLanes; ++j)
                if (changed[j]) {
                    used[j] = e[j];
                    hv_mjs_lane<false>(d, len, tabs, nat, e[j], sub_end(j), 0, 0, nullptr, &exits[j], &cnt[j]);
                    any = true;
                }
            if (!any) break;
            ++its, ++round_its;
        }
        if (round_its > c.iters) c.iters = round_its;
        // the lanes up to the first dead exit are exact, the ones behind it kept entries that mean nothing
        int64_t first = total;
        const int64_t in_round = subs - r * kLanes < kLanes ? subs - r * kLanes : kLanes;
        entry = exits[in_round - 1];
        for (int j = 0; j < in_round; ++j) {
            HvSyncState ex;
            int32_t again;
            hv_mjs_lane<true>(d, len, tabs, nat, used[j], sub_end(j), first, n_blocks, out, &ex, &again);
            if (cnt[j] > c.blocks) c.blocks = cnt[j];
            first += cnt[j];
            if (exits[j].pos < 0) {
                entry = hv_mjs_dead();
                break;
            }
        }
        total = first;
    }
    if (total >= n_blocks) {
        for (int comp = 0; comp < 3; ++comp) {
            int carry = 0;
            for (int64_t i = 0; i < (comp == 0 ? n * 4 : n); ++i) {
                int16_t* p = out + hv_mjs_dc_block(comp, i) * 64;
                carry = (int)(int16_t)(uint16_t)(carry + *p);
                *p = (int16_t)carry;
            }
        }
        *iters = its;
        walk(d, len, tabs, n_blocks, sub, c);
        return HV_MJD_OK;
    }
    int16_t* stage = (int16_t*)aligned_alloc(16, 128);
    const int st = hv_mjd_interval(d, 0, len, expect, tabs, nat, n, stage, out);
    free(stage);
    *iters = -1;
    ++c.fallback;
    return st;
}

// every interval of one frame, both decoders, each against exactly sized heap buffers; false if they differ.  include_rst: every RSTm
// lies inside the interval it ends.  frame_coefs / frame_status (may be null) receive the sync decoder's result.
bool check_frame(const Frame& f, const uint8_t* scan, size_t scan_bytes, const uint8_t* huff, int sub, bool include_rst, Census& c,
                 std::vector<int16_t>* frame_coefs, std::vector<int>* frame_status) {
    if (!hv_mjd_tables_ok(huff)) return true;                                     // the entry point refuses: nothing is decoded
    HvHuffTab* tabs = (HvHuffTab*)malloc(4 * sizeof(HvHuffTab));
    for (int i = 0; i < 4; ++i) hv_mjd_build(huff + i * kMjdTableBytes, &tabs[i]);
    const int64_t mpf = (int64_t)((f.W + 15) / 16) * ((f.H + 15) / 16);
    const int64_t ipf = f.Ri == 0 ? 1 : (mpf + f.Ri - 1) / f.Ri;
    std::vector<size_t> ib(ipf, scan_bytes), ie(ipf, scan_bytes);
    ib[0] = 0;
    int64_t k = 0;
    for (size_t j = 0; j + 1 < scan_bytes && k < ipf - 1; ++j)
        if (scan[j] == 0xFF && (scan[j + 1] & 0xF8) == 0xD0) ie[k] = include_rst ? j + 2 : j, ib[k + 1] = j + 2, ++k;
    uint8_t nat[64];
    for (int i = 0; i < 64; ++i) nat[i] = (uint8_t)hv_mjd_natural(i);
    if (frame_coefs) frame_coefs->assign((size_t)mpf * 384, 0);
    bool same = true;
    for (int64_t u = 0; u < ipf && same; ++u) {
        const int64_t m0 = u * f.Ri, n = f.Ri == 0 || mpf - m0 < f.Ri ? mpf - m0 : f.Ri;
        const size_t len = ie[u] - ib[u];
        const int expect = u < ipf - 1 ? 0xD0 + (int)(u & 7) : 0;
        uint8_t* data = (uint8_t*)malloc(len ? len : 1);
        if (len) memcpy(data, scan + ib[u], len);
        int16_t* want = (int16_t*)aligned_alloc(16, (size_t)n * 768);
        int16_t* got = (int16_t*)aligned_alloc(16, (size_t)n * 768);
        int16_t* stage = (int16_t*)aligned_alloc(16, 128);
        memset(got, 0x5A, (size_t)n * 768);
        const int st_want = hv_mjd_interval(data, 0, (int64_t)len, expect, tabs, nat, n, stage, want);
        int32_t iters = 0;
        const int st_got = sync_unit(data, (int64_t)len, expect, tabs, nat, n, sub, got, &iters, c);
        same = st_want == st_got && memcmp(want, got, (size_t)n * 768) == 0 && (st_got == 0 || iters == -1) &&
               (iters == -1 || (iters >= 1 && iters <= (int64_t)((len + sub - 1) / sub + kLanes - 1) / kLanes * (kLanes + 1)));
        if (!same) fprintf(stderr, "unit %ld sub_bytes %d: status %d / %d (serial / sync), iters %d\n", (long)u, sub, st_want, st_got, iters);
        ++c.units, ++g_units;
        if (st_got >= 0 && st_got <= 4) ++g_status[st_got];
        if (u < ipf - 1 && !include_rst && ie[u] + 1 < scan_bytes && scan[ie[u]] == 0xFF && scan[ie[u] + 1] == 0xD0 + (u & 7)) ++c.rst_end;
        if (frame_coefs) memcpy(frame_coefs->data() + (size_t)m0 * 384, got, (size_t)n * 768);
        if (frame_status) frame_status->push_back(st_got);
        free(stage), free(got), free(want), free(data);
    }
    free(tabs);
    return same;
}

}  // namespace

int main(int argc, char** argv) {
    int mutations = 400, dump_sub = 16;
    std::string dump;
    std::vector<const char*> files;
    for (int a = 1; a < argc; ++a) {
        if (!strncmp(argv[a], "--mutations=", 12)) mutations = atoi(argv[a] + 12);
        else if (!strncmp(argv[a], "--dump=", 7)) dump = argv[a] + 7;
        else if (!strncmp(argv[a], "--dump-sub=", 11)) dump_sub = atoi(argv[a] + 11);
        else files.push_back(argv[a]);
    }
    if (files.empty()) {
        fprintf(stderr, "usage: %s [--mutations=N] [--dump=DIR] [--dump-sub=S] file.jpg ...\n", argv[0]);
        return 2;
    }
    std::vector<int> sizes;
    for (int s = HV_MJPEG_SYNC_MIN_SUB; s <= 64; ++s) sizes.push_back(s);
    sizes.push_back(128), sizes.push_back(1024), sizes.push_back(HV_MJPEG_SYNC_MAX_SUB);
    for (const char* path : files) {
        FILE* fp = fopen(path, "rb");
        if (!fp) {
            fprintf(stderr, "%s: cannot open\n", path);
            return 2;
        }
        std::vector<uint8_t> d;
        uint8_t buf[4096];
        for (size_t n; (n = fread(buf, 1, sizeof buf, fp)) > 0;) d.insert(d.end(), buf, buf + n);
        fclose(fp);
        Frame f;
        if (d.size() < 4 || !parse(d, f)) {
            fprintf(stderr, "%s: not a fixture this program reads\n", path);
            return 2;
        }
        const std::vector<uint8_t> scan(d.begin() + f.begin, d.begin() + f.end);
        const char* base = strrchr(path, '/') ? strrchr(path, '/') + 1 : path;
        for (int sub : sizes)
            for (int inc = 0; inc < (f.Ri ? 2 : 1); ++inc) {
                Census c;
                std::vector<int16_t> coefs;
                std::vector<int> status;
                if (!check_frame(f, scan.data(), scan.size(), f.huff, sub, inc != 0, c, &coefs, &status)) {
                    fprintf(stderr, "%s: sub_bytes %d: the decoders differ\n", path, sub);
                    return 1;
                }
                for (int st : status)
                    if (st != 0) {
                        fprintf(stderr, "%s: the unmutated file does not decode with status 0\n", path);
                        return 1;
                    }
                printf("census %s sub=%d rst_inside=%d scan=%zu units=%ld fallback=%ld straddle=%ld value_cross=%ld span=%ld blocks=%ld code=%ld "
                       "rounds=%ld short=%ld rst_end=%ld iters=%ld\n", base, sub, inc, scan.size(), c.units, c.fallback, c.straddle, c.value_cross,
                       c.span, c.blocks, c.code, c.rounds, c.short_units, c.rst_end, c.iters);
                g_all.add(c);
                if (!dump.empty() && sub == dump_sub && inc == 0) {
                    FILE* o = fopen((dump + "/" + base + ".coefs").c_str(), "wb");
                    FILE* s = fopen((dump + "/" + base + ".status").c_str(), "w");
                    if (!o || !s) {
                        fprintf(stderr, "%s: cannot write\n", dump.c_str());
                        return 2;
                    }
                    fwrite(coefs.data(), 2, coefs.size(), o);
                    for (int st : status) fprintf(s, "%d\n", st);
                    fclose(o), fclose(s);
                }
            }
        for (int sub : {16, 128})
            for (int i = 0; i < mutations; ++i) {
                std::vector<uint8_t> s = scan;
                uint8_t huff[4 * kMjdTableBytes];
                memcpy(huff, f.huff, sizeof huff);
                switch (i % 8) {
                    case 0:                                                        // bit flips
                        for (int k = 0, n = 1 + rnd() % 4; k < n && !s.empty(); ++k) s[rnd() % s.size()] ^= (uint8_t)(1u << (rnd() % 8));
                        break;
                    case 1: s.resize(rnd() % (s.size() + 1)); break;               // truncation
                    case 2: memset(s.data(), 0xFF, s.size()); break;               // all ones
                    case 3: memset(s.data(), 0x00, s.size()); break;               // all zeros
                    case 4:                                                        // random bytes
                        for (auto& v : s) v = (uint8_t)rnd();
                        break;
                    case 5:                                                        // a random tail
                        for (size_t k = s.empty() ? 0 : rnd() % s.size(); k < s.size(); ++k) s[k] = (uint8_t)rnd();
                        break;
                    case 6:                                                        // a random byte value somewhere, markers included
                        if (!s.empty()) s[rnd() % s.size()] = (uint8_t)(0xC0 + rnd() % 0x40);
                        break;
                    case 7:                                                        // a changed table (refused ones are skipped)
                        for (int k = 0, n = 1 + rnd() % 3; k < n; ++k) huff[rnd() % sizeof huff] = (uint8_t)rnd();
                        break;
                }
                if (i % 16 == 2) s.resize(s.size() + 64, 0xFF);                    // longer than the frame needs
                Census c;
                if (!check_frame(f, s.data(), s.size(), huff, sub, (i & 8) != 0 && f.Ri != 0, c, nullptr, nullptr)) {
                    fprintf(stderr, "%s: sub_bytes %d, mutation %d: the decoders differ\n", path, sub, i);
                    return 1;
                }
                g_all.add(c);
            }
    }
    printf("mjpeg_sync_check: %ld units compared with the serial decoder, %ld through the fallback, status counts 0:%ld 1:%ld 2:%ld 3:%ld "
           "4:%ld, nothing differs\n", g_units, g_all.fallback, g_status[0], g_status[1], g_status[2], g_status[3], g_status[4]);
    return 0;
}
