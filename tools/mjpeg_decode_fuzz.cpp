// Host fuzz program of the entropy decoder csrc/hv_mjpeg_decode.hpp: the same text the GPU kernel compiles, here for the CPU under
// -fsanitize=address,undefined, with its own main and nothing preloaded.  It decodes every JPEG file given on the command line, then
// a few thousand mutations of each from a fixed seed (byte flips, truncations, all-ones, all-zeros, random bytes, random tails, Huffman
// tables with changed bytes), every interval against heap buffers of exactly the size the contract names: the interval's bytes, its
// n_mcus * 768 bytes of coefficients, 128 bytes of staging.  Exit 0 only if every run ends with a status 0 .. 4 (and the unmutated files
// with 0); a sanitizer report aborts with its own exit code.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I hunyuanvideo_efficiency_amd/csrc \
//       tools/mjpeg_decode_fuzz.cpp -o /tmp/mjpeg_decode_fuzz && /tmp/mjpeg_decode_fuzz tests/golden/mjpeg_read/*.jpg
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hv_mjpeg_decode.hpp"

namespace {

struct Frame {
    int W = 0, H = 0, Ri = 0;
    uint8_t huff[4 * kMjdTableBytes] = {};
    bool have_huff = false;
    size_t begin = 0, end = 0;
};

// the headers of a baseline 4:2:0 file the fixtures' maker wrote (no refusals here: mjpeg_io.parse_jpeg owns those)
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

long g_runs = 0, g_status[5] = {0, 0, 0, 0, 0};

// every interval of one frame, each against exactly sized heap buffers; -1 if a status is out of range, else the largest status
int decode_frame(const Frame& f, const uint8_t* scan, size_t scan_bytes, const uint8_t* huff) {
    if (!hv_mjd_tables_ok(huff)) return 0;                                        // the entry point refuses: nothing is decoded
    HvHuffTab* tabs = (HvHuffTab*)malloc(4 * sizeof(HvHuffTab));
    for (int i = 0; i < 4; ++i) hv_mjd_build(huff + i * kMjdTableBytes, &tabs[i]);
    const int64_t mpf = (int64_t)((f.W + 15) / 16) * ((f.H + 15) / 16);
    const int64_t ipf = f.Ri == 0 ? 1 : (mpf + f.Ri - 1) / f.Ri;
    // stage A on the host: the intervals between the RSTm markers
    std::vector<size_t> ib(ipf, scan_bytes), ie(ipf, scan_bytes);
    ib[0] = 0;
    int64_t k = 0;
    for (size_t j = 0; j + 1 < scan_bytes && k < ipf - 1; ++j)
        if (scan[j] == 0xFF && (scan[j + 1] & 0xF8) == 0xD0) ie[k] = j, ib[k + 1] = j + 2, ++k;
    int worst = 0;
    uint8_t nat[64];
    for (int i = 0; i < 64; ++i) nat[i] = (uint8_t)hv_mjd_natural(i);
    for (int64_t u = 0; u < ipf; ++u) {
        const int64_t m0 = u * f.Ri, n = f.Ri == 0 || mpf - m0 < f.Ri ? mpf - m0 : f.Ri;
        const size_t len = ie[u] - ib[u];
        uint8_t* data = (uint8_t*)malloc(len ? len : 1);
        if (len) memcpy(data, scan + ib[u], len);
        int16_t* out = (int16_t*)aligned_alloc(16, (size_t)n * 768);
        int16_t* stage = (int16_t*)aligned_alloc(16, 128);
        const int st = hv_mjd_interval(data, 0, (int64_t)len, u < ipf - 1 ? 0xD0 + (int)(u & 7) : 0, tabs, nat, n, stage, out);
        free(stage), free(out), free(data);
        ++g_runs;
        if (st < 0 || st > 4) {
            free(tabs);
            return -1;
        }
        ++g_status[st];
        if (st > worst) worst = st;
    }
    free(tabs);
    return worst;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s file.jpg ...\n", argv[0]);
        return 2;
    }
    const int kMutations = argc > 2 && !strncmp(argv[1], "--mutations=", 12) ? atoi(argv[1] + 12) : 400;
    for (int a = 1; a < argc; ++a) {
        if (!strncmp(argv[a], "--", 2)) continue;
        FILE* fp = fopen(argv[a], "rb");
        if (!fp) {
            fprintf(stderr, "%s: cannot open\n", argv[a]);
            return 2;
        }
        std::vector<uint8_t> d;
        uint8_t buf[4096];
        for (size_t n; (n = fread(buf, 1, sizeof buf, fp)) > 0;) d.insert(d.end(), buf, buf + n);
        fclose(fp);
        Frame f;
        if (d.size() < 4 || !parse(d, f)) {
            fprintf(stderr, "%s: not a fixture this program reads\n", argv[a]);
            return 2;
        }
        const std::vector<uint8_t> scan(d.begin() + f.begin, d.begin() + f.end);
        if (decode_frame(f, scan.data(), scan.size(), f.huff) != 0) {
            fprintf(stderr, "%s: the unmutated file does not decode with status 0\n", argv[a]);
            return 1;
        }
        for (int i = 0; i < kMutations; ++i) {
            std::vector<uint8_t> s = scan;
            uint8_t huff[4 * kMjdTableBytes];
            memcpy(huff, f.huff, sizeof huff);
            switch (i % 8) {
                case 0:                                                            // byte flips
                    for (int k = 0, n = 1 + rnd() % 4; k < n && !s.empty(); ++k) s[rnd() % s.size()] ^= (uint8_t)(1u << (rnd() % 8));
                    break;
                case 1: s.resize(rnd() % (s.size() + 1)); break;                   // truncation
                case 2: memset(s.data(), 0xFF, s.size()); break;                   // all ones
                case 3: memset(s.data(), 0x00, s.size()); break;                   // all zeros
                case 4:                                                            // random bytes
                    for (auto& v : s) v = (uint8_t)rnd();
                    break;
                case 5:                                                            // a random tail
                    for (size_t k = s.empty() ? 0 : rnd() % s.size(); k < s.size(); ++k) s[k] = (uint8_t)rnd();
                    break;
                case 6:                                                            // a random byte value somewhere, markers included
                    if (!s.empty()) s[rnd() % s.size()] = (uint8_t)(0xC0 + rnd() % 0x40);
                    break;
                case 7:                                                            // a changed table (refused ones are skipped)
                    for (int k = 0, n = 1 + rnd() % 3; k < n; ++k) huff[rnd() % sizeof huff] = (uint8_t)rnd();
                    break;
            }
            if (i % 16 == 2) s.resize(s.size() + 64, 0xFF);                        // longer than the frame needs
            if (decode_frame(f, s.data(), s.size(), huff) < 0) {
                fprintf(stderr, "%s: mutation %d: a status outside 0 .. 4\n", argv[a], i);
                return 1;
            }
        }
    }
    printf("mjpeg_decode_fuzz: %ld interval decodes, status counts 0:%ld 1:%ld 2:%ld 3:%ld 4:%ld, no sanitizer report\n", g_runs,
           g_status[0], g_status[1], g_status[2], g_status[3], g_status[4]);
    return 0;
}
