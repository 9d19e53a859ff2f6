// CPU only, stand-alone: the per-strip automaton of the device GeoTIFF encoder (csrc/lzw_strip.h, run here with one lane)
// against the host encoder msr_lzw_encode (csrc/host_codecs.cpp), under AddressSanitizer / UBSan.  Source and destination are
// heap blocks of exactly the strip's and the stream's size, so a read or write one byte outside either is an error; every case
// runs again with a destination one byte short (the result must be -1 and the bytes before the end the same).
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Imoonsuperresolution_amd/csrc \
//       tools/lzw_strip_check.cpp moonsuperresolution_amd/csrc/host_codecs.cpp -o /tmp/lzw_strip_check && /tmp/lzw_strip_check
// Cases: every prefix 0 .. 4400 of a random buffer (each width change, the table clear) and all 12000 bytes, 280000 zeros, a
// 2-byte pattern, a four-symbol alphabet, and the horizontal predictor for 1 / 2 / 4-byte samples over rows of 1 .. 70001.
#include "lzw_strip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <random>
extern "C" int64_t msr_lzw_encode(const uint8_t* in, int64_t n_in, uint8_t* out, int64_t cap);
static msr::LzwWorkspace ws;
static int check(const std::vector<uint8_t>& raw, int sb, int rb, const char* what) {
    std::vector<uint8_t> d(raw);
    if (sb) {
        size_t rows = raw.size() / rb;
        for (size_t r = 0; r < rows; ++r)
            for (int j = rb / sb - 1; j >= 1; --j) {
                uint32_t a = 0, b = 0;
                memcpy(&a, &raw[r * rb + j * sb], sb); memcpy(&b, &raw[r * rb + (j - 1) * sb], sb);
                uint32_t v = a - b; memcpy(&d[r * rb + j * sb], &v, sb);
            }
    }
    size_t cap = raw.size() + raw.size() / 2 + 1024;
    std::vector<uint8_t> ref(cap);
    uint8_t dummy = 0; int64_t nr = msr_lzw_encode(d.size() ? d.data() : &dummy, d.size(), ref.data(), cap);
    // exact-size heap buffers so ASan sees any overrun
    uint8_t* src = (uint8_t*)malloc(raw.size() ? raw.size() : 1); if (raw.size()) memcpy(src, raw.data(), raw.size());
    uint8_t* out = (uint8_t*)malloc(nr);
    int32_t n = msr::lzw_encode_strip(&ws, src, (int32_t)raw.size(), sb, rb, out, (int32_t)nr, 0, 1);
    int bad = (n != nr) || memcmp(out, ref.data(), nr);
    // one byte short: -1, and nothing past
    uint8_t* out2 = (uint8_t*)malloc(nr - 1);
    int32_t n2 = msr::lzw_encode_strip(&ws, src, (int32_t)raw.size(), sb, rb, out2, (int32_t)nr - 1, 0, 1);
    bad |= (n2 != -1) || memcmp(out2, ref.data(), nr - 1);
    free(src); free(out); free(out2);
    if (bad) printf("MISMATCH %s n=%zu sb=%d rb=%d got %d want %ld\n", what, raw.size(), sb, rb, n, (long)nr);
    return bad;
}
int main() {
    std::mt19937 g(1234);
    std::vector<uint8_t> buf(12000);
    for (auto& b : buf) b = g() & 255;
    int bad = 0;
    for (int n = 0; n <= 4400; ++n) bad += check(std::vector<uint8_t>(buf.begin(), buf.begin() + n), 0, 0, "prefix");
    bad += check(buf, 0, 0, "full");
    bad += check(std::vector<uint8_t>(280000, 0), 0, 0, "zeros");
    { std::vector<uint8_t> p(100000); for (size_t i = 0; i < p.size(); ++i) p[i] = (i & 1) ? 0 : 31; bad += check(p, 0, 0, "pattern"); }
    { std::vector<uint8_t> p(60000); for (auto& b : p) b = g() & 3; bad += check(p, 0, 0, "four"); }
    for (int sb : {1, 2, 4}) for (int cols : {1, 3, 257, 300, 70001}) for (int rows : {1, 5}) {
        int rb = cols * sb;
        std::vector<uint8_t> p((size_t)rows * rb);
        // smooth-ish data
        for (size_t i = 0; i < p.size(); ++i) p[i] = (uint8_t)((i / 7) + (g() & 3));
        bad += check(p, sb, rb, "pred");
    }
    printf("%s (%d mismatches)\n", bad ? "FAIL" : "OK", bad);
    return bad != 0;
}
