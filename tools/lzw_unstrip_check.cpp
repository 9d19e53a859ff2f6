// CPU only, stand-alone: the per-block automaton of the device GeoTIFF decoder (csrc/lzw_unstrip.h, run here with one lane)
// against the host decoder msr_lzw_decode (csrc/host_codecs.cpp), under AddressSanitizer / UBSan.  Source and destination are
// heap blocks of exactly n_in and cap bytes, so a read or write one byte outside either is an error.  Compared: the return
// value, bytes [0, return value), and the zeroed tail [return value, cap).
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Imoonsuperresolution_amd/csrc \
//       tools/lzw_unstrip_check.cpp moonsuperresolution_amd/csrc/host_codecs.cpp -o /tmp/lzw_unstrip_check && /tmp/lzw_unstrip_check
// Cases (those of tests/test_geotiff_decode_host.py, but for the libtiff-written strips): the streams of msr_lzw_encode for
// every prefix 0 .. 4400 of a random buffer and all 12000 bytes, 280000 zeros, a 2-byte pattern, a four-symbol alphabet;
// hand-packed streams (no leading Clear, two Clears in a row, bytes after EOI, an encoder that never clears); the empty input,
// a 300-byte stream cut at every length, cap one short and cap 0, a code above `next`, a first code >= 258 after Clear, 200
// single-bit flips and 100 garbage streams.
#include "lzw_unstrip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>
extern "C" int64_t msr_lzw_encode(const uint8_t* in, int64_t n_in, uint8_t* out, int64_t cap);
extern "C" int64_t msr_lzw_decode(const uint8_t* in, int64_t n_in, uint8_t* out, int64_t n_out);
typedef std::vector<uint8_t> Bytes;
static msr::LzwDecodeWorkspace ws;
static int n_cases = 0;

// `expect` >= -1: what both must return (the hand-packed streams, whose encoder lives in this file)
static int check(const Bytes& stream, int64_t cap, const char* what, int64_t expect = -2) {
    ++n_cases;
    Bytes ref(cap ? cap : 1, 0xEE);
    uint8_t dummy = 0;
    const int64_t want = msr_lzw_decode(stream.size() ? stream.data() : &dummy, stream.size(), ref.data(), cap);
    uint8_t* src = (uint8_t*)malloc(stream.size() ? stream.size() : 1);     // exact-size heap buffers: ASan sees any overrun
    if (stream.size()) memcpy(src, stream.data(), stream.size());
    uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
    memset(out, 0xA5, cap ? cap : 1);
    const int32_t got = msr::lzw_decode_strip(&ws, src, (int32_t)stream.size(), out, (int32_t)cap, 0, 1);
    int bad = got != want || (expect >= -1 && want != expect);
    if (!bad && want >= 0) {
        bad |= memcmp(out, ref.data(), want) != 0;
        for (int64_t i = want; i < cap; ++i) bad |= out[i] != 0;
    }
    free(src);
    free(out);
    if (bad) printf("MISMATCH %s n_in=%zu cap=%ld got %d want %ld\n", what, stream.size(), (long)cap, got, (long)want);
    return bad;
}

static Bytes encode(const Bytes& raw) {
    Bytes s(raw.size() + raw.size() / 2 + 1024);
    uint8_t dummy = 0;
    s.resize(msr_lzw_encode(raw.size() ? raw.data() : &dummy, raw.size(), s.data(), s.size()));
    return s;
}

struct Packer {                                // MSB-first codes of explicit widths
    Bytes out;
    uint64_t buf = 0;
    int nbits = 0;
    void put(int code, int width) {
        buf = (buf << width) | (uint32_t)code;
        nbits += width;
        while (nbits >= 8) out.push_back((uint8_t)(buf >> (nbits - 8))), nbits -= 8;
    }
    Bytes done() {
        if (nbits) out.push_back((uint8_t)(buf << (8 - nbits))), nbits = 0;
        return out;
    }
};

// A greedy encoder with the decoder's width rule that never sends a Clear after the first: the table fills to 4096 and
// 12-bit codes go on without new entries.  `lead` = false drops the leading Clear too.
static Bytes encode_no_clear(const Bytes& raw, bool lead) {
    std::map<std::string, int> tab;
    Packer p;
    int next = 258;                            // the decoder's `next` lags one entry behind the encoder's
    if (lead) p.put(256, 9);
    std::string cur;
    int emitted = 0;
    auto width = [&]() { return msr::lzwd_width(next); };
    auto code_of = [&](const std::string& s) { return s.size() == 1 ? (int)(uint8_t)s[0] : tab[s]; };
    int enc_next = 258;
    for (uint8_t b : raw) {
        std::string ext = cur + (char)b;
        if (ext.size() == 1 || tab.count(ext)) { cur = ext; continue; }
        p.put(code_of(cur), width());
        if (emitted && next < 4096) ++next;    // the decoder adds an entry for every code but the first
        ++emitted;
        if (enc_next < 4096) tab[ext] = enc_next++;
        cur = std::string(1, (char)b);
    }
    if (!cur.empty()) {
        p.put(code_of(cur), width());
        if (emitted && next < 4096) ++next;
        ++emitted;
    }
    p.put(257, width());
    return p.done();
}

int main() {
    std::mt19937 g(1234);
    Bytes buf(12000);
    for (auto& b : buf) b = g() & 255;
    int bad = 0;
    for (int n = 0; n <= 4400; ++n) bad += check(encode(Bytes(buf.begin(), buf.begin() + n)), n, "prefix");
    bad += check(encode(buf), buf.size(), "full");
    bad += check(encode(Bytes(280000, 0)), 280000, "zeros");
    Bytes pat(200000), four(60000);
    for (size_t i = 0; i < pat.size(); ++i) pat[i] = (i & 1) ? 0 : 31;
    for (auto& b : four) b = g() & 3;
    bad += check(encode(pat), pat.size(), "pattern");
    bad += check(encode(four), four.size(), "four");
    // hand-packed
    bad += check(encode_no_clear(four, true), four.size(), "never clears", four.size());
    bad += check(encode_no_clear(four, false), four.size(), "no leading clear", four.size());
    bad += check(encode_no_clear(buf, true), buf.size(), "never clears, random", buf.size());
    { Packer p; p.put(256, 9); p.put(256, 9); p.put(65, 9); p.put(66, 9); p.put(258, 9); p.put(256, 9); p.put(256, 9); p.put(67, 9);
      p.put(257, 9); bad += check(p.done(), 16, "two clears", 5); }
    { Packer p; p.put(256, 9); p.put(65, 9); p.put(258, 9); p.put(257, 9); Bytes s = p.done(); s.push_back(0xFF); s.push_back(0x12);
      s.push_back(0x80); bad += check(s, 8, "bytes after EOI", 3); }
    // malformed or short
    bad += check(Bytes(), 16, "empty");
    bad += check(Bytes(), 0, "empty, cap 0");
    Bytes e300 = encode(Bytes(buf.begin(), buf.begin() + 280));
    e300.resize(300, 0);
    for (size_t n = 0; n <= 300; ++n) bad += check(Bytes(e300.begin(), e300.begin() + n), 280, "truncated");
    bad += check(encode(four), four.size() - 1, "cap one short");
    bad += check(encode(four), 0, "cap 0");
    bad += check(encode(Bytes(buf.begin(), buf.begin() + 700)), 699, "cap one short, random");
    { Packer p; p.put(256, 9); p.put(65, 9); p.put(66, 9); p.put(300, 9); p.put(257, 9); bad += check(p.done(), 64, "code above next", -1); }
    { Packer p; p.put(256, 9); p.put(258, 9); p.put(257, 9); bad += check(p.done(), 64, "first code 258", -1); }
    { Packer p; p.put(256, 9); p.put(65, 9); p.put(256, 9); p.put(300, 9); p.put(257, 9); bad += check(p.done(), 64, "300 after clear", -1); }
    const Bytes good = encode(Bytes(buf.begin(), buf.begin() + 3000));
    for (int i = 0; i < 200; ++i) {
        Bytes s(good);
        const size_t bit = g() % (s.size() * 8);
        s[bit >> 3] ^= (uint8_t)(0x80 >> (bit & 7));
        bad += check(s, 3000, "bit flip");
    }
    const Bytes good4 = encode(four);
    for (int i = 0; i < 50; ++i) {
        Bytes s(good4);
        const size_t bit = g() % (s.size() * 8);
        s[bit >> 3] ^= (uint8_t)(0x80 >> (bit & 7));
        bad += check(s, four.size(), "bit flip, long strings");
    }
    for (int i = 0; i < 100; ++i) {
        Bytes s(1 + g() % 2000);
        for (auto& b : s) b = g() & 255;
        if (i & 1) s[0] = 0x80, s[1] &= 0x7F;                  // every other one starts with a Clear
        bad += check(s, 4096, "garbage");
    }
    printf("%s (%d mismatches in %d cases)\n", bad ? "FAIL" : "OK", bad, n_cases);
    return bad != 0;
}
