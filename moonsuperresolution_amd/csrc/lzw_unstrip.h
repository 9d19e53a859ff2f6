// lzw_unstrip.h — the TIFF 6.0 LZW decoder of ONE strip or tile as one __host__ __device__ function, the twin of
// lzw_strip.h: the kernel of geotiff_codec.hip runs it with the 64 lanes of a one-wave workgroup, a host program runs it
// with one "lane" (nlanes = 1) under a sanitizer against msr_lzw_decode (host_codecs.cpp), whose return value and bytes
// [0, return value) it reproduces for every input, well-formed or not.
//
// Between two ClearCodes the width of a code depends only on how many codes came before it (`next` advances by one per
// code while it is below 4096, the first code after a Clear does not advance it, and the width is a function of `next`),
// so the stream is taken in batches of 64 codes:
//   1. lane k computes the bit position of the batch's k-th code in closed form from (bitpos, next, have_prev) of the
//      batch start (lzwd_bits_before: the prefix sum of the widths, which are piecewise constant in `next`) and extracts
//      its code; a code that would cross the end of the input becomes LZWD_END;
//   2. the uniform part walks the codes in order exactly as the host automaton does: it stops at the first 256 (the next
//      batch starts behind it with next = 258), 257 or LZWD_END, validates each code against its `next`, gives it its
//      output offset and writes the new table entry (prefix code, last byte, length | first byte);
//   3. lane k writes the string of code k by walking its prefix chain backwards from offset + length - 1.  A KwKwK code
//      (code == next) is the entry step 2 has just written for it, so it needs no case of its own.
//
// Every loop is bounded by an argument or a constant, never by table contents alone: the batch loop by n_in * 8 / 9 codes,
// the walk by 64, a chain by the entry's stored length (at most 3839) with the write position kept inside the string;
// a table entry is read only for a code already checked < next (entries are written before they can be named, and an
// entry's prefix is always a lower code); every store is guarded by cap.  A malformed stream is an ordinary return value.
#pragma once
#include "lzw_strip.h"

namespace msr {

constexpr int LZWD_BATCH = 64;                // codes taken at a time: one per lane of the wave
constexpr uint32_t LZWD_END = 0xFFFFu;        // "the code at this position would cross the end of the input"

struct LzwDecodeWorkspace {                   // 20864 bytes
    uint32_t ent[4096];                       // codes 258..4095: prefix code | last byte << 12 | length << 20 (<= 3839)
    uint8_t first[4096];                      // first byte of the code's string
    uint16_t code[LZWD_BATCH];                // the batch's codes
    int32_t off[LZWD_BATCH];                  // output offset of each code's string
};

// The width of a code read while the next free code is `next` (the "early change" of TIFF: one code before 512 / 1024 / 2048).
LZW_HD inline int lzwd_width(int next) { return next < 511 ? 9 : next < 1023 ? 10 : next < 2047 ? 11 : 12; }

// Bits of the codes read while `next` runs over 258 .. n - 1 (258 <= n <= 4096), one code per value.
LZW_HD inline int64_t lzwd_bits_before(int n) {
    int64_t b = 9 * (int64_t)((n < 511 ? n : 511) - 258);
    if (n > 511) b += 10 * (int64_t)((n < 1023 ? n : 1023) - 511);
    if (n > 1023) b += 11 * (int64_t)((n < 2047 ? n : 2047) - 1023);
    if (n > 2047) b += 12 * (int64_t)(n - 2047);
    return b;
}

// Code k of the batch for the uniform walk: lane k holds it in a register on the device (nlanes == 64 there).
LZW_HD inline uint32_t lzwd_code_at(const LzwDecodeWorkspace* ws, uint32_t mine, int k) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__builtin_amdgcn_readlane((int)mine, k);
#else
    (void)mine;
    return ws->code[k];
#endif
}

// Decodes the n_in bytes at src to dst[0 .. cap): msr_lzw_decode(src, n_in, dst, cap), i.e. the number of bytes produced
// (a stream that ends without EndOfInformation gives what it produced), or -1 for a malformed stream, an output longer than
// cap or a negative n_in / cap.  One addition: a result 0 <= r < cap zeroes bytes [r, cap) (what geotiff.lzw_decode does on
// the host afterwards).  No byte at or beyond dst + cap is written.  Every lane of the nlanes that call it together gets
// the same result; on the device nlanes is 64, the lanes of one wave.
LZW_HD inline int32_t lzw_decode_strip(LzwDecodeWorkspace* ws, const uint8_t* src, int32_t n_in, uint8_t* dst, int32_t cap,
                                       int lane, int nlanes) {
    if (n_in < 0 || cap < 0) return -1;
    const int64_t bits_in = (int64_t)n_in * 8;
    int64_t bitpos = 0;
    int next = 258, prev = -1;
    uint32_t prev_first = 0, prev_len = 0;     // first byte and length of prev's string
    int32_t op = 0;                            // bytes produced: <= cap
    int status = 0;                            // 0: more to read, 1: end of the stream, -1: malformed / too long
    const int64_t max_batches = bits_in / 9 + 2;   // a batch that does not end the stream consumes at least one code
    for (int64_t it = 0; it < max_batches && status == 0; ++it) {
        // 1. the batch's codes, as if no Clear or EOI came among them
        const bool have_prev = prev >= 0;
        const int64_t base = bitpos - lzwd_bits_before(next);
        uint32_t mine = LZWD_END;
        for (int k = lane; k < LZWD_BATCH; k += nlanes) {
            const int steps = have_prev ? k : (k > 0 ? k - 1 : 0);      // how often `next` advanced before code k
            int nk = next + steps, beyond = 0;
            if (nk > 4096) beyond = nk - 4096, nk = 4096;               // a full table: 12 bits a code, no new entries
            const int64_t bp = base + lzwd_bits_before(nk) + 12 * (int64_t)beyond + ((!have_prev && k > 0) ? 9 : 0);
            const int w = lzwd_width(nk);
            uint32_t c = LZWD_END;
            if (bp + w <= bits_in) {                                    // so bp / 8 < n_in
                const int64_t b = bp >> 3;
                uint32_t v = (uint32_t)src[b] << 16;
                if (b + 1 < n_in) v |= (uint32_t)src[b + 1] << 8;
                if (b + 2 < n_in) v |= (uint32_t)src[b + 2];
                c = (v >> (24 - (int)(bp & 7) - w)) & ((1u << w) - 1);
            }
            ws->code[k] = (uint16_t)c;
            mine = c;
        }
        lzw_sync();
        // 2. the automaton, on wave-uniform values: validate, place, extend the table
        int m = 0;                                                      // codes of this batch that produce a string
        for (int k = 0; k < LZWD_BATCH; ++k) {
            const uint32_t c = lzw_uniform(lzwd_code_at(ws, mine, k));
            if (c == LZWD_END || c == 257) { status = 1; break; }
            bitpos += lzwd_width(next);
            if (c == 256) { next = 258; prev = -1; break; }
            uint32_t first, len;
            if (prev < 0) {
                if (c >= 256) { status = -1; break; }
            } else if ((int)c >= next) {
                if ((int)c != next) { status = -1; break; }
            }
            if (c < 256) {
                first = c, len = 1;
            } else if ((int)c == next) {                               // KwKwK: prev's string + its own first byte
                first = prev_first, len = prev_len + 1;
            } else {
                first = lzw_uniform(ws->first[c]);
                len = lzw_uniform(ws->ent[c]) >> 20;
            }
            if ((int64_t)op + len > cap) { status = -1; break; }
            if (prev >= 0 && next < 4096) {
                ws->ent[next] = (uint32_t)prev | first << 12 | (prev_len + 1) << 20;
                ws->first[next] = (uint8_t)prev_first;
                ++next;
            }
            ws->off[k] = op;
            op += (int32_t)len;
            prev = (int)c, prev_first = first, prev_len = len;
            m = k + 1;
        }
        lzw_sync();
        // 3. the strings, one per lane
        for (int k = lane; k < m; k += nlanes) {
            uint32_t c = ws->code[k] & 4095u;
            const int64_t o = ws->off[k];
            const int32_t len = c < 256 ? 1 : (int32_t)(ws->ent[c] >> 20);
            int64_t pos = o + len - 1;
            for (int i = 0; i < len - 1 && c >= 258; ++i) {
                const uint32_t e = ws->ent[c];
                if (pos >= o && pos < cap) dst[pos] = (uint8_t)(e >> 12);
                --pos;
                c = e & 4095u;
            }
            if (pos >= o && pos < cap) dst[pos] = (uint8_t)c;
        }
        lzw_sync();
    }
    if (status < 0) return -1;
    for (int64_t i = (int64_t)op + lane; i < cap; i += nlanes) dst[i] = 0;
    return op;
}

}  // namespace msr
