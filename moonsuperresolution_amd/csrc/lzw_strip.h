// lzw_strip.h — the TIFF 6.0 LZW encoder of ONE strip, with the horizontal predictor fused into its input fetch, as one
// __host__ __device__ function: the kernel of geotiff_codec.hip runs it with the 64 lanes of a one-wave workgroup, a host
// program can run it with one "lane" (nlanes = 1) under a sanitizer against msr_lzw_encode (host_codecs.cpp).  The input is
// a strip that lies contiguous in memory (lzw_fetch, lzw_encode_strip) or a block — a tile — read where it lies in a
// row-major raster, its padding synthesised (lzw_fetch_block, lzw_encode_block); the automaton (lzw_encode_stream) is one.
// For float32 samples either input can go through the floating-point predictor instead (lzw_fetch_fp, lzw_encode_strip_fp,
// lzw_encode_block_fp).
//
// The stream is byte for byte msr_lzw_encode's for the same (differenced) bytes: ClearCode first, MSB-first codes of 9..12
// bits, the width grows when `next` reaches 512 / 1024 / 2048, Clear when it reaches 4095, one more ++next (and width bump)
// before EndOfInformation, zero padding of the last byte; the empty strip is Clear, EOI.  Greedy longest match is canonical,
// so only the dictionary's data structure differs: an open-addressing hash of (prefix code << 8 | byte) -> code.
//
// The automaton is serial, so every lane runs it on the same values (the state is wave-uniform and lives in registers; the
// dictionary, the differenced input chunk and the output bytes live in the workspace, LDS on the device).  The lanes
// share the work that is parallel: fetching and differencing 256 input bytes, clearing the table, storing the output.
//
// Every loop is bounded by an argument or a constant, never by table contents: the input loop by n, a probe by
// LZW_SLOTS, the byte drain of the bit buffer by the 12-bit code width.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LZW_HD __host__ __device__
#else
#define LZW_HD
#endif

namespace msr {

constexpr int LZW_SLOTS = 8192;               // hash slots: at most 3837 entries (codes 258..4094) live at once, load <= 0.47
constexpr int LZW_CHUNK = 256;                // input bytes fetched at a time (a multiple of every sample width)
constexpr int LZW_STAGE = 512;                // output ring: flushed 256 bytes at a time, a code adds at most 2
constexpr uint32_t LZW_EMPTY = 0xFFFFFFFFu;   // (key << 12 | code) of no entry: it would need code 4095, which is never given

struct LzwWorkspace {
    uint32_t tab[LZW_SLOTS];                  // key << 12 | code
    uint8_t raw[LZW_CHUNK + 4];               // the chunk as read, behind the 4 bytes before it (the previous sample)
    alignas(4) uint8_t in[LZW_CHUNK];         // the chunk the automaton reads (four bytes at a time): differenced if a
                                              // predictor is asked for
    uint8_t stage[LZW_STAGE];                 // output bytes not stored yet, at position & (LZW_STAGE - 1)
};

// A value every lane holds alike (it was read from one LDS address by all of them), declared so: on the device the automaton's
// state then lives in scalar registers and its branches are scalar, instead of 64 lanes repeating the same vector arithmetic.
LZW_HD inline uint32_t lzw_uniform(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
#else
    return v;
#endif
}

LZW_HD inline void lzw_sync() {
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#endif
}

// Bytes [base, base + LZW_CHUNK) of the strip into ws->in, zero past n.  sample_bytes 1 / 2 / 4: every sample but the
// first of a row of row_bytes becomes u[j] - u[j-1] modulo the sample width (little-endian); 0: the bytes as they are.
LZW_HD inline void lzw_fetch(LzwWorkspace* ws, const uint8_t* src, int32_t n, int64_t base, int32_t sample_bytes,
                             int32_t row_bytes, int lane, int nlanes) {
    for (int i = lane; i < LZW_CHUNK + 4; i += nlanes) {
        const int64_t p = base + i - 4;
        ws->raw[i] = (p >= 0 && p < n) ? src[p] : (uint8_t)0;
    }
    lzw_sync();
    for (int i = lane; i < LZW_CHUNK; i += nlanes) {
        const uint8_t* r = ws->raw + 4 + i;
        uint8_t v = r[0];
        if (sample_bytes > 0) {
            const int32_t col = (int32_t)((uint32_t)(base + i) % (uint32_t)row_bytes);   // base + i < 2^31 + LZW_CHUNK
            const int32_t k = col & (sample_bytes - 1);         // byte of the sample; samples never straddle a chunk
            if (col - k > 0) {
                uint32_t cur = 0, prev = 0;
                for (int b = 0; b <= k; ++b) {                  // the borrow only travels upwards: bytes 0..k decide byte k
                    cur |= (uint32_t)r[b - k] << (8 * b);
                    prev |= (uint32_t)r[b - k - sample_bytes] << (8 * b);
                }
                v = (uint8_t)((cur - prev) >> (8 * k));
            }
        }
        ws->in[i] = v;
    }
    lzw_sync();
}

// A block of a row-major raster, read where it lies: byte q of the block is row q / block_w_bytes, column byte
// q % block_w_bytes; it is src[row * pitch + column] inside the valid part (row < valid_rows, column < valid_w_bytes) and zero
// elsewhere: the padding of an edge tile, the 4 bytes in front of the block and the tail of the last chunk.  src points at the
// block's first sample; row * pitch is 64-bit (a block of a 4.2 GB level lies past the 2 GiB and 4 GiB lines).
struct LzwBlock {
    const uint8_t* src;
    int64_t pitch;                            // bytes between raster rows
    int32_t valid_w_bytes, valid_rows;        // the part of the block that lies in the raster
    int32_t block_w_bytes;                    // a block row, padding included
};

LZW_HD inline uint8_t lzw_block_byte(const LzwBlock& b, int64_t q) {
    if (q < 0) return 0;
    const uint32_t y = (uint32_t)q / (uint32_t)b.block_w_bytes;                 // q < 2^30 + LZW_CHUNK: 32-bit division
    const uint32_t x = (uint32_t)q - y * (uint32_t)b.block_w_bytes;
    return (y < (uint32_t)b.valid_rows && x < (uint32_t)b.valid_w_bytes) ? b.src[(int64_t)y * b.pitch + x] : (uint8_t)0;
}

// lzw_fetch for a block read in place: bytes [base, base + LZW_CHUNK) of the block into ws->in.  The padding is there before
// the predictor, which restarts on every block row: the first padding sample of a row is 0 - the last valid sample.  The
// sample in front of a chunk comes from the same rule (block position q - sample_bytes), not from memory in front of the row.
LZW_HD inline void lzw_fetch_block(LzwWorkspace* ws, const LzwBlock& blk, int64_t base, int32_t sample_bytes, int lane,
                                   int nlanes) {
    for (int i = lane; i < LZW_CHUNK + 4; i += nlanes) ws->raw[i] = lzw_block_byte(blk, base + i - 4);
    lzw_sync();
    for (int i = lane; i < LZW_CHUNK; i += nlanes) {
        const uint8_t* r = ws->raw + 4 + i;
        uint8_t v = r[0];
        if (sample_bytes > 0) {
            const int32_t col = (int32_t)((uint32_t)(base + i) % (uint32_t)blk.block_w_bytes);
            const int32_t k = col & (sample_bytes - 1);         // byte of the sample; samples never straddle a chunk
            if (col - k > 0) {
                uint32_t cur = 0, prev = 0;
                for (int b = 0; b <= k; ++b) {                  // as in lzw_fetch: bytes 0..k decide byte k
                    cur |= (uint32_t)r[b - k] << (8 * b);
                    prev |= (uint32_t)r[b - k - sample_bytes] << (8 * b);
                }
                v = (uint8_t)((cur - prev) >> (8 * k));
            }
        }
        ws->in[i] = v;
    }
    lzw_sync();
}

// ---- the floating-point predictor (PREDICTOR=3, TIFF Technical Note 3) for float32 samples ------------------------------------
// A row of w samples (row_bytes = 4 w) is regrouped into four planes, the most significant byte of every sample first:
// regrouped byte q = p * w + x is T(q) = byte 3 - p of (little-endian) sample x.  The regrouped row is then byte-differenced
// from end to end, across the plane boundaries: output byte q is T(q) - T(q - 1) for q > 0 and T(0) for q = 0 (libtiff's
// fpDiff with stride 1).  Consecutive q of a plane read the same byte of consecutive samples, so the fetch is not contiguous
// and ws->raw with its "4 bytes in front" is not used: T(q - 1) comes from the same rule.

// Sample x of a row that begins at `row`.  A row on a 4-byte boundary is read with one aligned load per sample, the byte
// extracted by the caller; any other row byte by byte.
LZW_HD inline uint32_t lzw_fp_sample(const uint8_t* row, uint32_t x, bool aligned) {
    const uint8_t* s = row + 4 * (int64_t)x;
    if (aligned) return *reinterpret_cast<const uint32_t*>(s);
    return (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24;
}

// Output bytes [base, base + LZW_CHUNK) of the predictor into ws->in, zero past n, for a raster of rows of row_bytes bytes (a
// multiple of 4) whose sample x of row r is ``sample(r, x)``.  A lane takes runs of four consecutive output bytes: one division
// finds the position (row, plane, sample) of the byte in front of its run, the rest is stepping, so a chunk boundary inside a
// plane, a plane boundary inside a chunk and a row restart are all the same step.  base + LZW_CHUNK < 2^31 + LZW_CHUNK.
template <class Sample>
LZW_HD inline void lzw_fetch_fp(LzwWorkspace* ws, int32_t n, int64_t base, int32_t row_bytes, Sample sample, int lane, int nlanes) {
    const uint32_t w = (uint32_t)row_bytes >> 2;
    uint32_t* in32 = reinterpret_cast<uint32_t*>(ws->in);
    lzw_sync();                                                  // the automaton has read the chunk before: ws->in is free
    for (int i = 4 * lane; i < LZW_CHUNK; i += 4 * nlanes) {
        const uint32_t g = (uint32_t)(base + i);                 // the run's first byte, counted from the strip's start
        uint32_t r = 0, p = 0, x = 0, prev = 0;
        if (g > 0 && g < (uint32_t)n) {                          // the byte in front of the run, then one step
            r = (g - 1) / (uint32_t)row_bytes;
            const uint32_t q = (g - 1) - r * (uint32_t)row_bytes;
            p = q / w;
            x = q - p * w;
            prev = (sample(r, x) >> (8 * (3 - p))) & 0xFF;
            if (++x == w) { x = 0; if (++p == 4) { p = 0; ++r; } }
        }
        uint32_t out = 0;
        for (int j = 0; j < 4; ++j) {
            if (g + j >= (uint32_t)n) break;                     // zero past n
            const uint32_t cur = (sample(r, x) >> (8 * (3 - p))) & 0xFF;
            out |= (((p | x) ? cur - prev : cur) & 0xFF) << (8 * j);     // the first byte of a row passes through
            prev = cur;
            if (++x == w) { x = 0; if (++p == 4) { p = 0; ++r; } }
        }
        in32[i >> 2] = out;
    }
    lzw_sync();
}

LZW_HD inline void lzw_clear(LzwWorkspace* ws, int lane, int nlanes) {
    for (int i = lane; i < LZW_SLOTS; i += nlanes) ws->tab[i] = LZW_EMPTY;
    lzw_sync();
}

// Output bytes [from, to) of the ring to dst, those below cap only.
LZW_HD inline void lzw_store(const LzwWorkspace* ws, uint8_t* dst, int64_t from, int64_t to, int64_t cap, int lane, int nlanes) {
    lzw_sync();
    for (int64_t i = from + lane; i < to; i += nlanes)
        if (i < cap) dst[i] = ws->stage[i & (LZW_STAGE - 1)];
    lzw_sync();
}

// The automaton: encodes the n bytes (n >= 0) that ``fetch(base)`` puts into ws->in, LZW_CHUNK at a time, to dst[0 .. cap).
// Returns the stream's byte count, or -1 when it exceeds cap; no byte at or beyond dst + cap is written either way.  Every
// lane of the nlanes that call it together gets the same result.
template <class Fetch>
LZW_HD inline int32_t lzw_encode_stream(LzwWorkspace* ws, int32_t n, Fetch fetch, uint8_t* dst, int32_t cap, int lane, int nlanes) {
    uint64_t bitbuf = 0;
    int nbits = 0, width = 9, next = 258;
    int64_t op = 0, stored = 0;                // bytes produced / bytes handed to lzw_store
    const int64_t capl = cap > 0 ? cap : 0;

    // a code of `width` bits behind the pending bits; whole bytes go to the ring (at most 2: nbits < 8 before)
#define LZW_PUT(code)                                                                        \
    do {                                                                                     \
        bitbuf = (bitbuf << width) | (uint32_t)(code);                                       \
        nbits += width;                                                                      \
        for (int q_ = 0; q_ < 2 && nbits >= 8; ++q_) {                                       \
            ws->stage[op & (LZW_STAGE - 1)] = (uint8_t)(bitbuf >> (nbits - 8));               \
            ++op;                                                                            \
            nbits -= 8;                                                                      \
        }                                                                                    \
        if (op - stored >= 256) {                                                            \
            lzw_store(ws, dst, stored, stored + 256, capl, lane, nlanes);                    \
            stored += 256;                                                                   \
        }                                                                                    \
    } while (0)

    lzw_clear(ws, lane, nlanes);
    LZW_PUT(256);
    int cur = 0;
    bool overflow = false;
    for (int64_t base = 0; base < n && !overflow; base += LZW_CHUNK) {
        fetch(base);
        const int m = n - base < LZW_CHUNK ? (int)(n - base) : LZW_CHUNK;
        const uint32_t* in32 = reinterpret_cast<const uint32_t*>(ws->in);
        uint32_t word = lzw_uniform(in32[0]);
        int i = 0;
        if (base == 0) cur = (int)(word & 0xFF), i = 1;
        for (; i < m; ++i) {
            if ((i & 3) == 0) word = lzw_uniform(in32[i >> 2]);
            const uint32_t c = (word >> (8 * (i & 3))) & 0xFF;
            const uint32_t key = ((uint32_t)cur << 8) | c;
            uint32_t h = (key * 2654435761u) >> 19;            // 13 bits
            uint32_t slot = LZW_EMPTY;
            for (int t = 0; t < LZW_SLOTS; ++t) {
                slot = lzw_uniform(ws->tab[h]);
                if (slot == LZW_EMPTY || (slot >> 12) == key) break;
                h = (h + 1) & (LZW_SLOTS - 1);
            }
            if (slot != LZW_EMPTY && (slot >> 12) == key) { cur = (int)(slot & 0xFFF); continue; }
            LZW_PUT(cur);
            if (slot == LZW_EMPTY) ws->tab[h] = (key << 12) | (uint32_t)next;   // (a full table cannot happen: load <= 0.47)
            ++next;
            if (next == 512 || next == 1024 || next == 2048) ++width;
            if (next == 4095) {
                LZW_PUT(256);
                lzw_clear(ws, lane, nlanes);
                next = 258;
                width = 9;
            }
            cur = (int)c;
        }
        overflow = op > capl;                  // the result is decided; what follows would only be dropped
    }
    if (n > 0) {
        LZW_PUT(cur);
        ++next;
        if (next == 512 || next == 1024 || next == 2048) ++width;
    }
    LZW_PUT(257);
    if (nbits) {
        ws->stage[op & (LZW_STAGE - 1)] = (uint8_t)((bitbuf << (8 - nbits)) & 0xFF);
        ++op;
    }
    lzw_store(ws, dst, stored, op, capl, lane, nlanes);
#undef LZW_PUT
    return op > capl ? -1 : (int32_t)op;
}

// Encodes the n bytes at src (n >= 0) to dst[0 .. cap): lzw_encode_stream of what lzw_fetch reads.
LZW_HD inline int32_t lzw_encode_strip(LzwWorkspace* ws, const uint8_t* src, int32_t n, int32_t sample_bytes, int32_t row_bytes,
                                       uint8_t* dst, int32_t cap, int lane, int nlanes) {
    return lzw_encode_stream(
        ws, n, [=](int64_t base) { lzw_fetch(ws, src, n, base, sample_bytes, row_bytes, lane, nlanes); }, dst, cap, lane, nlanes);
}

// Encodes a block of block_h rows of block_w_bytes bytes read in place from a raster (LzwBlock) to dst[0 .. cap):
// lzw_encode_stream of what lzw_fetch_block reads, so the stream is lzw_encode_strip's of the padded block laid out contiguous
// with row_bytes = block_w_bytes.  block_w_bytes * block_h <= 2^30.
LZW_HD inline int32_t lzw_encode_block(LzwWorkspace* ws, const LzwBlock& blk, int32_t block_h, int32_t sample_bytes, uint8_t* dst,
                                       int32_t cap, int lane, int nlanes) {
    return lzw_encode_stream(
        ws, blk.block_w_bytes * block_h, [=](int64_t base) { lzw_fetch_block(ws, blk, base, sample_bytes, lane, nlanes); }, dst,
        cap, lane, nlanes);
}

// lzw_encode_strip with the floating-point predictor (lzw_fetch_fp): the n bytes at src are whole rows of row_bytes bytes of
// float32 samples, row_bytes a positive multiple of 4; a sample that does not lie whole inside the n bytes counts as zero.
LZW_HD inline int32_t lzw_encode_strip_fp(LzwWorkspace* ws, const uint8_t* src, int32_t n, int32_t row_bytes, uint8_t* dst,
                                          int32_t cap, int lane, int nlanes) {
    const bool aligned = (reinterpret_cast<uintptr_t>(src) & 3) == 0;       // of every row: row_bytes is a multiple of 4
    const auto sample = [=](uint32_t r, uint32_t x) -> uint32_t {
        const int64_t row = (int64_t)r * row_bytes;
        return row + 4 * (int64_t)x + 4 <= n ? lzw_fp_sample(src + row, x, aligned) : 0u;
    };
    return lzw_encode_stream(
        ws, n, [=](int64_t base) { lzw_fetch_fp(ws, n, base, row_bytes, sample, lane, nlanes); }, dst, cap, lane, nlanes);
}

// lzw_encode_block with the floating-point predictor: LzwBlock's geometry with block_w_bytes a positive multiple of 4.  A
// sample is zero unless it lies whole inside the valid part: the padding is in place before the predictor, which restarts on
// every block row; row offsets are y * pitch in 64-bit.  The stream is lzw_encode_strip_fp's of the padded block laid out
// contiguous with row_bytes = block_w_bytes.
LZW_HD inline int32_t lzw_encode_block_fp(LzwWorkspace* ws, const LzwBlock& blk, int32_t block_h, uint8_t* dst, int32_t cap,
                                          int lane, int nlanes) {
    const bool aligned = ((reinterpret_cast<uintptr_t>(blk.src) | (uint64_t)blk.pitch) & 3) == 0;
    const auto sample = [=](uint32_t y, uint32_t x) -> uint32_t {
        return (y < (uint32_t)blk.valid_rows && 4 * (int64_t)x + 4 <= blk.valid_w_bytes)
                   ? lzw_fp_sample(blk.src + (int64_t)y * blk.pitch, x, aligned) : 0u;
    };
    const int32_t n = blk.block_w_bytes * block_h;
    return lzw_encode_stream(
        ws, n, [=](int64_t base) { lzw_fetch_fp(ws, n, base, blk.block_w_bytes, sample, lane, nlanes); }, dst, cap, lane, nlanes);
}

}  // namespace msr
