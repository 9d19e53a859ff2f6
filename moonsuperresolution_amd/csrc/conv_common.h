// What more than one conv unit uses (conv_igemm.hip and the per-kernel units conv_generic / conv_bvgpr / conv_halo / conv_pp /
// conv_splitk / conv_sw / conv_gbr): vector types of the MFMA operands, the tile geometry, lane exchanges, and the host
// entry points the units call across files.  Not for the non-conv units.
#pragma once
#include "kernels.h"
#include <cstdlib>

namespace msr {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// MODE.FP16_OVFL on for the converting part of an epilogue only (kernels.h MSR_SATURATING_CONVERSIONS): the accumulators pass
// through the statement that sets the bit, so everything computed from them follows it; the statement that clears it orders
// the stores of the converted values before it ("memory"); nothing is scheduled across either.
__device__ __forceinline__ void msr_saturate_begin(f32x4 (&a)[4][4]) {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile(MSR_SATURATE_BEGIN_ASM
                 : "+v"(a[0][0]), "+v"(a[0][1]), "+v"(a[0][2]), "+v"(a[0][3]), "+v"(a[1][0]), "+v"(a[1][1]), "+v"(a[1][2]), "+v"(a[1][3]),
                   "+v"(a[2][0]), "+v"(a[2][1]), "+v"(a[2][2]), "+v"(a[2][3]), "+v"(a[3][0]), "+v"(a[3][1]), "+v"(a[3][2]), "+v"(a[3][3])
                 : : "memory");
}
__device__ __forceinline__ void msr_saturate_begin(f32x4 (&a)[16][2]) {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile(MSR_SATURATE_BEGIN_ASM
                 : "+v"(a[0][0]), "+v"(a[0][1]), "+v"(a[1][0]), "+v"(a[1][1]), "+v"(a[2][0]), "+v"(a[2][1]), "+v"(a[3][0]), "+v"(a[3][1]),
                   "+v"(a[4][0]), "+v"(a[4][1]), "+v"(a[5][0]), "+v"(a[5][1]), "+v"(a[6][0]), "+v"(a[6][1]), "+v"(a[7][0]), "+v"(a[7][1])
                 : : "memory");
    asm volatile("" : "+v"(a[8][0]), "+v"(a[8][1]), "+v"(a[9][0]), "+v"(a[9][1]), "+v"(a[10][0]), "+v"(a[10][1]), "+v"(a[11][0]), "+v"(a[11][1]),
                      "+v"(a[12][0]), "+v"(a[12][1]), "+v"(a[13][0]), "+v"(a[13][1]), "+v"(a[14][0]), "+v"(a[14][1]), "+v"(a[15][0]), "+v"(a[15][1]));
}
// the light form: four values that every conversion of the epilogue depends on (the SPADE epilogue's 1 / sigma)
__device__ __forceinline__ void msr_saturate_begin(float& a0, float& a1, float& a2, float& a3) {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile(MSR_SATURATE_BEGIN_ASM : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : : "memory");
}
__device__ __forceinline__ void msr_saturate_begin(f32x4& a0, f32x4& a1) {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile(MSR_SATURATE_BEGIN_ASM : "+v"(a0), "+v"(a1) : : "memory");
}
__device__ __forceinline__ void msr_saturate_end() {
    asm volatile(MSR_SATURATE_END_ASM ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void msr_saturate_end(f16x8& h, f16x8& l) {      // the converted values are consumed from registers
    asm volatile(MSR_SATURATE_END_ASM : "+v"(h), "+v"(l) : : "memory");
    __builtin_amdgcn_sched_barrier(0);
}
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x6 __attribute__((ext_vector_type(6)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));

// Workgroup barrier of the ping-pong kernel, spelled as what it is on gfx950: a workgroup-scope release (every LDS
// store of this wave has completed: s_waitcnt lgkmcnt(0)), the hardware s_barrier, a workgroup-scope acquire.  That is
// exactly what __syncthreads() lowers to, but the ping-pong schedule executes its barriers under WAVE-GROUP-dependent
// control flow (group Y runs one barrier more at the start and one fewer at the end), which __syncthreads() — defined
// for barriers every thread reaches at the same textual call — does not promise to support.  s_barrier itself only
// counts arrivals: it releases when every wave of the workgroup has executed one more s_barrier, wherever that
// instruction sits in its stream.  The counts are balanced by construction (table at the kernel).
#define MSR_WG_BARRIER()                                       \
    {                                                          \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); \
        __builtin_amdgcn_s_barrier();                          \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); \
    }

__device__ __forceinline__ int xcd_remap(int orig, int nwg) {
    // Blocks are dealt round-robin over the 8 XCDs; give each XCD a contiguous range of logical tiles so
    // that neighbouring tiles (same pixels, next channel block) share that XCD's L2.  Bijective for any nwg.
    const int q = nwg >> 3, r = nwg & 7, x = orig & 7;
    const int base = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    return base + (orig >> 3);
}

struct TileGeom {
    int th_l, tw_l, tb;            // log2 tile height/width, samples per tile
    int tiles_x, tiles_y, tiles_b, tiles_n;
    int tiles_mn;                  // tiles_x * tiles_y * tiles_b * tiles_n (the grid is ksplit times that)
    // Tile walk of the persistent kernels (conv_walk, conv_igemm.hip): consecutive tile numbers cover walk_nb channel blocks of
    // walk_pb pixel tiles before they move to the next channel blocks of the same pixel tiles.  (1, tiles_n) = channel
    // block fastest (the round-2 walk).
    int walk_pb, walk_nb;
};

__device__ __forceinline__ unsigned lane_xor1(unsigned v) {
    // neighbour exchange lane <-> lane ^ 1 in the VALU (DPP quad_perm [1,0,3,2]), no LDS crossbar
    return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);
}

// sum over the 16 lanes of a DPP row (here: the 16 pixels of a tile row), result in every lane; 4 VALU pairs
__device__ __forceinline__ float row16_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));  // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));  // row_mirror
    return v;
}

// Tile range of a workgroup of the persistent kernels (grid = persistent_grid(items): a multiple of 8).  Workgroups are dealt
// round-robin over the 8 XCDs, so XCD x owns the contiguous range [base, base + cnt) of the logical tiles (as xcd_remap) and
// its `slots` = gridDim.x / 8 workgroups take consecutive tiles of that range in every round, the first one at index
// blockIdx.x >> 3: the tiles in flight on an XCD share their halo (same pixels, next channel block) and weights in its L2.
__device__ __forceinline__ void xcd_tile_range(int items, int& slots, int& cnt, int& base) {
    const int xcd = blockIdx.x & 7;
    const int tq = items >> 3, tr = items & 7;
    slots = gridDim.x >> 3;
    cnt = tq + (xcd < tr ? 1 : 0);
    base = xcd < tr ? xcd * (tq + 1) : tr * (tq + 1) + (xcd - tr) * tq;
}

// ---- host: conv_igemm.hip ----
bool make_geom(const ConvParams& p, int BM, int BN, int BKC, TileGeom& g);   // false: the shape is not tileable
void conv_walk(TileGeom& g);                                                 // fills walk_pb / walk_nb (conv_walk_pick)
// Grid of a persistent kernel for `items` work items: one workgroup per CU, a multiple of 8 so that every XCD gets the same
// count (the CU count is read once, rounded down to a multiple of 8, at least 8).  0: the device query failed.
int persistent_grid(int items);
// ---- host: one launcher and one LDS-attribute setup per kernel unit ----
hipError_t set_attr_generic();                                                          // conv_generic.hip
hipError_t launch_generic(const ConvParams& p, int epi, int tile, hipStream_t s);
hipError_t set_attr_bvgpr();                                                            // conv_bvgpr.hip
hipError_t launch_bvgpr(const ConvParams& p, int epi, int tile, hipStream_t s);
hipError_t set_attr_halo();                                                             // conv_halo.hip
hipError_t launch_halo(const ConvParams& p, int epi, int sh, hipStream_t s);
hipError_t set_attr_pp();                                                               // conv_pp.hip
hipError_t launch_pp(const ConvParams& p, int epi, hipStream_t s);
hipError_t finish_splitk(const ConvParams& p, int epi, hipStream_t s);                  // conv_splitk.hip

}  // namespace msr
