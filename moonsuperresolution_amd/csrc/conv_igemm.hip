// conv_igemm — the front door of the NHWC implicit-GEMM convolutions for gfx950: tile geometry, the tile and K-split pickers,
// the LDS-attribute setup and the switch from a form's kernel to its launcher (launch_conv).  The kernels live one per unit
// (conv_generic, conv_bvgpr, conv_halo, conv_pp, conv_sw; split-K pass and moment slabs in conv_splitk), what they share in
// conv_common.h and conv_epilogue.h.
#include "conv_common.h"

namespace msr {

void conv_walk_pick(int tiles_m, int tiles_n, int* walk_pb, int* walk_nb) {
    *walk_pb = 1;
    *walk_nb = tiles_n;
    if (switches().tile_walk && tiles_n > 4 && tiles_n % 4 == 0 && tiles_m % 8 == 0) { *walk_pb = 8; *walk_nb = 4; }
}
void conv_walk(TileGeom& g) { conv_walk_pick(g.tiles_x * g.tiles_y * g.tiles_b, g.tiles_n, &g.walk_pb, &g.walk_nb); }

hipError_t conv_igemm_init() {
    hipError_t e;
    if ((e = set_attr_pp()) != hipSuccess) return e;
    if ((e = set_attr_halo()) != hipSuccess) return e;
    if ((e = conv_sw_init()) != hipSuccess) return e;
    if ((e = set_attr_generic()) != hipSuccess) return e;
    return set_attr_bvgpr();
}

static int ilog2_floor(int v) {
    int l = 0;
    while ((2 << l) <= v) ++l;
    return l;
}

bool make_geom(const ConvParams& p, int BM, int BN, int BKC, TileGeom& g) {
    auto pow2 = [](int v) { return v > 0 && (v & (v - 1)) == 0; };
    if (!pow2(p.Hout) || !pow2(p.Wout)) return false;
    if (p.N % BN || p.Cin % BKC) return false;
    int tw = p.Wout < 16 ? p.Wout : 16;
    if (tw > BM) tw = BM;
    int th = BM / tw;
    if (th > p.Hout) th = p.Hout;
    int tb = BM / (tw * th);
    g.tw_l = ilog2_floor(tw);
    g.th_l = ilog2_floor(th);
    g.tb = tb;
    g.tiles_x = p.Wout / tw;
    g.tiles_y = p.Hout / th;
    g.tiles_b = (p.B + tb - 1) / tb;
    g.tiles_n = p.N / BN;
    g.tiles_mn = g.tiles_x * g.tiles_y * g.tiles_b * g.tiles_n;
    g.walk_pb = 1;
    g.walk_nb = g.tiles_n;
    return true;
}

int conv_stat_slabs(const ConvParams& p, int tile) {
    const int bm = tile == TILE_64x64 ? 64 : 128, wm = 2;
    TileGeom g;
    if (!make_geom(p, bm, bm, tile == TILE_128x128_K16 ? 16 : 32, g)) return 0;
    return g.tiles_x * g.tiles_y * g.tiles_b * wm;
}

int persistent_grid(int items) {
    static int n_cu = 0;
    if (!n_cu) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
        n_cu = prop.multiProcessorCount & ~7;
        if (n_cu < 8) n_cu = 8;
    }
    return items < n_cu ? (items + 7) & ~7 : n_cu;
}

int conv_pick_tile(int M, int N, int epilogue, int prec, int ksteps) {
    // The big tile needs >= ~2 waves of workgroups per CU to hide its barrier; otherwise take the small one.
    // Measured on MI355X (tools/gpu_conv_bench.py): the 16-channel K-step (3 workgroups per CU) is ~8 % faster
    // than the 32-channel one for the SPADE epilogue (its long epilogue is covered by a third resident
    // workgroup) and ~3 % slower for plain long-K convs.
    // At bf16 rates the 128 x 128 tile is 1.6x as efficient as the 64 x 64 one, so one workgroup per CU is enough.
    const long big_blocks = (long)((M + 127) / 128) * (N / 128);
    if (N % 128 == 0 && big_blocks >= (prec == PREC_BF16X3 ? 256 : 512))
        return (epilogue == EPI_SPADE && prec == PREC_F32) ? TILE_128x128_K16 : TILE_128x128;
    // Few pixels, long K (the r <= 8 main convs, r = 16 at small batch): these layers stream their weights, and the
    // 128-row tile reads each weight for twice as many pixels; split-K (>= 72 K-steps) supplies the workgroups.
    // tools/gpu_smalltile_sweep.py: 93 -> 70 us (B=16, r=8, 1024 -> 1024), 171 -> 120 us (B=8, r=16).
    if (prec == PREC_BF16X3 && N % 128 == 0 && M >= 128 && ksteps >= 72 && big_blocks * 16 >= 256) return TILE_128x128;
    return TILE_64x64;
}

int conv_pick_ksplit(int M, int N, int ksteps, int tile, int prec) {
    // Low-resolution layers (M = B*r*r of a few hundred pixels) do not produce enough tiles to fill 256 CUs:
    // cut K so that about 1024 small (512 big) workgroups exist.  Every range keeps >= 4 K-steps.
    const int bm = tile == TILE_64x64 ? 64 : 128;
    const long blocks = (long)((M + bm - 1) / bm) * (N / bm);
    long want = tile == TILE_64x64 ? 1024 : 512;
    // short K at bf16 rates (the gamma/beta convs, 36 K-steps): the split-K pass costs more than it buys beyond one
    // workgroup per CU (tools/gpu_smalltile_sweep.py: 28 vs 33 us at B=16, r=8)
    if (prec == PREC_BF16X3 && ksteps < 72) want = 256;
    int ks = 1;
    while (blocks * ks < want && ks < 16 && ksteps / (ks * 2) >= 4) ks *= 2;
    return ks;
}

hipError_t launch_conv(const ConvParams& p, int epilogue, int kernel, int tile, hipStream_t s) {
    switch (kernel) {
        case KERNEL_GENERIC: return launch_generic(p, epilogue, tile, s);
        case KERNEL_BVGPR: return launch_bvgpr(p, epilogue, tile, s);
        case KERNEL_HALO: return launch_halo(p, epilogue, 0, s);
        case KERNEL_HALO16: return launch_halo(p, epilogue, 1, s);
        case KERNEL_PP: return launch_pp(p, epilogue, s);
        case KERNEL_SW: return launch_conv_f16c_sw(p, epilogue, s);
    }
    return hipErrorInvalidValue;                      // conv_kernel_for's -1: no kernel has the form
}

}  // namespace msr
