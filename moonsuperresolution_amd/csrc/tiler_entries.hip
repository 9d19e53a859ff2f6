// tiler_entries.hip — the C entries of the tiler / stitcher kernels (tiler.hip): patch statistics, extraction, compaction,
// resizes, the blend window and the stitch / halo-merge passes.
#include "host.h"

using namespace msr;

extern "C" {

int msr_patch_stats(msr_handle* h, const float* img, const float* dem, int32_t rows, int32_t cols, const int32_t* ox,
                    const int32_t* oy, int32_t n, float no_value, uint8_t* valid, float* minmax, void* stream) {
    if (!h) return MSR_ERR_INVALID;
    if (!img || !dem || !ox || !oy || !valid || !minmax || n < 0 || rows <= 0 || cols <= 0)
        return fail(h, MSR_ERR_INVALID, "msr_patch_stats: bad argument");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, launch_patch_stats(img, dem, rows, cols, ox, oy, n, h->S, no_value, valid, minmax, (hipStream_t)stream));
    return MSR_OK;
}

int msr_extract_patches(msr_handle* h, const float* img, const float* dem, int32_t rows, int32_t cols,
                        const int32_t* ox, const int32_t* oy, const float* minmax, int32_t n, float* out,
                        void* stream) {
    if (!h) return MSR_ERR_INVALID;
    if (!img || !dem || !ox || !oy || !minmax || !out || n < 0)
        return fail(h, MSR_ERR_INVALID, "msr_extract_patches: bad argument");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, launch_extract_patches(img, dem, rows, cols, ox, oy, minmax, n, h->S, out, (hipStream_t)stream));
    return MSR_OK;
}

int msr_compact_patches(msr_handle* h, const uint8_t* valid, const int32_t* ox, const int32_t* oy, const float* minmax,
                        int32_t n, int32_t tile_x, int32_t tile_y, int32_t batch, int32_t cap, int32_t* sel_x,
                        int32_t* sel_y, float* sel_mm, int32_t* key, float* dmm, int32_t* meta, void* stream) {
    if (!h) return MSR_ERR_INVALID;
    if (!valid || !ox || !oy || !minmax || !sel_x || !sel_y || !sel_mm || !key || !dmm || !meta || n < 0 || batch < 1)
        return fail(h, MSR_ERR_INVALID, "msr_compact_patches: bad argument");
    if (cap < (n + batch - 1) / batch * batch)
        return fail(h, MSR_ERR_INVALID, "msr_compact_patches: cap %d < ceil(%d / %d) * %d", cap, n, batch, batch);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, launch_compact_patches(valid, ox, oy, minmax, n, tile_x, tile_y, batch, cap, sel_x, sel_y, sel_mm, key, dmm,
                                     meta, (hipStream_t)stream));
    return MSR_OK;
}

int msr_compact_patches_carry(msr_handle* h, const uint8_t* valid, const int32_t* ox, const int32_t* oy, const float* minmax,
                              int32_t n, int32_t tile_x, int32_t tile_y, int32_t batch, int32_t cap, int32_t carry_n,
                              int32_t* sel_x, int32_t* sel_y, float* sel_mm, int32_t* key, float* dmm, int32_t* meta,
                              void* stream) {
    if (!h) return MSR_ERR_INVALID;
    if (!valid || !ox || !oy || !minmax || !sel_x || !sel_y || !sel_mm || !key || !dmm || !meta || n < 0 || batch < 1)
        return fail(h, MSR_ERR_INVALID, "msr_compact_patches_carry: bad argument");
    if (carry_n < 0 || carry_n >= batch)
        return fail(h, MSR_ERR_INVALID, "msr_compact_patches_carry: carry_n %d outside [0, %d)", carry_n, batch);
    const int64_t need = ((int64_t)carry_n + n + batch - 1) / batch * batch;
    if (cap < need)
        return fail(h, MSR_ERR_INVALID, "msr_compact_patches_carry: cap %d < ceil((%d + %d) / %d) * %d", cap, carry_n, n, batch,
                    batch);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, launch_compact_patches(valid, ox, oy, minmax, n, tile_x, tile_y, batch, cap, sel_x, sel_y, sel_mm, key, dmm,
                                     meta, (hipStream_t)stream, carry_n));
    return MSR_OK;
}

int msr_resize_area_rows(msr_handle* h, const float* src, int32_t src_row0, int32_t src_rows, int32_t full_rows,
                         int32_t cols, int32_t factor, float* dst, int32_t dst_row0, int32_t dst_rows, int32_t dst_cols,
                         float no_value, int32_t flags, void* stream) {
    if (!h) return MSR_ERR_INVALID;
    if (!src || !dst || src_row0 < 0 || src_rows <= 0 || full_rows <= 0 || src_rows > full_rows - src_row0 || cols <= 0 ||
        factor < 1 || dst_row0 < 0 || dst_rows <= 0 || dst_cols <= 0 ||
        (flags & ~(MSR_RESIZE_NODATA_TO_NAN | MSR_RESIZE_NAN_TO_NODATA)))
        return fail(h, MSR_ERR_INVALID, "msr_resize_area_rows: bad argument");
    if ((int64_t)dst_row0 + dst_rows > INT32_MAX / factor)
        return fail(h, MSR_ERR_INVALID, "msr_resize_area_rows: destination rows x factor exceed int32");
    const RowWindow win{src_row0, src_rows, full_rows, dst_row0, dst_rows, 0};
    long lo, hi;
    resize_area_needs(win, factor, &lo, &hi);
    if (hi > lo && (lo < src_row0 || hi > (long)src_row0 + src_rows))
        return fail(h, MSR_ERR_INVALID, "msr_resize_area_rows: destination rows [%d, %d) read source rows [%ld, %ld), the "
                    "window holds [%d, %d)", dst_row0, dst_row0 + dst_rows, lo, hi, src_row0, src_row0 + src_rows);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, launch_resize_area(src, win, cols, dst, dst_cols, factor, no_value, flags, (hipStream_t)stream));
    return MSR_OK;
}

int msr_resize_cubic_rows(msr_handle* h, const float* src, int32_t src_row0, int32_t src_rows, int32_t full_src_rows,
                          int32_t cols, float* dst, int32_t dst_row0, int32_t dst_rows, int32_t full_dst_rows,
                          int32_t dst_cols, float no_value, int32_t flags, void* stream) {
    if (!h) return MSR_ERR_INVALID;
    if (!src || !dst || src_row0 < 0 || src_rows <= 0 || full_src_rows <= 0 || src_rows > full_src_rows - src_row0 ||
        cols <= 0 || dst_row0 < 0 || dst_rows <= 0 || full_dst_rows <= 0 || dst_rows > full_dst_rows - dst_row0 ||
        dst_cols <= 0 || (flags & ~(MSR_RESIZE_NODATA_TO_NAN | MSR_RESIZE_NAN_TO_NODATA)))
        return fail(h, MSR_ERR_INVALID, "msr_resize_cubic_rows: bad argument");
    const RowWindow win{src_row0, src_rows, full_src_rows, dst_row0, dst_rows, full_dst_rows};
    long lo, hi;
    resize_cubic_needs(win, &lo, &hi);
    if (lo < src_row0 || hi > (long)src_row0 + src_rows)
        return fail(h, MSR_ERR_INVALID, "msr_resize_cubic_rows: destination rows [%d, %d) read source rows [%ld, %ld), the "
                    "window holds [%d, %d)", dst_row0, dst_row0 + dst_rows, lo, hi, src_row0, src_row0 + src_rows);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, launch_resize_cubic(src, win, cols, dst, dst_cols, no_value, flags, (hipStream_t)stream));
    return MSR_OK;
}

// The whole-raster forms: the window is the raster.
int msr_resize_area(msr_handle* h, const float* src, int32_t rows, int32_t cols, int32_t factor, float* dst,
                    int32_t dst_rows, int32_t dst_cols, void* stream) {
    if (!h) return MSR_ERR_INVALID;
    if (!src || !dst || rows <= 0 || cols <= 0 || factor < 1 || dst_rows <= 0 || dst_cols <= 0)
        return fail(h, MSR_ERR_INVALID, "msr_resize_area: bad argument");
    return msr_resize_area_rows(h, src, 0, rows, rows, cols, factor, dst, 0, dst_rows, dst_cols, 0.f, 0, stream);
}

int msr_resize_cubic(msr_handle* h, const float* src, int32_t rows, int32_t cols, float* dst, int32_t dst_rows,
                     int32_t dst_cols, void* stream) {
    if (!h) return MSR_ERR_INVALID;
    if (!src || !dst || rows <= 0 || cols <= 0 || dst_rows <= 0 || dst_cols <= 0)
        return fail(h, MSR_ERR_INVALID, "msr_resize_cubic: bad argument");
    return msr_resize_cubic_rows(h, src, 0, rows, rows, cols, dst, 0, dst_rows, dst_rows, dst_cols, 0.f, 0, stream);
}

int msr_set_blend_window(msr_handle* h, const double* host_window, int32_t side) {
    if (!h) return MSR_ERR_INVALID;
    const int ws = h->S - 2 * (h->S / 16);
    if (!host_window || side != ws) return fail(h, MSR_ERR_INVALID, "blend window must be [%d,%d] float64", ws, ws);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!h->window) HIPCHK(h, hipMalloc(&h->window, (size_t)ws * ws * sizeof(double)));
    HIPCHK(h, hipMemcpy(h->window, host_window, (size_t)ws * ws * sizeof(double), hipMemcpyHostToDevice));
    return MSR_OK;
}

static int default_window(msr_handle* h) {
    // makeGaussianKernel (process_full_tiles.py:347-361) + 1e-7, purged (:391-393), in float64 like NumPy.
    const int S = h->S, p = S / 16, ws = S - 2 * p;
    std::vector<double> ax(S), k((size_t)S * S);
    const double start = -S / 2.0, stop = S / 2.0, step = (stop - start) / (S - 1);
    for (int i = 0; i < S; ++i) ax[i] = i * step + start;
    ax[S - 1] = stop;
    const double sx = S / 5.0;
    double mn = INFINITY, mx = -INFINITY;
    for (int y = 0; y < S; ++y)
        for (int x = 0; x < S; ++x) {
            const double v = 1.0 / (2.0 * M_PI * sx * sx) *
                             std::exp(-(std::pow(ax[x] - 0, 2.0) / (2.0 * std::pow(sx, 2.0)) +
                                        std::pow(ax[y] - 0, 2.0) / (2.0 * std::pow(sx, 2.0))));
            k[(size_t)y * S + x] = v;
            mn = std::min(mn, v); mx = std::max(mx, v);
        }
    std::vector<double> w((size_t)ws * ws);
    for (int y = 0; y < ws; ++y)
        for (int x = 0; x < ws; ++x) w[(size_t)y * ws + x] = (k[(size_t)(y + p) * S + x + p] - mn) / (mx - mn) + 1e-7;
    return msr_set_blend_window(h, w.data(), ws);
}

static int stitch_impl(msr_handle* h, const float* pred, const int32_t* key, const float* dmm, int32_t n,
                       int32_t tile_size, int32_t stride, float no_value, int32_t as_implemented, float* mean,
                       float* stdv, uint8_t* good, float* wsum_partial, void* stream, int pitch = 0, int resume = 0) {
    if (tile_size <= 0 || stride <= 0 || stride > h->S)
        return fail(h, MSR_ERR_INVALID, "msr_stitch_tile: tile_size %d / stride %d invalid for image_size %d", tile_size,
                    stride, h->S);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!h->window) { int rc = default_window(h); if (rc) return rc; }
    const int NG = (tile_size + h->S - 1) / stride;
    if (NG * NG > h->stitch_grid_cap) {
        if (h->stitch_grid) HIPCHK(h, hipFree(h->stitch_grid));
        HIPCHK(h, hipMalloc(&h->stitch_grid, (size_t)NG * NG * sizeof(int)));
        h->stitch_grid_cap = NG * NG;
    }
    HIPCHK(h, launch_stitch_tile(pred, key, dmm, n, h->S, tile_size, stride, no_value, as_implemented, h->window,
                                 h->stitch_grid, mean, stdv, good, (hipStream_t)stream, wsum_partial, pitch, resume));
    return MSR_OK;
}

int msr_stitch_tile(msr_handle* h, const float* pred, const int32_t* key, const float* dmm, int32_t n,
                    int32_t tile_size, int32_t stride, float no_value, int32_t as_implemented, float* mean,
                    float* stdv, uint8_t* good, void* stream) {
    if (!h) return MSR_ERR_INVALID;
    if (!mean || !stdv || !good || n < 0 || (n > 0 && (!pred || !key || !dmm)))
        return fail(h, MSR_ERR_INVALID, "msr_stitch_tile: null pointer");
    return stitch_impl(h, pred, key, dmm, n, tile_size, stride, no_value, as_implemented, mean, stdv, good, nullptr, stream);
}

int msr_stitch_partial(msr_handle* h, const float* pred, const int32_t* key, const float* dmm, int32_t n,
                       int32_t tile_size, int32_t stride, float* wsum, float* mean, float* s_acc, void* stream) {
    if (!h) return MSR_ERR_INVALID;
    if (!wsum || !mean || !s_acc || n < 0 || (n > 0 && (!pred || !key || !dmm)))
        return fail(h, MSR_ERR_INVALID, "msr_stitch_partial: null pointer");
    return stitch_impl(h, pred, key, dmm, n, tile_size, stride, 0.f, /*as_implemented=*/0, mean, s_acc, nullptr, wsum, stream);
}

int msr_stitch_accumulate(msr_handle* h, const float* pred, const int32_t* key, const float* dmm, int32_t n,
                          int32_t tile_size, int32_t stride, float* wsum, float* mean, float* s_acc, int32_t pitch,
                          int32_t resume, void* stream) {
    if (!h) return MSR_ERR_INVALID;
    if (!wsum || !mean || !s_acc || n < 0 || pitch < tile_size || (n > 0 && (!pred || !key || !dmm)))
        return fail(h, MSR_ERR_INVALID, "msr_stitch_accumulate: bad argument (pitch >= tile_size)");
    return stitch_impl(h, pred, key, dmm, n, tile_size, stride, 0.f, /*as_implemented=*/0, mean, s_acc, nullptr, wsum, stream,
                       pitch, resume ? 1 : 0);
}

int msr_stitch_accumulate_band(msr_handle* h, const float* pred, const int32_t* key, const float* dmm, int32_t n,
                               int32_t stride, int32_t grid_x0, int32_t grid_y0, int32_t ngx, int32_t ngy, int32_t* grid_ws,
                               float* wsum, float* mean, float* s_acc, int32_t pitch, int32_t acc_row0, int32_t row_lo,
                               int32_t row_hi, int32_t width, void* stream) {
    if (!h) return MSR_ERR_INVALID;
    if (!wsum || !mean || !s_acc || !grid_ws || n < 0 || (n > 0 && (!pred || !key || !dmm)))
        return fail(h, MSR_ERR_INVALID, "msr_stitch_accumulate_band: null pointer");
    if (stride <= 0 || stride > h->S)
        return fail(h, MSR_ERR_INVALID, "msr_stitch_accumulate_band: stride %d invalid for image_size %d", stride, h->S);
    if (ngx <= 0 || ngy <= 0 || (int64_t)ngx * ngy > INT32_MAX)
        return fail(h, MSR_ERR_INVALID, "msr_stitch_accumulate_band: patch grid %d x %d", ngx, ngy);
    if (width <= 0 || pitch < width)
        return fail(h, MSR_ERR_INVALID, "msr_stitch_accumulate_band: pitch %d < width %d", pitch, width);
    if (row_hi <= row_lo || row_lo < acc_row0)
        return fail(h, MSR_ERR_INVALID, "msr_stitch_accumulate_band: rows [%d, %d) empty, inverted or above the slab's row %d",
                    row_lo, row_hi, acc_row0);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!h->window) { int rc = default_window(h); if (rc) return rc; }
    HIPCHK(h, launch_stitch_accumulate_band(pred, key, dmm, n, h->S, stride, grid_x0, grid_y0, ngx, ngy, grid_ws, h->window,
                                            wsum, mean, s_acc, pitch, acc_row0, row_lo, row_hi, width, (hipStream_t)stream));
    return MSR_OK;
}

int msr_halo_merge(msr_handle* h, const float* wa, const float* ma, const float* sa, const float* wb, const float* mb,
                   const float* sb, int64_t count, float no_value, float* mean, float* stdv, uint8_t* good,
                   void* stream) {
    if (!h) return MSR_ERR_INVALID;
    if (!wa || !ma || !sa || !mean || !stdv || !good || count < 0 || (wb && (!mb || !sb)))
        return fail(h, MSR_ERR_INVALID, "msr_halo_merge: bad argument");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, launch_halo_merge(wa, ma, sa, wb, mb, sb, (long)count, no_value, mean, stdv, good, (hipStream_t)stream));
    return MSR_OK;
}

}  // extern "C"
