// infill.hip — msr_infill_small_holes: the no-data in-filling of preprocess on the device (preprocess(infill="device")).
// The contract is in include/moonsr.h, the arithmetic of one component in infill_solve.h.
//
// Stage 1 (infill_label_kernel, one thread per pixel, one wave per 64 consecutive pixels of a row) writes the hole bitmap and
// finds the components to fill.  A hole none of whose W / NW / N / NE neighbours is a hole may be the first pixel (row-major)
// of its component; such a thread floods from it over at most max_area - 1 pixels and gives up at an earlier pixel or at the
// max_area-th.  No two such pixels are 8-neighbours, so there are at most ceil(rows / 2) * ceil(cols / 2) of them: the
// capacity of the list.  A component with a pixel in the fill set appends its first pixel to the list (atomic counter: the
// components are independent, the order does not reach the output).
// Stage 2 (infill_solve_kernel, one one-wave workgroup per component) floods again from the first pixel, builds and solves
// (infill_solve.h) and stores at K ∩ F.  It tests holes on stage 1's bitmap, never on the grid, and reads grid values of
// valid pixels only: no wave reads a pixel another one stores, whatever the order (two components one valid pixel apart
// share a ring pixel, whose equation neither may use).
#include "host.h"
#include "infill_solve.h"

using namespace msr;

namespace {

struct InfillArgs {
    float* g;
    int32_t row0, n_rows, full_rows, cols;
    float no_value;
    int32_t max_area, margin;
    int32_t words;              // 64-bit words of a bitmap row
    int32_t cap;                // entries of `first`
    int32_t* count;             // workspace: [0, 16) the counter
    uint64_t* holes;            //            [16, 16 + 8 rows words) the bitmap
    int32_t* first;             //            then cap first-pixel indices r * cols + c
};

__global__ __launch_bounds__(256) void infill_label_kernel(InfillArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);       // wave-uniform
    if (item >= (int64_t)a.n_rows * a.words) return;
    const int r = (int)(item / a.words), wd = (int)(item % a.words), c = wd * 64 + lane;
    const InfillGrid v{a.g, nullptr, a.n_rows, a.cols, a.words, a.no_value};
    const bool hole = c < a.cols && infill_hole(v, r, c);
    const uint64_t mask = __ballot(hole);
    if (lane == 0) a.holes[item] = mask;
    if (!hole) return;
    if ((c > 0 && infill_hole(v, r, c - 1)) ||
        (r > 0 && ((c > 0 && infill_hole(v, r - 1, c - 1)) || infill_hole(v, r - 1, c) ||
                   (c + 1 < a.cols && infill_hole(v, r - 1, c + 1)))))
        return;
    int32_t pr[INFILL_MAX_N], pc[INFILL_MAX_N];
    const int n = infill_flood(v, a.max_area, r, c, pr, pc);
    bool any = false;
    for (int i = 0; i < n; ++i) any |= infill_fillable(pr[i], pc[i], a.row0, a.n_rows, a.full_rows, a.cols, a.max_area, a.margin);
    if (!any) return;
    const int slot = atomicAdd(a.count, 1);
    if (slot >= 0 && slot < a.cap) a.first[slot] = r * a.cols + c;             // rows * cols <= INT32_MAX (entry)
}

__global__ __launch_bounds__(64) void infill_solve_kernel(InfillArgs a) {
    __shared__ InfillWork w;
    const int lane = threadIdx.x;
    const InfillGrid v{a.g, a.holes, a.n_rows, a.cols, a.words, a.no_value};
    int total = *a.count;
    total = total < a.cap ? total : a.cap;
    for (int k = blockIdx.x; k < total; k += gridDim.x) {
        const int32_t p = a.first[k];
        if (lane == 0) w.n = p >= 0 ? infill_flood(v, a.max_area, p / a.cols, p % a.cols, w.pr, w.pc) : 0;
        __syncthreads();
        const int n = w.n;
        if (n > 0) {
            infill_solve_component(v, &w, lane, 64);
            if (lane < n && infill_fillable(w.pr[lane], w.pc[lane], a.row0, a.n_rows, a.full_rows, a.cols, a.max_area, a.margin))
                a.g[(int64_t)w.pr[lane] * a.cols + w.pc[lane]] = (float)w.b[lane];
        }
        __syncthreads();
    }
}

int64_t list_capacity(int32_t n_rows, int32_t cols) { return (int64_t)((n_rows + 1) / 2) * ((cols + 1) / 2); }
int32_t bitmap_words(int32_t cols) { return (cols + 63) / 64; }

// stages: 1 = label, 2 = solve (which reads what a label pass on the same arguments left in the workspace)
int run(msr_handle* h, const char* what, float* grid_dev, int32_t row0, int32_t n_rows, int32_t full_rows, int32_t cols,
        float no_value, int32_t max_area, int32_t margin, void* workspace_dev, int64_t workspace_bytes, void* stream, int stages) {
    if (!grid_dev) return fail(h, MSR_ERR_INVALID, "%s: grid_dev is null", what);
    if (!workspace_dev) return fail(h, MSR_ERR_INVALID, "%s: workspace_dev is null", what);
    if (n_rows <= 0 || full_rows <= 0 || cols <= 0)
        return fail(h, MSR_ERR_INVALID, "%s: n_rows %d, full_rows %d and cols %d must be positive", what, n_rows, full_rows, cols);
    if (max_area < 2 || max_area > INFILL_MAX_AREA)
        return fail(h, MSR_ERR_INVALID, "%s: max_area %d outside [2, %d]", what, max_area, INFILL_MAX_AREA);
    if (margin < max_area + 1) return fail(h, MSR_ERR_INVALID, "%s: margin %d < max_area + 1 = %d", what, margin, max_area + 1);
    if (row0 < 0 || n_rows > full_rows - row0)
        return fail(h, MSR_ERR_INVALID, "%s: row0 %d, n_rows %d: rows [%d, %lld) are not rows of a grid of full_rows %d", what, row0,
                    n_rows, row0, (long long)row0 + n_rows, full_rows);
    if ((int64_t)n_rows * cols > INT32_MAX)
        return fail(h, MSR_ERR_INVALID, "%s: n_rows %d x cols %d exceed 2^31 - 1 pixels: use row windows", what, n_rows, cols);
    const int64_t need = msr_infill_workspace_bytes(n_rows, cols);
    if (workspace_bytes < need)
        return fail(h, MSR_ERR_INVALID, "%s: workspace_bytes %lld < %lld (msr_infill_workspace_bytes)", what,
                    (long long)workspace_bytes, (long long)need);
    if ((uintptr_t)workspace_dev % 8) return fail(h, MSR_ERR_INVALID, "%s: workspace_dev is not 8-byte aligned", what);
    InfillArgs a{};
    a.g = grid_dev;
    a.row0 = row0; a.n_rows = n_rows; a.full_rows = full_rows; a.cols = cols;
    a.no_value = no_value; a.max_area = max_area; a.margin = margin;
    a.words = bitmap_words(cols);
    a.cap = (int32_t)list_capacity(n_rows, cols);
    a.count = (int32_t*)workspace_dev;
    a.holes = (uint64_t*)((char*)workspace_dev + 16);
    a.first = (int32_t*)((char*)workspace_dev + 16 + 8 * (int64_t)n_rows * a.words);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (h) HIPCHK(h, hipSetDevice(h->cfg.device));
    if (stages & 1) {
        HIPCHK(h, hipMemsetAsync(workspace_dev, 0, 16, s));
        const int64_t items = (int64_t)n_rows * a.words;
        hipLaunchKernelGGL(infill_label_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, s, a);
        HIPCHK(h, hipGetLastError());
    }
    if (stages & 2) {
        const int blocks = (int)std::min<int64_t>(a.cap, 256 * 16);
        hipLaunchKernelGGL(infill_solve_kernel, dim3(blocks), dim3(64), 0, s, a);
        HIPCHK(h, hipGetLastError());
    }
    return MSR_OK;
}

}  // namespace

extern "C" {

int64_t msr_infill_workspace_bytes(int32_t n_rows, int32_t cols) {
    if (n_rows <= 0 || cols <= 0 || (int64_t)n_rows * cols > INT32_MAX) return -1;
    return 16 + 8 * (int64_t)n_rows * bitmap_words(cols) + 4 * list_capacity(n_rows, cols);
}

int msr_infill_small_holes(msr_handle* h, float* grid_dev, int32_t row0, int32_t n_rows, int32_t full_rows, int32_t cols,
                           float no_value, int32_t max_area, int32_t margin, void* workspace_dev, int64_t workspace_bytes,
                           void* stream) {
    return run(h, "msr_infill_small_holes", grid_dev, row0, n_rows, full_rows, cols, no_value, max_area, margin, workspace_dev,
               workspace_bytes, stream, 3);
}

int msr_debug_infill_stage(msr_handle* h, float* grid_dev, int32_t row0, int32_t n_rows, int32_t full_rows, int32_t cols,
                           float no_value, int32_t max_area, int32_t margin, void* workspace_dev, int64_t workspace_bytes,
                           void* stream, int32_t stage) {
    if (stage != 1 && stage != 2) return fail(h, MSR_ERR_INVALID, "msr_debug_infill_stage: stage %d is not 1 or 2", stage);
    return run(h, "msr_debug_infill_stage", grid_dev, row0, n_rows, full_rows, cols, no_value, max_area, margin, workspace_dev,
               workspace_bytes, stream, stage);
}

}  // extern "C"
