// Host-only unit of libmoonsr_hip.so (no device code): the per-component build-and-solve of the device in-filling
// (infill_solve.h) with one lane on host buffers, so that the CPU suite and tools/infill_check.cpp can hold it against the
// NumPy twin and a dense solve without a GPU.  Compiled with -ffp-contract=off like the device units.
#include "../../include/moonsr.h"
#include "infill_solve.h"

extern "C" int32_t msr_infill_component_host(const float* grid, int32_t rows, int32_t cols, float no_value, const int32_t* pix_r,
                                             const int32_t* pix_c, int32_t n, float* out) {
    if (!grid || !pix_r || !pix_c || !out || rows <= 0 || cols <= 0 || n < 1 || n > msr::INFILL_MAX_N) return -1;
    static thread_local msr::InfillWork w;
    for (int i = 0; i < n; ++i) {
        const int32_t r = pix_r[i], c = pix_c[i];
        if (r < 1 || r >= rows - 1 || c < 1 || c >= cols - 1) return -1;
        if (i && (r < pix_r[i - 1] || (r == pix_r[i - 1] && c <= pix_c[i - 1]))) return -1;
        if (r - pix_r[0] >= msr::INFILL_MAX_N || c - pix_c[0] >= msr::INFILL_MAX_N || pix_c[0] - c >= msr::INFILL_MAX_N) return -1;
        w.pr[i] = r;
        w.pc[i] = c;
    }
    w.n = n;
    const msr::InfillGrid v{grid, nullptr, rows, cols, (cols + 63) / 64, no_value};
    msr::infill_solve_component(v, &w, 0, 1);
    for (int i = 0; i < n; ++i) out[i] = (float)w.b[i];
    return 0;
}
