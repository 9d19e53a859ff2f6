// infill_solve.h — the in-fill of ONE small no-data component as __host__ __device__ functions, in the manner of
// lzw_unstrip.h: the kernels of infill.hip run them (the flood with one lane, the build and the factorisation with the lanes
// of a one-wave workgroup), a host program runs them with one "lane" (nlanes = 1) under a sanitizer, and
// moonsuperresolution_amd/infill.py::infill_reference is the NumPy twin whose bits they reproduce.
//
// The grid is a row window of float32; a pixel is a HOLE iff !(G[p] > no_value) (NaN is a hole), everything outside the
// window is neither a hole nor valid.  A component K is an 8-connected set of holes of fewer than A <= 32 pixels.
//
// The fill is the least-squares solution of "5-point Laplacian = 0" at the centres K and the 4-neighbours of K:
//   unknowns      x_i = u(p_i), p_0 < p_1 < ... the pixels of K in row-major order;
//   centre q      used iff each of its five stencil pixels (N, W, q, E, S) is inside the window and is in K or valid;
//   equation      -4 u(q) + u(N) + u(W) + u(E) + u(S) = 0, i.e.  sum over stencil pixels in K of w x  =  d_q, with w = -4 for q
//                 itself and 1 for a neighbour, and
//                 d_q = -(s), s = 0.0, then s += w * (double)G[t] for the VALID stencil pixels t in the order N, W, q, E, S;
//   normal eqs    N_ij = sum over used centres of w_i w_j (small integers: exact in any order);
//                 b_i: b = 0.0, then b += w * d_q for the used centres q among the stencil positions N, W, p_i, E, S of p_i,
//                 in that order (the only centres whose equation holds x_i), w = -4 for q = p_i and 1 otherwise;
//   Cholesky      N = L L^T without pivoting, column by column: for j = 0 .. n-1 and every i >= j,
//                 s = N_ij, then s -= L_ik * L_jk for k = 0 .. j-1 in that order; L_jj = sqrt(s_j), L_ij = s_i / L_jj;
//   forward       y_i: s = b_i, then s -= L_ik * y_k for k = 0 .. i-1; y_i = s / L_ii;             i = 0 .. n-1
//   backward      x_i: s = y_i, then s -= L_ki * x_k for k = i+1 .. n-1 (ascending); x_i = s / L_ii;  i = n-1 .. 0
//   result        (float)x_i.
// All of it in float64 with separate multiplies and adds (the units that include this compile with -ffp-contract=off); `/`
// and sqrt are correctly rounded.  Every pixel of a component that the callers hand over is itself a used centre (its
// neighbours are in K or valid and it lies two pixels inside the window), so N is positive definite.  Only positions relative
// to the component enter: the same component in another place of another grid gets the same bits.
//
// Every loop is bounded by an argument or a constant (A <= 32, n <= 31, the 5 stencil pixels, the 8 neighbours), never by the
// grid's data alone, and every read of the grid is behind a bounds test.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define INFILL_HD __host__ __device__
#else
#define INFILL_HD
#endif

namespace msr {

constexpr int INFILL_MAX_AREA = 32;                     // largest max_area: components of up to 31 pixels are filled
constexpr int INFILL_MAX_N = INFILL_MAX_AREA - 1;       // unknowns of one component
constexpr int INFILL_MAP_ROWS = INFILL_MAX_N + 4;       // pixel rows r0 - 2 .. r0 + 32 around the first pixel (r0, c0)
constexpr int INFILL_MAP_COLS = 2 * INFILL_MAX_N + 3;   // pixel columns c0 - 32 .. c0 + 32
constexpr uint8_t INFILL_NONE = 0xFF;

struct InfillGrid {
    const float* g;            // [rows][cols]
    const uint64_t* holes;     // [rows][words] bit c & 63 of word c >> 6: the pixel is a hole; nullptr: test g itself
    int32_t rows, cols, words;
    float no_value;
};

struct InfillWork {                                      // 10.8 KB: LDS on the device
    double L[INFILL_MAX_N][INFILL_MAX_N];                // lower triangle: N, then L below the diagonal
    double diag[INFILL_MAX_N];                           // L_jj
    double b[INFILL_MAX_N];                              // b, then y, then x
    int32_t pr[INFILL_MAX_N], pc[INFILL_MAX_N];          // the pixels of K, row-major
    int32_t n;
    uint8_t idx[INFILL_MAP_ROWS][INFILL_MAP_COLS];       // unknown index of the pixel (r0 - 2 + row, c0 - 32 + col), or NONE
};

INFILL_HD inline void infill_sync() {
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();                                     // the workgroup is one wave
#endif
}

INFILL_HD inline bool infill_inside(const InfillGrid& v, int r, int c) { return r >= 0 && r < v.rows && c >= 0 && c < v.cols; }

// (r, c) must be inside
INFILL_HD inline bool infill_hole(const InfillGrid& v, int r, int c) {
    if (v.holes) return (v.holes[(int64_t)r * v.words + (c >> 6)] >> (c & 63)) & 1;
    return !(v.g[(int64_t)r * v.cols + c] > v.no_value);
}

// The pixel is in the fill set of a window [row0, row0 + n_rows) of a grid of full_rows: margin pixels from every edge of the
// whole grid, and max_area rows from a cut edge of the window (there its component, ring and stencils are all in the window).
INFILL_HD inline bool infill_fillable(int r, int c, int row0, int n_rows, int full_rows, int cols, int max_area, int margin) {
    const int64_t gr = (int64_t)row0 + r;
    return gr >= margin && gr < (int64_t)full_rows - margin && c >= margin && c < cols - margin &&
           (row0 == 0 || r >= max_area) && ((int64_t)row0 + n_rows == full_rows || r < n_rows - max_area);
}

// The component of the hole (r0, c0) if (r0, c0) is its first pixel in row-major order and it has fewer than max_area
// pixels: their number, with pr / pc (room for INFILL_MAX_N) in row-major order.  0 otherwise.
INFILL_HD inline int infill_flood(const InfillGrid& v, int max_area, int r0, int c0, int32_t* pr, int32_t* pc) {
    if (max_area < 2 || max_area > INFILL_MAX_AREA || !infill_inside(v, r0, c0) || !infill_hole(v, r0, c0)) return 0;
    pr[0] = r0;
    pc[0] = c0;
    int n = 1;
    for (int head = 0; head < n; ++head) {               // n < max_area
        for (int k = 0; k < 9; ++k) {
            const int r = pr[head] + k / 3 - 1, c = pc[head] + k % 3 - 1;
            if (k == 4 || !infill_inside(v, r, c) || !infill_hole(v, r, c)) continue;
            if (r < r0 || (r == r0 && c < c0)) return 0;          // an earlier pixel: (r0, c0) is not the first
            bool seen = false;
            for (int s = 0; s < n; ++s) seen |= pr[s] == r && pc[s] == c;
            if (seen) continue;
            if (n == max_area - 1) return 0;                      // max_area pixels or more
            pr[n] = r;
            pc[n] = c;
            ++n;
        }
    }
    for (int i = 1; i < n; ++i) {                        // insertion sort to row-major order
        const int32_t r = pr[i], c = pc[i];
        int j = i;
        for (; j > 0 && (pr[j - 1] > r || (pr[j - 1] == r && pc[j - 1] > c)); --j) {
            pr[j] = pr[j - 1];
            pc[j] = pc[j - 1];
        }
        pr[j] = r;
        pc[j] = c;
    }
    return n;
}

// Unknown index of pixel (r, c), or INFILL_NONE
INFILL_HD inline int infill_index(const InfillWork* w, int r, int c) {
    const int mr = r - w->pr[0] + 2, mc = c - w->pc[0] + INFILL_MAX_N + 1;
    if (mr < 0 || mr >= INFILL_MAP_ROWS || mc < 0 || mc >= INFILL_MAP_COLS) return INFILL_NONE;
    return w->idx[mr][mc];
}

INFILL_HD inline int infill_stencil_dr(int t) { return t == 0 ? -1 : t == 4 ? 1 : 0; }     // N, W, centre, E, S
INFILL_HD inline int infill_stencil_dc(int t) { return t == 1 ? -1 : t == 3 ? 1 : 0; }

// Is (r, c) a used centre, and the right-hand side d of its equation
INFILL_HD inline bool infill_centre(const InfillGrid& v, const InfillWork* w, int r, int c, double* d) {
    double s = 0.0;
    for (int t = 0; t < 5; ++t) {
        const int rr = r + infill_stencil_dr(t), cc = c + infill_stencil_dc(t);
        if (!infill_inside(v, rr, cc)) return false;
        if (infill_hole(v, rr, cc)) {
            if (infill_index(w, rr, cc) == INFILL_NONE) return false;
            continue;
        }
        s += (t == 2 ? -4.0 : 1.0) * (double)v.g[(int64_t)rr * v.cols + cc];
    }
    *d = -s;
    return true;
}

// Builds and solves the system of the component in w->n, w->pr, w->pc (set by one lane and synchronised before the call; the
// pixels row-major, all within INFILL_MAX_N - 1 rows and columns of the first).  Every lane of the wave calls it with the same
// arguments; afterwards w->b[i] is x_i for every lane.
INFILL_HD inline void infill_solve_component(const InfillGrid& v, InfillWork* w, int lane, int nlanes) {
    const int n = w->n < INFILL_MAX_N ? w->n : INFILL_MAX_N;
    uint8_t* map = &w->idx[0][0];
    for (int k = lane; k < INFILL_MAP_ROWS * INFILL_MAP_COLS; k += nlanes) map[k] = INFILL_NONE;
    infill_sync();
    for (int i = lane; i < n; i += nlanes) {
        const int mr = w->pr[i] - w->pr[0] + 2, mc = w->pc[i] - w->pc[0] + INFILL_MAX_N + 1;
        if (mr >= 0 && mr < INFILL_MAP_ROWS && mc >= 0 && mc < INFILL_MAP_COLS) w->idx[mr][mc] = (uint8_t)i;
    }
    infill_sync();
    for (int i = lane; i < n; i += nlanes) {             // row i of the normal matrix and b_i
        for (int j = 0; j <= i; ++j) w->L[i][j] = 0.0;
        double b = 0.0;
        for (int t = 0; t < 5; ++t) {
            const int qr = w->pr[i] + infill_stencil_dr(t), qc = w->pc[i] + infill_stencil_dc(t);
            double d;
            if (!infill_centre(v, w, qr, qc, &d)) continue;
            const double wi = t == 2 ? -4.0 : 1.0;
            b += wi * d;
            for (int u = 0; u < 5; ++u) {
                const int j = infill_index(w, qr + infill_stencil_dr(u), qc + infill_stencil_dc(u));
                if (j != INFILL_NONE && j <= i) w->L[i][j] += wi * (u == 2 ? -4.0 : 1.0);
            }
        }
        w->b[i] = b;
    }
    infill_sync();
    for (int j = 0; j < n; ++j) {                        // column j of L
        for (int i = j + lane; i < n; i += nlanes) {
            double s = w->L[i][j];
            for (int k = 0; k < j; ++k) s -= w->L[i][k] * w->L[j][k];
            if (i == j) w->diag[j] = sqrt(s);
            else w->L[i][j] = s;
        }
        infill_sync();
        const double d = w->diag[j];
        for (int i = j + 1 + lane; i < n; i += nlanes) w->L[i][j] = w->L[i][j] / d;
        infill_sync();
    }
    if (lane == 0) {
        for (int i = 0; i < n; ++i) {
            double s = w->b[i];
            for (int k = 0; k < i; ++k) s -= w->L[i][k] * w->b[k];
            w->b[i] = s / w->diag[i];
        }
        for (int i = n - 1; i >= 0; --i) {
            double s = w->b[i];
            for (int k = i + 1; k < n; ++k) s -= w->L[k][i] * w->b[k];
            w->b[i] = s / w->diag[i];
        }
    }
    infill_sync();
}

}  // namespace msr
