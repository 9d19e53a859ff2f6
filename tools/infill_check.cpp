// CPU only, stand-alone: the per-component flood, build and solve of the device in-filling (csrc/infill_solve.h, run here with
// one lane through msr_infill_component_host and msr::infill_flood) under AddressSanitizer / UBSan, against a straightforward
// dense solve written here: the centres K and N4(K) listed explicitly, the matrix M of their equations, M^T M x = M^T d by
// Gaussian elimination with partial pivoting in long double.  The grid, the hole bitmap, the pixel lists and the output are heap
// blocks of exactly their size, so a read or write outside any of them is an error.
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Imoonsuperresolution_amd/csrc tools/infill_check.cpp moonsuperresolution_amd/csrc/host_infill.cpp \
//       -o /tmp/infill_check && /tmp/infill_check
// Cases: 400 random 8-connected shapes of 1 .. 31 pixels, each in a grid cut as closely as the entry allows (one pixel of
// border) and in a roomy one, next to other holes (a second component one valid pixel away, a large hole); lines and blobs of
// 23 and 31 pixels; the flood from every pixel of every grid, on the float grid and on the bitmap, against a plain flood fill;
// the entry's refusals.  Compared: the pixel lists exactly, the fill values to 1e-9 relative to the grid's range.
#include "infill_solve.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <utility>
#include <vector>
extern "C" int32_t msr_infill_component_host(const float* grid, int32_t rows, int32_t cols, float no_value, const int32_t* pix_r,
                                             const int32_t* pix_c, int32_t n, float* out);
typedef std::pair<int, int> Px;
static const float NV = -32768.f;
static int n_cases = 0;

struct Grid {
    int rows, cols;
    float* g;            // exact-size heap block
    uint64_t* bits;
    int words;
    Grid(int r, int c) : rows(r), cols(c), words((c + 63) / 64) {
        g = (float*)malloc(sizeof(float) * r * c);
        bits = (uint64_t*)malloc(sizeof(uint64_t) * r * words);
        for (int i = 0; i < r; ++i)
            for (int j = 0; j < c; ++j) g[i * c + j] = -2000.f + 300.f * std::sin(j / 7.f) * std::cos(i / 5.f) + 3.f * ((i * 31 + j * 17) % 11);
    }
    ~Grid() { free(g); free(bits); }
    bool inside(int r, int c) const { return r >= 0 && r < rows && c >= 0 && c < cols; }
    bool hole(int r, int c) const { return !(g[r * cols + c] > NV); }
    void finish() {
        memset(bits, 0, sizeof(uint64_t) * rows * words);
        for (int i = 0; i < rows; ++i)
            for (int j = 0; j < cols; ++j)
                if (hole(i, j)) bits[i * words + (j >> 6)] |= 1ull << (j & 63);
    }
};

static std::vector<Px> plain_component(const Grid& G, int r, int c) {
    std::set<Px> seen{{r, c}};
    std::vector<Px> todo{{r, c}};
    while (!todo.empty()) {
        Px p = todo.back();
        todo.pop_back();
        for (int dr = -1; dr <= 1; ++dr)
            for (int dc = -1; dc <= 1; ++dc) {
                Px q{p.first + dr, p.second + dc};
                if (G.inside(q.first, q.second) && G.hole(q.first, q.second) && seen.insert(q).second) todo.push_back(q);
            }
    }
    return std::vector<Px>(seen.begin(), seen.end());           // row-major
}

static std::vector<double> dense_solve(const Grid& G, const std::vector<Px>& K) {
    const int n = (int)K.size();
    std::set<Px> inK(K.begin(), K.end()), centres(K.begin(), K.end());
    const int dr[4] = {-1, 0, 0, 1}, dc[4] = {0, -1, 1, 0};
    for (auto& p : K)
        for (int t = 0; t < 4; ++t) centres.insert({p.first + dr[t], p.second + dc[t]});
    std::vector<std::vector<long double>> A(n, std::vector<long double>(n + 1, 0.0L));
    for (auto& q : centres) {
        std::vector<long double> row(n, 0.0L);
        long double d = 0.0L;
        bool used = true;
        for (int t = -1; t < 4 && used; ++t) {
            Px s = t < 0 ? q : Px{q.first + dr[t], q.second + dc[t]};
            const long double w = t < 0 ? -4.0L : 1.0L;
            if (!G.inside(s.first, s.second)) used = false;
            else if (inK.count(s)) row[std::lower_bound(K.begin(), K.end(), s) - K.begin()] += w;
            else if (G.hole(s.first, s.second)) used = false;
            else d -= w * G.g[s.first * G.cols + s.second];
        }
        if (!used) continue;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) A[i][j] += row[i] * row[j];
        for (int i = 0; i < n; ++i) A[i][n] += row[i] * d;
    }
    for (int k = 0; k < n; ++k) {
        int piv = k;
        for (int i = k + 1; i < n; ++i)
            if (fabsl(A[i][k]) > fabsl(A[piv][k])) piv = i;
        std::swap(A[k], A[piv]);
        for (int i = k + 1; i < n; ++i) {
            const long double f = A[i][k] / A[k][k];
            for (int j = k; j <= n; ++j) A[i][j] -= f * A[k][j];
        }
    }
    std::vector<double> x(n);
    for (int i = n - 1; i >= 0; --i) {
        long double s = A[i][n];
        for (int j = i + 1; j < n; ++j) s -= A[i][j] * x[j];
        x[i] = (double)(s / A[i][i]);
    }
    return x;
}

// the flood from every pixel, float grid and bitmap, against the plain flood fill
static int check_floods(const Grid& G, int max_area) {
    int bad = 0;
    for (int view = 0; view < 2; ++view) {
        const msr::InfillGrid v{G.g, view ? G.bits : nullptr, G.rows, G.cols, G.words, NV};
        for (int r = 0; r < G.rows; ++r)
            for (int c = 0; c < G.cols; ++c) {
                int32_t* pr = (int32_t*)malloc(sizeof(int32_t) * msr::INFILL_MAX_N);
                int32_t* pc = (int32_t*)malloc(sizeof(int32_t) * msr::INFILL_MAX_N);
                const int n = msr::infill_flood(v, max_area, r, c, pr, pc);
                int want = 0;
                std::vector<Px> K;
                if (G.hole(r, c)) {
                    K = plain_component(G, r, c);
                    if (K[0] == Px{r, c} && (int)K.size() < max_area) want = (int)K.size();
                }
                int wrong = n != want;
                for (int i = 0; i < n && !wrong; ++i) wrong |= pr[i] != K[i].first || pc[i] != K[i].second;
                if (wrong) printf("MISMATCH flood view %d at (%d, %d): got %d want %d\n", view, r, c, n, want);
                bad += wrong;
                free(pr);
                free(pc);
                ++n_cases;
            }
    }
    return bad;
}

static int check_solve(const Grid& G, const std::vector<Px>& K, const char* what) {
    ++n_cases;
    const int n = (int)K.size();
    int32_t* pr = (int32_t*)malloc(sizeof(int32_t) * n);
    int32_t* pc = (int32_t*)malloc(sizeof(int32_t) * n);
    float* out = (float*)malloc(sizeof(float) * n);
    for (int i = 0; i < n; ++i) pr[i] = K[i].first, pc[i] = K[i].second;
    const int rc = msr_infill_component_host(G.g, G.rows, G.cols, NV, pr, pc, n, out);
    int bad = rc != 0;
    if (!bad) {
        const std::vector<double> x = dense_solve(G, K);
        for (int i = 0; i < n; ++i) {
            const double tol = 1e-9 * 3000.0 + std::fabs(x[i]) * 6e-8;          // float64 solve, then one float32 rounding
            if (!(std::fabs((double)out[i] - x[i]) <= tol)) {
                printf("MISMATCH %s n=%d pixel %d: got %.9g want %.12g\n", what, n, i, out[i], x[i]);
                bad = 1;
                break;
            }
        }
    } else {
        printf("MISMATCH %s n=%d: the entry returned %d\n", what, n, rc);
    }
    free(pr);
    free(pc);
    free(out);
    return bad;
}

static std::vector<Px> random_shape(std::mt19937& g, int n) {
    std::vector<Px> p{{0, 0}};
    while ((int)p.size() < n) {
        Px b = p[g() % p.size()];
        Px q{b.first + (int)(g() % 3) - 1, b.second + (int)(g() % 3) - 1};
        if (std::find(p.begin(), p.end(), q) == p.end()) p.push_back(q);
    }
    return p;
}

// The shape punched into a grid with `pad` pixels around its bounding box, other holes added where there is room
static int run_shape(const std::vector<Px>& shape, int pad, const char* what) {
    int r0 = 0, r1 = 0, c0 = 0, c1 = 0;
    for (auto& p : shape) {
        r0 = std::min(r0, p.first), r1 = std::max(r1, p.first);
        c0 = std::min(c0, p.second), c1 = std::max(c1, p.second);
    }
    Grid G(r1 - r0 + 1 + 2 * pad, c1 - c0 + 1 + 2 * pad);
    std::vector<Px> K;
    for (auto& p : shape) K.push_back({p.first - r0 + pad, p.second - c0 + pad});
    std::sort(K.begin(), K.end());
    for (auto& p : K) G.g[p.first * G.cols + p.second] = NV;
    if (pad >= 6) {
        // a hole one valid pixel right of the component's last pixel, if that does not join it; a large hole in a corner
        Px q{K.back().first, K.back().second + 2};
        bool joins = false;
        for (auto& p : K) joins |= std::abs(p.first - q.first) <= 1 && std::abs(p.second - q.second) <= 1;
        if (!joins && G.inside(q.first, q.second)) G.g[q.first * G.cols + q.second] = NAN;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) G.g[i * G.cols + j] = NV - 1.f;
    }
    G.finish();
    std::vector<Px> seen = plain_component(G, K[0].first, K[0].second);
    int bad = seen != K;
    if (bad) printf("MISMATCH %s: the case's own component is not the shape\n", what);
    bad += check_solve(G, K, what);
    bad += check_floods(G, 24);
    bad += check_floods(G, 32);
    return bad;
}

int main() {
    std::mt19937 g(4321);
    int bad = 0;
    for (int i = 0; i < 400; ++i) {
        const std::vector<Px> s = random_shape(g, 1 + g() % 31);
        bad += run_shape(s, 1, "random, tight");
        if (i % 4 == 0) bad += run_shape(s, 6, "random, roomy");
    }
    for (int n : {23, 31}) {
        std::vector<Px> h, v, d, b;
        for (int i = 0; i < n; ++i) h.push_back({0, i}), v.push_back({i, 0}), d.push_back({i, i}), b.push_back({i / 6, i % 6});
        bad += run_shape(h, 1, "row") + run_shape(v, 1, "column") + run_shape(d, 2, "diagonal") + run_shape(b, 7, "blob");
    }
    {   // refusals
        Grid G(12, 12);
        float out[2];
        int32_t r[2] = {5, 5}, c[2] = {5, 6};
        G.g[5 * 12 + 5] = G.g[5 * 12 + 6] = NV;
        int ok = msr_infill_component_host(G.g, 12, 12, NV, r, c, 2, out) == 0;
        ok &= msr_infill_component_host(nullptr, 12, 12, NV, r, c, 2, out) == -1;
        ok &= msr_infill_component_host(G.g, 12, 12, NV, r, c, 0, out) == -1;
        ok &= msr_infill_component_host(G.g, 12, 12, NV, r, c, 32, out) == -1;
        int32_t c_rev[2] = {6, 5}, r_edge[2] = {0, 0}, c_far[2] = {5, 11};
        ok &= msr_infill_component_host(G.g, 12, 12, NV, r, c_rev, 2, out) == -1;
        ok &= msr_infill_component_host(G.g, 12, 12, NV, r_edge, c, 2, out) == -1;
        ok &= msr_infill_component_host(G.g, 12, 12, NV, r, c_far, 2, out) == -1;
        if (!ok) printf("MISMATCH refusals\n");
        bad += !ok;
        ++n_cases;
    }
    printf("%s (%d mismatches in %d cases)\n", bad ? "FAIL" : "OK", bad, n_cases);
    return bad != 0;
}
