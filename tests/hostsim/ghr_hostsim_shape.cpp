// ghr_hostsim_shape.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Compiles gaussianhaircut_amd/csrc/ghr_shape.h as plain C++ for the host and walks its four kernels with a 64-lane wave kept in
// arrays: the per-element functions are the header's own, the loops, the neighbouring-lane reads, the butterflies and the fold are
// restated here in the launch's order.  Every index a walk forms is checked (GHR_SHAPE_CHECK aborts with the expression).
// tests/shape_sim.py loads this as a shared library; ghr_shape_selfcheck.cpp includes it and adds a main().
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../gaussianhaircut_amd/csrc/ghr_shape.h"

#define GHR_SHAPE_CHECK(cond) \
    do { if (!(cond)) { std::fprintf(stderr, "ghr_hostsim_shape: %s:%d: %s\n", __FILE__, __LINE__, #cond); std::abort(); } } while (0)

namespace ghrsim_shape {

const int WV = GHR_SHAPE_WAVE;

// a += a[lane ^ m], m = 1 .. 32: every lane ends with the same bits
inline float butterfly(float* a)
{
    for (int m = 1; m < WV; m <<= 1) {
        float t[WV];
        for (int l = 0; l < WV; l++) t[l] = a[l] + a[l ^ m];
        std::memcpy(a, t, sizeof(t));
    }
    for (int l = 1; l < WV; l++) GHR_SHAPE_CHECK(std::memcmp(&a[l], &a[0], 4) == 0);
    return a[0];
}

struct Row {
    const float* dirs;
    long long S, n;
    const float* at(long long s, long long i) const
    {
        GHR_SHAPE_CHECK(s >= 0 && s < S && i >= 0 && i < n);
        return dirs + (s * n + i) * 3;
    }
};

inline void unit_of(const Row& r, const float* rest, long long t, long long i, float* u)
{
    const float* p = r.at(t, i);
    ghr::shape_unit(ghr::shape_seg(p[0], p[1], p[2], rest[t]), u);
}

}  // namespace ghrsim_shape

extern "C" {

float ghrsim_shape_dead(void) { return GHR_SHAPE_DEAD; }

void ghrsim_shape_neighbours(int S, const float* roots, float r2, int32_t* nbr)
{
    using namespace ghrsim_shape;
    for (int s = 0; s < S; s++) {
        ghr::ShapeTop top;
        ghr::shape_top_init(top);
        for (int base = 0; base < S; base += GHR_SHAPE_TILE) {
            const int count = S - base < GHR_SHAPE_TILE ? S - base : GHR_SHAPE_TILE;
            for (int j = 0; j < count; j++) {
                const int cand = base + j;
                GHR_SHAPE_CHECK(cand >= 0 && cand < S);
                const float d = ghr::shape_dist2(roots + 3 * (size_t)s, roots[3 * (size_t)cand], roots[3 * (size_t)cand + 1], roots[3 * (size_t)cand + 2]);
                if (cand != s) ghr::shape_top_insert(top, d, cand);
            }
        }
        for (int k = 0; k < GHR_SHAPE_K; k++) nbr[GHR_SHAPE_K * (size_t)s + k] = ghr::shape_top_entry(top, k, r2);
    }
}

void ghrsim_shape_forward(int S, int n, const float* dirs, const float* rest, const int32_t* nbr, long long M, float* partial, float* E)
{
    using namespace ghrsim_shape;
    const Row row{dirs, S, n};
    float div[3];
    ghr::shape_divisors(S, n, M, div);
    for (int s = 0; s < S; s++) {
        const float r = rest[s], r2 = r * r;
        int t[GHR_SHAPE_K];
        for (int k = 0; k < GHR_SHAPE_K; k++) {
            const int x = nbr[GHR_SHAPE_K * (size_t)s + k];
            t[k] = (unsigned)x < (unsigned)S ? x : -1;
        }
        float acc[3][WV];
        std::memset(acc, 0, sizeof(acc));
        for (int base = 0; base < n; base += WV)
            for (int lane = 0; lane < WV; lane++) {
                const int i = base + lane;
                if (i >= n) continue;
                const float* d = row.at(s, i);
                const ghr::ShapeSeg g = ghr::shape_seg(d[0], d[1], d[2], r);
                float u[3];
                ghr::shape_unit(g, u);
                acc[0][lane] = acc[0][lane] + ghr::shape_stretch(g.len, r);
                if (i + 1 < n) acc[1][lane] = acc[1][lane] + ghr::shape_bend(d, row.at(s, i + 1), r2);
                for (int k = 0; k < GHR_SHAPE_K; k++) {
                    if (t[k] < 0) continue;
                    float ut[3];
                    unit_of(row, rest, t[k], i, ut);
                    acc[2][lane] = acc[2][lane] + ghr::shape_coherence(u, ut);
                }
            }
        for (int c = 0; c < 3; c++) partial[3 * (size_t)s + c] = butterfly(acc[c]);
    }
    // k_shape_fold
    const int NW = GHR_SHAPE_FOLD / WV;
    for (int c = 0; c < 3; c++) {
        float waves[NW];
        for (int w = 0; w < NW; w++) {
            float acc[WV];
            for (int l = 0; l < WV; l++) {
                acc[l] = 0.f;
                for (int s = w * WV + l; s < S; s += GHR_SHAPE_FOLD) acc[l] = acc[l] + partial[3 * (size_t)s + c];
            }
            waves[w] = butterfly(acc);
        }
        float sum = waves[0];
        for (int w = 1; w < NW; w++) sum = sum + waves[w];
        E[c] = div[c] > 0.f ? sum / div[c] : 0.f;
    }
}

void ghrsim_shape_backward(int S, int n, const float* dirs, const float* rest, const int32_t* nbr, const int32_t* start, const int32_t* list,
                           long long list_len, long long M, const float* dE, float* d_dirs)
{
    using namespace ghrsim_shape;
    const Row row{dirs, S, n};
    float div[3], w[3];
    ghr::shape_divisors(S, n, M, div);
    ghr::shape_weights(dE, div, w);
    for (int s = 0; s < S; s++) {
        int t[GHR_SHAPE_K];
        for (int k = 0; k < GHR_SHAPE_K; k++) {
            const int x = nbr[GHR_SHAPE_K * (size_t)s + k];
            t[k] = (unsigned)x < (unsigned)S ? x : -1;
        }
        int beg = start[s], L = start[s + 1] - beg;
        if (beg < 0 || L < 0 || (long long)beg + L > M) { beg = 0; L = 0; }
        GHR_SHAPE_CHECK((long long)beg + L <= list_len);
        for (int i = 0; i < n; i++) {
            const float* d = row.at(s, i);
            const ghr::ShapeSeg g = ghr::shape_seg(d[0], d[1], d[2], rest[s]);
            float sum[3] = {0.f, 0.f, 0.f};
            for (int k = 0; k < GHR_SHAPE_K; k++) {
                if (t[k] < 0) continue;
                float ut[3];
                unit_of(row, rest, t[k], i, ut);
                for (int c = 0; c < 3; c++) sum[c] = sum[c] + ut[c];
            }
            for (int e = 0; e < L; e++) {
                const int x = list[beg + e] >> 2;
                if ((unsigned)x >= (unsigned)S) continue;
                float ut[3];
                unit_of(row, rest, x, i, ut);
                for (int c = 0; c < 3; c++) sum[c] = sum[c] + ut[c];
            }
            float* out = d_dirs + ((size_t)s * n + i) * 3;
            ghr::shape_grad(g, i > 0 ? row.at(s, i - 1) : nullptr, i + 1 < n ? row.at(s, i + 1) : nullptr, sum, w, rest[s], out);
        }
    }
}

}  // extern "C"
