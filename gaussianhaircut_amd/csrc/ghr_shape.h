// ghr_shape.h -- the strand stage's shape term: stretch, bend and neighbour coherence of explicit strands.  The
// reference keeps strands hair-like with a pretrained strand decoder and a diffusion prior; on create_from_polylines the optimised
// parameter is the segment vectors themselves and every one of them is free.  This term needs no network.
//
// The definition (ours, exact).  Everything is float32 without contraction: + - * / and sqrtf.
//   inputs      d[s][i]: the segment vectors, [S][n][3];  rest[s] > 0: a rest length per strand, static;
//               nbr[s][k], k < K = 4: another strand or -1, static;  GHR_SHAPE_DEAD = 1e-4f.
//   per segment len = sqrtf((dx*dx + dy*dy) + dz*dz);  q = d / len componentwise, the zero vector where len == 0;
//               alive(s, i) = len > GHR_SHAPE_DEAD * rest[s];  u = q where alive, else the zero vector AS A CONSTANT (no gradient
//               passes through a dead u).
//   stretch     E0 = sum_{s,i} (len / rest_s - 1)^2 / (S n);  the derivative of len is q.
//   bend        E1 = sum_{s, i < n-1} (((ex*ex + ey*ey) + ez*ez) / (rest_s * rest_s)) / (S (n - 1)),  e = d[s][i+1] - d[s][i];
//               0 when n == 1.
//   coherence   E2 = sum_{s,k: nbr >= 0} sum_i (1 - ((ux*tx + uy*ty) + uz*tz)) / (n M),  t = u[nbr[s][k]][i] (dead by ITS strand's
//               rest), M the number of valid (s, k); 0 when M == 0.  A pair with a dead member contributes exactly 1 and no
//               gradient.  A pair that two strands both chose counts twice.
//   divisors    (float)(S n), (float)(S (n - 1)), (float)(n M), the products formed in 64-bit integers.
// Order of the sums: per lane (segments lane, lane + 64, ...) ascending i, per i the terms in the order stretch | bend | k = 0..3;
// then the butterfly a += a[lane ^ m], m = 1, 2, ... 32, over the wave (every lane ends with the same bits); the three partials
// of strand s go to partial[s][3].  k_shape_fold, one workgroup of GHR_SHAPE_FOLD threads: thread t adds partial[t], partial[t +
// GHR_SHAPE_FOLD], ... ascending, the same butterfly over each wave, then the waves' sums in ascending wave order; E = sum / divisor.
//
// Backward, from a device cotangent dE[3] (no host read):  w0 = dE[0] / (float)(S n),  w1 = dE[1] / (float)(S (n-1)) (0 when n == 1),
// w2 = dE[2] / (float)(n M) (0 when M == 0).  Per segment:
//   gs = (((w0 * 2) * (len / rest - 1)) / rest) * q
//   gb = ((w1 * 2) / (rest * rest)) * (A - B),  A = d[i] - d[i-1] (0 at i == 0),  B = d[i+1] - d[i] (0 at i == n - 1)
//   gc = ((-w2) / len) * (sum - u * ((ux*sx + uy*sy) + uz*sz))  where alive, else 0;  sum = 0 + the u_t[i] first of the strand's own
//        valid choices in k order, then of its inverted list (the entries 4 t + k with nbr[t][k] == s, ascending) in list order
//   d_dirs = (gs + gb) + gc: every element assigned; no floating-point atomics, no zero fill.
// A result's bits depend on the inputs alone, not on the launch.
//
// Neighbours (k_shape_nbr), over the roots [S][3]: strand s gets its 4 nearest OTHER roots by d2 = ((dx*dx) + (dy*dy)) + (dz*dz),
// dx = root[c] - root[s], ascending, equal distances to the lower index, coincident roots being ordinary neighbours: the candidates
// are visited in ascending index and inserted on strict `<` into a sorted top-4 that starts at +inf (a candidate whose d2 is +inf
// or NaN is never taken).  An entry is -1 where d2 > r2 or no candidate was taken.  Brute force, one lane per query root, the
// candidates staged through LDS in tiles; once per model.
//
// Mapping: k_shape_fwd / k_shape_bwd one wave per strand, a lane per segment in chunks of 64; a lane reads its 12 bytes straight
// from the row (a wave's 768 contiguous bytes), d[i+1] / d[i-1] come from the neighbouring lane and from memory at the chunk edge.
// Per-element functions are GHR_HD and the header is plain C++ outside __HIPCC__ (tests/hostsim/ghr_hostsim_shape.cpp walks them).
#pragma once
#if defined(__HIPCC__)
#include "ghr_device.h"
#else
#include <stdint.h>
#define GHR_HD inline
#endif
#include <math.h>
#include <stddef.h>

#define GHR_SHAPE_K 4
#define GHR_SHAPE_DEAD 1e-4f
#define GHR_SHAPE_WAVE 64
#define GHR_SHAPE_BLOCK 256   // four waves: four strands per workgroup of k_shape_fwd / k_shape_bwd
#define GHR_SHAPE_FOLD 1024   // threads of k_shape_fold's one workgroup
#define GHR_SHAPE_TILE 256    // candidate roots per LDS tile of k_shape_nbr

namespace ghr {

// one segment: its vector, length, q = d / len (0 where len == 0) and whether it is alive under its strand's rest length
struct ShapeSeg {
    float d[3], q[3], len;
    bool alive;
};

GHR_HD ShapeSeg shape_seg(float dx, float dy, float dz, float rest)
{
    ShapeSeg g;
    g.d[0] = dx; g.d[1] = dy; g.d[2] = dz;
    g.len = sqrtf((dx * dx + dy * dy) + dz * dz);
    const bool pos = g.len > 0.f;
    const float den = pos ? g.len : 1.f;
    for (int c = 0; c < 3; c++) g.q[c] = pos ? g.d[c] / den : 0.f;
    g.alive = g.len > GHR_SHAPE_DEAD * rest;
    return g;
}

// u: q where alive, else 0
GHR_HD void shape_unit(const ShapeSeg& g, float* u)
{
    for (int c = 0; c < 3; c++) u[c] = g.alive ? g.q[c] : 0.f;
}

GHR_HD float shape_stretch(float len, float rest)
{
    const float t = len / rest - 1.f;
    return t * t;
}

GHR_HD float shape_bend(const float* d, const float* dn, float rest2)
{
    const float ex = dn[0] - d[0], ey = dn[1] - d[1], ez = dn[2] - d[2];
    return ((ex * ex + ey * ey) + ez * ez) / rest2;
}

GHR_HD float shape_coherence(const float* u, const float* t) { return 1.f - ((u[0] * t[0] + u[1] * t[1]) + u[2] * t[2]); }

// the three cotangents over their divisors
GHR_HD void shape_weights(const float* dE, const float* div, float* w)
{
    for (int c = 0; c < 3; c++) w[c] = div[c] > 0.f ? dE[c] / div[c] : 0.f;
}

// the gradient of one segment; prev / next: the neighbouring segment vectors or NULL at the strand's ends; sum: the u_t it met
GHR_HD void shape_grad(const ShapeSeg& g, const float* prev, const float* next, const float* sum, const float* w, float rest, float* out)
{
    const float cs = ((w[0] * 2.f) * (g.len / rest - 1.f)) / rest;
    const float cb = (w[1] * 2.f) / (rest * rest);
    float u[3];
    shape_unit(g, u);
    const float p = (u[0] * sum[0] + u[1] * sum[1]) + u[2] * sum[2];
    const float cc = g.alive ? (-w[2]) / g.len : 0.f;
    for (int c = 0; c < 3; c++) {
        const float A = prev ? g.d[c] - prev[c] : 0.f, B = next ? next[c] - g.d[c] : 0.f;
        const float gs = cs * g.q[c], gb = cb * (A - B);
        const float gc = g.alive ? cc * (sum[c] - u[c] * p) : 0.f;
        out[c] = (gs + gb) + gc;
    }
}

// the sorted four nearest of one query root
struct ShapeTop {
    float d[GHR_SHAPE_K];
    int32_t j[GHR_SHAPE_K];
};

GHR_HD void shape_top_init(ShapeTop& t)
{
    for (int k = 0; k < GHR_SHAPE_K; k++) { t.d[k] = INFINITY; t.j[k] = -1; }
}

GHR_HD float shape_dist2(const float* q, float cx, float cy, float cz)
{
    const float dx = cx - q[0], dy = cy - q[1], dz = cz - q[2];
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// insertion on strict `<`: among equal distances the candidate that came first (the lower index) stays in front
GHR_HD void shape_top_insert(ShapeTop& t, float d, int32_t j)
{
    if (!(d < t.d[3])) return;
    if (d < t.d[0]) {
        t.d[3] = t.d[2]; t.j[3] = t.j[2]; t.d[2] = t.d[1]; t.j[2] = t.j[1]; t.d[1] = t.d[0]; t.j[1] = t.j[0]; t.d[0] = d; t.j[0] = j;
    } else if (d < t.d[1]) {
        t.d[3] = t.d[2]; t.j[3] = t.j[2]; t.d[2] = t.d[1]; t.j[2] = t.j[1]; t.d[1] = d; t.j[1] = j;
    } else if (d < t.d[2]) {
        t.d[3] = t.d[2]; t.j[3] = t.j[2]; t.d[2] = d; t.j[2] = j;
    } else {
        t.d[3] = d; t.j[3] = j;
    }
}

GHR_HD int32_t shape_top_entry(const ShapeTop& t, int k, float r2) { return (t.j[k] >= 0 && !(t.d[k] > r2)) ? t.j[k] : -1; }

// the three divisors (0: the term is 0)
inline void shape_divisors(int64_t S, int64_t n, int64_t M, float* div)
{
    div[0] = (float)(S * n);
    div[1] = n > 1 ? (float)(S * (n - 1)) : 0.f;
    div[2] = M > 0 ? (float)(n * M) : 0.f;
}

struct ShapeArgs {
    int S, n;
    const float* dirs;     // [S][n][3]
    const float* rest;     // [S]
    const int32_t* nbr;    // [S][4]
    const int32_t* start;  // [S + 1]   (backward)
    const int32_t* list;   // [M]       (backward)
    int M;                 // the valid entries of nbr: the length of list
    float div[3];
    float* partial;        // [S][3]   (forward)
    const float* dE;       // [3]      (backward)
    float* d_dirs;         // [S][n][3] (backward)
};

#if defined(__HIPCC__)

__device__ __forceinline__ float shape_wave_sum(float a)
{
    for (int m = 1; m < GHR_SHAPE_WAVE; m <<= 1) a = a + __shfl_xor(a, m, GHR_SHAPE_WAVE);
    return a;
}

// One lane per query root, one wave per workgroup; the candidates go through LDS in tiles of GHR_SHAPE_TILE, in ascending index.
__global__ void __launch_bounds__(GHR_SHAPE_WAVE) k_shape_nbr(int S, const float* __restrict__ roots, float r2, int32_t* __restrict__ nbr)
{
    __shared__ float tile[3][GHR_SHAPE_TILE];
    const int lane = threadIdx.x;
    const int s = blockIdx.x * GHR_SHAPE_WAVE + lane;
    const bool has = s < S;
    const int sq = has ? s : S - 1;
    const float q[3] = {roots[3 * (size_t)sq], roots[3 * (size_t)sq + 1], roots[3 * (size_t)sq + 2]};
    ShapeTop top;
    shape_top_init(top);
    for (int base = 0; base < S; base += GHR_SHAPE_TILE) {
        const int count = min(GHR_SHAPE_TILE, S - base);
        __syncthreads();  // every lane is done with the previous tile
        for (int j = lane; j < count; j += GHR_SHAPE_WAVE)
            for (int c = 0; c < 3; c++) tile[c][j] = roots[3 * (size_t)(base + j) + c];
        __syncthreads();
        for (int j = 0; j < count; j++) {
            const int cand = base + j;
            const float d = shape_dist2(q, tile[0][j], tile[1][j], tile[2][j]);  // every lane reads the same address
            if (cand != s) shape_top_insert(top, d, cand);
        }
    }
    if (has)
        for (int k = 0; k < GHR_SHAPE_K; k++) nbr[GHR_SHAPE_K * (size_t)s + k] = shape_top_entry(top, k, r2);
}

// One wave per strand: the three partial sums of strand s.
__global__ void __launch_bounds__(GHR_SHAPE_BLOCK) k_shape_fwd(ShapeArgs a)
{
    const int lane = threadIdx.x & (GHR_SHAPE_WAVE - 1);
    const int s = __builtin_amdgcn_readfirstlane(blockIdx.x * (GHR_SHAPE_BLOCK / GHR_SHAPE_WAVE) + (threadIdx.x >> 6));
    if (s >= a.S) return;
    const int n = a.n;
    const float rest = a.rest[s], rest2 = rest * rest;
    int t[GHR_SHAPE_K];
    float rest_t[GHR_SHAPE_K];
    for (int k = 0; k < GHR_SHAPE_K; k++) {
        const int x = a.nbr[GHR_SHAPE_K * (size_t)s + k];
        t[k] = (unsigned)x < (unsigned)a.S ? x : -1;  // (an entry outside [0, S) is no neighbour: no access leaves the buffers)
        rest_t[k] = t[k] >= 0 ? a.rest[t[k]] : 1.f;
    }
    const float* row = a.dirs + (size_t)s * n * 3;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int base = 0; base < n; base += GHR_SHAPE_WAVE) {
        const int i = base + lane;
        const bool has = i < n;
        float d[3] = {0.f, 0.f, 0.f};
        if (has) { d[0] = row[3 * i]; d[1] = row[3 * i + 1]; d[2] = row[3 * i + 2]; }
        float dn[3];
        for (int c = 0; c < 3; c++) dn[c] = __shfl_down(d[c], 1, GHR_SHAPE_WAVE);
        const bool has_next = i + 1 < n;
        if (lane == GHR_SHAPE_WAVE - 1 && has_next) { dn[0] = row[3 * i + 3]; dn[1] = row[3 * i + 4]; dn[2] = row[3 * i + 5]; }  // the chunk's edge
        if (!has) continue;
        const ShapeSeg g = shape_seg(d[0], d[1], d[2], rest);
        float u[3];
        shape_unit(g, u);
        acc[0] = acc[0] + shape_stretch(g.len, rest);
        if (has_next) acc[1] = acc[1] + shape_bend(d, dn, rest2);
        for (int k = 0; k < GHR_SHAPE_K; k++) {
            if (t[k] < 0) continue;
            const float* p = a.dirs + ((size_t)t[k] * n + i) * 3;
            float ut[3];
            shape_unit(shape_seg(p[0], p[1], p[2], rest_t[k]), ut);
            acc[2] = acc[2] + shape_coherence(u, ut);
        }
    }
    for (int c = 0; c < 3; c++) acc[c] = shape_wave_sum(acc[c]);
    if (lane == 0)
        for (int c = 0; c < 3; c++) a.partial[3 * (size_t)s + c] = acc[c];
}

// One workgroup in all: the partials in ascending s per thread, a butterfly per wave, the waves in ascending order.
__global__ void __launch_bounds__(GHR_SHAPE_FOLD) k_shape_fold(int S, const float* __restrict__ partial, float div0, float div1, float div2,
                                                               float* __restrict__ E)
{
    __shared__ float waves[GHR_SHAPE_FOLD / GHR_SHAPE_WAVE][3];
    const int lane = threadIdx.x & (GHR_SHAPE_WAVE - 1), wave = threadIdx.x >> 6;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int s = threadIdx.x; s < S; s += GHR_SHAPE_FOLD)
        for (int c = 0; c < 3; c++) acc[c] = acc[c] + partial[3 * (size_t)s + c];
    for (int c = 0; c < 3; c++) acc[c] = shape_wave_sum(acc[c]);
    if (lane == 0)
        for (int c = 0; c < 3; c++) waves[wave][c] = acc[c];
    __syncthreads();
    if (threadIdx.x < 3) {
        const int c = threadIdx.x;
        float sum = waves[0][c];
        for (int w = 1; w < GHR_SHAPE_FOLD / GHR_SHAPE_WAVE; w++) sum = sum + waves[w][c];
        const float div = c == 0 ? div0 : c == 1 ? div1 : div2;
        E[c] = div > 0.f ? sum / div : 0.f;
    }
}

// One wave per strand, a lane per segment: gather form, every element of d_dirs assigned.
__global__ void __launch_bounds__(GHR_SHAPE_BLOCK) k_shape_bwd(ShapeArgs a)
{
    const int lane = threadIdx.x & (GHR_SHAPE_WAVE - 1);
    const int s = __builtin_amdgcn_readfirstlane(blockIdx.x * (GHR_SHAPE_BLOCK / GHR_SHAPE_WAVE) + (threadIdx.x >> 6));
    if (s >= a.S) return;
    const int n = a.n;
    const float rest = a.rest[s];
    const float dE[3] = {a.dE[0], a.dE[1], a.dE[2]};
    float w[3];
    shape_weights(dE, a.div, w);
    int t[GHR_SHAPE_K];
    float rest_t[GHR_SHAPE_K];
    for (int k = 0; k < GHR_SHAPE_K; k++) {
        const int x = a.nbr[GHR_SHAPE_K * (size_t)s + k];
        t[k] = (unsigned)x < (unsigned)a.S ? x : -1;
        rest_t[k] = t[k] >= 0 ? a.rest[t[k]] : 1.f;
    }
    // the strand's inverted list; a range that does not lie inside the list (only a caller's bad table can hold one) is empty
    int beg = a.start[s], L = a.start[s + 1] - beg;
    if (beg < 0 || L < 0 || (long long)beg + L > a.M) { beg = 0; L = 0; }
    const float* row = a.dirs + (size_t)s * n * 3;
    float* out = a.d_dirs + (size_t)s * n * 3;
    for (int base = 0; base < n; base += GHR_SHAPE_WAVE) {
        const int i = base + lane;
        const bool has = i < n;
        float d[3] = {0.f, 0.f, 0.f};
        if (has) { d[0] = row[3 * i]; d[1] = row[3 * i + 1]; d[2] = row[3 * i + 2]; }
        float dn[3], dp[3];
        for (int c = 0; c < 3; c++) { dn[c] = __shfl_down(d[c], 1, GHR_SHAPE_WAVE); dp[c] = __shfl_up(d[c], 1, GHR_SHAPE_WAVE); }
        const bool has_next = i + 1 < n, has_prev = has && i > 0;
        if (lane == GHR_SHAPE_WAVE - 1 && has_next) { dn[0] = row[3 * i + 3]; dn[1] = row[3 * i + 4]; dn[2] = row[3 * i + 5]; }
        if (lane == 0 && has_prev) { dp[0] = row[3 * i - 3]; dp[1] = row[3 * i - 2]; dp[2] = row[3 * i - 1]; }
        if (!has) continue;
        const ShapeSeg g = shape_seg(d[0], d[1], d[2], rest);
        float sum[3] = {0.f, 0.f, 0.f};
        for (int k = 0; k < GHR_SHAPE_K; k++) {
            if (t[k] < 0) continue;
            const float* p = a.dirs + ((size_t)t[k] * n + i) * 3;
            float ut[3];
            shape_unit(shape_seg(p[0], p[1], p[2], rest_t[k]), ut);
            for (int c = 0; c < 3; c++) sum[c] = sum[c] + ut[c];
        }
        for (int e = 0; e < L; e++) {
            const int x = a.list[beg + e] >> 2;  // the entry 4 t + k
            if ((unsigned)x >= (unsigned)a.S) continue;
            const float* p = a.dirs + ((size_t)x * n + i) * 3;
            float ut[3];
            shape_unit(shape_seg(p[0], p[1], p[2], a.rest[x]), ut);
            for (int c = 0; c < 3; c++) sum[c] = sum[c] + ut[c];
        }
        float grad[3];
        shape_grad(g, has_prev ? dp : nullptr, has_next ? dn : nullptr, sum, w, rest, grad);
        out[3 * i] = grad[0]; out[3 * i + 1] = grad[1]; out[3 * i + 2] = grad[2];
    }
}

#endif  // __HIPCC__

}  // namespace ghr
