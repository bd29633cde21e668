// ghr_sds.h -- the strand stage's prior term between its two networks (src/scene/gaussian_model_strands.py:456-503
// restated): guiding strands into their scalp-local frames, and the G x G latent texture blended from each texel's four nearest
// guiding strands in UV space by HAAR's cosine-similarity rule.  The strand encoder and the prior's loss are the caller's.
//
//   local frame   P[g, j] = sum_{i < j} dirs[idx[g], i],  e[g, j] = (M P[g, j]) scale,  v[g, j] = (M dirs[idx[g], j]) scale,
//                 M = local2world[idx[g]]^-1 (given, or the adjugate form sds_inv3 of the given frame)
//   neighbours    d2(q, g) = (cx - u_g)^2 + (cy - v_g)^2; the four smallest under (d2 ascending, then g ascending): a total
//                 order when no distance is NaN, so the answer then does not depend on how the candidates are split or merged
//   similarity    cos(a, b) = (a / max(|a|, 1e-8)) . (b / max(|b|, 1e-8)); csim_full[j][k] = mean over segments;
//                 csim[q] = mean of the ten pairs j <= k, for texel q < N -- and alpha[g] reads csim[q = g] (the reference's
//                 indexing: strand g's coefficient comes from the neighbourhood of TEXEL number g)
//   blend         alpha_q = sum_k w_k alpha[nbr_k],  z_q = z[nbr_0] alpha_q + (sum_k w_k z[nbr_k]) (1 - alpha_q)
//
// Mapping: one wave per guiding strand (local frame, lists, the gathers of the backward), one wave per texel (neighbours +
// similarity, blend).  The backward is gather-form: k_sds_lists leaves, per guiding strand, the (q, k) that chose it in
// ascending q (integer counting only), and every gradient is a sum in that order -- no floating-point atomics, two passes give
// the same bits.  Per-element arithmetic is GHR_HD: tests/hostsim/ghr_hostsim_sds.cpp runs it on the CPU.
#pragma once
#if defined(__HIPCC__)
#include "ghr_device.h"
#else
#include <stdint.h>
#define GHR_HD inline
#endif
#include <math.h>
#include <stddef.h>

#define GHR_SDS_K 4
#define GHR_SDS_PAIRS 10
#define GHR_SDS_WAVE 64
#define GHR_SDS_BLOCK 256  // four waves: four strands or four texels per workgroup
#define GHR_SDS_DIST_EPS 1e-7f
#define GHR_SDS_COS_EPS 1e-8f
#define GHR_SDS_CSIM_KNEE 0.9f

namespace ghr {

// row-major 3 x 3 inverse: adjugate over determinant
GHR_HD void sds_inv3(const float* m, float* o)
{
    const float c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
    const float r = 1.f / ((m[0] * c00 + m[1] * c01) + m[2] * c02);
    o[0] = c00 * r; o[1] = (m[2] * m[7] - m[1] * m[8]) * r; o[2] = (m[1] * m[5] - m[2] * m[4]) * r;
    o[3] = c01 * r; o[4] = (m[0] * m[8] - m[2] * m[6]) * r; o[5] = (m[2] * m[3] - m[0] * m[5]) * r;
    o[6] = c02 * r; o[7] = (m[1] * m[6] - m[0] * m[7]) * r; o[8] = (m[0] * m[4] - m[1] * m[3]) * r;
}

// o = (M x) scale
GHR_HD void sds_mv(const float* M, const float* x, float scale, float* o)
{
    for (int r = 0; r < 3; r++) o[r] = ((M[3 * r] * x[0] + M[3 * r + 1] * x[1]) + M[3 * r + 2] * x[2]) * scale;
}

// o = (M^T d) scale: the VJP of sds_mv
GHR_HD void sds_mtv(const float* M, const float* d, float scale, float* o)
{
    for (int c = 0; c < 3; c++) o[c] = ((M[c] * d[0] + M[3 + c] * d[1]) + M[6 + c] * d[2]) * scale;
}

// ---- the four nearest, ties to the lower guiding index ----------------------------------------------------------------------
struct SdsTop {
    float d[GHR_SDS_K];
    int32_t g[GHR_SDS_K];
};

// (d, g) sorts before (e, h): a strict total order on finite and infinite distances (the indices differ).  With a NaN distance
// neither `<` holds and the index decides; the relation is then no longer transitive, so WHICH four are kept can depend on how
// the candidates were split and merged.  What holds whatever the UVs are: any real candidate displaces a sentinel, so after four
// candidates every stored index is a guiding strand.
GHR_HD bool sds_before(float d, int32_t g, float e, int32_t h) { return d < e || (!(e < d) && g < h); }

GHR_HD void sds_top_init(SdsTop& t)
{
    for (int k = 0; k < GHR_SDS_K; k++) { t.d[k] = INFINITY; t.g[k] = 0x7fffffff; }
}

GHR_HD void sds_top_insert(SdsTop& t, float d, int32_t g)
{
    if (!sds_before(d, g, t.d[3], t.g[3])) return;
    t.d[3] = d; t.g[3] = g;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 3; k > 0; k--) {
        if (sds_before(t.d[k], t.g[k], t.d[k - 1], t.g[k - 1])) {
            const float fd = t.d[k]; t.d[k] = t.d[k - 1]; t.d[k - 1] = fd;
            const int32_t fg = t.g[k]; t.g[k] = t.g[k - 1]; t.g[k - 1] = fg;
        }
    }
}

GHR_HD float sds_dist2(float cx, float cy, float u, float v)
{
    const float dx = cx - u, dy = cy - v;
    return dx * dx + dy * dy;
}

// w_k = 1 / (d_k + 1e-7), normalised
GHR_HD void sds_weights(const float* d, float* w)
{
    float r[GHR_SDS_K];
    for (int k = 0; k < GHR_SDS_K; k++) r[k] = 1.f / (d[k] + GHR_SDS_DIST_EPS);
    const float s = ((r[0] + r[1]) + r[2]) + r[3];
    for (int k = 0; k < GHR_SDS_K; k++) w[k] = r[k] / s;
}

// ---- cosine similarity of the four neighbours' segment vectors ---------------------------------------------------------------
// u = a / max(|a|, eps); returns the clamped norm, *len the unclamped one
GHR_HD float sds_unit(const float* a, float* u, float* len)
{
    const float l = sqrtf((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    const float m = l > GHR_SDS_COS_EPS ? l : GHR_SDS_COS_EPS;
    u[0] = a[0] / m; u[1] = a[1] / m; u[2] = a[2] / m;
    *len = l;
    return m;
}

GHR_HD float sds_dot(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// the ten pair cosines of one segment, in the order (0,0) (0,1) (0,2) (0,3) (1,1) (1,2) (1,3) (2,2) (2,3) (3,3), added to acc
GHR_HD void sds_pair_cos(const float a[GHR_SDS_K][3], float* acc)
{
    float u[GHR_SDS_K][3], len;
    for (int m = 0; m < GHR_SDS_K; m++) (void)sds_unit(a[m], u[m], &len);
    int p = 0;
    for (int j = 0; j < GHR_SDS_K; j++)
        for (int k = j; k < GHR_SDS_K; k++) acc[p++] += sds_dot(u[j], u[k]);
}

// csim from the ten sums over n segments
GHR_HD float sds_csim(const float* acc, int n)
{
    float s = 0.f;
    for (int p = 0; p < GHR_SDS_PAIRS; p++) s += acc[p] / (float)n;
    return s / (float)GHR_SDS_PAIRS;
}

GHR_HD float sds_alpha(float c)
{
    const float c2 = c * c;
    return c <= GHR_SDS_CSIM_KNEE ? 1.f - 1.63f * ((c2 * c2) * c) : 0.4f - 0.4f * c;
}

GHR_HD float sds_alpha_dc(float c)
{
    const float c2 = c * c;
    return c <= GHR_SDS_CSIM_KNEE ? -(1.63f * 5.f) * (c2 * c2) : -0.4f;
}

// d of neighbour k's segment vector when every pair cosine of the segment receives dc: with u_m the clamped unit vectors and
// U their sum, d u_k = dc (U + u_k) (the pair (k, k) counts u_k twice), and through u = a / m, m = max(|a|, eps) with the
// clamp passing the norm's derivative (as F.cosine_similarity's autograd has it):  d a = d u / m - a (a . d u) / (|a| m^2).
GHR_HD void sds_pair_cos_vjp(const float a[GHR_SDS_K][3], int k, float dc, float* da)
{
    float u[GHR_SDS_K][3], len = 0.f, lk = 0.f, mk = 1.f;
    for (int m = 0; m < GHR_SDS_K; m++) {
        const float mm = sds_unit(a[m], u[m], &len);
        if (m == k) { lk = len; mk = mm; }
    }
    float du[3];
    for (int c = 0; c < 3; c++) du[c] = dc * ((((u[0][c] + u[1][c]) + u[2][c]) + u[3][c]) + u[k][c]);
    const float t = lk > 0.f ? sds_dot(a[k], du) / (lk * (mk * mk)) : 0.f;
    for (int c = 0; c < 3; c++) da[c] = du[c] / mk - a[k][c] * t;
}

// ---- the blend ------------------------------------------------------------------------------------------------------------------
GHR_HD float sds_mix4(const float* w, const float* x) { return ((w[0] * x[0] + w[1] * x[1]) + w[2] * x[2]) + w[3] * x[3]; }

GHR_HD float sds_blend(float z0, float bil, float alpha_q) { return z0 * alpha_q + bil * (1.f - alpha_q); }

// d z_q / d z[nbr_k]
GHR_HD float sds_blend_dz(int k, float w_k, float alpha_q) { return (k == 0 ? alpha_q : 0.f) + w_k * (1.f - alpha_q); }

// d z_q / d alpha_q, per channel
GHR_HD float sds_blend_dalpha(float z0, float bil) { return z0 - bil; }

// the chunk of segments a lane owns in the local-frame scans
GHR_HD void sds_chunk(int n, int lane, int* lo, int* hi)
{
    const int per = (n + GHR_SDS_WAVE - 1) / GHR_SDS_WAVE;
    const int a = lane * per, b = a + per;
    *lo = a < n ? a : n;
    *hi = b < n ? b : n;
}

#if defined(__HIPCC__)

__device__ __forceinline__ float sds_wave_sum(float x)
{
    for (int m = 1; m < GHR_SDS_WAVE; m <<= 1) x += __shfl_xor(x, m, GHR_SDS_WAVE);
    return x;
}

// exclusive sum over the lanes below (dir > 0) or above (dir < 0) this one, in Hillis-Steele order
__device__ __forceinline__ float sds_wave_excl(float x, int lane, int dir)
{
    for (int d = 1; d < GHR_SDS_WAVE; d <<= 1) {
        const float t = dir > 0 ? __shfl_up(x, d, GHR_SDS_WAVE) : __shfl_down(x, d, GHR_SDS_WAVE);
        if (dir > 0 ? lane >= d : lane + d < GHR_SDS_WAVE) x += t;
    }
    const float t = dir > 0 ? __shfl_up(x, 1, GHR_SDS_WAVE) : __shfl_down(x, 1, GHR_SDS_WAVE);
    return (dir > 0 ? lane == 0 : lane == GHR_SDS_WAVE - 1) ? 0.f : t;
}

struct SdsLocalArgs {
    int32_t S, N, n, frames_are_inverse;
    float scale;
    const float* dirs;       // [S][n][3]
    const float* frames;     // [S][3][3]: local2world, or its inverse
    const int64_t* idx;      // [N]; in the backward: the stably sorted values
    const int64_t* order;    // backward: the guiding strand of each sorted place
    float* e;                // [N][n + 1][3]
    float* v;                // [N][n][3]
    const float* d_e;        // may be NULL
    const float* d_v;        // may be NULL
    float* d_dirs;           // [S][n][3], zero-filled by the caller; rows of drawn strands are added to
};

__device__ __forceinline__ void sds_frame(const SdsLocalArgs& a, int64_t s, float* M)
{
    float f[9];
    for (int i = 0; i < 9; i++) f[i] = a.frames[(size_t)s * 9 + i];
    if (a.frames_are_inverse) { for (int i = 0; i < 9; i++) M[i] = f[i]; }
    else sds_inv3(f, M);
}

// one wave per guiding strand: lane totals of its chunk of segments, a scan over the lanes, a second walk that writes
__global__ void __launch_bounds__(GHR_SDS_BLOCK) k_sds_local(SdsLocalArgs a)
{
    const int lane = threadIdx.x & (GHR_SDS_WAVE - 1);
    const int g = blockIdx.x * (GHR_SDS_BLOCK / GHR_SDS_WAVE) + (threadIdx.x >> 6);
    if (g >= a.N) return;
    const int64_t s = a.idx[g];
    const int n = a.n;
    float* e = a.e + (size_t)g * (n + 1) * 3;
    float* v = a.v + (size_t)g * n * 3;
    int lo, hi;
    sds_chunk(n, lane, &lo, &hi);
    if (s < 0 || s >= a.S) {  // an index outside the model names no strand: the row says so, nothing is read
        for (int i = lo; i < hi; i++)
            for (int c = 0; c < 3; c++) { v[i * 3 + c] = NAN; e[(i + 1) * 3 + c] = NAN; }
        if (lane == 0) e[0] = e[1] = e[2] = NAN;
        return;
    }
    float M[9];
    sds_frame(a, s, M);
    const float* d = a.dirs + (size_t)s * n * 3;
    float run[3] = {0.f, 0.f, 0.f};
    for (int i = lo; i < hi; i++)
        for (int c = 0; c < 3; c++) run[c] += d[i * 3 + c];
    for (int c = 0; c < 3; c++) run[c] = sds_wave_excl(run[c], lane, +1);
    if (lane == 0) e[0] = e[1] = e[2] = 0.f;
    for (int i = lo; i < hi; i++) {
        const float x[3] = {d[i * 3], d[i * 3 + 1], d[i * 3 + 2]};
        float o[3];
        sds_mv(M, x, a.scale, o);
        for (int c = 0; c < 3; c++) { v[i * 3 + c] = o[c]; run[c] += x[c]; }
        sds_mv(M, run, a.scale, o);
        for (int c = 0; c < 3; c++) e[(i + 1) * 3 + c] = o[c];
    }
}

// one wave per place of the sorted draw; the first place of a run of equal strands adds the run's guiding strands in ascending
// g (the sort is stable) into the strand's row: t[i] = d_v[g, i] + sum_{j > i} d_e[g, j], d dirs[s, i] += (M^T t[i]) scale
__global__ void __launch_bounds__(GHR_SDS_BLOCK) k_sds_local_bwd(SdsLocalArgs a)
{
    const int lane = threadIdx.x & (GHR_SDS_WAVE - 1);
    const int p = blockIdx.x * (GHR_SDS_BLOCK / GHR_SDS_WAVE) + (threadIdx.x >> 6);
    if (p >= a.N) return;
    const int64_t s = a.idx[p];
    if (s < 0 || s >= a.S) return;
    if (p > 0 && a.idx[p - 1] == s) return;
    const int n = a.n;
    float M[9];
    sds_frame(a, s, M);
    float* out = a.d_dirs + (size_t)s * n * 3;
    int lo, hi;
    sds_chunk(n, lane, &lo, &hi);
    for (int r = p; r < a.N && a.idx[r] == s; r++) {
        const int64_t g = a.order[r];
        if (g < 0 || g >= a.N) continue;
        const float* de = a.d_e ? a.d_e + (size_t)g * (n + 1) * 3 : nullptr;
        const float* dv = a.d_v ? a.d_v + (size_t)g * n * 3 : nullptr;
        float run[3] = {0.f, 0.f, 0.f};
        if (de) {
            for (int i = hi - 1; i >= lo; i--)
                for (int c = 0; c < 3; c++) run[c] += de[(i + 1) * 3 + c];
            for (int c = 0; c < 3; c++) run[c] = sds_wave_excl(run[c], lane, -1);
        }
        for (int i = hi - 1; i >= lo; i--) {
            float t[3], o[3];
            for (int c = 0; c < 3; c++) {
                if (de) run[c] += de[(i + 1) * 3 + c];
                t[c] = (dv ? dv[i * 3 + c] : 0.f) + run[c];
            }
            sds_mtv(M, t, a.scale, o);
            for (int c = 0; c < 3; c++) out[i * 3 + c] += o[c];
        }
    }
}

struct SdsTexArgs {
    int32_t N, n, C, G;
    const float* uvg;      // [N][2]: the guiding strands' UVs
    const float* centres;  // [G]: the texel centres along one axis
    const float* z;        // [N][C]
    const float* v;        // [N][n][3]
    int32_t* nbr;          // [G G][4]
    float* w;              // [G G][4]
    float* csim;           // [N]: of TEXEL q < N
    float* alpha;          // [N]
    float* alpha_q;        // [G G]
    int32_t* count;        // [N]: zero on entry; how many (q, k) chose each guiding strand
    int32_t* start;        // [N + 1]
    int32_t* list;         // [4 G G]: 4 q + k, ascending within a guiding strand
    float* texture;        // [C][G][G]
    // backward
    const float* d_texture;
    float* dalpha_q;       // [G G]
    float* d_csim;         // [N]
    float* d_z;            // [N][C]
    float* d_v;            // [N][n][3], may be NULL
};

__device__ __forceinline__ void sds_load4(const SdsTexArgs& a, const int32_t* g, int i, float x[GHR_SDS_K][3])
{
    for (int m = 0; m < GHR_SDS_K; m++) {
        const float* p = a.v + ((size_t)g[m] * a.n + i) * 3;
        x[m][0] = p[0]; x[m][1] = p[1]; x[m][2] = p[2];
    }
}

// one wave per texel: lanes split the candidates, a butterfly merges their four; texels q < N go on to the ten pair cosines
__global__ void __launch_bounds__(GHR_SDS_BLOCK) k_sds_knn(SdsTexArgs a)
{
    const int lane = threadIdx.x & (GHR_SDS_WAVE - 1);
    const int q = blockIdx.x * (GHR_SDS_BLOCK / GHR_SDS_WAVE) + (threadIdx.x >> 6);
    if (q >= a.G * a.G) return;
    const float cx = a.centres[q % a.G], cy = a.centres[q / a.G];
    SdsTop t;
    sds_top_init(t);
    for (int g = lane; g < a.N; g += GHR_SDS_WAVE) sds_top_insert(t, sds_dist2(cx, cy, a.uvg[2 * g], a.uvg[2 * g + 1]), g);
    for (int m = 1; m < GHR_SDS_WAVE; m <<= 1) {
        float od[GHR_SDS_K];
        int32_t og[GHR_SDS_K];
#pragma unroll
        for (int k = 0; k < GHR_SDS_K; k++) { od[k] = __shfl_xor(t.d[k], m, GHR_SDS_WAVE); og[k] = __shfl_xor(t.g[k], m, GHR_SDS_WAVE); }
#pragma unroll
        for (int k = 0; k < GHR_SDS_K; k++) sds_top_insert(t, od[k], og[k]);
    }
    // N >= 4: every slot holds a guiding strand (sds_before); the clamp keeps a reader in bounds whatever happens
    for (int k = 0; k < GHR_SDS_K; k++) t.g[k] = t.g[k] < 0 ? 0 : (t.g[k] >= a.N ? a.N - 1 : t.g[k]);
    float w[GHR_SDS_K];
    sds_weights(t.d, w);
    if (lane < GHR_SDS_K) {
        const int32_t g = lane == 0 ? t.g[0] : lane == 1 ? t.g[1] : lane == 2 ? t.g[2] : t.g[3];
        a.nbr[q * GHR_SDS_K + lane] = g;
        a.w[q * GHR_SDS_K + lane] = lane == 0 ? w[0] : lane == 1 ? w[1] : lane == 2 ? w[2] : w[3];
        atomicAdd(&a.count[g], 1);
    }
    if (q >= a.N) return;
    float acc[GHR_SDS_PAIRS];
    for (int p = 0; p < GHR_SDS_PAIRS; p++) acc[p] = 0.f;
    for (int i = lane; i < a.n; i += GHR_SDS_WAVE) {
        float x[GHR_SDS_K][3];
        sds_load4(a, t.g, i, x);
        sds_pair_cos(x, acc);
    }
    for (int p = 0; p < GHR_SDS_PAIRS; p++) acc[p] = sds_wave_sum(acc[p]);
    if (lane == 0) {
        const float c = sds_csim(acc, a.n);
        a.csim[q] = c;
        a.alpha[q] = sds_alpha(c);
    }
}

// one wave per guiding strand: its place in the lists is the sum of the counts below it; then a walk over all 4 G G choices
// in order, each lane's match placed by the ballot's prefix -- ascending (q, k), integers only
__global__ void __launch_bounds__(GHR_SDS_BLOCK) k_sds_lists(SdsTexArgs a)
{
    const int lane = threadIdx.x & (GHR_SDS_WAVE - 1);
    const int g = blockIdx.x * (GHR_SDS_BLOCK / GHR_SDS_WAVE) + (threadIdx.x >> 6);
    if (g >= a.N) return;
    int base = 0;
    for (int h = lane; h < g; h += GHR_SDS_WAVE) base += a.count[h];
    for (int m = 1; m < GHR_SDS_WAVE; m <<= 1) base += __shfl_xor(base, m, GHR_SDS_WAVE);
    const int total = GHR_SDS_K * a.G * a.G;
    if (lane == 0) {
        a.start[g] = base;
        if (g == a.N - 1) a.start[a.N] = base + a.count[g];
    }
    int pos = base;
    for (int e0 = 0; e0 < total; e0 += GHR_SDS_WAVE) {
        const int e = e0 + lane;
        const bool hit = e < total && a.nbr[e] == g;
        const unsigned long long mask = __ballot(hit);
        const int at = pos + __popcll(mask & ((1ull << lane) - 1ull));
        if (hit && at < total) a.list[at] = e;
        pos += __popcll(mask);
    }
}

// one wave per texel, lane = channel
__global__ void __launch_bounds__(GHR_SDS_BLOCK) k_sds_blend(SdsTexArgs a)
{
    const int lane = threadIdx.x & (GHR_SDS_WAVE - 1);
    const int q = blockIdx.x * (GHR_SDS_BLOCK / GHR_SDS_WAVE) + (threadIdx.x >> 6);
    const int GG = a.G * a.G;
    if (q >= GG) return;
    int32_t g[GHR_SDS_K];
    float w[GHR_SDS_K], al[GHR_SDS_K];
    for (int k = 0; k < GHR_SDS_K; k++) { g[k] = a.nbr[q * GHR_SDS_K + k]; w[k] = a.w[q * GHR_SDS_K + k]; al[k] = a.alpha[g[k]]; }
    const float aq = sds_mix4(w, al);
    if (lane == 0) a.alpha_q[q] = aq;
    for (int c = lane; c < a.C; c += GHR_SDS_WAVE) {
        float zk[GHR_SDS_K];
        for (int k = 0; k < GHR_SDS_K; k++) zk[k] = a.z[(size_t)g[k] * a.C + c];
        a.texture[(size_t)c * GG + q] = sds_blend(zk[0], sds_mix4(w, zk), aq);
    }
}

// backward 1, one wave per texel: d alpha_q = sum_c d z_q[c] (z[nbr_0][c] - bilinear[c])
__global__ void __launch_bounds__(GHR_SDS_BLOCK) k_sds_bwd_texel(SdsTexArgs a)
{
    const int lane = threadIdx.x & (GHR_SDS_WAVE - 1);
    const int q = blockIdx.x * (GHR_SDS_BLOCK / GHR_SDS_WAVE) + (threadIdx.x >> 6);
    const int GG = a.G * a.G;
    if (q >= GG) return;
    int32_t g[GHR_SDS_K];
    float w[GHR_SDS_K];
    for (int k = 0; k < GHR_SDS_K; k++) { g[k] = a.nbr[q * GHR_SDS_K + k]; w[k] = a.w[q * GHR_SDS_K + k]; }
    float part = 0.f;
    for (int c = lane; c < a.C; c += GHR_SDS_WAVE) {
        float zk[GHR_SDS_K];
        for (int k = 0; k < GHR_SDS_K; k++) zk[k] = a.z[(size_t)g[k] * a.C + c];
        part += a.d_texture[(size_t)c * GG + q] * sds_blend_dalpha(zk[0], sds_mix4(w, zk));
    }
    part = sds_wave_sum(part);
    if (lane == 0) a.dalpha_q[q] = part;
}

// backward 2, one wave per guiding strand, lane = channel: d z[g] and d alpha[g] over the strand's list in its order
__global__ void __launch_bounds__(GHR_SDS_BLOCK) k_sds_bwd_gather(SdsTexArgs a)
{
    const int lane = threadIdx.x & (GHR_SDS_WAVE - 1);
    const int g = blockIdx.x * (GHR_SDS_BLOCK / GHR_SDS_WAVE) + (threadIdx.x >> 6);
    const int GG = a.G * a.G;
    if (g >= a.N) return;
    const int beg = a.start[g], end = a.start[g + 1];
    float dal = 0.f;
    for (int t = beg; t < end; t++) {
        const int e = a.list[t];
        dal += a.dalpha_q[e >> 2] * a.w[e];
    }
    if (lane == 0) a.d_csim[g] = dal * sds_alpha_dc(a.csim[g]);
    for (int c = lane; c < a.C; c += GHR_SDS_WAVE) {
        float acc = 0.f;
        for (int t = beg; t < end; t++) {
            const int e = a.list[t], q = e >> 2;
            acc += a.d_texture[(size_t)c * GG + q] * sds_blend_dz(e & 3, a.w[e], a.alpha_q[q]);
        }
        a.d_z[(size_t)g * a.C + c] = acc;
    }
}

// backward 3, one wave per guiding strand, lane = segment: the texels q < N of its list pass d csim[q] to its segment vectors
__global__ void __launch_bounds__(GHR_SDS_BLOCK) k_sds_bwd_v(SdsTexArgs a)
{
    const int lane = threadIdx.x & (GHR_SDS_WAVE - 1);
    const int g = blockIdx.x * (GHR_SDS_BLOCK / GHR_SDS_WAVE) + (threadIdx.x >> 6);
    if (g >= a.N) return;
    const int beg = a.start[g], end = a.start[g + 1];
    for (int i = lane; i < a.n; i += GHR_SDS_WAVE) {
        float acc[3] = {0.f, 0.f, 0.f};
        for (int t = beg; t < end; t++) {
            const int e = a.list[t], q = e >> 2;
            if (q >= a.N) break;  // ascending q: the rest of the list has no csim row
            const float dc = (a.d_csim[q] / (float)GHR_SDS_PAIRS) / (float)a.n;
            float x[GHR_SDS_K][3], da[3];
            sds_load4(a, a.nbr + q * GHR_SDS_K, i, x);
            sds_pair_cos_vjp(x, e & 3, dc, da);
            for (int c = 0; c < 3; c++) acc[c] += da[c];
        }
        float* o = a.d_v + ((size_t)g * a.n + i) * 3;
        o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2];
    }
}

#endif  // __HIPCC__

}  // namespace ghr
