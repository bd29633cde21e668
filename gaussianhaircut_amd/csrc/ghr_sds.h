// ghr_sds.h -- the strand stage's prior term between its two networks (src/scene/gaussian_model_strands.py:456-503
// restated): guiding strands into their scalp-local frames, and the G x G latent texture blended from each texel's four nearest
// guiding strands in UV space by HAAR's cosine-similarity rule.  The strand encoder and the prior's loss are the caller's.
//
//   local frame   P[g, j] = sum_{i < j} dirs[idx[g], i],  e[g, j] = (M P[g, j]) scale,  v[g, j] = (M dirs[idx[g], j]) scale,
//                 M = local2world[idx[g]]^-1 (given, or the adjugate form sds_inv3 of the given frame)
//   texture       the HAAR blend of csrc/ghr_haar.h with the G G texels as its queries (HaarTexels): texel q's UV is
//                 (centres[q % G], centres[q / G]), the output is channel-major [C][G][G], and alpha[g] reads csim[q = g] (the
//                 reference's indexing: strand g's coefficient comes from the neighbourhood of TEXEL number g)
//
// Mapping: one wave per guiding strand (local frame, lists).  The blend's backward is gather-form: k_sds_lists leaves, per
// guiding strand, the (q, k) that chose it in ascending q (integer counting only): one launch that walks all 4 G G choices per
// guiding strand, which is cheap at the prior's size.  Per-element arithmetic is GHR_HD: tests/hostsim/ghr_hostsim_sds.cpp runs
// it on the CPU.
#pragma once
#include "ghr_haar.h"

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

// the chunk of segments a lane owns in the local-frame scans
GHR_HD void sds_chunk(int n, int lane, int* lo, int* hi)
{
    const int per = (n + GHR_SDS_WAVE - 1) / GHR_SDS_WAVE;
    const int a = lane * per, b = a + per;
    *lo = a < n ? a : n;
    *hi = b < n ? b : n;
}

#if defined(__HIPCC__)

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

// one wave per guiding strand: its place in the lists is the sum of the counts below it; then a walk over all 4 G G choices
// in order, each lane's match placed by the ballot's prefix -- ascending (q, k), integers only
__global__ void __launch_bounds__(GHR_SDS_BLOCK) k_sds_lists(HaarArgs a)
{
    const int lane = threadIdx.x & (GHR_SDS_WAVE - 1);
    const int g = blockIdx.x * (GHR_SDS_BLOCK / GHR_SDS_WAVE) + (threadIdx.x >> 6);
    if (g >= a.N) return;
    int base = 0;
    for (int h = lane; h < g; h += GHR_SDS_WAVE) base += a.count[h];
    for (int m = 1; m < GHR_SDS_WAVE; m <<= 1) base += __shfl_xor(base, m, GHR_SDS_WAVE);
    const int total = GHR_SDS_K * a.Q;
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

#endif  // __HIPCC__

}  // namespace ghr
