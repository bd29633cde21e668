// ghr_guides.h -- guiding strands of the textured generator (the reference's num_guiding_strands,
// src/scene/gaussian_model_strands.py:479-501 restated over STRANDS): the first N roots of a draw of S are the guides, fetched and
// decoded as they are; every other root's latent row is blended from its four nearest guides in UV by HAAR's cosine-similarity
// rule.  The networks, the texture fetch and the local frames are the caller's (csrc/ghr_texstrands.h).
//
//   neighbours    d2(s, g) = (u_s.x - u_g.x)^2 + (u_s.y - u_g.y)^2 over g < N, for EVERY s < S (guides included); the four smallest
//                 under (d2 ascending, then g ascending): sds_before; w = sds_weights(d2)
//   similarity    csim[g] = mean of the ten pair cosines j <= k of guide g's OWN four neighbours' segment vectors, averaged over
//                 the n segments; alpha[g] = sds_alpha(csim[g]).  The guides are the first N queries, so the reference block's
//                 alpha[g] = f(csim[q = g]) -- the indexing quirk csrc/ghr_sds.h reproduces for texels -- is here HAAR's eq. 4:
//                 a guide's coefficient comes from the guide's own neighbourhood.
//   blend         z[s] = z_g[s] for s < N; for s >= N  alpha_s = sum_k w_k alpha[nbr_k],
//                 z[s] = z_g[nbr_0] alpha_s + (sum_k w_k z_g[nbr_k]) (1 - alpha_s), all C channels (sds_mix4, sds_blend)
//
// Per-element arithmetic is ghr_sds.h's GHR_HD functions, unchanged; what is new is the mapping: one wave per drawn root
// (neighbours + similarity, blend, d alpha_s), one wave per guide (the gathers of the backward).  The backward is gather-form:
// per guide the list of the 4 s + k that chose it, ASCENDING, and every gradient is a sum in that order -- no floating-point
// atomics, two passes give the same bits.  The lists are built in O(S K) plus a sort of each list: k_gd_knn counts, k_gd_start
// scans the counts, k_gd_fill drops each choice into its guide's range in arrival order (integer atomics) and k_gd_lists ranks
// each range into ascending order -- whatever order the choices arrived in, the list is the same.
// tests/hostsim/ghr_hostsim_guides.cpp walks these loops on the CPU.
#pragma once
#include "ghr_sds.h"

#define GHR_GD_BLOCK 256  // four waves: four roots or four guides per workgroup

namespace ghr {

// the place of value x among the L distinct values of t: how many are smaller
GHR_HD int gd_rank(const int32_t* t, int L, int32_t x)
{
    int r = 0;
    for (int j = 0; j < L; j++) r += t[j] < x ? 1 : 0;
    return r;
}

// the chunk of counts a lane owns in the scan of k_gd_start
GHR_HD void gd_chunk(int N, int lane, int* lo, int* hi)
{
    const int per = (N + GHR_SDS_WAVE - 1) / GHR_SDS_WAVE;
    const long long a = (long long)lane * per, b = a + per;
    *lo = (int)(a < N ? a : N);
    *hi = (int)(b < N ? b : N);
}

#if defined(__HIPCC__)

struct GdArgs {
    int32_t S, N, n, C;
    const float* uvs;      // [S][2]: the drawn roots' UVs, the guides first
    const float* z_g;      // [N][C]
    const float* v_g;      // [N][n][3]
    int32_t* nbr;          // [S][4]
    float* w;              // [S][4]
    float* csim;           // [N]
    float* alpha;          // [N]
    float* alpha_s;        // [S]
    int32_t* count;        // [N]: zero on entry; how many (s, k) chose each guide; zero again after k_gd_fill
    int32_t* start;        // [N + 1]
    int32_t* unsorted;     // [4 S]: the lists in arrival order
    int32_t* list;         // [4 S]: 4 s + k, ascending within a guide
    float* z;              // [S][C]
    // backward
    const float* d_z;      // [S][C]
    float* dalpha_s;       // [S]
    float* d_csim;         // [N]
    float* d_zg;           // [N][C]
    float* d_vg;           // [N][n][3], may be NULL
};

__device__ __forceinline__ void gd_load4(const GdArgs& a, const int32_t* g, int i, float x[GHR_SDS_K][3])
{
    for (int m = 0; m < GHR_SDS_K; m++) {
        const float* p = a.v_g + ((size_t)g[m] * a.n + i) * 3;
        x[m][0] = p[0]; x[m][1] = p[1]; x[m][2] = p[2];
    }
}

// one wave per drawn root: lanes split the N guides, a butterfly merges their four; the guides' own waves (s < N) go on to the
// ten pair cosines with lane = segment
__global__ void __launch_bounds__(GHR_GD_BLOCK) k_gd_knn(GdArgs a)
{
    const int lane = threadIdx.x & (GHR_SDS_WAVE - 1);
    const int s = blockIdx.x * (GHR_GD_BLOCK / GHR_SDS_WAVE) + (threadIdx.x >> 6);
    if (s >= a.S) return;
    const float cx = a.uvs[2 * (size_t)s], cy = a.uvs[2 * (size_t)s + 1];
    SdsTop t;
    sds_top_init(t);
    for (int g = lane; g < a.N; g += GHR_SDS_WAVE) sds_top_insert(t, sds_dist2(cx, cy, a.uvs[2 * (size_t)g], a.uvs[2 * (size_t)g + 1]), g);
    for (int m = 1; m < GHR_SDS_WAVE; m <<= 1) {
        float od[GHR_SDS_K];
        int32_t og[GHR_SDS_K];
#pragma unroll
        for (int k = 0; k < GHR_SDS_K; k++) { od[k] = __shfl_xor(t.d[k], m, GHR_SDS_WAVE); og[k] = __shfl_xor(t.g[k], m, GHR_SDS_WAVE); }
#pragma unroll
        for (int k = 0; k < GHR_SDS_K; k++) sds_top_insert(t, od[k], og[k]);
    }
    // N >= 4: every slot holds a guide (sds_before); the clamp keeps a reader in bounds whatever the UVs are
    for (int k = 0; k < GHR_SDS_K; k++) t.g[k] = t.g[k] < 0 ? 0 : (t.g[k] >= a.N ? a.N - 1 : t.g[k]);
    float w[GHR_SDS_K];
    sds_weights(t.d, w);
    if (lane < GHR_SDS_K) {
        const int32_t g = lane == 0 ? t.g[0] : lane == 1 ? t.g[1] : lane == 2 ? t.g[2] : t.g[3];
        a.nbr[(size_t)s * GHR_SDS_K + lane] = g;
        a.w[(size_t)s * GHR_SDS_K + lane] = lane == 0 ? w[0] : lane == 1 ? w[1] : lane == 2 ? w[2] : w[3];
        atomicAdd(&a.count[g], 1);
    }
    if (s >= a.N) return;
    float acc[GHR_SDS_PAIRS];
    for (int p = 0; p < GHR_SDS_PAIRS; p++) acc[p] = 0.f;
    for (int i = lane; i < a.n; i += GHR_SDS_WAVE) {
        float x[GHR_SDS_K][3];
        gd_load4(a, t.g, i, x);
        sds_pair_cos(x, acc);
    }
    for (int p = 0; p < GHR_SDS_PAIRS; p++) acc[p] = sds_wave_sum(acc[p]);
    if (lane == 0) {
        const float c = sds_csim(acc, a.n);
        a.csim[s] = c;
        a.alpha[s] = sds_alpha(c);
    }
}

// one wave in all: each lane sums its chunk of the counts, an integer scan over the lanes, a second walk that writes
__global__ void __launch_bounds__(GHR_SDS_WAVE) k_gd_start(GdArgs a)
{
    const int lane = threadIdx.x;
    int lo, hi;
    gd_chunk(a.N, lane, &lo, &hi);
    int sum = 0;
    for (int g = lo; g < hi; g++) sum += a.count[g];
    int run = sum;
    for (int d = 1; d < GHR_SDS_WAVE; d <<= 1) {
        const int t = __shfl_up(run, d, GHR_SDS_WAVE);
        if (lane >= d) run += t;
    }
    run -= sum;
    for (int g = lo; g < hi; g++) { a.start[g] = run; run += a.count[g]; }
    if (hi == a.N && lo < hi) a.start[a.N] = run;
}

// one thread per choice e = 4 s + k: a place in its guide's range, counted down from the range's end in arrival order
__global__ void __launch_bounds__(GHR_GD_BLOCK) k_gd_fill(GdArgs a)
{
    const int e = blockIdx.x * GHR_GD_BLOCK + threadIdx.x;
    const int total = GHR_SDS_K * a.S;
    if (e >= total) return;
    const int g = a.nbr[e];
    const int at = a.start[g] + atomicSub(&a.count[g], 1) - 1;
    if (at >= 0 && at < total) a.unsorted[at] = e;
}

// one wave per guide: each choice of its range goes to the place of its rank -- ascending 4 s + k, integers only
__global__ void __launch_bounds__(GHR_GD_BLOCK) k_gd_lists(GdArgs a)
{
    const int lane = threadIdx.x & (GHR_SDS_WAVE - 1);
    const int g = blockIdx.x * (GHR_GD_BLOCK / GHR_SDS_WAVE) + (threadIdx.x >> 6);
    if (g >= a.N) return;
    const int beg = a.start[g], L = a.start[g + 1] - beg;
    const int total = GHR_SDS_K * a.S;
    if (beg < 0 || L < 0 || beg + L > total) return;
    for (int i = lane; i < L; i += GHR_SDS_WAVE) {
        const int32_t x = a.unsorted[beg + i];
        a.list[beg + gd_rank(a.unsorted + beg, L, x)] = x;
    }
}

// one wave per drawn root, lane = channel: a guide's row is copied, every other row blended
__global__ void __launch_bounds__(GHR_GD_BLOCK) k_gd_blend(GdArgs a)
{
    const int lane = threadIdx.x & (GHR_SDS_WAVE - 1);
    const int s = blockIdx.x * (GHR_GD_BLOCK / GHR_SDS_WAVE) + (threadIdx.x >> 6);
    if (s >= a.S) return;
    int32_t g[GHR_SDS_K];
    float w[GHR_SDS_K], al[GHR_SDS_K];
    for (int k = 0; k < GHR_SDS_K; k++) { g[k] = a.nbr[(size_t)s * GHR_SDS_K + k]; w[k] = a.w[(size_t)s * GHR_SDS_K + k]; al[k] = a.alpha[g[k]]; }
    const float as = sds_mix4(w, al);
    if (lane == 0) a.alpha_s[s] = as;
    float* out = a.z + (size_t)s * a.C;
    if (s < a.N) {
        for (int c = lane; c < a.C; c += GHR_SDS_WAVE) out[c] = a.z_g[(size_t)s * a.C + c];
        return;
    }
    for (int c = lane; c < a.C; c += GHR_SDS_WAVE) {
        float zk[GHR_SDS_K];
        for (int k = 0; k < GHR_SDS_K; k++) zk[k] = a.z_g[(size_t)g[k] * a.C + c];
        out[c] = sds_blend(zk[0], sds_mix4(w, zk), as);
    }
}

// backward 1, one wave per drawn root: d alpha_s = sum_c d z[s][c] (z_g[nbr_0][c] - bilinear[c]); 0 for a guide's copied row
__global__ void __launch_bounds__(GHR_GD_BLOCK) k_gd_dalpha(GdArgs a)
{
    const int lane = threadIdx.x & (GHR_SDS_WAVE - 1);
    const int s = blockIdx.x * (GHR_GD_BLOCK / GHR_SDS_WAVE) + (threadIdx.x >> 6);
    if (s >= a.S) return;
    if (s < a.N) {
        if (lane == 0) a.dalpha_s[s] = 0.f;
        return;
    }
    int32_t g[GHR_SDS_K];
    float w[GHR_SDS_K];
    for (int k = 0; k < GHR_SDS_K; k++) { g[k] = a.nbr[(size_t)s * GHR_SDS_K + k]; w[k] = a.w[(size_t)s * GHR_SDS_K + k]; }
    float part = 0.f;
    for (int c = lane; c < a.C; c += GHR_SDS_WAVE) {
        float zk[GHR_SDS_K];
        for (int k = 0; k < GHR_SDS_K; k++) zk[k] = a.z_g[(size_t)g[k] * a.C + c];
        part += a.d_z[(size_t)s * a.C + c] * sds_blend_dalpha(zk[0], sds_mix4(w, zk));
    }
    part = sds_wave_sum(part);
    if (lane == 0) a.dalpha_s[s] = part;
}

// backward 2, one wave per guide, lane = channel: d z_g[g] = its own row's cotangent, then the interpolated rows of its list in
// their order; d alpha[g] over the same rows, through to d csim[g]
__global__ void __launch_bounds__(GHR_GD_BLOCK) k_gd_gather(GdArgs a)
{
    const int lane = threadIdx.x & (GHR_SDS_WAVE - 1);
    const int g = blockIdx.x * (GHR_GD_BLOCK / GHR_SDS_WAVE) + (threadIdx.x >> 6);
    if (g >= a.N) return;
    const int beg = a.start[g], end = a.start[g + 1];
    float dal = 0.f;
    for (int t = beg; t < end; t++) {
        const int e = a.list[t], s = e >> 2;
        if (s < a.N || s >= a.S) continue;  // a guide's row is a copy: it has no alpha_s
        dal += a.dalpha_s[s] * a.w[e];
    }
    if (lane == 0) a.d_csim[g] = dal * sds_alpha_dc(a.csim[g]);
    for (int c = lane; c < a.C; c += GHR_SDS_WAVE) {
        float acc = a.d_z[(size_t)g * a.C + c];
        for (int t = beg; t < end; t++) {
            const int e = a.list[t], s = e >> 2;
            if (s < a.N || s >= a.S) continue;
            acc += a.d_z[(size_t)s * a.C + c] * sds_blend_dz(e & 3, a.w[e], a.alpha_s[s]);
        }
        a.d_zg[(size_t)g * a.C + c] = acc;
    }
}

// backward 3, one wave per guide, lane = segment: the guides q < N of its list pass d csim[q] to its segment vectors
__global__ void __launch_bounds__(GHR_GD_BLOCK) k_gd_bwd_v(GdArgs a)
{
    const int lane = threadIdx.x & (GHR_SDS_WAVE - 1);
    const int g = blockIdx.x * (GHR_GD_BLOCK / GHR_SDS_WAVE) + (threadIdx.x >> 6);
    if (g >= a.N) return;
    const int beg = a.start[g], end = a.start[g + 1];
    for (int i = lane; i < a.n; i += GHR_SDS_WAVE) {
        float acc[3] = {0.f, 0.f, 0.f};
        for (int t = beg; t < end; t++) {
            const int e = a.list[t], q = e >> 2;
            if (q < 0 || q >= a.N) break;  // ascending: the rest of the list are interpolated rows, which have no csim
            const float dc = (a.d_csim[q] / (float)GHR_SDS_PAIRS) / (float)a.n;
            float x[GHR_SDS_K][3], da[3];
            gd_load4(a, a.nbr + (size_t)q * GHR_SDS_K, i, x);
            sds_pair_cos_vjp(x, e & 3, dc, da);
            for (int c = 0; c < 3; c++) acc[c] += da[c];
        }
        float* o = a.d_vg + ((size_t)g * a.n + i) * 3;
        o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2];
    }
}

#endif  // __HIPCC__

}  // namespace ghr
