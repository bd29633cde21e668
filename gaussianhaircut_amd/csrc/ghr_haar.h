// ghr_haar.h -- HAAR's blend of a latent row from its four nearest guiding strands, once, for both of its users: the G x G
// latent texture of the strand stage's prior term (ghr_sds.h) and the drawn roots of the textured generator
// (ghr_guides.h).  Q queries, N guiding strands:
//
//   neighbours    d2(q, g) = (cx - u_g)^2 + (cy - v_g)^2; the four smallest under (d2 ascending, then g ascending): a total
//                 order when no distance is NaN, so the answer then does not depend on how the candidates are split or merged
//   similarity    cos(a, b) = (a / max(|a|, 1e-8)) . (b / max(|b|, 1e-8)); csim_full[j][k] = mean over segments;
//                 csim[q] = mean of the ten pairs j <= k, for query q < N -- and alpha[g] reads csim[q = g]
//   blend         alpha_q = sum_k w_k alpha[nbr_k],  out_q = z[nbr_0] alpha_q + (sum_k w_k z[nbr_k]) (1 - alpha_q)
//
// The two users differ in a query policy and in nothing else: where query q's UV comes from, where (q, c) lies in the output and
// in its cotangent, and whether the first N queries ARE the guiding strands (their rows are then copies: no blend, no alpha_q).
//
// Mapping: one wave per query (neighbours + similarity, blend, d alpha_q), one wave per guiding strand (the gathers of the
// backward).  The backward is gather-form over per-guide lists of the 4 q + k that chose it, ascending (each user builds them its
// own way), and every gradient is a sum in that order -- no floating-point atomics, two passes give the same bits.  Per-element
// arithmetic and the policies are GHR_HD: tests/hostsim/ghr_hostsim_haar.h runs them on the CPU.
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
#define GHR_SDS_BLOCK 256  // four waves: four queries or four guiding strands per workgroup
#define GHR_SDS_DIST_EPS 1e-7f
#define GHR_SDS_COS_EPS 1e-8f
#define GHR_SDS_CSIM_KNEE 0.9f

namespace ghr {

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

// d out_q / d z[nbr_k]
GHR_HD float sds_blend_dz(int k, float w_k, float alpha_q) { return (k == 0 ? alpha_q : 0.f) + w_k * (1.f - alpha_q); }

// d out_q / d alpha_q, per channel
GHR_HD float sds_blend_dalpha(float z0, float bil) { return z0 - bil; }

// ---- one argument struct, two query policies ----------------------------------------------------------------------------------
struct HaarArgs {
    int32_t Q, N, n, C, G;  // Q queries: G G texels, or the drawn roots; G: the texels' only
    const float* uvg;       // [N][2]: the guiding strands' UVs ([Q][2], the guides first, when the queries are the drawn roots)
    const float* centres;   // [G]: the texel centres along one axis; the texels' only
    const float* z;         // [N][C]
    const float* v;         // [N][n][3]
    int32_t* nbr;           // [Q][4]
    float* w;               // [Q][4]
    float* csim;            // [N]: of QUERY q < N
    float* alpha;           // [N]
    float* alpha_q;         // [Q]
    int32_t* count;         // [N]: zero on entry; how many (q, k) chose each guiding strand
    int32_t* start;         // [N + 1]
    int32_t* unsorted;      // [4 Q]: the lists in arrival order; k_gd_fill / k_gd_lists only
    int32_t* list;          // [4 Q]: 4 q + k, ascending within a guiding strand
    float* out;             // Policy::at(q, c): the texture [C][G][G], or the roots' rows [Q][C]
    // backward
    const float* d_out;     // as out
    float* dalpha_q;        // [Q]
    float* d_csim;          // [N]
    float* d_z;             // [N][C]
    float* d_v;             // [N][n][3], may be NULL
};

// the texels of the latent texture: centres on a grid, the output channel-major (a lane stride of 4 Q bytes)
struct HaarTexels {
    static constexpr bool guides_first = false;
    static GHR_HD void uv(const HaarArgs& a, int q, float* cx, float* cy) { *cx = a.centres[q % a.G]; *cy = a.centres[q / a.G]; }
    static GHR_HD size_t at(const HaarArgs& a, int q, int c) { return (size_t)c * a.Q + q; }
};

// the drawn roots of the generator: their own UVs, the output row-major, and the first N of them are the guides themselves
struct HaarRoots {
    static constexpr bool guides_first = true;
    static GHR_HD void uv(const HaarArgs& a, int q, float* cx, float* cy) { *cx = a.uvg[2 * (size_t)q]; *cy = a.uvg[2 * (size_t)q + 1]; }
    static GHR_HD size_t at(const HaarArgs& a, int q, int c) { return (size_t)q * a.C + c; }
};

// a list entry's query has a blended row: inside the queries and, where the first N are the guides' copied rows, past them
template <class P>
GHR_HD bool haar_blended(const HaarArgs& a, int q) { return q >= (P::guides_first ? a.N : 0) && q < a.Q; }

#if defined(__HIPCC__)

__device__ __forceinline__ float sds_wave_sum(float x)
{
    for (int m = 1; m < GHR_SDS_WAVE; m <<= 1) x += __shfl_xor(x, m, GHR_SDS_WAVE);
    return x;
}

__device__ __forceinline__ void haar_load4(const HaarArgs& a, const int32_t* g, int i, float x[GHR_SDS_K][3])
{
    for (int m = 0; m < GHR_SDS_K; m++) {
        const float* p = a.v + ((size_t)g[m] * a.n + i) * 3;
        x[m][0] = p[0]; x[m][1] = p[1]; x[m][2] = p[2];
    }
}

// one wave per query: lanes split the N candidates, a butterfly merges their four; queries q < N go on to the ten pair cosines
// with lane = segment
template <class P>
__global__ void __launch_bounds__(GHR_SDS_BLOCK) k_haar_knn(HaarArgs a)
{
    const int lane = threadIdx.x & (GHR_SDS_WAVE - 1);
    const int q = blockIdx.x * (GHR_SDS_BLOCK / GHR_SDS_WAVE) + (threadIdx.x >> 6);
    if (q >= a.Q) return;
    float cx, cy;
    P::uv(a, q, &cx, &cy);
    SdsTop t;
    sds_top_init(t);
    for (int g = lane; g < a.N; g += GHR_SDS_WAVE) sds_top_insert(t, sds_dist2(cx, cy, a.uvg[2 * (size_t)g], a.uvg[2 * (size_t)g + 1]), g);
    for (int m = 1; m < GHR_SDS_WAVE; m <<= 1) {
        float od[GHR_SDS_K];
        int32_t og[GHR_SDS_K];
#pragma unroll
        for (int k = 0; k < GHR_SDS_K; k++) { od[k] = __shfl_xor(t.d[k], m, GHR_SDS_WAVE); og[k] = __shfl_xor(t.g[k], m, GHR_SDS_WAVE); }
#pragma unroll
        for (int k = 0; k < GHR_SDS_K; k++) sds_top_insert(t, od[k], og[k]);
    }
    // N >= 4: every slot holds a guiding strand (sds_before); the clamp keeps a reader in bounds whatever the UVs are
    for (int k = 0; k < GHR_SDS_K; k++) t.g[k] = t.g[k] < 0 ? 0 : (t.g[k] >= a.N ? a.N - 1 : t.g[k]);
    float w[GHR_SDS_K];
    sds_weights(t.d, w);
    if (lane < GHR_SDS_K) {
        const int32_t g = lane == 0 ? t.g[0] : lane == 1 ? t.g[1] : lane == 2 ? t.g[2] : t.g[3];
        a.nbr[(size_t)q * GHR_SDS_K + lane] = g;
        a.w[(size_t)q * GHR_SDS_K + lane] = lane == 0 ? w[0] : lane == 1 ? w[1] : lane == 2 ? w[2] : w[3];
        atomicAdd(&a.count[g], 1);
    }
    if (q >= a.N) return;
    float acc[GHR_SDS_PAIRS];
    for (int p = 0; p < GHR_SDS_PAIRS; p++) acc[p] = 0.f;
    for (int i = lane; i < a.n; i += GHR_SDS_WAVE) {
        float x[GHR_SDS_K][3];
        haar_load4(a, t.g, i, x);
        sds_pair_cos(x, acc);
    }
    for (int p = 0; p < GHR_SDS_PAIRS; p++) acc[p] = sds_wave_sum(acc[p]);
    if (lane == 0) {
        const float c = sds_csim(acc, a.n);
        a.csim[q] = c;
        a.alpha[q] = sds_alpha(c);
    }
}

// one wave per query, lane = channel: a guide's own row is copied, every other row blended
template <class P>
__global__ void __launch_bounds__(GHR_SDS_BLOCK) k_haar_blend(HaarArgs a)
{
    const int lane = threadIdx.x & (GHR_SDS_WAVE - 1);
    const int q = blockIdx.x * (GHR_SDS_BLOCK / GHR_SDS_WAVE) + (threadIdx.x >> 6);
    if (q >= a.Q) return;
    int32_t g[GHR_SDS_K];
    float w[GHR_SDS_K], al[GHR_SDS_K];
    for (int k = 0; k < GHR_SDS_K; k++) { g[k] = a.nbr[(size_t)q * GHR_SDS_K + k]; w[k] = a.w[(size_t)q * GHR_SDS_K + k]; al[k] = a.alpha[g[k]]; }
    const float aq = sds_mix4(w, al);
    if (lane == 0) a.alpha_q[q] = aq;
    if (P::guides_first && q < a.N) {
        for (int c = lane; c < a.C; c += GHR_SDS_WAVE) a.out[P::at(a, q, c)] = a.z[(size_t)q * a.C + c];
        return;
    }
    for (int c = lane; c < a.C; c += GHR_SDS_WAVE) {
        float zk[GHR_SDS_K];
        for (int k = 0; k < GHR_SDS_K; k++) zk[k] = a.z[(size_t)g[k] * a.C + c];
        a.out[P::at(a, q, c)] = sds_blend(zk[0], sds_mix4(w, zk), aq);
    }
}

// backward 1, one wave per query: d alpha_q = sum_c d out_q[c] (z[nbr_0][c] - bilinear[c]); 0 for a guide's copied row
template <class P>
__global__ void __launch_bounds__(GHR_SDS_BLOCK) k_haar_dalpha(HaarArgs a)
{
    const int lane = threadIdx.x & (GHR_SDS_WAVE - 1);
    const int q = blockIdx.x * (GHR_SDS_BLOCK / GHR_SDS_WAVE) + (threadIdx.x >> 6);
    if (q >= a.Q) return;
    if (P::guides_first && q < a.N) {
        if (lane == 0) a.dalpha_q[q] = 0.f;
        return;
    }
    int32_t g[GHR_SDS_K];
    float w[GHR_SDS_K];
    for (int k = 0; k < GHR_SDS_K; k++) { g[k] = a.nbr[(size_t)q * GHR_SDS_K + k]; w[k] = a.w[(size_t)q * GHR_SDS_K + k]; }
    float part = 0.f;
    for (int c = lane; c < a.C; c += GHR_SDS_WAVE) {
        float zk[GHR_SDS_K];
        for (int k = 0; k < GHR_SDS_K; k++) zk[k] = a.z[(size_t)g[k] * a.C + c];
        part += a.d_out[P::at(a, q, c)] * sds_blend_dalpha(zk[0], sds_mix4(w, zk));
    }
    part = sds_wave_sum(part);
    if (lane == 0) a.dalpha_q[q] = part;
}

// backward 2, one wave per guiding strand, lane = channel: d z[g] = its own row's cotangent where it is a query itself, then the
// blended rows of its list in their order; d alpha[g] over the same rows, through to d csim[g]
template <class P>
__global__ void __launch_bounds__(GHR_SDS_BLOCK) k_haar_gather(HaarArgs a)
{
    const int lane = threadIdx.x & (GHR_SDS_WAVE - 1);
    const int g = blockIdx.x * (GHR_SDS_BLOCK / GHR_SDS_WAVE) + (threadIdx.x >> 6);
    if (g >= a.N) return;
    const int beg = a.start[g], end = a.start[g + 1];
    float dal = 0.f;
    for (int t = beg; t < end; t++) {
        const int e = a.list[t], q = e >> 2;
        if (!haar_blended<P>(a, q)) continue;
        dal += a.dalpha_q[q] * a.w[e];
    }
    if (lane == 0) a.d_csim[g] = dal * sds_alpha_dc(a.csim[g]);
    for (int c = lane; c < a.C; c += GHR_SDS_WAVE) {
        float acc = P::guides_first ? a.d_out[P::at(a, g, c)] : 0.f;
        for (int t = beg; t < end; t++) {
            const int e = a.list[t], q = e >> 2;
            if (!haar_blended<P>(a, q)) continue;
            acc += a.d_out[P::at(a, q, c)] * sds_blend_dz(e & 3, a.w[e], a.alpha_q[q]);
        }
        a.d_z[(size_t)g * a.C + c] = acc;
    }
}

// backward 3, one wave per guiding strand, lane = segment: the queries q < N of its list pass d csim[q] to its segment vectors
template <class P>
__global__ void __launch_bounds__(GHR_SDS_BLOCK) k_haar_bwd_v(HaarArgs a)
{
    const int lane = threadIdx.x & (GHR_SDS_WAVE - 1);
    const int g = blockIdx.x * (GHR_SDS_BLOCK / GHR_SDS_WAVE) + (threadIdx.x >> 6);
    if (g >= a.N) return;
    const int beg = a.start[g], end = a.start[g + 1];
    for (int i = lane; i < a.n; i += GHR_SDS_WAVE) {
        float acc[3] = {0.f, 0.f, 0.f};
        for (int t = beg; t < end; t++) {
            const int e = a.list[t], q = e >> 2;
            if (q < 0 || q >= a.N) break;  // ascending q: the rest of the list has no csim row
            const float dc = (a.d_csim[q] / (float)GHR_SDS_PAIRS) / (float)a.n;
            float x[GHR_SDS_K][3], da[3];
            haar_load4(a, a.nbr + (size_t)q * GHR_SDS_K, i, x);
            sds_pair_cos_vjp(x, e & 3, dc, da);
            for (int c = 0; c < 3; c++) acc[c] += da[c];
        }
        float* o = a.d_v + ((size_t)g * a.n + i) * 3;
        o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2];
    }
}

#endif  // __HIPCC__

}  // namespace ghr
