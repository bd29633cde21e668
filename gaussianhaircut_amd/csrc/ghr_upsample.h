// ghr_upsample.h -- groom upsampling: child strands blended from guide strands.  The optimised strands are the
// guides; every other scalp root gets a strand that is a blend of its nearest guides, each expressed in its own scalp-local frame
// and gated by shape similarity, so that strands on two sides of a parting are not averaged into one that stands up between them.
// Forward only: no backward, no floating-point atomics.
//
// The definition (ours, exact).  Everything is float32 without contraction, in the order written: + - * / and sqrtf.
//   inputs      gp [G][L][3]: the guides' points, L >= 2, the root gp[g][0];  gM [G][3][3]: their local2world frames, row-major,
//               columns (tangent, bitangent, normal);  gf [G][F]: optional features, F >= 0;  co [N][3], cM [N][3][3]: the children's
//               origins and frames;  r2: the squared search radius (+inf: no cut);  eps2 > 0;  tau in [-1, 1) with a flag `gate`.
//   products    M^T x = ((M[c]*x0 + M[3+c]*x1) + M[6+c]*x2), c = 0..2 (sds_mtv's bracketing);  M x = ((M[3r]*x0 + M[3r+1]*x1) +
//               M[3r+2]*x2) (sds_mv's);  a . b = (a0*b0 + a1*b1) + a2*b2.
//   neighbours  (k_ups_near) child c gets its 4 nearest guides by d2 = ((dx*dx) + (dy*dy)) + (dz*dz), dx = gp[g][0].x - co[c].x:
//               k_shape_nbr's rule -- the candidates are visited in ascending index and inserted on strict `<` into a sorted top-4
//               that starts at +inf, so equal distances go to the lower index and a candidate whose d2 is +inf or NaN is never
//               taken.  An entry is -1, and its d2 +inf, where d2 > r2 or no candidate was taken.  nbr [N][4] int32, nd2 [N][4].
//   the list    k runs over the LEADING entries with 0 <= nbr[c][k] < G: any other value ends the list and is never dereferenced.
//               K is their number, g_k = nbr[c][k].
//   similarity  e_k[i] = gM[g_k]^T (gp[g_k][i+1] - gp[g_k][i]), i < n = L - 1.  For k > 0 (only when K > 1):
//               D_k = sum_i e_k[i] . e_0[i],  A_k = sum_i e_k[i] . e_k[i],  A_0 = sum_i e_0[i] . e_0[i];
//               den = sqrtf(A_k) * sqrtf(A_0);  s_k = den > 0 ? D_k / den : 0;
//               q_k = gate ? clamp01((s_k - tau) / (1 - tau)) : 1,  clamp01(x) = x < 0 ? 0 : (x > 1 ? 1 : x);  q_0 = 1 exactly.
//               Order of each sum: per lane the segments lane, lane + 64, ... ascending; then the butterfly a += a[lane ^ m],
//               m = 1, 2, ... 32 (every lane ends with the same bits), as in ghr_shape.h.
//   weights     a_k = q_k / (nd2[c][k] + eps2);  W = a_0, then + a_1, ... in k order;  w_k = a_k / W;  w_k = 0 for k >= K.
//   points      r_k[j] = gM[g_k]^T (gp[g_k][j] - gp[g_k][0]);  Pl[j] = w_0 * r_0[j], then + w_1 * r_1[j], ... in k order;
//               out[c][j] = co[c] + cM[c] Pl[j] for j > 0, and out[c][0] = co[c] (assigned: exact whatever the sign of a zero).
//   features    of[c][f] = w_0 * gf[g_0][f], then + w_1 * gf[g_1][f], ... in k order.
//   no list     K == 0: valid[c] = 0, the weights 0, every point co[c], every feature 0.  Otherwise valid[c] = 1.
// There is no running sum along a strand: every point depends only on its own column of the guides, so a result's bits depend on
// the inputs alone, not on the launch.  Every element of nbr, nd2, out [N][L][3], w [N][4], of [N][F] and valid [N] is written.
//
// Mapping: k_ups_near one lane per child, 256 per workgroup, the guide roots staged through LDS in tiles of 256 (every lane reads
// the same LDS address: a broadcast).  k_ups_blend one wave per child, four per workgroup, lane = point in chunks of 64; a lane's
// segment needs the neighbouring lane's point, which comes from memory at the chunk's edge; the five frames, the list and the
// weights are wave-uniform; a child with a single neighbour skips the similarity pass.  The guide rows are read a second time for
// the blend (from cache: the four rows are 4.8 KB at L = 100) rather than kept in registers, which would bound L.
// Per-element functions are GHR_HD and the header is plain C++ outside __HIPCC__ (tests/hostsim/ghr_hostsim_upsample.cpp walks them).
#pragma once
#include "ghr_shape.h"  // ShapeTop, shape_dist2, shape_top_insert: the neighbour rule is k_shape_nbr's

#define GHR_UPS_K 4
#define GHR_UPS_WAVE 64
#define GHR_UPS_BLOCK 256  // k_ups_near: 256 children; k_ups_blend: four waves, four children
#define GHR_UPS_TILE 256   // guide roots per LDS tile of k_ups_near

namespace ghr {

GHR_HD float ups_dot(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// o = M^T x
GHR_HD void ups_mtv(const float* M, const float* x, float* o)
{
    for (int c = 0; c < 3; c++) o[c] = (M[c] * x[0] + M[3 + c] * x[1]) + M[6 + c] * x[2];
}

// o = M x
GHR_HD void ups_mv(const float* M, const float* x, float* o)
{
    for (int r = 0; r < 3; r++) o[r] = (M[3 * r] * x[0] + M[3 * r + 1] * x[1]) + M[3 * r + 2] * x[2];
}

// o = M^T (a - b): a segment (a = the next point, b = this one) or a point relative to its root (b = the root)
GHR_HD void ups_local(const float* M, const float* a, const float* b, float* o)
{
    const float d[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]};
    ups_mtv(M, d, o);
}

// the neighbour entry k of a sorted top-4 and its squared distance under the cut
GHR_HD int32_t ups_entry(const ShapeTop& t, int k, float r2, float* d2)
{
    const int32_t j = shape_top_entry(t, k, r2);
    *d2 = j >= 0 ? t.d[k] : INFINITY;
    return j;
}

// K: the leading entries inside [0, G)
GHR_HD int ups_count(const int32_t* nbr, int G)
{
    int K = 0;
    bool open = true;
    for (int k = 0; k < GHR_UPS_K; k++) {
        open = open && (uint32_t)nbr[k] < (uint32_t)G;
        K += open ? 1 : 0;
    }
    return K;
}

GHR_HD float ups_clamp01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }

// q_k of one later neighbour from its three sums
GHR_HD float ups_gate(float D, float Ak, float A0, float tau, int gate)
{
    const float den = sqrtf(Ak) * sqrtf(A0);
    const float s = den > 0.f ? D / den : 0.f;
    return gate ? ups_clamp01((s - tau) / (1.f - tau)) : 1.f;
}

// the weights of a child with K >= 1 neighbours; q[0] is not read (q_0 = 1)
GHR_HD void ups_weights(int K, const float* q, const float* nd2, float eps2, float* w)
{
    float a[GHR_UPS_K], W = 0.f;
    for (int k = 0; k < GHR_UPS_K; k++) {
        a[k] = k < K ? (k == 0 ? 1.f : q[k]) / (nd2[k] + eps2) : 0.f;
        if (k < K) W = k == 0 ? a[0] : W + a[k];
    }
    for (int k = 0; k < GHR_UPS_K; k++) w[k] = k < K ? a[k] / W : 0.f;
}

// out = co + cM Pl
GHR_HD void ups_world(const float* co, const float* cM, const float* Pl, float* out)
{
    float o[3];
    ups_mv(cM, Pl, o);
    for (int c = 0; c < 3; c++) out[c] = co[c] + o[c];
}

struct UpsArgs {
    int G, L, F, N;
    const float* gp;      // [G][L][3]
    const float* gM;      // [G][3][3]
    const float* gf;      // [G][F] or NULL when F == 0
    const float* co;      // [N][3]
    const float* cM;      // [N][3][3]
    const int32_t* nbr;   // [N][4]
    const float* nd2;     // [N][4]
    float eps2, tau;
    int gate;
    float* out;           // [N][L][3]
    float* w;             // [N][4]
    float* of;            // [N][F] or NULL when F == 0
    uint8_t* valid;       // [N]
};

#if defined(__HIPCC__)

// One lane per child; the guide roots go through LDS in tiles of GHR_UPS_TILE, in ascending index.
__global__ void __launch_bounds__(GHR_UPS_BLOCK) k_ups_near(int G, const float* __restrict__ groots, int N, const float* __restrict__ co,
                                                            float r2, int32_t* __restrict__ nbr, float* __restrict__ nd2)
{
    __shared__ float tile[3][GHR_UPS_TILE];
    const int t = threadIdx.x;
    const long long c = (long long)blockIdx.x * GHR_UPS_BLOCK + t;
    const bool has = c < N;
    const size_t cq = has ? (size_t)c : (size_t)N - 1;
    const float q[3] = {co[3 * cq], co[3 * cq + 1], co[3 * cq + 2]};
    ShapeTop top;
    shape_top_init(top);
    for (int base = 0; base < G; base += GHR_UPS_TILE) {
        const int count = min(GHR_UPS_TILE, G - base);
        __syncthreads();  // every lane is done with the previous tile
        if (t < count)
            for (int x = 0; x < 3; x++) tile[x][t] = groots[3 * (size_t)(base + t) + x];
        __syncthreads();
        for (int j = 0; j < count; j++)
            shape_top_insert(top, shape_dist2(q, tile[0][j], tile[1][j], tile[2][j]), base + j);  // every lane reads the same address
    }
    if (has)
        for (int k = 0; k < GHR_UPS_K; k++) {
            float d2;
            nbr[GHR_UPS_K * (size_t)c + k] = ups_entry(top, k, r2, &d2);
            nd2[GHR_UPS_K * (size_t)c + k] = d2;
        }
}

// One wave per child, a lane per point in chunks of 64.
__global__ void __launch_bounds__(GHR_UPS_BLOCK) k_ups_blend(UpsArgs a)
{
    const int lane = threadIdx.x & (GHR_UPS_WAVE - 1);
    const long long cl = (long long)blockIdx.x * (GHR_UPS_BLOCK / GHR_UPS_WAVE) + (threadIdx.x >> 6);
    if (cl >= a.N) return;
    const size_t c = (size_t)cl;
    const int L = a.L, n = L - 1, F = a.F;
    int32_t e4[GHR_UPS_K];
    float d4[GHR_UPS_K];
#pragma unroll
    for (int k = 0; k < GHR_UPS_K; k++) {
        e4[k] = __builtin_amdgcn_readfirstlane(a.nbr[GHR_UPS_K * c + k]);
        d4[k] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, a.nd2[GHR_UPS_K * c + k])));
    }
    const int K = ups_count(e4, a.G);
    float* out = a.out + c * (size_t)L * 3;
    float o[3], cM[9];
#pragma unroll
    for (int x = 0; x < 3; x++) o[x] = a.co[3 * c + x];
#pragma unroll
    for (int x = 0; x < 9; x++) cM[x] = a.cM[9 * c + x];
    if (K == 0) {
        for (int j = lane; j < L; j += GHR_UPS_WAVE) { out[3 * j] = o[0]; out[3 * j + 1] = o[1]; out[3 * j + 2] = o[2]; }
        for (int f = lane; f < F; f += GHR_UPS_WAVE) a.of[c * (size_t)F + f] = 0.f;
        if (lane < GHR_UPS_K) a.w[GHR_UPS_K * c + lane] = 0.f;
        if (lane == 0) a.valid[c] = 0;
        return;
    }
    const float* row[GHR_UPS_K];
    float M[GHR_UPS_K][9];
#pragma unroll
    for (int k = 0; k < GHR_UPS_K; k++) {
        const size_t g = (size_t)(k < K ? e4[k] : e4[0]);  // (k >= K: an address that is never read)
        row[k] = a.gp + g * (size_t)L * 3;
#pragma unroll
        for (int x = 0; x < 9; x++) M[k][x] = k < K ? a.gM[9 * g + x] : 0.f;
    }
    float q[GHR_UPS_K] = {1.f, 1.f, 1.f, 1.f};
    if (K > 1) {
        float D[GHR_UPS_K] = {0.f, 0.f, 0.f, 0.f}, A[GHR_UPS_K] = {0.f, 0.f, 0.f, 0.f};
        for (int base = 0; base < n; base += GHR_UPS_WAVE) {
            const int i = base + lane;
            const bool has = i < n;
            float e0[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < GHR_UPS_K; k++) {
                if (k >= K) continue;  // wave-uniform
                float p[3] = {0.f, 0.f, 0.f}, pn[3];
                if (i < L) { p[0] = row[k][3 * i]; p[1] = row[k][3 * i + 1]; p[2] = row[k][3 * i + 2]; }
#pragma unroll
                for (int x = 0; x < 3; x++) pn[x] = __shfl_down(p[x], 1, GHR_UPS_WAVE);
                if (lane == GHR_UPS_WAVE - 1 && has) { pn[0] = row[k][3 * i + 3]; pn[1] = row[k][3 * i + 4]; pn[2] = row[k][3 * i + 5]; }  // the chunk's edge
                if (!has) continue;
                float e[3];
                ups_local(M[k], pn, p, e);
                if (k == 0) {
                    e0[0] = e[0]; e0[1] = e[1]; e0[2] = e[2];
                    A[0] = A[0] + ups_dot(e, e);
                } else {
                    D[k] = D[k] + ups_dot(e, e0);
                    A[k] = A[k] + ups_dot(e, e);
                }
            }
        }
        A[0] = shape_wave_sum(A[0]);
#pragma unroll
        for (int k = 1; k < GHR_UPS_K; k++) {
            if (k >= K) continue;
            q[k] = ups_gate(shape_wave_sum(D[k]), shape_wave_sum(A[k]), A[0], a.tau, a.gate);
        }
    }
    float w[GHR_UPS_K];
    ups_weights(K, q, d4, a.eps2, w);
    for (int base = 0; base < L; base += GHR_UPS_WAVE) {
        const int j = base + lane;
        if (j >= L) continue;
        float Pl[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < GHR_UPS_K; k++) {
            if (k >= K) continue;
            const float p[3] = {row[k][3 * j], row[k][3 * j + 1], row[k][3 * j + 2]};
            float r[3];
            ups_local(M[k], p, row[k], r);
#pragma unroll
            for (int x = 0; x < 3; x++) Pl[x] = k == 0 ? w[0] * r[x] : Pl[x] + w[k] * r[x];
        }
        float pt[3];
        ups_world(o, cM, Pl, pt);
        if (j == 0) { pt[0] = o[0]; pt[1] = o[1]; pt[2] = o[2]; }
        out[3 * j] = pt[0]; out[3 * j + 1] = pt[1]; out[3 * j + 2] = pt[2];
    }
    for (int f = lane; f < F; f += GHR_UPS_WAVE) {
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < GHR_UPS_K; k++) {
            if (k >= K) continue;
            const float x = a.gf[(size_t)e4[k] * F + f];
            v = k == 0 ? w[0] * x : v + w[k] * x;
        }
        a.of[c * (size_t)F + f] = v;
    }
    if (lane < GHR_UPS_K) a.w[GHR_UPS_K * c + lane] = lane == 0 ? w[0] : lane == 1 ? w[1] : lane == 2 ? w[2] : w[3];
    if (lane == 0) a.valid[c] = 1;
}

#endif  // __HIPCC__

}  // namespace ghr
