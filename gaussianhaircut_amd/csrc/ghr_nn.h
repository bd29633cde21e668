// ghr_nn.h -- exact nearest neighbour of every point of one cloud among the points of another (K = 1, the index returned),
// the per-point terms of a chamfer distance around it and their gather-form backward (what the reference's
// src/utils/loss_chamfer_utils.py takes from pytorch3d's knn_points / knn_gather).
//
// Contract (gaussianhaircut_amd/nearest.py states it for the callers): for query x_i and every candidate y_j, j < Py,
//   norm = 2:  d = (dx*dx + dy*dy) + dz*dz      (the SQUARED distance, as pytorch3d returns it)
//   norm = 1:  d = (|dx| + |dy|) + |dz|
// with dx = y_j.x - x_i.x, in fp32 without contraction.  The winner is the smallest d and, among equal d, the lowest ORIGINAL
// index j: a total order when no d is NaN, so dist[i] and idx[i] are the same bits for any launch schedule and any permutation
// of either input (permuting y renames the indices; on ties the lowest original one still wins).  idx is always in [0, Py).
// Non-finite coordinates are the caller's responsibility (as in ghr_knn.h): the result is then unspecified, but a candidate
// index never comes from arithmetic on coordinates, so no access leaves the buffers.  Py == 0 is refused by the C entry.
//
// Pipeline (ghr_knn_keys on both clouds with the bounds of their UNION -- equal keys then mean equal places --, a key sort of
// each on the host side, ghr_nn_search):
//   k_knn_boxes   (ghr_knn.h) once per cloud: points in key order as float4 (x, y, z, original index as bits) and the boxes of
//                 every block of 64 and every superblock of 64 blocks; of x only the sorted points are used.
//   k_nn_search   one wave per block of 64 queries in the key order of x, one query per lane, around knn_walk (ghr_knn.h) over
//                 y's cloud.  Its own are the walk's first block and the policy NnNearest<NORM>:
//     seed        there is no own block, and without a first bound every box passes.  The first block is the y block at which
//                 the key of the wave's median query would be inserted into y's sorted keys (nn_seed_block: wave-uniform
//                 values, i.e. scalar code), nothing skipped in it.  The seed decides speed only: the winner under the
//                 total order above does not depend on the order candidates are met in.
//     pruning     a lane needs a box unless boxdist > best, NOT >=: a box at exactly the best distance may hold a lower index
//                 that ties.  boxdist (knn_box_dist, nn_box_dist_l1) is a true lower bound of the fp32 d of every point in
//                 the box, so a skipped point can neither win nor tie.  The price: with exact duplicates (best = 0) every
//                 box that CONTAINS the query is scanned, where distCUDA2's >= would skip them.
//   k_chamfer_point   one thread per query, a kernel of its own (the search keeps its registers for the walk, and many callers
//                 want no normals): term[i] = 1 - cos or 1 - |cos|, cos = (a . b) / (max(|a|, eps) max(|b|, eps)), eps = 1e-6,
//                 a = x_normals[i], b = y_normals[idx[i]] (the formula torch documents for F.cosine_similarity); and
//                 weight[i] = y_weights[idx[i]].
//   backward      gather-form, no floating-point atomics.  x side (k_chamfer_bwd_x), one thread per query:
//                 d_x[i] = -(t + t), t = g_i (y_idx - x_i) for norm 2 -- 2 g_i (x_i - y_idx), written the way autograd
//                 evaluates it so that the bits agree --, -(g_i sign(y_idx - x_i)) for norm 1, and d_x_normals[i] from the
//                 cosine term.  y side (k_chamfer_bwd_y), one thread per candidate: the caller gives the inverted lists
//                 (start [Py + 1], members in ASCENDING i: a stable sort of idx, integers only); the thread walks its list
//                 with one fp32 accumulator per component, the first product assigned, later ones added.  A candidate nobody
//                 chose gets +0.  The same bits run after run.  (Kernels under __HIPCC__; the rest is GHR_HD for the host walk.)
#pragma once
#include "ghr_knn.h"

#define GHR_NN_WAVES 4        // waves per workgroup of k_nn_search
#define GHR_NN_BLOCK 256      // threads per workgroup of the per-point kernels
#define GHR_NN_COS_EPS 1e-6f

namespace ghr {

// The L1 sibling of knn_box_dist: a lower bound of d = (|dx| + |dy|) + |dz| from q to any point c inside [lo, hi].  Along x,
// as there: q.x < lo.x gives fl(c.x - q.x) >= fl(lo.x - q.x) = gx >= 0 (fp32 subtraction is monotone under round-to-nearest),
// q.x > hi.x gives |fl(c.x - q.x)| = fl(q.x - c.x) >= fl(q.x - hi.x) = gx, otherwise gx = 0; so |dx| >= gx, and likewise y, z.
// Adding non-negative values is monotone in each operand, and the bound adds in d's order, so boxdist <= d, inf included.
GHR_HD float nn_box_dist_l1(float3 q, float4 lo, float4 hi)
{
    const float gx = fmaxf(fmaxf(lo.x - q.x, q.x - hi.x), 0.f);
    const float gy = fmaxf(fmaxf(lo.y - q.y, q.y - hi.y), 0.f);
    const float gz = fmaxf(fmaxf(lo.z - q.z, q.z - hi.z), 0.f);
    return (gx + gy) + gz;
}

template <int NORM>
GHR_HD float nn_dist(const float4& c, const float3& q)
{
    return NORM == 2 ? knn_dist2(c, q) : (fabsf(c.x - q.x) + fabsf(c.y - q.y)) + fabsf(c.z - q.z);
}

// (d, original index) ascending; a NaN d never enters
GHR_HD void nn_take(float d, int cj, float& best, int& besti)
{
    if (d < best || (d == best && cj < besti)) {
        best = d;
        besti = cj;
    }
}

// knn_walk's policy (see KnnTop3): the nearest candidate and, among equal d, the lowest original index.
template <int NORM>
struct NnNearest {
    // +inf, not FLT_MAX: a d that overflowed still has to find its lowest index; INT_MAX loses every index tie
    float best = __builtin_inff();
    int besti = 0x7fffffff;
    GHR_HD float bound(float3 q, float4 lo, float4 hi) const { return NORM == 2 ? knn_box_dist(q, lo, hi) : nn_box_dist_l1(q, lo, hi); }
    GHR_HD bool needs(float boxdist) const { return !(boxdist > best); }
    GHR_HD void scan(const float4* tile, int n, int skip, float3 q)
    {
        float b = best;
        int bi = besti;
        for (int j = 0; j < n; ++j) {
            const float4 c = tile[j];  // the same address in every lane: an LDS broadcast
            const float d = nn_dist<NORM>(c, q);
            if (j != skip) nn_take(d, knn_as_int(c.w), b, bi);
        }
        best = b;
        besti = bi;
    }
    GHR_HD int index(int Py) const { return (unsigned)besti < (unsigned)Py ? besti : 0; }  // (every d NaN: nothing entered)
};

// The block of sorted keys [P] at which key kq would be inserted (lower bound), P >= 1.
GHR_HD int nn_seed_block(const unsigned long long* keys, int P, unsigned long long kq)
{
    int lo = 0, hi = P;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < kq) lo = mid + 1; else hi = mid;
    }
    return (lo < P - 1 ? lo : P - 1) / GHR_KNN_BLOCK;
}

#if defined(__HIPCC__)
// x / y: the clouds in key order (k_knn_boxes; of x only the sorted points are read); keys_x / keys_y: their SORTED keys.
// dist / idx: [Px], written at the queries' original indices.
template <int NORM>
__global__ void __launch_bounds__(64 * GHR_NN_WAVES) k_nn_search(KnnCloud x, const unsigned long long* __restrict__ keys_x,
                                                                  KnnCloud y, const unsigned long long* __restrict__ keys_y,
                                                                  float* __restrict__ dist, int* __restrict__ idx)
{
    __shared__ float4 tiles[GHR_NN_WAVES][GHR_KNN_BLOCK];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long qb = (long long)blockIdx.x * GHR_NN_WAVES + wave;
    if (qb >= x.nblocks) return;
    const long long q0 = qb * GHR_KNN_BLOCK;
    const bool valid = q0 + lane < x.P;
    const int nq = (int)min((long long)GHR_KNN_BLOCK, x.P - q0);
    const float4 q4 = x.sorted[valid ? q0 + lane : q0];
    const int seed = nn_seed_block(keys_y, y.P, keys_x[q0 + nq / 2]);
    NnNearest<NORM> near;
    knn_walk(y, tiles[wave], make_float3(q4.x, q4.y, q4.z), valid, seed, -1, near);
    if (valid) {
        const int o = knn_as_int(q4.w);  // in [0, Px): k_knn_boxes clamps the caller's permutation
        dist[o] = near.best;
        idx[o] = near.index(y.P);
    }
}

// ---- the per-point terms -----------------------------------------------------------------------------------------------
__device__ __forceinline__ float nn_sign(float v) { return (float)((v > 0.f) - (v < 0.f)); }

// cos of the contract; na / nb: the norms, nac / nbc: clamped at eps
__device__ __forceinline__ float nn_cos(const float* a, const float* b, float& na, float& nb, float& nac, float& nbc)
{
    const float dot = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
    na = sqrtf((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    nb = sqrtf((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
    nac = fmaxf(na, GHR_NN_COS_EPS);
    nbc = fmaxf(nb, GHR_NN_COS_EPS);
    return dot / (nac * nbc);
}

// gradient of term = 1 - cos (or 1 - |cos|) times g, w.r.t. a (da) and b (db).  d cos / d a = b / (nac nbc) - cos a / |a|^2
// where |a| > eps (the clamp passes the norm's gradient), b / (nac nbc) below; |cos|' is sign(cos), 0 at 0 as torch.abs has it.
__device__ __forceinline__ void nn_cos_grad(const float* a, const float* b, int abs_cosine, float g, float* da, float* db)
{
    float na, nb, nac, nbc;
    const float c = nn_cos(a, b, na, nb, nac, nbc);
    const float gc = -((abs_cosine ? nn_sign(c) : 1.f) * g);
    const float inv = 1.f / (nac * nbc);
    const float ka = na > GHR_NN_COS_EPS ? c / (na * na) : 0.f, kb = nb > GHR_NN_COS_EPS ? c / (nb * nb) : 0.f;
    for (int k = 0; k < 3; ++k) {
        da[k] = gc * (b[k] * inv - ka * a[k]);
        db[k] = gc * (a[k] * inv - kb * b[k]);
    }
}

// idx [Px] int32 (k_nn_search's; an entry outside [0, Py) is read as 0).  x_normals / y_normals: both or neither; term [Px].
// y_weights [Py] and weight [Px]: both or neither.
__global__ void __launch_bounds__(GHR_NN_BLOCK) k_chamfer_point(int Px, int Py, const int* __restrict__ idx,
                                                                 const float* __restrict__ x_normals,
                                                                 const float* __restrict__ y_normals, int abs_cosine,
                                                                 const float* __restrict__ y_weights,
                                                                 float* __restrict__ term, float* __restrict__ weight)
{
    const long long i = (long long)blockIdx.x * GHR_NN_BLOCK + threadIdx.x;
    if (i >= Px) return;
    int j = idx[i];
    if ((unsigned)j >= (unsigned)Py) j = 0;
    if (term) {
        float a[3], b[3], na, nb, nac, nbc;
        for (int k = 0; k < 3; ++k) a[k] = x_normals[(size_t)i * 3 + k], b[k] = y_normals[(size_t)j * 3 + k];
        const float c = nn_cos(a, b, na, nb, nac, nbc);
        term[i] = 1.f - (abs_cosine ? fabsf(c) : c);
    }
    if (weight) weight[i] = y_weights[j];
}

// g_dist [Px] with d_x [Px][3] (both or neither), g_cos [Px] with d_x_normals [Px][3] (both or neither)
template <int NORM>
__global__ void __launch_bounds__(GHR_NN_BLOCK) k_chamfer_bwd_x(int Px, int Py, const float* __restrict__ x,
                                                                 const float* __restrict__ y, const int* __restrict__ idx,
                                                                 const float* __restrict__ g_dist,
                                                                 const float* __restrict__ x_normals,
                                                                 const float* __restrict__ y_normals, int abs_cosine,
                                                                 const float* __restrict__ g_cos, float* __restrict__ d_x,
                                                                 float* __restrict__ d_x_normals)
{
    const long long i = (long long)blockIdx.x * GHR_NN_BLOCK + threadIdx.x;
    if (i >= Px) return;
    int j = idx[i];
    if ((unsigned)j >= (unsigned)Py) j = 0;
    if (d_x) {
        const float g = g_dist[i];
        for (int k = 0; k < 3; ++k) {
            const float diff = y[(size_t)j * 3 + k] - x[(size_t)i * 3 + k];
            const float t = NORM == 2 ? g * diff : g * nn_sign(diff);
            d_x[(size_t)i * 3 + k] = NORM == 2 ? -(t + t) : -t;
        }
    }
    if (d_x_normals) {
        float a[3], b[3], da[3], db[3];
        for (int k = 0; k < 3; ++k) a[k] = x_normals[(size_t)i * 3 + k], b[k] = y_normals[(size_t)j * 3 + k];
        nn_cos_grad(a, b, abs_cosine, g_cos[i], da, db);
        for (int k = 0; k < 3; ++k) d_x_normals[(size_t)i * 3 + k] = da[k];
    }
}

// start [Py + 1], members [Px] (int64): candidate j was chosen by queries members[start[j] .. start[j + 1]), ascending.
// Entries outside their ranges (only a caller's bad lists can hold one) are clamped or skipped: no access leaves the buffers.
template <int NORM>
__global__ void __launch_bounds__(GHR_NN_BLOCK) k_chamfer_bwd_y(int Px, int Py, const float* __restrict__ x,
                                                                 const float* __restrict__ y,
                                                                 const long long* __restrict__ start,
                                                                 const long long* __restrict__ members,
                                                                 const float* __restrict__ g_dist,
                                                                 const float* __restrict__ x_normals,
                                                                 const float* __restrict__ y_normals, int abs_cosine,
                                                                 const float* __restrict__ g_cos, float* __restrict__ d_y,
                                                                 float* __restrict__ d_y_normals)
{
    const long long j = (long long)blockIdx.x * GHR_NN_BLOCK + threadIdx.x;
    if (j >= Py) return;
    const long long s = min(max(start[j], 0ll), (long long)Px), e = min(max(start[j + 1], s), (long long)Px);
    float acc[3] = {0.f, 0.f, 0.f}, accn[3] = {0.f, 0.f, 0.f};
    float yj[3] = {0.f, 0.f, 0.f}, b[3] = {0.f, 0.f, 0.f};
    if (d_y)
        for (int k = 0; k < 3; ++k) yj[k] = y[(size_t)j * 3 + k];
    if (d_y_normals)
        for (int k = 0; k < 3; ++k) b[k] = y_normals[(size_t)j * 3 + k];
    bool first = true;
    for (long long m = s; m < e; ++m) {
        const long long i = members[m];
        if (i < 0 || i >= Px) continue;
        if (d_y) {
            const float g = g_dist[i];
            for (int k = 0; k < 3; ++k) {
                const float diff = yj[k] - x[(size_t)i * 3 + k];
                const float t = NORM == 2 ? g * diff : g * nn_sign(diff);
                const float p = NORM == 2 ? t + t : t;
                acc[k] = first ? p : acc[k] + p;
            }
        }
        if (d_y_normals) {
            float a[3], da[3], db[3];
            for (int k = 0; k < 3; ++k) a[k] = x_normals[(size_t)i * 3 + k];
            nn_cos_grad(a, b, abs_cosine, g_cos[i], da, db);
            for (int k = 0; k < 3; ++k) accn[k] = first ? db[k] : accn[k] + db[k];
        }
        first = false;
    }
    if (d_y)
        for (int k = 0; k < 3; ++k) d_y[(size_t)j * 3 + k] = acc[k];
    if (d_y_normals)
        for (int k = 0; k < 3; ++k) d_y_normals[(size_t)j * 3 + k] = accn[k];
}
#endif  // __HIPCC__

}  // namespace ghr
