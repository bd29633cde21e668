// ghr_knn.h -- exact mean squared distance to the 3 nearest neighbours of every point (simple_knn's distCUDA2, which the
// reference calls once per model in create_from_pcd, src/scene/gaussian_model.py:409).
//
// Contract (gaussianhaircut_amd/simple_knn/_C.py states it for the callers): for query i and every j != i (by index:
// a duplicate point is a neighbour at distance 0), d = (dx*dx + dy*dy) + dz*dz with dx = p_j.x - q_i.x, in fp32 without
// contraction.  Three slots b0 <= b1 <= b2 start at FLT_MAX and take d only when d < b2, so d >= FLT_MAX (inf from
// overflow included) never enters; out[i] = ((b0 + b1) + b2) / 3.  The three smallest values of a set do not depend on
// the order they are met in, so the result is the same bits for any launch schedule and any input permutation.
//
// Pipeline (ghr_knn_keys, torch.sort on the host side, ghr_knn_mean_dist2):
//   k_knn_keys    63-bit Morton code (21 bits per axis) over the cloud's bounds.  Keys only decide which points share a
//                 block, i.e. the speed; a NaN or an overflowed coordinate is clamped into range, never used as an index.
//   k_knn_boxes   gathers the points in key order into float4 (x, y, z, original index as bits) and writes the AABB of
//                 every block of 64 sorted points and of every superblock of 64 blocks (4096 points).
//   k_knn_search  one wave per block of 64 sorted queries, one query per lane: the own block first (the query itself
//                 skipped by sorted position), then every superblock whose box some lane still needs, and inside it every
//                 block whose box some lane needs (wave ballots), each such block loaded once as 64 coalesced float4 into
//                 LDS and scanned by all lanes.  A lane whose own box test failed scans it too: its d >= boxdist >= b2
//                 cannot enter, so the extra work changes nothing.  Every block is scanned at most once per wave.
//
// Pruning is exact: a box is skipped when boxdist >= b2, and boxdist is a true lower bound of the fp32 d of every point
// in the box (knn_box_dist), so no skipped point could have entered a slot.  `>=` (not `>`) matters: with exact
// duplicates b2 drops to 0 and every other box is then skipped instead of scanned.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cstdint>

namespace ghr {

#define GHR_KNN_BLOCK 64      // sorted points per block (one wave of queries)
#define GHR_KNN_SUPER 64      // blocks per superblock
#define GHR_KNN_WAVES 4       // waves per workgroup of k_knn_search / k_knn_boxes
#define GHR_KNN_MORTON_MAX 2097151.0f  // 2^21 - 1

// 21 low bits of v spread to every third bit
__device__ __forceinline__ unsigned long long knn_spread3(unsigned long long v)
{
    v &= 0x1fffffull;
    v = (v | v << 32) & 0x1f00000000ffffull;
    v = (v | v << 16) & 0x1f0000ff0000ffull;
    v = (v | v << 8) & 0x100f00f00f00f00full;
    v = (v | v << 4) & 0x10c30c30c30c30c3ull;
    v = (v | v << 2) & 0x1249249249249249ull;
    return v;
}

// quantised coordinate in [0, 2^21 - 1]; NaN (a NaN point, or inf - inf) lands on 0
__device__ __forceinline__ unsigned long long knn_quant(float p, float lo, float scale)
{
    const float t = (p - lo) * scale;
    const float c = t >= 0.f ? fminf(t, GHR_KNN_MORTON_MAX) : 0.f;
    return (unsigned long long)(unsigned)c;
}

// bounds: min x, y, z, max x, y, z (device; torch.aminmax of the points).  keys: [P] 63-bit Morton codes (as int64).
__global__ void __launch_bounds__(256) k_knn_keys(int P, const float* __restrict__ pts, const float* __restrict__ bounds,
                                                   unsigned long long* __restrict__ keys)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;  // 64-bit: P may be close to 2^31
    if (i >= P) return;
    float lo[3], scale[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = bounds[a];
        const float ext = bounds[3 + a] - bounds[a];
        // a flat axis, an overflowed extent or NaN bounds: the axis contributes 0 to every key
        scale[a] = (ext > 0.f && ext <= FLT_MAX) ? GHR_KNN_MORTON_MAX / ext : 0.f;
    }
    const size_t b = (size_t)i * 3;
    keys[i] = knn_spread3(knn_quant(pts[b], lo[0], scale[0])) << 2 | knn_spread3(knn_quant(pts[b + 1], lo[1], scale[1])) << 1 |
              knn_spread3(knn_quant(pts[b + 2], lo[2], scale[2]));
}

__device__ __forceinline__ float knn_wave_min(float v)
{
    for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ float knn_wave_max(float v)
{
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}

// One workgroup per superblock, each wave every GHR_KNN_WAVES-th block of it.  order: [P] int64 from the key sort; an
// entry outside [0, P) (only a caller's bad permutation can hold one) is read as 0, so no access leaves the buffers.
// sorted: [P] float4; bbox: [nblocks][2] float4 (min, max); sbox: [nsuper][2] float4.
__global__ void __launch_bounds__(64 * GHR_KNN_WAVES) k_knn_boxes(int P, const float* __restrict__ pts,
                                                                   const long long* __restrict__ order,
                                                                   float4* __restrict__ sorted, float4* __restrict__ bbox,
                                                                   float4* __restrict__ sbox)
{
    __shared__ float red[GHR_KNN_WAVES][6];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nblocks = (int)(((long long)P + GHR_KNN_BLOCK - 1) / GHR_KNN_BLOCK);
    const int sb = blockIdx.x;
    const int b_end = min(nblocks, (sb + 1) * GHR_KNN_SUPER);
    float smin[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, smax[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int blk = sb * GHR_KNN_SUPER + wave; blk < b_end; blk += GHR_KNN_WAVES) {
        const long long i = (long long)blk * GHR_KNN_BLOCK + lane;
        float c[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, C[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
        if (i < P) {
            long long o = order[i];
            if (o < 0 || o >= P) o = 0;
            const size_t b = (size_t)o * 3;
            const float x = pts[b], y = pts[b + 1], z = pts[b + 2];
            sorted[i] = make_float4(x, y, z, __int_as_float((int)o));
            c[0] = C[0] = x; c[1] = C[1] = y; c[2] = C[2] = z;
        }
        for (int a = 0; a < 3; ++a) {
            c[a] = knn_wave_min(c[a]);
            C[a] = knn_wave_max(C[a]);
            smin[a] = fminf(smin[a], c[a]);
            smax[a] = fmaxf(smax[a], C[a]);
        }
        if (lane == 0) {
            bbox[2 * (size_t)blk] = make_float4(c[0], c[1], c[2], 0.f);
            bbox[2 * (size_t)blk + 1] = make_float4(C[0], C[1], C[2], 0.f);
        }
    }
    if (lane == 0)
        for (int a = 0; a < 3; ++a) red[wave][a] = smin[a], red[wave][3 + a] = smax[a];
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < GHR_KNN_WAVES; ++w)
            for (int a = 0; a < 3; ++a) {
                red[0][a] = fminf(red[0][a], red[w][a]);
                red[0][3 + a] = fmaxf(red[0][3 + a], red[w][3 + a]);
            }
        sbox[2 * (size_t)sb] = make_float4(red[0][0], red[0][1], red[0][2], 0.f);
        sbox[2 * (size_t)sb + 1] = make_float4(red[0][3], red[0][4], red[0][5], 0.f);
    }
}

// Lower bound of the fp32 distance d (above) from q to any point c inside [lo, hi].  Along x: when q.x < lo.x, every
// c.x >= lo.x, and fp32 subtraction is monotone under round-to-nearest, so fl(c.x - q.x) >= fl(lo.x - q.x) = gx >= 0;
// when q.x > hi.x, |fl(c.x - q.x)| = fl(q.x - c.x) >= fl(q.x - hi.x) = gx (subtraction is exactly sign-symmetric);
// otherwise gx = 0.  Squaring non-negative values and adding them are monotone too, so computing the bound in the same
// order as d, (gx*gx + gy*gy) + gz*gz, gives boxdist <= d for every point of the box, overflow to inf included.
__device__ __forceinline__ float knn_box_dist(float3 q, float4 lo, float4 hi)
{
    const float gx = fmaxf(fmaxf(lo.x - q.x, q.x - hi.x), 0.f);
    const float gy = fmaxf(fmaxf(lo.y - q.y, q.y - hi.y), 0.f);
    const float gz = fmaxf(fmaxf(lo.z - q.z, q.z - hi.z), 0.f);
    return (gx * gx + gy * gy) + gz * gz;
}

// the three smallest d met so far; d enters only when d < b2 (NaN and d >= FLT_MAX never do)
__device__ __forceinline__ void knn_insert(float d, float& b0, float& b1, float& b2)
{
    if (d < b2) {
        b2 = fmaxf(b1, d);
        b1 = fmaxf(b0, fminf(b1, d));
        b0 = fminf(b0, d);
    }
}

__device__ __forceinline__ void knn_wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Scans n (<= 64) points of the block staged in `tile`, skipping tile position `skip` (-1: none).
__device__ __forceinline__ void knn_scan_tile(const float4* tile, int n, int skip, float3 q, float& b0, float& b1,
                                              float& b2)
{
    for (int j = 0; j < n; ++j) {
        const float4 c = tile[j];  // the same address in every lane: an LDS broadcast
        const float dx = c.x - q.x, dy = c.y - q.y, dz = c.z - q.z;
        const float d = (dx * dx + dy * dy) + dz * dz;
        if (j != skip) knn_insert(d, b0, b1, b2);
    }
}

// Each wave works on its own: its LDS tile is private and only wave-level fences order the tile's reuse.
__global__ void __launch_bounds__(64 * GHR_KNN_WAVES) k_knn_search(int P, const float4* __restrict__ sorted,
                                                                    const float4* __restrict__ bbox,
                                                                    const float4* __restrict__ sbox,
                                                                    float* __restrict__ out)
{
    __shared__ float4 tiles[GHR_KNN_WAVES][GHR_KNN_BLOCK];
    // readfirstlane: the compiler then knows every block / superblock index below is wave-uniform (scalar box loads,
    // scalar loop control)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float4* tile = tiles[wave];
    const int nblocks = (int)(((long long)P + GHR_KNN_BLOCK - 1) / GHR_KNN_BLOCK);
    const int nsuper = (nblocks + GHR_KNN_SUPER - 1) / GHR_KNN_SUPER;
    const int qb = blockIdx.x * GHR_KNN_WAVES + wave;
    if (qb >= nblocks) return;
    const long long qi = (long long)qb * GHR_KNN_BLOCK + lane;
    const bool valid = qi < P;
    const int nq = min(GHR_KNN_BLOCK, P - qb * GHR_KNN_BLOCK);
    const float4 q4 = sorted[valid ? qi : qb * GHR_KNN_BLOCK];
    const float3 q = make_float3(q4.x, q4.y, q4.z);
    float b0 = FLT_MAX, b1 = FLT_MAX, b2 = FLT_MAX;

    // own block: after it b2 is a real distance unless the block holds fewer than 4 points
    tile[lane] = q4;
    knn_wave_lds_fence();
    knn_scan_tile(tile, nq, lane, q, b0, b1, b2);

    const int own_sb = qb / GHR_KNN_SUPER;
    for (int s = 0; s < nsuper; ++s) {
        const int sb = own_sb + s < nsuper ? own_sb + s : own_sb + s - nsuper;  // own superblock first
        if (!__any(valid && knn_box_dist(q, sbox[2 * sb], sbox[2 * sb + 1]) < b2)) continue;
        const int b_end = min(nblocks, (sb + 1) * GHR_KNN_SUPER);
        for (int blk = sb * GHR_KNN_SUPER; blk < b_end; ++blk) {
            if (blk == qb) continue;  // scanned above
            if (!__any(valid && knn_box_dist(q, bbox[2 * blk], bbox[2 * blk + 1]) < b2)) continue;
            const int n = min(GHR_KNN_BLOCK, P - blk * GHR_KNN_BLOCK);
            knn_wave_lds_fence();  // every lane is done reading the previous tile
            if (lane < n) tile[lane] = sorted[(long long)blk * GHR_KNN_BLOCK + lane];
            knn_wave_lds_fence();
            knn_scan_tile(tile, n, -1, q, b0, b1, b2);
        }
    }
    if (valid) out[__float_as_int(q4.w)] = ((b0 + b1) + b2) / 3.0f;
}

}  // namespace ghr
