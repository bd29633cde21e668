// ghr_knn.h -- the key-ordered point cloud, the pruned block walk over it (ghr_nn.h's too) and on them the exact mean squared
// distance to the 3 nearest neighbours of every point (simple_knn's distCUDA2: create_from_pcd, src/scene/gaussian_model.py:409).
//
// Contract of distCUDA2 (gaussianhaircut_amd/simple_knn/_C.py states it for the callers): for query i and every j != i (by
// index: a duplicate point is a neighbour at distance 0), d = (dx*dx + dy*dy) + dz*dz with dx = p_j.x - q_i.x, in fp32 without
// contraction.  Three slots b0 <= b1 <= b2 start at FLT_MAX and take d only when d < b2, so d >= FLT_MAX (inf from
// overflow included) never enters; out[i] = ((b0 + b1) + b2) / 3.  The three smallest values of a set do not depend on
// the order they are met in, so the result is the same bits for any launch schedule and any input permutation.
//
// The cloud (knn_layout, knn_cloud; ghr_knn_keys, a key sort on the host side, k_knn_boxes):
//   k_knn_keys    63-bit Morton code (21 bits per axis) over given bounds (knn_key).  Keys only decide which points share a
//                 block, i.e. the speed; a NaN or an overflowed coordinate is clamped into range, never used as an index.
//   k_knn_boxes   gathers the points in key order into float4 (x, y, z, original index as bits) and writes the AABB of
//                 every block of 64 sorted points and of every superblock of 64 blocks (4096 points).
// The walk (knn_walk): one wave per block of 64 queries, one query per lane.  A first block is staged in the wave's private
// LDS tile and scanned; then the superblocks in rotation from the first block's on and inside each its blocks: one whose box
// no lane still needs is skipped by a wave ballot, a needed block is loaded once as 64 coalesced float4 into the tile and
// scanned by all lanes, at most once per wave.  A lane's state, the lower bound of a box and whether the lane still needs a
// box at that bound are a policy object's; the walk does not know its caller.  A lane whose own box test failed scans the
// block too: `needs` is exact, so nothing of that block can enter its state.
//   k_knn_search  the walk from the wave's OWN block, the query skipped by its tile position, with KnnTop3: a box is skipped
//                 when boxdist >= b2, a true lower bound of the fp32 d of every point in it (knn_box_dist).  `>=` (not `>`)
//                 matters: with exact duplicates b2 drops to 0 and every other box is then skipped instead of scanned.
// Per-element functions are GHR_HD and the header is plain C++ outside __HIPCC__: tests/hostsim/ghr_hostsim_knn.cpp walks them.
#pragma once
#if defined(__HIPCC__)
#include "ghr_device.h"
#else
#include <stdint.h>
#define GHR_HD inline
#endif
#include <float.h>
#include <math.h>
#include <string.h>

#define GHR_KNN_BLOCK 64      // sorted points per block (one wave of queries)
#define GHR_KNN_SUPER 64      // blocks per superblock
#define GHR_KNN_WAVES 4       // waves per workgroup of k_knn_search / k_knn_boxes
#define GHR_KNN_MORTON_MAX 2097151.0f  // 2^21 - 1
#define GHR_KNN_ALIGN 256     // of a cloud's three regions (the C API's workspace alignment)

namespace ghr {

#if !defined(__HIPCC__)
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };
#endif

GHR_HD int knn_as_int(float f) { int i; memcpy(&i, &f, 4); return i; }
GHR_HD float knn_as_float(int i) { float f; memcpy(&f, &i, 4); return f; }

// The cloud: sorted float4 points, then a (min, max) float4 pair per block, then a pair per superblock; offsets in bytes from a
// base aligned to GHR_KNN_ALIGN.  P in [0, 2^31).
struct KnnLayout { uint64_t nblocks, nsuper, off_sorted, off_bbox, off_sbox, bytes; };
inline uint64_t knn_up(uint64_t x) { return (x + GHR_KNN_ALIGN - 1) / GHR_KNN_ALIGN * GHR_KNN_ALIGN; }
inline KnnLayout knn_layout(uint64_t P)
{
    const uint64_t nb = (P + GHR_KNN_BLOCK - 1) / GHR_KNN_BLOCK, ns = (nb + GHR_KNN_SUPER - 1) / GHR_KNN_SUPER;
    const uint64_t off_bbox = knn_up(P * sizeof(float4)), off_sbox = off_bbox + knn_up(nb * 2 * sizeof(float4));
    return KnnLayout{nb, ns, 0, off_bbox, off_sbox, off_sbox + knn_up(ns * 2 * sizeof(float4))};
}
// sorted [P]: x, y, z, original index as bits; bbox [nblocks][2], sbox [nsuper][2]: (min, max)
struct KnnCloud { int P, nblocks, nsuper; float4 *sorted, *bbox, *sbox; };
inline KnnCloud knn_cloud(char* base, uint64_t P)
{
    const KnnLayout L = knn_layout(P);
    return KnnCloud{(int)P, (int)L.nblocks, (int)L.nsuper, (float4*)(base + L.off_sorted), (float4*)(base + L.off_bbox),
                    (float4*)(base + L.off_sbox)};
}

// 21 low bits of v spread to every third bit
GHR_HD unsigned long long knn_spread3(unsigned long long v)
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
GHR_HD unsigned long long knn_quant(float p, float lo, float scale)
{
    const float t = (p - lo) * scale;
    const float c = t >= 0.f ? fminf(t, GHR_KNN_MORTON_MAX) : 0.f;
    return (unsigned long long)(unsigned)c;
}

// The key of point p[3].  bounds: min x, y, z, max x, y, z.
GHR_HD unsigned long long knn_key(const float* p, const float* bounds)
{
    unsigned long long q[3];
    for (int a = 0; a < 3; ++a) {
        const float ext = bounds[3 + a] - bounds[a];
        // a flat axis, an overflowed extent or NaN bounds: the axis contributes 0 to every key
        const float scale = (ext > 0.f && ext <= FLT_MAX) ? GHR_KNN_MORTON_MAX / ext : 0.f;
        q[a] = knn_spread3(knn_quant(p[a], bounds[a], scale));
    }
    return q[0] << 2 | q[1] << 1 | q[2];
}

// Lower bound of the fp32 distance d (above) from q to any point c inside [lo, hi].  Along x: when q.x < lo.x, every
// c.x >= lo.x, and fp32 subtraction is monotone under round-to-nearest, so fl(c.x - q.x) >= fl(lo.x - q.x) = gx >= 0;
// when q.x > hi.x, |fl(c.x - q.x)| = fl(q.x - c.x) >= fl(q.x - hi.x) = gx (subtraction is exactly sign-symmetric);
// otherwise gx = 0.  Squaring non-negative values and adding them are monotone too, so computing the bound in the same
// order as d, (gx*gx + gy*gy) + gz*gz, gives boxdist <= d for every point of the box, overflow to inf included.
GHR_HD float knn_box_dist(float3 q, float4 lo, float4 hi)
{
    const float gx = fmaxf(fmaxf(lo.x - q.x, q.x - hi.x), 0.f);
    const float gy = fmaxf(fmaxf(lo.y - q.y, q.y - hi.y), 0.f);
    const float gz = fmaxf(fmaxf(lo.z - q.z, q.z - hi.z), 0.f);
    return (gx * gx + gy * gy) + gz * gz;
}

GHR_HD float knn_dist2(const float4& c, const float3& q)  // (by reference: by value costs the scan loop an s_nop)
{
    const float dx = c.x - q.x, dy = c.y - q.y, dz = c.z - q.z;
    return (dx * dx + dy * dy) + dz * dz;
}

// the three smallest d met so far; d enters only when d < b2 (NaN and d >= FLT_MAX never do)
GHR_HD void knn_insert(float d, float& b0, float& b1, float& b2)
{
    if (d < b2) {
        b2 = fmaxf(b1, d);
        b1 = fmaxf(b0, fminf(b1, d));
        b0 = fminf(b0, d);
    }
}

// A policy is one lane's state with bound(q, lo, hi), a lower bound of the lane's d over a box; needs(bound), whether a point
// at that bound could still change the state; scan(tile, n, skip, q), n (<= 64) staged points, tile position `skip` (or -1) left out.
struct KnnTop3 {
    float b0 = FLT_MAX, b1 = FLT_MAX, b2 = FLT_MAX;
    GHR_HD float bound(float3 q, float4 lo, float4 hi) const { return knn_box_dist(q, lo, hi); }
    GHR_HD bool needs(float boxdist) const { return boxdist < b2; }
    GHR_HD void scan(const float4* tile, int n, int skip, float3 q)
    {
        for (int j = 0; j < n; ++j) {
            const float d = knn_dist2(tile[j], q);  // the same address in every lane: an LDS broadcast
            if (j != skip) knn_insert(d, b0, b1, b2);
        }
    }
    GHR_HD float mean() const { return ((b0 + b1) + b2) / 3.0f; }
};

// A policy may also have stage(blk, n, lane): the lane's share of staging something of its own beside block blk's n points,
// between the walk's two fences (ghr_field.h's payload tile).  A policy without one costs nothing.
template <class Policy>
GHR_HD auto knn_stage(Policy& pol, int blk, int n, int lane, int) -> decltype(pol.stage(blk, n, lane), void()) { pol.stage(blk, n, lane); }
template <class Policy>
GHR_HD void knn_stage(Policy&, int, int, int, long) {}

#if defined(__HIPCC__)
#ifdef GHR_NN_COUNT_BLOCKS
// measurement build only (tools/build_variant.sh -DGHR_NN_COUNT_BLOCKS): [0] blocks scanned by knn_walk, [1] waves
__device__ unsigned long long g_nn_count[2];
#define GHR_KNN_COUNTING(code) code
#else
#define GHR_KNN_COUNTING(code)
#endif

// bounds: device, e.g. torch.aminmax of the points.  keys: [P] 63-bit Morton codes (as int64).
__global__ void __launch_bounds__(256) k_knn_keys(int P, const float* __restrict__ pts, const float* __restrict__ bounds,
                                                   unsigned long long* __restrict__ keys)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;  // 64-bit: P may be close to 2^31
    if (i >= P) return;
    keys[i] = knn_key(pts + (size_t)i * 3, bounds);
}

__device__ __forceinline__ void knn_wave_min_max(float& lo, float& hi)
{
    for (int m = 32; m >= 1; m >>= 1) lo = fminf(lo, __shfl_xor(lo, m)), hi = fmaxf(hi, __shfl_xor(hi, m));
}

// One workgroup per superblock, each wave every GHR_KNN_WAVES-th block of it.  order: [P] int64 from the key sort; an
// entry outside [0, P) (only a caller's bad permutation can hold one) is read as 0, so no access leaves the buffers.
__global__ void __launch_bounds__(64 * GHR_KNN_WAVES) k_knn_boxes(KnnCloud c, const float* __restrict__ pts,
                                                                   const long long* __restrict__ order)
{
    __shared__ float red[GHR_KNN_WAVES][6];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int P = c.P, sb = blockIdx.x;
    const int b_end = min(c.nblocks, (sb + 1) * GHR_KNN_SUPER);
    float smin[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, smax[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int blk = sb * GHR_KNN_SUPER + wave; blk < b_end; blk += GHR_KNN_WAVES) {
        const long long i = (long long)blk * GHR_KNN_BLOCK + lane;
        float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
        if (i < P) {
            long long o = order[i];
            if (o < 0 || o >= P) o = 0;
            const size_t b = (size_t)o * 3;
            const float x = pts[b], y = pts[b + 1], z = pts[b + 2];
            c.sorted[i] = make_float4(x, y, z, knn_as_float((int)o));
            lo[0] = hi[0] = x; lo[1] = hi[1] = y; lo[2] = hi[2] = z;
        }
        for (int a = 0; a < 3; ++a) {
            knn_wave_min_max(lo[a], hi[a]);
            smin[a] = fminf(smin[a], lo[a]);
            smax[a] = fmaxf(smax[a], hi[a]);
        }
        if (lane == 0) {
            c.bbox[2 * (size_t)blk] = make_float4(lo[0], lo[1], lo[2], 0.f);
            c.bbox[2 * (size_t)blk + 1] = make_float4(hi[0], hi[1], hi[2], 0.f);
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
        c.sbox[2 * (size_t)sb] = make_float4(red[0][0], red[0][1], red[0][2], 0.f);
        c.sbox[2 * (size_t)sb + 1] = make_float4(red[0][3], red[0][4], red[0][5], 0.f);
    }
}

__device__ __forceinline__ void knn_wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The walk of candidate cloud `c` by one wave (every lane makes the call): `tile` is the wave's private GHR_KNN_BLOCK float4 of
// LDS, q the lane's query, `valid` whether the lane has one (an invalid lane votes in no ballot), `first` the wave-uniform
// block scanned first, with tile position `skip` left out of that scan (-1: none), pol the lane's state.  Each wave works on
// its own: only wave-level fences order the tile's reuse.
template <class Policy>
__device__ __forceinline__ void knn_walk(const KnnCloud& c, float4* tile, float3 q, bool valid, int first, int skip, Policy& pol)
{
    const int lane = threadIdx.x & 63;
    GHR_KNN_COUNTING(unsigned scanned = 0;)
    auto scan_block = [&](int blk, int skip_pos) {
        const int n = min(GHR_KNN_BLOCK, c.P - blk * GHR_KNN_BLOCK);
        knn_wave_lds_fence();  // every lane is done reading the previous tile
        if (lane < n) tile[lane] = c.sorted[(long long)blk * GHR_KNN_BLOCK + lane];
        knn_stage(pol, blk, n, lane, 0);
        knn_wave_lds_fence();
        pol.scan(tile, n, skip_pos, q);
        GHR_KNN_COUNTING(++scanned;)
    };
    scan_block(first, skip);  // after it a lane's bound is a real distance (distCUDA2: unless the block has fewer than 4 points)
    const int first_sb = first / GHR_KNN_SUPER;
    for (int s = 0; s < c.nsuper; ++s) {
        const int sb = first_sb + s < c.nsuper ? first_sb + s : first_sb + s - c.nsuper;  // the first block's superblock first
        if (!__any(valid && pol.needs(pol.bound(q, c.sbox[2 * sb], c.sbox[2 * sb + 1])))) continue;
        const int b_end = min(c.nblocks, (sb + 1) * GHR_KNN_SUPER);
        for (int blk = sb * GHR_KNN_SUPER; blk < b_end; ++blk) {
            if (blk == first) continue;  // scanned above
            if (!__any(valid && pol.needs(pol.bound(q, c.bbox[2 * blk], c.bbox[2 * blk + 1])))) continue;  // (32-bit index: 8j)
            scan_block(blk, -1);
        }
    }
    GHR_KNN_COUNTING(if (lane == 0) { atomicAdd(&g_nn_count[0], (unsigned long long)scanned); atomicAdd(&g_nn_count[1], 1ull); })
}

// out: [P], written at the queries' original indices.
__global__ void __launch_bounds__(64 * GHR_KNN_WAVES) k_knn_search(KnnCloud c, float* __restrict__ out)
{
    __shared__ float4 tiles[GHR_KNN_WAVES][GHR_KNN_BLOCK];
    // readfirstlane: the compiler then knows every block / superblock index below is wave-uniform (scalar box loads,
    // scalar loop control)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int qb = blockIdx.x * GHR_KNN_WAVES + wave;
    if (qb >= c.nblocks) return;
    const long long qi = (long long)qb * GHR_KNN_BLOCK + lane;
    const bool valid = qi < c.P;
    const float4 q4 = c.sorted[valid ? qi : qb * GHR_KNN_BLOCK];
    KnnTop3 top;
    knn_walk(c, tiles[wave], make_float3(q4.x, q4.y, q4.z), valid, qb, lane, top);  // own block first, the query itself skipped
    if (valid) out[knn_as_int(q4.w)] = top.mean();
}
#endif  // __HIPCC__

}  // namespace ghr
