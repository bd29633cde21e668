// ghr_meshdist.h -- closest point on and signed distance to a triangle mesh: what the strand collision term and
// the strand split between the stages ask of the head mesh (pysdf's magnitude and trimesh.proximity.closest_point in the
// reference's commented-out src/scene/gaussian_model_strands.py:552-563 and src/preprocessing/export_curves.py:48-101).
//
// The definition (ours, exact).  Everything is float32 without contraction, only + - * /, sqrtf and comparisons;
// dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z, cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x);
// clamp(x, lo, hi) = min(max(x, lo), hi) written as two selects (x > lo ? x : lo, then < hi), so that a NaN lands on lo in every
// implementation.  A face's three vertices are taken SORTED BY VERTEX INDEX as A, B, C: a shared edge is evaluated identically
// from both of its faces (as the canonical edges of ghr_mesh.h).  For a query q and one face, up to four candidates, in order:
//   1. the edges (A,B), (A,C), (B,C), each as (P0,P1):  e = P1 - P0, w = q - P0, ee = dot(e,e), ew = dot(e,w),
//      t = ee > 0 ? clamp(ew / ee, 0, 1) : 0,  c = (t == 1) ? P1 : P0 + t*e,  then c clamped componentwise into
//      [min(P0,P1), max(P0,P1)];
//   2. the interior:  n = cross(B-A, C-A), nn = dot(n,n); accepted iff nn > 0 and dot(cross(C-B, q-B), n),
//      dot(cross(A-C, q-C), n), dot(cross(B-A, q-A), n) are all >= 0;  c = q - (dot(n, q-A) / nn) * n, clamped componentwise
//      into the triangle's box.
//   d = dot(c - q, c - q).  The face's result is the smallest d, among equal d the first candidate in the order above; the
//   mesh's result is the smallest d, among equal d the LOWEST ORIGINAL FACE INDEX.  That is a total order (no d is NaN for a
//   finite query: every c is finite), so dist2, face and point are the same bits for any schedule and any order of the faces.
//   A degenerate face needs no special case: its edges still answer.  A query with a non-finite coordinate gives
//   dist2 = +inf, face = -1, point = q, and indexes nothing.  The sign is HeadMesh.contains' (ghr_mesh.h), applied by the caller.
//
// The clamp is part of the definition and what makes the pruning exact: every candidate lies in its triangle's box, hence in
// the box of its block of 64 faces, and d is knn_dist2's expression -- so knn_box_dist (ghr_knn.h:104-108, the argument carries
// over word for word) is a true lower bound of the fp32 d of every face of the block.  A block is skipped only when
// boxdist > best, never on >=: a block at exactly the best distance may hold a lower face index that ties (as ghr_nn.h).
//
// Tables (ghr_mesh_tris_build, host, deterministic), one blob, offsets 16-B aligned from its start:
//   records [F][12 words]  Ax Ay Az Bx | By Bz Cx Cy | Cz face 0 0, read as three 16-B units; the faces ordered by (63-bit
//                          Morton key of the centre of the triangle's box over the mesh's bounds, face index)
//   bbox [nblocks][2], sbox [nsuper][2]  (min, max) float4 of the vertices of every block of 64 faces / superblock of 64 blocks
//   bkeys [nblocks]        the key of every block's first face: the seed block of a wave is found in it by binary search
// The search (k_meshdist_search): one wave per 64 queries in the key order of the queries, GHR_MD_WAVES waves per workgroup;
// the wave stages a block's records in its private 3 KB of LDS and every lane reads the same address (broadcasts); the walk
// (md_wave_search, shared with ghr_grow.h's guarded trace) is knn_walk's: seed block, then the superblocks in rotation, wave
// ballots on needs(bound) -- and inside a staged block one more
// ballot per face on the bound of the face's own box, which skips most faces of a neighbouring block.  k_meshdist_bwd: one thread per
// point, no atomics.  Per-element functions are GHR_HD and the header is plain C++ outside __HIPCC__
// (tests/hostsim/ghr_hostsim_meshdist.cpp walks them); GHR_MD_CHECK(cond) is an assert there and nothing in the library.
#pragma once
#include "ghr_nn.h"
#include "ghr_mesh.h"
#include <algorithm>
#include <vector>

#ifndef GHR_MD_CHECK
#define GHR_MD_CHECK(cond) ((void)0)
#endif

#define GHR_MD_MAGIC 0x54524847u  // "GHRT"
#define GHR_MD_REC_WORDS 12       // three 16-B units per face
#define GHR_MD_WAVES 4            // waves per workgroup of k_meshdist_search
#define GHR_MD_BLOCK 256          // threads per workgroup of k_meshdist_bwd
#define GHR_MD_COORD_MAX 1073741824.0f  // 2^30: with |coordinate| <= this no ee, nn of a face overflows

namespace ghr {

// The header of the triangle blob (== ghr_mesh_tris of include/ghr.h); offsets in bytes from the blob's start.
struct MeshTris {
    uint32_t magic;
    int32_t n_faces, n_blocks, n_super;
    float lo[3], hi[3];  // the box of the vertices that faces use: the bounds of the faces' and the queries' keys
    uint32_t pad_[2];
    uint64_t off_rec, off_bbox, off_sbox, off_keys;
    uint64_t bytes;
};

#if defined(__HIPCC__)
GHR_HD float4 md_f4(float x, float y, float z) { return make_float4(x, y, z, 0.f); }
#else
inline float4 md_f4(float x, float y, float z) { return float4{x, y, z, 0.f}; }
#endif

struct MdVec { float x, y, z; };
GHR_HD MdVec md_sub(MdVec a, MdVec b) { return MdVec{a.x - b.x, a.y - b.y, a.z - b.z}; }
GHR_HD float md_dot(MdVec a, MdVec b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
GHR_HD MdVec md_cross(MdVec a, MdVec b) { return MdVec{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
GHR_HD float md_min(float a, float b) { return a < b ? a : b; }
GHR_HD float md_max(float a, float b) { return a > b ? a : b; }
GHR_HD float md_clamp(float x, float lo, float hi)
{
    const float t = x > lo ? x : lo;  // (a NaN lands on lo)
    return t < hi ? t : hi;
}
GHR_HD MdVec md_clamp3(MdVec c, MdVec lo, MdVec hi) { return MdVec{md_clamp(c.x, lo.x, hi.x), md_clamp(c.y, lo.y, hi.y), md_clamp(c.z, lo.z, hi.z)}; }
GHR_HD bool md_finite(float x) { return fabsf(x) <= FLT_MAX; }  // (a NaN fails the comparison)

// candidate 1: the closest point of segment (P0, P1), and its d
GHR_HD float md_edge(MdVec P0, MdVec P1, MdVec q, MdVec* c)
{
    const MdVec e = md_sub(P1, P0), w = md_sub(q, P0);
    const float ee = md_dot(e, e), ew = md_dot(e, w);
    const float t = ee > 0.f ? md_clamp(ew / ee, 0.f, 1.f) : 0.f;
    MdVec p{P0.x + t * e.x, P0.y + t * e.y, P0.z + t * e.z};
    if (t == 1.f) p = P1;
    p = md_clamp3(p, MdVec{md_min(P0.x, P1.x), md_min(P0.y, P1.y), md_min(P0.z, P1.z)},
                  MdVec{md_max(P0.x, P1.x), md_max(P0.y, P1.y), md_max(P0.z, P1.z)});
    *c = p;
    const MdVec r = md_sub(p, q);
    return md_dot(r, r);
}

// One face (A, B, C in vertex-index order) against one query: its d and closest point.
GHR_HD float md_face(MdVec A, MdVec B, MdVec C, MdVec q, MdVec* c)
{
    MdVec best, p;
    float d = md_edge(A, B, q, &best);
    float dk = md_edge(A, C, q, &p);
    if (dk < d) { d = dk; best = p; }
    dk = md_edge(B, C, q, &p);
    if (dk < d) { d = dk; best = p; }
    const MdVec ab = md_sub(B, A), ac = md_sub(C, A);
    const MdVec n = md_cross(ab, ac);
    const float nn = md_dot(n, n);
    const float s0 = md_dot(md_cross(md_sub(C, B), md_sub(q, B)), n);
    const float s1 = md_dot(md_cross(md_sub(A, C), md_sub(q, C)), n);
    const float s2 = md_dot(md_cross(ab, md_sub(q, A)), n);
    const bool accepted = nn > 0.f && s0 >= 0.f && s1 >= 0.f && s2 >= 0.f;
    const float k = nn > 0.f ? md_dot(n, md_sub(q, A)) / nn : 0.f;
    p = MdVec{q.x - k * n.x, q.y - k * n.y, q.z - k * n.z};
    p = md_clamp3(p, MdVec{md_min(md_min(A.x, B.x), C.x), md_min(md_min(A.y, B.y), C.y), md_min(md_min(A.z, B.z), C.z)},
                  MdVec{md_max(md_max(A.x, B.x), C.x), md_max(md_max(A.y, B.y), C.y), md_max(md_max(A.z, B.z), C.z)});
    const MdVec r = md_sub(p, q);
    dk = md_dot(r, r);
    if (accepted && dk < d) { d = dk; best = p; }
    *c = best;
    return d;
}

// One lane's state of the walk (the policy of knn_walk, for records instead of points).
struct MdNearest {
    float best = __builtin_inff();  // +inf: a d that overflowed still has to find its lowest face
    int face = 0x7fffffff;          // loses every index tie
    MdVec point = MdVec{0.f, 0.f, 0.f};
    GHR_HD float bound(float3 q, float4 lo, float4 hi) const { return knn_box_dist(q, lo, hi); }
    GHR_HD bool needs(float boxdist) const { return !(boxdist > best); }
    // one staged record (three float4); every lane of a wave reads the same address
    GHR_HD void take(const float4* r, MdVec q)
    {
        const float4 r0 = r[0], r1 = r[1], r2 = r[2];
        MdVec c;
        const float d = md_face(MdVec{r0.x, r0.y, r0.z}, MdVec{r0.w, r1.x, r1.y}, MdVec{r1.z, r1.w, r2.x}, q, &c);
        const int f = knn_as_int(r2.y);
        if (d < best || (d == best && f < face)) { best = d; face = f; point = c; }
    }
    // the lower bound of d over one staged record's own box (every candidate of a face lies in its triangle's box)
    GHR_HD float face_bound(const float4* r, float3 q) const
    {
        const float4 r0 = r[0], r1 = r[1], r2 = r[2];
        const float4 lo = md_f4(fminf(fminf(r0.x, r0.w), r1.z), fminf(fminf(r0.y, r1.x), r1.w), fminf(fminf(r0.z, r1.y), r2.x));
        const float4 hi = md_f4(fmaxf(fmaxf(r0.x, r0.w), r1.z), fmaxf(fmaxf(r0.y, r1.x), r1.w), fmaxf(fmaxf(r0.z, r1.y), r2.x));
        return knn_box_dist(q, lo, hi);
    }
};

// The block whose first key is the last one <= kq (block 0 when none is): where a face at key kq would be.
GHR_HD int md_seed_block(const unsigned long long* bkeys, int nblocks, unsigned long long kq)
{
    int lo = 0, hi = nblocks;  // first block whose key is > kq
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (bkeys[mid] <= kq) lo = mid + 1; else hi = mid;
    }
    return lo > 0 ? lo - 1 : 0;
}

// The tables of one blob, as pointers (host or device memory alike).
struct MdView {
    int n_faces, n_blocks, n_super;
    const float4 *rec, *bbox, *sbox;
    const unsigned long long* bkeys;
};

GHR_HD MdView md_view(const MeshTris& h, const void* blob)
{
    const char* b = static_cast<const char*>(blob);
    return MdView{h.n_faces, h.n_blocks, h.n_super, reinterpret_cast<const float4*>(b + h.off_rec),
                  reinterpret_cast<const float4*>(b + h.off_bbox), reinterpret_cast<const float4*>(b + h.off_sbox),
                  reinterpret_cast<const unsigned long long*>(b + h.off_keys)};
}

// the gradient of sd = sign sqrt(d) to the query: t = g sign, t ((q - c) / sqrtf(d)) per component; 0 where d == 0 or not finite
GHR_HD void md_backward_one(const float* q, const float* c, float d, bool inside, float g, float* out)
{
    const bool live = d > 0.f && d <= FLT_MAX && md_finite(q[0]) && md_finite(q[1]) && md_finite(q[2]);
    const float t = g * (inside ? -1.f : 1.f), s = live ? sqrtf(d) : 1.f;
    for (int k = 0; k < 3; ++k) out[k] = live ? t * ((q[k] - c[k]) / s) : 0.f;
}

// ---- the builder (host) --------------------------------------------------------------------------------------------------
// Validates the mesh and sizes the blob: fills every field of *h.  Returns NULL or what is wrong.
inline const char* mesh_tris_plan(int n_vertices, const float* vertices, int n_faces, const int32_t* faces, MeshTris* h)
{
    if (n_vertices < 0 || n_faces < 0) return "negative count";
    if (n_faces == 0) return "F == 0: there is no closest point on an empty mesh";
    if (!vertices || !faces) return "NULL vertices or faces";
    for (size_t i = 0; i < 3 * (size_t)n_faces; i++)
        if (faces[i] < 0 || faces[i] >= n_vertices) return "a face index is outside the vertices";
    memset(h, 0, sizeof(*h));
    h->magic = GHR_MD_MAGIC;
    h->n_faces = n_faces;
    h->n_blocks = (n_faces + GHR_KNN_BLOCK - 1) / GHR_KNN_BLOCK;
    h->n_super = (h->n_blocks + GHR_KNN_SUPER - 1) / GHR_KNN_SUPER;
    for (size_t i = 0; i < 3 * (size_t)n_faces; i++)
        for (int c = 0; c < 3; c++) {
            const float x = vertices[3 * (size_t)faces[i] + c];
            if (!(fabsf(x) <= GHR_MD_COORD_MAX)) return "a vertex coordinate is not finite or beyond 2^30";
            if (i == 0) { h->lo[c] = x; h->hi[c] = x; }
            h->lo[c] = fminf(h->lo[c], x); h->hi[c] = fmaxf(h->hi[c], x);
        }
    size_t off = mesh_up16(sizeof(MeshTris));
    h->off_rec = off; off = mesh_up16(off + sizeof(float) * GHR_MD_REC_WORDS * (size_t)n_faces);
    h->off_bbox = off; off = mesh_up16(off + 2 * sizeof(float4) * (size_t)h->n_blocks);
    h->off_sbox = off; off = mesh_up16(off + 2 * sizeof(float4) * (size_t)h->n_super);
    h->off_keys = off; off = mesh_up16(off + sizeof(uint64_t) * (size_t)h->n_blocks);
    h->bytes = off;
    return nullptr;
}

// Fills a blob of plan.bytes bytes (16-B aligned).  Returns NULL or what is wrong.
inline const char* mesh_tris_fill(const float* vertices, const int32_t* faces, const MeshTris& plan, void* blob)
{
    const MeshTris h = plan;
    char* out = static_cast<char*>(blob);
    memset(out, 0, (size_t)h.bytes);
    const int F = h.n_faces;
    const float bounds[6] = {h.lo[0], h.lo[1], h.lo[2], h.hi[0], h.hi[1], h.hi[2]};
    struct Item { unsigned long long key; int32_t face; };
    std::vector<Item> items((size_t)F);
    for (int f = 0; f < F; f++) {
        const int32_t* t = faces + 3 * (size_t)f;
        float centre[3];
        for (int c = 0; c < 3; c++) {
            const float a = vertices[3 * (size_t)t[0] + c], b = vertices[3 * (size_t)t[1] + c], d = vertices[3 * (size_t)t[2] + c];
            centre[c] = (fminf(fminf(a, b), d) + fmaxf(fmaxf(a, b), d)) * 0.5f;
        }
        items[(size_t)f] = Item{knn_key(centre, bounds), f};
    }
    std::sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.key < b.key || (a.key == b.key && a.face < b.face); });
    float* rec = reinterpret_cast<float*>(out + h.off_rec);
    float4* bbox = reinterpret_cast<float4*>(out + h.off_bbox);
    float4* sbox = reinterpret_cast<float4*>(out + h.off_sbox);
    uint64_t* bkeys = reinterpret_cast<uint64_t*>(out + h.off_keys);
    for (int s = 0; s < h.n_super; s++) {
        sbox[2 * s] = md_f4(FLT_MAX, FLT_MAX, FLT_MAX);
        sbox[2 * s + 1] = md_f4(-FLT_MAX, -FLT_MAX, -FLT_MAX);
    }
    for (int b = 0; b < h.n_blocks; b++) {
        float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
        const int end = F < (b + 1) * GHR_KNN_BLOCK ? F : (b + 1) * GHR_KNN_BLOCK;
        bkeys[b] = items[(size_t)b * GHR_KNN_BLOCK].key;
        for (int i = b * GHR_KNN_BLOCK; i < end; i++) {
            const int32_t f = items[(size_t)i].face;
            int32_t t[3] = {faces[3 * (size_t)f], faces[3 * (size_t)f + 1], faces[3 * (size_t)f + 2]};
            // A, B, C: the vertices in vertex-index order
            if (t[0] > t[1]) std::swap(t[0], t[1]);
            if (t[1] > t[2]) std::swap(t[1], t[2]);
            if (t[0] > t[1]) std::swap(t[0], t[1]);
            float* r = rec + (size_t)GHR_MD_REC_WORDS * i;
            for (int k = 0; k < 3; k++)
                for (int c = 0; c < 3; c++) {
                    const float x = vertices[3 * (size_t)t[k] + c];
                    r[3 * k + c] = x;
                    lo[c] = fminf(lo[c], x); hi[c] = fmaxf(hi[c], x);
                }
            memcpy(r + 9, &f, 4);
        }
        bbox[2 * b] = md_f4(lo[0], lo[1], lo[2]);
        bbox[2 * b + 1] = md_f4(hi[0], hi[1], hi[2]);
        float4 &slo = sbox[2 * (b / GHR_KNN_SUPER)], &shi = sbox[2 * (b / GHR_KNN_SUPER) + 1];
        slo = md_f4(fminf(slo.x, lo[0]), fminf(slo.y, lo[1]), fminf(slo.z, lo[2]));
        shi = md_f4(fmaxf(shi.x, hi[0]), fmaxf(shi.y, hi[1]), fmaxf(shi.z, hi[2]));
    }
    memcpy(out, &h, sizeof(h));
    return nullptr;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#ifdef GHR_MD_COUNT_BLOCKS
// measurement build only (tools/build_variant.sh -DGHR_MD_COUNT_BLOCKS): [0] blocks scanned by the walk, [1] waves, [2] faces
// evaluated (the faces of scanned blocks that passed their own box's ballot)
__device__ unsigned long long g_md_count[3];
#define GHR_MD_COUNTING(code) code
#else
#define GHR_MD_COUNTING(code)
#endif

struct MdSearchArgs {
    MdView m;
    int Q;
    const float* points;                // [Q][3]
    const long long* order;             // [Q]: the permutation that sorts the queries' keys
    const unsigned long long* keys;     // [Q]: the sorted keys
    float* dist2;                       // [Q]
    int* face;                          // [Q]
    float* point;                       // [Q][3]
};

// The wave loop of the search (every lane of the wave makes the call): `tile` is the wave's private 3 * GHR_KNN_BLOCK float4 of
// LDS, q the lane's query, `valid` whether the lane has a finite one (an invalid lane votes in no ballot), `first` the
// wave-uniform seed block, near the lane's state.  Seed block, then the superblocks in rotation from the seed's on; wave ballots on
// needs(bound) skip superblocks and blocks, and inside a staged block one more ballot per face on the bound of the face's own box.
// The results do not depend on `first` (the total order of the definition).  k_meshdist_search and k_grow_guarded (ghr_grow.h)
// call it; each wave works on its own, only wave-level fences order the tile's reuse.
__device__ __forceinline__ void md_wave_search(const MdView& m, float4* tile, MdVec q, bool valid, int first, MdNearest& near)
{
    const int lane = threadIdx.x & 63;
    const float3 q3 = make_float3(q.x, q.y, q.z);
    GHR_MD_COUNTING(unsigned scanned = 0; unsigned taken = 0;)
    auto scan_block = [&](int blk) {
        const int n = min(GHR_KNN_BLOCK, m.n_faces - blk * GHR_KNN_BLOCK);
        knn_wave_lds_fence();  // every lane is done reading the previous tile
        for (int k = 0; k < 3; ++k) {
            const int i = k * GHR_KNN_BLOCK + lane;  // 64 consecutive 16-B units per pass
            if (i < 3 * n) tile[i] = m.rec[(size_t)blk * (3 * GHR_KNN_BLOCK) + i];
        }
        knn_wave_lds_fence();
        for (int j = 0; j < n; ++j) {
            // a face whose own box no lane still needs is skipped by the wave, as a block is: the same bound, the same `>`
            if (!__any(valid && near.needs(near.face_bound(tile + 3 * j, q3)))) continue;
            near.take(tile + 3 * j, q);
            GHR_MD_COUNTING(++taken;)
        }
        GHR_MD_COUNTING(++scanned;)
    };
    scan_block(first);
    const int first_sb = first / GHR_KNN_SUPER;
    for (int s = 0; s < m.n_super; ++s) {
        const int sb = first_sb + s < m.n_super ? first_sb + s : first_sb + s - m.n_super;
        if (!__any(valid && near.needs(near.bound(q3, m.sbox[2 * sb], m.sbox[2 * sb + 1])))) continue;
        const int b_end = min(m.n_blocks, (sb + 1) * GHR_KNN_SUPER);
        for (int blk = sb * GHR_KNN_SUPER; blk < b_end; ++blk) {
            if (blk == first) continue;  // scanned above
            if (!__any(valid && near.needs(near.bound(q3, m.bbox[2 * blk], m.bbox[2 * blk + 1])))) continue;
            scan_block(blk);
        }
    }
    GHR_MD_COUNTING(if (lane == 0) { atomicAdd(&g_md_count[0], (unsigned long long)scanned); atomicAdd(&g_md_count[1], 1ull);
                                      atomicAdd(&g_md_count[2], (unsigned long long)taken); })
}

// One wave per 64 queries in key order; outputs at the queries' original indices.  An order entry outside [0, Q) (only a
// caller's bad permutation can hold one) is read as 0, so no access leaves the buffers.
__global__ void __launch_bounds__(64 * GHR_MD_WAVES) k_meshdist_search(MdSearchArgs a)
{
    __shared__ float4 tiles[GHR_MD_WAVES][3 * GHR_KNN_BLOCK];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long qb = (long long)blockIdx.x * GHR_MD_WAVES + wave;
    const long long q0 = qb * GHR_KNN_BLOCK;
    if (q0 >= a.Q) return;
    const MdView& m = a.m;
    const bool has = q0 + lane < a.Q;
    const int nq = (int)min((long long)GHR_KNN_BLOCK, a.Q - q0);
    long long o = a.order[has ? q0 + lane : q0];
    if (o < 0 || o >= a.Q) o = 0;
    const MdVec q{a.points[3 * o], a.points[3 * o + 1], a.points[3 * o + 2]};
    const bool finite = md_finite(q.x) && md_finite(q.y) && md_finite(q.z);
    const bool valid = has && finite;  // a lane without a finite query votes in no ballot
    const int first = __builtin_amdgcn_readfirstlane(md_seed_block(m.bkeys, m.n_blocks, a.keys[q0 + nq / 2]));
    MdNearest near;
    md_wave_search(m, tiles[wave], q, valid, first, near);
    if (has) {
        a.dist2[o] = finite ? near.best : __builtin_inff();
        a.face[o] = finite && (unsigned)near.face < (unsigned)m.n_faces ? near.face : -1;
        a.point[3 * o] = finite ? near.point.x : q.x;
        a.point[3 * o + 1] = finite ? near.point.y : q.y;
        a.point[3 * o + 2] = finite ? near.point.z : q.z;
    }
}

// One thread per point.  closest [Q][3], dist2 [Q], inside [Q] (HeadMesh.contains'), g [Q] -> d_points [Q][3].
__global__ void __launch_bounds__(GHR_MD_BLOCK) k_meshdist_bwd(long long Q, const float* __restrict__ points,
                                                                const float* __restrict__ closest, const float* __restrict__ dist2,
                                                                const unsigned char* __restrict__ inside, const float* __restrict__ g,
                                                                float* __restrict__ d_points)
{
    const long long i = (long long)blockIdx.x * GHR_MD_BLOCK + threadIdx.x;
    if (i >= Q) return;
    const float q[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
    const float c[3] = {closest[3 * i], closest[3 * i + 1], closest[3 * i + 2]};
    float out[3];
    md_backward_one(q, c, dist2[i], inside[i] != 0, g[i], out);
    d_points[3 * i] = out[0]; d_points[3 * i + 1] = out[1]; d_points[3 * i + 2] = out[2];
}
#endif  // __HIPCC__

}  // namespace ghr
