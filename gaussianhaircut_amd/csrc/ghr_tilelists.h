// ghr_tilelists.h -- per-tile lists of screen primitives, and the walk of one tile's list by a workgroup.  The head-mesh raster
// (ghr_visibility.h: faces), the strand preview and its deep opacity map (ghr_strandview.h: segments) are built on it; what a
// primitive is, how its record is set up and what happens at a pixel stay with them.
//
//   Points are projected to {sx, sy, q = 1 / w, valid} (16 B each).  Every primitive has a RECORD of `UNITS` 16-B units, written by
//   its owner's setup; the record's last two words are the list builder's (tl_rect):
//       xy   = first tile x | first tile y << 16
//       bits = the owner's flags (bits 0 .. 2) | GHR_TL_NEVER | GHR_TL_EMPTY | GHR_TL_BIG | (tiles across - 1) << 8 | (tiles down - 1) << 16
//   The rectangle is the 16 x 16 tiles that hold a pixel centre of the primitive's closed box (tl_pixel_range: conservative by
//   monotone rounding, clipped to the image, EMPTY when off-screen or NEVER).  A primitive of at most `big_rect` tiles is counted
//   into each of them; a larger one (BIG; the two extents are then left 0) goes to the view's one big list, which every tile
//   walks after its own: the lists never hold more than `big_rect` entries per primitive, so the workspace is sized from the
//   counts and the image alone, with no read-back.  big_rect <= 256 keeps either extent of a listed rectangle in its 8 bits.
//
// Per view: one fill of the tile counts and the big list's length (and whatever its owner put behind them), then
//   k_tl_project   one thread per point
//   (the owner's setup kernel: one thread per primitive, the record, then tl_count)
//   k_tl_scan      one workgroup: exclusive scan of the tile counts -> start [T + 1]; the counts become the fill cursors
//   k_tl_scatter   one thread per primitive: its id into the lists of its tiles (integer atomics; the order inside a list is free)
// and the owner's raster: one 256-thread workgroup per tile, one pixel per thread, around tl_walk -- records staged in LDS a chunk at
// a time; a wave none of whose lanes is in a record's box skips it by ballot.
// Everything per element is GHR_HD so that tests/hostsim/ghr_hostsim_tilelists.h runs the same arithmetic in a checked host walk.
#pragma once
#include "ghr_mesh.h"

#define GHR_TL_TILE 16
#define GHR_TL_BLOCK 256
#define GHR_TL_NEVER 8u   // covers no pixel, whatever its box
#define GHR_TL_EMPTY 16u  // no tile
#define GHR_TL_BIG 32u    // on the big list

namespace ghr {

GHR_HD bool vis_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }  // (a NaN fails the comparison)

// One point: out = {sx, sy, q, valid ? 1 : 0}.
GHR_HD void vis_project_one(const float* M, const float* X, float near, float* out)
{
    const float xp = (M[0] * X[0] + M[1] * X[1]) + (M[2] * X[2] + M[3]);
    const float yp = (M[4] * X[0] + M[5] * X[1]) + (M[6] * X[2] + M[7]);
    const float w = (M[8] * X[0] + M[9] * X[1]) + (M[10] * X[2] + M[11]);
    out[0] = xp / w;
    out[1] = yp / w;
    out[2] = 1.f / w;
    out[3] = (vis_finite(w) && w > near) ? 1.f : 0.f;
}

// The pixel columns (or rows) whose centre can lie in [lo, hi], clipped to 0 .. n - 1; false when there is none.
// j + 0.5 >= lo implies j >= fl(lo - 0.5) (rounding is monotone, j exact), so floor() of the rounded difference is never
// too large; likewise at the upper end.  A NaN bound gives an empty range: the box test then fails at every centre too.
GHR_HD bool tl_pixel_range(float lo, float hi, int n, int* j0, int* j1)
{
    if (!(lo <= (float)n) || !(hi >= 0.f)) return false;
    const float a = lo - 0.5f, b = hi - 0.5f;
    *j0 = a <= 0.f ? 0 : (int)floorf(a);             // (a <= n: the conversion is in range)
    *j1 = b >= (float)(n - 1) ? n - 1 : (int)floorf(b);  // (b >= -0.5: -1 at the least)
    return *j0 <= *j1;
}

// The last two words of a record, tail[2] = {xy, bits}, from the owner's flags and the primitive's closed box.
GHR_HD void tl_rect(uint32_t flags, float ulo, float uhi, float vlo, float vhi, int H, int W, uint32_t big_rect, float* tail)
{
    uint32_t xy = 0u, bits = flags;
    int j0 = 0, j1 = -1, i0 = 0, i1 = -1;
    if (!(flags & GHR_TL_NEVER) && tl_pixel_range(ulo, uhi, W, &j0, &j1) && tl_pixel_range(vlo, vhi, H, &i0, &i1)) {
        const uint32_t x0 = (uint32_t)j0 / GHR_TL_TILE, x1 = (uint32_t)j1 / GHR_TL_TILE;
        const uint32_t y0 = (uint32_t)i0 / GHR_TL_TILE, y1 = (uint32_t)i1 / GHR_TL_TILE;
        xy = x0 | (y0 << 16);
        if ((uint64_t)(x1 - x0 + 1u) * (y1 - y0 + 1u) > big_rect) bits |= GHR_TL_BIG;
        else bits |= ((x1 - x0) << 8) | ((y1 - y0) << 16);  // (each below big_rect)
    } else {
        bits |= GHR_TL_EMPTY;
    }
    memcpy(tail, &xy, 4);
    memcpy(tail + 1, &bits, 4);
}

// The tiles x0 .. x1, y0 .. y1 of a record that is neither EMPTY nor BIG.
GHR_HD void tl_rect_tiles(uint32_t xy, uint32_t bits, uint32_t* x0, uint32_t* x1, uint32_t* y0, uint32_t* y1)
{
    *x0 = xy & 0xffffu; *x1 = *x0 + ((bits >> 8) & 0xffu);
    *y0 = xy >> 16; *y1 = *y0 + ((bits >> 16) & 0xffu);
}

// ---- the workspace ---------------------------------------------------------------------------------------------------------
// Offsets in bytes, 16-B aligned.  [off_fill, off_fill + fill_bytes) is what a view zeroes first: the tile counts and the length
// of the big list.  It is the last region, so that an owner can put more of what starts a view at 0 behind it, in the same fill.
struct TileListLayout {
    uint64_t off_proj, off_rec, off_start, off_list, off_big, off_fill, off_count, off_nbig, fill_bytes;
    uint64_t list_cap;
    int32_t tiles_x, tiles_y;
};

inline const char* tl_layout(int64_t n_points, int64_t n_prims, int64_t H, int64_t W, uint32_t rec_units, uint32_t big_rect,
                             TileListLayout* L)
{
    if (n_points < 0 || n_prims < 0 || H < 0 || W < 0) return "negative size";
    if (n_points > 0x7fffffff || n_prims > 0x7fffffff || H > 0x7fffffff || W > 0x7fffffff) return "a size exceeds 2^31 - 1";
    if ((uint64_t)H * (uint64_t)W > 0x7fffffffull) return "H * W exceeds 32-bit offsets";
    const uint64_t tx = ((uint64_t)W + GHR_TL_TILE - 1) / GHR_TL_TILE, ty = ((uint64_t)H + GHR_TL_TILE - 1) / GHR_TL_TILE;
    if (tx > 65535 || ty > 65535) return "image too large for 16-bit tile coordinates";
    const uint64_t T = tx * ty;
    const uint64_t cap = (uint64_t)n_prims * (T < big_rect ? T : big_rect);
    if (cap > 0x7fffffffull) return "the tile lists exceed 32-bit offsets";
    L->tiles_x = (int32_t)tx; L->tiles_y = (int32_t)ty;
    L->list_cap = cap;
    uint64_t off = 0;
    L->off_proj = off; off = mesh_up16(off + 16ull * (uint64_t)n_points);
    L->off_rec = off; off += 16ull * rec_units * (uint64_t)n_prims;
    L->off_start = off; off = mesh_up16(off + 4ull * (T + 1));
    L->off_list = off; off = mesh_up16(off + 4ull * cap);
    L->off_big = off; off = mesh_up16(off + 4ull * (uint64_t)n_prims);
    L->off_fill = off;
    L->off_count = off; off = mesh_up16(off + 4ull * T);
    L->off_nbig = off; off += 16;
    L->fill_bytes = off - L->off_fill;
    return nullptr;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
struct TileLists {
    uint32_t n_points, n_prims;
    int32_t tiles_x, tiles_y;
    float near;
    float M[12];
    const float* points;  // [n_points][3]
    float* proj;          // [n_points][4]
    float* rec;           // [n_prims][4 UNITS]
    uint32_t* start;      // [T + 1]
    uint32_t* count;      // [T]: counts, then fill cursors
    uint32_t* nbig;
    uint32_t* list;       // [list_cap]
    uint32_t* big;        // [n_prims]
    uint32_t list_cap;
};

__global__ void __launch_bounds__(GHR_TL_BLOCK) k_tl_project(TileLists tl)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t v = blockIdx.x * GHR_TL_BLOCK + threadIdx.x;
    if (v >= tl.n_points) return;
    const float X[3] = {tl.points[3 * (size_t)v], tl.points[3 * (size_t)v + 1], tl.points[3 * (size_t)v + 2]};
    float o[4];
    vis_project_one(tl.M, X, tl.near, o);
    reinterpret_cast<f4*>(tl.proj)[v] = f4{o[0], o[1], o[2], o[3]};
#endif
}

// The end of an owner's setup thread: primitive `id`, whose record ends in tail[2], into the big list or the counts of its tiles.
__device__ __forceinline__ void tl_count(const TileLists& tl, const float* tail, uint32_t id)
{
    uint32_t xy, bits, x0, x1, y0, y1;
    memcpy(&xy, tail, 4); memcpy(&bits, tail + 1, 4);
    if (bits & GHR_TL_EMPTY) return;
    if (bits & GHR_TL_BIG) {
        const uint32_t pos = atomicAdd(tl.nbig, 1u);
        if (pos < tl.n_prims) tl.big[pos] = id;  // (one entry per primitive at the most: always true)
        return;
    }
    tl_rect_tiles(xy, bits, &x0, &x1, &y0, &y1);
    for (uint32_t y = y0; y <= y1; y++)
        for (uint32_t x = x0; x <= x1; x++) atomicAdd(&tl.count[y * (uint32_t)tl.tiles_x + x], 1u);
}

// One workgroup.  start[t] = the entries of the tiles before t; count[t] becomes the fill cursor of tile t (= start[t]).
__global__ void __launch_bounds__(GHR_TL_BLOCK) k_tl_scan(TileLists tl)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ uint32_t s_tmp[4];
    const uint32_t T = (uint32_t)tl.tiles_x * (uint32_t)tl.tiles_y;
    uint32_t run = 0u;
    for (uint32_t base = 0u; base < T; base += GHR_TL_BLOCK) {
        const uint32_t t = base + threadIdx.x;
        const uint32_t n = t < T ? tl.count[t] : 0u;
        uint32_t total;
        const uint32_t before = block_excl_scan_256(n, s_tmp, &total);
        if (t < T) { tl.start[t] = run + before; tl.count[t] = run + before; }
        run += total;
        __syncthreads();  // s_tmp is written again in the next round
    }
    if (threadIdx.x == 0) tl.start[T] = run;
#endif
}

template <int UNITS>
__global__ void __launch_bounds__(GHR_TL_BLOCK) k_tl_scatter(TileLists tl)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t id = blockIdx.x * GHR_TL_BLOCK + threadIdx.x;
    if (id >= tl.n_prims) return;
    const uint32_t* tail = reinterpret_cast<const uint32_t*>(tl.rec) + (size_t)(4 * UNITS) * id + (4 * UNITS - 2);
    const uint32_t xy = tail[0], bits = tail[1];
    if (bits & (GHR_TL_EMPTY | GHR_TL_BIG)) return;
    uint32_t x0, x1, y0, y1;
    tl_rect_tiles(xy, bits, &x0, &x1, &y0, &y1);
    for (uint32_t y = y0; y <= y1; y++)
        for (uint32_t x = x0; x <= x1; x++) {
            const uint32_t pos = atomicAdd(&tl.count[y * (uint32_t)tl.tiles_x + x], 1u);
            if (pos < tl.list_cap) tl.list[pos] = id;  // (at most big_rect entries per primitive: always true)
        }
#endif
}

// One walk of a tile's entries (its own list, then the big list) by its 256-thread workgroup: CHUNK records at a time into
// s_rec [UNITS * CHUNK] (UNITS * CHUNK <= 256: one 16-B unit per thread) and, with IDS, their ids into s_id [CHUNK]; a walk that
// needs no ids stages none (s_id is not touched) and its visit gets 0.  in_box(r) is the caller's cheap test of a record's box at
// the thread's pixel (false outside the image); visit(r, id) runs in the lanes where it holds, and a wave where it holds nowhere
// skips the record.  Every thread of the workgroup makes the call (it has barriers).
template <int UNITS, int CHUNK, bool IDS, class InBox, class Visit>
__device__ __forceinline__ void tl_walk(const TileLists& tl, uint32_t tile, f4* s_rec, uint32_t* s_id, InBox in_box, Visit visit)
{
    static_assert(UNITS * CHUNK <= GHR_TL_BLOCK, "one 16-B unit per thread");
    const uint32_t beg = tl.start[tile], n_own = tl.start[tile + 1] - beg;
    const uint32_t n_big = tl.n_prims > 0u ? min(*tl.nbig, tl.n_prims) : 0u;
    const uint32_t n = n_own + n_big;  // (workgroup-uniform)
    for (uint32_t c0 = 0u; c0 < n; c0 += CHUNK) {
        const uint32_t m = min((uint32_t)CHUNK, n - c0);
        if (threadIdx.x < (uint32_t)UNITS * m) {
            const uint32_t k = threadIdx.x / UNITS, part = threadIdx.x % UNITS, e = c0 + k;
            // (beg + e < start[T] <= list_cap and every id < n_prims; the clamps keep a workspace that two streams were wrongly
            // given at once from ever indexing outside it)
            uint32_t id = e < n_own ? tl.list[min(beg + e, tl.list_cap - 1u)] : tl.big[e - n_own];
            id = min(id, tl.n_prims - 1u);
            s_rec[UNITS * k + part] = reinterpret_cast<const f4*>(tl.rec)[UNITS * (size_t)id + part];
            if (IDS && part == 0u) s_id[k] = id;
        }
        __syncthreads();
        for (uint32_t k = 0u; k < m; k++) {
            float r[4 * UNITS];
#pragma unroll
            for (int u = 0; u < UNITS; u++) {
                const f4 q = s_rec[UNITS * k + u];  // (one address per wave: broadcast)
                r[4 * u] = q.x; r[4 * u + 1] = q.y; r[4 * u + 2] = q.z; r[4 * u + 3] = q.w;
            }
            const bool box = in_box(r);
            if (__builtin_amdgcn_ballot_w64(box) == 0ull) continue;  // nobody in this wave is inside the box
            if (!box) continue;
            if constexpr (IDS) visit(r, s_id[k]);  // (the LDS word itself: read where the visit uses it, if it does)
            else visit(r, 0u);
        }
        __syncthreads();
    }
}
#endif  // __HIPCC__

}  // namespace ghr
