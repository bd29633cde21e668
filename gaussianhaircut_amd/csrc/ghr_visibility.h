// ghr_visibility.h -- which vertices of the head mesh does a training view see, at all and through the head-minus-hair mask
// (DESIGN.md 8h): the triangle rasterizer of src/preprocessing/extract_non_visible_head_scalp.py:51-72,112-115.  The reference
// asks pytorch3d's MeshRasterizer; that library is not a dependency, so the result is DEFINED here, exactly and independently
// of any traversal order, and every form (these kernels, the host simulator, the PyTorch comparator, the numpy model of the
// tests) is held to it bit for bit.  Everything is float32 without contraction, in the operand order written.
//
//   View: M[12], a row-major 3 x 4 matrix; H, W; near.
//   Vertex X:  x' = (M0 X0 + M1 X1) + (M2 X2 + M3), likewise y' (M4..7) and w (M8..11);  sx = x' / w, sy = y' / w, q = 1 / w.
//       It is VALID iff w is finite and w > near.
//   Pixel (row i, column j) is sampled at its centre (j + 0.5, i + 0.5).
//   A face COVERS a pixel when its three vertices are valid, its three indices differ (and index a vertex), mesh_flat of its
//       screen triangle is false, the centre lies in the closed box of the three screen vertices (fminf / fmaxf), and the centre
//       is on the same side of its three edges -- either winding: back faces count (the script's cull_backfaces=False).  Every
//       edge is evaluated ONCE with ghr::mesh_edge (csrc/ghr_mesh.h) in its canonical direction, from the lower to the higher
//       vertex index; a triangle that walks it the other way takes the complement, so the two faces of a shared edge see
//       complementary predicates: a centre on a shared edge belongs to exactly one of them.
//   Its inverse depth there is  ((e1 q0 + e2 q1) + e0 q2) / ((e0 + e1) + e2),  e_k = the edge value in the triangle's own
//       direction (inverse depth is planar in screen space, which w is not).
//   The WINNER of a pixel is the covering face with the largest inverse depth, the lowest face index among equals; a covering
//       face whose inverse depth is NaN (or -Inf) never wins.  pix_to_face [H][W] int32, -1 where nothing wins.  This is a
//       maximum under a total order: binning, chunking and traversal order cannot change a bit of it.
//   Head mask from two uint8 planes:  head = (max5x5(body) >= 128) and not (max5x5(hair) >= 128), the window clipped to the image
//       (script lines 112-115: cv2.dilate's default border ignores what lies outside; / 255. >= 0.5 is >= 128).
//   A vertex is SEEN in the view when one of its faces wins a pixel, SEEN THROUGH THE HEAD when one wins a pixel where head
//       holds; vis [H][W] is 255 where pix_to_face >= 0 and head, else 0.
//
// Per view (ghr_vis_view): one fill of the counters and flags, then
//   k_vis_project   one thread per vertex: {sx, sy, q, valid}, 16 B
//   k_vis_setup     one thread per face: a 48-B record  sx0 sy0 sx1 sy1 | sx2 sy2 q0 q1 | q2 bits rect_x rect_y  and the face's
//                   rectangle of 16 x 16 tiles (the tiles that hold a pixel centre of its closed box: conservative by monotone
//                   rounding, clipped to the image, empty when off-screen).  A face of at most GHR_VIS_BIG_RECT tiles is counted
//                   into each of them; a larger one goes to the view's one BIG list, which every tile walks after its own: the
//                   lists then never hold more than GHR_VIS_BIG_RECT entries per face, whatever the mesh (a workspace sized
//                   from V, F, H, W alone, no read-back), and a tile's work is the faces whose box overlaps it plus the few
//                   faces that span more than GHR_VIS_BIG_RECT tiles.
//                   bits: k = edge k (vertex k -> k + 1) runs against its canonical direction; 3 = never covers; 4 = empty rect;
//                   5 = big.
//   k_vis_scan      one workgroup: exclusive scan of the tile counts -> start [T + 1]; the counts become the fill cursors
//   k_vis_scatter   one thread per face: its id into the lists of its tiles (integer atomics; the order inside a list is free)
//   k_vis_head_mask the dilate-and-threshold, an LDS tile with a 2-pixel halo
//   k_vis_raster    one 256-thread workgroup per tile, one pixel per thread; records staged in LDS GHR_VIS_CHUNK at a time; a
//                   wave none of whose lanes is in a record's box skips it by ballot.  Writes pix_to_face and vis; stores the byte
//                   1 into seen[] / seen_head[] of the winner's three vertices (plain stores of one value: no float atomics)
//   k_vis_accumulate one thread per vertex: the two flags into the int32 counts.
// Everything per element is GHR_HD so that tests/hostsim/ghr_hostsim_visibility.cpp runs the product's own arithmetic on the
// CPU, with a host walk of the same tables in which every index is checked.
#pragma once
#include "ghr_mesh.h"

#define GHR_VIS_TILE 16
#define GHR_VIS_BLOCK 256
#define GHR_VIS_CHUNK 64      // records staged in LDS per round of k_vis_raster
#define GHR_VIS_REC_WORDS 12  // three 16-B units per face
#define GHR_VIS_BIG_RECT 64   // a face of more tiles than this goes to the big list
#define GHR_VIS_NEVER 8u
#define GHR_VIS_EMPTY 16u
#define GHR_VIS_BIG 32u

namespace ghr {

GHR_HD bool vis_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }  // (a NaN fails the comparison)

// One vertex: out = {sx, sy, q, valid ? 1 : 0}.
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
GHR_HD bool vis_pixel_range(float lo, float hi, int n, int* j0, int* j1)
{
    if (!(lo <= (float)n) || !(hi >= 0.f)) return false;
    const float a = lo - 0.5f, b = hi - 0.5f;
    *j0 = a <= 0.f ? 0 : (int)floorf(a);             // (a <= n: the conversion is in range)
    *j1 = b >= (float)(n - 1) ? n - 1 : (int)floorf(b);  // (b >= -0.5: -1 at the least)
    return *j0 <= *j1;
}

// One face: its record from the projected vertices proj [V][4].  t[3] are its indices.
GHR_HD void vis_setup_one(const float* proj, int V, const int32_t* t, int H, int W, float* r)
{
    const bool in_range = t[0] >= 0 && t[0] < V && t[1] >= 0 && t[1] < V && t[2] >= 0 && t[2] < V;
    float p[3][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    if (in_range)
        for (int k = 0; k < 3; k++)
            for (int c = 0; c < 4; c++) p[k][c] = proj[4 * (size_t)t[k] + c];
    bool never = !in_range || t[0] == t[1] || t[1] == t[2] || t[0] == t[2] || p[0][3] == 0.f || p[1][3] == 0.f || p[2][3] == 0.f;
    never = never || mesh_flat(p[0][0], p[0][1], p[1][0], p[1][1], p[2][0], p[2][1]);
    for (int k = 0; k < 3; k++) { r[2 * k] = p[k][0]; r[2 * k + 1] = p[k][1]; r[6 + k] = p[k][2]; }
    uint32_t bits = (t[0] > t[1] ? 1u : 0u) | (t[1] > t[2] ? 2u : 0u) | (t[2] > t[0] ? 4u : 0u) | (never ? GHR_VIS_NEVER : 0u);
    uint32_t rx = 0u, ry = 0u;
    int j0 = 0, j1 = -1, i0 = 0, i1 = -1;
    const float ulo = fminf(fminf(p[0][0], p[1][0]), p[2][0]), uhi = fmaxf(fmaxf(p[0][0], p[1][0]), p[2][0]);
    const float vlo = fminf(fminf(p[0][1], p[1][1]), p[2][1]), vhi = fmaxf(fmaxf(p[0][1], p[1][1]), p[2][1]);
    if (!never && vis_pixel_range(ulo, uhi, W, &j0, &j1) && vis_pixel_range(vlo, vhi, H, &i0, &i1)) {
        const uint32_t x0 = (uint32_t)j0 / GHR_VIS_TILE, x1 = (uint32_t)j1 / GHR_VIS_TILE;
        const uint32_t y0 = (uint32_t)i0 / GHR_VIS_TILE, y1 = (uint32_t)i1 / GHR_VIS_TILE;
        rx = x0 | (x1 << 16);
        ry = y0 | (y1 << 16);
        if ((uint64_t)(x1 - x0 + 1u) * (y1 - y0 + 1u) > GHR_VIS_BIG_RECT) bits |= GHR_VIS_BIG;
    } else {
        bits |= GHR_VIS_EMPTY;
    }
    memcpy(r + 9, &bits, 4);
    memcpy(r + 10, &rx, 4);
    memcpy(r + 11, &ry, 4);
}

// One record against one pixel centre: does the face cover it, and with which inverse depth?
GHR_HD bool vis_in_box(const float* r, float px, float py)
{
    const float ulo = fminf(fminf(r[0], r[2]), r[4]), uhi = fmaxf(fmaxf(r[0], r[2]), r[4]);
    const float vlo = fminf(fminf(r[1], r[3]), r[5]), vhi = fmaxf(fmaxf(r[1], r[3]), r[5]);
    return px >= ulo && px <= uhi && py >= vlo && py <= vhi;
}

GHR_HD bool vis_covers(const float* r, float px, float py, float* inv_depth)
{
    const float u0 = r[0], v0 = r[1], u1 = r[2], v1 = r[3], u2 = r[4], v2 = r[5], q0 = r[6], q1 = r[7], q2 = r[8];
    uint32_t bits;
    memcpy(&bits, r + 9, 4);
    const bool f0 = bits & 1u, f1 = bits & 2u, f2 = bits & 4u;
    bool l0, l1, l2;
    const float E0 = f0 ? mesh_edge(u1, v1, u0, v0, px, py, &l0) : mesh_edge(u0, v0, u1, v1, px, py, &l0);
    const float E1 = f1 ? mesh_edge(u2, v2, u1, v1, px, py, &l1) : mesh_edge(u1, v1, u2, v2, px, py, &l1);
    const float E2 = f2 ? mesh_edge(u0, v0, u2, v2, px, py, &l2) : mesh_edge(u2, v2, u0, v0, px, py, &l2);
    const bool s0 = l0 != f0, s1 = l1 != f1, s2 = l2 != f2;  // left of the triangle's own edge
    if ((bits & GHR_VIS_NEVER) || !vis_in_box(r, px, py) || s0 != s1 || s1 != s2) return false;
    const float e0 = f0 ? -E0 : E0, e1 = f1 ? -E1 : E1, e2 = f2 ? -E2 : E2;
    *inv_depth = ((e1 * q0 + e2 * q1) + e0 * q2) / ((e0 + e1) + e2);
    return true;
}

// The total order of the winner: (inverse depth, lower index).  best starts at (-Inf, -1); a NaN never gets in.
GHR_HD void vis_take(float d, int32_t f, float* best_d, int32_t* best_f)
{
    if (d > *best_d || (d == *best_d && f < *best_f)) { *best_d = d; *best_f = f; }
}

GHR_HD bool vis_head_rule(uint32_t max_body, uint32_t max_hair) { return max_body >= 128u && !(max_hair >= 128u); }

// The head mask at one pixel, from the planes themselves (the kernel reads the same window from its LDS tile).
GHR_HD bool vis_head_one(const uint8_t* body, const uint8_t* hair, int H, int W, int i, int j)
{
    uint32_t mb = 0u, mh = 0u;
    for (int di = -2; di <= 2; di++)
        for (int dj = -2; dj <= 2; dj++) {
            const int y = i + di, x = j + dj;
            if (y < 0 || y >= H || x < 0 || x >= W) continue;
            const size_t o = (size_t)y * W + x;
            mb = body[o] > mb ? body[o] : mb;
            mh = hair[o] > mh ? hair[o] : mh;
        }
    return vis_head_rule(mb, mh);
}

// ---- the workspace ---------------------------------------------------------------------------------------------------------
// Offsets in bytes, 16-B aligned.  [off_fill, off_fill + fill_bytes) is what a view zeroes first: the tile counts, the length of
// the big list and the vertex flags.
struct VisLayout {
    uint64_t off_proj, off_rec, off_start, off_fill, off_count, off_nbig, off_seen, off_seen_head, fill_bytes, off_list, off_big, off_head, bytes;
    uint64_t list_cap;
    int32_t tiles_x, tiles_y;
};

inline const char* vis_layout(int64_t V, int64_t F, int64_t H, int64_t W, VisLayout* L)
{
    if (V < 0 || F < 0 || H < 0 || W < 0) return "negative size";
    if (V > 0x7fffffff || F > 0x7fffffff || H > 0x7fffffff || W > 0x7fffffff) return "a size exceeds 2^31 - 1";
    if ((uint64_t)H * (uint64_t)W > 0x7fffffffull) return "H * W exceeds 32-bit offsets";
    const uint64_t tx = ((uint64_t)W + GHR_VIS_TILE - 1) / GHR_VIS_TILE, ty = ((uint64_t)H + GHR_VIS_TILE - 1) / GHR_VIS_TILE;
    if (tx > 65535 || ty > 65535) return "image too large for 16-bit tile coordinates";
    const uint64_t T = tx * ty;
    const uint64_t per_face = T < GHR_VIS_BIG_RECT ? T : GHR_VIS_BIG_RECT;
    const uint64_t cap = (uint64_t)F * per_face;
    if (cap > 0x7fffffffull) return "the tile lists exceed 32-bit offsets";
    L->tiles_x = (int32_t)tx; L->tiles_y = (int32_t)ty;
    L->list_cap = cap;
    uint64_t off = 0;
    L->off_proj = off; off = mesh_up16(off + 16ull * (uint64_t)V);
    L->off_rec = off; off = mesh_up16(off + 4ull * GHR_VIS_REC_WORDS * (uint64_t)F);
    L->off_start = off; off = mesh_up16(off + 4ull * (T + 1));
    L->off_fill = off;
    L->off_count = off; off = mesh_up16(off + 4ull * T);
    L->off_nbig = off; off += 16;
    L->off_seen = off; off = mesh_up16(off + (uint64_t)V);
    L->off_seen_head = off; off = mesh_up16(off + (uint64_t)V);
    L->fill_bytes = off - L->off_fill;
    L->off_list = off; off = mesh_up16(off + 4ull * cap);
    L->off_big = off; off = mesh_up16(off + 4ull * (uint64_t)F);
    L->off_head = off; off = mesh_up16(off + (uint64_t)H * (uint64_t)W);
    L->bytes = off + 16;  // (never 0: a caller's allocation of `bytes` has an address)
    return nullptr;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
struct VisArgs {
    int32_t V, F, H, W, tiles_x, tiles_y;
    float near;
    float M[12];
    const float* vertices;  // [V][3]
    const int32_t* faces;   // [F][3]
    const uint8_t* head;    // [H][W] 0 / 1, or NULL: head holds nowhere
    float* proj;            // [V][4]
    float* rec;             // [F][12]
    uint32_t* start;        // [T + 1]
    uint32_t* count;        // [T]: counts, then fill cursors
    uint32_t* nbig;
    uint32_t* list;         // [list_cap]
    uint32_t* big;          // [F]
    uint32_t list_cap;
    uint8_t* seen;          // [V]
    uint8_t* seen_head;     // [V]
    int32_t* pix_to_face;   // [H][W]
    uint8_t* vis;           // [H][W] or NULL
    int32_t* cnt;           // [V] or NULL
    int32_t* cnt_head;      // [V] or NULL
};

__global__ void __launch_bounds__(GHR_VIS_BLOCK) k_vis_project(VisArgs a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int64_t v = (int64_t)blockIdx.x * GHR_VIS_BLOCK + threadIdx.x;
    if (v >= a.V) return;
    const float X[3] = {a.vertices[3 * v], a.vertices[3 * v + 1], a.vertices[3 * v + 2]};
    float o[4];
    vis_project_one(a.M, X, a.near, o);
    reinterpret_cast<f4*>(a.proj)[v] = f4{o[0], o[1], o[2], o[3]};
#endif
}

__global__ void __launch_bounds__(GHR_VIS_BLOCK) k_vis_setup(VisArgs a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int64_t f = (int64_t)blockIdx.x * GHR_VIS_BLOCK + threadIdx.x;
    if (f >= a.F) return;
    const int32_t t[3] = {a.faces[3 * f], a.faces[3 * f + 1], a.faces[3 * f + 2]};
    float r[GHR_VIS_REC_WORDS];
    vis_setup_one(a.proj, a.V, t, a.H, a.W, r);
    f4* out = reinterpret_cast<f4*>(a.rec) + 3 * f;
    out[0] = f4{r[0], r[1], r[2], r[3]};
    out[1] = f4{r[4], r[5], r[6], r[7]};
    out[2] = f4{r[8], r[9], r[10], r[11]};
    uint32_t bits, rx, ry;
    memcpy(&bits, r + 9, 4); memcpy(&rx, r + 10, 4); memcpy(&ry, r + 11, 4);
    if (bits & GHR_VIS_EMPTY) return;
    if (bits & GHR_VIS_BIG) {
        const uint32_t pos = atomicAdd(a.nbig, 1u);
        if (pos < (uint32_t)a.F) a.big[pos] = (uint32_t)f;  // (one entry per face at the most: always true)
        return;
    }
    for (uint32_t y = ry & 0xffffu; y <= (ry >> 16); y++)
        for (uint32_t x = rx & 0xffffu; x <= (rx >> 16); x++) atomicAdd(&a.count[y * (uint32_t)a.tiles_x + x], 1u);
#endif
}

// One workgroup.  start[t] = the entries of the tiles before t; count[t] becomes the fill cursor of tile t (= start[t]).
__global__ void __launch_bounds__(GHR_VIS_BLOCK) k_vis_scan(VisArgs a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ uint32_t s_tmp[4];
    const uint32_t T = (uint32_t)a.tiles_x * (uint32_t)a.tiles_y;
    uint32_t run = 0u;
    for (uint32_t base = 0u; base < T; base += GHR_VIS_BLOCK) {
        const uint32_t t = base + threadIdx.x;
        const uint32_t n = t < T ? a.count[t] : 0u;
        uint32_t total;
        const uint32_t before = block_excl_scan_256(n, s_tmp, &total);
        if (t < T) { a.start[t] = run + before; a.count[t] = run + before; }
        run += total;
        __syncthreads();  // s_tmp is written again in the next round
    }
    if (threadIdx.x == 0) a.start[T] = run;
#endif
}

__global__ void __launch_bounds__(GHR_VIS_BLOCK) k_vis_scatter(VisArgs a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int64_t f = (int64_t)blockIdx.x * GHR_VIS_BLOCK + threadIdx.x;
    if (f >= a.F) return;
    const uint32_t* r = reinterpret_cast<const uint32_t*>(a.rec) + (size_t)GHR_VIS_REC_WORDS * f;
    const uint32_t bits = r[9], rx = r[10], ry = r[11];
    if (bits & (GHR_VIS_EMPTY | GHR_VIS_BIG)) return;
    for (uint32_t y = ry & 0xffffu; y <= (ry >> 16); y++)
        for (uint32_t x = rx & 0xffffu; x <= (rx >> 16); x++) {
            const uint32_t pos = atomicAdd(&a.count[y * (uint32_t)a.tiles_x + x], 1u);
            if (pos < a.list_cap) a.list[pos] = (uint32_t)f;  // (at most GHR_VIS_BIG_RECT entries per face: always true)
        }
#endif
}

struct VisHeadArgs {
    int32_t H, W;
    const uint8_t* body;
    const uint8_t* hair;
    uint8_t* head;
};

// One 16 x 16 tile per workgroup; the 20 x 20 window of both planes in LDS, 0 outside the image (0 never raises a maximum).
__global__ void __launch_bounds__(GHR_VIS_BLOCK) k_vis_head_mask(VisHeadArgs a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int S = GHR_VIS_TILE + 4;
    __shared__ uint8_t s_b[S * S], s_h[S * S];
    const int i0 = (int)blockIdx.y * GHR_VIS_TILE - 2, j0 = (int)blockIdx.x * GHR_VIS_TILE - 2;
    for (int k = threadIdx.x; k < S * S; k += GHR_VIS_BLOCK) {
        const int i = i0 + k / S, j = j0 + k % S;
        const bool in = i >= 0 && i < a.H && j >= 0 && j < a.W;
        const size_t o = in ? (size_t)i * a.W + j : 0;
        s_b[k] = in ? a.body[o] : (uint8_t)0;
        s_h[k] = in ? a.hair[o] : (uint8_t)0;
    }
    __syncthreads();
    const int li = threadIdx.x / GHR_VIS_TILE, lj = threadIdx.x % GHR_VIS_TILE;
    const int i = i0 + 2 + li, j = j0 + 2 + lj;
    if (i >= a.H || j >= a.W) return;
    uint32_t mb = 0u, mh = 0u;
#pragma unroll
    for (int di = 0; di < 5; di++)
#pragma unroll
        for (int dj = 0; dj < 5; dj++) {
            const uint32_t b = s_b[(li + di) * S + lj + dj], h = s_h[(li + di) * S + lj + dj];
            mb = b > mb ? b : mb;
            mh = h > mh ? h : mh;
        }
    a.head[(size_t)i * a.W + j] = vis_head_rule(mb, mh) ? 1 : 0;
#endif
}

// One tile per workgroup, one pixel per thread (a wave holds 4 rows of 16 pixels).
__global__ void __launch_bounds__(GHR_VIS_BLOCK) k_vis_raster(VisArgs a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ f4 s_rec[3 * GHR_VIS_CHUNK];
    __shared__ uint32_t s_id[GHR_VIS_CHUNK];
    const uint32_t tile = blockIdx.y * (uint32_t)a.tiles_x + blockIdx.x;
    const int i = (int)blockIdx.y * GHR_VIS_TILE + (int)threadIdx.x / GHR_VIS_TILE;
    const int j = (int)blockIdx.x * GHR_VIS_TILE + (int)threadIdx.x % GHR_VIS_TILE;
    const bool in_image = i < a.H && j < a.W;
    const float px = (float)j + 0.5f, py = (float)i + 0.5f;
    const uint32_t beg = a.start[tile], n_own = a.start[tile + 1] - beg;
    const uint32_t n_big = a.F > 0 ? min(*a.nbig, (uint32_t)a.F) : 0u;
    const uint32_t n = n_own + n_big;  // (workgroup-uniform)
    float best_d = -INFINITY;
    int32_t best_f = -1;
    for (uint32_t c0 = 0u; c0 < n; c0 += GHR_VIS_CHUNK) {
        const uint32_t m = min((uint32_t)GHR_VIS_CHUNK, n - c0);
        if (threadIdx.x < 3u * m) {
            const uint32_t k = threadIdx.x / 3u, part = threadIdx.x % 3u, e = c0 + k;
            // (beg + e < start[T] <= list_cap and every id < F; the clamps keep a workspace that two streams were wrongly
            // given at once from ever indexing outside it)
            uint32_t id = e < n_own ? a.list[min(beg + e, a.list_cap - 1u)] : a.big[e - n_own];
            id = min(id, (uint32_t)a.F - 1u);
            s_rec[3u * k + part] = reinterpret_cast<const f4*>(a.rec)[3 * (size_t)id + part];
            if (part == 0u) s_id[k] = id;
        }
        __syncthreads();
        for (uint32_t k = 0u; k < m; k++) {
            const f4 r0 = s_rec[3u * k], r1 = s_rec[3u * k + 1u], r2 = s_rec[3u * k + 2u];  // (one address per wave: broadcast)
            const float r[GHR_VIS_REC_WORDS] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
            const bool box = in_image && vis_in_box(r, px, py);
            if (__builtin_amdgcn_ballot_w64(box) == 0ull) continue;  // nobody in this wave is inside the box
            float d;
            if (box && vis_covers(r, px, py, &d)) vis_take(d, (int32_t)s_id[k], &best_d, &best_f);
        }
        __syncthreads();
    }
    if (!in_image) return;
    const size_t o = (size_t)i * a.W + j;
    const bool head = a.head && a.head[o];
    a.pix_to_face[o] = best_f;
    if (a.vis) a.vis[o] = (best_f >= 0 && head) ? 255 : 0;
    if (best_f >= 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int32_t v = a.faces[3 * (size_t)best_f + k];  // (a winner's indices were checked by k_vis_setup)
            a.seen[v] = 1;
            if (head) a.seen_head[v] = 1;
        }
    }
#endif
}

__global__ void __launch_bounds__(GHR_VIS_BLOCK) k_vis_accumulate(VisArgs a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int64_t v = (int64_t)blockIdx.x * GHR_VIS_BLOCK + threadIdx.x;
    if (v >= a.V) return;
    a.cnt[v] += a.seen[v];
    a.cnt_head[v] += a.seen_head[v];
#endif
}
#endif  // __HIPCC__

}  // namespace ghr
