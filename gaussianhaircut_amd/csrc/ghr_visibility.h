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
// Per view (ghr_vis_view): the fill, projection, scan and scatter of ghr_tilelists.h (which also owns the tile rectangle and the
// staged walk of a tile's list); the fill also zeroes the vertex flags.  This header's own kernels:
//   k_vis_setup     one thread per face: a 48-B record  sx0 sy0 sx1 sy1 | sx2 sy2 q0 q1 | q2 - xy bits  from its three projected
//                   vertices, then tl_count.  The owner's flags in bits: k = edge k (vertex k -> k + 1) runs against its canonical
//                   direction.  A face of more than GHR_VIS_BIG_RECT tiles goes to the big list.
//   k_vis_head_mask the dilate-and-threshold, an LDS tile with a 2-pixel halo
//   k_vis_raster    tl_walk with GHR_VIS_CHUNK records per round and the winner's total order; writes pix_to_face and vis; stores
//                   the byte 1 into seen[] / seen_head[] of the winner's three vertices (plain stores of one value: no float atomics)
//   k_vis_accumulate one thread per vertex: the two flags into the int32 counts.
// Everything per element is GHR_HD so that tests/hostsim/ghr_hostsim_visibility.cpp runs the product's own arithmetic on the
// CPU, with a host walk of the same tables in which every index is checked.
#pragma once
#include "ghr_tilelists.h"

#define GHR_VIS_TILE GHR_TL_TILE
#define GHR_VIS_BLOCK GHR_TL_BLOCK
#define GHR_VIS_CHUNK 64      // records staged in LDS per round of k_vis_raster
#define GHR_VIS_REC_WORDS 12  // three 16-B units per face
#define GHR_VIS_REC_UNITS (GHR_VIS_REC_WORDS / 4)
#define GHR_VIS_BIG_RECT 64   // a face of more tiles than this goes to the big list

namespace ghr {

// The nine floats of a face's record from its three projected vertices p0, p1, p2 = {sx, sy, q, valid}; t[3] are its indices.
// Returns its flags: the edge directions, and GHR_TL_NEVER for a face that covers no pixel.
GHR_HD uint32_t vis_face_record(const float* p0, const float* p1, const float* p2, const int32_t* t, float* r)
{
    bool never = t[0] == t[1] || t[1] == t[2] || t[0] == t[2] || p0[3] == 0.f || p1[3] == 0.f || p2[3] == 0.f;
    never = never || mesh_flat(p0[0], p0[1], p1[0], p1[1], p2[0], p2[1]);
    r[0] = p0[0]; r[1] = p0[1]; r[2] = p1[0]; r[3] = p1[1]; r[4] = p2[0]; r[5] = p2[1];
    r[6] = p0[2]; r[7] = p1[2]; r[8] = p2[2];
    r[9] = 0.f;
    return (t[0] > t[1] ? 1u : 0u) | (t[1] > t[2] ? 2u : 0u) | (t[2] > t[0] ? 4u : 0u) | (never ? GHR_TL_NEVER : 0u);
}

// One face: its record from the projected vertices proj [V][4].  An index outside 0 .. V - 1 gives three invalid vertices.
GHR_HD void vis_setup_one(const float* proj, int V, const int32_t* t, int H, int W, float* r)
{
    const bool in_range = t[0] >= 0 && t[0] < V && t[1] >= 0 && t[1] < V && t[2] >= 0 && t[2] < V;
    float p[3][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    if (in_range)
        for (int k = 0; k < 3; k++)
            for (int c = 0; c < 4; c++) p[k][c] = proj[4 * (size_t)t[k] + c];
    const uint32_t flags = vis_face_record(p[0], p[1], p[2], t, r);
    const float ulo = fminf(fminf(p[0][0], p[1][0]), p[2][0]), uhi = fmaxf(fmaxf(p[0][0], p[1][0]), p[2][0]);
    const float vlo = fminf(fminf(p[0][1], p[1][1]), p[2][1]), vhi = fmaxf(fmaxf(p[0][1], p[1][1]), p[2][1]);
    tl_rect(flags, ulo, uhi, vlo, vhi, H, W, GHR_VIS_BIG_RECT, r + 10);
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
    memcpy(&bits, r + 11, 4);
    const bool f0 = bits & 1u, f1 = bits & 2u, f2 = bits & 4u;
    bool l0, l1, l2;
    const float E0 = f0 ? mesh_edge(u1, v1, u0, v0, px, py, &l0) : mesh_edge(u0, v0, u1, v1, px, py, &l0);
    const float E1 = f1 ? mesh_edge(u2, v2, u1, v1, px, py, &l1) : mesh_edge(u1, v1, u2, v2, px, py, &l1);
    const float E2 = f2 ? mesh_edge(u0, v0, u2, v2, px, py, &l2) : mesh_edge(u2, v2, u0, v0, px, py, &l2);
    const bool s0 = l0 != f0, s1 = l1 != f1, s2 = l2 != f2;  // left of the triangle's own edge
    if ((bits & GHR_TL_NEVER) || !vis_in_box(r, px, py) || s0 != s1 || s1 != s2) return false;
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
// The tile lists of ghr_tilelists.h, the two vertex flag arrays behind their counters (inside the fill: a view starts them at 0)
// and the head plane.
struct VisLayout : TileListLayout {  // (fill_bytes: with the flags)
    uint64_t off_seen, off_seen_head, off_head, bytes;
};

inline const char* vis_layout(int64_t V, int64_t F, int64_t H, int64_t W, VisLayout* L)
{
    if (const char* why = tl_layout(V, F, H, W, GHR_VIS_REC_UNITS, GHR_VIS_BIG_RECT, L)) return why;
    uint64_t off = L->off_fill + L->fill_bytes;
    L->off_seen = off; off = mesh_up16(off + (uint64_t)V);
    L->off_seen_head = off; off = mesh_up16(off + (uint64_t)V);
    L->fill_bytes = off - L->off_fill;
    L->off_head = off; off = mesh_up16(off + (uint64_t)H * (uint64_t)W);
    L->bytes = off + 16;  // (never 0: a caller's allocation of `bytes` has an address)
    return nullptr;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
struct VisArgs {
    TileLists tl;           // points: the vertices [V][3]
    int32_t V, F, H, W;
    const int32_t* faces;   // [F][3]
    const uint8_t* head;    // [H][W] 0 / 1, or NULL: head holds nowhere
    uint8_t* seen;          // [V]
    uint8_t* seen_head;     // [V]
    int32_t* pix_to_face;   // [H][W]
    uint8_t* vis;           // [H][W] or NULL
    int32_t* cnt;           // [V] or NULL
    int32_t* cnt_head;      // [V] or NULL
};

__global__ void __launch_bounds__(GHR_VIS_BLOCK) k_vis_setup(VisArgs a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int64_t f = (int64_t)blockIdx.x * GHR_VIS_BLOCK + threadIdx.x;
    if (f >= a.F) return;
    const int32_t t[3] = {a.faces[3 * f], a.faces[3 * f + 1], a.faces[3 * f + 2]};
    float r[GHR_VIS_REC_WORDS];
    vis_setup_one(a.tl.proj, a.V, t, a.H, a.W, r);
    f4* out = reinterpret_cast<f4*>(a.tl.rec) + 3 * f;
    out[0] = f4{r[0], r[1], r[2], r[3]};
    out[1] = f4{r[4], r[5], r[6], r[7]};
    out[2] = f4{r[8], r[9], r[10], r[11]};
    tl_count(a.tl, r + 10, (uint32_t)f);
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
    __shared__ f4 s_rec[GHR_VIS_REC_UNITS * GHR_VIS_CHUNK];
    __shared__ uint32_t s_id[GHR_VIS_CHUNK];
    const int i = (int)blockIdx.y * GHR_VIS_TILE + (int)threadIdx.x / GHR_VIS_TILE;
    const int j = (int)blockIdx.x * GHR_VIS_TILE + (int)threadIdx.x % GHR_VIS_TILE;
    const bool in_image = i < a.H && j < a.W;
    const float px = (float)j + 0.5f, py = (float)i + 0.5f;
    float best_d = -INFINITY;
    int32_t best_f = -1;
    tl_walk<GHR_VIS_REC_UNITS, GHR_VIS_CHUNK, true>(
        a.tl, blockIdx.y * (uint32_t)a.tl.tiles_x + blockIdx.x, s_rec, s_id,
        [&](const float* r) { return in_image && vis_in_box(r, px, py); },
        [&](const float* r, const uint32_t& id) {
            float d;
            if (vis_covers(r, px, py, &d)) vis_take(d, (int32_t)id, &best_d, &best_f);
        });
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
