// ghr_mesh.h -- is a point inside a triangle mesh, and the two workloads of the steps between the training stages that ask it
// (DESIGN.md 8g): 12 probes per Gaussian against the head mesh (src/preprocessing/filter_flame_intersections.py:88,109-118)
// and every strand point against it (src/preprocessing/export_strands.py:60-64).  Every call site reads only the SIGN of the
// reference's signed distance, so that is what is computed -- by a definition of our own, exact and reproducible:
//
//   For each axis a cast the ray +a from the query; u = (a + 1) % 3, v = (a + 2) % 3 are the projected coordinates, a the
//   height.  Every projected edge is evaluated ONCE, from its lower to its higher vertex index,
//       E = dx (pv - av) - dy (pu - au),   dx = bu - au, dy = bv - av            (float32, no contraction)
//   the query is LEFT of that canonical edge iff E > 0, or E == 0 and (dy < 0 or (dy == 0 and dx > 0)) -- the side a query
//   displaced by (+eps, +eps^2) would be on.  A triangle that walks the edge the other way takes the complement, so the two
//   triangles of a shared edge see complementary predicates: no ray slips between them, none is counted twice.
//   A triangle COUNTS for a query when it has projected area (its float32 doubled area is not 0 and its three indices
//   differ), the query lies in the closed box of its three projected vertices, and the query is on the same side of its three
//   edges (either winding).  It is CROSSED when it counts and its plane's height over the query,
//       ((e1 h0 + e2 h1) + e0 h2) / ((e0 + e1) + e2),    e_k = the edge value in the triangle's own direction,
//   is strictly greater than the query's.  Odd crossings = inside along that axis; the answer is the majority of the axes
//   (a mesh with an opening, as the head at the neck, still answers for the points two of the three rays get right).
//   A query with a non-finite coordinate or outside the mesh's bounding box is outside and indexes nothing.
//
// The box rule is implied by the side rule in exact arithmetic; stating it makes the grid below EXACT: cell_of() is one
// monotone function for the builder and the query, a triangle is listed in cell_of(box min) .. cell_of(box max), so a triangle
// whose box holds the query is in the query's cell whatever the rounding, and walking one cell's list gives the bits of
// walking all faces (the PyTorch comparator and the numpy model do the latter).
//
// Tables (ghr_mesh_grid_build, host, deterministic: count, scan, fill in face order), one set per axis:
//   records [F][12 words]: u0 v0 u1 v1 | u2 v2 h0 h1 | h2 bits 0 0    bits: k = edge k (vertex k -> k + 1) runs against
//                          its canonical direction; 3 = the triangle never counts
//   start   [G G + 1], list [start[G G]]: CSR of the faces whose projected box overlaps each cell, in face order.
// Everything per element is GHR_HD so that tests/hostsim/ghr_hostsim_mesh.cpp runs the product's own arithmetic on the CPU;
// GHR_MESH_CHECK(cond) is an assert there and nothing in the library.
#pragma once
#if defined(__HIPCC__)
#include "ghr_device.h"
#else
#include <stdint.h>
#define GHR_HD inline
#endif
#include <math.h>
#include <stddef.h>
#include <string.h>

#ifndef GHR_MESH_CHECK
#define GHR_MESH_CHECK(cond) ((void)0)
#endif

#define GHR_MESH_MAGIC 0x4d524847u  // "GHRM"
#define GHR_MESH_REC_WORDS 12       // three 16-B units per (axis, face)
#define GHR_MESH_G_MAX 256
#define GHR_MESH_BLOCK 256
#define GHR_PROBES 12
// pytorch3d's level-0 ico_sphere, which tabulates (0, +-a, +-b) and its cyclic shifts to four digits (quoted from memory: that
// library is not a dependency).  Vertex k: coordinate k / 4 is (k & 1 ? +a : -a), the next one (cyclic) is (k & 2 ? -b : +b),
// the third is 0 -- the order of its table, though the filter (an AND over the twelve) does not depend on it.
#define GHR_ICO_A 0.5257f
#define GHR_ICO_B 0.8507f

namespace ghr {

// The header of the grid blob (== ghr_mesh_grid of include/ghr.h); offsets are in bytes from the blob's start, 16-B aligned.
struct MeshGrid {
    uint32_t magic;
    int32_t G, n_faces, n_vertices;
    float lo[3], hi[3];      // the mesh's bounding box
    float scale[3];          // cells per unit along each WORLD coordinate: G / (hi - lo), 0 for a flat extent
    uint32_t list_total[3];  // entries of each axis' lists
    uint32_t list_max[3];    // longest list of each axis
    uint32_t pad_;
    uint64_t off_rec[3], off_start[3], off_list[3];
    uint64_t bytes;
};

GHR_HD int mesh_cell_of(float x, float lo, float scale, int G)
{
    const float t = (x - lo) * scale;  // monotone in x: one subtraction, one product with a non-negative factor
    if (!(t >= 0.f)) return 0;  // (also a NaN; the callers' x is in the box, so this is rounding at its low end)
    if (t >= (float)G) return G - 1;
    return (int)t;
}

// One edge, canonical direction a -> b.  Returns E; *left as defined above.
GHR_HD float mesh_edge(float au, float av, float bu, float bv, float pu, float pv, bool* left)
{
    const float dx = bu - au, dy = bv - av;
    const float E = dx * (pv - av) - dy * (pu - au);
    *left = E > 0.f || (E == 0.f && (dy < 0.f || (dy == 0.f && dx > 0.f)));
    return E;
}

// "never counts": no projected area.  (The builder sets bit 3 from this and from repeated indices.)
GHR_HD bool mesh_flat(float u0, float v0, float u1, float v1, float u2, float v2)
{
    const float area2 = (u1 - u0) * (v2 - v0) - (v1 - v0) * (u2 - u0);
    return area2 == 0.f;
}

// One record against one projected query: is the triangle crossed by the ray?
GHR_HD bool mesh_crossed(const float* r, float pu, float pv, float ph)
{
    const float u0 = r[0], v0 = r[1], u1 = r[2], v1 = r[3], u2 = r[4], v2 = r[5], h0 = r[6], h1 = r[7], h2 = r[8];
    uint32_t bits;
    memcpy(&bits, r + 9, 4);
    const float ulo = fminf(fminf(u0, u1), u2), uhi = fmaxf(fmaxf(u0, u1), u2);
    const float vlo = fminf(fminf(v0, v1), v2), vhi = fmaxf(fmaxf(v0, v1), v2);
    const bool in_box = pu >= ulo && pu <= uhi && pv >= vlo && pv <= vhi;
    const bool f0 = bits & 1u, f1 = bits & 2u, f2 = bits & 4u;
    bool l0, l1, l2;
    const float E0 = f0 ? mesh_edge(u1, v1, u0, v0, pu, pv, &l0) : mesh_edge(u0, v0, u1, v1, pu, pv, &l0);
    const float E1 = f1 ? mesh_edge(u2, v2, u1, v1, pu, pv, &l1) : mesh_edge(u1, v1, u2, v2, pu, pv, &l1);
    const float E2 = f2 ? mesh_edge(u0, v0, u2, v2, pu, pv, &l2) : mesh_edge(u2, v2, u0, v0, pu, pv, &l2);
    const bool s0 = l0 != f0, s1 = l1 != f1, s2 = l2 != f2;  // left of the triangle's own edge
    if ((bits & 8u) || !in_box || s0 != s1 || s1 != s2) return false;  // (most records of a list end here: no division)
    const float e0 = f0 ? -E0 : E0, e1 = f1 ? -E1 : E1, e2 = f2 ? -E2 : E2;
    const float height = ((e1 * h0 + e2 * h1) + e0 * h2) / ((e0 + e1) + e2);
    return height > ph;
}

// The tables of one blob, as pointers (host or device memory alike).
struct MeshView {
    int G, n_faces;
    float lo[3], hi[3], scale[3];
    const float* rec[3];
    const uint32_t* start[3];
    const uint32_t* list[3];
    uint32_t list_total[3];
};

GHR_HD MeshView mesh_view(const MeshGrid& h, const void* blob)
{
    MeshView m;
    m.G = h.G; m.n_faces = h.n_faces;
    const char* b = static_cast<const char*>(blob);
    for (int i = 0; i < 3; i++) {
        m.lo[i] = h.lo[i]; m.hi[i] = h.hi[i]; m.scale[i] = h.scale[i];
        m.rec[i] = reinterpret_cast<const float*>(b + h.off_rec[i]);
        m.start[i] = reinterpret_cast<const uint32_t*>(b + h.off_start[i]);
        m.list[i] = reinterpret_cast<const uint32_t*>(b + h.off_list[i]);
        m.list_total[i] = h.list_total[i];
    }
    return m;
}

// Crossings of the ray +AXIS from (x, y, z); the caller has checked the query against the bounding box.
template <int AXIS>
GHR_HD uint32_t mesh_axis_crossings(const MeshView& m, float x, float y, float z)
{
    constexpr int U = (AXIS + 1) % 3, V = (AXIS + 2) % 3;
    const float pu = U == 0 ? x : (U == 1 ? y : z), pv = V == 0 ? x : (V == 1 ? y : z);
    const float ph = AXIS == 0 ? x : (AXIS == 1 ? y : z);
    const int cu = mesh_cell_of(pu, m.lo[U], m.scale[U], m.G), cv = mesh_cell_of(pv, m.lo[V], m.scale[V], m.G);
    GHR_MESH_CHECK(cu >= 0 && cu < m.G && cv >= 0 && cv < m.G);
    const int cell = cv * m.G + cu;
    const uint32_t b = m.start[AXIS][cell], e = m.start[AXIS][cell + 1];
    GHR_MESH_CHECK(b <= e && e <= m.list_total[AXIS]);
    uint32_t n = 0;
    for (uint32_t i = b; i < e; i++) {
        const uint32_t f = m.list[AXIS][i];
        GHR_MESH_CHECK(f < (uint32_t)m.n_faces);
#if defined(__HIP_DEVICE_COMPILE__)
        const f4* rp = reinterpret_cast<const f4*>(m.rec[AXIS]) + 3 * (size_t)f;
        const f4 a = rp[0], bq = rp[1], c = rp[2];
        const float r[GHR_MESH_REC_WORDS] = {a.x, a.y, a.z, a.w, bq.x, bq.y, bq.z, bq.w, c.x, c.y, c.z, c.w};
#else
        const float* r = m.rec[AXIS] + (size_t)GHR_MESH_REC_WORDS * f;
#endif
        n += mesh_crossed(r, pu, pv, ph) ? 1u : 0u;
    }
    return n;
}

// One query.  counts[3] (may be NULL) get the crossings per axis (0 for a refused query).  Returns inside.
GHR_HD bool mesh_contains_one(const MeshView& m, float x, float y, float z, uint32_t* counts)
{
    uint32_t c0 = 0, c1 = 0, c2 = 0;
    // (comparisons written so that a NaN fails them; +-Inf and 1e30 fail against the finite box)
    const bool in_box = x >= m.lo[0] && x <= m.hi[0] && y >= m.lo[1] && y <= m.hi[1] && z >= m.lo[2] && z <= m.hi[2];
    if (in_box) {
        c0 = mesh_axis_crossings<0>(m, x, y, z);
        c1 = mesh_axis_crossings<1>(m, x, y, z);
        c2 = mesh_axis_crossings<2>(m, x, y, z);
    }
    if (counts) { counts[0] = c0; counts[1] = c1; counts[2] = c2; }
    return (c0 & 1u) + (c1 & 1u) + (c2 & 1u) >= 2u;
}

// ---- the Gaussian probes -------------------------------------------------------------------------------------------------
// mode 0 (GHR_PROBE_REFERENCE): the script's  v (diag(3 s) Rt) + xyz  with v a row vector and Rt what its build_rotation
//   returns -- the TRANSPOSE of the rotation matrix R of the normalised quaternion (general_utils.py:100-108).  Component j is
//   sum_i v_i (3 s_i) R[j][i]: the point R diag(3 s) v + xyz of the 3-sigma ellipsoid.
// mode 1 (GHR_PROBE_AXIS_SCALED): (3 s_j) (Rt v)_j + xyz_j -- the inverse rotation first, then a scale along the world axes.
GHR_HD void mesh_ico_vertex(int k, float* v)
{
    const int g = k >> 2;
    const float sa = (k & 1) ? GHR_ICO_A : -GHR_ICO_A, sb = (k & 2) ? -GHR_ICO_B : GHR_ICO_B;
    v[0] = g == 0 ? sa : (g == 2 ? sb : 0.f);
    v[1] = g == 1 ? sa : (g == 0 ? sb : 0.f);
    v[2] = g == 2 ? sa : (g == 1 ? sb : 0.f);
}

GHR_HD void mesh_probe_point(int mode, int k, const float* xyz, const float* s, const float* rot, float* p)
{
    const float n = sqrtf(((rot[0] * rot[0] + rot[1] * rot[1]) + rot[2] * rot[2]) + rot[3] * rot[3]);
    const float w = rot[0] / n, x = rot[1] / n, y = rot[2] / n, z = rot[3] / n;
    // R[j][i], the rotation matrix (the expressions of build_rotation, which stores them transposed)
    const float R00 = 1.f - 2.f * (y * y + z * z), R01 = 2.f * (x * y - w * z), R02 = 2.f * (x * z + w * y);
    const float R10 = 2.f * (x * y + w * z), R11 = 1.f - 2.f * (x * x + z * z), R12 = 2.f * (y * z - w * x);
    const float R20 = 2.f * (x * z - w * y), R21 = 2.f * (y * z + w * x), R22 = 1.f - 2.f * (x * x + y * y);
    const float s0 = s[0] * 3.f, s1 = s[1] * 3.f, s2 = s[2] * 3.f;
    float v[3];
    mesh_ico_vertex(k, v);
    if (mode == 0) {
        p[0] = ((v[0] * (s0 * R00) + v[1] * (s1 * R01)) + v[2] * (s2 * R02)) + xyz[0];
        p[1] = ((v[0] * (s0 * R10) + v[1] * (s1 * R11)) + v[2] * (s2 * R12)) + xyz[1];
        p[2] = ((v[0] * (s0 * R20) + v[1] * (s1 * R21)) + v[2] * (s2 * R22)) + xyz[2];
    } else {
        p[0] = s0 * ((v[0] * R00 + v[1] * R10) + v[2] * R20) + xyz[0];
        p[1] = s1 * ((v[0] * R01 + v[1] * R11) + v[2] * R21) + xyz[1];
        p[2] = s2 * ((v[0] * R02 + v[1] * R12) + v[2] * R22) + xyz[2];
    }
}

// One Gaussian: are all twelve probes outside?  (The kernel gives one probe to a lane and ANDs by ballot.)
GHR_HD bool mesh_probes_outside_one(const MeshView& m, int mode, const float* xyz, const float* s, const float* rot)
{
    bool all_out = true;
    for (int k = 0; k < GHR_PROBES; k++) {
        float p[3];
        mesh_probe_point(mode, k, xyz, s, rot, p);
        all_out = all_out && !mesh_contains_one(m, p[0], p[1], p[2], nullptr);
    }
    return all_out;
}

// ---- the builder (host) --------------------------------------------------------------------------------------------------
inline int mesh_default_G(int n_faces)
{
    int g = (int)ceil(sqrt((double)(n_faces > 0 ? n_faces : 1)));  // about one cell per face and axis
    return g < 1 ? 1 : (g > GHR_MESH_G_MAX ? GHR_MESH_G_MAX : g);
}

inline size_t mesh_up16(size_t x) { return (x + 15) / 16 * 16; }

// Validates the mesh and sizes the blob: fills every field of *h (the offsets included).  Returns NULL or what is wrong.
// The count pass of the build: the fill pass below walks the faces in the same order with the same cell ranges.
inline const char* mesh_grid_plan(int n_vertices, const float* vertices, int n_faces, const int32_t* faces, int G, MeshGrid* h)
{
    if (n_vertices < 0 || n_faces < 0) return "negative count";
    if (G < 0 || G > GHR_MESH_G_MAX) return "G outside 0 (default) .. 256";
    if ((n_vertices && !vertices) || (n_faces && !faces)) return "NULL vertices or faces";
    memset(h, 0, sizeof(*h));
    h->magic = GHR_MESH_MAGIC;
    h->G = G ? G : mesh_default_G(n_faces);
    h->n_faces = n_faces; h->n_vertices = n_vertices;
    for (size_t i = 0; i < 3 * (size_t)n_vertices; i++)
        if (!(fabsf(vertices[i]) <= 3.0e38f)) return "a vertex coordinate is not finite";
    for (size_t i = 0; i < 3 * (size_t)n_faces; i++)
        if (faces[i] < 0 || faces[i] >= n_vertices) return "a face index is outside the vertices";
    // the box of the vertices that faces use; an empty mesh gets an empty box (lo > hi: every query is outside)
    for (int c = 0; c < 3; c++) { h->lo[c] = 1.f; h->hi[c] = -1.f; }
    for (size_t i = 0; i < 3 * (size_t)n_faces; i++)
        for (int c = 0; c < 3; c++) {
            const float x = vertices[3 * (size_t)faces[i] + c];
            if (i == 0) { h->lo[c] = x; h->hi[c] = x; }
            h->lo[c] = fminf(h->lo[c], x); h->hi[c] = fmaxf(h->hi[c], x);
        }
    for (int c = 0; c < 3; c++) {
        const float ext = h->hi[c] - h->lo[c];
        h->scale[c] = ext > 0.f ? (float)h->G / ext : 0.f;
        if (!(h->scale[c] <= 3.0e38f)) h->scale[c] = 0.f;  // an extent so small that G / ext overflows: one cell
    }
    const size_t cells = (size_t)h->G * h->G;
    size_t off = mesh_up16(sizeof(MeshGrid));
    for (int a = 0; a < 3; a++) {
        const int U = (a + 1) % 3, V = (a + 2) % 3;
        uint64_t total = 0;
        for (int f = 0; f < n_faces; f++) {
            const int32_t* t = faces + 3 * (size_t)f;
            const float* p0 = vertices + 3 * (size_t)t[0];
            const float* p1 = vertices + 3 * (size_t)t[1];
            const float* p2 = vertices + 3 * (size_t)t[2];
            if (t[0] == t[1] || t[1] == t[2] || t[0] == t[2] || mesh_flat(p0[U], p0[V], p1[U], p1[V], p2[U], p2[V])) continue;
            const int cu0 = mesh_cell_of(fminf(fminf(p0[U], p1[U]), p2[U]), h->lo[U], h->scale[U], h->G);
            const int cu1 = mesh_cell_of(fmaxf(fmaxf(p0[U], p1[U]), p2[U]), h->lo[U], h->scale[U], h->G);
            const int cv0 = mesh_cell_of(fminf(fminf(p0[V], p1[V]), p2[V]), h->lo[V], h->scale[V], h->G);
            const int cv1 = mesh_cell_of(fmaxf(fmaxf(p0[V], p1[V]), p2[V]), h->lo[V], h->scale[V], h->G);
            total += (uint64_t)(cu1 - cu0 + 1) * (uint64_t)(cv1 - cv0 + 1);
        }
        if (total > 0x7fffffffu) return "the cell lists exceed 2^31 entries";
        h->list_total[a] = (uint32_t)total;
        h->off_rec[a] = off; off = mesh_up16(off + sizeof(float) * GHR_MESH_REC_WORDS * (size_t)n_faces);
        h->off_start[a] = off; off = mesh_up16(off + sizeof(uint32_t) * (cells + 1));
        h->off_list[a] = off; off = mesh_up16(off + sizeof(uint32_t) * (size_t)total);
    }
    h->bytes = off;
    return nullptr;
}

// Fills a blob of plan.bytes bytes (16-B aligned).  Returns NULL or what is wrong.
inline const char* mesh_grid_fill(const float* vertices, const int32_t* faces, const MeshGrid& plan, void* blob)
{
    MeshGrid h = plan;
    char* out = static_cast<char*>(blob);
    memset(out, 0, (size_t)h.bytes);
    const int G = h.G, F = h.n_faces;
    const size_t cells = (size_t)G * G;
    for (int a = 0; a < 3; a++) {
        const int U = (a + 1) % 3, V = (a + 2) % 3;
        float* rec = reinterpret_cast<float*>(out + h.off_rec[a]);
        uint32_t* start = reinterpret_cast<uint32_t*>(out + h.off_start[a]);
        uint32_t* list = reinterpret_cast<uint32_t*>(out + h.off_list[a]);
        // records, and the counts (in start[cell + 1])
        for (int pass = 0; pass < 2; pass++) {
            for (int f = 0; f < F; f++) {
                const int32_t* t = faces + 3 * (size_t)f;
                const float* p[3] = {vertices + 3 * (size_t)t[0], vertices + 3 * (size_t)t[1], vertices + 3 * (size_t)t[2]};
                const bool never = t[0] == t[1] || t[1] == t[2] || t[0] == t[2] ||
                                   mesh_flat(p[0][U], p[0][V], p[1][U], p[1][V], p[2][U], p[2][V]);
                if (pass == 0) {
                    float* r = rec + (size_t)GHR_MESH_REC_WORDS * f;
                    for (int k = 0; k < 3; k++) { r[2 * k] = p[k][U]; r[2 * k + 1] = p[k][V]; r[6 + k] = p[k][a]; }
                    const uint32_t bits = (t[0] > t[1] ? 1u : 0u) | (t[1] > t[2] ? 2u : 0u) | (t[2] > t[0] ? 4u : 0u) | (never ? 8u : 0u);
                    memcpy(r + 9, &bits, 4);
                }
                if (never) continue;
                const int cu0 = mesh_cell_of(fminf(fminf(p[0][U], p[1][U]), p[2][U]), h.lo[U], h.scale[U], G);
                const int cu1 = mesh_cell_of(fmaxf(fmaxf(p[0][U], p[1][U]), p[2][U]), h.lo[U], h.scale[U], G);
                const int cv0 = mesh_cell_of(fminf(fminf(p[0][V], p[1][V]), p[2][V]), h.lo[V], h.scale[V], G);
                const int cv1 = mesh_cell_of(fmaxf(fmaxf(p[0][V], p[1][V]), p[2][V]), h.lo[V], h.scale[V], G);
                for (int cv = cv0; cv <= cv1; cv++)
                    for (int cu = cu0; cu <= cu1; cu++) {
                        const size_t cell = (size_t)cv * G + cu;
                        GHR_MESH_CHECK(cell < cells);
                        if (pass == 0) start[cell + 1]++;
                        else {
                            // (pass 1: start[cell + 1] is the cursor of `cell`, see below)
                            GHR_MESH_CHECK(start[cell + 1] < h.list_total[a]);
                            list[start[cell + 1]++] = (uint32_t)f;
                        }
                    }
            }
            if (pass == 0) {
                // exclusive scan, kept one slot to the right: after it start[c + 1] is where list c BEGINS, and the fill moves
                // it to where list c ends = where list c + 1 begins -- the finished table, with start[0] = 0
                uint32_t run = 0, longest = 0;
                for (size_t c = 0; c < cells; c++) {
                    const uint32_t n = start[c + 1];
                    longest = n > longest ? n : longest;
                    start[c + 1] = run;
                    run += n;
                }
                if (run != h.list_total[a]) return "the count pass and the plan disagree";
                h.list_max[a] = longest;
            }
        }
        if (start[cells] != h.list_total[a]) return "the fill pass and the plan disagree";
    }
    memcpy(out, &h, sizeof(h));
    return nullptr;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
struct MeshQueryArgs {
    MeshView m;
    int64_t Q;
    const float* points;  // [Q][3]
    uint8_t* inside;      // [Q]
    uint32_t* crossings;  // [Q][3] or NULL
};

// One thread per query.  The lists and records of a ~10 k-face mesh are a few MB: they stay in L2, the gathers are per lane.
__global__ void __launch_bounds__(GHR_MESH_BLOCK) k_mesh_contains(MeshQueryArgs a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int64_t q = (int64_t)blockIdx.x * GHR_MESH_BLOCK + threadIdx.x;
    if (q >= a.Q) return;
    const float x = a.points[3 * q], y = a.points[3 * q + 1], z = a.points[3 * q + 2];
    uint32_t c[3];
    a.inside[q] = mesh_contains_one(a.m, x, y, z, c) ? 1 : 0;
    if (a.crossings) { a.crossings[3 * q] = c[0]; a.crossings[3 * q + 1] = c[1]; a.crossings[3 * q + 2] = c[2]; }
#endif
}

struct MeshProbeArgs {
    MeshView m;
    int64_t P;
    int mode;
    const float* xyz;       // [P][3]
    const float* scaling;   // [P][3] activated
    const float* rotation;  // [P][4] raw
    uint8_t* outside;       // [P]: all twelve probes outside
};

// One 16-lane row per Gaussian (4 per wave, 16 per workgroup), lanes 0-11 one probe each; the probes live in registers only:
// 40 B read and 1 B written per Gaussian.  The row's AND is taken from the wave's ballot.
__global__ void __launch_bounds__(GHR_MESH_BLOCK) k_gaussian_probe_outside(MeshProbeArgs a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int lane = threadIdx.x & 63, row = lane >> 4, k = lane & 15;
    const int64_t g = ((int64_t)blockIdx.x * GHR_MESH_BLOCK + threadIdx.x) >> 4;
    bool inside = false;
    if (g < a.P && k < GHR_PROBES) {
        const float xyz[3] = {a.xyz[3 * g], a.xyz[3 * g + 1], a.xyz[3 * g + 2]};
        const float s[3] = {a.scaling[3 * g], a.scaling[3 * g + 1], a.scaling[3 * g + 2]};
        const float r[4] = {a.rotation[4 * g], a.rotation[4 * g + 1], a.rotation[4 * g + 2], a.rotation[4 * g + 3]};
        float p[3];
        mesh_probe_point(a.mode, k, xyz, s, r, p);
        inside = mesh_contains_one(a.m, p[0], p[1], p[2], nullptr);
    }
    const unsigned long long any_inside = __builtin_amdgcn_ballot_w64(inside);  // every lane of the wave arrives here
    if (g < a.P && k == 0) a.outside[g] = ((any_inside >> (16 * row)) & 0xffffull) == 0 ? 1 : 0;
#endif
}
#endif  // __HIPCC__

}  // namespace ghr
