// ghr_hostsim_mesh.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Compiles gaussianhaircut_amd/csrc/ghr_mesh.h as plain C++ for the host: the grid builder (host code in the product too) and
// the per-element functions the two kernels call, run query by query.  Every index the walk forms is checked
// (GHR_MESH_CHECK aborts with the expression), and the finished tables are verified entry by entry by ghrsim_mesh_verify.
// tests/test_mesh_cpu.py loads this as a shared library; ghr_mesh_selfcheck.cpp includes it and adds a main().
#include <cstdio>
#include <cstdlib>
#include <cstring>
#define GHR_MESH_CHECK(cond)                                                                 \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            std::fprintf(stderr, "ghr_mesh.h:%d: check failed: %s\n", __LINE__, #cond);      \
            std::abort();                                                                    \
        }                                                                                    \
    } while (0)
#include "../../gaussianhaircut_amd/csrc/ghr_mesh.h"

extern "C" {

int ghrsim_mesh_header_bytes(void) { return (int)sizeof(ghr::MeshGrid); }

// 0, or -1 with the reason in why[128]
int ghrsim_mesh_sizes(int nv, const float* v, int nf, const int32_t* f, int G, ghr::MeshGrid* h, char* why)
{
    const char* w = ghr::mesh_grid_plan(nv, v, nf, f, G, h);
    if (w) std::snprintf(why, 128, "%s", w);
    return w ? -1 : 0;
}

int ghrsim_mesh_build(int nv, const float* v, int nf, const int32_t* f, int G, void* blob, unsigned long long bytes, char* why)
{
    ghr::MeshGrid plan;
    const char* w = ghr::mesh_grid_plan(nv, v, nf, f, G, &plan);
    if (!w && plan.bytes != bytes) w = "bytes";
    if (!w) w = ghr::mesh_grid_fill(v, f, plan, blob);
    if (w) std::snprintf(why, 128, "%s", w);
    return w ? -1 : 0;
}

// The finished tables against their specification, without the builder's code: start is a non-decreasing scan from 0 to
// list_total, every list is strictly increasing (face order, no duplicates) and in range, and face f is in the list of cell
// (cu, cv) exactly when it can count and the cell lies in cell_of(its box).  Returns 0 or the line of the first failure.
int ghrsim_mesh_verify(const float* v, const int32_t* f, const void* blob)
{
    ghr::MeshGrid h;
    std::memcpy(&h, blob, sizeof(h));
    if (h.magic != GHR_MESH_MAGIC || h.G < 1 || h.G > GHR_MESH_G_MAX) return __LINE__;
    const ghr::MeshView m = ghr::mesh_view(h, blob);
    const size_t cells = (size_t)h.G * h.G;
    for (int a = 0; a < 3; a++) {
        const int U = (a + 1) % 3, V = (a + 2) % 3;
        if (m.start[a][0] != 0 || m.start[a][cells] != h.list_total[a]) return __LINE__;
        uint32_t longest = 0;
        for (size_t c = 0; c < cells; c++) {
            if (m.start[a][c] > m.start[a][c + 1]) return __LINE__;
            const uint32_t n = m.start[a][c + 1] - m.start[a][c];
            longest = n > longest ? n : longest;
        }
        if (longest != h.list_max[a]) return __LINE__;
        for (int face = 0; face < h.n_faces; face++) {
            const int32_t* t = f + 3 * (size_t)face;
            const float* p[3] = {v + 3 * (size_t)t[0], v + 3 * (size_t)t[1], v + 3 * (size_t)t[2]};
            const float* r = m.rec[a] + (size_t)GHR_MESH_REC_WORDS * face;
            uint32_t bits;
            std::memcpy(&bits, r + 9, 4);
            for (int k = 0; k < 3; k++) {
                if (r[2 * k] != p[k][U] || r[2 * k + 1] != p[k][V] || r[6 + k] != p[k][a]) return __LINE__;
                if (((bits >> k) & 1u) != (t[k] > t[(k + 1) % 3] ? 1u : 0u)) return __LINE__;
            }
            const bool never = t[0] == t[1] || t[1] == t[2] || t[0] == t[2] ||
                               ghr::mesh_flat(p[0][U], p[0][V], p[1][U], p[1][V], p[2][U], p[2][V]);
            if (((bits >> 3) & 1u) != (never ? 1u : 0u) || (bits >> 4)) return __LINE__;
            float ulo = p[0][U], uhi = p[0][U], vlo = p[0][V], vhi = p[0][V];
            for (int k = 1; k < 3; k++) {
                ulo = fminf(ulo, p[k][U]); uhi = fmaxf(uhi, p[k][U]); vlo = fminf(vlo, p[k][V]); vhi = fmaxf(vhi, p[k][V]);
            }
            const int cu0 = ghr::mesh_cell_of(ulo, h.lo[U], h.scale[U], h.G), cu1 = ghr::mesh_cell_of(uhi, h.lo[U], h.scale[U], h.G);
            const int cv0 = ghr::mesh_cell_of(vlo, h.lo[V], h.scale[V], h.G), cv1 = ghr::mesh_cell_of(vhi, h.lo[V], h.scale[V], h.G);
            for (size_t c = 0; c < cells; c++) {
                const int cu = (int)(c % h.G), cv = (int)(c / h.G);
                bool in = false;
                for (uint32_t i = m.start[a][c]; i < m.start[a][c + 1]; i++) {
                    if (m.list[a][i] >= (uint32_t)h.n_faces) return __LINE__;
                    if (i > m.start[a][c] && m.list[a][i] <= m.list[a][i - 1]) return __LINE__;
                    in = in || m.list[a][i] == (uint32_t)face;
                }
                if (in != (!never && cu >= cu0 && cu <= cu1 && cv >= cv0 && cv <= cv1)) return __LINE__;
            }
        }
    }
    return 0;
}

// length of the list of cell (cu, cv) of `axis`
int ghrsim_mesh_list_length(const void* blob, int axis, int cu, int cv)
{
    ghr::MeshGrid h;
    std::memcpy(&h, blob, sizeof(h));
    const ghr::MeshView m = ghr::mesh_view(h, blob);
    GHR_MESH_CHECK(axis >= 0 && axis < 3 && cu >= 0 && cu < h.G && cv >= 0 && cv < h.G);
    const size_t c = (size_t)cv * h.G + cu;
    return (int)(m.start[axis][c + 1] - m.start[axis][c]);
}

// k_mesh_contains, query by query
void ghrsim_mesh_contains(const void* blob, long long Q, const float* points, uint8_t* inside, uint32_t* crossings)
{
    ghr::MeshGrid h;
    std::memcpy(&h, blob, sizeof(h));
    const ghr::MeshView m = ghr::mesh_view(h, blob);
    for (long long q = 0; q < Q; q++)
        inside[q] = ghr::mesh_contains_one(m, points[3 * q], points[3 * q + 1], points[3 * q + 2], crossings ? crossings + 3 * q : nullptr);
}

// the probes of k_gaussian_probe_outside: points [P][12][3]
void ghrsim_mesh_probe_points(long long P, const float* xyz, const float* scaling, const float* rotation, int mode, float* points)
{
    for (long long g = 0; g < P; g++)
        for (int k = 0; k < GHR_PROBES; k++)
            ghr::mesh_probe_point(mode, k, xyz + 3 * g, scaling + 3 * g, rotation + 4 * g, points + 3 * (GHR_PROBES * g + k));
}

// k_gaussian_probe_outside, Gaussian by Gaussian
void ghrsim_mesh_probes_outside(const void* blob, long long P, const float* xyz, const float* scaling, const float* rotation,
                                int mode, uint8_t* outside)
{
    ghr::MeshGrid h;
    std::memcpy(&h, blob, sizeof(h));
    const ghr::MeshView m = ghr::mesh_view(h, blob);
    for (long long g = 0; g < P; g++)
        outside[g] = ghr::mesh_probes_outside_one(m, mode, xyz + 3 * g, scaling + 3 * g, rotation + 4 * g);
}

}  // extern "C"
