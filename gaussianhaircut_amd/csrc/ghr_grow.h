// ghr_grow.h -- strands grown AROUND the head: ghr_field.h's trace with the head mesh asked at every step (strand_growing.py;
// DESIGN.md 8t).  There is no counterpart in the reference; this header is the definition, and every form (this kernel,
// tests/hostsim/ghr_hostsim_grow.cpp's walk of it, strand_growing.py's composed form, tests/grow_cases.py's float64 arbiter) is
// held to it.  It extends ghr_field.h's trace and changes none of it.
//
// All arithmetic is fp32, without contraction, in the order written; sqrtf and / are IEEE.
//
// Inputs beside the trace's: a head mesh as its two blobs -- ghr_meshdist.h's triangle tables (the closest point) and ghr_mesh.h's
// grids (the containment) -- and a margin m > 0.
//
// The guarded trace of strand s: the state and the loop of ghr_field.h's trace, with contacts = 0 and stop = 0 beside them.  Per
// step the heading update is that trace's (field_strand_heading: support, blend, coast, C, R; a strand whose coast exceeds
// max_coast stops with stop = 1 and appends no point).  Then, where that trace sets x += h t:
//     y = x + h t                                                  (per component, that trace's expression)
//     (d2, face, c) = the closest point of y by ghr_meshdist.h's definition;  in = mesh_contains_one(y)  (ghr_mesh.h)
//     a y with a non-finite coordinate has d2 = +inf, in = false (both by those definitions)
//     d = sqrtf(d2);  sd = in ? -d : d
//     FREE iff !(sd < m):  x = y
//     CONTACT otherwise:
//         d2 == 0:  no correction, x = y, t unchanged (the next step sees the strand inside or free)
//         otherwise  u_k = (y_k - c_k) / d;  n = in ? -u : u;  tn = (t.x*n.x + t.y*n.y) + t.z*n.z
//             if tn < 0:  s_k = t_k - tn*n_k;  l = field_len(s)
//                 if l <= 1e-4:  the strand stops HEAD-ON: stop = 2, not live, no point appended (as a coast stop)
//                 else  t_k = s_k / l                              (the heading slides along the surface)
//             x_k = c_k + m*n_k                                     (one projection, not iterated)
//         contacts += 1                                             (every contact step that appends a point, d2 == 0 included)
//     path[rows++] = x;  if supported: steps = rows - 1             (a supported step sets steps, contact or not)
// Outputs beside path, steps, rgb (ghr_field.h's): contacts [S] int32; stop [S] uint8: 0 ran out of M, 1 coast, 2 head-on.
//
// The bits of a strand depend on the cloud, the mesh and the strand alone -- not on the wave's other strands, the root order, the
// seed block of the mesh search or the launch: ghr_meshdist.h guarantees it for (d2, face, c) (a total order), ghr_mesh.h for in,
// ghr_field.h for the field (every wave walks the cloud's blocks in ascending order).
// On a convex mesh a pushed point lies at distance m from c, and c stays its closest point.  Nothing is promised in concavities,
// and there is no tunnelling check: the caller keeps h below the head's features.
//
// The kernel (k_grow_guarded): one strand per lane, one wave per 64 roots in root_order, GHR_FIELD_WAVES waves per workgroup; the
// wave loops over the steps and per step takes, for its live lanes, the field walk (knn_walk + FieldGather), the mesh search
// (md_wave_search) and the containment (mesh_contains_one, per lane).  The two walks never overlap in time and share the wave's one
// LDS tile of 3 * 64 float4 (knn_wave_lds_fence between them): 12 KiB per workgroup, as k_field_trace.  A lane that is not live, or
// whose y is not finite, votes in no ballot of the search.  The search's seed block is the block md_seed_block finds for the key
// of the y of the wave's lowest searching lane: the results do not depend on it, a block near one of the wave's queries gives every
// lane near it a tight bound from the first scan on, and one lane's key costs no sort.  The strand's state stays in registers.  No
// floating-point atomics.  Per-element functions are GHR_HD: the host walks them.
#pragma once
#include "ghr_field.h"
#include "ghr_meshdist.h"

#define GHR_GROW_HEADON_EPS 1e-4f
#define GHR_GROW_STOP_STEPS 0  // ran out of M
#define GHR_GROW_STOP_COAST 1
#define GHR_GROW_STOP_HEADON 2

namespace ghr {

// One guarded strand's state: ghr_field.h's, the contact steps so far and why the strand stopped.
struct GrowStrand {
    FieldStrand f;
    int contacts, stop;
};

GHR_HD void grow_strand_init(GrowStrand& s, const float* o, const float* nrm)
{
    field_strand_init(s.f, o, nrm);
    s.contacts = 0;
    s.stop = GHR_GROW_STOP_STEPS;
}

// The guard of one step, after field_strand_heading: y = x + h t was asked of the mesh, (d2, c) is its closest point and `in` its
// containment.  Returns whether a point was appended (it is s.f.x then); a strand that stops head-on appends none and is not live
// afterwards.  The kernel, the host walk and nothing else call it.
GHR_HD bool grow_guard_step(GrowStrand& s, const float* y, float d2, const float* c, bool in, bool supported, float margin)
{
    FieldStrand& f = s.f;
    const float d = sqrtf(d2);
    const float sd = in ? -d : d;
    float x0 = y[0], x1 = y[1], x2 = y[2];
    if (sd < margin) {
        if (!(d2 == 0.f)) {
            const float u0 = (y[0] - c[0]) / d, u1 = (y[1] - c[1]) / d, u2 = (y[2] - c[2]) / d;
            const float n0 = in ? -u0 : u0, n1 = in ? -u1 : u1, n2 = in ? -u2 : u2;
            const float tn = (f.t[0] * n0 + f.t[1] * n1) + f.t[2] * n2;
            if (tn < 0.f) {
                const float s0 = f.t[0] - tn * n0, s1 = f.t[1] - tn * n1, s2 = f.t[2] - tn * n2;
                const float l = field_len(s0, s1, s2);
                if (l <= GHR_GROW_HEADON_EPS) {
                    f.live = false;
                    s.stop = GHR_GROW_STOP_HEADON;
                    return false;
                }
                f.t[0] = s0 / l; f.t[1] = s1 / l; f.t[2] = s2 / l;
            }
            x0 = c[0] + margin * n0; x1 = c[1] + margin * n1; x2 = c[2] + margin * n2;
        }
        s.contacts += 1;
    }
    f.x[0] = x0; f.x[1] = x1; f.x[2] = x2;
    f.rows += 1;
    if (supported) f.steps = f.rows - 1;
    return true;
}

#if defined(__HIPCC__)
struct GrowArgs {
    KnnCloud c;
    FieldPayload pay;
    MdView md;
    float md_bounds[6];  // the triangle blob's lo, hi: the bounds of the seed block's key
    MeshView mesh;
    FieldTraceArgs a;
    float margin;
    int S;
    const float *roots, *normals;    // [S][3]
    const long long* order;          // [S] or NULL (the roots' key order: a wave's strands stay near each other)
    float* path;                     // [S][M+1][3]
    int* steps;                      // [S]
    float* rgb;                      // [S][3]
    int* contacts;                   // [S]
    unsigned char* stop;             // [S]
};

__global__ void __launch_bounds__(64 * GHR_FIELD_WAVES) k_grow_guarded(GrowArgs g)
{
    __shared__ float4 tiles[GHR_FIELD_WAVES][3 * GHR_KNN_BLOCK];  // one tile per wave, shared by the field walk and the mesh search
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long s0 = ((long long)blockIdx.x * GHR_FIELD_WAVES + wave) * GHR_KNN_BLOCK;
    if (s0 >= g.S) return;
    const FieldTraceArgs& a = g.a;
    const bool mine = s0 + lane < g.S;
    const size_t row = (size_t)field_row(g.order, mine ? s0 + lane : s0, g.S);
    GrowStrand st;
    grow_strand_init(st, g.roots + row * 3, g.normals + row * 3);
    st.f.live = mine;
    float* out = g.path + row * (size_t)(a.M + 1) * 3;
    if (mine)
        for (int k = 0; k < 3; ++k) out[k] = st.f.x[k];
    for (int j = 0; j < a.M; ++j) {
        if (!__any(st.f.live)) break;
        FieldGather fg(a.r2, st.f.t[0], st.f.t[1], st.f.t[2], g.pay, tiles[wave] + GHR_KNN_BLOCK);
        knn_walk(g.c, tiles[wave], make_float3(st.f.x[0], st.f.x[1], st.f.x[2]), st.f.live, 0, -1, fg);
        const bool was = st.f.live;
        const int how = was ? field_strand_heading(st.f, fg, a) : FIELD_STOPPED;
        if (was && how == FIELD_STOPPED) st.stop = GHR_GROW_STOP_COAST;
        const float y[3] = {st.f.x[0] + a.h * st.f.t[0], st.f.x[1] + a.h * st.f.t[1], st.f.x[2] + a.h * st.f.t[2]};
        const bool asks = st.f.live && md_finite(y[0]) && md_finite(y[1]) && md_finite(y[2]);
        const unsigned long long askers = __ballot(asks);
        MdNearest near;
        bool in = false;
        if (askers) {
            const unsigned long long key = knn_key(y, g.md_bounds);
            const int src = __ffsll(askers) - 1;  // the lowest searching lane: its key finds the seed block
            const unsigned klo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)key, src);
            const unsigned khi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(key >> 32), src);
            const int seed = md_seed_block(g.md.bkeys, g.md.n_blocks, ((unsigned long long)khi << 32) | klo);
            knn_wave_lds_fence();  // the field walk is done with the tile
            md_wave_search(g.md, tiles[wave], MdVec{y[0], y[1], y[2]}, asks, seed, near);
            knn_wave_lds_fence();
            if (asks) in = mesh_contains_one(g.mesh, y[0], y[1], y[2], nullptr);
        }
        if (st.f.live) {
            const float c[3] = {near.point.x, near.point.y, near.point.z};
            if (grow_guard_step(st, y, asks ? near.best : __builtin_inff(), c, in, how == FIELD_SUPPORTED, g.margin))
                for (int k = 0; k < 3; ++k) out[(size_t)(st.f.rows - 1) * 3 + k] = st.f.x[k];
        }
    }
    if (mine) {
        for (int r = st.f.rows; r <= a.M; ++r)
            for (int k = 0; k < 3; ++k) out[(size_t)r * 3 + k] = st.f.x[k];
        g.steps[row] = st.f.steps;
        field_strand_rgb(st.f, g.rgb + row * 3);
        g.contacts[row] = st.contacts;
        g.stop[row] = (unsigned char)st.stop;
    }
}
#endif  // __HIPCC__

}  // namespace ghr
