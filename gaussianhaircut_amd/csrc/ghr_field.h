// ghr_field.h -- the orientation field of a cloud of strand-aligned hair points, strands traced through it from scalp roots, and
// their resampling to a fixed number of points: a network-free initial groom (strand_growing.py).  There is no
// counterpart in the reference; this header is the definition, and every form (these kernels, tests/hostsim/ghr_hostsim_field.cpp's
// walk of them, strand_growing.py's composed form, tests/field_cases.py's float64 arbiter) is held to it.
//
// All arithmetic is fp32, without contraction, in the order written; sqrtf and / are IEEE.
//
// The cloud: P hair points, each with position p_i, unit line direction d_i (its sign is meaningless), weight m_i >= 0 and colour
// f_i (3 floats), the positions in Morton-key order over their bounds as knn_cloud lays them out (ghr_knn.h); the order is part of
// the field's state.
//
// The field at x under heading t: over the cloud points in ASCENDING key-ordered position, every accumulator a sequential sum from 0,
//     dx = p_i.x - x.x (y, z alike);  d2 = (dx*dx + dy*dy) + dz*dz        (knn_dist2's expression)
//     inside = d2 < r2                                                     (r2 = r*r formed once in fp32 by the caller)
//     u = 1 - d2 / r2;  k = u*u;  a = m_i * k
//     s = ((d_i.x*t.x + d_i.y*t.y) + d_i.z*t.z) < 0 ? -1 : +1             (the line aligned with the heading; 0 counts as +)
//     rho += a;  v += (a*s) * d_i;  c += a * f_i;  n += 1                  (inside points only)
// Outputs, none normalised: rho [Q], v [Q,3], c [Q,3], n [Q] (int32).  A box is skipped when knn_box_dist >= r2: exact, the bound
// is below every d2 of the box; and a lane that scans a block it did not need adds nothing.  So a query's bits do not depend on
// which queries share its wave, on the query order or on the launch schedule -- PROVIDED every wave walks the blocks in ascending
// order: knn_walk with first = 0, never from a seed that depends on the wave.
//
// The trace of strand s from root o with initial heading n (the scalp normal), step h, at most M steps, inertia beta, rho_min > 0,
// max_coast:
//     x = o;  t = n / max(|n|, 1e-8);  coast = 0;  steps = 0;  rows = 1;  C = (0,0,0);  R = 0
//     for j in 0 .. M-1:
//         (rho, v, c) = field(x, t);  lv = sqrtf((v.x*v.x + v.y*v.y) + v.z*v.z)
//         if rho >= rho_min and lv > 0:                       supported
//             u = v / lv;  b = t*(1-beta) + u*beta;  t = b / max(|b|, 1e-8);  coast = 0;  C += c;  R += rho
//         else:
//             coast += 1;  if coast > max_coast: stop
//         x = x + h*t;  path[rows++] = x;  if supported: steps = rows - 1
// path [S, M+1, 3]: every row is written, rows past the last computed one repeat it.  steps [S]: the last point reached by a
// supported step (trailing coasted points are cut).  rgb [S,3] = C / R, or 0 when R == 0.
//
// Resampling to L >= 2 points (integers decide the span, so every form agrees in bits): n = steps[s]; for k in 0 .. L-1:
//     num = k*n (int64);  q = num / (L-1);  rem = num % (L-1);  a = path[s, q];  b = path[s, min(q+1, n)]
//     out[s, k] = a + (b - a) * ((float)rem / (float)(L-1))
// With n = 0 all L points are the root.
//
// Kernels: k_field_pack (d_i, m_i, f_i into two float4 planes in the cloud's sorted order, after ghr_knn.h's k_knn_boxes),
// k_field_query (one query per lane, one wave per 64 queries, FieldGather on knn_walk: the payload of a staged block goes to a
// second LDS tile of the wave through the walk's stage hook and is read, as a broadcast, only by lanes an entry is inside of),
// k_field_trace (one strand per lane, the wave loops over the steps with one walk per step; a stopped lane is valid = false and
// votes in no ballot; all state in registers), k_strands_resample.  No floating-point atomics.  Per-element functions are GHR_HD:
// the host walks them.
#pragma once
#include "ghr_knn.h"

#define GHR_FIELD_WAVES 4     // waves per workgroup of k_field_query / k_field_trace
#define GHR_FIELD_BLOCK 256   // threads per workgroup of k_field_pack / k_strands_resample
#define GHR_FIELD_NORM_EPS 1e-8f

namespace ghr {

// The payload beside a cloud of P points: two planes of P float4 each, (d.x, d.y, d.z, m) and (f.x, f.y, f.z, 0).
inline uint64_t field_payload_bytes(uint64_t P) { return 2 * knn_up(P * sizeof(float4)); }
struct FieldPayload { const float4 *dm, *f; };
inline FieldPayload field_payload(char* base, uint64_t P)
{
    return FieldPayload{(const float4*)base, (const float4*)(base + knn_up(P * sizeof(float4)))};
}

// knn_walk's policy (see KnnTop3): the sums of the definition over the points inside the radius.  ptile: the wave's private
// 2 * GHR_KNN_BLOCK float4 of LDS.
struct FieldGather {
    float rho = 0.f, vx = 0.f, vy = 0.f, vz = 0.f, cx = 0.f, cy = 0.f, cz = 0.f;
    int n = 0;
    float r2, tx, ty, tz;
    FieldPayload pay;
    float4* ptile;
    GHR_HD FieldGather(float r2_, float tx_, float ty_, float tz_, FieldPayload pay_, float4* ptile_)
        : r2(r2_), tx(tx_), ty(ty_), tz(tz_), pay(pay_), ptile(ptile_) {}
    GHR_HD float bound(float3 q, float4 lo, float4 hi) const { return knn_box_dist(q, lo, hi); }
    GHR_HD bool needs(float boxdist) const { return boxdist < r2; }
    GHR_HD void stage(int blk, int n_, int lane)
    {
        if (lane < n_) {
            const long long at = (long long)blk * GHR_KNN_BLOCK + lane;
            ptile[lane] = pay.dm[at];
            ptile[GHR_KNN_BLOCK + lane] = pay.f[at];
        }
    }
    GHR_HD void add(float d2, const float4& dm, const float4& f)
    {
        const float u = 1.f - d2 / r2;
        const float k = u * u;
        const float a = dm.w * k;
        const float s = ((dm.x * tx + dm.y * ty) + dm.z * tz) < 0.f ? -1.f : 1.f;
        const float as = a * s;
        rho += a;
        vx += as * dm.x; vy += as * dm.y; vz += as * dm.z;
        cx += a * f.x; cy += a * f.y; cz += a * f.z;
        n += 1;
    }
    GHR_HD void scan(const float4* tile, int n_, int, float3 q)
    {
        for (int j = 0; j < n_; ++j) {
            const float d2 = knn_dist2(tile[j], q);  // the same address in every lane: an LDS broadcast
            if (d2 < r2) add(d2, ptile[j], ptile[GHR_KNN_BLOCK + j]);  // (a broadcast among the lanes the entry is inside of)
        }
    }
};

struct FieldTraceArgs { float r2, h, beta, one_minus_beta, rho_min; int M, max_coast; };

GHR_HD float field_len(float x, float y, float z) { return sqrtf((x * x + y * y) + z * z); }

// One strand's state.  x is the last point of the path, rows the points written so far.
struct FieldStrand {
    float x[3], t[3], C[3], R;
    int coast, steps, rows;
    bool live;
};

GHR_HD void field_strand_init(FieldStrand& s, const float* o, const float* nrm)
{
    const float l = fmaxf(field_len(nrm[0], nrm[1], nrm[2]), GHR_FIELD_NORM_EPS);
    for (int k = 0; k < 3; ++k) s.x[k] = o[k], s.t[k] = nrm[k] / l, s.C[k] = 0.f;
    s.R = 0.f;
    s.coast = s.steps = 0;
    s.rows = 1;
    s.live = true;
}

// The heading update of one step from the field at (s.x, s.t): field_strand_step below up to its new t (support, blend, coast, C,
// R, the coast stop), for ghr_grow.h's guarded trace, which asks the mesh before it moves.  Returns FIELD_STOPPED (the strand is
// not live afterwards), FIELD_COASTED or FIELD_SUPPORTED.  field_strand_step keeps its own copy of these lines: routed through
// this function k_field_trace compiles to other code; a guarded strand that never touches the mesh must equal the
// unguarded one bit for bit, which tests/test_grow_guarded_cpu.py holds the two to.
enum { FIELD_STOPPED = 0, FIELD_COASTED = 1, FIELD_SUPPORTED = 2 };
GHR_HD int field_strand_heading(FieldStrand& s, const FieldGather& g, const FieldTraceArgs& a)
{
    const float lv = field_len(g.vx, g.vy, g.vz);
    const bool supported = g.rho >= a.rho_min && lv > 0.f;
    if (supported) {
        const float b0 = s.t[0] * a.one_minus_beta + (g.vx / lv) * a.beta;
        const float b1 = s.t[1] * a.one_minus_beta + (g.vy / lv) * a.beta;
        const float b2 = s.t[2] * a.one_minus_beta + (g.vz / lv) * a.beta;
        const float lb = fmaxf(field_len(b0, b1, b2), GHR_FIELD_NORM_EPS);
        s.t[0] = b0 / lb; s.t[1] = b1 / lb; s.t[2] = b2 / lb;
        s.coast = 0;
        s.C[0] += g.cx; s.C[1] += g.cy; s.C[2] += g.cz;
        s.R += g.rho;
    } else {
        s.coast += 1;
        if (s.coast > a.max_coast) {
            s.live = false;
            return FIELD_STOPPED;
        }
    }
    return supported ? FIELD_SUPPORTED : FIELD_COASTED;
}

// One step of the definition's loop from the field at (s.x, s.t).  Returns whether a point was appended (it is s.x then); a
// strand that stops appends none and is not live afterwards.
GHR_HD bool field_strand_step(FieldStrand& s, const FieldGather& g, const FieldTraceArgs& a)
{
    const float lv = field_len(g.vx, g.vy, g.vz);
    const bool supported = g.rho >= a.rho_min && lv > 0.f;
    if (supported) {
        const float b0 = s.t[0] * a.one_minus_beta + (g.vx / lv) * a.beta;
        const float b1 = s.t[1] * a.one_minus_beta + (g.vy / lv) * a.beta;
        const float b2 = s.t[2] * a.one_minus_beta + (g.vz / lv) * a.beta;
        const float lb = fmaxf(field_len(b0, b1, b2), GHR_FIELD_NORM_EPS);
        s.t[0] = b0 / lb; s.t[1] = b1 / lb; s.t[2] = b2 / lb;
        s.coast = 0;
        s.C[0] += g.cx; s.C[1] += g.cy; s.C[2] += g.cz;
        s.R += g.rho;
    } else {
        s.coast += 1;
        if (s.coast > a.max_coast) {
            s.live = false;
            return false;
        }
    }
    for (int k = 0; k < 3; ++k) s.x[k] = s.x[k] + a.h * s.t[k];
    s.rows += 1;
    if (supported) s.steps = s.rows - 1;
    return true;
}

GHR_HD void field_strand_rgb(const FieldStrand& s, float* rgb)
{
    for (int k = 0; k < 3; ++k) rgb[k] = s.R == 0.f ? 0.f : s.C[k] / s.R;
}

// Point k of L of a strand whose path [M+1][3] has n kept steps (n clamped into [0, M]: only a caller's bad table holds another).
GHR_HD void field_resample_point(const float* path, int M, int n, int L, int k, float* out)
{
    n = n < 0 ? 0 : (n > M ? M : n);
    const long long num = (long long)k * n;
    const int q = (int)(num / (L - 1)), rem = (int)(num % (L - 1));
    const int q1 = q + 1 < n ? q + 1 : n;
    const float w = (float)rem / (float)(L - 1);
    for (int a = 0; a < 3; ++a) {
        const float pa = path[(size_t)q * 3 + a], pb = path[(size_t)q1 * 3 + a];
        out[a] = pa + (pb - pa) * w;
    }
}

#if defined(__HIPCC__)
// directions / colors [P][3], weights [P] in the caller's order; c.sorted is k_knn_boxes' (its w: the original index, in [0, P)).
__global__ void __launch_bounds__(GHR_FIELD_BLOCK) k_field_pack(KnnCloud c, const float* __restrict__ directions,
                                                                 const float* __restrict__ weights, const float* __restrict__ colors,
                                                                 float4* __restrict__ dm, float4* __restrict__ f)
{
    const long long i = (long long)blockIdx.x * GHR_FIELD_BLOCK + threadIdx.x;
    if (i >= c.P) return;
    int o = knn_as_int(c.sorted[i].w);
    if ((unsigned)o >= (unsigned)c.P) o = 0;
    const size_t b = (size_t)o * 3;
    dm[i] = make_float4(directions[b], directions[b + 1], directions[b + 2], weights[o]);
    f[i] = make_float4(colors[b], colors[b + 1], colors[b + 2], 0.f);
}

// The lane's row of a launch over N rows: order[i] (an entry outside [0, N) is read as 0) or i itself.
__device__ __forceinline__ long long field_row(const long long* __restrict__ order, long long i, long long N)
{
    if (!order) return i;
    const long long o = order[i];
    return (o < 0 || o >= N) ? 0 : o;
}

// x / t [Q][3]; order [Q] int64 or NULL: lane i of the launch takes query order[i]; rho, v, cc, n at the queries' own rows.
__global__ void __launch_bounds__(64 * GHR_FIELD_WAVES) k_field_query(KnnCloud c, FieldPayload pay, int Q, const float* __restrict__ x,
                                                                       const float* __restrict__ t,
                                                                       const long long* __restrict__ order, float r2,
                                                                       float* __restrict__ rho, float* __restrict__ v,
                                                                       float* __restrict__ cc, int* __restrict__ n)
{
    __shared__ float4 tiles[GHR_FIELD_WAVES][3 * GHR_KNN_BLOCK];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long q0 = ((long long)blockIdx.x * GHR_FIELD_WAVES + wave) * GHR_KNN_BLOCK;
    if (q0 >= Q) return;
    const bool valid = q0 + lane < Q;
    const size_t row = (size_t)field_row(order, valid ? q0 + lane : q0, Q);
    const float3 q = make_float3(x[row * 3], x[row * 3 + 1], x[row * 3 + 2]);
    FieldGather g(r2, t[row * 3], t[row * 3 + 1], t[row * 3 + 2], pay, tiles[wave] + GHR_KNN_BLOCK);
    knn_walk(c, tiles[wave], q, valid, 0, -1, g);  // ascending from block 0: the definition's order
    if (valid) {
        rho[row] = g.rho;
        v[row * 3] = g.vx; v[row * 3 + 1] = g.vy; v[row * 3 + 2] = g.vz;
        cc[row * 3] = g.cx; cc[row * 3 + 1] = g.cy; cc[row * 3 + 2] = g.cz;
        n[row] = g.n;
    }
}

// roots / normals [S][3]; order [S] int64 or NULL (the roots' key order: a wave's strands stay near each other); path [S][M+1][3],
// steps [S], rgb [S][3] at the strands' own rows.
__global__ void __launch_bounds__(64 * GHR_FIELD_WAVES) k_field_trace(KnnCloud c, FieldPayload pay, int S, const float* __restrict__ roots,
                                                                       const float* __restrict__ normals,
                                                                       const long long* __restrict__ order, FieldTraceArgs a,
                                                                       float* __restrict__ path, int* __restrict__ steps,
                                                                       float* __restrict__ rgb)
{
    __shared__ float4 tiles[GHR_FIELD_WAVES][3 * GHR_KNN_BLOCK];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long s0 = ((long long)blockIdx.x * GHR_FIELD_WAVES + wave) * GHR_KNN_BLOCK;
    if (s0 >= S) return;
    const bool mine = s0 + lane < S;
    const size_t row = (size_t)field_row(order, mine ? s0 + lane : s0, S);
    FieldStrand st;
    field_strand_init(st, roots + row * 3, normals + row * 3);
    st.live = mine;
    float* out = path + row * (size_t)(a.M + 1) * 3;
    if (mine)
        for (int k = 0; k < 3; ++k) out[k] = st.x[k];
    for (int j = 0; j < a.M; ++j) {
        if (!__any(st.live)) break;
        FieldGather g(a.r2, st.t[0], st.t[1], st.t[2], pay, tiles[wave] + GHR_KNN_BLOCK);
        knn_walk(c, tiles[wave], make_float3(st.x[0], st.x[1], st.x[2]), st.live, 0, -1, g);
        if (st.live && field_strand_step(st, g, a))
            for (int k = 0; k < 3; ++k) out[(size_t)(st.rows - 1) * 3 + k] = st.x[k];
    }
    if (mine) {
        for (int r = st.rows; r <= a.M; ++r)
            for (int k = 0; k < 3; ++k) out[(size_t)r * 3 + k] = st.x[k];
        steps[row] = st.steps;
        field_strand_rgb(st, rgb + row * 3);
    }
}

// path [S][M+1][3], steps [S] -> out [S][L][3]; one thread per point.
__global__ void __launch_bounds__(GHR_FIELD_BLOCK) k_strands_resample(int S, int M, int L, const float* __restrict__ path,
                                                                       const int* __restrict__ steps, float* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * GHR_FIELD_BLOCK + threadIdx.x;
    if (i >= (long long)S * L) return;
    const int s = (int)(i / L), k = (int)(i % L);
    field_resample_point(path + (size_t)s * (M + 1) * 3, M, steps[s], L, k, out + (size_t)i * 3);
}
#endif  // __HIPCC__

}  // namespace ghr
