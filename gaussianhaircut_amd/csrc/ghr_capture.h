// ghr_capture.h -- synthetic captures: the masks and the orientation map of a groom seen through a camera.
// The reference's third dataset type, "Synthetic", gets its views from Blender; Blender is not a dependency, so the capture is
// DEFINED here, as 8l and 8m define their pictures, and every form (this kernel, the host walk, the PyTorch comparator, the numpy
// model of the tests) is held to it bit for bit.  float32 + - x / and sqrtf only, in the operand order written, no contraction,
// integer counts.
//
//   View, raster and supersampling: the view is (M, H, W) with near and half_width r, supersampled by s in {1, 2, 4} exactly as 8l
//       does: Ms, rs = rows 0 and 1 of M and r times s.  The planes pix_to_segment and pix_to_face_out of ghr_strandview_raster at
//       sH x sW are the inputs.  n = s s.
//   Walk order: output pixel (i, j) owns the subsamples (s i + a, s j + b), visited a-major, then b, both ascending.
//   Per subsample, with k its segment entry and f its face entry:
//       if 0 <= k < S (L - 1):  n_hair += 1;  A, B are the segment's two world points, projected by vis_project_one(Ms, near) to
//           (ax, ay) and (bx, by).  If both are valid: dx = bx - ax, dy = by - ay, len2 = dx dx + dy dy.  If len2 > 0:
//           c2 = (dy dy - dx dx) / len2 and s2 = (2.f (dx dy)) / len2.  If both are finite: C += c2, then S += s2 -- sequential
//           float32 sums in the walk order.  (c2, s2) is the doubled angle of the direction (sin th, cos th).
//       otherwise, if 0 <= f < F:  n_face += 1.
//       An entry outside its table counts as nothing.
//   Outputs per pixel:
//       mask_hair = (255 n_hair + n / 2) / n, in integers;
//       mask_body = (255 (n_hair + n_face) + n / 2) / n: the silhouette, hair included (the loader forms image * body);
//       angle = the lowest k in 0 .. 179 that maximises C T[k][0] + S T[k][1]: strict > from k = 0, a NaN score never wins, 0 when
//           none wins.  T[k] = (cos 2 th_k, sin 2 th_k), th_k = k pi / 180, formed on the host in float64 and rounded once; T is an
//           INPUT table on the device, as k_gt_assemble's tables are.  Byte k is the screen direction (sin k deg, cos k deg), x right,
//           y down: the rasterizer's acos(dir.y sign(dir.x)) / pi and the Gabor bank's degree byte.
//       var = var_floor + 0.5f fmaxf(0.f, 1.f - sqrtf(C C + S S) / (float)n): the small-angle variance of th in rad^2; 0.5 where no
//           strand is seen -- the resultant is over all n subsamples, so a thin or half-covered pixel is less certain and the empty
//           pixel needs no special case.  var_floor >= 0, finite, default 0.
//   Image: render_strands' picture at the same arguments, byte for byte (the shade and resolve kernels of ghr_strandview.h); the
//       raster is made once and serves both.
//
// k_sv_capture: a thread makes four consecutive output pixels (k_gt_from_render's form): per pixel and row a one 16-B (s = 4), 8-B
// (s = 2) or 4-B load from each index plane, a lane's four pixels side by side; a repeated segment entry is not projected again
// (the same bits: the projection is a function of k); the table is staged in LDS and each entry is read once for the four pixels, at
// an address the whole wave shares; the three byte planes leave as one dword each and var as 16 B, with byte / float stores at the
// tail (and for planes that are not aligned so).  No atomics, no scratch.
// Everything per element is GHR_HD so that tests/hostsim/ghr_hostsim_capture.cpp runs the product's own arithmetic on the CPU.
#pragma once
#include "ghr_tilelists.h"

#define GHR_CAP_BLOCK 256
#define GHR_CAP_BINS 180
#define GHR_CAP_QUAD 4  // output pixels per thread

namespace ghr {

// The doubled angle of segment k (0 <= k < S (L - 1)); false: it adds nothing to C and S.
GHR_HD bool cap_segment_dir(int32_t k, int L, const float* points, const float* Ms, float near, float* c2, float* s2)
{
    const int s = k / (L - 1), i = k % (L - 1);
    const float* A = points + 3 * ((size_t)s * L + i);
    float pa[4], pb[4];
    vis_project_one(Ms, A, near, pa);
    vis_project_one(Ms, A + 3, near, pb);
    if (pa[3] == 0.f || pb[3] == 0.f) return false;
    const float dx = pb[0] - pa[0], dy = pb[1] - pa[1];
    const float len2 = dx * dx + dy * dy;
    if (!(len2 > 0.f)) return false;
    const float c = (dy * dy - dx * dx) / len2, sn = (2.f * (dx * dy)) / len2;
    if (!vis_finite(c) || !vis_finite(sn)) return false;
    *c2 = c; *s2 = sn;
    return true;
}

// The sums of one output pixel; last_k .. ok remember the latest projected segment.
struct CapAcc {
    int32_t n_hair, n_face;
    float C, S;
    int32_t last_k;
    float c2, s2;
    bool ok;
};

GHR_HD CapAcc cap_begin()
{
    CapAcc a;
    a.n_hair = 0; a.n_face = 0; a.C = 0.f; a.S = 0.f; a.last_k = -1; a.c2 = 0.f; a.s2 = 0.f; a.ok = false;
    return a;
}

// One subsample: n_seg = S (L - 1).
GHR_HD void cap_sample(CapAcc& a, int32_t k, int32_t f, int64_t n_seg, int F, int L, const float* points, const float* Ms, float near)
{
    if (k >= 0 && (int64_t)k < n_seg) {
        a.n_hair += 1;
        if (k != a.last_k) {
            a.ok = cap_segment_dir(k, L, points, Ms, near, &a.c2, &a.s2);
            a.last_k = k;
        }
        if (a.ok) { a.C += a.c2; a.S += a.s2; }
    } else if (f >= 0 && f < F) {
        a.n_face += 1;
    }
}

GHR_HD uint32_t cap_mask(int32_t count, int n) { return (uint32_t)(255 * count + n / 2) / (uint32_t)n; }

GHR_HD float cap_var(float C, float S, int n, float var_floor)
{
    return var_floor + 0.5f * fmaxf(0.f, 1.f - sqrtf(C * C + S * S) / (float)n);
}

// The bin of (C, S): table [180][2].
GHR_HD uint32_t cap_angle(float C, float S, const float* table)
{
    float best = -INFINITY;
    uint32_t arg = 0u;
    for (uint32_t k = 0u; k < GHR_CAP_BINS; k++) {
        const float score = C * table[2 * k] + S * table[2 * k + 1];
        if (score > best) { best = score; arg = k; }
    }
    return arg;
}

// One output pixel from the two index planes [s H][s W]: what the host walk runs.
GHR_HD void cap_pixel_one(int i, int j, int W, int s, const int32_t* pix_to_segment, const int32_t* pix_to_face_out, int S, int L,
                          const float* points, const float* Ms, float near, int F, const float* table, float var_floor,
                          uint8_t* mask_hair, uint8_t* mask_body, uint8_t* angle, float* var)
{
    CapAcc acc = cap_begin();
    const int64_t n_seg = (int64_t)S * (L - 1);
    for (int a = 0; a < s; a++)
        for (int b = 0; b < s; b++) {
            const size_t o = ((size_t)i * s + a) * ((size_t)W * s) + (size_t)j * s + b;
            cap_sample(acc, pix_to_segment[o], pix_to_face_out[o], n_seg, F, L, points, Ms, near);
        }
    const int n = s * s;
    *mask_hair = (uint8_t)cap_mask(acc.n_hair, n);
    *mask_body = (uint8_t)cap_mask(acc.n_hair + acc.n_face, n);
    *angle = (uint8_t)cap_angle(acc.C, acc.S, table);
    *var = cap_var(acc.C, acc.S, n, var_floor);
}

#if defined(__HIPCC__)
struct CapArgs {
    int32_t S, L, H, W, F;
    float near, var_floor;
    float Ms[12];
    int32_t out_dword, out_f4;      // the byte planes are 4-B aligned / var is 16-B aligned: whole quads leave as one store
    const float* points;            // [S][L][3]
    const int32_t* pix_to_segment;  // [s H][s W]
    const int32_t* pix_to_face_out; // [s H][s W]
    const float* table;             // [180][2]
    uint8_t* mask_hair;             // [H][W]
    uint8_t* mask_body;             // [H][W]
    uint8_t* angle;                 // [H][W]
    float* var;                     // [H][W]
};

typedef int32_t cap_i4 __attribute__((ext_vector_type(4)));
typedef int32_t cap_i2 __attribute__((ext_vector_type(2)));

// SS entries of one plane row; VEC: the plane's base is 4 SS-B aligned (every row of a pixel then is: a row holds SS W entries)
template <int SS, bool VEC>
__device__ __forceinline__ void cap_load_row(const int32_t* p, int32_t* out)
{
    if (VEC && SS == 4) {
        const cap_i4 v = *reinterpret_cast<const cap_i4*>(p);
        out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
    } else if (VEC && SS == 2) {
        const cap_i2 v = *reinterpret_cast<const cap_i2*>(p);
        out[0] = v.x; out[1] = v.y;
    } else {
#pragma unroll
        for (int b = 0; b < SS; b++) out[b] = p[b];
    }
}

// grid ceil(ceil(H W / 4) / 256), block 256
template <int SS, bool VEC>
__global__ void __launch_bounds__(GHR_CAP_BLOCK) k_sv_capture(CapArgs a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ float s_table[2 * GHR_CAP_BINS];
    for (uint32_t e = threadIdx.x; e < 2u * GHR_CAP_BINS; e += GHR_CAP_BLOCK) s_table[e] = a.table[e];
    __syncthreads();
    const uint32_t N = (uint32_t)a.H * (uint32_t)a.W;  // (<= 2^31 / n: checked by the entry)
    const uint32_t p0 = GHR_CAP_QUAD * (blockIdx.x * GHR_CAP_BLOCK + threadIdx.x);
    if (p0 >= N) return;
    constexpr int n = SS * SS;
    const int64_t n_seg = (int64_t)a.S * (a.L - 1);
    const size_t row = (size_t)a.W * SS;
    float C[GHR_CAP_QUAD], S[GHR_CAP_QUAD];
    uint32_t hair = 0u, body = 0u;
#pragma unroll
    for (int q = 0; q < GHR_CAP_QUAD; q++) { C[q] = 0.f; S[q] = 0.f; }
    // (the pixel and row loops stay loops: one copy of the projection per column of a row, not one per subsample of the quad)
#pragma unroll 1
    for (int q = 0; q < GHR_CAP_QUAD; q++) {
        CapAcc acc = cap_begin();
        const uint32_t p = p0 + q;
        if (p < N) {
            const uint32_t i = p / (uint32_t)a.W, j = p % (uint32_t)a.W;
            const size_t o = (size_t)i * SS * row + (size_t)j * SS;
#pragma unroll 1
            for (int r = 0; r < SS; r++) {
                int32_t k[SS], f[SS];
                cap_load_row<SS, VEC>(a.pix_to_segment + o + r * row, k);
                cap_load_row<SS, VEC>(a.pix_to_face_out + o + r * row, f);
#pragma unroll
                for (int b = 0; b < SS; b++) cap_sample(acc, k[b], f[b], n_seg, a.F, a.L, a.points, a.Ms, a.near);
            }
        }
#pragma unroll
        for (int e = 0; e < GHR_CAP_QUAD; e++)  // (selects, not an indexed store: the arrays stay in registers)
            if (e == q) { C[e] = acc.C; S[e] = acc.S; }
        hair |= cap_mask(acc.n_hair, n) << (8 * q);
        body |= cap_mask(acc.n_hair + acc.n_face, n) << (8 * q);
    }
    float best[GHR_CAP_QUAD];
    uint32_t arg[GHR_CAP_QUAD];
#pragma unroll
    for (int q = 0; q < GHR_CAP_QUAD; q++) { best[q] = -INFINITY; arg[q] = 0u; }
    for (uint32_t k = 0u; k < GHR_CAP_BINS; k++) {  // cap_angle for the four pixels: one read of the entry (one address per wave)
        const float t0 = s_table[2u * k], t1 = s_table[2u * k + 1u];
#pragma unroll
        for (int q = 0; q < GHR_CAP_QUAD; q++) {
            const float score = C[q] * t0 + S[q] * t1;
            if (score > best[q]) { best[q] = score; arg[q] = k; }
        }
    }
    const uint32_t deg = arg[0] | arg[1] << 8 | arg[2] << 16 | arg[3] << 24;
    float v[GHR_CAP_QUAD];
#pragma unroll
    for (int q = 0; q < GHR_CAP_QUAD; q++) v[q] = cap_var(C[q], S[q], n, a.var_floor);
    const bool whole = p0 + GHR_CAP_QUAD <= N;
    if (whole && a.out_dword) {  // (p0 is a multiple of 4: the dwords are aligned as the planes are)
        *reinterpret_cast<uint32_t*>(a.mask_hair + p0) = hair;
        *reinterpret_cast<uint32_t*>(a.mask_body + p0) = body;
        *reinterpret_cast<uint32_t*>(a.angle + p0) = deg;
    } else {
#pragma unroll
        for (int q = 0; q < GHR_CAP_QUAD; q++)
            if (p0 + q < N) {
                a.mask_hair[p0 + q] = (uint8_t)(hair >> (8 * q));
                a.mask_body[p0 + q] = (uint8_t)(body >> (8 * q));
                a.angle[p0 + q] = (uint8_t)(deg >> (8 * q));
            }
    }
    if (whole && a.out_f4) {
        *reinterpret_cast<f4*>(a.var + p0) = f4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int q = 0; q < GHR_CAP_QUAD; q++)
            if (p0 + q < N) a.var[p0 + q] = v[q];
    }
#endif
}
#endif  // __HIPCC__

}  // namespace ghr
