// ghr_latent.h -- the Gaussian side of the latent-strand stage (src/train_latent_strands.py, src/scene/gaussian_model_latent_strands.py).
//
// Three things stand between a strand generator and the renderer in that stage, and one behind it:
//   * the strands arrive as POINTS p [S, L, 3] (a non-leaf tensor), :451-452, 490-499:
//         xyz = (p[:, 1:] + p[:, :-1]) * 0.5,  dir = p[:, 1:] - p[:, :-1],  rotation = parallel_transport(x^, dir),
//         scaling = (|dir| / 2, s, s)            -- k_points_build / k_points_build_bwd (no prefix sum, any L >= 2);
//   * the appearance is per STRAND and `repeat`ed over the L - 1 segments, :463-475 -- k_rows_expand / k_rows_reduce;
//   * the loss has no SSIM, a ONE-channel mask mean and four NaN rules, src/train_latent_strands.py:130-152 --
//     k_latent_loss_fwd / k_latent_loss_fold / k_latent_loss_bwd: pointwise, 13 planes read and 10 written.
// Row s * n_seg + k is segment k of strand s, the layout of ghr_strands.h, whose row functions are used as they are.
// All per-row and per-pixel arithmetic is in GHR_HD functions (tests/hostsim/ghr_hostsim_latent.cpp runs them on the CPU).
#pragma once
#include "ghr_device.h"
#include "ghr_loss.h"
#include "ghr_strands.h"

namespace ghr {

#define GHR_LATENT_BLOCK 256
#define GHR_LATENT_AUX 8      // floats in front of the loss slots: {Ll1, LCE, LOR, nan(Ll1), nan(LCE), nan(LOR), sum of weights, pad}
#define GHR_LATENT_TERMS 4    // partial sums per slot: l1, ce, or_num, or_den
#define GHR_LATENT_QUAD 4     // pixels per thread of the loss kernels (one 16-B load per plane)

// ---- points -> segment rows -------------------------------------------------------------------------------------------
// One segment from its two end points a (start), b (end).
GHR_HD void points_seg_fwd(const float* a, const float* b, float scale, float* xyz, float* dir, float* rot, float* scaling)
{
#pragma unroll
    for (int c = 0; c < 3; c++) {
        xyz[c] = (b[c] + a[c]) * 0.5f;
        dir[c] = b[c] - a[c];
    }
    strand_row_fwd(dir[0], dir[1], dir[2], scale, rot, scaling);
}

// Total cotangent g of one segment's direction: strand_row_bwd (rotation, scaling[0]) plus the direction rows' own.
GHR_HD void points_seg_cot(const float* a, const float* b, const float* d_rot, const float* d_scaling, const float* d_dir, float* g)
{
    const float dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
    strand_row_bwd(dx, dy, dz, d_rot, d_scaling != nullptr ? d_scaling[0] : 0.f, g);
    if (d_dir != nullptr) { g[0] += d_dir[0]; g[1] += d_dir[1]; g[2] += d_dir[2]; }
}

// Point j of a strand whose points start at p and whose segment rows start at row 0 of the cotangent pointers (any may be NULL):
// + d_xyz / 2 + g from segment j - 1 (its end), then + d_xyz / 2 - g from segment j (its start).
GHR_HD void points_point_bwd(const float* p, int j, int L, const float* d_xyz, const float* d_rot, const float* d_scaling,
                             const float* d_dir, float* out)
{
    float o[3] = {0.f, 0.f, 0.f};
    if (j >= 1) {
        const int k = j - 1;
        float g[3];
        points_seg_cot(p + 3 * k, p + 3 * j, d_rot ? d_rot + 4 * k : nullptr, d_scaling ? d_scaling + 3 * k : nullptr,
                       d_dir ? d_dir + 3 * k : nullptr, g);
#pragma unroll
        for (int c = 0; c < 3; c++) o[c] = (d_xyz ? 0.5f * d_xyz[3 * k + c] : 0.f) + g[c];
    }
    if (j + 1 < L) {
        const int k = j;
        float g[3];
        points_seg_cot(p + 3 * j, p + 3 * (j + 1), d_rot ? d_rot + 4 * k : nullptr, d_scaling ? d_scaling + 3 * k : nullptr,
                       d_dir ? d_dir + 3 * k : nullptr, g);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float t = (d_xyz ? 0.5f * d_xyz[3 * k + c] : 0.f) - g[c];
            o[c] = j >= 1 ? o[c] + t : t;
        }
    }
    out[0] = o[0]; out[1] = o[1]; out[2] = o[2];
}

struct PointsArgs {
    int S, L;
    const float* p;   // [S, L, 3]
    float scale;
    float* xyz;       // [S (L-1), 3]
    float* rot;       // [S (L-1), 4]
    float* scaling;   // [S (L-1), 3]
    float* dir;       // [S (L-1), 3]
};

// A workgroup owns GHR_LATENT_BLOCK consecutive segment rows.  Their end points are ONE contiguous range of p (row r of
// strand s has the points r + s and r + s + 1): at most 2 x 256 points, staged in LDS by coalesced loads; the three 3-float
// outputs go back through LDS so that every global store instruction writes consecutive dwords, the 4-float one as b128.
__global__ void __launch_bounds__(GHR_LATENT_BLOCK) k_points_build(PointsArgs a)
{
    __shared__ float s_p[2 * GHR_LATENT_BLOCK * 3];
    __shared__ float s_o[3][GHR_LATENT_BLOCK * 3];
    const int tid = threadIdx.x, n_seg = a.L - 1;
    const size_t rows = (size_t)a.S * n_seg;
    const size_t r0 = (size_t)blockIdx.x * GHR_LATENT_BLOCK;
    const int nr = rows - r0 < GHR_LATENT_BLOCK ? (int)(rows - r0) : GHR_LATENT_BLOCK;
    const size_t s_first = r0 / n_seg, s_last = (r0 + nr - 1) / n_seg;
    const size_t pt0 = r0 + s_first;                              // first point of the range
    const int npt = (int)((r0 + nr - 1 + s_last + 1) - pt0) + 1;  // <= 2 nr
    for (int i = tid; i < 3 * npt; i += GHR_LATENT_BLOCK) s_p[i] = a.p[3 * pt0 + i];
    __syncthreads();
    if (tid < nr) {
        const size_t r = r0 + tid;
        const int lp = (int)(r + r / n_seg - pt0);
        float xyz[3], dir[3], q[4], sc[3];
        points_seg_fwd(s_p + 3 * lp, s_p + 3 * lp + 3, a.scale, xyz, dir, q, sc);
        *reinterpret_cast<f4*>(a.rot + r * 4) = f4{q[0], q[1], q[2], q[3]};
#pragma unroll
        for (int c = 0; c < 3; c++) {
            s_o[0][3 * tid + c] = xyz[c];
            s_o[1][3 * tid + c] = sc[c];
            s_o[2][3 * tid + c] = dir[c];
        }
    }
    __syncthreads();
    for (int i = tid; i < 3 * nr; i += GHR_LATENT_BLOCK) {
        a.xyz[3 * r0 + i] = s_o[0][i];
        a.scaling[3 * r0 + i] = s_o[1][i];
        a.dir[3 * r0 + i] = s_o[2][i];
    }
}

struct PointsBwdArgs {
    int S, L;
    const float* p;
    const float* d_xyz;      // [S (L-1), 3] or NULL
    const float* d_rot;      // [S (L-1), 4] or NULL
    const float* d_scaling;  // [S (L-1), 3] or NULL (column 0 is read)
    const float* d_dir;      // [S (L-1), 3] or NULL
    float* d_p;              // [S, L, 3], assigned
};

// Gather form: one thread per point, no atomics -- the same bits run after run.
__global__ void __launch_bounds__(GHR_LATENT_BLOCK) k_points_build_bwd(PointsBwdArgs a)
{
    const size_t i = (size_t)blockIdx.x * GHR_LATENT_BLOCK + threadIdx.x;
    if (i >= (size_t)a.S * a.L) return;
    const size_t s = i / a.L;
    const int j = (int)(i - s * a.L);
    const size_t row0 = s * (a.L - 1);
    float o[3];
    points_point_bwd(a.p + 3 * s * a.L, j, a.L, a.d_xyz ? a.d_xyz + 3 * row0 : nullptr, a.d_rot ? a.d_rot + 4 * row0 : nullptr,
                     a.d_scaling ? a.d_scaling + 3 * row0 : nullptr, a.d_dir ? a.d_dir + 3 * row0 : nullptr, o);
    float* out = a.d_p + 3 * i;
    out[0] = o[0]; out[1] = o[1]; out[2] = o[2];
}

// ---- per-strand rows <-> per-segment rows -----------------------------------------------------------------------------
// dst[(s n_seg + k) C + c] = src[s C + c].  V = 4: C % 4 == 0 and 16-B aligned pointers, one float4 per thread.
template <int V>
__global__ void __launch_bounds__(GHR_LATENT_BLOCK) k_rows_expand(size_t total, int n_seg, int C, const float* src, float* dst)
{
    const size_t i = (size_t)blockIdx.x * GHR_LATENT_BLOCK + threadIdx.x;  // element (V = 1) or float4 (V = 4) of dst
    if (i >= total) return;
    const int cv = C / V;
    const size_t row = i / cv;
    const int c = (int)(i - row * cv);
    const size_t s = row / n_seg;
    if (V == 4) reinterpret_cast<f4*>(dst)[i] = reinterpret_cast<const f4*>(src)[s * cv + c];
    else dst[i] = src[s * cv + c];
}

// Sum of a strand's n_seg rows in index order, one fp32 accumulator per (s, c).
GHR_HD float rows_reduce_one(const float* g, int n_seg, int C)
{
    float acc = g[0];
    for (int k = 1; k < n_seg; k++) acc = acc + g[(size_t)k * C];
    return acc;
}

template <int V>
__global__ void __launch_bounds__(GHR_LATENT_BLOCK) k_rows_reduce(size_t total, int n_seg, int C, const float* g, float* out)
{
    const size_t i = (size_t)blockIdx.x * GHR_LATENT_BLOCK + threadIdx.x;  // element (V = 1) or float4 (V = 4) of out
    if (i >= total) return;
    const int cv = C / V;
    const size_t s = i / cv;
    const int c = (int)(i - s * cv);
    if (V == 4) {
        const f4* src = reinterpret_cast<const f4*>(g) + s * n_seg * cv + c;
        f4 acc = src[0];
#pragma unroll 4
        for (int k = 1; k < n_seg; k++) acc = acc + src[(size_t)k * cv];  // component-wise: the order of rows_reduce_one
        reinterpret_cast<f4*>(out)[i] = acc;
    } else {
        out[i] = rows_reduce_one(g + s * n_seg * C + c, n_seg, C);
    }
}

// ---- the stage's loss ----------------------------------------------------------------------------------------------------
struct LatentLossArgs {
    int W, H;
    const float* image;     // [3,H,W] rendered
    const float* mask0;     // [1,H,W] rendered hair label
    const float* dir2d;     // [2,H,W] rendered 2D direction
    const float* oconf;     // [1,H,W] rendered orientation confidence or NULL (train_orient_conf = False)
    const float* gt_image;  // [3,H,W]
    const float* gt_mask0;  // [1,H,W]
    const float* gt_angle;  // [1,H,W]
    const float* gt_oconf;  // [1,H,W] or NULL: weight 1 (use_gt_orient_conf = False)
    float w_l1, w_mask, w_orient;
    float* sums;            // [GHR_LATENT_AUX | n_wg slots of GHR_LATENT_TERMS]
    const float* grad_loss; // backward: device scalar or NULL (1)
    float* d_packed;        // backward: [10,H,W]
};

struct LatentPix { float l1, ce, orn, ord; };

// Orientation term of one pixel through orient_pixel (ghr_loss.h).  Without a confidence, or_loss is |.|min pi * mask
// (loss_utils.py:40-41 skipped): orient_pixel at conf = 1 and mask = 1 gives  lmin pi - log(1 + 1e-7)  and derivatives that are
// the wanted ones exactly; the constant is added back (one rounding, <= 1 ulp of the value) and the mask applied afterwards.
// A NaN direction makes the term NaN, as F.normalize makes it (orient_pixel's fmaxf / fminf would swallow it, and this stage
// decides by isnan whether the term counts).
GHR_HD OrientPix latent_orient_pixel(float d0, float d1, bool has_conf, float conf, float gt_angle, float m)
{
    if (d0 != d0 || d1 != d1) {
        const float nan = d0 != d0 ? d0 : d1;
        return OrientPix{nan, nan, nan, nan};
    }
    if (has_conf) return orient_pixel(d0, d1, conf, gt_angle, m);
    const OrientPix one = orient_pixel(d0, d1, 1.0f, gt_angle, 1.0f);
    const float c0 = logf(1.0f + 1e-7f);  // what orient_pixel subtracted
    OrientPix o;
    o.l = (one.l + c0) * m;
    o.dl_dd0 = one.dl_dd0 * m;
    o.dl_dd1 = one.dl_dd1 * m;
    o.dl_dconf = 0.f;
    return o;
}

GHR_HD LatentPix latent_pixel_fwd(const float* im, const float* gt, float m0, float gm0, float d0, float d1, bool has_conf,
                                  float conf, float gt_angle, float w)
{
    LatentPix o;
    o.l1 = (fabsf(im[0] - gt[0]) + fabsf(im[1] - gt[1])) + fabsf(im[2] - gt[2]);
    o.ce = fabsf(m0 - gm0);
    o.orn = latent_orient_pixel(d0, d1, has_conf, conf, gt_angle, gm0).l * w;
    o.ord = w;
    return o;
}

GHR_HD float sign_(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

// Gradient of one pixel: out[0..2] image, out[3] mask0, out[4], out[5] dir2d, out[6] confidence.  k_l1 = up w_l1 / (3 N) or 0
// for a dropped term, k_ce = up w_mask / N or 0, k_or = up w_orient / sum(w) or 0 (then the orientation inputs are not read).
GHR_HD void latent_pixel_bwd(const float* im, const float* gt, float m0, float gm0, float d0, float d1, bool has_conf, float conf,
                             float gt_angle, float w, bool or_on, float k_l1, float k_ce, float k_or, float* out)
{
#pragma unroll
    for (int c = 0; c < 3; c++) out[c] = k_l1 * sign_(im[c] - gt[c]);
    out[3] = k_ce * sign_(m0 - gm0);
    out[4] = 0.f; out[5] = 0.f; out[6] = 0.f;
    if (or_on) {
        const OrientPix op = latent_orient_pixel(d0, d1, has_conf, conf, gt_angle, gm0);
        const float sc = k_or * w;
        out[4] = sc * op.dl_dd0;
        out[5] = sc * op.dl_dd1;
        out[6] = has_conf ? sc * op.dl_dconf : 0.f;
    }
}

// The fold's last step: totals of the four partial sums -> aux[GHR_LATENT_AUX] and the loss.  A term is dropped exactly when
// it is NaN (train_latent_strands.py:143-145 tests isnan, not isinf).
GHR_HD void latent_fold_finish(const double* t, double n_pix, float w_l1, float w_mask, float w_orient, float* aux, float* loss)
{
    float l1 = (float)(t[0] / (3.0 * n_pix)), ce = (float)(t[1] / n_pix), lo = (float)(t[2] / t[3]);
    const float b0 = l1 != l1 ? 1.f : 0.f, b1 = ce != ce ? 1.f : 0.f, b2 = lo != lo ? 1.f : 0.f;
    if (b0 != 0.f) l1 = 0.f;
    if (b1 != 0.f) ce = 0.f;
    if (b2 != 0.f) lo = 0.f;
    aux[0] = l1; aux[1] = ce; aux[2] = lo;
    aux[3] = b0; aux[4] = b1; aux[5] = b2;
    aux[6] = (float)t[3];
    aux[7] = 0.f;
    loss[0] = (l1 * w_l1 + ce * w_mask) + lo * w_orient;
}

// Backward's three uniform factors from aux.
GHR_HD void latent_bwd_factors(const float* aux, float up, double n_pix, float w_l1, float w_mask, float w_orient, float* k)
{
    k[0] = aux[3] != 0.f ? 0.f : up * w_l1 * (float)(1.0 / (3.0 * n_pix));
    k[1] = aux[4] != 0.f ? 0.f : up * w_mask * (float)(1.0 / n_pix);
    k[2] = (aux[5] != 0.f || w_orient == 0.f) ? 0.f : up * w_orient / aux[6];
}

#if defined(__HIP_DEVICE_COMPILE__)
// Sum over the 256 threads of a workgroup in a fixed tree (t += t + stride, stride 128 ... 1); every thread calls it.
template <int K>
__device__ __forceinline__ void latent_block_tree(float (&v)[K], float (*s_red)[GHR_LATENT_BLOCK])
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; k++) s_red[k][tid] = v[k];
    __syncthreads();
    for (int st = GHR_LATENT_BLOCK / 2; st >= 1; st >>= 1) {
        if (tid < st) {
#pragma unroll
            for (int k = 0; k < K; k++) s_red[k][tid] = s_red[k][tid] + s_red[k][tid + st];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = s_red[k][0];
}
#endif

// Thread t of workgroup b owns the pixels 4 (256 b + t) ... + 3 and adds them in pixel order, in both forms: VEC reads
// them as one float4 per plane (H W % 4 == 0, 16-B aligned planes), the scalar form one by one with the image's end as bound.
template <int VEC>
__global__ void __launch_bounds__(GHR_LATENT_BLOCK) k_latent_loss_fwd(LatentLossArgs a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ float s_red[GHR_LATENT_TERMS][GHR_LATENT_BLOCK];
    const size_t N = (size_t)a.W * a.H;
    const size_t p0 = ((size_t)blockIdx.x * GHR_LATENT_BLOCK + threadIdx.x) * GHR_LATENT_QUAD;
    const bool has_conf = a.oconf != nullptr, has_w = a.gt_oconf != nullptr;
    float v[13][GHR_LATENT_QUAD];  // image 0-2, gt 3-5, mask0, gt_mask0, dir 8-9, conf, gt_angle, weight
    const float* planes[13] = {a.image, a.image + N, a.image + 2 * N, a.gt_image, a.gt_image + N, a.gt_image + 2 * N, a.mask0,
                               a.gt_mask0, a.dir2d, a.dir2d + N, a.oconf, a.gt_angle, a.gt_oconf};
    int n = 0;
    if (p0 < N) n = N - p0 < GHR_LATENT_QUAD ? (int)(N - p0) : GHR_LATENT_QUAD;
#pragma unroll
    for (int k = 0; k < 13; k++) {
        const bool on = planes[k] != nullptr;
        const float fill = 1.0f;  // absent confidence / weight
        if (VEC) {
            f4 t = f4{fill, fill, fill, fill};
            if (on && n > 0) t = *reinterpret_cast<const f4*>(planes[k] + p0);
            v[k][0] = t.x; v[k][1] = t.y; v[k][2] = t.z; v[k][3] = t.w;
        } else {
#pragma unroll
            for (int q = 0; q < GHR_LATENT_QUAD; q++) v[k][q] = (on && q < n) ? planes[k][p0 + q] : fill;
        }
    }
    float s[GHR_LATENT_TERMS] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < GHR_LATENT_QUAD; q++) {
        if (q < n) {
            const float im[3] = {v[0][q], v[1][q], v[2][q]}, gt[3] = {v[3][q], v[4][q], v[5][q]};
            const LatentPix o = latent_pixel_fwd(im, gt, v[6][q], v[7][q], v[8][q], v[9][q], has_conf, v[10][q], v[11][q],
                                                 has_w ? v[12][q] : 1.0f);
            s[0] += o.l1; s[1] += o.ce; s[2] += o.orn; s[3] += o.ord;
        }
    }
    latent_block_tree<GHR_LATENT_TERMS>(s, s_red);
    if (threadIdx.x == 0) {
        float* dst = a.sums + GHR_LATENT_AUX + (size_t)blockIdx.x * GHR_LATENT_TERMS;
        *reinterpret_cast<f4*>(dst) = f4{s[0], s[1], s[2], s[3]};
    }
#endif
}

// One workgroup: thread t adds the slots t, t + 256, ... in that order, the fixed tree adds the 256 threads, thread 0 finishes.
__global__ void __launch_bounds__(GHR_LATENT_BLOCK) k_latent_loss_fold(LatentLossArgs a, uint32_t n_slots, float* loss_out)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ float s_red[GHR_LATENT_TERMS][GHR_LATENT_BLOCK];
    float s[GHR_LATENT_TERMS] = {0.f, 0.f, 0.f, 0.f};
    for (uint32_t i = threadIdx.x; i < n_slots; i += GHR_LATENT_BLOCK) {
        const f4 t = *reinterpret_cast<const f4*>(a.sums + GHR_LATENT_AUX + (size_t)i * GHR_LATENT_TERMS);
        s[0] += t.x; s[1] += t.y; s[2] += t.z; s[3] += t.w;
    }
    latent_block_tree<GHR_LATENT_TERMS>(s, s_red);
    if (threadIdx.x == 0) {
        const double t[4] = {(double)s[0], (double)s[1], (double)s[2], (double)s[3]};
        latent_fold_finish(t, (double)a.W * (double)a.H, a.w_l1, a.w_mask, a.w_orient, a.sums, loss_out);
    }
#endif
}

// Recomputes pointwise and writes all ten planes of d_packed (zeros in 4, 7, 9, in 8 without a confidence, and for a dropped term).
template <int VEC>
__global__ void __launch_bounds__(GHR_LATENT_BLOCK) k_latent_loss_bwd(LatentLossArgs a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const size_t N = (size_t)a.W * a.H;
    const size_t p0 = ((size_t)blockIdx.x * GHR_LATENT_BLOCK + threadIdx.x) * GHR_LATENT_QUAD;
    if (p0 >= N) return;
    const int n = N - p0 < GHR_LATENT_QUAD ? (int)(N - p0) : GHR_LATENT_QUAD;
    const bool has_conf = a.oconf != nullptr, has_w = a.gt_oconf != nullptr;
    float k[3];
    latent_bwd_factors(a.sums, a.grad_loss ? a.grad_loss[0] : 1.0f, (double)a.W * (double)a.H, a.w_l1, a.w_mask, a.w_orient, k);
    const bool or_on = k[2] != 0.f;  // (uniform)
    const float* planes[13] = {a.image, a.image + N, a.image + 2 * N, a.gt_image, a.gt_image + N, a.gt_image + 2 * N, a.mask0,
                               a.gt_mask0, a.dir2d, a.dir2d + N, a.oconf, a.gt_angle, a.gt_oconf};
    float v[13][GHR_LATENT_QUAD];
#pragma unroll
    for (int j = 0; j < 13; j++) {
        const bool on = planes[j] != nullptr && (j < 8 || or_on);
        if (VEC) {
            f4 t = f4{1.f, 1.f, 1.f, 1.f};
            if (on) t = *reinterpret_cast<const f4*>(planes[j] + p0);
            v[j][0] = t.x; v[j][1] = t.y; v[j][2] = t.z; v[j][3] = t.w;
        } else {
#pragma unroll
            for (int q = 0; q < GHR_LATENT_QUAD; q++) v[j][q] = (on && q < n) ? planes[j][p0 + q] : 1.f;
        }
    }
    float g[10][GHR_LATENT_QUAD];
#pragma unroll
    for (int q = 0; q < GHR_LATENT_QUAD; q++) {
        const float im[3] = {v[0][q], v[1][q], v[2][q]}, gt[3] = {v[3][q], v[4][q], v[5][q]};
        float o[7];
        latent_pixel_bwd(im, gt, v[6][q], v[7][q], v[8][q], v[9][q], has_conf, v[10][q], v[11][q], has_w ? v[12][q] : 1.0f, or_on,
                         k[0], k[1], k[2], o);
        g[0][q] = o[0]; g[1][q] = o[1]; g[2][q] = o[2]; g[3][q] = o[3]; g[4][q] = 0.f;
        g[5][q] = o[4]; g[6][q] = o[5]; g[7][q] = 0.f; g[8][q] = o[6]; g[9][q] = 0.f;
    }
#pragma unroll
    for (int c = 0; c < 10; c++) {
        float* dst = a.d_packed + (size_t)c * N + p0;
        if (VEC) *reinterpret_cast<f4*>(dst) = f4{g[c][0], g[c][1], g[c][2], g[c][3]};
        else {
#pragma unroll
            for (int q = 0; q < GHR_LATENT_QUAD; q++)
                if (q < n) dst[q] = g[c][q];
        }
    }
#endif
}

}  // namespace ghr
