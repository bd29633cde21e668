// ghr_eval.h -- the evaluation pass on the packed [10,H,W] rasterizer output: the metrics of training_report and metrics.py,
// and the seven products of render_set.
//
// Reference: src/train_gaussians.py:232-293 (training_report: L1, mask L1 -- which it logs as `ce` --, orientation error and
// PSNR, all on clamp(x, 0, 1) of render, mask, orientation angle and their ground truths), src/metrics.py:71-78 (SSIM and PSNR
// per view), src/render_gaussians.py:31-68 (render_set: render, hair mask, head mask, masked orientation, two vis_orient
// colourings as 8-bit images through torchvision's save_image, the masked confidence as a float tensor) and
// src/utils/image_utils.py:22-37 (vis_orient).  In PyTorch that is a tail of ~10 kernels for the orientation angle, four
// clamps, two l1_loss, or_loss, psnr, ssim (ten depthwise convolutions) and two vis_orient per view, and seven float products
// over PCIe.  Here, per view:
//   k_eval_points    one streaming pass over the rendered and the 7 ground-truth planes: seven partial sums per workgroup
//   k_eval_ssim[_v]  the SSIM map's sum: the loss kernels' forward bodies (ghr_loss.h, EVAL) on the clamped images
//   k_eval_finalize  folds both sets of slots in a fixed order in double into one row of GHR_EVAL_TERMS doubles
//   k_eval_products  12 bytes + 1 float per pixel, ready for one device-to-host copy
// The per-pixel functions of the products (orient_angle_of, quant8, vis_orient_pixel, product_pixel) are in ghr_products.h.
// Every workgroup owns one slot and stores it: no atomics, nothing to zero, the same bits run after run.
#pragma once
#include "ghr_device.h"
#include "ghr_loss.h"
#include "ghr_products.h"

namespace ghr {

#define GHR_EVAL_TERMS 8        // doubles per view: {l1, ce, or_num, or_den, mse[3], ssim}
#define GHR_EVAL_POINT_TERMS 7  // partial sums per slot of k_eval_points: the first seven of them
#define GHR_EVAL_MAX_GROUPS 2048

// One pixel of the packed render (rgb, hair label, foreground, dir2d x, dir2d y) and of the ground truth
struct EvalIn {
    float r[3], m[2], d0, d1;
    float g[3], gm[2], ga, gw;  // ga, gw: ground-truth angle and orientation weight (0 without the orientation terms)
};
// {|dr| + |dg| + |db|, |dm0| + |dm1|, orientation numerator, orientation weight, squared error per colour channel}
struct EvalPix { float t[GHR_EVAL_POINT_TERMS]; };
GHR_HD EvalPix eval_pixel(const EvalIn& p, bool orient)
{
    const float PI = 3.14159265358979323846f;
    EvalPix o;
    float e[3];
#pragma unroll
    for (int c = 0; c < 3; c++) e[c] = clamp01(p.r[c]) - clamp01(p.g[c]);
    const float gm0 = clamp01(p.gm[0]);
    o.t[0] = (fabsf(e[0]) + fabsf(e[1])) + fabsf(e[2]);
    o.t[1] = fabsf(clamp01(p.m[0]) - gm0) + fabsf(clamp01(p.m[1]) - clamp01(p.gm[1]));
    o.t[2] = 0.f;
    o.t[3] = 0.f;
    if (orient) {  // or_loss(angle, gt, mask = gt_mask[:1], weight = gt_orient_conf), confs = None
        const float d = clamp01(orient_angle_of(p.d0, p.d1)) - clamp01(p.ga);
        const float l = fminf(fabsf(d), fminf(fabsf(d - 1.f), fabsf(d + 1.f)));
        o.t[2] = l * PI * gm0 * p.gw;
        o.t[3] = p.gw;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) o.t[4 + c] = e[c] * e[c];
    return o;
}

struct EvalArgs {
    int W, H;
    const float* renders;   // [10,H,W] packed: rgb 0-2, mask 3-4, dir2d 5-6, orientation confidence 8
    const float* gt_image;  // [3,H,W]
    const float* gt_mask;   // [2,H,W]
    const float* gt_angle;  // [1,H,W] or NULL (no orientation terms)
    const float* gt_oconf;  // [1,H,W] or NULL
    float* slots;           // [GHR_EVAL_POINT_TERMS][n_slots]
    uint32_t n_slots;       // workgroups of k_eval_points
};

GHR_HD uint32_t eval_point_groups(int W, int H)
{
    const size_t quads = ((size_t)W * H + 3) / 4, g = (quads + 255) / 256;
    return (uint32_t)(g < GHR_EVAL_MAX_GROUPS ? g : GHR_EVAL_MAX_GROUPS);
}

// grid eval_point_groups(W, H), block 256.  A thread takes the quads (four consecutive pixels) t, t + T, ... of the image and
// adds their pixels' terms in pixel order, so the scalar form (any pointers, any size; it also takes the tail quad) and the
// float4 form build every slot from the same additions in the same order: bit-identical sums per slot.
template <bool VEC>
__device__ __forceinline__ void eval_points_body(const EvalArgs& a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ float s_red[4][8];
    const size_t N = (size_t)a.W * a.H, quads = (N + 3) / 4;
    const bool orient = a.gt_angle != nullptr;  // uniform
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (size_t)gridDim.x * 256) {
        const size_t p0 = 4 * q;
        float r[7][4], g[7][4];  // rendered planes 0-6 (the metrics read neither confidence nor depth); ground-truth image, mask, angle, weight
#pragma unroll
        for (int k = 0; k < 7; k++) load_quad<VEC>(a.renders + (size_t)k * N, p0, N, r[k]);
#pragma unroll
        for (int k = 0; k < 3; k++) load_quad<VEC>(a.gt_image + (size_t)k * N, p0, N, g[k]);
#pragma unroll
        for (int k = 0; k < 2; k++) load_quad<VEC>(a.gt_mask + (size_t)k * N, p0, N, g[3 + k]);
        if (orient) {
            load_quad<VEC>(a.gt_angle, p0, N, g[5]);
            load_quad<VEC>(a.gt_oconf, p0, N, g[6]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) g[5][j] = g[6][j] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (VEC || p0 + j < N) {
                EvalIn in;
                in.r[0] = r[0][j]; in.r[1] = r[1][j]; in.r[2] = r[2][j];
                in.m[0] = r[3][j]; in.m[1] = r[4][j];
                in.d0 = r[5][j]; in.d1 = r[6][j];
                in.g[0] = g[0][j]; in.g[1] = g[1][j]; in.g[2] = g[2][j];
                in.gm[0] = g[3][j]; in.gm[1] = g[4][j];
                in.ga = g[5][j]; in.gw = g[6][j];
                const EvalPix e = eval_pixel(in, orient);
#pragma unroll
                for (int k = 0; k < GHR_EVAL_POINT_TERMS; k++) s[k] += e.t[k];
            }
        }
    }
    block_sum_n<GHR_EVAL_POINT_TERMS>(s, s_red);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < GHR_EVAL_POINT_TERMS; k++) a.slots[(size_t)k * a.n_slots + blockIdx.x] = s[k];
#endif
}
__global__ void __launch_bounds__(256) k_eval_points(EvalArgs a) { eval_points_body<false>(a); }
__global__ void __launch_bounds__(256) k_eval_points_v(EvalArgs a) { eval_points_body<true>(a); }

// SSIM of clamp(render) against clamp(ground truth): the forward bodies of the loss kernels, one partial sum per workgroup.
// Grids as k_loss_fwd (tile form) and k_loss_fwd_v (marching form).
__global__ void __launch_bounds__(256) k_eval_ssim(LossArgs a) { loss_fwd_body<0, true>(a); }
__global__ void __launch_bounds__(64) k_eval_ssim_v(LossArgs a) { loss_fwd_march_any<0, true>(a); }

// One 256-thread workgroup: thread t adds the slots t, t + 256, ... of each term in double, then the 256 partial sums are
// folded pairwise through LDS -- a fixed order.  row = {l1, ce, or_num, or_den, mse[3], ssim}: means over the elements for
// l1 (3 H W), ce (2 H W), mse (H W each) and ssim (3 H W; 0 when no SSIM slots were written), plain sums for the two
// orientation terms (their quotient is formed by the caller: 0 / 0 is the reference's NaN).
__global__ void __launch_bounds__(256) k_eval_finalize(const float* point_slots, uint32_t n_point, const float* ssim_slots,
                                                       uint32_t n_ssim, double n_pix, double* row)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ double s_part[GHR_EVAL_TERMS][256];
    const int tid = threadIdx.x;
    double s[GHR_EVAL_TERMS];
#pragma unroll
    for (int k = 0; k < GHR_EVAL_TERMS; k++) s[k] = 0.0;
    for (uint32_t i = tid; i < n_point; i += 256u)
#pragma unroll
        for (int k = 0; k < GHR_EVAL_POINT_TERMS; k++) s[k] += (double)point_slots[(size_t)k * n_point + i];
    for (uint32_t i = tid; i < n_ssim; i += 256u) s[GHR_EVAL_TERMS - 1] += (double)ssim_slots[i];
#pragma unroll
    for (int k = 0; k < GHR_EVAL_TERMS; k++) s_part[k][tid] = s[k];
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if (tid < off)
#pragma unroll
            for (int k = 0; k < GHR_EVAL_TERMS; k++) s_part[k][tid] += s_part[k][tid + off];
        __syncthreads();
    }
    if (tid < GHR_EVAL_TERMS) {
        const double div[GHR_EVAL_TERMS] = {3.0 * n_pix, 2.0 * n_pix, 1.0, 1.0, n_pix, n_pix, n_pix, 3.0 * n_pix};
        double d = 1.0;
#pragma unroll
        for (int k = 0; k < GHR_EVAL_TERMS; k++) d = tid == k ? div[k] : d;
        row[tid] = s_part[tid][0] / d;
    }
#endif
}

struct ProductArgs {
    int W, H;
    const float* renders;  // [10,H,W] packed
    uint8_t* bytes;        // [render HWC3 | hair HW | head HW | orient HW | orient_vis HWC3 | conf_vis HWC3] = 12 H W bytes
    float* conf;           // [H,W]
};

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ uint32_t pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return a | (b << 8) | (c << 16) | (d << 24); }
// twelve bytes c0[0] c1[0] c2[0] c0[1] ... of four HWC3 pixels as three words
__device__ __forceinline__ void store_hwc3x4(uint8_t* dst, const uint32_t (*c)[3])
{
    uint32_t* w = reinterpret_cast<uint32_t*>(dst);
    w[0] = pack4(c[0][0], c[0][1], c[0][2], c[1][0]);
    w[1] = pack4(c[1][1], c[1][2], c[2][0], c[2][1]);
    w[2] = pack4(c[2][2], c[3][0], c[3][1], c[3][2]);
}
#endif

// grid ceil(ceil(H W / 4) / 256), block 256; a thread makes four consecutive pixels.  VEC (H*W % 4 == 0, 16-B aligned planes,
// 4-B aligned byte block): float4 loads and whole-word stores; otherwise single loads and byte stores with the end checked.
template <bool VEC>
__device__ __forceinline__ void eval_products_body(const ProductArgs& a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const size_t N = (size_t)a.W * a.H, quads = (N + 3) / 4;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= quads) return;
    const size_t p0 = 4 * q;
    float r[8][4];
#pragma unroll
    for (int k = 0; k < 7; k++) load_quad<VEC>(a.renders + (size_t)k * N, p0, N, r[k]);
    load_quad<VEC>(a.renders + (size_t)8 * N, p0, N, r[7]);
    ProductPix o[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float rgb[3] = {r[0][j], r[1][j], r[2][j]};
        o[j] = product_pixel(rgb, r[3][j], r[4][j], r[5][j], r[6][j], r[7][j]);
    }
    uint8_t* b_render = a.bytes;
    uint8_t* b_hair = a.bytes + 3 * N;
    uint8_t* b_head = a.bytes + 4 * N;
    uint8_t* b_orient = a.bytes + 5 * N;
    uint8_t* b_ovis = a.bytes + 6 * N;
    uint8_t* b_cvis = a.bytes + 9 * N;
    if (VEC) {
        uint32_t c[4][3];
#pragma unroll
        for (int j = 0; j < 4; j++) { c[j][0] = o[j].render[0]; c[j][1] = o[j].render[1]; c[j][2] = o[j].render[2]; }
        store_hwc3x4(b_render + 3 * p0, c);
#pragma unroll
        for (int j = 0; j < 4; j++) { c[j][0] = o[j].orient_vis[0]; c[j][1] = o[j].orient_vis[1]; c[j][2] = o[j].orient_vis[2]; }
        store_hwc3x4(b_ovis + 3 * p0, c);
#pragma unroll
        for (int j = 0; j < 4; j++) { c[j][0] = o[j].conf_vis[0]; c[j][1] = o[j].conf_vis[1]; c[j][2] = o[j].conf_vis[2]; }
        store_hwc3x4(b_cvis + 3 * p0, c);
        *reinterpret_cast<uint32_t*>(b_hair + p0) = pack4(o[0].hair, o[1].hair, o[2].hair, o[3].hair);
        *reinterpret_cast<uint32_t*>(b_head + p0) = pack4(o[0].head, o[1].head, o[2].head, o[3].head);
        *reinterpret_cast<uint32_t*>(b_orient + p0) = pack4(o[0].orient, o[1].orient, o[2].orient, o[3].orient);
        *reinterpret_cast<f4*>(a.conf + p0) = f4{o[0].conf, o[1].conf, o[2].conf, o[3].conf};
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const size_t p = p0 + j;
            if (p < N) {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    b_render[3 * p + c] = (uint8_t)o[j].render[c];
                    b_ovis[3 * p + c] = (uint8_t)o[j].orient_vis[c];
                    b_cvis[3 * p + c] = (uint8_t)o[j].conf_vis[c];
                }
                b_hair[p] = (uint8_t)o[j].hair;
                b_head[p] = (uint8_t)o[j].head;
                b_orient[p] = (uint8_t)o[j].orient;
                a.conf[p] = o[j].conf;
            }
        }
    }
#endif
}
__global__ void __launch_bounds__(256) k_eval_products(ProductArgs a) { eval_products_body<true>(a); }
__global__ void __launch_bounds__(256) k_eval_products_s(ProductArgs a) { eval_products_body<false>(a); }

}  // namespace ghr
