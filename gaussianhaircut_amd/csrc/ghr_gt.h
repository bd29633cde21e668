// ghr_gt.h -- the ground-truth loader: Pillow's 8-bit bicubic resize and the assembly of a view's four training tensors.
//
// Reference: src/preprocessing/resize_images.py:101-106 (Image.resize(..., Image.BICUBIC) to // 2 and // 4), src/utils/
// general_utils.py:22-28 (PILtoTorch: Image.resize with its default filter, bicubic), src/utils/camera_utils.py:29-84 (loadCam)
// and src/scene/cameras.py:51-64 (the clamps, original_mask, the white background).
//
//   k_resample_u8_h   Pillow's ImagingResampleHorizontal_8bpc: one thread per output pixel, all its channels; _lds: the source
//                     span of 64 outputs x 8 rows and their coefficients staged in LDS, two rows per thread
//   k_resample_u8_v   ImagingResampleVertical_8bpc: a row is W C bytes whatever the channels; one thread owns four consecutive
//                     bytes; the coefficients of an output row are uniform over the workgroup (scalar loads)
//   k_gt_assemble     x / 255 and x / 180 through host-divided tables, the mask threshold, the white background, the bilinear
//                     sample of the variance map and conf = 1 / ((v / pi^2)^2 + 1e-7) (orient_conf_of of ghr_orient.h)
//   k_gt_resize_var   the bilinear sample alone (what the tests compare with F.interpolate)
//   k_gt_from_render  load_synthetic_rgba + load_synthetic_geom at -r 1 (camera_utils.py:51-64): the four tensors straight from the
//                     packed [10,H,W] render -- the levels render_set would have written as PNGs (product_core of ghr_products.h),
//                     every one / 255 through the table, the same mask rule and composite, the masked confidence as it is
// The host computes the coefficients in double exactly as Pillow's precompute_coeffs / normalize_coeffs_8bpc do; the kernels do
// the integer part: 22 fractional bits, a 32-bit accumulator that starts at 1 << 21, an arithmetic shift and a clip to 0 ... 255.
// The intermediate between the two passes is uint8, as Pillow's is.  No atomics, no float in the resize: the same bytes run
// after run.  The per-output arithmetic is in __host__ __device__ functions so that tests/hostsim/ghr_hostsim_gt.cpp runs it on
// the CPU.
#pragma once
#include "ghr_device.h"
#include "ghr_orient.h"
#include "ghr_products.h"

namespace ghr {

#define GHR_RESAMPLE_BITS 22   // Pillow's PRECISION_BITS (32 - 8 - 2)

// ---- resize ------------------------------------------------------------------------------------------------------------------

GHR_HD uint8_t resample_clip8(int32_t acc)
{
    const int32_t v = acc >> GHR_RESAMPLE_BITS;   // arithmetic: a negative lobe floors, then clips to 0
    return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// One output byte: n taps src[0], src[stride], ... against k[0 .. n).  Normalised bicubic weights sum to 2^22 with the negative
// lobes adding at most 0.3 of that in magnitude: 255 * 1.3 * 2^22 < 2^31, the 32-bit accumulator Pillow uses does not overflow.
GHR_HD uint8_t resample_tap_sum(const uint8_t* src, size_t stride, int n, const int32_t* k)
{
    int32_t acc = 1 << (GHR_RESAMPLE_BITS - 1);
    for (int i = 0; i < n; i++) acc += (int32_t)src[(size_t)i * stride] * k[i];
    return resample_clip8(acc);
}

// The host checks every window before a launch (ghr_resample_u8); a kernel checks its own once more, so that bounds that changed
// in between cost wrong bytes, not a read outside the image: a window that does not fit has no taps.
GHR_HD int resample_taps(int first, int n, int ksize, int in_size) { return (first < 0 || n < 0 || n > ksize || first > in_size - n) ? 0 : n; }

struct ResampleArgs {
    int in_w, in_h;        // the pass's input, in pixels
    int out_w, out_h;      // the pass's output: one of the two equals the input's
    int channels;
    const uint8_t* in;     // [in_h][in_w][channels]
    uint8_t* out;          // [out_h][out_w][channels]
    const int32_t* bounds; // [out][2]: first source index, taps
    const int32_t* coef;   // [out][ksize]
    int ksize;
};

// The direct form: one thread per output pixel, every tap a byte load from global memory.  Takes any bounds; it is what runs
// when a workgroup's windows do not fit the staged form below (more than GHR_RESAMPLE_HK taps, or bounds that do not ascend) and
// for one channel with at most 11 taps, where it measured faster (ghr_resample_u8).
template <int C>
__global__ __launch_bounds__(256) void k_resample_u8_h(ResampleArgs a)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.out_w || y >= a.in_h) return;
    const int n = resample_taps(a.bounds[2 * x], a.bounds[2 * x + 1], a.ksize, a.in_w), xmin = n ? a.bounds[2 * x] : 0;
    const int32_t* __restrict__ k = a.coef + (size_t)x * a.ksize;
    const uint8_t* __restrict__ src = a.in + ((size_t)y * a.in_w + xmin) * C;
    int32_t acc[C];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = 1 << (GHR_RESAMPLE_BITS - 1);
    for (int i = 0; i < n; i++) {
        const int32_t kk = k[i];
#pragma unroll
        for (int c = 0; c < C; c++) acc[c] += (int32_t)src[i * C + c] * kk;
    }
    uint8_t* dst = a.out + ((size_t)y * a.out_w + x) * C;
#pragma unroll
    for (int c = 0; c < C; c++) dst[c] = resample_clip8(acc[c]);
}

#define GHR_RESAMPLE_HC 64       // output columns of a workgroup
#define GHR_RESAMPLE_HR 8        // source rows of a workgroup: two per thread
#define GHR_RESAMPLE_HK 33       // most taps per output the staged form takes (a downscale by 8)
#define GHR_RESAMPLE_SPAN 2048   // most bytes of a source row under a workgroup's windows
#define GHR_RESAMPLE_PITCH (GHR_RESAMPLE_SPAN + 8)

// The staged form.  The windows of 64 neighbouring outputs cover one contiguous span of a source row: the workgroup copies that
// span of eight rows into LDS with aligned dword loads (a row starts at any byte: 53 * 3 = 159 bytes a row; the dwords at the
// buffer's two ends are assembled from bytes, nothing outside [in, in + in_w in_h C) is touched) and the 64 outputs' coefficients,
// contiguous in memory, beside it.  Each thread then forms one output column of two rows from LDS: a tap's coefficient is read
// once for both (ksize is odd: the 64 columns' reads fall into different banks).  The host picks this form only when the
// bounds of every workgroup ascend and its span fits.
template <int C>
__global__ __launch_bounds__(256) void k_resample_u8_h_lds(ResampleArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[GHR_RESAMPLE_HR][GHR_RESAMPLE_PITCH];
    __shared__ int32_t kc[GHR_RESAMPLE_HC * GHR_RESAMPLE_HK];
    const int xf = blockIdx.x * GHR_RESAMPLE_HC, cols = a.out_w - xf < GHR_RESAMPLE_HC ? a.out_w - xf : GHR_RESAMPLE_HC;
    const int y0 = blockIdx.y * GHR_RESAMPLE_HR, rows = a.in_h - y0 < GHR_RESAMPLE_HR ? a.in_h - y0 : GHR_RESAMPLE_HR;
    const int xl = xf + cols - 1;
    const int x0 = a.bounds[2 * xf], x1 = a.bounds[2 * xl] + a.bounds[2 * xl + 1], span = (x1 - x0) * C;
    if (x0 < 0 || x1 > a.in_w || x1 < x0 || span > GHR_RESAMPLE_SPAN || a.ksize > GHR_RESAMPLE_HK) return;   // (the host's choice, checked)
    for (int i = threadIdx.x; i < cols * a.ksize; i += 256) kc[i] = a.coef[(size_t)xf * a.ksize + i];
    const uintptr_t lo = (uintptr_t)a.in, hi = lo + (size_t)a.in_w * a.in_h * C;
    const int nd_max = (span + 6) >> 2;   // dwords that cover `span` bytes from any misalignment
    for (int idx = threadIdx.x; idx < rows * nd_max; idx += 256) {
        const int r = idx / nd_max, j = idx - r * nd_max;
        const uintptr_t base = lo + ((size_t)(y0 + r) * a.in_w + x0) * C;
        const uintptr_t p = (base & ~(uintptr_t)3) + 4 * (uintptr_t)j;
        if (p >= base + span) continue;
        uint32_t v = 0;
        if (p >= lo && p + 4 <= hi) {
            v = *(const uint32_t*)p;
        } else {
#pragma unroll
            for (int b = 0; b < 4; b++)
                if (p + b >= lo && p + b < hi) v |= (uint32_t)(*(const uint8_t*)(p + b)) << (8 * b);
        }
        *(uint32_t*)&tile[r][4 * j] = v;
    }
    __syncthreads();
    const int col = threadIdx.x & 63, rg = threadIdx.x >> 6;
    if (col >= cols) return;
    const int x = xf + col;
    int xmin = a.bounds[2 * x], n = resample_taps(xmin, a.bounds[2 * x + 1], a.ksize, a.in_w);
    if (xmin < x0 || xmin + n > x1) n = 0;   // a window outside the staged span
    if (n == 0) xmin = x0;
    const int32_t* k = kc + col * a.ksize;
    const uint8_t* p0;
    const uint8_t* p1;
    {
        const int r0 = rg, r1 = rg + GHR_RESAMPLE_HR / 2;   // a row past the image reads LDS nobody wrote and is not stored
        const uintptr_t b0 = lo + ((size_t)(y0 + r0) * a.in_w + x0) * C, b1 = lo + ((size_t)(y0 + r1) * a.in_w + x0) * C;
        p0 = &tile[r0][(int)(b0 & 3) + (xmin - x0) * C];
        p1 = &tile[r1][(int)(b1 & 3) + (xmin - x0) * C];
    }
    int32_t acc0[C], acc1[C];
#pragma unroll
    for (int c = 0; c < C; c++) acc0[c] = acc1[c] = 1 << (GHR_RESAMPLE_BITS - 1);
    for (int i = 0; i < n; i++) {
        const int32_t kk = k[i];
#pragma unroll
        for (int c = 0; c < C; c++) {
            acc0[c] += (int32_t)p0[i * C + c] * kk;
            acc1[c] += (int32_t)p1[i * C + c] * kk;
        }
    }
    if (rg < rows) {
        uint8_t* dst = a.out + ((size_t)(y0 + rg) * a.out_w + x) * C;
#pragma unroll
        for (int c = 0; c < C; c++) dst[c] = resample_clip8(acc0[c]);
    }
    if (rg + GHR_RESAMPLE_HR / 2 < rows) {
        uint8_t* dst = a.out + ((size_t)(y0 + rg + GHR_RESAMPLE_HR / 2) * a.out_w + x) * C;
#pragma unroll
        for (int c = 0; c < C; c++) dst[c] = resample_clip8(acc1[c]);
    }
}

// VEC: the row length is a multiple of four bytes and both buffers are 4-byte aligned, so every thread's four bytes are one
// aligned dword in every source row.  Otherwise (53 * 3 = 159 bytes a row) the bytes go one by one.
template <bool VEC>
__global__ __launch_bounds__(256) void k_resample_u8_v(ResampleArgs a)
{
    const size_t row = (size_t)a.in_w * a.channels;
    const size_t b = ((size_t)blockIdx.y * 256 + threadIdx.x) * 4;
    const int y = blockIdx.x;
    if (b >= row) return;
    const int n = resample_taps(a.bounds[2 * y], a.bounds[2 * y + 1], a.ksize, a.in_h), ymin = n ? a.bounds[2 * y] : 0;
    const int32_t* __restrict__ k = a.coef + (size_t)y * a.ksize;
    const uint8_t* __restrict__ src = a.in + (size_t)ymin * row + b;
    uint8_t* dst = a.out + (size_t)y * row + b;
    int32_t acc[4];
#pragma unroll
    for (int j = 0; j < 4; j++) acc[j] = 1 << (GHR_RESAMPLE_BITS - 1);
    if (VEC) {
        for (int i = 0; i < n; i++) {
            const int32_t kk = k[i];
            const uint32_t v = *(const uint32_t*)(src + (size_t)i * row);
#pragma unroll
            for (int j = 0; j < 4; j++) acc[j] += (int32_t)((v >> (8 * j)) & 255u) * kk;
        }
        uint32_t o = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) o |= (uint32_t)resample_clip8(acc[j]) << (8 * j);
        *(uint32_t*)dst = o;
    } else {
        const int m = row - b < 4 ? (int)(row - b) : 4;
        for (int i = 0; i < n; i++) {
            const int32_t kk = k[i];
            const uint8_t* p = src + (size_t)i * row;
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (j < m) acc[j] += (int32_t)p[j] * kk;
        }
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (j < m) dst[j] = resample_clip8(acc[j]);
    }
}

// ---- assembly ----------------------------------------------------------------------------------------------------------------

// camera_utils.py:73-75: (m / 255 >= 0.5) is m >= 128 (127 / 255 < 0.5 < 128 / 255); otherwise the host's m / 255
GHR_HD float gt_mask_value(uint8_t m, const float* div255, int binarize) { return binarize ? (m >= 128 ? 1.f : 0.f) : div255[m]; }

// cameras.py:64: image * body + white_background * (1 - body), white 0 or 1
GHR_HD float gt_image_value(float v, float body, float white) { return v * body + white * (1.f - body); }

// cameras.py:55 on PILtoTorch(..., max_value=180)
GHR_HD float gt_angle_value(uint8_t a, const float* div180) { return fminf(fmaxf(div180[a], 0.f), 1.f); }

// The source cell of F.interpolate(mode='bilinear', align_corners=False) along one axis, in float32: index, upper neighbour
// (clamped) and the two weights.
GHR_HD void gt_lerp_coord(int dst, int in_size, int out_size, int* i0, int* i1, float* w0, float* w1)
{
    const float scale = (float)in_size / (float)out_size;
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    int i = (int)src;
    if (i > in_size - 1) i = in_size - 1;
    const float l = fminf(fmaxf(src - (float)i, 0.f), 1.f);
    *i0 = i;
    *i1 = i + (i < in_size - 1 ? 1 : 0);
    *w1 = l;
    *w0 = 1.f - l;
}

// camera_utils.py:67: the variance map [vh][vw] (the float16 of the reference's file when via_half) sampled at pixel (x, y) of
// W x H.  At equal sizes both lambdas are 0 and the sample is the map's own value.
GHR_HD float gt_var_sample(const float* var, int vw, int vh, int W, int H, int x, int y, int via_half)
{
    int x0, x1, y0, y1;
    float hx, lx, hy, ly;
    gt_lerp_coord(x, vw, W, &x0, &x1, &hx, &lx);
    gt_lerp_coord(y, vh, H, &y0, &y1, &hy, &ly);
    float a = var[(size_t)y0 * vw + x0], b = var[(size_t)y0 * vw + x1], c = var[(size_t)y1 * vw + x0], d = var[(size_t)y1 * vw + x1];
    if (via_half) { a = (float)(_Float16)a; b = (float)(_Float16)b; c = (float)(_Float16)c; d = (float)(_Float16)d; }
    return hy * (hx * a + lx * b) + ly * (hx * c + lx * d);
}

struct GtAssembleArgs {
    int W, H;
    const uint8_t* image;      // [H][W][3]
    const uint8_t* mask_hair;  // [H][W]
    const uint8_t* mask_body;  // [H][W]
    const uint8_t* angle;      // [H][W] or NULL
    const float* var;          // [var_h][var_w] or NULL
    int var_w, var_h;
    const float* div255;       // [256]: i / 255 as the host divides
    const float* div180;       // [256]: i / 180
    int white, binarize, via_half;
    float* out_image;          // [3][H][W]
    float* out_mask;           // [2][H][W]: hair, body
    float* out_angle;          // [1][H][W] or NULL
    float* out_conf;           // [1][H][W] or NULL
};

// image, mask_hair, mask_body of one pixel from its five bytes: what k_gt_assemble and k_gt_from_render share
struct GtPix { float image[3], hair, body; };
GHR_HD GtPix gt_assemble_pixel(const uint8_t* rgb, uint8_t hair, uint8_t body, const float* div255, int binarize, float white)
{
    GtPix o;
    o.hair = gt_mask_value(hair, div255, binarize);
    o.body = gt_mask_value(body, div255, binarize);
#pragma unroll
    for (int c = 0; c < 3; c++) o.image[c] = gt_image_value(div255[rgb[c]], o.body, white);
    return o;
}

__global__ __launch_bounds__(256) void k_gt_assemble(GtAssembleArgs a)
{
    const size_t N = (size_t)a.W * a.H;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    const uint8_t rgb[3] = {a.image[3 * p], a.image[3 * p + 1], a.image[3 * p + 2]};
    const GtPix o = gt_assemble_pixel(rgb, a.mask_hair[p], a.mask_body[p], a.div255, a.binarize, a.white ? 1.f : 0.f);
#pragma unroll
    for (int c = 0; c < 3; c++) a.out_image[c * N + p] = o.image[c];
    a.out_mask[p] = o.hair;
    a.out_mask[N + p] = o.body;
    if (a.angle) a.out_angle[p] = gt_angle_value(a.angle[p], a.div180);
    if (a.var) {
        const int y = (int)(p / a.W), x = (int)(p - (size_t)y * a.W);
        a.out_conf[p] = orient_conf_of(gt_var_sample(a.var, a.var_w, a.var_h, a.W, a.H, x, y, a.via_half), 0);
    }
}

__global__ __launch_bounds__(256) void k_gt_resize_var(int W, int H, const float* var, int vw, int vh, int via_half, float* out)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)W * H) return;
    const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
    out[p] = gt_var_sample(var, vw, vh, W, H, x, y, via_half);
}

// ---- synthetic ground truth --------------------------------------------------------------------------------------------------

// One pixel of camera_utils.py:51-64 + cameras.py:51-64 at -r 1.  render_set quantises render, hair mask, head mask and
// angle * hair to bytes (product_core) and saves orient_conf * hair as a float; loadCam reads every PNG back through PILtoTorch's
// default max_value: byte / 255, the angle too (the clamp of cameras.py:55 holds for every table value); the confidence goes
// through F.interpolate alone, which at equal size returns the plane's own (finite) values.
struct GtSynthPix { GtPix v; float angle, conf; };
GHR_HD GtSynthPix gt_from_render_pixel(const float* rgb, float m0, float m1, float d0, float d1, float conf, const float* div255,
                                       int binarize, float white)
{
    const ProductCore k = product_core(rgb, m0, m1, d0, d1, conf);
    const uint8_t b[3] = {(uint8_t)k.render[0], (uint8_t)k.render[1], (uint8_t)k.render[2]};
    GtSynthPix o;
    o.v = gt_assemble_pixel(b, (uint8_t)k.hair, (uint8_t)k.head, div255, binarize, white);
    o.angle = div255[k.orient];
    o.conf = k.conf;
    return o;
}

struct GtFromRenderArgs {
    int W, H;
    const float* renders;  // [10,H,W] packed: rgb 0-2, hair 3, head 4, dir2d 5-6, orientation confidence 8
    const float* div255;   // [256]
    int white, binarize;
    float* out_image;      // [3][H][W]
    float* out_mask;       // [2][H][W]: hair, body
    float* out_angle;      // [1][H][W]
    float* out_conf;       // [1][H][W]
};

// grid ceil(ceil(H W / 4) / 256), block 256; a thread makes four consecutive pixels: eight planes in, seven out, 60 B a pixel.
// VEC (H*W % 4 == 0, every pointer 16-B aligned): float4 loads and stores; otherwise single ones with the end checked.  The table
// is staged in LDS: six look-ups per pixel at addresses the render decides.
template <bool VEC>
__global__ __launch_bounds__(256) void k_gt_from_render(GtFromRenderArgs a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ float s_div255[256];
    s_div255[threadIdx.x] = a.div255[threadIdx.x];
    __syncthreads();
    const size_t N = (size_t)a.W * a.H, quads = (N + 3) / 4;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= quads) return;
    const size_t p0 = 4 * q;
    float r[8][4];
#pragma unroll
    for (int k = 0; k < 7; k++) load_quad<VEC>(a.renders + (size_t)k * N, p0, N, r[k]);
    load_quad<VEC>(a.renders + (size_t)8 * N, p0, N, r[7]);
    const float white = a.white ? 1.f : 0.f;
    float o[7][4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float rgb[3] = {r[0][j], r[1][j], r[2][j]};
        const GtSynthPix g = gt_from_render_pixel(rgb, r[3][j], r[4][j], r[5][j], r[6][j], r[7][j], s_div255, a.binarize, white);
        o[0][j] = g.v.image[0]; o[1][j] = g.v.image[1]; o[2][j] = g.v.image[2];
        o[3][j] = g.v.hair; o[4][j] = g.v.body;
        o[5][j] = g.angle; o[6][j] = g.conf;
    }
    float* dst[7] = {a.out_image, a.out_image + N, a.out_image + 2 * N, a.out_mask, a.out_mask + N, a.out_angle, a.out_conf};
#pragma unroll
    for (int k = 0; k < 7; k++) {
        if (VEC) {
            *reinterpret_cast<f4*>(dst[k] + p0) = f4{o[k][0], o[k][1], o[k][2], o[k][3]};
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (p0 + j < N) dst[k][p0 + j] = o[k][j];
        }
    }
#endif
}

}  // namespace ghr
