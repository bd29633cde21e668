// ghr_products.h -- the per-pixel functions of the render products: what render_set makes of one pixel of the packed [10,H,W]
// rasterizer output.  No kernels here: ghr_eval.h (k_eval_products, the writer's side) and ghr_gt.h (k_gt_from_render, the
// reader's side of the same hand-off) both build on them, and each stays includable without the other's kernels.
//
// Reference: src/gaussian_renderer/__init__.py:100-105 (the orientation angle), src/render_gaussians.py:31-68 (render_set),
// src/utils/image_utils.py:22-37 (vis_orient), torchvision.utils.save_image (the 8-bit quantisation).
#pragma once
#include "ghr_device.h"

namespace ghr {

GHR_HD float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// Orientation angle / pi in (0, 1) of a rendered 2D strand direction (src/gaussian_renderer/__init__.py:100-105): the
// normalise / mirror / clamp / acos chain of orient_pixel (ghr_loss.h), operation for operation.
GHR_HD float orient_angle_of(float d0, float d1)
{
    const float INV_PI = 0.31830988618379067154f;
    const float nrm = fast_sqrt(d0 * d0 + d1 * d1);
    const float den = fmaxf(nrm, 1e-12f);  // F.normalize(dim=0), eps = 1e-12
    const float iden = fast_rcp(den);
    const float u0 = d0 * iden, u1 = d1 * iden;
    const float mirror = u0 < 0.f ? -1.f : 1.f;
    const float lo = -1.f + 1e-3f, hi = 1.f - 1e-3f;
    const float uc = fminf(hi, fmaxf(lo, u1));
    return acosf(uc * mirror) * INV_PI;
}

// torchvision.utils.save_image: mul(255).add_(0.5).clamp_(0, 255).to(uint8)
GHR_HD uint32_t quant8(float v) { return (uint32_t)fminf(fmaxf(v * 255.f + 0.5f, 0.f), 255.f); }

// image_utils.py:22-37: the four colour ramps over the angle in degrees, BGR, swapped to RGB, times `mask`
GHR_HD void vis_orient_pixel(float angle, float mask, float* rgb)
{
    const float deg = angle * 180.f;
    const float red = clamp01(1.f - fabsf(deg - 0.f) / 45.f) + clamp01(1.f - fabsf(deg - 180.f) / 45.f);
    const float green = clamp01(1.f - fabsf(deg - 90.f) / 45.f);
    const float magenta = clamp01(1.f - fabsf(deg - 45.f) / 45.f);
    const float teal = clamp01(1.f - fabsf(deg - 135.f) / 45.f);
    rgb[0] = (red + magenta) * mask;  // bgr[2]
    rgb[1] = (green + teal) * mask;   // bgr[1]
    rgb[2] = (magenta + teal) * mask; // bgr[0]
}

// The five products the strand stages read back (camera_utils.py:51-64) and the angle the two colourings are made from
struct ProductCore {
    uint32_t render[3], hair, head, orient;  // 8-bit levels
    float conf;                              // orient_conf * hair: the reference's .pth product
    float angle;                             // before the mask and the quantisation
};
GHR_HD ProductCore product_core(const float* r, float m0, float m1, float d0, float d1, float conf)
{
    ProductCore o;
#pragma unroll
    for (int c = 0; c < 3; c++) o.render[c] = quant8(r[c]);
    o.hair = quant8(m0);
    o.head = quant8(m1);
    o.angle = orient_angle_of(d0, d1);
    o.orient = quant8(o.angle * m0);
    o.conf = conf * m0;
    return o;
}

struct ProductPix {
    uint32_t render[3], hair, head, orient, orient_vis[3], conf_vis[3];  // 8-bit levels
    float conf;                                                        // orient_conf * hair: the reference's .pth product
};
GHR_HD ProductPix product_pixel(const float* r, float m0, float m1, float d0, float d1, float conf)
{
    const ProductCore k = product_core(r, m0, m1, d0, d1, conf);
    ProductPix o;
#pragma unroll
    for (int c = 0; c < 3; c++) o.render[c] = k.render[c];
    o.hair = k.hair;
    o.head = k.head;
    o.orient = k.orient;
    float v[3];
    vis_orient_pixel(k.angle, m0, v);
#pragma unroll
    for (int c = 0; c < 3; c++) o.orient_vis[c] = quant8(v[c]);
    o.conf = k.conf;
    vis_orient_pixel(k.angle, 1.f - 1.f / (o.conf + 1.f), v);
#pragma unroll
    for (int c = 0; c < 3; c++) o.conf_vis[c] = quant8(v[c]);
    return o;
}

#if defined(__HIP_DEVICE_COMPILE__)
// Four consecutive pixels of a plane: one 16-B load (VEC: H*W % 4 == 0 and a 16-B aligned plane) or four 4-B loads with the
// image's end checked (what lies past it reads 0 and is not used)
template <bool VEC>
__device__ __forceinline__ void load_quad(const float* plane, size_t p0, size_t N, float* v)
{
    if (VEC) {
        const f4 t = *reinterpret_cast<const f4*>(plane + p0);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = p0 + j < N ? plane[p0 + j] : 0.f;
    }
}
#endif

}  // namespace ghr
