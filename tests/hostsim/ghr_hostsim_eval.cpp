// ghr_hostsim_eval.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Runs the evaluation pass's own `__host__ __device__` per-pixel functions (gaussianhaircut_amd/csrc/ghr_eval.h: eval_pixel,
// product_pixel) over an image on the CPU, with the table row of k_eval_finalize and the block layout of k_eval_products, so
// that the `-m "not gpu"` suite compares the kernels' arithmetic with the reference's golden before any GPU time is spent.
// The SSIM window, the slots and their fold, and the float4 forms are covered by the `-m gpu` tests.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/ghr.h"
#include "../../gaussianhaircut_amd/csrc/ghr_eval.h"

extern "C" {

// row: GHR_EVAL_TERMS doubles {l1, ce, or_num, or_den, mse[3], ssim = 0}; gt_angle / gt_oconf may be NULL (both)
void ghrsim_eval_metrics(int W, int H, const float* renders, const float* gt_image, const float* gt_mask, const float* gt_angle,
                         const float* gt_oconf, double* row)
{
    const size_t N = (size_t)W * H;
    const bool orient = gt_angle != nullptr && gt_oconf != nullptr;
    double s[GHR_EVAL_TERMS] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t p = 0; p < N; p++) {
        ghr::EvalIn in;
        for (int c = 0; c < 3; c++) { in.r[c] = renders[c * N + p]; in.g[c] = gt_image[c * N + p]; }
        for (int c = 0; c < 2; c++) { in.m[c] = renders[(3 + c) * N + p]; in.gm[c] = gt_mask[c * N + p]; }
        in.d0 = renders[5 * N + p]; in.d1 = renders[6 * N + p];
        in.ga = orient ? gt_angle[p] : 0.f;
        in.gw = orient ? gt_oconf[p] : 0.f;
        const ghr::EvalPix e = ghr::eval_pixel(in, orient);
        for (int k = 0; k < GHR_EVAL_POINT_TERMS; k++) s[k] += (double)e.t[k];
    }
    const double n = (double)N;
    const double div[GHR_EVAL_TERMS] = {3.0 * n, 2.0 * n, 1.0, 1.0, n, n, n, 3.0 * n};
    for (int k = 0; k < GHR_EVAL_TERMS; k++) row[k] = s[k] / div[k];
}

// bytes: 12 H W, conf: H W (the layout of ghr_eval_products)
void ghrsim_eval_products(int W, int H, const float* renders, uint8_t* bytes, float* conf)
{
    const size_t N = (size_t)W * H;
    for (size_t p = 0; p < N; p++) {
        const float rgb[3] = {renders[p], renders[N + p], renders[2 * N + p]};
        const ghr::ProductPix o = ghr::product_pixel(rgb, renders[3 * N + p], renders[4 * N + p], renders[5 * N + p],
                                                     renders[6 * N + p], renders[8 * N + p]);
        for (int c = 0; c < 3; c++) {
            bytes[3 * p + c] = (uint8_t)o.render[c];
            bytes[6 * N + 3 * p + c] = (uint8_t)o.orient_vis[c];
            bytes[9 * N + 3 * p + c] = (uint8_t)o.conf_vis[c];
        }
        bytes[3 * N + p] = (uint8_t)o.hair;
        bytes[4 * N + p] = (uint8_t)o.head;
        bytes[5 * N + p] = (uint8_t)o.orient;
        conf[p] = o.conf;
    }
}

}  // extern "C"
