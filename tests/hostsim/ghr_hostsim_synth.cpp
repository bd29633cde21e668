// ghr_hostsim_synth.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Runs the synthetic ground truth's own `__host__ __device__` per-pixel function (gaussianhaircut_amd/csrc/ghr_gt.h:
// gt_from_render_pixel, on product_core of ghr_products.h and gt_assemble_pixel) over a packed render on the CPU, with the
// plane layout of ghr_gt_from_render, so that the `-m "not gpu"` suite compares the kernel's arithmetic with the comparator
// and the float64 model before any GPU time is spent.  The float4 form, the LDS copy of the table and the launch are covered
// by the `-m gpu` tests.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ghr.h"
#include "../../gaussianhaircut_amd/csrc/ghr_gt.h"

extern "C" {

// renders [10][H][W]; out_image [3][H][W], out_mask [2][H][W], out_angle [H][W], out_conf [H][W]
void ghrsim_gt_from_render(int W, int H, const float* renders, const float* div255, int white, int binarize, float* out_image,
                           float* out_mask, float* out_angle, float* out_conf)
{
    const size_t N = (size_t)W * H;
    for (size_t p = 0; p < N; p++) {
        const float rgb[3] = {renders[p], renders[N + p], renders[2 * N + p]};
        const ghr::GtSynthPix o = ghr::gt_from_render_pixel(rgb, renders[3 * N + p], renders[4 * N + p], renders[5 * N + p],
                                                            renders[6 * N + p], renders[8 * N + p], div255, binarize, white ? 1.f : 0.f);
        for (int c = 0; c < 3; c++) out_image[c * N + p] = o.v.image[c];
        out_mask[p] = o.v.hair;
        out_mask[N + p] = o.v.body;
        out_angle[p] = o.angle;
        out_conf[p] = o.conf;
    }
}

}  // extern "C"
