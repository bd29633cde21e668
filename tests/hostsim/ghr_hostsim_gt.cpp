// ghr_hostsim_gt.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Runs the ground-truth loader's own `__host__ __device__` functions (gaussianhaircut_amd/csrc/ghr_gt.h: resample_tap_sum and
// resample_clip8; gt_mask_value, gt_image_value, gt_angle_value, gt_var_sample over gt_lerp_coord; orient_conf_of of
// ghr_orient.h) over an image on the CPU, so that the `-m "not gpu"` suite compares the kernels' arithmetic with the reference's
// golden before any GPU time is spent.  The kernels' indexing, the four-byte form of the vertical pass and the launch geometry are
// covered by the `-m gpu` tests.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/ghr.h"
#include "../../gaussianhaircut_amd/csrc/ghr_gt.h"

extern "C" {

// Both passes in Pillow's order with the uint8 intermediate; bounds / coef of an axis may be NULL when its sizes are equal.
void ghrsim_resample_u8(int in_w, int in_h, int C, const uint8_t* in, int out_w, int out_h, uint8_t* out, const int32_t* bx,
                        const int32_t* cx, int kx, const int32_t* by, const int32_t* cy, int ky)
{
    std::vector<uint8_t> mid;
    const uint8_t* src = in;
    if (in_w != out_w) {
        mid.resize((size_t)in_h * out_w * C);
        for (int y = 0; y < in_h; y++)
            for (int x = 0; x < out_w; x++)
                for (int c = 0; c < C; c++)
                    mid[((size_t)y * out_w + x) * C + c] =
                        ghr::resample_tap_sum(in + ((size_t)y * in_w + bx[2 * x]) * C + c, (size_t)C, bx[2 * x + 1], cx + (size_t)x * kx);
        src = mid.data();
    }
    const size_t row = (size_t)out_w * C;
    for (int y = 0; y < out_h; y++)
        for (size_t b = 0; b < row; b++)
            out[(size_t)y * row + b] = in_h != out_h ? ghr::resample_tap_sum(src + (size_t)by[2 * y] * row + b, row, by[2 * y + 1], cy + (size_t)y * ky)
                                                     : src[(size_t)y * row + b];
}

// the per-pixel body of k_gt_assemble; angle / var (and their outputs) may be NULL
void ghrsim_gt_assemble(int W, int H, const uint8_t* image, const uint8_t* hair, const uint8_t* body, const uint8_t* angle,
                        const float* var, int vw, int vh, const float* t255, const float* t180, int white, int binarize, int via_half,
                        float* o_image, float* o_mask, float* o_angle, float* o_conf, float* o_var)
{
    const size_t N = (size_t)W * H;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t p = (size_t)y * W + x;
            const float mh = ghr::gt_mask_value(hair[p], t255, binarize), mb = ghr::gt_mask_value(body[p], t255, binarize);
            for (int c = 0; c < 3; c++) o_image[c * N + p] = ghr::gt_image_value(t255[image[3 * p + c]], mb, white ? 1.f : 0.f);
            o_mask[p] = mh;
            o_mask[N + p] = mb;
            if (angle) o_angle[p] = ghr::gt_angle_value(angle[p], t180);
            if (var) {
                const float v = ghr::gt_var_sample(var, vw, vh, W, H, x, y, via_half);
                o_conf[p] = ghr::orient_conf_of(v, 0);
                if (o_var) o_var[p] = v;
            }
        }
}

}  // extern "C"
