// ghr_hostsim_orient.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Runs the orientation pass's own `__host__ __device__` functions (gaussianhaircut_amd/csrc/ghr_orient.h: orient_grey,
// dog_tap_sum through dog_axis0 / dog_axis1, orient_pick and the functions it composes, orient_conf_of) over an image on the
// CPU, so that the `-m "not gpu"` suite compares the kernels' arithmetic with the reference's golden before any GPU time is
// spent.  The responses are formed as the matrix unit forms them: one fmaf per tap, taps ascending.  The LDS gather, the fragment
// order of the weights and the fold over lanes and waves are covered by the `-m gpu` tests.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/ghr.h"
#include "../../gaussianhaircut_amd/csrc/ghr_orient.h"

extern "C" {

// scratch: 2 W H doubles; filtered: W H floats
void ghrsim_orient_dog(int W, int H, int channels, int is_u8, const void* image, int r_low, const double* w_low, int r_high,
                       const double* w_high, double* scratch, float* filtered)
{
    ghr::OrientDogArgs a{W, H, channels, is_u8, image, r_low, r_high, w_low, w_high, scratch, filtered};
    const size_t N = (size_t)W * H;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) ghr::dog_axis0(a, x, y, &scratch[(size_t)y * W + x], &scratch[N + (size_t)y * W + x]);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) filtered[(size_t)y * W + x] = ghr::dog_axis1(a, x, y);
}

// weights [F][K][K], thetas [F]; deg int32 [H W], var / conf float [H W] (conf may be NULL)
void ghrsim_orient_gabor(int W, int H, const float* plane, int n_filters, int K, const float* weights, const float* thetas,
                         int32_t* deg, float* var, float* conf, int via_half)
{
    const int R = K / 2;
    std::vector<float> resp((size_t)n_filters);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            for (int k = 0; k < n_filters; k++) {
                float acc = 0.f;
                for (int t = 0; t < K * K; t++) {
                    const int yy = y + t / K - R, xx = x + t % K - R;
                    const float v = (xx >= 0 && xx < W && yy >= 0 && yy < H) ? plane[(size_t)yy * W + xx] : 0.f;
                    acc = fmaf(weights[(size_t)k * K * K + t], v, acc);
                }
                resp[k] = acc;
            }
            const size_t p = (size_t)y * W + x;
            int d;
            ghr::orient_pick(resp.data(), n_filters, thetas, &d, &var[p]);
            deg[p] = d;
            if (conf) conf[p] = ghr::orient_conf_of(var[p], via_half);
        }
}

}  // extern "C"
