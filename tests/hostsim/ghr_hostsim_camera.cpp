// ghr_hostsim_camera.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Runs the camera bank's own `__host__ __device__` per-camera functions (gaussianhaircut_amd/csrc/ghr_camera.h: cam_compose_row,
// cam_compose_bwd_row, cam_adam_row) sequentially on the CPU with the row bookkeeping of k_cam_compose / k_cam_compose_bwd /
// k_cam_adam, so that the `-m "not gpu"` suite compares the kernels' arithmetic with the reference's golden before any GPU time
// is spent.  The barrier of k_cam_adam and the launch geometry are covered by the `-m gpu` tests.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/ghr.h"
#include "../../gaussianhaircut_amd/csrc/ghr_camera.h"

extern "C" {

void ghrsim_cam_compose(int param, int first, int n, const float* cst, int cst_stride, const float* par, int par_stride, float* out,
                        int out_stride)
{
    for (int r = 0; r < n; r++)
        ghr::cam_compose_row(param, cst + (size_t)(first + r) * cst_stride, par + (size_t)(first + r) * par_stride,
                             out + (size_t)r * out_stride);
}

void ghrsim_cam_compose_bwd(int param, int first, int n, const float* cst, int cst_stride, const float* par, int par_stride,
                            const float* d_view, const float* d_full, const float* d_proj, const float* d_center, const float* d_fovx,
                            const float* d_fovy, float* grads, int grad_stride, int* touched, int train_mask)
{
    const int rd = ghr::cam_rot_dim(param), W = ghr::cam_row(param);
    for (int r = 0; r < n; r++) {
        const size_t row = (size_t)(first + r);
        float g[11];
        ghr::cam_compose_bwd_row(param, cst + row * cst_stride, par + row * par_stride, d_view ? d_view + 16 * r : nullptr,
                                 d_full ? d_full + 16 * r : nullptr, d_proj ? d_proj + 16 * r : nullptr,
                                 d_center ? d_center + 3 * r : nullptr, d_fovx ? d_fovx + r : nullptr, d_fovy ? d_fovy + r : nullptr, g);
        float* dst = grads + row * grad_stride;
        const bool add = touched[row] != 0;
        for (int k = 0; k < W; k++) {
            const bool on = (train_mask & (k >= rd + 3 ? GHR_CAM_TRAIN_FOV : GHR_CAM_TRAIN_POSE)) != 0;
            if (on) dst[k] = add ? dst[k] + g[k] : g[k];
            else if (!add) dst[k] = 0.f;
        }
        touched[row] = 1;
    }
}

void ghrsim_cam_adam(int param, int n, float* p, float* g, float* m, float* v, int stride, int* steps, int* touched, float lr_rot,
                     float lr_trans, float lr_fov, double beta1, double beta2, float eps, int train_mask)
{
    const int rd = ghr::cam_rot_dim(param), W = ghr::cam_row(param);
    int bad = 0;
    for (int r = 0; r < n; r++) {
        if (!touched[r]) continue;
        for (int k = 0; k < W; k++) {
            const bool on = (train_mask & (k >= rd + 3 ? GHR_CAM_TRAIN_FOV : GHR_CAM_TRAIN_POSE)) != 0;
            const float x = g[(size_t)r * stride + k];
            bad |= (on && x != x) ? 1 : 0;
        }
    }
    for (int r = 0; r < n; r++) {
        if (!touched[r]) continue;
        const size_t o = (size_t)r * stride;
        if (!bad) {
            steps[r] += 1;
            ghr::cam_adam_row(param, p + o, g + o, m + o, v + o, steps[r], lr_rot, lr_trans, lr_fov, beta1, beta2, eps, train_mask);
        }
        for (int k = 0; k < W; k++) g[o + k] = 0.f;
        touched[r] = 0;
    }
}

}  // extern "C"
