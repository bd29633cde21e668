// ghr_hostsim_latent.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Runs the latent-strand stage's own `__host__ __device__` functions (gaussianhaircut_amd/csrc/ghr_latent.h: points_seg_fwd,
// points_point_bwd, rows_reduce_one, latent_pixel_fwd / latent_pixel_bwd, latent_fold_finish, latent_bwd_factors) sequentially on
// the CPU with the bookkeeping of their kernels -- a thread's four pixels in pixel order, the 256-thread tree, the fold's strided
// slots -- so that the `-m "not gpu"` suite compares the arithmetic with the reference's golden before any GPU time is spent.
// Launch geometry, LDS staging and the float4 form are covered by the `-m gpu` tests.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/ghr.h"
#include "../../gaussianhaircut_amd/csrc/ghr_latent.h"

namespace {
// latent_block_tree on the host: v[k][t] += v[k][t + st], st = 128 ... 1
void tree(float (*v)[GHR_LATENT_BLOCK], float* out)
{
    for (int st = GHR_LATENT_BLOCK / 2; st >= 1; st >>= 1)
        for (int t = 0; t < st; t++)
            for (int k = 0; k < GHR_LATENT_TERMS; k++) v[k][t] = v[k][t] + v[k][t + st];
    for (int k = 0; k < GHR_LATENT_TERMS; k++) out[k] = v[k][0];
}
}  // namespace

extern "C" {

void ghrsim_points_build(int S, int L, const float* p, float scale, float* xyz, float* rot, float* scaling, float* dir)
{
    const int n_seg = L - 1;
    for (int s = 0; s < S; s++)
        for (int k = 0; k < n_seg; k++) {
            const size_t r = (size_t)s * n_seg + k;
            const float* a = p + ((size_t)s * L + k) * 3;
            ghr::points_seg_fwd(a, a + 3, scale, xyz + 3 * r, dir + 3 * r, rot + 4 * r, scaling + 3 * r);
        }
}

void ghrsim_points_build_backward(int S, int L, const float* p, const float* d_xyz, const float* d_rot, const float* d_scaling,
                                  const float* d_dir, float* d_p)
{
    for (int s = 0; s < S; s++) {
        const size_t row0 = (size_t)s * (L - 1);
        for (int j = 0; j < L; j++)
            ghr::points_point_bwd(p + (size_t)3 * s * L, j, L, d_xyz ? d_xyz + 3 * row0 : nullptr, d_rot ? d_rot + 4 * row0 : nullptr,
                                  d_scaling ? d_scaling + 3 * row0 : nullptr, d_dir ? d_dir + 3 * row0 : nullptr,
                                  d_p + ((size_t)s * L + j) * 3);
    }
}

void ghrsim_rows_expand(int S, int n_seg, int C, const float* src, float* dst)
{
    for (size_t i = 0; i < (size_t)S * n_seg * C; i++) dst[i] = src[(i / C / n_seg) * C + i % C];
}

void ghrsim_rows_reduce(int S, int n_seg, int C, const float* g, float* out)
{
    for (int s = 0; s < S; s++)
        for (int c = 0; c < C; c++) out[(size_t)s * C + c] = ghr::rows_reduce_one(g + (size_t)s * n_seg * C + c, n_seg, C);
}

size_t ghrsim_latent_loss_sums_floats(int W, int H)
{
    const size_t per = (size_t)GHR_LATENT_BLOCK * GHR_LATENT_QUAD;
    return GHR_LATENT_AUX + GHR_LATENT_TERMS * (((size_t)W * H + per - 1) / per);
}

void ghrsim_latent_loss_forward(const ghr_latent_loss_args* l, float* sums, float* loss_out)
{
    const size_t N = (size_t)l->W * l->H, per = (size_t)GHR_LATENT_BLOCK * GHR_LATENT_QUAD;
    const size_t wgs = (N + per - 1) / per;
    for (size_t b = 0; b < wgs; b++) {
        static float v[GHR_LATENT_TERMS][GHR_LATENT_BLOCK];
        for (int t = 0; t < GHR_LATENT_BLOCK; t++) {
            float s[4] = {0.f, 0.f, 0.f, 0.f};
            for (int q = 0; q < GHR_LATENT_QUAD; q++) {
                const size_t p = (b * GHR_LATENT_BLOCK + t) * GHR_LATENT_QUAD + q;
                if (p >= N) break;
                const float im[3] = {l->image[p], l->image[N + p], l->image[2 * N + p]};
                const float gt[3] = {l->gt_image[p], l->gt_image[N + p], l->gt_image[2 * N + p]};
                const ghr::LatentPix o = ghr::latent_pixel_fwd(im, gt, l->mask0[p], l->gt_mask0[p], l->dir2d[p], l->dir2d[N + p],
                                                               l->orient_conf != nullptr, l->orient_conf ? l->orient_conf[p] : 1.0f,
                                                               l->gt_orient_angle[p], l->gt_orient_conf ? l->gt_orient_conf[p] : 1.0f);
                s[0] += o.l1; s[1] += o.ce; s[2] += o.orn; s[3] += o.ord;
            }
            for (int k = 0; k < 4; k++) v[k][t] = s[k];
        }
        tree(v, sums + GHR_LATENT_AUX + b * GHR_LATENT_TERMS);
    }
    static float v[GHR_LATENT_TERMS][GHR_LATENT_BLOCK];
    for (int t = 0; t < GHR_LATENT_BLOCK; t++) {
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (size_t i = t; i < wgs; i += GHR_LATENT_BLOCK)
            for (int k = 0; k < 4; k++) s[k] += sums[GHR_LATENT_AUX + i * GHR_LATENT_TERMS + k];
        for (int k = 0; k < 4; k++) v[k][t] = s[k];
    }
    float tot[4];
    tree(v, tot);
    const double t[4] = {(double)tot[0], (double)tot[1], (double)tot[2], (double)tot[3]};
    ghr::latent_fold_finish(t, (double)l->W * (double)l->H, l->w_l1, l->w_mask, l->w_orient, sums, loss_out);
}

void ghrsim_latent_loss_backward(const ghr_latent_loss_args* l, const float* sums, const float* grad_loss, float* d_packed)
{
    const size_t N = (size_t)l->W * l->H;
    float k[3];
    ghr::latent_bwd_factors(sums, grad_loss ? grad_loss[0] : 1.0f, (double)l->W * (double)l->H, l->w_l1, l->w_mask, l->w_orient, k);
    const bool or_on = k[2] != 0.f;
    static const int plane[7] = {0, 1, 2, 3, 5, 6, 8};
    for (size_t p = 0; p < N; p++) {
        const float im[3] = {l->image[p], l->image[N + p], l->image[2 * N + p]};
        const float gt[3] = {l->gt_image[p], l->gt_image[N + p], l->gt_image[2 * N + p]};
        float o[7];
        ghr::latent_pixel_bwd(im, gt, l->mask0[p], l->gt_mask0[p], or_on ? l->dir2d[p] : 1.f, or_on ? l->dir2d[N + p] : 1.f,
                              l->orient_conf != nullptr, (or_on && l->orient_conf) ? l->orient_conf[p] : 1.0f,
                              or_on ? l->gt_orient_angle[p] : 1.f, (or_on && l->gt_orient_conf) ? l->gt_orient_conf[p] : 1.0f, or_on,
                              k[0], k[1], k[2], o);
        for (int c = 0; c < 10; c++) d_packed[c * N + p] = 0.f;
        for (int c = 0; c < 7; c++) d_packed[plane[c] * N + p] = o[c];
    }
}

}  // extern "C"
