// ghr_hostsim_shared.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Runs the `__host__ __device__` functions behind the per-strand SH segment (gaussianhaircut_amd/csrc/ghr_shared.h and the
// row functions of ghr_project.h it calls) sequentially on the CPU, row by row with the bookkeeping of their kernels: the
// ModelArgs whose features_dc points at xyz, the strand's DC term loaded on top, the strand's `rest` block handed to
// project_colour / project_bwd_sh<CAM, false>, then the fold.  Beside them the ORDINARY forms on expanded arrays (project_one,
// project_bwd_one, rows_reduce_one), so that tests/test_shared_features_cpu.py compares the two before any GPU time is spent.
// Launch geometry and LDS staging are covered by the `-m gpu` tests.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/ghr.h"
#include "../../gaussianhaircut_amd/csrc/ghr_latent.h"
#include "../../gaussianhaircut_amd/csrc/ghr_shared.h"

namespace {
ghr::ModelGrads plain_grads(float* d_means2D, float* d_xyz, float* d_ls, float* d_rot, float* d_conf, float* d_dir)
{
    ghr::ModelGrads g;
    std::memset(&g, 0, sizeof(g));
    g.d_means2D = d_means2D; g.d_xyz = d_xyz; g.d_log_scales = d_ls; g.d_rotations = d_rot; g.d_orient_conf_log = d_conf;
    g.d_dir3d = d_dir;
    return g;
}
}  // namespace

extern "C" {

int ghrsim_shared_sizeof(void) { return (int)sizeof(ghr_shared_features); }

// n_seg == 0: the ordinary form, a->features_dc / features_rest are [P,...].  n_seg >= 1: they are [P / n_seg,...].
// out_rec [P][16], out_radii [P], out_means2D [P][3], out_depths [P], out_rects [P][4]
void ghrsim_shared_forward(const ghr::ModelArgs* a_in, int n_seg, float* out_rec, int* out_radii, float* out_means2D,
                           float* out_depths, uint32_t* out_rects)
{
    ghr::ModelArgs a = *a_in;
    const int P = a.P;
    a.gx = (a.W + 15) / 16; a.gy = (a.H + 15) / 16;
    std::vector<ghr::f4> rec((size_t)4 * P, ghr::f4{0, 0, 0, 0});
    a.rec = rec.data(); a.depths = out_depths; a.rects = reinterpret_cast<ghr::rect4*>(out_rects); a.radii = out_radii;
    a.means2D = out_means2D;
    const int row = 3 * (a.sh_coeffs - 1);
    const ghr::SharedFeat sf{n_seg ? P / n_seg : 0, n_seg, a.features_dc, a.features_rest};
    if (n_seg) { a.features_dc = a.xyz; a.features_rest = nullptr; }
    for (int i = 0; i < P; i++) {
        int x0, y0, x1, y1;
        out_depths[i] = 0.f;
        if (!n_seg) {
            ghr::project_one(a, i, sf.rest + (size_t)i * row, x0, y0, x1, y1);
            continue;
        }
        // k_shared_proj_fwd's row (stores as project_one's)
        const int strand = i / n_seg;
        ghr::RawIn in;
        ghr::load_raw(a, i, in);
        for (int c = 0; c < 3; c++) in.dc[c] = sf.dc[3 * (size_t)strand + c];
        ghr::ProjOut o;
        const bool ok = ghr::project_geom(a, in, x0, y0, x1, y1, o);
        if (ok) ghr::project_colour(a, in, sf.rest + (size_t)strand * row, o);
        out_means2D[3 * i] = o.ndc[0]; out_means2D[3 * i + 1] = o.ndc[1]; out_means2D[3 * i + 2] = o.ndc[2];
        out_radii[i] = o.radius;
        a.rects[i] = ok ? ghr::make_rect4(x0, y0, x1, y1, 0u) : ghr::rect4{0u, 0u, 0u, 0u};
        if (ok) {
            for (int q = 0; q < 4; q++) rec[4 * (size_t)i + q] = o.rec[q];
            out_depths[i] = o.depth;
        }
    }
    std::memcpy(out_rec, rec.data(), sizeof(float) * 16 * (size_t)P);
}

// gacc [P][16]: the packed rasterizer gradients of every row.  n_seg == 0: project_bwd_one on expanded arrays, d_fdc [P][3] /
// d_frest [P][3 (K-1)] stored per row.  n_seg >= 1: the factored form of k_shared_proj_bwd, d_rgb [P][3] assigned, d_fdc /
// d_frest untouched.  cam [P][GHR_CAM_PARTIALS] or NULL.  Returns whether a stored value was non-finite (the kernel's flag).
int ghrsim_shared_backward(const ghr::ModelArgs* a_in, int n_seg, const int* radii, const float* gacc, float* d_means2D,
                           float* d_xyz, float* d_ls, float* d_rot, float* d_conf, float* d_dir, float* d_fdc, float* d_frest,
                           float* d_rgb, float* cam)
{
    ghr::ModelArgs a = *a_in;
    a.gx = (a.W + 15) / 16; a.gy = (a.H + 15) / 16;
    a.radii = const_cast<int*>(radii);
    ghr::ModelGrads g = plain_grads(d_means2D, d_xyz, d_ls, d_rot, d_conf, d_dir);
    const int row = 3 * (a.sh_coeffs - 1);
    bool bad = false;
    if (!n_seg) {
        g.d_features_dc = d_fdc; g.d_features_rest = d_frest;
        std::vector<float> none(1);
        for (int i = 0; i < a.P; i++)
            bad |= ghr::project_bwd_one(a, g, i, gacc + 16 * (size_t)i, a.features_rest + (size_t)i * row,
                                        row ? d_frest + (size_t)i * row : none.data(), cam ? cam + (size_t)GHR_CAM_PARTIALS * i : nullptr);
        return bad;
    }
    const ghr::SharedFeat sf{a.P / n_seg, n_seg, a.features_dc, a.features_rest};
    a.features_dc = a.xyz; a.features_rest = nullptr;
    g.d_rgb = d_rgb;
    for (int i = 0; i < a.P; i++) {
        const int strand = i / n_seg;
        ghr::RawIn in;
        ghr::load_raw(a, i, in);
        for (int c = 0; c < 3; c++) in.dc[c] = sf.dc[3 * (size_t)strand + c];
        const float* ga = gacc + 16 * (size_t)i;
        const float* rest = sf.rest + (size_t)strand * row;
        ghr::ProjBwdOut o;
        if (cam) {
            float* cm = cam + (size_t)GHR_CAM_PARTIALS * i;
            ghr::project_bwd_geom<true>(a, in, radii[i], ga, o, cm, false);
            ghr::project_bwd_sh<true, false>(a, in, radii[i], ga, rest, nullptr, o, cm);
        } else {
            ghr::project_bwd_geom<false>(a, in, radii[i], ga, o, nullptr, false);
            ghr::project_bwd_sh<false, false>(a, in, radii[i], ga, rest, nullptr, o, nullptr);
        }
        bad |= ghr::project_bwd_store(a, g, i, ga, o, radii[i]);
    }
    return bad;
}

// k_shared_sh_fold: d_dc [S][3], d_rest [S][3 (K-1)] assigned; returns the flag
int ghrsim_shared_fold(int S, int n_seg, int deg, int K, const float* xyz, const float* campos, const float* d_rgb, float* d_dc,
                       float* d_rest)
{
    bool bad = false;
    const int row = 3 * (K - 1);
    std::vector<float> none(1);
    for (int s = 0; s < S; s++)
        bad |= ghr::shared_fold_strand(deg, K, n_seg, xyz + 3 * (size_t)s * n_seg, campos, d_rgb + 3 * (size_t)s * n_seg,
                                       d_dc + 3 * (size_t)s, row ? d_rest + (size_t)s * row : none.data());
    return bad;
}

// ghr_strand_rows_reduce: out [S][C] from g [S n_seg][C]
void ghrsim_shared_rows_reduce(int S, int n_seg, int C, const float* g, float* out)
{
    for (int s = 0; s < S; s++)
        for (int c = 0; c < C; c++) out[(size_t)s * C + c] = ghr::rows_reduce_one(g + (size_t)s * n_seg * C + c, n_seg, C);
}

}  // extern "C"
