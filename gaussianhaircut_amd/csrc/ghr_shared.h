// ghr_shared.h -- a mode-1 segment whose SH coefficients are stored once per STRAND (the latent-strand stage: the appearance
// decoder emits 48 floats per strand, src/scene/gaussian_model_latent_strands.py:463-475 `repeat`s them over the strand's L - 1
// segments).  Row i of the segment reads features_dc[i / n_seg] and features_rest[i / n_seg]; nothing is expanded:
//   k_shared_proj_fwd   k_project's work; a workgroup stages the `rest` rows of the (few) strands its 256 rows belong to;
//   k_shared_proj_bwd   project_bwd_body's work in FACTORED form: d_rgb [P,3] is assigned, no d_features_* row is stored;
//   k_shared_sh_fold    d sh[s][k][c] = sum over the strand's rows j, in index order, of basis_k(dir_j) d_rgb[s n_seg + j][c].
// The per-row arithmetic is project_geom / project_colour / project_bwd_geom / project_bwd_sh themselves (ghr_project.h), so
// the rasterizer state and every per-row gradient have the bits of k_project / k_project_bwd fed the expanded arrays, and the
// fold forms the products project_bwd_sh would have stored and adds them in the order rows_reduce_one (ghr_latent.h) adds them.
#pragma once
#include "ghr_project.h"

namespace ghr {

// REST: the model has SH coefficients beyond the DC term (as k_project)
template <bool REST>
__global__ void __launch_bounds__(GHR_BLOCK) k_shared_proj_fwd(ModelArgs a, SharedFeat sf)
{
#if defined(__HIP_DEVICE_COMPILE__)
    // 256 rows span at most min(256, 255 / n_seg + 2) strands; the record transpose and the big rects need the rest of it
    __shared__ __attribute__((aligned(16))) float s_rest[GHR_BLOCK * GHR_REST_MAX];
    const int row = REST ? 3 * (a.sh_coeffs - 1) : 0;
    const int base = blockIdx.x * GHR_BLOCK;
    const int nb = min(GHR_BLOCK, a.P - base);
    const int idx = base + threadIdx.x;
    const int idc = min(idx, a.P - 1);
    const int strand = idc / sf.n_seg, strand0 = base / sf.n_seg;
    const int n_str = (base + nb - 1) / sf.n_seg - strand0 + 1;
    // issue order as in k_project: the raw parameters (features_dc points at xyz: the value is replaced by the strand's), the
    // strand's DC term, then the strands' coefficient rows; the geometry runs while those are on their way
    RawIn in;
    load_raw(a, idc, in);
#pragma unroll
    for (int i = 0; i < 3; i++) in.dc[i] = sf.dc[3 * (size_t)strand + i];
    if (REST) shared_rest_to_lds<GHR_BLOCK>(s_rest, sf.rest + (size_t)strand0 * row, n_str * row, threadIdx.x);
    int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    ProjOut o;
    const bool ok = idx < a.P && project_geom(a, in, x0, y0, x1, y1, o);
    TileCountPending tc;
    count_tiles_issue(a.tile_count, a.gx, x0, y0, x1, y1, tc);
    __syncthreads();
    if (ok) project_colour(a, in, s_rest + (strand - strand0) * row, o);
    __shared__ uint32_t s_scan[4];
    uint32_t blk_total;
    const uint32_t slot0 = block_excl_scan_256(ok ? (uint32_t)((x1 - x0) * (y1 - y0)) : 0u, s_scan, &blk_total);
    // (from here on as k_project, comments there: the atomics' results are taken in, then stores only)
    __builtin_amdgcn_s_waitcnt(0x0f70);
    f4* s_rec = reinterpret_cast<f4*>(s_rest);
    if (idx < a.P) {
        const size_t rowi = (size_t)a.row0 + idx;
#pragma unroll
        for (int q = 0; q < 4; q++) s_rec[4 * threadIdx.x + q] = o.rec[q];
        if (a.means2D) { a.means2D[3 * rowi] = o.ndc[0]; a.means2D[3 * rowi + 1] = o.ndc[1]; a.means2D[3 * rowi + 2] = o.ndc[2]; }
        a.radii[rowi] = o.radius;
        rect4 r = rect4{0u, 0u, 0u, 0u};
        if (ok) { r = make_rect4(x0, y0, x1, y1, 0u); r.z = slot0; }
        a.rects[rowi] = r;
        if (ok) a.depths[rowi] = o.depth;
    }
    if (threadIdx.x == 0) a.slot_blk[blockIdx.x + (a.row0 >> 8)] = blk_total;
    __syncthreads();
    {
        f4* dst = a.rec + 4 * ((size_t)a.row0 + base);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int j = threadIdx.x + GHR_BLOCK * k;
            if (j < 4 * nb) dst[j] = s_rec[j];
        }
    }
    __syncthreads();
    count_tiles_finish(a.tile_count, (uint32_t)(a.gx * a.gy), a.gx, x0, y0, x1, y1, *reinterpret_cast<BigRects*>(s_rest),
                       a.pos + (size_t)GHR_BIG_RECT * ((size_t)a.row0 + (idx < a.P ? idx : 0)), tc);
#endif
}

// project_bwd_body<CAM, false, true>: one wave per workgroup, the register budget of k_project_bwd's camera instantiations
template <bool CAM>
__global__ void __launch_bounds__(GHR_PBW_BLOCK) __attribute__((amdgpu_waves_per_eu(3, 3)))
k_shared_proj_bwd(ModelArgs a, ModelGrads g, SharedFeat sf)
{
#if defined(__HIP_DEVICE_COMPILE__)
    project_bwd_body<CAM, false, true>(a, g, sf);
#endif
}

// ---- the fold ----------------------------------------------------------------------------------------------------------------
// One row's factors: b[16] = sh_basis(normalize(xyz - campos)) and gg[3] = its d_rgb, the expressions of project_bwd_sh and
// sh_grad_from_views_one.  A row without gradient (d_rgb == 0: culled, or invisible in every pixel) gets zeros for BOTH without
// its direction being evaluated -- it may be undefined (a Gaussian at the camera centre) -- so that its products are +0.
// A NaN compares unequal to zero: it is carried through.
GHR_HD void shared_fold_row(int deg, const float* xyz3, const float* cpos, const float* g3, float* b, float* gg)
{
    const float g0 = g3[0], g1 = g3[1], g2 = g3[2];
    if (g0 == 0.f && g1 == 0.f && g2 == 0.f) {
#pragma unroll
        for (int k = 0; k < GHR_SH_MAX; k++) b[k] = 0.f;
        gg[0] = gg[1] = gg[2] = 0.f;
        return;
    }
    const float dxv = xyz3[0] - cpos[0], dyv = xyz3[1] - cpos[1], dzv = xyz3[2] - cpos[2];
    const float len = sqrtf(dxv * dxv + dyv * dyv + dzv * dzv), il = 1.0f / len;
    sh_basis(deg, dxv * il, dyv * il, dzv * il, b);
    gg[0] = g0; gg[1] = g1; gg[2] = g2;
}

// One strand: xyz / d_rgb point at its first row.  The first row's product is ASSIGNED, later rows are added (rows_reduce_one
// starts from g[0]), one fp32 accumulator per (k, c).  Writes dc[3] and rest[3 (K - 1)]; returns whether a value written is
// non-finite.  (The kernel below walks the same rows in the same order with the lanes as accumulators.)
GHR_HD bool shared_fold_strand(int deg, int K, int n_seg, const float* xyz, const float* cpos, const float* d_rgb, float* dc,
                               float* rest)
{
    float acc[3 * GHR_SH_MAX];
    for (int j = 0; j < n_seg; j++) {
        float b[GHR_SH_MAX], gg[3];
        shared_fold_row(deg, xyz + 3 * (size_t)j, cpos, d_rgb + 3 * (size_t)j, b, gg);
        for (int k = 0; k < GHR_SH_MAX; k++)
            for (int ch = 0; ch < 3; ch++) {
                const float p = b[k] * gg[ch];
                acc[3 * k + ch] = j == 0 ? p : acc[3 * k + ch] + p;
            }
    }
    bool bad = false;
    for (int k = 0; k < K; k++)
        for (int ch = 0; ch < 3; ch++) {
            const float v = acc[3 * k + ch];
            bad |= nonfinite(v);
            if (k == 0) dc[ch] = v;
            else rest[3 * (k - 1) + ch] = v;
        }
    return bad;
}

struct SharedFoldArgs {
    int S, n_seg, sh_degree, sh_coeffs;
    const float* xyz;     // [S n_seg,3]
    const float* campos;  // [3]
    const float* d_rgb;   // [S n_seg,3]
    float* d_dc;          // [S,1,3]   assigned
    float* d_rest;        // [S,K-1,3] assigned
    int* nan_flag;        // optional
};

#define GHR_FOLD_BSTRIDE (GHR_SH_MAX + 1)  // lane = row writes 16 values at this odd stride: no bank conflicts

// One wave per strand.  64 rows at a time: lane = row loads its 24 B (coalesced) and leaves its factors in LDS, then lane =
// (k, c) (48 of 64) walks the 64 rows in order -- all lanes read the same row, 16 + 3 distinct addresses, broadcast.
__global__ void __launch_bounds__(GHR_PBW_BLOCK) k_shared_sh_fold(SharedFoldArgs a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int BLK = GHR_PBW_BLOCK;
    __shared__ float s_b[BLK * GHR_FOLD_BSTRIDE];
    __shared__ float s_g[BLK * 3];
    const int s = blockIdx.x, lane = threadIdx.x;
    const size_t r0 = (size_t)s * a.n_seg;
    const int k = lane / 3, ch = lane - 3 * k;  // lanes 48..63: k >= 16, nothing to accumulate
    const uniform_floats cp = GHR_UNIFORM(a.campos);
    const float cpos[3] = {cp[0], cp[1], cp[2]};
    float acc = 0.f;
    for (int j0 = 0; j0 < a.n_seg; j0 += BLK) {
        const int n = min(BLK, a.n_seg - j0);
        if (lane < n) {
            const size_t r = r0 + j0 + lane;
            const float x3[3] = {a.xyz[3 * r], a.xyz[3 * r + 1], a.xyz[3 * r + 2]};
            const float g3[3] = {a.d_rgb[3 * r], a.d_rgb[3 * r + 1], a.d_rgb[3 * r + 2]};
            float b[GHR_SH_MAX], gg[3];
            shared_fold_row(a.sh_degree, x3, cpos, g3, b, gg);
#pragma unroll
            for (int i = 0; i < GHR_SH_MAX; i++) s_b[lane * GHR_FOLD_BSTRIDE + i] = b[i];
            s_g[3 * lane] = gg[0]; s_g[3 * lane + 1] = gg[1]; s_g[3 * lane + 2] = gg[2];
        }
        __syncthreads();
        if (k < GHR_SH_MAX) {
            for (int j = 0; j < n; j++) {
                const float p = s_b[j * GHR_FOLD_BSTRIDE + k] * s_g[3 * j + ch];
                acc = (j0 + j == 0) ? p : acc + p;
            }
        }
        __syncthreads();
    }
    bool bad = false;
    if (k < a.sh_coeffs) {
        bad = nonfinite(acc);
        if (k == 0) a.d_dc[3 * (size_t)s + ch] = acc;
        else a.d_rest[(size_t)s * 3 * (a.sh_coeffs - 1) + (lane - 3)] = acc;
    }
    if (a.nan_flag != nullptr && __builtin_amdgcn_ballot_w64(bad) != 0 && lane == 0) atomicOr(a.nan_flag, 1);
#endif
}

}  // namespace ghr
