// ghr_hostsim_guides.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Compiles gaussianhaircut_amd/csrc/ghr_guides.h (and through it ghr_sds.h) as plain C++ for the host and walks the kernels'
// loops with a 64-lane wave kept in arrays: the same GHR_HD arithmetic, the same split of the work over lanes, the same butterfly
// orders.  k_gd_fill's arrival order is whatever the hardware makes it; here the choices arrive in DESCENDING order, the opposite
// of the order the lists must end in.  Every index a walk forms is checked (GD_CHECK aborts with the expression).
// tests/test_guides_cpu.py loads this as a shared library; ghr_guides_selfcheck.cpp includes it and adds a main().
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../gaussianhaircut_amd/csrc/ghr_guides.h"

#define GD_CHECK(cond)                                                                              \
    do {                                                                                            \
        if (!(cond)) {                                                                              \
            std::fprintf(stderr, "ghr_hostsim_guides.cpp:%d: check failed: %s\n", __LINE__, #cond); \
            std::abort();                                                                           \
        }                                                                                           \
    } while (0)

namespace {

constexpr int WV = GHR_SDS_WAVE;
constexpr int KK = GHR_SDS_K;

void wave_sum(float* x)  // sds_wave_sum
{
    for (int m = 1; m < WV; m <<= 1) {
        float t[WV];
        for (int l = 0; l < WV; l++) t[l] = x[l] + x[l ^ m];
        std::memcpy(x, t, sizeof(t));
    }
}

}  // namespace

extern "C" {

int ghrsim_gd_wave(void) { return WV; }

void ghrsim_gd_blend(int S, int N, int n, int C, const float* uvs, const float* z_g, const float* v_g, int32_t* nbr, float* w,
                     float* csim, float* alpha, float* alpha_s, int32_t* count, int32_t* start, int32_t* unsorted, int32_t* list,
                     float* z)
{
    const int total = KK * S;
    GD_CHECK(N >= KK && S >= N && n >= 1 && C >= 1);
    for (int g = 0; g < N; g++) count[g] = 0;
    // k_gd_knn
    for (int s = 0; s < S; s++) {
        const float cx = uvs[2 * s], cy = uvs[2 * s + 1];
        std::vector<ghr::SdsTop> t(WV);
        for (int l = 0; l < WV; l++) {
            ghr::sds_top_init(t[l]);
            for (int g = l; g < N; g += WV) ghr::sds_top_insert(t[l], ghr::sds_dist2(cx, cy, uvs[2 * g], uvs[2 * g + 1]), g);
        }
        for (int m = 1; m < WV; m <<= 1) {
            std::vector<ghr::SdsTop> o(t);
            for (int l = 0; l < WV; l++)
                for (int k = 0; k < KK; k++) ghr::sds_top_insert(t[l], o[l ^ m].d[k], o[l ^ m].g[k]);
        }
        for (int l = 1; l < WV; l++) GD_CHECK(std::memcmp(&t[l], &t[0], sizeof(ghr::SdsTop)) == 0);  // every lane holds the answer
        float ws[KK];
        ghr::sds_weights(t[0].d, ws);
        for (int k = 0; k < KK; k++) {
            GD_CHECK(t[0].g[k] >= 0 && t[0].g[k] < N);
            nbr[s * KK + k] = t[0].g[k];
            w[s * KK + k] = ws[k];
            count[t[0].g[k]]++;
        }
        if (s >= N) continue;
        float acc[GHR_SDS_PAIRS][WV];
        for (int l = 0; l < WV; l++) {
            float a[GHR_SDS_PAIRS];
            for (int p = 0; p < GHR_SDS_PAIRS; p++) a[p] = 0.f;
            for (int i = l; i < n; i += WV) {
                float x[KK][3];
                for (int m = 0; m < KK; m++) std::memcpy(x[m], v_g + ((size_t)t[0].g[m] * n + i) * 3, 3 * sizeof(float));
                ghr::sds_pair_cos(x, a);
            }
            for (int p = 0; p < GHR_SDS_PAIRS; p++) acc[p][l] = a[p];
        }
        float a0[GHR_SDS_PAIRS];
        for (int p = 0; p < GHR_SDS_PAIRS; p++) { wave_sum(acc[p]); a0[p] = acc[p][0]; }
        csim[s] = ghr::sds_csim(a0, n);
        alpha[s] = ghr::sds_alpha(csim[s]);
    }
    // k_gd_blend
    for (int s = 0; s < S; s++) {
        float ws[KK], al[KK];
        const int32_t* g = nbr + s * KK;
        for (int k = 0; k < KK; k++) { ws[k] = w[s * KK + k]; al[k] = alpha[g[k]]; }
        const float as = ghr::sds_mix4(ws, al);
        alpha_s[s] = as;
        for (int c = 0; c < C; c++) {
            if (s < N) { z[(size_t)s * C + c] = z_g[(size_t)s * C + c]; continue; }
            float zk[KK];
            for (int k = 0; k < KK; k++) zk[k] = z_g[(size_t)g[k] * C + c];
            z[(size_t)s * C + c] = ghr::sds_blend(zk[0], ghr::sds_mix4(ws, zk), as);
        }
    }
    // k_gd_start: the lanes' chunk sums, the inclusive scan over the lanes, the second walk
    {
        int lo[WV], hi[WV], sum[WV], run[WV];
        for (int l = 0; l < WV; l++) {
            ghr::gd_chunk(N, l, &lo[l], &hi[l]);
            GD_CHECK(0 <= lo[l] && lo[l] <= hi[l] && hi[l] <= N && (l == 0 ? lo[l] == 0 : lo[l] == hi[l - 1]));
            sum[l] = 0;
            for (int g = lo[l]; g < hi[l]; g++) sum[l] += count[g];
            run[l] = sum[l];
        }
        GD_CHECK(hi[WV - 1] == N);
        for (int d = 1; d < WV; d <<= 1) {
            int t[WV];
            for (int l = 0; l < WV; l++) t[l] = l >= d ? run[l] + run[l - d] : run[l];
            std::memcpy(run, t, sizeof(t));
        }
        int wrote_end = 0;
        for (int l = 0; l < WV; l++) {
            int r = run[l] - sum[l];
            for (int g = lo[l]; g < hi[l]; g++) { start[g] = r; r += count[g]; }
            if (hi[l] == N && lo[l] < hi[l]) { start[N] = r; wrote_end++; }
        }
        GD_CHECK(wrote_end == 1 && start[N] == total);
    }
    // k_gd_fill, the choices arriving last first
    for (int e = total - 1; e >= 0; e--) {
        const int g = nbr[e];
        const int at = start[g] + count[g]-- - 1;
        GD_CHECK(at >= start[g] && at < start[g + 1]);
        unsorted[at] = e;
    }
    for (int g = 0; g < N; g++) GD_CHECK(count[g] == 0);
    // k_gd_lists
    for (int g = 0; g < N; g++) {
        const int beg = start[g], L = start[g + 1] - beg;
        GD_CHECK(beg >= 0 && L >= 0 && beg + L <= total);
        std::vector<char> hit(L, 0);
        for (int i = 0; i < L; i++) {
            const int32_t x = unsorted[beg + i];
            const int r = ghr::gd_rank(unsorted + beg, L, x);
            GD_CHECK(r >= 0 && r < L && !hit[r]);
            hit[r] = 1;
            list[beg + r] = x;
        }
    }
}

void ghrsim_gd_blend_backward(int S, int N, int n, int C, const float* z_g, const float* v_g, const int32_t* nbr, const float* w,
                              const float* csim, const float* alpha_s, const int32_t* start, const int32_t* list, const float* d_z,
                              float* dalpha_s, float* d_csim, float* d_zg, float* d_vg)
{
    const int total = KK * S;
    for (int s = 0; s < S; s++) {  // k_gd_dalpha
        if (s < N) { dalpha_s[s] = 0.f; continue; }
        const int32_t* g = nbr + s * KK;
        const float* ws = w + s * KK;
        float part[WV];
        for (int l = 0; l < WV; l++) {
            part[l] = 0.f;
            for (int c = l; c < C; c += WV) {
                float zk[KK];
                for (int k = 0; k < KK; k++) { GD_CHECK(g[k] >= 0 && g[k] < N); zk[k] = z_g[(size_t)g[k] * C + c]; }
                part[l] += d_z[(size_t)s * C + c] * ghr::sds_blend_dalpha(zk[0], ghr::sds_mix4(ws, zk));
            }
        }
        wave_sum(part);
        dalpha_s[s] = part[0];
    }
    for (int g = 0; g < N; g++) {  // k_gd_gather
        const int beg = start[g], end = start[g + 1];
        GD_CHECK(0 <= beg && beg <= end && end <= total);
        float dal = 0.f;
        for (int t = beg; t < end; t++) {
            const int e = list[t], s = e >> 2;
            GD_CHECK(e >= 0 && e < total && nbr[e] == g && (t == beg || list[t - 1] < e));
            if (s < N) continue;
            dal += dalpha_s[s] * w[e];
        }
        d_csim[g] = dal * ghr::sds_alpha_dc(csim[g]);
        for (int c = 0; c < C; c++) {
            float acc = d_z[(size_t)g * C + c];
            for (int t = beg; t < end; t++) {
                const int e = list[t], s = e >> 2;
                if (s < N) continue;
                acc += d_z[(size_t)s * C + c] * ghr::sds_blend_dz(e & 3, w[e], alpha_s[s]);
            }
            d_zg[(size_t)g * C + c] = acc;
        }
    }
    if (!d_vg) return;
    for (int g = 0; g < N; g++) {  // k_gd_bwd_v
        const int beg = start[g], end = start[g + 1];
        for (int i = 0; i < n; i++) {
            float acc[3] = {0.f, 0.f, 0.f};
            for (int t = beg; t < end; t++) {
                const int e = list[t], q = e >> 2;
                if (q >= N) break;
                const float dc = (d_csim[q] / (float)GHR_SDS_PAIRS) / (float)n;
                float x[KK][3], da[3];
                for (int m = 0; m < KK; m++) std::memcpy(x[m], v_g + ((size_t)nbr[q * KK + m] * n + i) * 3, 3 * sizeof(float));
                ghr::sds_pair_cos_vjp(x, e & 3, dc, da);
                for (int c = 0; c < 3; c++) acc[c] += da[c];
            }
            for (int c = 0; c < 3; c++) d_vg[((size_t)g * n + i) * 3 + c] = acc[c];
        }
    }
}

}  // extern "C"
