// ghr_hostsim_haar.h -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// The host walk of gaussianhaircut_amd/csrc/ghr_haar.h that the strand prior's and the guides' simulators share: the five kernels'
// loops with a 64-lane wave kept in arrays, templated on the same query policies -- the walk calls the GHR_HD policy functions the
// kernels call, the same GHR_HD arithmetic, the same split of the work over lanes, the same butterfly orders.  Every index a walk
// forms is checked (GHR_HAAR_CHECK aborts with the expression).  The lists between the forward and the backward are each
// simulator's own.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define GHR_HAAR_CHECK(cond)                                                                 \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond);    \
            std::abort();                                                                    \
        }                                                                                    \
    } while (0)
#include "../../gaussianhaircut_amd/csrc/ghr_haar.h"

namespace ghrsim {

constexpr int WV = GHR_SDS_WAVE;
constexpr int KK = GHR_SDS_K;

inline void wave_sum(float* x)  // sds_wave_sum
{
    for (int m = 1; m < WV; m <<= 1) {
        float t[WV];
        for (int l = 0; l < WV; l++) t[l] = x[l] + x[l ^ m];
        std::memcpy(x, t, sizeof(t));
    }
}

inline void haar_load4(const ghr::HaarArgs& a, const int32_t* g, int i, float x[KK][3])
{
    for (int m = 0; m < KK; m++) std::memcpy(x[m], a.v + ((size_t)g[m] * a.n + i) * 3, 3 * sizeof(float));
}

// the fill of count, then k_haar_knn
template <class P>
void haar_knn(const ghr::HaarArgs& a)
{
    GHR_HAAR_CHECK(a.N >= KK && a.Q >= a.N && a.n >= 1 && a.C >= 1);
    for (int g = 0; g < a.N; g++) a.count[g] = 0;
    for (int q = 0; q < a.Q; q++) {
        float cx, cy;
        P::uv(a, q, &cx, &cy);
        std::vector<ghr::SdsTop> t(WV);
        for (int l = 0; l < WV; l++) {
            ghr::sds_top_init(t[l]);
            for (int g = l; g < a.N; g += WV) ghr::sds_top_insert(t[l], ghr::sds_dist2(cx, cy, a.uvg[2 * (size_t)g], a.uvg[2 * (size_t)g + 1]), g);
        }
        for (int m = 1; m < WV; m <<= 1) {
            std::vector<ghr::SdsTop> o(t);
            for (int l = 0; l < WV; l++)
                for (int k = 0; k < KK; k++) ghr::sds_top_insert(t[l], o[l ^ m].d[k], o[l ^ m].g[k]);
        }
        for (int l = 1; l < WV; l++) GHR_HAAR_CHECK(std::memcmp(&t[l], &t[0], sizeof(ghr::SdsTop)) == 0);  // every lane holds the answer
        float wq[KK];
        ghr::sds_weights(t[0].d, wq);
        for (int k = 0; k < KK; k++) {
            GHR_HAAR_CHECK(t[0].g[k] >= 0 && t[0].g[k] < a.N);
            a.nbr[(size_t)q * KK + k] = t[0].g[k];
            a.w[(size_t)q * KK + k] = wq[k];
            a.count[t[0].g[k]]++;
        }
        if (q >= a.N) continue;
        float acc[GHR_SDS_PAIRS][WV];
        for (int l = 0; l < WV; l++) {
            float s[GHR_SDS_PAIRS];
            for (int p = 0; p < GHR_SDS_PAIRS; p++) s[p] = 0.f;
            for (int i = l; i < a.n; i += WV) {
                float x[KK][3];
                haar_load4(a, t[0].g, i, x);
                ghr::sds_pair_cos(x, s);
            }
            for (int p = 0; p < GHR_SDS_PAIRS; p++) acc[p][l] = s[p];
        }
        float a0[GHR_SDS_PAIRS];
        for (int p = 0; p < GHR_SDS_PAIRS; p++) { wave_sum(acc[p]); a0[p] = acc[p][0]; }
        a.csim[q] = ghr::sds_csim(a0, a.n);
        a.alpha[q] = ghr::sds_alpha(a.csim[q]);
    }
}

// k_haar_blend
template <class P>
void haar_blend(const ghr::HaarArgs& a)
{
    for (int q = 0; q < a.Q; q++) {
        float wq[KK], al[KK];
        const int32_t* g = a.nbr + (size_t)q * KK;
        for (int k = 0; k < KK; k++) { wq[k] = a.w[(size_t)q * KK + k]; al[k] = a.alpha[g[k]]; }
        const float aq = ghr::sds_mix4(wq, al);
        a.alpha_q[q] = aq;
        for (int c = 0; c < a.C; c++) {
            if (P::guides_first && q < a.N) { a.out[P::at(a, q, c)] = a.z[(size_t)q * a.C + c]; continue; }
            float zk[KK];
            for (int k = 0; k < KK; k++) zk[k] = a.z[(size_t)g[k] * a.C + c];
            a.out[P::at(a, q, c)] = ghr::sds_blend(zk[0], ghr::sds_mix4(wq, zk), aq);
        }
    }
}

// k_haar_dalpha, k_haar_gather and, where d_v is asked for, k_haar_bwd_v
template <class P>
void haar_backward(const ghr::HaarArgs& a)
{
    const int total = KK * a.Q;
    for (int q = 0; q < a.Q; q++) {  // k_haar_dalpha
        if (P::guides_first && q < a.N) { a.dalpha_q[q] = 0.f; continue; }
        const int32_t* g = a.nbr + (size_t)q * KK;
        const float* wq = a.w + (size_t)q * KK;
        float part[WV];
        for (int l = 0; l < WV; l++) {
            part[l] = 0.f;
            for (int c = l; c < a.C; c += WV) {
                float zk[KK];
                for (int k = 0; k < KK; k++) { GHR_HAAR_CHECK(g[k] >= 0 && g[k] < a.N); zk[k] = a.z[(size_t)g[k] * a.C + c]; }
                part[l] += a.d_out[P::at(a, q, c)] * ghr::sds_blend_dalpha(zk[0], ghr::sds_mix4(wq, zk));
            }
        }
        wave_sum(part);
        a.dalpha_q[q] = part[0];
    }
    for (int g = 0; g < a.N; g++) {  // k_haar_gather
        const int beg = a.start[g], end = a.start[g + 1];
        GHR_HAAR_CHECK(0 <= beg && beg <= end && end <= total);
        float dal = 0.f;
        for (int t = beg; t < end; t++) {
            const int e = a.list[t], q = e >> 2;
            GHR_HAAR_CHECK(e >= 0 && e < total && a.nbr[e] == g && (t == beg || a.list[t - 1] < e));
            if (!ghr::haar_blended<P>(a, q)) continue;
            dal += a.dalpha_q[q] * a.w[e];
        }
        a.d_csim[g] = dal * ghr::sds_alpha_dc(a.csim[g]);
        for (int c = 0; c < a.C; c++) {
            float acc = P::guides_first ? a.d_out[P::at(a, g, c)] : 0.f;
            for (int t = beg; t < end; t++) {
                const int e = a.list[t], q = e >> 2;
                if (!ghr::haar_blended<P>(a, q)) continue;
                acc += a.d_out[P::at(a, q, c)] * ghr::sds_blend_dz(e & 3, a.w[e], a.alpha_q[q]);
            }
            a.d_z[(size_t)g * a.C + c] = acc;
        }
    }
    if (!a.d_v) return;
    for (int g = 0; g < a.N; g++) {  // k_haar_bwd_v
        const int beg = a.start[g], end = a.start[g + 1];
        for (int i = 0; i < a.n; i++) {
            float acc[3] = {0.f, 0.f, 0.f};
            for (int t = beg; t < end; t++) {
                const int e = a.list[t], q = e >> 2;
                if (q < 0 || q >= a.N) break;
                const float dc = (a.d_csim[q] / (float)GHR_SDS_PAIRS) / (float)a.n;
                float x[KK][3], da[3];
                haar_load4(a, a.nbr + (size_t)q * KK, i, x);
                ghr::sds_pair_cos_vjp(x, e & 3, dc, da);
                for (int c = 0; c < 3; c++) acc[c] += da[c];
            }
            for (int c = 0; c < 3; c++) a.d_v[((size_t)g * a.n + i) * 3 + c] = acc[c];
        }
    }
}

}  // namespace ghrsim
