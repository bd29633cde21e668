// ghr_hostsim_sds.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Compiles gaussianhaircut_amd/csrc/ghr_sds.h as plain C++ for the host and walks the kernels' loops with a 64-lane wave kept in
// arrays: the same GHR_HD arithmetic, the same split of the work over lanes, the same butterfly and Hillis-Steele orders.
// Every index a walk forms is checked (SDS_CHECK aborts with the expression).  tests/test_strand_prior_cpu.py loads this as a
// shared library; ghr_sds_selfcheck.cpp includes it and adds a main().
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../gaussianhaircut_amd/csrc/ghr_sds.h"

#define SDS_CHECK(cond)                                                                          \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            std::fprintf(stderr, "ghr_hostsim_sds.cpp:%d: check failed: %s\n", __LINE__, #cond); \
            std::abort();                                                                        \
        }                                                                                        \
    } while (0)

namespace {

constexpr int WV = GHR_SDS_WAVE;

void wave_sum(float* x)  // sds_wave_sum
{
    for (int m = 1; m < WV; m <<= 1) {
        float t[WV];
        for (int l = 0; l < WV; l++) t[l] = x[l] + x[l ^ m];
        std::memcpy(x, t, sizeof(t));
    }
}

void wave_excl(float* x, int dir)  // sds_wave_excl
{
    for (int d = 1; d < WV; d <<= 1) {
        float t[WV];
        for (int l = 0; l < WV; l++) {
            const int from = dir > 0 ? l - d : l + d;
            t[l] = (from >= 0 && from < WV) ? x[l] + x[from] : x[l];
        }
        std::memcpy(x, t, sizeof(t));
    }
    float t[WV];
    for (int l = 0; l < WV; l++) {
        const int from = dir > 0 ? l - 1 : l + 1;
        t[l] = (from >= 0 && from < WV) ? x[from] : 0.f;
    }
    std::memcpy(x, t, sizeof(t));
}

void frame(const float* frames, int inverse, long long s, float* M)
{
    if (inverse) std::memcpy(M, frames + s * 9, 9 * sizeof(float));
    else ghr::sds_inv3(frames + s * 9, M);
}

}  // namespace

extern "C" {

int ghrsim_sds_wave(void) { return WV; }

void ghrsim_sds_inv3(const float* m, float* o) { ghr::sds_inv3(m, o); }
float ghrsim_sds_alpha(float c) { return ghr::sds_alpha(c); }
float ghrsim_sds_alpha_dc(float c) { return ghr::sds_alpha_dc(c); }

// the insertion alone: candidates in the given order into one list
void ghrsim_sds_top4(int n, const float* d, const int32_t* g, float* od, int32_t* og)
{
    ghr::SdsTop t;
    ghr::sds_top_init(t);
    for (int i = 0; i < n; i++) ghr::sds_top_insert(t, d[i], g[i]);
    for (int k = 0; k < GHR_SDS_K; k++) { od[k] = t.d[k]; og[k] = t.g[k]; }
}

void ghrsim_sds_local(int S, int N, int n, const float* dirs, const float* frames, int inverse, const int64_t* idx, float scale,
                      float* e, float* v)
{
    for (int g = 0; g < N; g++) {
        const long long s = idx[g];
        SDS_CHECK(s >= 0 && s < S);
        float M[9];
        frame(frames, inverse, s, M);
        const float* d = dirs + (size_t)s * n * 3;
        float run[3][WV];
        int lo[WV], hi[WV];
        for (int l = 0; l < WV; l++) {
            ghr::sds_chunk(n, l, &lo[l], &hi[l]);
            SDS_CHECK(0 <= lo[l] && lo[l] <= hi[l] && hi[l] <= n && (l == 0 ? lo[l] == 0 : lo[l] == hi[l - 1]));
            for (int c = 0; c < 3; c++) run[c][l] = 0.f;
            for (int i = lo[l]; i < hi[l]; i++)
                for (int c = 0; c < 3; c++) run[c][l] += d[i * 3 + c];
        }
        SDS_CHECK(hi[WV - 1] == n);
        for (int c = 0; c < 3; c++) wave_excl(run[c], +1);
        float* eg = e + (size_t)g * (n + 1) * 3;
        float* vg = v + (size_t)g * n * 3;
        eg[0] = eg[1] = eg[2] = 0.f;
        for (int l = 0; l < WV; l++) {
            float r[3] = {run[0][l], run[1][l], run[2][l]};
            for (int i = lo[l]; i < hi[l]; i++) {
                const float x[3] = {d[i * 3], d[i * 3 + 1], d[i * 3 + 2]};
                float o[3];
                ghr::sds_mv(M, x, scale, o);
                for (int c = 0; c < 3; c++) { vg[i * 3 + c] = o[c]; r[c] += x[c]; }
                ghr::sds_mv(M, r, scale, o);
                for (int c = 0; c < 3; c++) eg[(i + 1) * 3 + c] = o[c];
            }
        }
    }
}

void ghrsim_sds_local_backward(int S, int N, int n, const float* frames, int inverse, const int64_t* sidx, const int64_t* order,
                               float scale, const float* d_e, const float* d_v, float* d_dirs)
{
    if (!d_e && !d_v) return;
    for (int p = 0; p < N; p++) {
        const long long s = sidx[p];
        SDS_CHECK(s >= 0 && s < S);
        if (p > 0) SDS_CHECK(sidx[p - 1] <= s);
        if (p > 0 && sidx[p - 1] == s) continue;
        float M[9];
        frame(frames, inverse, s, M);
        float* out = d_dirs + (size_t)s * n * 3;
        for (int r = p; r < N && sidx[r] == s; r++) {
            const long long g = order[r];
            SDS_CHECK(g >= 0 && g < N);
            if (r > p) SDS_CHECK(order[r - 1] < g);  // the sort was stable: ascending g within a run
            const float* de = d_e ? d_e + (size_t)g * (n + 1) * 3 : nullptr;
            const float* dv = d_v ? d_v + (size_t)g * n * 3 : nullptr;
            float run[3][WV];
            int lo[WV], hi[WV];
            for (int l = 0; l < WV; l++) {
                ghr::sds_chunk(n, l, &lo[l], &hi[l]);
                for (int c = 0; c < 3; c++) run[c][l] = 0.f;
                if (de)
                    for (int i = hi[l] - 1; i >= lo[l]; i--)
                        for (int c = 0; c < 3; c++) run[c][l] += de[(i + 1) * 3 + c];
            }
            if (de)
                for (int c = 0; c < 3; c++) wave_excl(run[c], -1);
            for (int l = 0; l < WV; l++) {
                float rr[3] = {run[0][l], run[1][l], run[2][l]};
                for (int i = hi[l] - 1; i >= lo[l]; i--) {
                    float t[3], o[3];
                    for (int c = 0; c < 3; c++) {
                        if (de) rr[c] += de[(i + 1) * 3 + c];
                        t[c] = (dv ? dv[i * 3 + c] : 0.f) + rr[c];
                    }
                    ghr::sds_mtv(M, t, scale, o);
                    for (int c = 0; c < 3; c++) out[i * 3 + c] += o[c];
                }
            }
        }
    }
}

void ghrsim_sds_texture(int N, int n, int C, int G, const float* uvg, const float* centres, const float* z, const float* v,
                        int32_t* nbr, float* w, float* csim, float* alpha, float* alpha_q, int32_t* count, int32_t* start,
                        int32_t* list, float* texture)
{
    const int GG = G * G, total = GHR_SDS_K * GG;
    SDS_CHECK(N >= GHR_SDS_K && GG >= N && n >= 1 && C >= 1);
    for (int g = 0; g < N; g++) count[g] = 0;
    // k_sds_knn
    for (int q = 0; q < GG; q++) {
        const float cx = centres[q % G], cy = centres[q / G];
        std::vector<ghr::SdsTop> t(WV);
        for (int l = 0; l < WV; l++) {
            ghr::sds_top_init(t[l]);
            for (int g = l; g < N; g += WV) ghr::sds_top_insert(t[l], ghr::sds_dist2(cx, cy, uvg[2 * g], uvg[2 * g + 1]), g);
        }
        for (int m = 1; m < WV; m <<= 1) {
            std::vector<ghr::SdsTop> o(t);
            for (int l = 0; l < WV; l++)
                for (int k = 0; k < GHR_SDS_K; k++) ghr::sds_top_insert(t[l], o[l ^ m].d[k], o[l ^ m].g[k]);
        }
        for (int l = 1; l < WV; l++) SDS_CHECK(std::memcmp(&t[l], &t[0], sizeof(ghr::SdsTop)) == 0);  // every lane holds the answer
        float wq[GHR_SDS_K];
        ghr::sds_weights(t[0].d, wq);
        for (int k = 0; k < GHR_SDS_K; k++) {
            SDS_CHECK(t[0].g[k] >= 0 && t[0].g[k] < N);
            nbr[q * GHR_SDS_K + k] = t[0].g[k];
            w[q * GHR_SDS_K + k] = wq[k];
            count[t[0].g[k]]++;
        }
        if (q >= N) continue;
        float acc[GHR_SDS_PAIRS][WV];
        for (int l = 0; l < WV; l++) {
            float a[GHR_SDS_PAIRS];
            for (int p = 0; p < GHR_SDS_PAIRS; p++) a[p] = 0.f;
            for (int i = l; i < n; i += WV) {
                float x[GHR_SDS_K][3];
                for (int m = 0; m < GHR_SDS_K; m++) std::memcpy(x[m], v + ((size_t)t[0].g[m] * n + i) * 3, 3 * sizeof(float));
                ghr::sds_pair_cos(x, a);
            }
            for (int p = 0; p < GHR_SDS_PAIRS; p++) acc[p][l] = a[p];
        }
        float a0[GHR_SDS_PAIRS];
        for (int p = 0; p < GHR_SDS_PAIRS; p++) { wave_sum(acc[p]); a0[p] = acc[p][0]; }
        csim[q] = ghr::sds_csim(a0, n);
        alpha[q] = ghr::sds_alpha(csim[q]);
    }
    // k_sds_lists: the 64-strided count sums with their butterfly, then the ballot-prefix placement chunk by chunk
    for (int g = 0; g < N; g++) {
        int part[WV];
        for (int l = 0; l < WV; l++) {
            part[l] = 0;
            for (int h = l; h < g; h += WV) part[l] += count[h];
        }
        for (int m = 1; m < WV; m <<= 1) {
            int t[WV];
            for (int l = 0; l < WV; l++) t[l] = part[l] + part[l ^ m];
            std::memcpy(part, t, sizeof(t));
        }
        const int base = part[0];
        for (int l = 1; l < WV; l++) SDS_CHECK(part[l] == base);
        start[g] = base;
        if (g == N - 1) start[N] = base + count[g];
        int pos = base;
        for (int e0 = 0; e0 < total; e0 += WV) {
            unsigned long long mask = 0;
            for (int l = 0; l < WV; l++)
                if (e0 + l < total && nbr[e0 + l] == g) mask |= 1ull << l;
            for (int l = 0; l < WV; l++) {
                if (!((mask >> l) & 1ull)) continue;
                const int at = pos + __builtin_popcountll(mask & ((1ull << l) - 1ull));
                SDS_CHECK(at >= 0 && at < total);
                list[at] = e0 + l;
            }
            pos += __builtin_popcountll(mask);
        }
        SDS_CHECK(pos == base + count[g]);
    }
    SDS_CHECK(start[N] == total);
    // k_sds_blend
    for (int q = 0; q < GG; q++) {
        float wq[GHR_SDS_K], al[GHR_SDS_K];
        const int32_t* g = nbr + q * GHR_SDS_K;
        for (int k = 0; k < GHR_SDS_K; k++) { wq[k] = w[q * GHR_SDS_K + k]; al[k] = alpha[g[k]]; }
        const float aq = ghr::sds_mix4(wq, al);
        alpha_q[q] = aq;
        for (int c = 0; c < C; c++) {
            float zk[GHR_SDS_K];
            for (int k = 0; k < GHR_SDS_K; k++) zk[k] = z[(size_t)g[k] * C + c];
            texture[(size_t)c * GG + q] = ghr::sds_blend(zk[0], ghr::sds_mix4(wq, zk), aq);
        }
    }
}

void ghrsim_sds_texture_backward(int N, int n, int C, int G, const float* z, const float* v, const int32_t* nbr, const float* w,
                                 const float* csim, const float* alpha_q, const int32_t* start, const int32_t* list,
                                 const float* d_texture, float* dalpha_q, float* d_csim, float* d_z, float* d_v)
{
    const int GG = G * G, total = GHR_SDS_K * GG;
    for (int q = 0; q < GG; q++) {  // k_sds_bwd_texel
        const int32_t* g = nbr + q * GHR_SDS_K;
        const float* wq = w + q * GHR_SDS_K;
        float part[WV];
        for (int l = 0; l < WV; l++) {
            part[l] = 0.f;
            for (int c = l; c < C; c += WV) {
                float zk[GHR_SDS_K];
                for (int k = 0; k < GHR_SDS_K; k++) { SDS_CHECK(g[k] >= 0 && g[k] < N); zk[k] = z[(size_t)g[k] * C + c]; }
                part[l] += d_texture[(size_t)c * GG + q] * ghr::sds_blend_dalpha(zk[0], ghr::sds_mix4(wq, zk));
            }
        }
        wave_sum(part);
        dalpha_q[q] = part[0];
    }
    for (int g = 0; g < N; g++) {  // k_sds_bwd_gather
        const int beg = start[g], end = start[g + 1];
        SDS_CHECK(0 <= beg && beg <= end && end <= total);
        float dal = 0.f;
        for (int t = beg; t < end; t++) {
            const int e = list[t];
            SDS_CHECK(e >= 0 && e < total && nbr[e] == g && (t == beg || list[t - 1] < e));
            dal += dalpha_q[e >> 2] * w[e];
        }
        d_csim[g] = dal * ghr::sds_alpha_dc(csim[g]);
        for (int c = 0; c < C; c++) {
            float acc = 0.f;
            for (int t = beg; t < end; t++) {
                const int e = list[t], q = e >> 2;
                acc += d_texture[(size_t)c * GG + q] * ghr::sds_blend_dz(e & 3, w[e], alpha_q[q]);
            }
            d_z[(size_t)g * C + c] = acc;
        }
    }
    if (!d_v) return;
    for (int g = 0; g < N; g++) {  // k_sds_bwd_v
        const int beg = start[g], end = start[g + 1];
        for (int i = 0; i < n; i++) {
            float acc[3] = {0.f, 0.f, 0.f};
            for (int t = beg; t < end; t++) {
                const int e = list[t], q = e >> 2;
                if (q >= N) break;
                const float dc = (d_csim[q] / (float)GHR_SDS_PAIRS) / (float)n;
                float x[GHR_SDS_K][3], da[3];
                for (int m = 0; m < GHR_SDS_K; m++) std::memcpy(x[m], v + ((size_t)nbr[q * GHR_SDS_K + m] * n + i) * 3, 3 * sizeof(float));
                ghr::sds_pair_cos_vjp(x, e & 3, dc, da);
                for (int c = 0; c < 3; c++) acc[c] += da[c];
            }
            for (int c = 0; c < 3; c++) d_v[((size_t)g * n + i) * 3 + c] = acc[c];
        }
    }
}

}  // extern "C"
