// ghr_hostsim_upsample.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Compiles gaussianhaircut_amd/csrc/ghr_upsample.h as plain C++ for the host and walks its two kernels with a 64-lane wave kept in
// arrays: the per-element functions are the header's own; the loops, the neighbouring-lane reads and the butterflies are restated
// here in the launch's order.  Every index a walk forms is checked (GHR_UPS_CHECK aborts with the expression).
// tests/upsample_sim.py loads this as a shared library; ghr_upsample_selfcheck.cpp includes it and adds a main().
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../gaussianhaircut_amd/csrc/ghr_upsample.h"

#define GHR_UPS_CHECK(cond) \
    do { if (!(cond)) { std::fprintf(stderr, "ghr_hostsim_upsample: %s:%d: %s\n", __FILE__, __LINE__, #cond); std::abort(); } } while (0)

namespace ghrsim_ups {

const int WV = GHR_UPS_WAVE;

// a += a[lane ^ m], m = 1 .. 32: every lane ends with the same bits
inline float butterfly(float* a)
{
    for (int m = 1; m < WV; m <<= 1) {
        float t[WV];
        for (int l = 0; l < WV; l++) t[l] = a[l] + a[l ^ m];
        std::memcpy(a, t, sizeof(t));
    }
    for (int l = 1; l < WV; l++) GHR_UPS_CHECK(std::memcmp(&a[l], &a[0], 4) == 0);
    return a[0];
}

struct Rows {
    const float* gp;
    long long G, L;
    const float* at(long long g, long long j) const
    {
        GHR_UPS_CHECK(g >= 0 && g < G && j >= 0 && j < L);
        return gp + (g * L + j) * 3;
    }
};

}  // namespace ghrsim_ups

extern "C" {

void ghrsim_ups_near(int G, const float* groots, int N, const float* co, float r2, int32_t* nbr, float* nd2)
{
    for (int c = 0; c < N; c++) {
        ghr::ShapeTop top;
        ghr::shape_top_init(top);
        for (int base = 0; base < G; base += GHR_UPS_TILE) {
            const int count = G - base < GHR_UPS_TILE ? G - base : GHR_UPS_TILE;
            for (int j = 0; j < count; j++) {
                const int cand = base + j;
                GHR_UPS_CHECK(cand >= 0 && cand < G);
                const float* r = groots + 3 * (size_t)cand;
                ghr::shape_top_insert(top, ghr::shape_dist2(co + 3 * (size_t)c, r[0], r[1], r[2]), cand);
            }
        }
        for (int k = 0; k < GHR_UPS_K; k++) {
            float d2;
            nbr[GHR_UPS_K * (size_t)c + k] = ghr::ups_entry(top, k, r2, &d2);
            nd2[GHR_UPS_K * (size_t)c + k] = d2;
        }
    }
}

void ghrsim_ups_blend(int G, int L, const float* gp, const float* gM, const float* gf, int F, int N, const float* co, const float* cM,
                      const int32_t* nbr, const float* nd2, float eps2, float tau, int gate, float* out, float* w, float* of,
                      uint8_t* valid)
{
    using namespace ghrsim_ups;
    const Rows rows{gp, G, L};
    const int n = L - 1;
    for (int c = 0; c < N; c++) {
        const int32_t* e4 = nbr + GHR_UPS_K * (size_t)c;
        const float* d4 = nd2 + GHR_UPS_K * (size_t)c;
        const float* o = co + 3 * (size_t)c;
        const float* Mc = cM + 9 * (size_t)c;
        float* row_out = out + (size_t)c * L * 3;
        const int K = ghr::ups_count(e4, G);
        if (K == 0) {
            for (int j = 0; j < L; j++)
                for (int x = 0; x < 3; x++) row_out[3 * j + x] = o[x];
            for (int f = 0; f < F; f++) of[(size_t)c * F + f] = 0.f;
            for (int k = 0; k < GHR_UPS_K; k++) w[GHR_UPS_K * (size_t)c + k] = 0.f;
            valid[c] = 0;
            continue;
        }
        const float* M[GHR_UPS_K] = {nullptr, nullptr, nullptr, nullptr};
        for (int k = 0; k < K; k++) {
            GHR_UPS_CHECK(e4[k] >= 0 && e4[k] < G);
            M[k] = gM + 9 * (size_t)e4[k];
        }
        float q[GHR_UPS_K] = {1.f, 1.f, 1.f, 1.f};
        if (K > 1) {
            float D[GHR_UPS_K][WV], A[GHR_UPS_K][WV];
            std::memset(D, 0, sizeof(D));
            std::memset(A, 0, sizeof(A));
            for (int base = 0; base < n; base += WV)
                for (int lane = 0; lane < WV; lane++) {
                    const int i = base + lane;
                    if (i >= n) continue;
                    float e0[3] = {0.f, 0.f, 0.f};
                    for (int k = 0; k < K; k++) {
                        float e[3];
                        ghr::ups_local(M[k], rows.at(e4[k], i + 1), rows.at(e4[k], i), e);
                        if (k == 0) {
                            std::memcpy(e0, e, sizeof(e));
                            A[0][lane] = A[0][lane] + ghr::ups_dot(e, e);
                        } else {
                            D[k][lane] = D[k][lane] + ghr::ups_dot(e, e0);
                            A[k][lane] = A[k][lane] + ghr::ups_dot(e, e);
                        }
                    }
                }
            const float A0 = butterfly(A[0]);
            for (int k = 1; k < K; k++) {
                const float Dk = butterfly(D[k]), Ak = butterfly(A[k]);
                q[k] = ghr::ups_gate(Dk, Ak, A0, tau, gate);
            }
        }
        float wk[GHR_UPS_K];
        ghr::ups_weights(K, q, d4, eps2, wk);
        for (int j = 0; j < L; j++) {
            float Pl[3] = {0.f, 0.f, 0.f};
            for (int k = 0; k < K; k++) {
                float r[3];
                ghr::ups_local(M[k], rows.at(e4[k], j), rows.at(e4[k], 0), r);
                for (int x = 0; x < 3; x++) Pl[x] = k == 0 ? wk[0] * r[x] : Pl[x] + wk[k] * r[x];
            }
            float pt[3];
            ghr::ups_world(o, Mc, Pl, pt);
            for (int x = 0; x < 3; x++) row_out[3 * j + x] = j == 0 ? o[x] : pt[x];
        }
        for (int f = 0; f < F; f++) {
            float v = 0.f;
            for (int k = 0; k < K; k++) {
                const float x = gf[(size_t)e4[k] * F + f];
                v = k == 0 ? wk[0] * x : v + wk[k] * x;
            }
            of[(size_t)c * F + f] = v;
        }
        for (int k = 0; k < GHR_UPS_K; k++) w[GHR_UPS_K * (size_t)c + k] = wk[k];
        valid[c] = 1;
    }
}

}  // extern "C"
