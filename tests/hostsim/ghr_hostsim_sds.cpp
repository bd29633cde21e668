// ghr_hostsim_sds.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Compiles gaussianhaircut_amd/csrc/ghr_sds.h as plain C++ for the host and walks the kernels' loops with a 64-lane wave kept in
// arrays: the same GHR_HD arithmetic, the same split of the work over lanes, the same butterfly and Hillis-Steele orders.
// The texture's neighbours, blend and backward are ghr_hostsim_haar.h's shared walk over the texels; the local frames and
// k_sds_lists are walked here.  Every index a walk forms is checked (GHR_HAAR_CHECK aborts with the expression).
// tests/test_strand_prior_cpu.py loads this as a shared library; ghr_sds_selfcheck.cpp includes it and adds a main().
#include "ghr_hostsim_haar.h"
#include "../../gaussianhaircut_amd/csrc/ghr_sds.h"

namespace {

using ghrsim::WV;

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
        GHR_HAAR_CHECK(s >= 0 && s < S);
        float M[9];
        frame(frames, inverse, s, M);
        const float* d = dirs + (size_t)s * n * 3;
        float run[3][WV];
        int lo[WV], hi[WV];
        for (int l = 0; l < WV; l++) {
            ghr::sds_chunk(n, l, &lo[l], &hi[l]);
            GHR_HAAR_CHECK(0 <= lo[l] && lo[l] <= hi[l] && hi[l] <= n && (l == 0 ? lo[l] == 0 : lo[l] == hi[l - 1]));
            for (int c = 0; c < 3; c++) run[c][l] = 0.f;
            for (int i = lo[l]; i < hi[l]; i++)
                for (int c = 0; c < 3; c++) run[c][l] += d[i * 3 + c];
        }
        GHR_HAAR_CHECK(hi[WV - 1] == n);
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
        GHR_HAAR_CHECK(s >= 0 && s < S);
        if (p > 0) GHR_HAAR_CHECK(sidx[p - 1] <= s);
        if (p > 0 && sidx[p - 1] == s) continue;
        float M[9];
        frame(frames, inverse, s, M);
        float* out = d_dirs + (size_t)s * n * 3;
        for (int r = p; r < N && sidx[r] == s; r++) {
            const long long g = order[r];
            GHR_HAAR_CHECK(g >= 0 && g < N);
            if (r > p) GHR_HAAR_CHECK(order[r - 1] < g);  // the sort was stable: ascending g within a run
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
    ghr::HaarArgs a{};
    a.Q = GG; a.N = N; a.n = n; a.C = C; a.G = G; a.uvg = uvg; a.centres = centres; a.z = z; a.v = v;
    a.nbr = nbr; a.w = w; a.csim = csim; a.alpha = alpha; a.alpha_q = alpha_q; a.count = count; a.start = start; a.list = list;
    a.out = texture;
    ghrsim::haar_knn<ghr::HaarTexels>(a);
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
        for (int l = 1; l < WV; l++) GHR_HAAR_CHECK(part[l] == base);
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
                GHR_HAAR_CHECK(at >= 0 && at < total);
                list[at] = e0 + l;
            }
            pos += __builtin_popcountll(mask);
        }
        GHR_HAAR_CHECK(pos == base + count[g]);
    }
    GHR_HAAR_CHECK(start[N] == total);
    ghrsim::haar_blend<ghr::HaarTexels>(a);
}

void ghrsim_sds_texture_backward(int N, int n, int C, int G, const float* z, const float* v, const int32_t* nbr, const float* w,
                                 const float* csim, const float* alpha_q, const int32_t* start, const int32_t* list,
                                 const float* d_texture, float* dalpha_q, float* d_csim, float* d_z, float* d_v)
{
    ghr::HaarArgs a{};
    a.Q = G * G; a.N = N; a.n = n; a.C = C; a.G = G; a.z = z; a.v = v;
    a.nbr = const_cast<int32_t*>(nbr); a.w = const_cast<float*>(w); a.csim = const_cast<float*>(csim);
    a.alpha_q = const_cast<float*>(alpha_q); a.start = const_cast<int32_t*>(start); a.list = const_cast<int32_t*>(list);
    a.d_out = d_texture; a.dalpha_q = dalpha_q; a.d_csim = d_csim; a.d_z = d_z; a.d_v = d_v;
    ghrsim::haar_backward<ghr::HaarTexels>(a);
}

}  // extern "C"
