// ghr_hostsim_guides.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Compiles gaussianhaircut_amd/csrc/ghr_guides.h (and through it ghr_haar.h) as plain C++ for the host.  The neighbours, the blend
// and the backward are ghr_hostsim_haar.h's shared walk over the drawn roots; the list builders are walked here with a 64-lane wave
// kept in arrays.  k_gd_fill's arrival order is whatever the hardware makes it; here the choices arrive in DESCENDING order, the
// opposite of the order the lists must end in.  Every index a walk forms is checked (GHR_HAAR_CHECK aborts with the expression).
// tests/test_guides_cpu.py loads this as a shared library; ghr_guides_selfcheck.cpp includes it and adds a main().
#include "ghr_hostsim_haar.h"
#include "../../gaussianhaircut_amd/csrc/ghr_guides.h"

using ghrsim::KK;
using ghrsim::WV;

extern "C" {

int ghrsim_gd_wave(void) { return WV; }

void ghrsim_gd_blend(int S, int N, int n, int C, const float* uvs, const float* z_g, const float* v_g, int32_t* nbr, float* w,
                     float* csim, float* alpha, float* alpha_s, int32_t* count, int32_t* start, int32_t* unsorted, int32_t* list,
                     float* z)
{
    const int total = KK * S;
    ghr::HaarArgs a{};
    a.Q = S; a.N = N; a.n = n; a.C = C; a.uvg = uvs; a.z = z_g; a.v = v_g;
    a.nbr = nbr; a.w = w; a.csim = csim; a.alpha = alpha; a.alpha_q = alpha_s; a.count = count; a.start = start;
    a.unsorted = unsorted; a.list = list; a.out = z;
    ghrsim::haar_knn<ghr::HaarRoots>(a);
    ghrsim::haar_blend<ghr::HaarRoots>(a);
    // k_gd_start: the lanes' chunk sums, the inclusive scan over the lanes, the second walk
    {
        int lo[WV], hi[WV], sum[WV], run[WV];
        for (int l = 0; l < WV; l++) {
            ghr::gd_chunk(N, l, &lo[l], &hi[l]);
            GHR_HAAR_CHECK(0 <= lo[l] && lo[l] <= hi[l] && hi[l] <= N && (l == 0 ? lo[l] == 0 : lo[l] == hi[l - 1]));
            sum[l] = 0;
            for (int g = lo[l]; g < hi[l]; g++) sum[l] += count[g];
            run[l] = sum[l];
        }
        GHR_HAAR_CHECK(hi[WV - 1] == N);
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
        GHR_HAAR_CHECK(wrote_end == 1 && start[N] == total);
    }
    // k_gd_fill, the choices arriving last first
    for (int e = total - 1; e >= 0; e--) {
        const int g = nbr[e];
        const int at = start[g] + count[g]-- - 1;
        GHR_HAAR_CHECK(at >= start[g] && at < start[g + 1]);
        unsorted[at] = e;
    }
    for (int g = 0; g < N; g++) GHR_HAAR_CHECK(count[g] == 0);
    // k_gd_lists
    for (int g = 0; g < N; g++) {
        const int beg = start[g], L = start[g + 1] - beg;
        GHR_HAAR_CHECK(beg >= 0 && L >= 0 && beg + L <= total);
        std::vector<char> hit(L, 0);
        for (int i = 0; i < L; i++) {
            const int32_t x = unsorted[beg + i];
            const int r = ghr::gd_rank(unsorted + beg, L, x);
            GHR_HAAR_CHECK(r >= 0 && r < L && !hit[r]);
            hit[r] = 1;
            list[beg + r] = x;
        }
    }
}

void ghrsim_gd_blend_backward(int S, int N, int n, int C, const float* z_g, const float* v_g, const int32_t* nbr, const float* w,
                              const float* csim, const float* alpha_s, const int32_t* start, const int32_t* list, const float* d_z,
                              float* dalpha_s, float* d_csim, float* d_zg, float* d_vg)
{
    ghr::HaarArgs a{};
    a.Q = S; a.N = N; a.n = n; a.C = C; a.z = z_g; a.v = v_g;
    a.nbr = const_cast<int32_t*>(nbr); a.w = const_cast<float*>(w); a.csim = const_cast<float*>(csim);
    a.alpha_q = const_cast<float*>(alpha_s); a.start = const_cast<int32_t*>(start); a.list = const_cast<int32_t*>(list);
    a.d_out = d_z; a.dalpha_q = dalpha_s; a.d_csim = d_csim; a.d_z = d_zg; a.d_v = d_vg;
    ghrsim::haar_backward<ghr::HaarRoots>(a);
}

}  // extern "C"
