// ghr_guides.h -- guiding strands of the textured generator (the reference's num_guiding_strands,
// src/scene/gaussian_model_strands.py:479-501 restated over STRANDS): the first N roots of a draw of S are the guides, fetched and
// decoded as they are; every other root's latent row is blended from its four nearest guides in UV by HAAR's cosine-similarity
// rule.  The networks, the texture fetch and the local frames are the caller's (csrc/ghr_texstrands.h).
//
// The blend and its backward are csrc/ghr_haar.h's with the S drawn roots as the queries (HaarRoots): root s's UV is uvs[s], the
// output is row-major [S][C], and the first N queries are the guides themselves -- z[s] = z_g[s] for s < N, and the reference
// block's alpha[g] = f(csim[q = g]), the indexing quirk csrc/ghr_sds.h reproduces for texels, is here HAAR's eq. 4: a guide's
// coefficient comes from the guide's own neighbourhood.
//
// What is this file's own is how the backward's lists are built -- per guide the 4 s + k that chose it, ASCENDING -- in O(S K)
// plus a sort of each list: k_haar_knn counts, k_gd_start scans the counts, k_gd_fill drops each choice into its guide's range in
// arrival order (integer atomics) and k_gd_lists ranks each range into ascending order -- whatever order the choices arrived in,
// the list is the same.  tests/hostsim/ghr_hostsim_guides.cpp walks these loops on the CPU.
#pragma once
#include "ghr_haar.h"

namespace ghr {

// the place of value x among the L distinct values of t: how many are smaller
GHR_HD int gd_rank(const int32_t* t, int L, int32_t x)
{
    int r = 0;
    for (int j = 0; j < L; j++) r += t[j] < x ? 1 : 0;
    return r;
}

// the chunk of counts a lane owns in the scan of k_gd_start
GHR_HD void gd_chunk(int N, int lane, int* lo, int* hi)
{
    const int per = (N + GHR_SDS_WAVE - 1) / GHR_SDS_WAVE;
    const long long a = (long long)lane * per, b = a + per;
    *lo = (int)(a < N ? a : N);
    *hi = (int)(b < N ? b : N);
}

#if defined(__HIPCC__)

// one wave in all: each lane sums its chunk of the counts, an integer scan over the lanes, a second walk that writes
__global__ void __launch_bounds__(GHR_SDS_WAVE) k_gd_start(HaarArgs a)
{
    const int lane = threadIdx.x;
    int lo, hi;
    gd_chunk(a.N, lane, &lo, &hi);
    int sum = 0;
    for (int g = lo; g < hi; g++) sum += a.count[g];
    int run = sum;
    for (int d = 1; d < GHR_SDS_WAVE; d <<= 1) {
        const int t = __shfl_up(run, d, GHR_SDS_WAVE);
        if (lane >= d) run += t;
    }
    run -= sum;
    for (int g = lo; g < hi; g++) { a.start[g] = run; run += a.count[g]; }
    if (hi == a.N && lo < hi) a.start[a.N] = run;
}

// one thread per choice e = 4 s + k: a place in its guide's range, counted down from the range's end in arrival order; the
// counts are zero again afterwards
__global__ void __launch_bounds__(GHR_SDS_BLOCK) k_gd_fill(HaarArgs a)
{
    const int e = blockIdx.x * GHR_SDS_BLOCK + threadIdx.x;
    const int total = GHR_SDS_K * a.Q;
    if (e >= total) return;
    const int g = a.nbr[e];
    const int at = a.start[g] + atomicSub(&a.count[g], 1) - 1;
    if (at >= 0 && at < total) a.unsorted[at] = e;
}

// one wave per guide: each choice of its range goes to the place of its rank -- ascending 4 s + k, integers only
__global__ void __launch_bounds__(GHR_SDS_BLOCK) k_gd_lists(HaarArgs a)
{
    const int lane = threadIdx.x & (GHR_SDS_WAVE - 1);
    const int g = blockIdx.x * (GHR_SDS_BLOCK / GHR_SDS_WAVE) + (threadIdx.x >> 6);
    if (g >= a.N) return;
    const int beg = a.start[g], L = a.start[g + 1] - beg;
    const int total = GHR_SDS_K * a.Q;
    if (beg < 0 || L < 0 || beg + L > total) return;
    for (int i = lane; i < L; i += GHR_SDS_WAVE) {
        const int32_t x = a.unsorted[beg + i];
        a.list[beg + gd_rank(a.unsorted + beg, L, x)] = x;
    }
}

#endif  // __HIPCC__

}  // namespace ghr
