// ghr_hostsim_capture.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Compiles gaussianhaircut_amd/csrc/ghr_capture.h as plain C++ for the host and walks k_sv_capture's pixels with the product's own
// per-pixel function (cap_pixel_one: the subsamples in the definition's order, the remembered projection, the masks, the bin and
// the variance).  tests/test_capture_cpu.py loads this as a shared library; ghr_capture_selfcheck.cpp includes it and adds a main().
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../gaussianhaircut_amd/csrc/ghr_capture.h"

extern "C" {

int ghrsim_cap_bins(void) { return GHR_CAP_BINS; }

// ghr_strandview_capture on the host; walk = 0: every pixel through cap_pixel_one; walk = 1: the kernel's form -- quads of four
// consecutive pixels, the table read once per entry for the four, the bytes packed into dwords.  Returns 0.
int ghrsim_capture(int S, int L, const float* points, const float* Ms, float near_w, int H, int W, int s, int F,
                   const int32_t* pix_to_segment, const int32_t* pix_to_face_out, const float* table, float var_floor,
                   uint8_t* mask_hair, uint8_t* mask_body, uint8_t* angle, float* var, int walk)
{
    const size_t N = (size_t)H * W;
    if (walk == 0) {
        for (int i = 0; i < H; i++)
            for (int j = 0; j < W; j++) {
                const size_t p = (size_t)i * W + j;
                ghr::cap_pixel_one(i, j, W, s, pix_to_segment, pix_to_face_out, S, L, points, Ms, near_w, F, table, var_floor,
                                   mask_hair + p, mask_body + p, angle + p, var + p);
            }
        return 0;
    }
    const int n = s * s;
    const int64_t n_seg = (int64_t)S * (L - 1);
    for (size_t p0 = 0; p0 < N; p0 += GHR_CAP_QUAD) {
        float C[GHR_CAP_QUAD], Sm[GHR_CAP_QUAD], best[GHR_CAP_QUAD];
        uint32_t hair = 0u, body = 0u, arg[GHR_CAP_QUAD];
        for (int q = 0; q < GHR_CAP_QUAD; q++) {
            ghr::CapAcc acc = ghr::cap_begin();
            if (p0 + q < N) {
                const size_t i = (p0 + q) / W, j = (p0 + q) % W;
                for (int a = 0; a < s; a++)
                    for (int b = 0; b < s; b++) {
                        const size_t o = (i * s + a) * ((size_t)W * s) + j * s + b;
                        if (o >= N * n) std::abort();
                        ghr::cap_sample(acc, pix_to_segment[o], pix_to_face_out[o], n_seg, F, L, points, Ms, near_w);
                    }
            }
            C[q] = acc.C; Sm[q] = acc.S; best[q] = -INFINITY; arg[q] = 0u;
            hair |= ghr::cap_mask(acc.n_hair, n) << (8 * q);
            body |= ghr::cap_mask(acc.n_hair + acc.n_face, n) << (8 * q);
        }
        for (uint32_t k = 0u; k < GHR_CAP_BINS; k++)
            for (int q = 0; q < GHR_CAP_QUAD; q++) {
                const float score = C[q] * table[2 * k] + Sm[q] * table[2 * k + 1];
                if (score > best[q]) { best[q] = score; arg[q] = k; }
            }
        for (int q = 0; q < GHR_CAP_QUAD && p0 + q < N; q++) {
            mask_hair[p0 + q] = (uint8_t)(hair >> (8 * q));
            mask_body[p0 + q] = (uint8_t)(body >> (8 * q));
            angle[p0 + q] = (uint8_t)arg[q];
            var[p0 + q] = ghr::cap_var(C[q], Sm[q], n, var_floor);
        }
    }
    return 0;
}

}  // extern "C"
