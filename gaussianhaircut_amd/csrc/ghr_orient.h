// ghr_orient.h -- ground-truth orientation maps from an image: difference of Gaussians, then a bank of oriented Gabor filters
// with the arg-max angle and its circular variance per pixel.
//
// Reference: src/preprocessing/calc_orientation_maps.py (rgb2gray, skimage's difference_of_gaussians(gray, 0.4, 10) -- two
// scipy.ndimage.gaussian_filter calls in float64, mode 'nearest' --, generate_gabor_filters, calc_orients) and the loader of its
// two files, src/utils/camera_utils.py:66-68.  The reference runs the bank as nn.Conv2d(1, 180, 17) over 64 x 64 patches, 256
// launches per 1024^2 image plus a dozen elementwise kernels per patch.  Here, per image:
//   k_orient_dog<0>   grey value and both Gaussians along axis 0, in double, into a scratch of two double planes
//   k_orient_dog<1>   both Gaussians along axis 1, their difference narrowed to the float32 plane
//   k_orient_gabor    the whole bank as an implicit GEMM (filters x taps against taps x pixels) on v_mfma_f32_16x16x4_f32, the
//                     |response|, first-maximum arg-max, sum and variance in the epilogue: the n_filters responses of a pixel
//                     never reach memory.  Writes deg (uint8), var, angle = deg / 180 and conf = 1 / ((var / pi^2)^2 + 1e-7).
// The MFMA is exact fp32 (a k-ordered fmaf chain), every reduction has a fixed order, there are no atomics: the same bits
// run after run.  The per-pixel arithmetic is in __host__ __device__ functions (dog_tap_sum, orient_grey, orient_better,
// orient_dist, orient_var_finish, orient_conf_of; orient_pick composes them sequentially) so that
// tests/hostsim/ghr_hostsim_orient.cpp runs it on the CPU.
#pragma once
#include "ghr_device.h"

namespace ghr {

#define GHR_ORIENT_MAX_FILTERS 256
#define GHR_ORIENT_MAX_KSIZE 25
#define GHR_ORIENT_TW 16     // pixel columns of a workgroup = the N of the MFMA
#define GHR_ORIENT_TH 8      // pixel rows of a workgroup = pixel groups (accumulator sets) of a wave
#define GHR_ORIENT_WAVES 4   // the filter tiles of a pixel group are dealt over these
#define GHR_ORIENT_PIX (GHR_ORIENT_TW * GHR_ORIENT_TH)
#define GHR_ORIENT_LDS_TILE ((GHR_ORIENT_TH + GHR_ORIENT_MAX_KSIZE - 1) * (GHR_ORIENT_TW + GHR_ORIENT_MAX_KSIZE - 1))

// ---- difference of Gaussians ----------------------------------------------------------------------------------------------

// rgb2gray in float64 on the 0 ... 255 (uint8) or float32 image, [H,W,channels] interleaved; one channel: the value itself
GHR_HD double orient_grey(const void* image, int is_u8, int channels, size_t pix)
{
    double c[3];
    for (int k = 0; k < channels; k++)
        c[k] = is_u8 ? (double)((const uint8_t*)image)[pix * channels + k] : (double)((const float*)image)[pix * channels + k];
    if (channels == 1) return c[0];
    return (0.2989 * c[0] + 0.5870 * c[1]) + 0.1140 * c[2];
}

// One output of scipy.ndimage.correlate1d with a symmetric filter w[0 .. 2 r] and mode 'nearest': the centre tap first, then the
// mirrored pairs from the outermost inwards, indices clamped to [0, n).  get(i): element i of the line, as double.
template <class Get>
GHR_HD double dog_tap_sum(Get get, int pos, int n, int r, const double* w)
{
    double t = get(pos) * w[r];
    for (int j = -r; j < 0; j++) {
        const int lo = pos + j < 0 ? 0 : pos + j, hi = pos - j > n - 1 ? n - 1 : pos - j;
        t += (get(lo) + get(hi)) * w[j + r];
    }
    return t;
}

struct OrientDogArgs {
    int W, H, channels, is_u8;
    const void* image;
    int r_low, r_high;
    const double* w_low;   // [2 r_low + 1]
    const double* w_high;  // [2 r_high + 1]
    double* scratch;       // [2][H][W]: the low and the high Gaussian after axis 0
    float* filtered;       // [H][W]
};

GHR_HD void dog_axis0(const OrientDogArgs& a, int x, int y, double* low, double* high)
{
    auto get = [&](int i) { return orient_grey(a.image, a.is_u8, a.channels, (size_t)i * a.W + x); };
    *low = dog_tap_sum(get, y, a.H, a.r_low, a.w_low);
    *high = dog_tap_sum(get, y, a.H, a.r_high, a.w_high);
}

GHR_HD float dog_axis1(const OrientDogArgs& a, int x, int y)
{
    const size_t N = (size_t)a.W * a.H;
    const double* row = a.scratch + (size_t)y * a.W;
    auto get_low = [&](int i) { return row[i]; };
    auto get_high = [&](int i) { return row[N + i]; };
    return (float)(dog_tap_sum(get_low, x, a.W, a.r_low, a.w_low) - dog_tap_sum(get_high, x, a.W, a.r_high, a.w_high));
}

template <int AXIS>
__global__ __launch_bounds__(256) void k_orient_dog(OrientDogArgs a)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const size_t p = (size_t)y * a.W + x;
    if (AXIS == 0) {
        double low, high;
        dog_axis0(a, x, y, &low, &high);
        a.scratch[p] = low;
        a.scratch[(size_t)a.W * a.H + p] = high;
    } else {
        a.filtered[p] = dog_axis1(a, x, y);
    }
}

// ---- the filter bank ---------------------------------------------------------------------------------------------------------

// the first maximum wins: a later filter takes over only with a strictly larger response
GHR_HD bool orient_better(float F, int k, float bestF, int bestK) { return F > bestF || (F == bestF && k < bestK); }

// calc_orientation_maps.py:81: deg / num_filters * pi, in float32
GHR_HD float orient_rad(int deg, int n_filters) { return (float)deg / (float)n_filters * 3.14159265358979323846f; }

// :82-84: the distance of two orientations, which live on a circle of circumference pi
GHR_HD float orient_dist(float o, float theta)
{
    const float PI = 3.14159265358979323846f;
    const float d = o - theta;
    return fminf(fabsf(d), fminf(fabsf(d - PI), fabsf(d + PI)));
}

// :79, :85: sum_k d_k^2 F_k / max(sum_k F_k, 1e-12) (F.normalize(p = 1)'s floor)
GHR_HD float orient_var_finish(float num, float sum) { return num / fmaxf(sum, 1e-12f); }

// camera_utils.py:67-68: 1 / ((var / pi^2)^2 + 1e-7), var as the float16 the reference's file holds when via_half
GHR_HD float orient_conf_of(float var, int via_half)
{
    const float v = via_half ? (float)(_Float16)var : var;
    const float q = v / 9.869604401089358f;
    return 1.f / (q * q + 1e-7f);
}

// The pick and the variance of one pixel's response vector, sequentially (the kernel's epilogue is the same functions folded
// over lanes and waves).
GHR_HD void orient_pick(const float* resp, int n_filters, const float* thetas, int* deg, float* var)
{
    float bestF = -1.f, sum = 0.f;
    int bestK = 0;
    for (int k = 0; k < n_filters; k++) {
        const float F = fabsf(resp[k]);
        if (orient_better(F, k, bestF, bestK)) { bestF = F; bestK = k; }
        sum += F;
    }
    const float o = orient_rad(bestK, n_filters);
    float num = 0.f;
    for (int k = 0; k < n_filters; k++) {
        const float d = orient_dist(o, thetas[k]);
        num += d * d * fabsf(resp[k]);
    }
    *deg = bestK;
    *var = orient_var_finish(num, sum);
}

struct OrientGaborArgs {
    int W, H;
    const float* plane;    // [H][W]
    int n_filters, ksize;
    int n_chunks;          // ceil(ksize^2 / 4): k steps of the MFMA
    const float* wfrag;    // [4 NT tiles][n_chunks][64]: lane l holds filter 16 tile + (l & 15), tap 4 chunk + (l >> 4); zero padded
    const float* thetas;   // [n_filters]
    uint8_t* deg;          // each of the four may be NULL
    float* var;
    float* angle;
    float* conf;
    int via_half;
};

__device__ __forceinline__ f4 orient_mfma(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// One workgroup: a 16 x 8 pixel tile against every filter.  Wave w owns the filter tiles w, w + 4, ..., w + 4 (NT - 1) of all
// eight pixel rows: NT x 8 accumulators of 4 registers that never leave the register file.  The B operand (tap 4 c + (l >> 4) of
// pixel column l & 15) is gathered from the LDS image of the tile and its halo; the A operand comes through L2 in fragment order.
template <int NT>
__global__ __launch_bounds__(64 * GHR_ORIENT_WAVES, NT <= 3 ? 2 : 1) void k_orient_gabor(OrientGaborArgs a)
{
    __shared__ float tile[GHR_ORIENT_LDS_TILE];
    __shared__ float red_f[2][GHR_ORIENT_WAVES][GHR_ORIENT_PIX];  // [0]: largest |response|, then the variance numerator; [1]: sum
    __shared__ int red_k[GHR_ORIENT_WAVES][GHR_ORIENT_PIX];

    const int K = a.ksize, R = K >> 1, KK = K * K;
    const int pitch = GHR_ORIENT_TW + K - 1, rows = GHR_ORIENT_TH + K - 1;
    const int x0 = blockIdx.x * GHR_ORIENT_TW, y0 = blockIdx.y * GHR_ORIENT_TH;
    for (int i = threadIdx.x; i < pitch * rows; i += 64 * GHR_ORIENT_WAVES) {
        const int ty = i / pitch, tx = i - ty * pitch;
        const int x = x0 + tx - R, y = y0 + ty - R;
        tile[i] = (x >= 0 && x < a.W && y >= 0 && y < a.H) ? a.plane[(size_t)y * a.W + x] : 0.f;  // nn.Conv2d's zero padding
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, kq = lane >> 4;
    f4 acc[NT][GHR_ORIENT_TH];
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int g = 0; g < GHR_ORIENT_TH; g++) acc[t][g] = f4{0.f, 0.f, 0.f, 0.f};

    const float* wp[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) wp[t] = a.wfrag + (size_t)(wave + GHR_ORIENT_WAVES * t) * a.n_chunks * 64 + lane;
    float wv[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) wv[t] = wp[t][0];
    int tap = kq, dy = kq / K, dx = kq - dy * K;
    float b[GHR_ORIENT_TH];
    {
        const int off = tap < KK ? dy * pitch + dx + col : col;  // a padded tap has weight 0: any finite pixel will do
#pragma unroll
        for (int g = 0; g < GHR_ORIENT_TH; g++) b[g] = tile[off + g * pitch];
    }
    for (int c = 0; c < a.n_chunks; c++) {
        // the next chunk's operands, in flight under this chunk's MFMAs (the last chunk reloads itself)
        const int cn = c + 1 < a.n_chunks ? c + 1 : c;
        float wn[NT], bn[GHR_ORIENT_TH];
#pragma unroll
        for (int t = 0; t < NT; t++) wn[t] = wp[t][(size_t)cn * 64];
        if (cn != c) {
            tap += 4;
            dx += 4;
            while (dx >= K) { dx -= K; dy++; }
        }
        const int off = tap < KK ? dy * pitch + dx + col : col;
#pragma unroll
        for (int g = 0; g < GHR_ORIENT_TH; g++) bn[g] = tile[off + g * pitch];
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int g = 0; g < GHR_ORIENT_TH; g++) acc[t][g] = orient_mfma(wv[t], b[g], acc[t][g]);
#pragma unroll
        for (int t = 0; t < NT; t++) wv[t] = wn[t];
#pragma unroll
        for (int g = 0; g < GHR_ORIENT_TH; g++) b[g] = bn[g];
    }

    // Epilogue.  acc[t][g][r] is filter 16 (wave + 4 t) + 4 kq + r at pixel (row g, column col).
    float sum[GHR_ORIENT_TH];
    int bestK[GHR_ORIENT_TH];
#pragma unroll
    for (int g = 0; g < GHR_ORIENT_TH; g++) {
        float bF = -1.f, s = 0.f;
        int bK = 0;
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float F = fabsf(acc[t][g][r]);
                const int k = 16 * (wave + GHR_ORIENT_WAVES * t) + 4 * kq + r;
                acc[t][g][r] = F;
                if (orient_better(F, k, bF, bK)) { bF = F; bK = k; }
                s += F;
            }
#pragma unroll
        for (int m = 16; m <= 32; m <<= 1) {  // the four lane groups of the wave
            const float oF = __shfl_xor(bF, m), oS = __shfl_xor(s, m);
            const int oK = __shfl_xor(bK, m);
            if (orient_better(oF, oK, bF, bK)) { bF = oF; bK = oK; }
            s += oS;
        }
        if (kq == 0) {
            red_f[0][wave][g * GHR_ORIENT_TW + col] = bF;
            red_f[1][wave][g * GHR_ORIENT_TW + col] = s;
            red_k[wave][g * GHR_ORIENT_TW + col] = bK;
        }
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < GHR_ORIENT_TH; g++) {  // the waves, in order: every lane of a pixel arrives at the same pick
        const int p = g * GHR_ORIENT_TW + col;
        float bF = red_f[0][0][p], s = red_f[1][0][p];
        int bK = red_k[0][p];
#pragma unroll
        for (int w = 1; w < GHR_ORIENT_WAVES; w++) {
            const float oF = red_f[0][w][p];
            const int oK = red_k[w][p];
            if (orient_better(oF, oK, bF, bK)) { bF = oF; bK = oK; }
            s += red_f[1][w][p];
        }
        bestK[g] = bK; sum[g] = s;
    }
    __syncthreads();  // red_f[0] is reused for the variance numerators
    float th[NT][4];
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int k = 16 * (wave + GHR_ORIENT_WAVES * t) + 4 * kq + r;
            th[t][r] = k < a.n_filters ? a.thetas[k] : 0.f;  // a padding filter's response is exactly 0
        }
#pragma unroll
    for (int g = 0; g < GHR_ORIENT_TH; g++) {
        const float o = orient_rad(bestK[g], a.n_filters);
        float num = 0.f;
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float d = orient_dist(o, th[t][r]);
                num += d * d * acc[t][g][r];
            }
        num += __shfl_xor(num, 16);
        num += __shfl_xor(num, 32);
        if (kq == 0) red_f[0][wave][g * GHR_ORIENT_TW + col] = num;
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < GHR_ORIENT_TH; g++) {  // each wave writes two of the rows, 16 lanes a row
        if (g / (GHR_ORIENT_TH / GHR_ORIENT_WAVES) != wave || kq != 0) continue;
        const int p = g * GHR_ORIENT_TW + col, x = x0 + col, y = y0 + g;
        if (x >= a.W || y >= a.H) continue;
        float num = red_f[0][0][p];
#pragma unroll
        for (int w = 1; w < GHR_ORIENT_WAVES; w++) num += red_f[0][w][p];
        const float v = orient_var_finish(num, sum[g]);
        const size_t i = (size_t)y * a.W + x;
        if (a.deg) a.deg[i] = (uint8_t)bestK[g];
        if (a.var) a.var[i] = v;
        if (a.angle) a.angle[i] = (float)bestK[g] / 180.f;
        if (a.conf) a.conf[i] = orient_conf_of(v, a.via_half);
    }
}

}  // namespace ghr
