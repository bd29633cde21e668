// ghr_texstrands.h -- the textured strand generator between its two networks: the bilinear fetch of a
// [1, C, T, T] latent texture at the drawn roots' UVs, the decoded local segments summed and taken through each root's frame to
// world points, and the backward of both -- the gradient of the WHOLE texture included.  The decoders are the caller's.
//
//   taps      per root r, made once on the host in float64: x0, y0 (int32), fx, fy (float32).  Tap k = 0..3 is the texel
//             (x0 + (k & 1), y0 + (k >> 1)) with weight (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy; a tap outside 0..T-1 is dropped
//   fetch     z[s, c] = ((w0 t0 + w1 t1) + w2 t2) + w3 t3 over the taps of root idx[s] that are not dropped, in this order
//   to world  Pl[s, j] = (sum_{i < j} v[s, i]) inv_scale,  p[s, j] = origins[idx[s]] + M Pl[s, j],  M = local2world[idx[s]]
//   backward  d_v[s, i] = (M^T sum_{j > i} d_p[s, j] + sum_{j > i} d_pl[s, j]) inv_scale
//             d_texture[c, q] = sum over texel q's STATIC list of (root r, tap k), ascending, of w_k d_z[pos[r], c], skipping the
//             roots this draw left out (pos[r] = -1): every element assigned, no floating-point atomics, the order by root and
//             not by row -- two passes, or a permuted draw of the same roots, give the same bits
//
// Mapping.  k_ts_fetch: one wave per drawn root, lane = channel -- the texture is channel-major, so a root's 4 C tap reads are
// 4 C separate 4-byte gathers whichever way lanes are bound (2 C lines touched: taps k and k + 1 are neighbours in x); this
// binding makes the 4 C-byte row of z one contiguous store.  k_ts_texgrad: a workgroup takes 64 consecutive texels, each of its
// eight waves 8 of them; a wave walks a texel's list with lane = channel (a row of d_z is read contiguously), the partial row goes
// into a 64 x 192 LDS tile (rows padded to 193 floats, 49 408 B), and the workgroup writes each channel's 256 B with lane = texel;
// channels in passes of 192.  k_ts_world / k_ts_world_bwd: one wave per strand, the chunked Hillis-Steele scans of k_sds_local.
// Per-element arithmetic is GHR_HD: tests/hostsim/ghr_hostsim_texstrands.cpp runs it on the CPU.
#pragma once
#include "ghr_sds.h"

#define GHR_TS_WAVE 64
#define GHR_TS_BLOCK 256
#define GHR_TS_GRAD_BLOCK 512  // k_ts_texgrad: eight waves, eight texels each
#define GHR_TS_TEXELS 64       // texels per workgroup of k_ts_texgrad
#define GHR_TS_CHUNK 64        // channels a lane-wide access covers
#define GHR_TS_PASS 3          // such chunks per pass over the lists: 192 channels in registers, the yaml's 129 in one pass
#define GHR_TS_PITCH (GHR_TS_CHUNK * GHR_TS_PASS + 1)  // floats per tile row (193 = 1 mod 32): lane = texel reads fall on 32 banks

namespace ghr {

// tap k of (x0, y0) lies inside the T x T texture; written so that no x0 + 1 can overflow
GHR_HD bool ts_tap_in(int32_t x0, int32_t y0, int k, int32_t T)
{
    const int32_t dx = k & 1, dy = k >> 1;
    return x0 >= -dx && x0 < T - dx && y0 >= -dy && y0 < T - dy;
}

GHR_HD float ts_weight(int k, float fx, float fy)
{
    const float ax = (k & 1) ? fx : 1.f - fx, ay = (k >> 1) ? fy : 1.f - fy;
    return ax * ay;
}

// the sum of the taps that are present, left to right; no tap: 0
GHR_HD float ts_mix(const float* w, const float* t, const bool* in)
{
    float acc = 0.f;
    bool first = true;
    for (int k = 0; k < 4; k++) {
        if (!in[k]) continue;
        const float term = w[k] * t[k];
        acc = first ? term : acc + term;
        first = false;
    }
    return acc;
}

// Pl = run inv_scale; p = origin + M Pl (sds_mv's product and bracketing)
GHR_HD void ts_point(const float* M, const float* origin, const float* run, float inv_scale, float* pl, float* p)
{
    float o[3];
    for (int c = 0; c < 3; c++) pl[c] = run[c] * inv_scale;
    sds_mv(M, pl, 1.f, o);
    for (int c = 0; c < 3; c++) p[c] = origin[c] + o[c];
}

// d_v = (M^T rp + rl) inv_scale
GHR_HD void ts_point_vjp(const float* M, const float* rp, const float* rl, float inv_scale, float* dv)
{
    float o[3];
    sds_mtv(M, rp, 1.f, o);
    for (int c = 0; c < 3; c++) dv[c] = (o[c] + rl[c]) * inv_scale;
}

#if defined(__HIPCC__)

struct TsFetchArgs {
    int32_t Smax, S, T, C, list_len;
    const float* texture;  // [C][T][T]
    const int32_t* x0;     // [Smax]
    const int32_t* y0;     // [Smax]
    const float* fx;       // [Smax]
    const float* fy;       // [Smax]
    const int64_t* idx;    // [S]
    float* z;              // [S][C]
    // backward
    const int32_t* start;  // [T T + 1]
    const int32_t* list;   // [list_len]: 4 r + k, ascending within a texel
    const float* d_z;      // [S][C]
    int32_t* pos;          // [Smax]
    float* d_texture;      // [C][T][T]
};

// one wave per drawn root, lane = channel
__global__ void __launch_bounds__(GHR_TS_BLOCK) k_ts_fetch(TsFetchArgs a)
{
    const int lane = threadIdx.x & (GHR_TS_WAVE - 1);
    const int s = blockIdx.x * (GHR_TS_BLOCK / GHR_TS_WAVE) + (threadIdx.x >> 6);
    if (s >= a.S) return;
    const int64_t r = a.idx[s];
    float* z = a.z + (size_t)s * a.C;
    if (r < 0 || r >= a.Smax) {  // an index outside the roots names none: the row says so, nothing is read
        for (int c = lane; c < a.C; c += GHR_TS_WAVE) z[c] = NAN;
        return;
    }
    const int32_t x0 = a.x0[r], y0 = a.y0[r];
    const float fx = a.fx[r], fy = a.fy[r];
    const size_t TT = (size_t)a.T * a.T;
    float w[4];
    bool in[4];
    size_t at[4];
    for (int k = 0; k < 4; k++) {
        in[k] = ts_tap_in(x0, y0, k, a.T);
        w[k] = ts_weight(k, fx, fy);
        at[k] = in[k] ? (size_t)(y0 + (k >> 1)) * a.T + (size_t)(x0 + (k & 1)) : 0;
    }
    for (int c = lane; c < a.C; c += GHR_TS_WAVE) {
        const float* plane = a.texture + (size_t)c * TT;
        float t[4];
        for (int k = 0; k < 4; k++) t[k] = in[k] ? plane[at[k]] : 0.f;
        z[c] = ts_mix(w, t, in);
    }
}

// pos[idx[s]] = s over a pos the entry point has filled with -1
__global__ void __launch_bounds__(GHR_TS_BLOCK) k_ts_positions(TsFetchArgs a)
{
    const int s = blockIdx.x * GHR_TS_BLOCK + threadIdx.x;
    if (s >= a.S) return;
    const int64_t r = a.idx[s];
    if (r >= 0 && r < a.Smax) a.pos[r] = s;
}

// a workgroup per 64 consecutive texels; see the mapping at the top of the file.  The lists of a wave's consecutive texels are
// one contiguous stretch of `list`: the wave fetches its boundaries with one load (lane = texel) and the stretch 64 entries at a
// time (lane = entry: entry, pos, weight), so the walk itself waits only for the rows of d_z.
__global__ void __launch_bounds__(GHR_TS_GRAD_BLOCK) k_ts_texgrad(TsFetchArgs a)
{
    __shared__ float tile[GHR_TS_TEXELS * GHR_TS_PITCH];
    const int lane = threadIdx.x & (GHR_TS_WAVE - 1), wave = threadIdx.x >> 6;
    const int64_t TT = (int64_t)a.T * a.T;
    const int64_t q0 = (int64_t)blockIdx.x * GHR_TS_TEXELS;
    constexpr int PER = GHR_TS_TEXELS / (GHR_TS_GRAD_BLOCK / GHR_TS_WAVE);  // texels per wave
    int bound = 0;  // lane i <= PER: where the list of the wave's texel i begins (texels past the texture: empty lists)
    if (lane <= PER) {
        const int64_t q = q0 + wave * PER + lane;
        bound = a.start[q < TT ? q : TT];
        bound = bound < 0 ? 0 : (bound > a.list_len ? a.list_len : bound);
    }
    const int wave_end = __shfl(bound, PER, GHR_TS_WAVE);
    for (int c0 = 0; c0 < a.C; c0 += GHR_TS_CHUNK * GHR_TS_PASS) {
        int base = -1, pl = -1;
        float wl = 0.f;
        for (int i = 0; i < PER; i++) {
            const int beg = __shfl(bound, i, GHR_TS_WAVE), end = __shfl(bound, i + 1, GHR_TS_WAVE);
            float acc[GHR_TS_PASS];
#pragma unroll
            for (int ch = 0; ch < GHR_TS_PASS; ch++) acc[ch] = 0.f;
            for (int t = beg; t < end; t++) {
                if (base < 0 || t - base >= GHR_TS_WAVE) {  // the next 64 entries of the wave's stretch, lane = entry
                    base = t;
                    pl = -1;
                    wl = 0.f;
                    const int te = base + lane;
                    if (te < wave_end) {
                        const int32_t e = a.list[te], r = e >> 2;
                        if (r >= 0 && r < a.Smax) {
                            const int32_t p = a.pos[r];
                            if (p >= 0 && p < a.S) { pl = p; wl = ts_weight(e & 3, a.fx[r], a.fy[r]); }
                        }
                    }
                }
                const int p = __shfl(pl, t - base, GHR_TS_WAVE);
                const float w = __shfl(wl, t - base, GHR_TS_WAVE);
                if (p < 0) continue;  // a root this draw left out
                const float* row = a.d_z + (size_t)p * a.C;
#pragma unroll
                for (int ch = 0; ch < GHR_TS_PASS; ch++) {
                    const int c = c0 + ch * GHR_TS_CHUNK + lane;
                    if (c < a.C) acc[ch] += w * row[c];
                }
            }
#pragma unroll
            for (int ch = 0; ch < GHR_TS_PASS; ch++) tile[(wave * PER + i) * GHR_TS_PITCH + ch * GHR_TS_CHUNK + lane] = acc[ch];
        }
        __syncthreads();
        const int64_t q = q0 + lane;
        if (q < TT)
            for (int cc = wave; cc < GHR_TS_CHUNK * GHR_TS_PASS && c0 + cc < a.C; cc += GHR_TS_GRAD_BLOCK / GHR_TS_WAVE)
                a.d_texture[(size_t)(c0 + cc) * TT + q] = tile[lane * GHR_TS_PITCH + cc];
        __syncthreads();
    }
}

struct TsWorldArgs {
    int32_t Smax, S, n;
    float inv_scale;
    const float* v;        // [S][n][3]
    const float* frames;   // [Smax][3][3]: local2world
    const float* origins;  // [Smax][3]
    const int64_t* idx;    // [S]
    float* p;              // [S][n + 1][3]
    float* p_local;        // [S][n + 1][3], may be NULL
    const float* d_p;      // may be NULL
    const float* d_pl;     // may be NULL
    float* d_v;            // [S][n][3]
};

// one wave per strand: lane totals of its chunk of segments, a scan over the lanes, a second walk that writes
__global__ void __launch_bounds__(GHR_TS_BLOCK) k_ts_world(TsWorldArgs a)
{
    const int lane = threadIdx.x & (GHR_TS_WAVE - 1);
    const int s = blockIdx.x * (GHR_TS_BLOCK / GHR_TS_WAVE) + (threadIdx.x >> 6);
    if (s >= a.S) return;
    const int64_t r = a.idx[s];
    const int n = a.n;
    float* p = a.p + (size_t)s * (n + 1) * 3;
    float* pl = a.p_local ? a.p_local + (size_t)s * (n + 1) * 3 : nullptr;
    int lo, hi;
    sds_chunk(n, lane, &lo, &hi);
    if (r < 0 || r >= a.Smax) {
        for (int i = lo; i < hi; i++)
            for (int c = 0; c < 3; c++) { p[(i + 1) * 3 + c] = NAN; if (pl) pl[(i + 1) * 3 + c] = NAN; }
        if (lane == 0)
            for (int c = 0; c < 3; c++) { p[c] = NAN; if (pl) pl[c] = NAN; }
        return;
    }
    float M[9], org[3];
    for (int i = 0; i < 9; i++) M[i] = a.frames[(size_t)r * 9 + i];
    for (int c = 0; c < 3; c++) org[c] = a.origins[(size_t)r * 3 + c];
    const float* v = a.v + (size_t)s * n * 3;
    float run[3] = {0.f, 0.f, 0.f};
    for (int i = lo; i < hi; i++)
        for (int c = 0; c < 3; c++) run[c] += v[i * 3 + c];
    for (int c = 0; c < 3; c++) run[c] = sds_wave_excl(run[c], lane, +1);
    if (lane == 0)
        for (int c = 0; c < 3; c++) { p[c] = org[c]; if (pl) pl[c] = 0.f; }
    for (int i = lo; i < hi; i++) {
        float l[3], w[3];
        for (int c = 0; c < 3; c++) run[c] += v[i * 3 + c];
        ts_point(M, org, run, a.inv_scale, l, w);
        for (int c = 0; c < 3; c++) { p[(i + 1) * 3 + c] = w[c]; if (pl) pl[(i + 1) * 3 + c] = l[c]; }
    }
}

// one wave per strand: the matching suffix scans of d_p and d_p_local
__global__ void __launch_bounds__(GHR_TS_BLOCK) k_ts_world_bwd(TsWorldArgs a)
{
    const int lane = threadIdx.x & (GHR_TS_WAVE - 1);
    const int s = blockIdx.x * (GHR_TS_BLOCK / GHR_TS_WAVE) + (threadIdx.x >> 6);
    if (s >= a.S) return;
    const int64_t r = a.idx[s];
    const int n = a.n;
    float* dv = a.d_v + (size_t)s * n * 3;
    int lo, hi;
    sds_chunk(n, lane, &lo, &hi);
    if (r < 0 || r >= a.Smax) {
        for (int i = lo; i < hi; i++)
            for (int c = 0; c < 3; c++) dv[i * 3 + c] = NAN;
        return;
    }
    float M[9];
    for (int i = 0; i < 9; i++) M[i] = a.frames[(size_t)r * 9 + i];
    const float* dp = a.d_p ? a.d_p + (size_t)s * (n + 1) * 3 : nullptr;
    const float* dl = a.d_pl ? a.d_pl + (size_t)s * (n + 1) * 3 : nullptr;
    float rp[3] = {0.f, 0.f, 0.f}, rl[3] = {0.f, 0.f, 0.f};
    for (int i = hi - 1; i >= lo; i--)
        for (int c = 0; c < 3; c++) {
            if (dp) rp[c] += dp[(i + 1) * 3 + c];
            if (dl) rl[c] += dl[(i + 1) * 3 + c];
        }
    for (int c = 0; c < 3; c++) {
        if (dp) rp[c] = sds_wave_excl(rp[c], lane, -1);
        if (dl) rl[c] = sds_wave_excl(rl[c], lane, -1);
    }
    for (int i = hi - 1; i >= lo; i--) {
        float o[3];
        for (int c = 0; c < 3; c++) {
            if (dp) rp[c] += dp[(i + 1) * 3 + c];
            if (dl) rl[c] += dl[(i + 1) * 3 + c];
        }
        ts_point_vjp(M, rp, rl, a.inv_scale, o);
        for (int c = 0; c < 3; c++) dv[i * 3 + c] = o[c];
    }
}

#endif  // __HIPCC__

}  // namespace ghr
