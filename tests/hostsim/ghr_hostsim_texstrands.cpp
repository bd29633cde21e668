// ghr_hostsim_texstrands.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Compiles gaussianhaircut_amd/csrc/ghr_texstrands.h as plain C++ for the host and walks the five kernels' loops with a 64-lane
// wave kept in arrays: the same GHR_HD arithmetic, the same split of the work over lanes and waves, the same Hillis-Steele order,
// the same LDS tile with its pitch.  Every index a walk forms is checked (TS_CHECK aborts with the expression).
// tests/test_textured_strands_cpu.py loads this as a shared library; ghr_texstrands_selfcheck.cpp includes it and adds a main().
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../gaussianhaircut_amd/csrc/ghr_texstrands.h"

#define TS_CHECK(cond)                                                                                  \
    do {                                                                                                \
        if (!(cond)) {                                                                                  \
            std::fprintf(stderr, "ghr_hostsim_texstrands.cpp:%d: check failed: %s\n", __LINE__, #cond); \
            std::abort();                                                                               \
        }                                                                                               \
    } while (0)

namespace {

constexpr int TWV = GHR_TS_WAVE;

void ts_wave_excl(float* x, int dir)  // sds_wave_excl
{
    for (int d = 1; d < TWV; d <<= 1) {
        float t[TWV];
        for (int l = 0; l < TWV; l++) {
            const int from = dir > 0 ? l - d : l + d;
            t[l] = (from >= 0 && from < TWV) ? x[l] + x[from] : x[l];
        }
        std::memcpy(x, t, sizeof(t));
    }
    float t[TWV];
    for (int l = 0; l < TWV; l++) {
        const int from = dir > 0 ? l - 1 : l + 1;
        t[l] = (from >= 0 && from < TWV) ? x[from] : 0.f;
    }
    std::memcpy(x, t, sizeof(t));
}

}  // namespace

extern "C" {

int ghrsim_ts_wave(void) { return TWV; }
int ghrsim_ts_tile_bytes(void) { return GHR_TS_TEXELS * GHR_TS_PITCH * (int)sizeof(float); }
float ghrsim_ts_weight(int k, float fx, float fy) { return ghr::ts_weight(k, fx, fy); }
int ghrsim_ts_tap_in(int x0, int y0, int k, int T) { return ghr::ts_tap_in(x0, y0, k, T) ? 1 : 0; }

// k_ts_fetch
void ghrsim_ts_fetch(int Smax, int S, int T, int C, const float* texture, const int32_t* x0, const int32_t* y0, const float* fx,
                     const float* fy, const int64_t* idx, float* z)
{
    const size_t TT = (size_t)T * T;
    for (int s = 0; s < S; s++) {
        const long long r = idx[s];
        TS_CHECK(r >= 0 && r < Smax);
        float w[4];
        bool in[4];
        size_t at[4];
        for (int k = 0; k < 4; k++) {
            in[k] = ghr::ts_tap_in(x0[r], y0[r], k, T);
            w[k] = ghr::ts_weight(k, fx[r], fy[r]);
            at[k] = in[k] ? (size_t)(y0[r] + (k >> 1)) * T + (size_t)(x0[r] + (k & 1)) : 0;
            TS_CHECK(at[k] < TT);
        }
        for (int lane = 0; lane < TWV; lane++)
            for (int c = lane; c < C; c += TWV) {
                float t[4];
                for (int k = 0; k < 4; k++) t[k] = in[k] ? texture[(size_t)c * TT + at[k]] : 0.f;
                z[(size_t)s * C + c] = ghr::ts_mix(w, t, in);
            }
    }
}

// the fill, k_ts_positions and k_ts_texgrad: workgroup by workgroup, wave by wave, with the LDS tile
void ghrsim_ts_fetch_backward(int Smax, int S, int T, int C, const float* fx, const float* fy, const int32_t* start,
                              const int32_t* list, int list_len, const int64_t* idx, const float* d_z, int32_t* pos, float* d_texture)
{
    for (int r = 0; r < Smax; r++) pos[r] = -1;
    for (int s = 0; s < S; s++) {
        TS_CHECK(idx[s] >= 0 && idx[s] < Smax);
        TS_CHECK(pos[idx[s]] == -1);  // no root twice
        pos[idx[s]] = s;
    }
    const long long TT = (long long)T * T;
    constexpr int WAVES = GHR_TS_GRAD_BLOCK / GHR_TS_WAVE, PER = GHR_TS_TEXELS / WAVES, SPAN = GHR_TS_CHUNK * GHR_TS_PASS;
    std::vector<float> tile((size_t)GHR_TS_TEXELS * GHR_TS_PITCH);
    for (long long q0 = 0; q0 < TT; q0 += GHR_TS_TEXELS) {
        for (int c0 = 0; c0 < C; c0 += SPAN) {
            for (int wave = 0; wave < WAVES; wave++) {
                int bound[PER + 1];  // the boundaries the wave's lanes 0 .. PER fetch
                for (int l = 0; l <= PER; l++) {
                    const long long q = q0 + wave * PER + l;
                    bound[l] = start[q < TT ? q : TT];
                    TS_CHECK(0 <= bound[l] && bound[l] <= list_len && (l == 0 || bound[l - 1] <= bound[l]));
                }
                const int wave_end = bound[PER];
                int base = -1, pl[TWV];
                float wl[TWV];
                for (int i = 0; i < PER; i++) {
                    const int tl = wave * PER + i;
                    float acc[SPAN];
                    for (int c = 0; c < SPAN; c++) acc[c] = 0.f;
                    for (int t = bound[i]; t < bound[i + 1]; t++) {
                        if (base < 0 || t - base >= TWV) {
                            base = t;
                            for (int l = 0; l < TWV; l++) {  // lane = entry
                                pl[l] = -1;
                                wl[l] = 0.f;
                                const int te = base + l;
                                if (te >= wave_end) continue;
                                const int32_t e = list[te], r = e >> 2;
                                TS_CHECK(r >= 0 && r < Smax);
                                const int32_t p = pos[r];
                                if (p < 0) continue;
                                TS_CHECK(p < S);
                                pl[l] = p;
                                wl[l] = ghr::ts_weight(e & 3, fx[r], fy[r]);
                            }
                        }
                        TS_CHECK(t - base >= 0 && t - base < TWV);
                        TS_CHECK(t == bound[i] || list[t - 1] < list[t]);  // ascending (r, k) within a texel
                        const int p = pl[t - base];
                        const float w = wl[t - base];
                        if (p < 0) continue;
                        for (int c = 0; c < SPAN && c0 + c < C; c++) acc[c] += w * d_z[(size_t)p * C + c0 + c];
                    }
                    for (int c = 0; c < SPAN; c++) {
                        TS_CHECK((size_t)tl * GHR_TS_PITCH + c < tile.size());
                        tile[(size_t)tl * GHR_TS_PITCH + c] = acc[c];
                    }
                }
            }
            for (int wave = 0; wave < WAVES; wave++)
                for (int lane = 0; lane < TWV; lane++) {
                    const long long q = q0 + lane;
                    if (q >= TT) continue;
                    for (int cc = wave; cc < SPAN && c0 + cc < C; cc += WAVES) {
                        TS_CHECK((size_t)(c0 + cc) * TT + q < (size_t)C * TT);
                        d_texture[(size_t)(c0 + cc) * TT + q] = tile[(size_t)lane * GHR_TS_PITCH + cc];
                    }
                }
        }
    }
}

// k_ts_world
void ghrsim_ts_world(int Smax, int S, int n, const float* v, const float* frames, const float* origins, const int64_t* idx,
                     float inv_scale, float* p, float* p_local)
{
    for (int s = 0; s < S; s++) {
        const long long r = idx[s];
        TS_CHECK(r >= 0 && r < Smax);
        const float* M = frames + (size_t)r * 9;
        const float* org = origins + (size_t)r * 3;
        const float* vs = v + (size_t)s * n * 3;
        float* ps = p + (size_t)s * (n + 1) * 3;
        float* ls = p_local ? p_local + (size_t)s * (n + 1) * 3 : nullptr;
        float run[3][TWV];
        int lo[TWV], hi[TWV];
        for (int l = 0; l < TWV; l++) {
            ghr::sds_chunk(n, l, &lo[l], &hi[l]);
            TS_CHECK(0 <= lo[l] && lo[l] <= hi[l] && hi[l] <= n && (l == 0 ? lo[l] == 0 : lo[l] == hi[l - 1]));
            for (int c = 0; c < 3; c++) run[c][l] = 0.f;
            for (int i = lo[l]; i < hi[l]; i++)
                for (int c = 0; c < 3; c++) run[c][l] += vs[i * 3 + c];
        }
        TS_CHECK(hi[TWV - 1] == n);
        for (int c = 0; c < 3; c++) ts_wave_excl(run[c], +1);
        for (int c = 0; c < 3; c++) { ps[c] = org[c]; if (ls) ls[c] = 0.f; }
        for (int l = 0; l < TWV; l++) {
            float rr[3] = {run[0][l], run[1][l], run[2][l]};
            for (int i = lo[l]; i < hi[l]; i++) {
                float a[3], w[3];
                for (int c = 0; c < 3; c++) rr[c] += vs[i * 3 + c];
                ghr::ts_point(M, org, rr, inv_scale, a, w);
                for (int c = 0; c < 3; c++) { ps[(i + 1) * 3 + c] = w[c]; if (ls) ls[(i + 1) * 3 + c] = a[c]; }
            }
        }
    }
}

// k_ts_world_bwd
void ghrsim_ts_world_backward(int Smax, int S, int n, const float* frames, const int64_t* idx, float inv_scale, const float* d_p,
                              const float* d_pl, float* d_v)
{
    TS_CHECK(d_p || d_pl);
    for (int s = 0; s < S; s++) {
        const long long r = idx[s];
        TS_CHECK(r >= 0 && r < Smax);
        const float* M = frames + (size_t)r * 9;
        const float* dp = d_p ? d_p + (size_t)s * (n + 1) * 3 : nullptr;
        const float* dl = d_pl ? d_pl + (size_t)s * (n + 1) * 3 : nullptr;
        float* dv = d_v + (size_t)s * n * 3;
        float rp[3][TWV], rl[3][TWV];
        int lo[TWV], hi[TWV];
        for (int l = 0; l < TWV; l++) {
            ghr::sds_chunk(n, l, &lo[l], &hi[l]);
            for (int c = 0; c < 3; c++) rp[c][l] = rl[c][l] = 0.f;
            for (int i = hi[l] - 1; i >= lo[l]; i--)
                for (int c = 0; c < 3; c++) {
                    if (dp) rp[c][l] += dp[(i + 1) * 3 + c];
                    if (dl) rl[c][l] += dl[(i + 1) * 3 + c];
                }
        }
        for (int c = 0; c < 3; c++) {
            if (dp) ts_wave_excl(rp[c], -1);
            if (dl) ts_wave_excl(rl[c], -1);
        }
        for (int l = 0; l < TWV; l++) {
            float a[3] = {rp[0][l], rp[1][l], rp[2][l]}, b[3] = {rl[0][l], rl[1][l], rl[2][l]};
            for (int i = hi[l] - 1; i >= lo[l]; i--) {
                float o[3];
                for (int c = 0; c < 3; c++) {
                    if (dp) a[c] += dp[(i + 1) * 3 + c];
                    if (dl) b[c] += dl[(i + 1) * 3 + c];
                }
                ghr::ts_point_vjp(M, a, b, inv_scale, o);
                for (int c = 0; c < 3; c++) dv[i * 3 + c] = o[c];
            }
        }
    }
}

}  // extern "C"
