// ghr_hostsim_strandshadow.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Compiles the self-shadowing part of gaussianhaircut_amd/csrc/ghr_strandview.h as plain C++ for the host: the per-element functions
// the kernels call (sv_layer_of, sv_occluders, sv_transmittance, sv_shadow_at, sv_shade_one_shadowed) and a host walk of the light
// pass in the product's workspace layout -- counts, scan, scatter, the big list, then k_sv_layers' TWO walks of every tile's
// entries: the front plane, then the four counts behind it.  Every index the walk forms is checked (GHR_SS_CHECK aborts with the
// expression), and no tile may meet a segment twice.  tests/test_strand_shadow_cpu.py loads this as a shared library;
// ghr_strandshadow_selfcheck.cpp includes it and adds a main().
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define GHR_SS_CHECK(cond)                                                                         \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            std::fprintf(stderr, "ghr_hostsim_strandshadow.cpp:%d: check failed: %s\n", __LINE__, #cond); \
            std::abort();                                                                          \
        }                                                                                          \
    } while (0)
#include "../../gaussianhaircut_amd/csrc/ghr_strandview.h"

extern "C" {

int ghrsim_ss_chunk(void) { return GHR_SV_CHUNK; }
int ghrsim_ss_shadow_bytes(void) { return (int)sizeof(ghr::SvShadow); }

// ghr_strandview_opacity on the host.  tile_len [T] (may be NULL) gets the entries every tile walks (its own list and the big list);
// n_big (may be NULL) the length of the big list.  Returns 0, or -1 when the layout refuses the sizes.
int ghrsim_ss_opacity(int S, int Lp, const float* points, const float* Ml, float near_w, int Hl, int Wl, float rl, float layer,
                      float* q0, uint32_t* layers, uint32_t* tile_len, uint32_t* n_big)
{
    ghr::SvLayout Y;
    if (ghr::sv_layout(S, Lp, Hl, Wl, &Y)) return -1;
    struct alignas(16) Unit { unsigned char b[16]; };
    GHR_SS_CHECK(Y.bytes % 16 == 0);
    std::vector<Unit> storage((size_t)Y.bytes / 16);
    char* ws = reinterpret_cast<char*>(storage.data());
    std::memset(ws, 0xA5, (size_t)Y.bytes);  // what is not written is not read
    GHR_SS_CHECK(Y.off_fill + Y.fill_bytes <= Y.bytes && Y.off_big + 4 * Y.n_segments <= Y.bytes);
    std::memset(ws + Y.off_fill, 0, (size_t)Y.fill_bytes);
    float* proj = reinterpret_cast<float*>(ws + Y.off_proj);
    float* rec = reinterpret_cast<float*>(ws + Y.off_rec);
    uint32_t* start = reinterpret_cast<uint32_t*>(ws + Y.off_start);
    uint32_t* count = reinterpret_cast<uint32_t*>(ws + Y.off_count);
    uint32_t* nbig = reinterpret_cast<uint32_t*>(ws + Y.off_nbig);
    uint32_t* list = reinterpret_cast<uint32_t*>(ws + Y.off_list);
    uint32_t* big = reinterpret_cast<uint32_t*>(ws + Y.off_big);
    const uint32_t tx = (uint32_t)Y.tiles_x, ty = (uint32_t)Y.tiles_y, T = tx * ty;
    const uint32_t N = (uint32_t)Y.n_points, K = (uint32_t)Y.n_segments;
    if (n_big) *n_big = 0;
    if ((long long)Hl * Wl == 0) return 0;
    for (uint32_t v = 0; v < N; v++) ghr::vis_project_one(Ml, points + 3 * (size_t)v, near_w, proj + 4 * (size_t)v);  // k_sv_project
    for (uint32_t k = 0; k < K; k++) {                                                                              // k_sv_setup
        const uint32_t s = k / (uint32_t)(Lp - 1), i = k % (uint32_t)(Lp - 1);
        const size_t p = (size_t)s * Lp + i;
        GHR_SS_CHECK(p + 1 < N);
        float* rc = rec + (size_t)GHR_SV_REC_WORDS * k;
        ghr::sv_setup_one(proj + 4 * p, proj + 4 * (p + 1), rl, Hl, Wl, rc);
        uint32_t xy, bits;
        std::memcpy(&xy, rc + 6, 4); std::memcpy(&bits, rc + 7, 4);
        if (bits & GHR_SV_EMPTY) continue;
        if (bits & GHR_SV_BIG) {
            GHR_SS_CHECK(*nbig < K);
            big[(*nbig)++] = k;
            continue;
        }
        const uint32_t x0 = xy & 0xffffu, y0 = xy >> 16, nx = (bits >> 8) & 0xffu, ny = (bits >> 16) & 0xffu;
        GHR_SS_CHECK(x0 + nx < tx && y0 + ny < ty && (nx + 1u) * (ny + 1u) <= GHR_SV_BIG_RECT);
        for (uint32_t y = y0; y <= y0 + ny; y++)
            for (uint32_t x = x0; x <= x0 + nx; x++) count[y * tx + x]++;
    }
    uint32_t run = 0;                                                                                               // k_sv_scan
    for (uint32_t t = 0; t < T; t++) { const uint32_t n = count[t]; start[t] = run; count[t] = run; run += n; }
    start[T] = run;
    GHR_SS_CHECK((uint64_t)run <= Y.list_cap);
    for (uint32_t k = 0; k < K; k++) {                                                                              // k_sv_scatter
        const float* rc = rec + (size_t)GHR_SV_REC_WORDS * k;
        uint32_t xy, bits;
        std::memcpy(&xy, rc + 6, 4); std::memcpy(&bits, rc + 7, 4);
        if (bits & (GHR_SV_EMPTY | GHR_SV_BIG)) continue;
        const uint32_t x0 = xy & 0xffffu, y0 = xy >> 16, nx = (bits >> 8) & 0xffu, ny = (bits >> 16) & 0xffu;
        for (uint32_t y = y0; y <= y0 + ny; y++)
            for (uint32_t x = x0; x <= x0 + nx; x++) {
                const uint32_t pos = count[y * tx + x]++;
                GHR_SS_CHECK(pos < start[y * tx + x + 1] && pos < Y.list_cap);
                list[pos] = k;
            }
    }
    for (uint32_t t = 0; t < T; t++) GHR_SS_CHECK(count[t] == start[t + 1]);
    if (n_big) *n_big = *nbig;
    // k_sv_layers, tile by tile.  Walk 1 goes forwards through a tile's entries and walk 2 BACKWARDS: the order is free.
    std::vector<uint32_t> met(K, 0xffffffffu);  // the last tile that walked each segment
    for (uint32_t tile = 0; tile < T; tile++) {
        const uint32_t beg = start[tile], n_own = start[tile + 1] - beg, n = n_own + *nbig;
        if (tile_len) tile_len[tile] = n;
        for (uint32_t e = 0; e < n; e++) {
            GHR_SS_CHECK(e < n_own ? beg + e < Y.list_cap : e - n_own < K);
            const uint32_t id = e < n_own ? list[beg + e] : big[e - n_own];
            GHR_SS_CHECK(id < K && met[id] != tile);  // in no tile twice: a segment counted twice would be a wrong count
            met[id] = tile;
        }
        for (int li = 0; li < GHR_SV_TILE; li++)
            for (int lj = 0; lj < GHR_SV_TILE; lj++) {
                const int i = (int)(tile / tx) * GHR_SV_TILE + li, j = (int)(tile % tx) * GHR_SV_TILE + lj;
                if (i >= Hl || j >= Wl) continue;
                const float px = (float)j + 0.5f, py = (float)i + 0.5f;
                float best_q = 0.f, t, q;
                for (uint32_t e = 0; e < n; e++) {
                    const uint32_t id = e < n_own ? list[beg + e] : big[e - n_own];
                    if (ghr::sv_covers(rec + (size_t)GHR_SV_REC_WORDS * id, rl, px, py, &t, &q) && q > best_q) best_q = q;
                }
                uint32_t c[4] = {0u, 0u, 0u, 0u};
                const float inv_q0 = 1.f / best_q;
                for (uint32_t e = n; e-- > 0;) {
                    const uint32_t id = e < n_own ? list[beg + e] : big[e - n_own];
                    if (ghr::sv_covers(rec + (size_t)GHR_SV_REC_WORDS * id, rl, px, py, &t, &q) && q > 0.f) {
                        const int layer_k = ghr::sv_layer_of(1.f / q - inv_q0, layer);
                        GHR_SS_CHECK(layer_k >= 0 && layer_k < 4);
                        c[layer_k]++;
                    }
                }
                const size_t o = (size_t)i * Wl + j;
                q0[o] = best_q;
                for (int k = 0; k < 4; k++) layers[4 * o + k] = c[k];
            }
    }
    return 0;
}

static ghr::SvShadow ss_shadow(const float* Ml, float near_w, int Hl, int Wl, float layer, float kappa, float bias, const float* q0,
                               const uint32_t* layers, const float* qfl)
{
    ghr::SvShadow sd;
    std::memcpy(sd.Ml, Ml, sizeof(sd.Ml));
    sd.near_w = near_w; sd.Hl = Hl; sd.Wl = Wl; sd.layer = layer; sd.kappa = kappa; sd.bias = bias;
    sd.q0 = q0; sd.layers = layers; sd.qfl = qfl;
    return sd;
}

// the lookup of `count` world points P [count][3]: the occluders in front of each and its transmittance
void ghrsim_ss_lookup(int count, const float* P, const float* Ml, float near_w, int Hl, int Wl, float layer, float kappa, float bias,
                      const float* q0, const uint32_t* layers, const float* qfl, float* n_out, float* tr_out)
{
    const ghr::SvShadow sd = ss_shadow(Ml, near_w, Hl, Wl, layer, kappa, bias, q0, layers, qfl);
    for (int k = 0; k < count; k++) tr_out[k] = ghr::sv_shadow_at(sd, P + 3 * (size_t)k, n_out + k);
}

// k_sv_shade_shadowed, pixel by pixel; sh: a ghr::SvShading
void ghrsim_ss_shade(int S, int Lp, const float* points, int V, const float* vertices, int F, const int32_t* faces, int H, int W,
                     const int32_t* pix_to_segment, const int32_t* pix_to_face_out, const float* t, int mode, const void* sh,
                     const float* base, const float* Ml, float near_w, int Hl, int Wl, float layer, float kappa, float bias,
                     const float* q0, const uint32_t* layers, const float* qfl, uint8_t* rgb)
{
    ghr::SvShading s;
    std::memcpy(&s, sh, sizeof(s));
    const ghr::SvShadow sd = ss_shadow(Ml, near_w, Hl, Wl, layer, kappa, bias, q0, layers, qfl);
    for (size_t o = 0; o < (size_t)H * W; o++)
        ghr::sv_shade_one_shadowed(pix_to_segment[o], pix_to_face_out[o], t[o], S, Lp, points, V, vertices, F, faces, base, mode, s, sd,
                                   rgb + 3 * o);
}

}  // extern "C"
