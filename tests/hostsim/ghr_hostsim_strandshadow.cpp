// ghr_hostsim_strandshadow.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Compiles the self-shadowing part of gaussianhaircut_amd/csrc/ghr_strandview.h as plain C++ for the host: the per-element functions
// the kernels call (sv_layer_of, sv_occluders, sv_transmittance, sv_shadow_at, sv_shade_one_shadowed) and the light pass over the
// checked host walk of the tile lists (ghr_hostsim_tilelists.h: every index checked, no segment twice in a tile -- a segment
// counted twice would be a wrong count), with k_sv_layers' TWO walks of every tile's entries: the front plane, then the four counts
// behind it.  tests/test_strand_shadow_cpu.py loads this as a shared library; ghr_strandshadow_selfcheck.cpp includes it and adds
// a main().
#include "ghr_hostsim_tilelists.h"
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
    ghrsim::TileListsHost<GHR_SV_REC_UNITS> tl(Y, Y.bytes, Y.fill_bytes, Y.n_points, Y.n_segments);
    if (n_big) *n_big = 0;
    if ((long long)Hl * Wl == 0) return 0;
    // k_sv_setup
    tl.build(points, Ml, near_w, GHR_SV_BIG_RECT, [&](uint32_t k, float* rc) {
        const size_t p = (size_t)(k / (uint32_t)(Lp - 1)) * Lp + k % (uint32_t)(Lp - 1);
        GHR_TL_CHECK(p + 1 < tl.n_points);
        ghr::sv_setup_one(tl.proj + 4 * p, tl.proj + 4 * (p + 1), rl, Hl, Wl, rc);
    });
    if (n_big) *n_big = *tl.nbig;
    // k_sv_layers, tile by tile.  Walk 1 goes forwards through a tile's entries and walk 2 BACKWARDS: the order is free.
    tl.for_each_tile([&](uint32_t tile, const std::vector<uint32_t>& ids) {
        if (tile_len) tile_len[tile] = (uint32_t)ids.size();
        for (int li = 0; li < GHR_SV_TILE; li++)
            for (int lj = 0; lj < GHR_SV_TILE; lj++) {
                const int i = (int)(tile / tl.tx) * GHR_SV_TILE + li, j = (int)(tile % tl.tx) * GHR_SV_TILE + lj;
                if (i >= Hl || j >= Wl) continue;
                const float px = (float)j + 0.5f, py = (float)i + 0.5f;
                float best_q = 0.f, t, q;
                for (size_t e = 0; e < ids.size(); e++)
                    if (ghr::sv_covers(tl.record(ids[e]), rl, px, py, &t, &q) && q > best_q) best_q = q;
                uint32_t c[4] = {0u, 0u, 0u, 0u};
                const float inv_q0 = 1.f / best_q;
                for (size_t e = ids.size(); e-- > 0;) {
                    if (ghr::sv_covers(tl.record(ids[e]), rl, px, py, &t, &q) && q > 0.f) {
                        const int layer_k = ghr::sv_layer_of(1.f / q - inv_q0, layer);
                        GHR_TL_CHECK(layer_k >= 0 && layer_k < 4);
                        c[layer_k]++;
                    }
                }
                const size_t o = (size_t)i * Wl + j;
                q0[o] = best_q;
                for (int k = 0; k < 4; k++) layers[4 * o + k] = c[k];
            }
    });
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
