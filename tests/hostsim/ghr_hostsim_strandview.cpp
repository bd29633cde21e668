// ghr_hostsim_strandview.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Compiles gaussianhaircut_amd/csrc/ghr_strandview.h as plain C++ for the host: the per-element functions the kernels call
// (segment setup, coverage and inverse depth, the winner's order, the head test, the face depth, the shader, the resolve) over the
// checked host walk of the tile lists (ghr_hostsim_tilelists.h: every index checked, no segment twice in a tile).
// tests/test_strand_view_cpu.py loads this as a shared library; ghr_strandview_selfcheck.cpp includes it and adds a main().
#include "ghr_hostsim_tilelists.h"
#include "../../gaussianhaircut_amd/csrc/ghr_strandview.h"

extern "C" {

int ghrsim_sv_chunk(void) { return GHR_SV_CHUNK; }
int ghrsim_sv_big_rect(void) { return GHR_SV_BIG_RECT; }
int ghrsim_sv_shading_bytes(void) { return (int)sizeof(ghr::SvShading); }

// k_sv_face_depth, pixel by pixel
void ghrsim_sv_face_depth(int V, const float* vertices, int F, const int32_t* faces, const float* M, float near_w, int H, int W,
                          const int32_t* pix_to_face, float* qf)
{
    for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++)
            qf[(size_t)i * W + j] = ghr::sv_face_depth_one(M, near_w, vertices, V, faces, F, pix_to_face[(size_t)i * W + j],
                                                           (float)j + 0.5f, (float)i + 0.5f);
}

// ghr_strandview_raster on the host.  pix_to_face / qf may be NULL together; tile_len [T] (may be NULL) gets the entries every
// tile walks (its own list and the big list); n_big (may be NULL) the length of the big list.  Returns 0, or -1 when the layout
// refuses the sizes.
int ghrsim_sv_raster(int S, int Lp, const float* points, const float* M, float near_w, int H, int W, float r, float head_bias,
                     const int32_t* pix_to_face, const float* qf, int32_t* pix_to_segment, float* t_out, int32_t* pix_to_face_out,
                     float* inv_depth, uint32_t* tile_len, uint32_t* n_big)
{
    ghr::SvLayout Y;
    if (ghr::sv_layout(S, Lp, H, W, &Y)) return -1;
    ghrsim::TileListsHost<GHR_SV_REC_UNITS> tl(Y, Y.bytes, Y.fill_bytes, Y.n_points, Y.n_segments);
    if (n_big) *n_big = 0;
    if ((long long)H * W == 0) return 0;
    // k_sv_setup
    tl.build(points, M, near_w, GHR_SV_BIG_RECT, [&](uint32_t k, float* rc) {
        const size_t p = (size_t)(k / (uint32_t)(Lp - 1)) * Lp + k % (uint32_t)(Lp - 1);
        GHR_TL_CHECK(p + 1 < tl.n_points);
        ghr::sv_setup_one(tl.proj + 4 * p, tl.proj + 4 * (p + 1), r, H, W, rc);
    });
    if (n_big) *n_big = *tl.nbig;
    // k_sv_raster, tile by tile; the walk goes BACKWARDS through a tile's entries: the order is free
    tl.for_each_tile([&](uint32_t tile, const std::vector<uint32_t>& ids) {
        if (tile_len) tile_len[tile] = (uint32_t)ids.size();
        for (int li = 0; li < GHR_SV_TILE; li++)
            for (int lj = 0; lj < GHR_SV_TILE; lj++) {
                const int i = (int)(tile / tl.tx) * GHR_SV_TILE + li, j = (int)(tile % tl.tx) * GHR_SV_TILE + lj;
                if (i >= H || j >= W) continue;
                const float px = (float)j + 0.5f, py = (float)i + 0.5f;
                float best_q = 0.f, best_t = 0.f;
                int32_t best_k = -1;
                for (size_t e = ids.size(); e-- > 0;) {
                    float t, q;
                    if (ghr::sv_covers(tl.record(ids[e]), r, px, py, &t, &q)) ghr::sv_take(q, t, (int32_t)ids[e], &best_q, &best_t, &best_k);
                }
                const size_t o = (size_t)i * W + j;
                ghr::sv_resolve_head(best_k, best_t, best_q, pix_to_face ? pix_to_face[o] : -1, pix_to_face ? qf[o] : 0.f, head_bias,
                                     pix_to_segment + o, t_out + o, pix_to_face_out + o, inv_depth + o);
            }
    });
    return 0;
}

// k_sv_shade, pixel by pixel; sh: a ghr::SvShading
void ghrsim_sv_shade(int S, int Lp, const float* points, int V, const float* vertices, int F, const int32_t* faces, int H, int W,
                     const int32_t* pix_to_segment, const int32_t* pix_to_face_out, int mode, const void* sh, const float* base,
                     uint8_t* rgb)
{
    ghr::SvShading s;
    std::memcpy(&s, sh, sizeof(s));
    for (size_t o = 0; o < (size_t)H * W; o++)
        ghr::sv_shade_one(pix_to_segment[o], pix_to_face_out[o], S, Lp, points, V, vertices, F, faces, base, mode, s, rgb + 3 * o);
}

// k_sv_resolve
void ghrsim_sv_resolve(int H, int W, int s, const uint8_t* src, uint8_t* dst)
{
    for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++) ghr::sv_resolve_one(src, W, s, i, j, dst);
}

}  // extern "C"
