// ghr_hostsim_visibility.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Compiles gaussianhaircut_amd/csrc/ghr_visibility.h as plain C++ for the host: the per-element functions the kernels call
// (face setup, coverage and inverse depth, the winner's order, the head-mask rule) over the checked host walk of the tile lists
// (ghr_hostsim_tilelists.h: every index checked, no face twice in a tile); the indices this file forms itself are checked the same
// way (GHR_TL_CHECK aborts with the expression).  tests/test_visibility_cpu.py loads this as a shared library;
// ghr_visibility_selfcheck.cpp includes it and adds a main().
#include "ghr_hostsim_tilelists.h"
#include "../../gaussianhaircut_amd/csrc/ghr_visibility.h"

extern "C" {

int ghrsim_vis_chunk(void) { return GHR_VIS_CHUNK; }
int ghrsim_vis_big_rect(void) { return GHR_VIS_BIG_RECT; }

// 0, or -1 with the reason in why[128]
int ghrsim_vis_sizes(long long V, long long F, long long H, long long W, unsigned long long* bytes, char* why)
{
    ghr::VisLayout L;
    const char* w = ghr::vis_layout(V, F, H, W, &L);
    if (w) std::snprintf(why, 128, "%s", w);
    else *bytes = L.bytes;
    return w ? -1 : 0;
}

// k_vis_head_mask, pixel by pixel
void ghrsim_vis_head_mask(int H, int W, const uint8_t* body, const uint8_t* hair, uint8_t* head)
{
    for (int i = 0; i < H; i++)
        for (int j = 0; j < W; j++) head[(size_t)i * W + j] = ghr::vis_head_one(body, hair, H, W, i, j) ? 1 : 0;
}

// ghr_vis_view on the host.  body / hair may be NULL together; tile_len [T] (may be NULL) gets the entries every tile walks
// (its own list and the big list).  cnt / cnt_head are added to.  Returns 0, or -1 when the layout refuses the sizes.
int ghrsim_vis_view(int V, const float* vertices, int F, const int32_t* faces, const float* M, float near_w, int H, int W,
                    const uint8_t* body, const uint8_t* hair, int32_t* pix_to_face, uint8_t* vis, int32_t* cnt, int32_t* cnt_head,
                    uint32_t* tile_len)
{
    ghr::VisLayout L;
    if (ghr::vis_layout(V, F, H, W, &L)) return -1;
    ghrsim::TileListsHost<GHR_VIS_REC_UNITS> tl(L, L.bytes, L.fill_bytes, V, F);
    GHR_TL_CHECK(L.off_fill + L.fill_bytes <= L.off_head && L.off_head + (uint64_t)H * W <= L.bytes);
    GHR_TL_CHECK(L.off_seen + V <= L.off_seen_head && L.off_seen_head + V <= L.off_fill + L.fill_bytes);
    uint8_t* seen = reinterpret_cast<uint8_t*>(tl.ws + L.off_seen);
    uint8_t* seen_head = reinterpret_cast<uint8_t*>(tl.ws + L.off_seen_head);
    uint8_t* head = reinterpret_cast<uint8_t*>(tl.ws + L.off_head);
    if ((long long)H * W == 0) return 0;
    // k_vis_setup
    tl.build(vertices, M, near_w, GHR_VIS_BIG_RECT, [&](uint32_t f, float* r) { ghr::vis_setup_one(tl.proj, V, faces + 3 * (size_t)f, H, W, r); });
    // k_vis_head_mask
    if (body) ghrsim_vis_head_mask(H, W, body, hair, head);
    // k_vis_raster, tile by tile; the walk goes BACKWARDS through a tile's entries: the order is free
    tl.for_each_tile([&](uint32_t tile, const std::vector<uint32_t>& ids) {
        if (tile_len) tile_len[tile] = (uint32_t)ids.size();
        for (int li = 0; li < GHR_VIS_TILE; li++)
            for (int lj = 0; lj < GHR_VIS_TILE; lj++) {
                const int i = (int)(tile / tl.tx) * GHR_VIS_TILE + li, j = (int)(tile % tl.tx) * GHR_VIS_TILE + lj;
                if (i >= H || j >= W) continue;
                const float px = (float)j + 0.5f, py = (float)i + 0.5f;
                float best_d = -INFINITY;
                int32_t best_f = -1;
                for (size_t e = ids.size(); e-- > 0;) {
                    const float* r = tl.record(ids[e]);
                    float d;
                    if (ghr::vis_in_box(r, px, py) && ghr::vis_covers(r, px, py, &d)) ghr::vis_take(d, (int32_t)ids[e], &best_d, &best_f);
                }
                const size_t o = (size_t)i * W + j;
                const bool hd = body && head[o];
                pix_to_face[o] = best_f;
                if (vis) vis[o] = (best_f >= 0 && hd) ? 255 : 0;
                if (best_f >= 0)
                    for (int k = 0; k < 3; k++) {
                        const int32_t v = faces[3 * (size_t)best_f + k];
                        GHR_TL_CHECK(v >= 0 && v < V);
                        seen[v] = 1;
                        if (hd) seen_head[v] = 1;
                    }
            }
    });
    // k_vis_accumulate
    if (cnt && cnt_head)
        for (int v = 0; v < V; v++) {
            GHR_TL_CHECK(seen[v] <= 1 && seen_head[v] <= seen[v]);
            cnt[v] += seen[v];
            cnt_head[v] += seen_head[v];
        }
    return 0;
}

}  // extern "C"
