// ghr_hostsim_visibility.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Compiles gaussianhaircut_amd/csrc/ghr_visibility.h as plain C++ for the host: the per-element functions the kernels call
// (projection, face setup, coverage and inverse depth, the winner's order, the head-mask rule) and a host walk of the same
// tables in the same workspace layout -- counts, scan, scatter, the big list, one tile after the other.  Every index the walk
// forms is checked (GHR_VIS_CHECK aborts with the expression).  tests/test_visibility_cpu.py loads this as a shared library;
// ghr_visibility_selfcheck.cpp includes it and adds a main().
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define GHR_VIS_CHECK(cond)                                                                       \
    do {                                                                                          \
        if (!(cond)) {                                                                            \
            std::fprintf(stderr, "ghr_hostsim_visibility.cpp:%d: check failed: %s\n", __LINE__, #cond); \
            std::abort();                                                                         \
        }                                                                                         \
    } while (0)
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
    // the workspace, exact to the byte and 16-B aligned (new[] of a 16-B type), poisoned: what is not written is not read
    struct alignas(16) Unit { unsigned char b[16]; };
    GHR_VIS_CHECK(L.bytes % 16 == 0);
    std::vector<Unit> storage((size_t)L.bytes / 16);
    char* ws = reinterpret_cast<char*>(storage.data());
    std::memset(ws, 0xA5, (size_t)L.bytes);
    GHR_VIS_CHECK(L.off_fill + L.fill_bytes <= L.bytes && L.off_head + (uint64_t)H * W <= L.bytes);
    std::memset(ws + L.off_fill, 0, (size_t)L.fill_bytes);
    float* proj = reinterpret_cast<float*>(ws + L.off_proj);
    float* rec = reinterpret_cast<float*>(ws + L.off_rec);
    uint32_t* start = reinterpret_cast<uint32_t*>(ws + L.off_start);
    uint32_t* count = reinterpret_cast<uint32_t*>(ws + L.off_count);
    uint32_t* nbig = reinterpret_cast<uint32_t*>(ws + L.off_nbig);
    uint32_t* list = reinterpret_cast<uint32_t*>(ws + L.off_list);
    uint32_t* big = reinterpret_cast<uint32_t*>(ws + L.off_big);
    uint8_t* seen = reinterpret_cast<uint8_t*>(ws + L.off_seen);
    uint8_t* seen_head = reinterpret_cast<uint8_t*>(ws + L.off_seen_head);
    uint8_t* head = reinterpret_cast<uint8_t*>(ws + L.off_head);
    const uint32_t tx = (uint32_t)L.tiles_x, ty = (uint32_t)L.tiles_y, T = tx * ty;
    if ((long long)H * W == 0) return 0;
    // k_vis_project
    for (int v = 0; v < V; v++) ghr::vis_project_one(M, vertices + 3 * (size_t)v, near_w, proj + 4 * (size_t)v);
    // k_vis_setup
    for (int f = 0; f < F; f++) {
        float* r = rec + (size_t)GHR_VIS_REC_WORDS * f;
        ghr::vis_setup_one(proj, V, faces + 3 * (size_t)f, H, W, r);
        uint32_t bits, rx, ry;
        std::memcpy(&bits, r + 9, 4); std::memcpy(&rx, r + 10, 4); std::memcpy(&ry, r + 11, 4);
        if (bits & GHR_VIS_EMPTY) continue;
        GHR_VIS_CHECK((rx & 0xffffu) <= (rx >> 16) && (rx >> 16) < tx && (ry & 0xffffu) <= (ry >> 16) && (ry >> 16) < ty);
        if (bits & GHR_VIS_BIG) {
            GHR_VIS_CHECK(*nbig < (uint32_t)F);
            big[(*nbig)++] = (uint32_t)f;
            continue;
        }
        GHR_VIS_CHECK(((rx >> 16) - (rx & 0xffffu) + 1u) * ((ry >> 16) - (ry & 0xffffu) + 1u) <= GHR_VIS_BIG_RECT);
        for (uint32_t y = ry & 0xffffu; y <= (ry >> 16); y++)
            for (uint32_t x = rx & 0xffffu; x <= (rx >> 16); x++) count[y * tx + x]++;
    }
    // k_vis_scan
    uint32_t run = 0;
    for (uint32_t t = 0; t < T; t++) { const uint32_t n = count[t]; start[t] = run; count[t] = run; run += n; }
    start[T] = run;
    GHR_VIS_CHECK((uint64_t)run <= L.list_cap);
    // k_vis_scatter
    for (int f = 0; f < F; f++) {
        const float* r = rec + (size_t)GHR_VIS_REC_WORDS * f;
        uint32_t bits, rx, ry;
        std::memcpy(&bits, r + 9, 4); std::memcpy(&rx, r + 10, 4); std::memcpy(&ry, r + 11, 4);
        if (bits & (GHR_VIS_EMPTY | GHR_VIS_BIG)) continue;
        for (uint32_t y = ry & 0xffffu; y <= (ry >> 16); y++)
            for (uint32_t x = rx & 0xffffu; x <= (rx >> 16); x++) {
                const uint32_t pos = count[y * tx + x]++;
                GHR_VIS_CHECK(pos < start[y * tx + x + 1] && pos < L.list_cap);
                list[pos] = (uint32_t)f;
            }
    }
    for (uint32_t t = 0; t < T; t++) GHR_VIS_CHECK(count[t] == start[t + 1]);
    // k_vis_head_mask
    if (body) ghrsim_vis_head_mask(H, W, body, hair, head);
    // k_vis_raster, tile by tile; the walk goes BACKWARDS through a tile's entries: the order is free
    for (uint32_t tile = 0; tile < T; tile++) {
        const uint32_t beg = start[tile], n_own = start[tile + 1] - beg, n = n_own + *nbig;
        if (tile_len) tile_len[tile] = n;
        for (int li = 0; li < GHR_VIS_TILE; li++)
            for (int lj = 0; lj < GHR_VIS_TILE; lj++) {
                const int i = (int)(tile / tx) * GHR_VIS_TILE + li, j = (int)(tile % tx) * GHR_VIS_TILE + lj;
                if (i >= H || j >= W) continue;
                const float px = (float)j + 0.5f, py = (float)i + 0.5f;
                float best_d = -INFINITY;
                int32_t best_f = -1;
                for (uint32_t e = n; e-- > 0;) {
                    GHR_VIS_CHECK(e < n_own ? beg + e < L.list_cap : e - n_own < (uint32_t)F);
                    const uint32_t id = e < n_own ? list[beg + e] : big[e - n_own];
                    GHR_VIS_CHECK(id < (uint32_t)F);
                    const float* r = rec + (size_t)GHR_VIS_REC_WORDS * id;
                    float d;
                    if (ghr::vis_in_box(r, px, py) && ghr::vis_covers(r, px, py, &d)) ghr::vis_take(d, (int32_t)id, &best_d, &best_f);
                }
                const size_t o = (size_t)i * W + j;
                const bool hd = body && head[o];
                pix_to_face[o] = best_f;
                if (vis) vis[o] = (best_f >= 0 && hd) ? 255 : 0;
                if (best_f >= 0)
                    for (int k = 0; k < 3; k++) {
                        const int32_t v = faces[3 * (size_t)best_f + k];
                        GHR_VIS_CHECK(v >= 0 && v < V);
                        seen[v] = 1;
                        if (hd) seen_head[v] = 1;
                    }
            }
    }
    // k_vis_accumulate
    if (cnt && cnt_head)
        for (int v = 0; v < V; v++) {
            GHR_VIS_CHECK(seen[v] <= 1 && seen_head[v] <= seen[v]);
            cnt[v] += seen[v];
            cnt_head[v] += seen_head[v];
        }
    return 0;
}

}  // extern "C"
