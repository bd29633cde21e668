// ghr_hostsim_strandview.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Compiles gaussianhaircut_amd/csrc/ghr_strandview.h as plain C++ for the host: the per-element functions the kernels call
// (projection, segment setup, coverage and inverse depth, the winner's order, the head test, the face depth, the shader, the
// resolve) and a host walk of the same tables in the same workspace layout -- counts, scan, scatter, the big list, one tile after
// the other.  Every index the walk forms is checked (GHR_SV_CHECK aborts with the expression), and no tile may meet a segment
// twice.  tests/test_strand_view_cpu.py loads this as a shared library; ghr_strandview_selfcheck.cpp includes it and adds a main().
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define GHR_SV_CHECK(cond)                                                                       \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            std::fprintf(stderr, "ghr_hostsim_strandview.cpp:%d: check failed: %s\n", __LINE__, #cond); \
            std::abort();                                                                        \
        }                                                                                        \
    } while (0)
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
    // the workspace, exact to the byte and 16-B aligned, poisoned: what is not written is not read
    struct alignas(16) Unit { unsigned char b[16]; };
    GHR_SV_CHECK(Y.bytes % 16 == 0);
    std::vector<Unit> storage((size_t)Y.bytes / 16);
    char* ws = reinterpret_cast<char*>(storage.data());
    std::memset(ws, 0xA5, (size_t)Y.bytes);
    GHR_SV_CHECK(Y.off_fill + Y.fill_bytes <= Y.bytes && Y.off_big + 4 * Y.n_segments <= Y.bytes);
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
    if ((long long)H * W == 0) return 0;
    // k_sv_project
    for (uint32_t v = 0; v < N; v++) ghr::vis_project_one(M, points + 3 * (size_t)v, near_w, proj + 4 * (size_t)v);
    // k_sv_setup
    for (uint32_t k = 0; k < K; k++) {
        const uint32_t s = k / (uint32_t)(Lp - 1), i = k % (uint32_t)(Lp - 1);
        const size_t p = (size_t)s * Lp + i;
        GHR_SV_CHECK(p + 1 < N);
        float* rc = rec + (size_t)GHR_SV_REC_WORDS * k;
        ghr::sv_setup_one(proj + 4 * p, proj + 4 * (p + 1), r, H, W, rc);
        uint32_t xy, bits;
        std::memcpy(&xy, rc + 6, 4); std::memcpy(&bits, rc + 7, 4);
        if (bits & GHR_SV_EMPTY) continue;
        if (bits & GHR_SV_BIG) {
            GHR_SV_CHECK(*nbig < K);
            big[(*nbig)++] = k;
            continue;
        }
        const uint32_t x0 = xy & 0xffffu, y0 = xy >> 16, nx = (bits >> 8) & 0xffu, ny = (bits >> 16) & 0xffu;
        GHR_SV_CHECK(x0 + nx < tx && y0 + ny < ty && (nx + 1u) * (ny + 1u) <= GHR_SV_BIG_RECT);
        for (uint32_t y = y0; y <= y0 + ny; y++)
            for (uint32_t x = x0; x <= x0 + nx; x++) count[y * tx + x]++;
    }
    // k_sv_scan
    uint32_t run = 0;
    for (uint32_t t = 0; t < T; t++) { const uint32_t n = count[t]; start[t] = run; count[t] = run; run += n; }
    start[T] = run;
    GHR_SV_CHECK((uint64_t)run <= Y.list_cap);
    // k_sv_scatter
    for (uint32_t k = 0; k < K; k++) {
        const float* rc = rec + (size_t)GHR_SV_REC_WORDS * k;
        uint32_t xy, bits;
        std::memcpy(&xy, rc + 6, 4); std::memcpy(&bits, rc + 7, 4);
        if (bits & (GHR_SV_EMPTY | GHR_SV_BIG)) continue;
        const uint32_t x0 = xy & 0xffffu, y0 = xy >> 16, nx = (bits >> 8) & 0xffu, ny = (bits >> 16) & 0xffu;
        for (uint32_t y = y0; y <= y0 + ny; y++)
            for (uint32_t x = x0; x <= x0 + nx; x++) {
                const uint32_t pos = count[y * tx + x]++;
                GHR_SV_CHECK(pos < start[y * tx + x + 1] && pos < Y.list_cap);
                list[pos] = k;
            }
    }
    for (uint32_t t = 0; t < T; t++) GHR_SV_CHECK(count[t] == start[t + 1]);
    if (n_big) *n_big = *nbig;
    // k_sv_raster, tile by tile; the walk goes BACKWARDS through a tile's entries: the order is free
    std::vector<uint32_t> met(K, 0xffffffffu);  // the last tile that walked each segment
    for (uint32_t tile = 0; tile < T; tile++) {
        const uint32_t beg = start[tile], n_own = start[tile + 1] - beg, n = n_own + *nbig;
        if (tile_len) tile_len[tile] = n;
        for (uint32_t e = 0; e < n; e++) {
            GHR_SV_CHECK(e < n_own ? beg + e < Y.list_cap : e - n_own < K);
            const uint32_t id = e < n_own ? list[beg + e] : big[e - n_own];
            GHR_SV_CHECK(id < K && met[id] != tile);  // in no tile twice
            met[id] = tile;
        }
        for (int li = 0; li < GHR_SV_TILE; li++)
            for (int lj = 0; lj < GHR_SV_TILE; lj++) {
                const int i = (int)(tile / tx) * GHR_SV_TILE + li, j = (int)(tile % tx) * GHR_SV_TILE + lj;
                if (i >= H || j >= W) continue;
                const float px = (float)j + 0.5f, py = (float)i + 0.5f;
                float best_q = 0.f, best_t = 0.f;
                int32_t best_k = -1;
                for (uint32_t e = n; e-- > 0;) {
                    const uint32_t id = e < n_own ? list[beg + e] : big[e - n_own];
                    const float* rc = rec + (size_t)GHR_SV_REC_WORDS * id;
                    float t, q;
                    if (ghr::sv_covers(rc, r, px, py, &t, &q)) ghr::sv_take(q, t, (int32_t)id, &best_q, &best_t, &best_k);
                }
                const size_t o = (size_t)i * W + j;
                ghr::sv_resolve_head(best_k, best_t, best_q, pix_to_face ? pix_to_face[o] : -1, pix_to_face ? qf[o] : 0.f, head_bias,
                                     pix_to_segment + o, t_out + o, pix_to_face_out + o, inv_depth + o);
            }
    }
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
