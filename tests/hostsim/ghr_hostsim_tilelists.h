// ghr_hostsim_tilelists.h -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// The host walk of gaussianhaircut_amd/csrc/ghr_tilelists.h that the visibility, strand-view and strand-shadow simulators share:
// one view's lists built in the product's layout -- projection, the owner's records, counts, scan, scatter, the big list -- inside a
// poisoned workspace that is exact to the byte and 16-B aligned, then every tile's entries handed to the simulator.  Every index
// the walk forms is checked (GHR_TL_CHECK aborts with the expression), and no tile may meet a primitive twice.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define GHR_TL_CHECK(cond)                                                                   \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond);    \
            std::abort();                                                                    \
        }                                                                                    \
    } while (0)
#include "../../gaussianhaircut_amd/csrc/ghr_tilelists.h"

namespace ghrsim {

template <int UNITS>
struct TileListsHost {
    struct alignas(16) Unit { unsigned char b[16]; };
    std::vector<Unit> storage;  // (new[] of a 16-B type: aligned)
    const ghr::TileListLayout L;
    const uint32_t n_points, n_prims, tx, ty, T;
    char* ws;
    float *proj, *rec;
    uint32_t *start, *count, *nbig, *list, *big;

    // A workspace of `bytes`, poisoned (what is not written is not read), with [L.off_fill, + fill_bytes) zeroed as a view does first.
    TileListsHost(const ghr::TileListLayout& layout, uint64_t bytes, uint64_t fill_bytes, uint64_t points, uint64_t prims)
        : L(layout), n_points((uint32_t)points), n_prims((uint32_t)prims), tx((uint32_t)layout.tiles_x), ty((uint32_t)layout.tiles_y), T(tx * ty)
    {
        GHR_TL_CHECK(bytes % 16 == 0);
        storage.resize((size_t)bytes / 16);
        ws = reinterpret_cast<char*>(storage.data());
        std::memset(ws, 0xA5, (size_t)bytes);
        GHR_TL_CHECK(L.off_proj + 16ull * n_points <= L.off_rec && L.off_rec + 16ull * UNITS * n_prims <= L.off_start);
        GHR_TL_CHECK(L.off_start + 4ull * (T + 1) <= L.off_list && L.off_list + 4 * L.list_cap <= L.off_big);
        GHR_TL_CHECK(L.off_big + 4ull * n_prims <= L.off_count && L.off_count + 4ull * T <= L.off_nbig);
        GHR_TL_CHECK(L.off_fill == L.off_count && L.off_nbig + 4 <= L.off_fill + fill_bytes && L.off_fill + fill_bytes <= bytes);
        std::memset(ws + L.off_fill, 0, (size_t)fill_bytes);
        proj = reinterpret_cast<float*>(ws + L.off_proj);
        rec = reinterpret_cast<float*>(ws + L.off_rec);
        start = reinterpret_cast<uint32_t*>(ws + L.off_start);
        count = reinterpret_cast<uint32_t*>(ws + L.off_count);
        nbig = reinterpret_cast<uint32_t*>(ws + L.off_nbig);
        list = reinterpret_cast<uint32_t*>(ws + L.off_list);
        big = reinterpret_cast<uint32_t*>(ws + L.off_big);
    }

    const float* record(uint32_t id) const { return rec + (size_t)(4 * UNITS) * id; }

    // k_tl_project, the owner's setup (setup(id, record): the record from proj), tl_count, k_tl_scan, k_tl_scatter
    template <class Setup>
    void build(const float* points, const float* M, float near_w, uint32_t big_rect, Setup setup)
    {
        for (uint32_t v = 0; v < n_points; v++) ghr::vis_project_one(M, points + 3 * (size_t)v, near_w, proj + 4 * (size_t)v);
        for (uint32_t id = 0; id < n_prims; id++) {
            float* r = rec + (size_t)(4 * UNITS) * id;
            setup(id, r);
            uint32_t xy, bits, x0, x1, y0, y1;
            std::memcpy(&xy, r + 4 * UNITS - 2, 4); std::memcpy(&bits, r + 4 * UNITS - 1, 4);
            if (bits & GHR_TL_EMPTY) continue;
            ghr::tl_rect_tiles(xy, bits, &x0, &x1, &y0, &y1);
            GHR_TL_CHECK(x0 <= x1 && x1 < tx && y0 <= y1 && y1 < ty);
            if (bits & GHR_TL_BIG) {
                GHR_TL_CHECK(*nbig < n_prims);
                big[(*nbig)++] = id;
                continue;
            }
            GHR_TL_CHECK((x1 - x0 + 1u) * (y1 - y0 + 1u) <= big_rect);
            for (uint32_t y = y0; y <= y1; y++)
                for (uint32_t x = x0; x <= x1; x++) count[y * tx + x]++;
        }
        uint32_t run = 0;
        for (uint32_t t = 0; t < T; t++) { const uint32_t n = count[t]; start[t] = run; count[t] = run; run += n; }
        start[T] = run;
        GHR_TL_CHECK((uint64_t)run <= L.list_cap);
        for (uint32_t id = 0; id < n_prims; id++) {
            const float* r = record(id);
            uint32_t xy, bits, x0, x1, y0, y1;
            std::memcpy(&xy, r + 4 * UNITS - 2, 4); std::memcpy(&bits, r + 4 * UNITS - 1, 4);
            if (bits & (GHR_TL_EMPTY | GHR_TL_BIG)) continue;
            ghr::tl_rect_tiles(xy, bits, &x0, &x1, &y0, &y1);
            for (uint32_t y = y0; y <= y1; y++)
                for (uint32_t x = x0; x <= x1; x++) {
                    const uint32_t pos = count[y * tx + x]++;
                    GHR_TL_CHECK(pos < start[y * tx + x + 1] && pos < L.list_cap);
                    list[pos] = id;
                }
        }
        for (uint32_t t = 0; t < T; t++) GHR_TL_CHECK(count[t] == start[t + 1]);
    }

    // visit(tile, ids): the entries a tile walks, its own list and then the big list.  The order inside is free: a simulator shows
    // it by walking them in another one.
    template <class Visit>
    void for_each_tile(Visit visit) const
    {
        std::vector<uint32_t> met(n_prims, 0xffffffffu), ids;  // met: the last tile that walked each primitive
        for (uint32_t tile = 0; tile < T; tile++) {
            const uint32_t beg = start[tile], n_own = start[tile + 1] - beg, n = n_own + *nbig;
            ids.resize(n);
            for (uint32_t e = 0; e < n; e++) {
                GHR_TL_CHECK(e < n_own ? beg + e < L.list_cap : e - n_own < n_prims);
                const uint32_t id = e < n_own ? list[beg + e] : big[e - n_own];
                GHR_TL_CHECK(id < n_prims && met[id] != tile);  // in no tile twice
                met[id] = tile;
                ids[e] = id;
            }
            visit(tile, ids);
        }
    }
};

}  // namespace ghrsim
