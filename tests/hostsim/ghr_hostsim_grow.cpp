// ghr_hostsim_grow.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Compiles gaussianhaircut_amd/csrc/ghr_grow.h as plain C++ for the host and walks k_grow_guarded with a 64-lane wave kept in
// arrays: ghr_hostsim_field.cpp's field walk, then a restatement of md_wave_search's loop (seed block, superblocks in rotation,
// blocks, the ballot on every face's own box; every ballot evaluated over the lanes' CURRENT states before the scan it guards), then
// mesh_contains_one per lane -- the headers' own GHR_HD functions throughout (field_strand_heading, MdNearest, md_seed_block,
// knn_key, mesh_contains_one, grow_guard_step).  The mesh comes as the product's two blobs, each with its header at its start.
// Every index is checked (KNN_CHECK aborts with the expression), the tile is poisoned past the staged records, and no wave may scan
// a block twice.  tests/test_grow_guarded_cpu.py loads this as a shared library; ghr_grow_selfcheck.cpp includes it and adds a main().
#include "ghr_hostsim_field.cpp"
#define GHR_MD_CHECK(cond) KNN_CHECK(cond)
#define GHR_MESH_CHECK(cond) KNN_CHECK(cond)
#include "../../gaussianhaircut_amd/csrc/ghr_grow.h"

#define GROW_LOG 29  // floats per (strand, step) of the log, see ghrsim_grow_guarded

namespace {

struct HeadBlobs {
    ghr::MeshTris th;
    ghr::MdView md;
    float bounds[6];
    ghr::MeshGrid gh;
    ghr::MeshView mesh;
    HeadBlobs(const void* tris, const void* grid)
    {
        std::memcpy(&th, tris, sizeof(th));
        KNN_CHECK(th.magic == GHR_MD_MAGIC && th.n_faces >= 1);
        KNN_CHECK(th.n_blocks == (th.n_faces + WV - 1) / WV && th.n_super == (th.n_blocks + GHR_KNN_SUPER - 1) / GHR_KNN_SUPER);
        md = ghr::md_view(th, tris);
        for (int k = 0; k < 3; k++) bounds[k] = th.lo[k], bounds[3 + k] = th.hi[k];
        std::memcpy(&gh, grid, sizeof(gh));
        KNN_CHECK(gh.magic == GHR_MESH_MAGIC && gh.G >= 1 && gh.G <= GHR_MESH_G_MAX && gh.n_faces == th.n_faces);
        mesh = ghr::mesh_view(gh, grid);
    }
};

// md_wave_search for one wave; returns the blocks scanned
unsigned grow_wave_search(const ghr::MdView& m, const ghr::MdVec* q, const bool* valid, int first, ghr::MdNearest* near)
{
    KNN_CHECK(first >= 0 && first < m.n_blocks);
    ghr::float3 q3[WV];
    for (int l = 0; l < WV; l++) q3[l] = ghr::float3{q[l].x, q[l].y, q[l].z};
    std::vector<unsigned char> seen((size_t)m.n_blocks, 0);
    unsigned scanned = 0;
    auto scan_block = [&](int blk) {
        KNN_CHECK(blk >= 0 && blk < m.n_blocks && !seen[(size_t)blk]);
        seen[(size_t)blk] = 1;
        const int n = WV < m.n_faces - blk * WV ? WV : m.n_faces - blk * WV;
        KNN_CHECK(n >= 1 && n <= WV);
        ghr::float4 tile[3 * WV];
        std::memset(tile, 0xff, sizeof(tile));  // what the lanes past 3 n leave: never read
        for (int i = 0; i < 3 * n; i++) {
            const size_t at = (size_t)blk * (3 * WV) + i;
            KNN_CHECK(at < 3 * (size_t)m.n_faces);
            tile[i] = m.rec[at];
        }
        for (int j = 0; j < n; j++) {
            bool any = false;
            for (int l = 0; l < WV; l++) any = any || (valid[l] && near[l].needs(near[l].face_bound(tile + 3 * j, q3[l])));
            if (!any) continue;
            for (int l = 0; l < WV; l++) near[l].take(tile + 3 * j, q[l]);
        }
        scanned++;
    };
    auto any_needs = [&](const ghr::float4* box) {
        bool any = false;
        for (int l = 0; l < WV; l++) any = any || (valid[l] && near[l].needs(near[l].bound(q3[l], box[0], box[1])));
        return any;
    };
    scan_block(first);
    const int first_sb = first / GHR_KNN_SUPER;
    for (int s = 0; s < m.n_super; s++) {
        const int sb = first_sb + s < m.n_super ? first_sb + s : first_sb + s - m.n_super;
        KNN_CHECK(sb >= 0 && sb < m.n_super);
        if (!any_needs(m.sbox + 2 * (size_t)sb)) continue;
        const int b_end = m.n_blocks < (sb + 1) * GHR_KNN_SUPER ? m.n_blocks : (sb + 1) * GHR_KNN_SUPER;
        for (int blk = sb * GHR_KNN_SUPER; blk < b_end; blk++) {
            if (blk == first) continue;
            if (!any_needs(m.bbox + 2 * (size_t)blk)) continue;
            scan_block(blk);
        }
    }
    return scanned;
}

}  // namespace

extern "C" {

// ghr_field_build + ghr_field_trace_guarded.  seed: -1 the kernel's seed block (the block of the key of the lowest searching lane's
// y), otherwise every search starts at block seed % n_blocks (the results must not depend on it).  log: [S][M][GROW_LOG] or NULL --
// for every step the strand made: x[3], t[3] (the state the field was asked at), rho, v[3], c[3] (what it answered), [13] 1
// supported / 0 coasted / -1 stopped by the coast rule; and unless it stopped there: [14..16] the heading after the update,
// [17..19] y, [20] d2, [21..23] the closest point, [24] in, [25] 0 free / 1 pushed / 2 contact with d2 == 0 / 3 stopped head-on, [26..28] the heading after the guard (not
// when it stopped).
// Rows never reached keep the caller's fill.
void ghrsim_grow_guarded(int64_t P, const float* pts, const int64_t* order, const float* dirs, const float* weights, const float* colors,
                         const void* tris_blob, const void* grid_blob, int64_t S, const float* roots, const float* normals,
                         const int64_t* rorder, int32_t M, float r2, float h, float beta, float rho_min, int32_t max_coast, float margin,
                         int32_t seed, float* path, int32_t* steps, float* rgb, int32_t* contacts, uint8_t* stop, float* log)
{
    Field fld(P, pts, order, dirs, weights, colors);
    const HeadBlobs head(tris_blob, grid_blob);
    const ghr::FieldTraceArgs a{r2, h, beta, 1.f - beta, rho_min, M, max_coast};
    for (int64_t s0 = 0; s0 < S; s0 += WV) {
        ghr::GrowStrand st[WV];
        bool mine[WV], live[WV];
        int64_t row[WV];
        for (int l = 0; l < WV; l++) {
            mine[l] = s0 + l < S;
            row[l] = field_row(rorder, mine[l] ? s0 + l : s0, S);
            KNN_CHECK(row[l] >= 0 && row[l] < S);
            ghr::grow_strand_init(st[l], roots + row[l] * 3, normals + row[l] * 3);
            st[l].f.live = mine[l];
            if (mine[l])
                for (int k = 0; k < 3; k++) path[(size_t)row[l] * (M + 1) * 3 + k] = st[l].f.x[k];
        }
        for (int j = 0; j < M; j++) {
            bool any = false;
            ghr::float3 q[WV];
            std::vector<ghr::FieldGather> g;
            for (int l = 0; l < WV; l++) {
                any = any || st[l].f.live;
                live[l] = st[l].f.live;
                q[l] = ghr::float3{st[l].f.x[0], st[l].f.x[1], st[l].f.x[2]};
                g.emplace_back(a.r2, st[l].f.t[0], st[l].f.t[1], st[l].f.t[2], fld.pay(), fld.ptile);
            }
            if (!any) break;
            field_walk(fld, q, live, g.data());
            int how[WV];
            bool asks[WV];
            ghr::MdVec y[WV];
            ghr::MdNearest near[WV];
            int src = -1;
            for (int l = 0; l < WV; l++) {
                float* lg = log && live[l] ? log + ((size_t)row[l] * M + j) * GROW_LOG : nullptr;
                if (lg) {
                    const float rec[13] = {st[l].f.x[0], st[l].f.x[1], st[l].f.x[2], st[l].f.t[0], st[l].f.t[1], st[l].f.t[2], g[l].rho,
                                           g[l].vx,      g[l].vy,      g[l].vz,      g[l].cx,      g[l].cy,      g[l].cz};
                    std::memcpy(lg, rec, sizeof(rec));
                }
                how[l] = live[l] ? ghr::field_strand_heading(st[l].f, g[l], a) : ghr::FIELD_STOPPED;
                if (live[l] && how[l] == ghr::FIELD_STOPPED) st[l].stop = GHR_GROW_STOP_COAST;
                if (lg) lg[13] = how[l] == ghr::FIELD_SUPPORTED ? 1.f : (how[l] == ghr::FIELD_COASTED ? 0.f : -1.f);
                y[l] = ghr::MdVec{st[l].f.x[0] + a.h * st[l].f.t[0], st[l].f.x[1] + a.h * st[l].f.t[1], st[l].f.x[2] + a.h * st[l].f.t[2]};
                asks[l] = st[l].f.live && ghr::md_finite(y[l].x) && ghr::md_finite(y[l].y) && ghr::md_finite(y[l].z);
                if (asks[l] && src < 0) src = l;
            }
            if (src >= 0) {
                const float ys[3] = {y[src].x, y[src].y, y[src].z};
                const int first = seed < 0 ? ghr::md_seed_block(head.md.bkeys, head.md.n_blocks, ghr::knn_key(ys, head.bounds))
                                           : seed % head.md.n_blocks;
                grow_wave_search(head.md, y, asks, first, near);
            }
            for (int l = 0; l < WV; l++) {
                if (!st[l].f.live) continue;
                const bool in = asks[l] && ghr::mesh_contains_one(head.mesh, y[l].x, y[l].y, y[l].z, nullptr);
                KNN_CHECK(!asks[l] || (unsigned)near[l].face < (unsigned)head.md.n_faces);  // a finite query always finds a face
                const float yy[3] = {y[l].x, y[l].y, y[l].z}, c[3] = {near[l].point.x, near[l].point.y, near[l].point.z};
                const float d2 = asks[l] ? near[l].best : __builtin_inff();
                float* lg = log ? log + ((size_t)row[l] * M + j) * GROW_LOG : nullptr;
                if (lg) {
                    const float rec[11] = {st[l].f.t[0], st[l].f.t[1], st[l].f.t[2], yy[0], yy[1], yy[2], d2, c[0], c[1], c[2], in ? 1.f : 0.f};
                    std::memcpy(lg + 14, rec, sizeof(rec));
                }
                const int before = st[l].contacts;
                if (ghr::grow_guard_step(st[l], yy, d2, c, in, how[l] == ghr::FIELD_SUPPORTED, margin)) {
                    KNN_CHECK(st[l].f.rows - 1 >= 1 && st[l].f.rows - 1 <= M);
                    for (int k = 0; k < 3; k++) path[((size_t)row[l] * (M + 1) + st[l].f.rows - 1) * 3 + k] = st[l].f.x[k];
                    if (lg) {
                        lg[25] = st[l].contacts == before ? 0.f : (d2 == 0.f ? 2.f : 1.f);
                        for (int k = 0; k < 3; k++) lg[26 + k] = st[l].f.t[k];
                    }
                } else if (lg) {
                    lg[25] = 3.f;
                }
            }
        }
        for (int l = 0; l < WV; l++) {
            if (!mine[l]) continue;
            for (int r = st[l].f.rows; r <= M; r++)
                for (int k = 0; k < 3; k++) path[((size_t)row[l] * (M + 1) + r) * 3 + k] = st[l].f.x[k];
            steps[row[l]] = st[l].f.steps;
            ghr::field_strand_rgb(st[l].f, rgb + row[l] * 3);
            contacts[row[l]] = st[l].contacts;
            stop[row[l]] = (uint8_t)st[l].stop;
        }
    }
}

}  // extern "C"
