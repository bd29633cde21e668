// ghr_hostsim_field.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Compiles gaussianhaircut_amd/csrc/ghr_field.h as plain C++ for the host and walks k_field_pack, k_field_query, k_field_trace and
// k_strands_resample with a 64-lane wave kept in arrays: the same GHR_HD arithmetic and policy, the cloud built by
// ghr_hostsim_knn.cpp's walk of k_knn_boxes, the payload planes in heap blocks of exactly their bytes, and knn_walk's order from
// block 0 -- the stage hook called for every lane between the staging of a block and its scan, every ballot evaluated over the
// lanes' CURRENT states before the scan it guards.  Every index is checked (KNN_CHECK aborts with the expression).
// tests/test_field_cpu.py loads this as a shared library; ghr_field_selfcheck.cpp includes it and adds a main().
#include "ghr_hostsim_knn.cpp"
#include "../../gaussianhaircut_amd/csrc/ghr_field.h"

namespace {

// A field as ghr_field_build leaves it: the cloud and the two payload planes (every byte 0xff until k_field_pack's walk writes it).
struct Field {
    Workspace ws;
    ghr::float4 *dm, *f, *ptile;
    Field(int64_t P, const float* pts, const int64_t* order, const float* dirs, const float* weights, const float* colors)
        : ws({(uint64_t)P})
    {
        KNN_CHECK(P >= 1);
        dm = (ghr::float4*)std::malloc((size_t)P * sizeof(ghr::float4));
        f = (ghr::float4*)std::malloc((size_t)P * sizeof(ghr::float4));
        ptile = (ghr::float4*)std::malloc(2 * WV * sizeof(ghr::float4));
        KNN_CHECK(dm && f && ptile);
        std::memset(dm, 0xff, (size_t)P * sizeof(ghr::float4));
        std::memset(f, 0xff, (size_t)P * sizeof(ghr::float4));
        const ghr::KnnCloud& c = ws.clouds[0];
        boxes(c, pts, order);
        for (int64_t i = 0; i < P; i++) {  // k_field_pack
            int o = ghr::knn_as_int(c.sorted[i].w);
            if ((unsigned)o >= (unsigned)c.P) o = 0;
            KNN_CHECK(o >= 0 && o < P);
            const size_t b = (size_t)o * 3;
            dm[i] = ghr::float4{dirs[b], dirs[b + 1], dirs[b + 2], weights[o]};
            f[i] = ghr::float4{colors[b], colors[b + 1], colors[b + 2], 0.f};
        }
    }
    ~Field() { std::free(dm); std::free(f); std::free(ptile); }
    Field(const Field&) = delete;
    Field& operator=(const Field&) = delete;
    const ghr::KnnCloud& cloud() const { return ws.clouds[0]; }
    ghr::FieldPayload pay() const { return ghr::FieldPayload{dm, f}; }
};

// knn_walk with first = 0, skip = -1 and the stage hook; returns the blocks scanned
unsigned field_walk(const Field& fld, const ghr::float3* q, const bool* valid, ghr::FieldGather* pol)
{
    const ghr::KnnCloud& c = fld.cloud();
    unsigned scanned = 0;
    auto scan_block = [&](int blk) {
        KNN_CHECK(blk >= 0 && blk < c.nblocks);
        const int n = GHR_KNN_BLOCK < c.P - blk * GHR_KNN_BLOCK ? GHR_KNN_BLOCK : c.P - blk * GHR_KNN_BLOCK;
        KNN_CHECK(n >= 1 && n <= WV);
        ghr::float4 tile[WV];
        std::memset(tile, 0xff, sizeof(tile));  // what a lane >= n would leave: never read
        std::memset(fld.ptile, 0xff, 2 * WV * sizeof(ghr::float4));
        for (int l = 0; l < n; l++) tile[l] = c.sorted[(long long)blk * GHR_KNN_BLOCK + l];
        for (int l = 0; l < WV; l++) {
            KNN_CHECK(l >= n || (long long)blk * GHR_KNN_BLOCK + l < c.P);
            ghr::knn_stage(pol[l], blk, n, l, 0);
        }
        for (int l = 0; l < WV; l++) pol[l].scan(tile, n, -1, q[l]);
        scanned++;
    };
    auto any_needs = [&](const ghr::float4* box) {
        bool any = false;
        for (int l = 0; l < WV; l++) any = any || (valid[l] && pol[l].needs(pol[l].bound(q[l], box[0], box[1])));
        return any;
    };
    scan_block(0);
    for (int sb = 0; sb < c.nsuper; sb++) {
        if (!any_needs(c.sbox + 2 * (size_t)sb)) continue;
        const int b_end = c.nblocks < (sb + 1) * GHR_KNN_SUPER ? c.nblocks : (sb + 1) * GHR_KNN_SUPER;
        for (int blk = sb * GHR_KNN_SUPER; blk < b_end; blk++) {
            if (blk == 0) continue;
            if (!any_needs(c.bbox + 2 * (size_t)blk)) continue;
            scan_block(blk);
        }
    }
    return scanned;
}

int64_t field_row(const int64_t* order, int64_t i, int64_t N)  // field_row of the kernels
{
    if (!order) return i;
    return (order[i] < 0 || order[i] >= N) ? 0 : order[i];
}

}  // namespace

extern "C" {

// ghr_field_build + ghr_field_query; scanned: [ceil(Q / 64)] blocks each wave scanned, or NULL
void ghrsim_field_query(int64_t P, const float* pts, const int64_t* order, const float* dirs, const float* weights, const float* colors,
                        int64_t Q, const float* x, const float* t, const int64_t* qorder, float r2, float* rho, float* v, float* c,
                        int32_t* n, uint32_t* scanned)
{
    Field fld(P, pts, order, dirs, weights, colors);
    for (int64_t q0 = 0; q0 < Q; q0 += WV) {
        ghr::float3 q[WV];
        bool valid[WV];
        int64_t row[WV];
        std::vector<ghr::FieldGather> g;
        for (int l = 0; l < WV; l++) {
            valid[l] = q0 + l < Q;
            row[l] = field_row(qorder, valid[l] ? q0 + l : q0, Q);
            KNN_CHECK(row[l] >= 0 && row[l] < Q);
            q[l] = ghr::float3{x[row[l] * 3], x[row[l] * 3 + 1], x[row[l] * 3 + 2]};
            g.emplace_back(r2, t[row[l] * 3], t[row[l] * 3 + 1], t[row[l] * 3 + 2], fld.pay(), fld.ptile);
        }
        const unsigned ns = field_walk(fld, q, valid, g.data());
        if (scanned) scanned[q0 / WV] = ns;
        for (int l = 0; l < WV; l++) {
            if (!valid[l]) continue;
            const int64_t r = row[l];
            rho[r] = g[l].rho;
            v[r * 3] = g[l].vx; v[r * 3 + 1] = g[l].vy; v[r * 3 + 2] = g[l].vz;
            c[r * 3] = g[l].cx; c[r * 3 + 1] = g[l].cy; c[r * 3 + 2] = g[l].cz;
            n[r] = g[l].n;
        }
    }
}

// ghr_field_build + ghr_field_trace.  log: [S][M][14] or NULL -- for every step the strand made, the state the field was asked at
// and what it answered: x[3], t[3], rho, v[3], c[3], then 1 (supported), 0 (coasted) or -1 (stopped here); rows never reached
// keep the caller's fill.
void ghrsim_field_trace(int64_t P, const float* pts, const int64_t* order, const float* dirs, const float* weights, const float* colors,
                        int64_t S, const float* roots, const float* normals, const int64_t* rorder, int32_t M, float r2, float h,
                        float beta, float rho_min, int32_t max_coast, float* path, int32_t* steps, float* rgb, float* log)
{
    Field fld(P, pts, order, dirs, weights, colors);
    const ghr::FieldTraceArgs a{r2, h, beta, 1.f - beta, rho_min, M, max_coast};
    for (int64_t s0 = 0; s0 < S; s0 += WV) {
        ghr::FieldStrand st[WV];
        bool mine[WV], live[WV];
        int64_t row[WV];
        for (int l = 0; l < WV; l++) {
            mine[l] = s0 + l < S;
            row[l] = field_row(rorder, mine[l] ? s0 + l : s0, S);
            KNN_CHECK(row[l] >= 0 && row[l] < S);
            ghr::field_strand_init(st[l], roots + row[l] * 3, normals + row[l] * 3);
            st[l].live = mine[l];
            if (mine[l])
                for (int k = 0; k < 3; k++) path[(size_t)row[l] * (M + 1) * 3 + k] = st[l].x[k];
        }
        for (int j = 0; j < M; j++) {
            bool any = false;
            ghr::float3 q[WV];
            std::vector<ghr::FieldGather> g;
            for (int l = 0; l < WV; l++) {
                any = any || st[l].live;
                live[l] = st[l].live;
                q[l] = ghr::float3{st[l].x[0], st[l].x[1], st[l].x[2]};
                g.emplace_back(a.r2, st[l].t[0], st[l].t[1], st[l].t[2], fld.pay(), fld.ptile);
            }
            if (!any) break;
            field_walk(fld, q, live, g.data());
            for (int l = 0; l < WV; l++) {
                if (!st[l].live) continue;
                float* lg = log ? log + ((size_t)row[l] * M + j) * 14 : nullptr;
                if (lg) {
                    const float rec[13] = {st[l].x[0], st[l].x[1], st[l].x[2], st[l].t[0], st[l].t[1], st[l].t[2], g[l].rho,
                                           g[l].vx,    g[l].vy,    g[l].vz,    g[l].cx,    g[l].cy,    g[l].cz};
                    std::memcpy(lg, rec, sizeof(rec));
                }
                const int steps_before = st[l].steps;
                if (ghr::field_strand_step(st[l], g[l], a)) {
                    KNN_CHECK(st[l].rows - 1 >= 1 && st[l].rows - 1 <= M);
                    for (int k = 0; k < 3; k++) path[((size_t)row[l] * (M + 1) + st[l].rows - 1) * 3 + k] = st[l].x[k];
                    if (lg) lg[13] = st[l].steps != steps_before ? 1.f : 0.f;
                } else if (lg) {
                    lg[13] = -1.f;
                }
            }
        }
        for (int l = 0; l < WV; l++) {
            if (!mine[l]) continue;
            for (int r = st[l].rows; r <= M; r++)
                for (int k = 0; k < 3; k++) path[((size_t)row[l] * (M + 1) + r) * 3 + k] = st[l].x[k];
            steps[row[l]] = st[l].steps;
            ghr::field_strand_rgb(st[l], rgb + row[l] * 3);
        }
    }
}

// k_strands_resample
void ghrsim_strands_resample(int64_t S, int32_t M, int32_t L, const float* path, const int32_t* steps, float* out)
{
    for (int64_t i = 0; i < S * L; i++) {
        const int s = (int)(i / L), k = (int)(i % L);
        ghr::field_resample_point(path + (size_t)s * (M + 1) * 3, M, steps[s], L, k, out + (size_t)i * 3);
    }
}

}  // extern "C"
