// ghr_hostsim_knn.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Compiles gaussianhaircut_amd/csrc/ghr_knn.h and ghr_nn.h as plain C++ for the host and walks k_knn_boxes, k_knn_search and
// k_nn_search with a 64-lane wave kept in arrays: the same GHR_HD arithmetic and policies, the cloud carved by knn_cloud inside a
// poisoned buffer of exactly the layout's bytes, and knn_walk's order -- first block, superblocks in rotation, blocks -- with every
// ballot evaluated over the lanes' CURRENT states before the scan it guards, as the kernel's lockstep does.  Every index a walk
// forms is checked (KNN_CHECK aborts with the expression), and no wave may scan a block twice.  tests/test_knn_cpu.py loads this
// as a shared library; ghr_knn_selfcheck.cpp includes it and adds a main().
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../gaussianhaircut_amd/csrc/ghr_nn.h"

#define KNN_CHECK(cond)                                                                          \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            std::fprintf(stderr, "ghr_hostsim_knn.cpp:%d: check failed: %s\n", __LINE__, #cond); \
            std::abort();                                                                        \
        }                                                                                        \
    } while (0)

namespace {

constexpr int WV = GHR_KNN_BLOCK;  // lanes of a wave = points of a block

// Clouds carved the way the C API carves them: one after the other in a heap block of exactly the layouts' bytes, every byte
// 0xff (a NaN in every float, -1 in every index) until k_knn_boxes' walk writes it.
struct Workspace {
    char* buf;
    std::vector<ghr::KnnCloud> clouds;
    explicit Workspace(std::vector<uint64_t> sizes)
    {
        uint64_t total = 0;
        for (uint64_t P : sizes) total += ghr::knn_layout(P).bytes;
        buf = (char*)std::malloc(total);
        KNN_CHECK(buf || total == 0);
        if (total) std::memset(buf, 0xff, total);
        uint64_t off = 0;
        for (uint64_t P : sizes) {
            const ghr::KnnLayout L = ghr::knn_layout(P);
            KNN_CHECK(L.off_sorted == 0 && L.off_sorted + P * sizeof(ghr::float4) <= L.off_bbox);
            KNN_CHECK(L.off_bbox + L.nblocks * 2 * sizeof(ghr::float4) <= L.off_sbox);
            KNN_CHECK(L.off_sbox + L.nsuper * 2 * sizeof(ghr::float4) <= L.bytes && off + L.bytes <= total);
            clouds.push_back(ghr::knn_cloud(buf + off, P));
            off += L.bytes;
        }
    }
    ~Workspace() { std::free(buf); }
    Workspace(const Workspace&) = delete;
    Workspace& operator=(const Workspace&) = delete;
};

void wave_min(float* v)  // knn_wave_min_max
{
    for (int m = 32; m >= 1; m >>= 1) {
        float t[WV];
        for (int l = 0; l < WV; l++) t[l] = fminf(v[l], v[l ^ m]);
        std::memcpy(v, t, sizeof(t));
    }
}

void wave_max(float* v)  // knn_wave_min_max
{
    for (int m = 32; m >= 1; m >>= 1) {
        float t[WV];
        for (int l = 0; l < WV; l++) t[l] = fmaxf(v[l], v[l ^ m]);
        std::memcpy(v, t, sizeof(t));
    }
}

void boxes(const ghr::KnnCloud& c, const float* pts, const int64_t* order)  // k_knn_boxes
{
    const int P = c.P;
    for (int sb = 0; sb < c.nsuper; sb++) {
        float red[GHR_KNN_WAVES][6];
        const int b_end = c.nblocks < (sb + 1) * GHR_KNN_SUPER ? c.nblocks : (sb + 1) * GHR_KNN_SUPER;
        for (int wave = 0; wave < GHR_KNN_WAVES; wave++) {
            float smin[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, smax[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
            for (int blk = sb * GHR_KNN_SUPER + wave; blk < b_end; blk += GHR_KNN_WAVES) {
                float lo[3][WV], hi[3][WV];
                for (int l = 0; l < WV; l++) {
                    const long long i = (long long)blk * GHR_KNN_BLOCK + l;
                    for (int a = 0; a < 3; a++) lo[a][l] = FLT_MAX, hi[a][l] = -FLT_MAX;
                    if (i >= P) continue;
                    const long long o = (order[i] < 0 || order[i] >= P) ? 0 : order[i];  // k_knn_boxes' clamp
                    KNN_CHECK(o >= 0 && o < P);
                    const float* p = pts + (size_t)o * 3;
                    c.sorted[i] = ghr::float4{p[0], p[1], p[2], ghr::knn_as_float((int)o)};
                    for (int a = 0; a < 3; a++) lo[a][l] = hi[a][l] = p[a];
                }
                for (int a = 0; a < 3; a++) {
                    wave_min(lo[a]);
                    wave_max(hi[a]);
                    smin[a] = fminf(smin[a], lo[a][0]);
                    smax[a] = fmaxf(smax[a], hi[a][0]);
                }
                KNN_CHECK(blk >= 0 && blk < c.nblocks);
                c.bbox[2 * (size_t)blk] = ghr::float4{lo[0][0], lo[1][0], lo[2][0], 0.f};
                c.bbox[2 * (size_t)blk + 1] = ghr::float4{hi[0][0], hi[1][0], hi[2][0], 0.f};
            }
            for (int a = 0; a < 3; a++) red[wave][a] = smin[a], red[wave][3 + a] = smax[a];
        }
        for (int w = 1; w < GHR_KNN_WAVES; w++)
            for (int a = 0; a < 3; a++) {
                red[0][a] = fminf(red[0][a], red[w][a]);
                red[0][3 + a] = fmaxf(red[0][3 + a], red[w][3 + a]);
            }
        c.sbox[2 * (size_t)sb] = ghr::float4{red[0][0], red[0][1], red[0][2], 0.f};
        c.sbox[2 * (size_t)sb + 1] = ghr::float4{red[0][3], red[0][4], red[0][5], 0.f};
    }
}

// One wave's queries: lane l holds q[l]; a lane without a query holds the block's first one and votes in no ballot.
struct Wave {
    ghr::float4 q4[WV];
    ghr::float3 q[WV];
    bool valid[WV];
};

Wave load_queries(const ghr::KnnCloud& c, long long qb)
{
    Wave w;
    for (int l = 0; l < WV; l++) {
        const long long qi = qb * GHR_KNN_BLOCK + l;
        w.valid[l] = qi < c.P;
        const long long at = w.valid[l] ? qi : qb * GHR_KNN_BLOCK;
        KNN_CHECK(at >= 0 && at < c.P);
        w.q4[l] = c.sorted[at];
        w.q[l] = ghr::float3{w.q4[l].x, w.q4[l].y, w.q4[l].z};
    }
    return w;
}

// knn_walk; skip_own: lane l leaves tile position l out of the first scan (k_knn_search), otherwise nothing is left out.
// Returns the number of blocks scanned.
template <class Policy>
unsigned walk(const ghr::KnnCloud& c, const Wave& w, int first, bool skip_own, Policy* pol)
{
    std::vector<unsigned char> seen(c.nblocks, 0);
    unsigned scanned = 0;
    auto scan_block = [&](int blk, bool skip_lane) {
        KNN_CHECK(blk >= 0 && blk < c.nblocks);
        KNN_CHECK(!seen[blk]);  // every block at most once per wave
        seen[blk] = 1;
        const int n = GHR_KNN_BLOCK < c.P - blk * GHR_KNN_BLOCK ? GHR_KNN_BLOCK : c.P - blk * GHR_KNN_BLOCK;
        KNN_CHECK(n >= 1 && n <= WV);
        ghr::float4 tile[WV];
        std::memset(tile, 0xff, sizeof(tile));  // what a lane >= n would leave: never read
        for (int l = 0; l < n; l++) {
            const long long at = (long long)blk * GHR_KNN_BLOCK + l;
            KNN_CHECK(at < c.P);
            tile[l] = c.sorted[at];
        }
        for (int l = 0; l < WV; l++) pol[l].scan(tile, n, skip_lane ? l : -1, w.q[l]);
        scanned++;
    };
    auto any_needs = [&](const ghr::float4* box) {
        bool any = false;
        for (int l = 0; l < WV; l++) any = any || (w.valid[l] && pol[l].needs(pol[l].bound(w.q[l], box[0], box[1])));
        return any;
    };
    scan_block(first, skip_own);
    const int first_sb = first / GHR_KNN_SUPER;
    for (int s = 0; s < c.nsuper; s++) {
        const int sb = first_sb + s < c.nsuper ? first_sb + s : first_sb + s - c.nsuper;
        KNN_CHECK(sb >= 0 && sb < c.nsuper);
        if (!any_needs(c.sbox + 2 * (size_t)sb)) continue;
        const int b_end = c.nblocks < (sb + 1) * GHR_KNN_SUPER ? c.nblocks : (sb + 1) * GHR_KNN_SUPER;
        for (int blk = sb * GHR_KNN_SUPER; blk < b_end; blk++) {
            if (blk == first) continue;
            if (!any_needs(c.bbox + 2 * (size_t)blk)) continue;
            scan_block(blk, false);
        }
    }
    return scanned;
}

template <int NORM>
void nn_search(const ghr::KnnCloud& x, const uint64_t* keys_x, const ghr::KnnCloud& y, const uint64_t* keys_y, float* dist,
               int32_t* idx, uint32_t* scanned)  // k_nn_search
{
    for (long long qb = 0; qb < x.nblocks; qb++) {
        const Wave w = load_queries(x, qb);
        const long long q0 = qb * GHR_KNN_BLOCK;
        const int nq = (int)(GHR_KNN_BLOCK < x.P - q0 ? GHR_KNN_BLOCK : x.P - q0);
        KNN_CHECK(q0 + nq / 2 < x.P);
        const int seed = ghr::nn_seed_block((const unsigned long long*)keys_y, y.P, keys_x[q0 + nq / 2]);
        KNN_CHECK(seed >= 0 && seed < y.nblocks);
        ghr::NnNearest<NORM> near[WV];
        const unsigned n = walk(y, w, seed, false, near);
        if (scanned) scanned[qb] = n;
        for (int l = 0; l < WV; l++) {
            if (!w.valid[l]) continue;
            const int o = ghr::knn_as_int(w.q4[l].w);
            KNN_CHECK(o >= 0 && o < x.P);
            dist[o] = near[l].best;
            idx[o] = near[l].index(y.P);
            KNN_CHECK(idx[o] >= 0 && idx[o] < y.P);
        }
    }
}

}  // namespace

extern "C" {

int ghrsim_knn_wave(void) { return WV; }

// {nblocks, nsuper, off_sorted, off_bbox, off_sbox, bytes}
void ghrsim_knn_layout(uint64_t P, uint64_t* out6)
{
    const ghr::KnnLayout L = ghr::knn_layout(P);
    const uint64_t v[6] = {L.nblocks, L.nsuper, L.off_sorted, L.off_bbox, L.off_sbox, L.bytes};
    std::memcpy(out6, v, sizeof(v));
}

void ghrsim_knn_keys(int64_t P, const float* pts, const float* bounds, uint64_t* keys)  // k_knn_keys
{
    for (int64_t i = 0; i < P; i++) keys[i] = ghr::knn_key(pts + (size_t)i * 3, bounds);
}

// ghr_knn_mean_dist2; scanned: [ceil(P / 64)] blocks each wave scanned, or NULL
void ghrsim_knn_mean_dist2(int64_t P, const float* pts, const int64_t* order, float* out, uint32_t* scanned)
{
    if (P == 0) return;
    Workspace ws({(uint64_t)P});
    const ghr::KnnCloud& c = ws.clouds[0];
    boxes(c, pts, order);
    for (int qb = 0; qb < c.nblocks; qb++) {  // k_knn_search
        const Wave w = load_queries(c, qb);
        ghr::KnnTop3 top[WV];
        const unsigned n = walk(c, w, qb, true, top);
        if (scanned) scanned[qb] = n;
        for (int l = 0; l < WV; l++) {
            if (!w.valid[l]) continue;
            const int o = ghr::knn_as_int(w.q4[l].w);
            KNN_CHECK(o >= 0 && o < P);
            out[o] = top[l].mean();
        }
    }
}

// ghr_nn_search; scanned: [ceil(Px / 64)] or NULL
void ghrsim_nn_search(int64_t Px, const float* x, const int64_t* order_x, const uint64_t* keys_x_sorted, int64_t Py, const float* y,
                      const int64_t* order_y, const uint64_t* keys_y_sorted, int norm, float* dist, int32_t* idx, uint32_t* scanned)
{
    KNN_CHECK(Py >= 1 && (norm == 1 || norm == 2));
    if (Px == 0) return;
    Workspace ws({(uint64_t)Px, (uint64_t)Py});
    boxes(ws.clouds[0], x, order_x);
    boxes(ws.clouds[1], y, order_y);
    if (norm == 2) nn_search<2>(ws.clouds[0], keys_x_sorted, ws.clouds[1], keys_y_sorted, dist, idx, scanned);
    else nn_search<1>(ws.clouds[0], keys_x_sorted, ws.clouds[1], keys_y_sorted, dist, idx, scanned);
}

}  // extern "C"
