// ghr_hostsim_meshdist.cpp -- TEST SCAFFOLDING (never shipped, never on the product path).
//
// Compiles gaussianhaircut_amd/csrc/ghr_meshdist.h as plain C++ for the host: the product's own builder (mesh_tris_plan /
// mesh_tris_fill), its per-element functions (md_face, MdNearest, md_seed_block, knn_key, knn_box_dist, md_backward_one) and a
// restatement of k_meshdist_search's wave walk with the 64 lanes kept in arrays -- seed block, superblocks in rotation, blocks,
// and inside a staged block the ballot on every face's own box; every ballot evaluated over the lanes' CURRENT states before the scan
// it guards, as the kernel's lockstep does.  Every index
// the walk forms is checked (MD_CHECK aborts with the expression), the tile is poisoned past the staged records, and no wave may
// scan a block twice.  tests/test_mesh_distance_cpu.py loads this as a shared library; ghr_meshdist_selfcheck.cpp includes it
// and adds a main().
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#define MD_CHECK(cond)                                                                                \
    do {                                                                                              \
        if (!(cond)) {                                                                                \
            std::fprintf(stderr, "ghr_hostsim_meshdist.cpp:%d: check failed: %s\n", __LINE__, #cond); \
            std::abort();                                                                             \
        }                                                                                             \
    } while (0)
#define GHR_MD_CHECK(cond) MD_CHECK(cond)
#include "../../gaussianhaircut_amd/csrc/ghr_meshdist.h"

namespace {

constexpr int WV = GHR_KNN_BLOCK;

struct Blob {
    ghr::MeshTris h;
    ghr::MdView m;
    explicit Blob(const void* blob)
    {
        std::memcpy(&h, blob, sizeof(h));
        MD_CHECK(h.magic == GHR_MD_MAGIC && h.n_faces >= 1);
        MD_CHECK(h.n_blocks == (h.n_faces + WV - 1) / WV && h.n_super == (h.n_blocks + GHR_KNN_SUPER - 1) / GHR_KNN_SUPER);
        MD_CHECK(h.off_rec >= sizeof(ghr::MeshTris) && h.off_rec + 48ull * h.n_faces <= h.off_bbox);
        MD_CHECK(h.off_bbox + 32ull * h.n_blocks <= h.off_sbox && h.off_sbox + 32ull * h.n_super <= h.off_keys);
        MD_CHECK(h.off_keys + 8ull * h.n_blocks <= h.bytes);
        MD_CHECK(((h.off_rec | h.off_bbox | h.off_sbox | h.off_keys | h.bytes) & 15u) == 0);
        m = ghr::md_view(h, blob);
    }
};

bool finite3(const float* p) { return ghr::md_finite(p[0]) && ghr::md_finite(p[1]) && ghr::md_finite(p[2]); }

unsigned long long faces_taken = 0;  // faces evaluated by the waves since the last ghrsim_md_faces_taken()

// k_meshdist_search for the wave of queries q0 .. q0 + 63 of the key order.  Returns the number of blocks scanned.
unsigned wave_search(const Blob& B, int64_t Q, const float* pts, const int64_t* order, const uint64_t* keys, int64_t q0, float* dist2,
                     int32_t* face, float* point)
{
    const ghr::MdView& m = B.m;
    MD_CHECK(q0 >= 0 && q0 < Q);
    const int nq = (int)(WV < Q - q0 ? WV : Q - q0);
    bool has[WV], finite[WV], valid[WV];
    int64_t o[WV];
    ghr::MdVec q[WV];
    ghr::float3 q3[WV];
    for (int l = 0; l < WV; l++) {
        has[l] = q0 + l < Q;
        const int64_t at = has[l] ? q0 + l : q0;
        MD_CHECK(at >= 0 && at < Q);
        o[l] = order[at];
        if (o[l] < 0 || o[l] >= Q) o[l] = 0;  // the kernel's clamp
        q[l] = ghr::MdVec{pts[3 * o[l]], pts[3 * o[l] + 1], pts[3 * o[l] + 2]};
        q3[l] = ghr::float3{q[l].x, q[l].y, q[l].z};
        finite[l] = finite3(pts + 3 * o[l]);
        valid[l] = has[l] && finite[l];
    }
    MD_CHECK(q0 + nq / 2 < Q);
    const int first = ghr::md_seed_block((const unsigned long long*)m.bkeys, m.n_blocks, keys[q0 + nq / 2]);
    MD_CHECK(first >= 0 && first < m.n_blocks);
    ghr::MdNearest near[WV];
    std::vector<unsigned char> seen((size_t)m.n_blocks, 0);
    unsigned scanned = 0;
    auto scan_block = [&](int blk) {
        MD_CHECK(blk >= 0 && blk < m.n_blocks);
        MD_CHECK(!seen[(size_t)blk]);
        seen[(size_t)blk] = 1;
        const int n = WV < m.n_faces - blk * WV ? WV : m.n_faces - blk * WV;
        MD_CHECK(n >= 1 && n <= WV);
        ghr::float4 tile[3 * WV];
        std::memset(tile, 0xff, sizeof(tile));  // what the lanes past 3 n leave: never read
        for (int k = 0; k < 3; k++)
            for (int l = 0; l < WV; l++) {
                const int i = k * WV + l;
                if (i >= 3 * n) continue;
                const size_t at = (size_t)blk * (3 * WV) + i;
                MD_CHECK(at < 3 * (size_t)m.n_faces);
                tile[i] = m.rec[at];
            }
        for (int j = 0; j < n; j++) {
            MD_CHECK(3 * j + 2 < 3 * WV);
            bool any = false;  // the ballot over the lanes' CURRENT states, before the face it guards
            for (int l = 0; l < WV; l++) any = any || (valid[l] && near[l].needs(near[l].face_bound(tile + 3 * j, q3[l])));
            if (!any) continue;
            faces_taken++;
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
        MD_CHECK(sb >= 0 && sb < m.n_super);
        if (!any_needs(m.sbox + 2 * (size_t)sb)) continue;
        const int b_end = m.n_blocks < (sb + 1) * GHR_KNN_SUPER ? m.n_blocks : (sb + 1) * GHR_KNN_SUPER;
        for (int blk = sb * GHR_KNN_SUPER; blk < b_end; blk++) {
            if (blk == first) continue;
            if (!any_needs(m.bbox + 2 * (size_t)blk)) continue;
            scan_block(blk);
        }
    }
    for (int l = 0; l < WV; l++) {
        if (!has[l]) continue;
        MD_CHECK(o[l] >= 0 && o[l] < Q);
        dist2[o[l]] = finite[l] ? near[l].best : __builtin_inff();
        face[o[l]] = finite[l] && (unsigned)near[l].face < (unsigned)m.n_faces ? near[l].face : -1;
        MD_CHECK(!finite[l] || face[o[l]] >= 0);  // a finite query always finds a face
        point[3 * o[l]] = finite[l] ? near[l].point.x : q[l].x;
        point[3 * o[l] + 1] = finite[l] ? near[l].point.y : q[l].y;
        point[3 * o[l] + 2] = finite[l] ? near[l].point.z : q[l].z;
    }
    return scanned;
}

}  // namespace

extern "C" {

unsigned long long ghrsim_md_faces_taken(void) { const unsigned long long n = faces_taken; faces_taken = 0; return n; }

int ghrsim_md_header_bytes(void) { return (int)sizeof(ghr::MeshTris); }

int ghrsim_md_sizes(int nv, const float* v, int nf, const int32_t* f, ghr::MeshTris* h, char* why128)
{
    const char* w = ghr::mesh_tris_plan(nv, v, nf, f, h);
    if (w) { std::snprintf(why128, 128, "%s", w); return -1; }
    return 0;
}

int ghrsim_md_build(int nv, const float* v, int nf, const int32_t* f, void* blob, unsigned long long bytes, char* why128)
{
    ghr::MeshTris plan;
    const char* w = ghr::mesh_tris_plan(nv, v, nf, f, &plan);
    if (!w && plan.bytes != bytes) w = "bytes";
    if (!w) w = ghr::mesh_tris_fill(v, f, plan, blob);
    if (w) { std::snprintf(why128, 128, "%s", w); return -1; }
    return 0;
}

// The tables against their specification: every face once, in (key, face) order; records hold the vertices in index order;
// block and superblock boxes contain their faces' vertices (hence every candidate); bkeys are the first keys.  0 or a line number.
int ghrsim_md_verify(const float* v, const int32_t* f, const void* blob)
{
    const Blob B(blob);
    const ghr::MdView& m = B.m;
    const float* rec = reinterpret_cast<const float*>(m.rec);
    const float bounds[6] = {B.h.lo[0], B.h.lo[1], B.h.lo[2], B.h.hi[0], B.h.hi[1], B.h.hi[2]};
    std::vector<unsigned char> seen((size_t)m.n_faces, 0);
    unsigned long long prev_key = 0;
    int32_t prev_face = -1;
    for (int i = 0; i < m.n_faces; i++) {
        const float* r = rec + (size_t)GHR_MD_REC_WORDS * i;
        int32_t face;
        std::memcpy(&face, r + 9, 4);
        if (face < 0 || face >= m.n_faces || seen[(size_t)face]) return __LINE__;
        seen[(size_t)face] = 1;
        int32_t t[3] = {f[3 * face], f[3 * face + 1], f[3 * face + 2]};
        std::sort(t, t + 3);
        float lo[3], hi[3], centre[3];
        for (int c = 0; c < 3; c++) {
            lo[c] = fminf(fminf(v[3 * t[0] + c], v[3 * t[1] + c]), v[3 * t[2] + c]);
            hi[c] = fmaxf(fmaxf(v[3 * t[0] + c], v[3 * t[1] + c]), v[3 * t[2] + c]);
            centre[c] = (lo[c] + hi[c]) * 0.5f;
            for (int k = 0; k < 3; k++)
                if (std::memcmp(r + 3 * k + c, v + 3 * t[k] + c, 4) != 0) return __LINE__;
        }
        const unsigned long long key = ghr::knn_key(centre, bounds);
        if (i > 0 && !(prev_key < key || (prev_key == key && prev_face < face))) return __LINE__;
        prev_key = key; prev_face = face;
        const int b = i / WV, s = b / GHR_KNN_SUPER;
        if (i % WV == 0 && m.bkeys[b] != key) return __LINE__;
        for (int c = 0; c < 3; c++) {
            const float blo = (&m.bbox[2 * b].x)[c], bhi = (&m.bbox[2 * b + 1].x)[c];
            const float slo = (&m.sbox[2 * s].x)[c], shi = (&m.sbox[2 * s + 1].x)[c];
            if (!(blo <= lo[c] && hi[c] <= bhi && slo <= blo && bhi <= shi)) return __LINE__;
        }
        uint32_t pad[2];
        std::memcpy(pad, r + 10, 8);
        if (pad[0] || pad[1]) return __LINE__;
    }
    return 0;
}

void ghrsim_md_keys(const void* blob, int64_t Q, const float* pts, uint64_t* keys)  // ghr_knn_keys over the header's bounds
{
    const Blob B(blob);
    const float bounds[6] = {B.h.lo[0], B.h.lo[1], B.h.lo[2], B.h.hi[0], B.h.hi[1], B.h.hi[2]};
    for (int64_t i = 0; i < Q; i++) keys[i] = ghr::knn_key(pts + 3 * i, bounds);
}

// ghr_mesh_closest: keys, a stable key sort, the waves.  order_in: the caller's permutation and sorted keys, or NULL for the
// simulator's own.  scanned: [ceil(Q / 64)] blocks each wave scanned, or NULL.
void ghrsim_md_closest(const void* blob, int64_t Q, const float* pts, const int64_t* order_in, const uint64_t* keys_in, float* dist2,
                       int32_t* face, float* point, uint32_t* scanned)
{
    if (Q == 0) return;
    const Blob B(blob);
    std::vector<int64_t> order((size_t)Q);
    std::vector<uint64_t> sorted((size_t)Q);
    if (order_in) {
        std::memcpy(order.data(), order_in, sizeof(int64_t) * (size_t)Q);
        std::memcpy(sorted.data(), keys_in, sizeof(uint64_t) * (size_t)Q);
    } else {
        std::vector<uint64_t> keys((size_t)Q);
        ghrsim_md_keys(blob, Q, pts, keys.data());
        std::iota(order.begin(), order.end(), (int64_t)0);
        std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return keys[(size_t)a] < keys[(size_t)b]; });
        for (int64_t i = 0; i < Q; i++) sorted[(size_t)i] = keys[(size_t)order[(size_t)i]];
    }
    for (int64_t q0 = 0; q0 < Q; q0 += WV) {
        const unsigned n = wave_search(B, Q, pts, order.data(), sorted.data(), q0, dist2, face, point);
        if (scanned) scanned[q0 / WV] = n;
    }
}

// For every finite query and every block: every face's d is >= the block's (and its superblock's) bound and every face's
// closest point lies in the block's box.  Returns the number of violations.
long long ghrsim_md_check_bounds(const void* blob, int64_t Q, const float* pts)
{
    const Blob B(blob);
    const ghr::MdView& m = B.m;
    long long bad = 0;
    for (int64_t i = 0; i < Q; i++) {
        if (!finite3(pts + 3 * i)) continue;
        const ghr::MdVec q{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
        const ghr::float3 q3{q.x, q.y, q.z};
        for (int f = 0; f < m.n_faces; f++) {
            const ghr::float4 r0 = m.rec[3 * (size_t)f], r1 = m.rec[3 * (size_t)f + 1], r2 = m.rec[3 * (size_t)f + 2];
            ghr::MdVec c;
            const float d = ghr::md_face(ghr::MdVec{r0.x, r0.y, r0.z}, ghr::MdVec{r0.w, r1.x, r1.y}, ghr::MdVec{r1.z, r1.w, r2.x}, q, &c);
            if (!(ghr::MdNearest().face_bound(m.rec + 3 * (size_t)f, q3) <= d)) bad++;  // the face's own box
            const int b = f / WV, s = b / GHR_KNN_SUPER;
            const ghr::float4 lo = m.bbox[2 * b], hi = m.bbox[2 * b + 1];
            if (!(ghr::knn_box_dist(q3, lo, hi) <= d)) bad++;
            if (!(ghr::knn_box_dist(q3, m.sbox[2 * s], m.sbox[2 * s + 1]) <= d)) bad++;
            if (!(c.x >= lo.x && c.x <= hi.x && c.y >= lo.y && c.y <= hi.y && c.z >= lo.z && c.z <= hi.z)) bad++;
        }
    }
    return bad;
}

void ghrsim_md_backward(int64_t Q, const float* pts, const float* closest, const float* dist2, const uint8_t* inside, const float* g,
                        float* d_points)  // k_meshdist_bwd
{
    for (int64_t i = 0; i < Q; i++) ghr::md_backward_one(pts + 3 * i, closest + 3 * i, dist2[i], inside[i] != 0, g[i], d_points + 3 * i);
}

}  // extern "C"
