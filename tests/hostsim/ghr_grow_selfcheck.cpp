// ghr_grow_selfcheck.cpp -- TEST SCAFFOLDING: ghr_hostsim_grow.cpp's walk as a program of its own, built with
// -fsanitize=address,undefined by tests/test_grow_guarded_cpu.py and run directly.  Every buffer has exactly its size; the mesh
// tables are built by the headers' own builders into heap blocks of exactly their bytes.  A latitude-longitude sphere of radius
// 0.35 about the middle of a seeded cloud in the unit cube (F = 12, 112 and 4140 faces: one block, a 64-face block end, a second
// superblock), S = 1, 65 and 130 strands: every output element is written, every strand stops for a stated reason, a second walk
// from another seed block of the mesh search and in reversed root order gives the same bits, and every appended point that came
// out of a contact lies outside the mesh's inscribed sphere.
#include <algorithm>
#include <cmath>
#include <numeric>
#include "ghr_hostsim_grow.cpp"

namespace {

uint32_t g_state = 2463534242u;
float rnd() { g_state = g_state * 1664525u + 1013904223u; return (float)(g_state >> 8) / 16777216.0f; }

struct Heap {
    void* p;
    explicit Heap(size_t bytes) : p(std::aligned_alloc(64, (bytes + 63) / 64 * 64)) { KNN_CHECK(p); }
    ~Heap() { std::free(p); }
};

void uv_sphere(int n_lon, int n_lat, float radius, std::vector<float>& v, std::vector<int32_t>& f)
{
    const float pi = 3.14159265358979f;
    auto put = [&](float x, float y, float z) { v.push_back(0.5f + radius * x); v.push_back(0.5f + radius * y); v.push_back(0.5f + radius * z); };
    put(0, 0, 1);
    for (int i = 1; i < n_lat; i++)
        for (int j = 0; j < n_lon; j++) {
            const float th = pi * i / n_lat, ph = 2 * pi * j / n_lon;
            put(std::sin(th) * std::cos(ph), std::sin(th) * std::sin(ph), std::cos(th));
        }
    put(0, 0, -1);
    const int last = (int)v.size() / 3 - 1;
    auto ring = [&](int i, int j) { return 1 + (i - 1) * n_lon + j % n_lon; };
    auto tri = [&](int a, int b, int c) { f.push_back(a); f.push_back(b); f.push_back(c); };
    for (int j = 0; j < n_lon; j++) {
        tri(0, ring(1, j), ring(1, j + 1));
        tri(last, ring(n_lat - 1, j + 1), ring(n_lat - 1, j));
    }
    for (int i = 1; i < n_lat - 1; i++)
        for (int j = 0; j < n_lon; j++) {
            tri(ring(i, j), ring(i + 1, j), ring(i + 1, j + 1));
            tri(ring(i, j), ring(i + 1, j + 1), ring(i, j + 1));
        }
}

int run(int n_lon, int n_lat, int P, int S, int M)
{
    std::vector<float> v;
    std::vector<int32_t> f;
    const float radius = 0.35f;
    uv_sphere(n_lon, n_lat, radius, v, f);
    const int nv = (int)v.size() / 3, nf = (int)f.size() / 3;
    ghr::MeshTris tp;
    KNN_CHECK(!ghr::mesh_tris_plan(nv, v.data(), nf, f.data(), &tp));
    Heap tris((size_t)tp.bytes);
    KNN_CHECK(!ghr::mesh_tris_fill(v.data(), f.data(), tp, tris.p));
    ghr::MeshGrid gp;
    KNN_CHECK(!ghr::mesh_grid_plan(nv, v.data(), nf, f.data(), 0, &gp));
    Heap grid((size_t)gp.bytes);
    KNN_CHECK(!ghr::mesh_grid_fill(v.data(), f.data(), gp, grid.p));

    std::vector<float> pts((size_t)P * 3), dirs((size_t)P * 3), col((size_t)P * 3), w(P);
    for (int i = 0; i < P; i++) {
        float d[3], l = 0.f;
        for (int k = 0; k < 3; k++) pts[i * 3 + k] = rnd(), d[k] = rnd() - 0.5f, col[i * 3 + k] = rnd(), l += d[k] * d[k];
        l = std::sqrt(l) > 0.f ? std::sqrt(l) : 1.f;
        for (int k = 0; k < 3; k++) dirs[i * 3 + k] = d[k] / l;
        w[i] = 0.1f + rnd();
    }
    float bounds[6] = {0.f, 0.f, 0.f, 1.f, 1.f, 1.f};
    std::vector<uint64_t> keys(P);
    ghrsim_knn_keys(P, pts.data(), bounds, keys.data());
    std::vector<int64_t> order(P);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return keys[a] < keys[b]; });

    // roots on a shell just above the sphere, headings random: about half of them lean into it
    std::vector<float> roots((size_t)S * 3), normals((size_t)S * 3);
    for (int s = 0; s < S; s++) {
        float u[3], l = 0.f;
        for (int k = 0; k < 3; k++) u[k] = rnd() - 0.5f, l += u[k] * u[k];
        l = std::sqrt(l) > 1e-3f ? std::sqrt(l) : 1.f;
        for (int k = 0; k < 3; k++) roots[s * 3 + k] = 0.5f + (radius + 0.02f) * u[k] / l, normals[s * 3 + k] = rnd() - 0.5f;
    }
    if (S > 2) {
        for (int k = 0; k < 3; k++) roots[3 + k] = 30.f;   // never supported
        const float inf = __builtin_inff();
        roots[6] = inf;                                     // not finite: free, asks nothing of the mesh
    }
    const float r = P < 100 ? 0.6f : 0.12f, h = r / 2.5f, margin = 0.03f;
    auto walk = [&](const int64_t* rorder, int seed, std::vector<float>& path, std::vector<int32_t>& steps, std::vector<float>& rgb,
                    std::vector<int32_t>& contacts, std::vector<uint8_t>& stop, std::vector<float>* log) {
        path.assign((size_t)S * (M + 1) * 3, NAN); steps.assign(S, -1); rgb.assign((size_t)S * 3, NAN); contacts.assign(S, -1);
        stop.assign(S, 255);
        if (log) log->assign((size_t)S * M * GROW_LOG, NAN);
        ghrsim_grow_guarded(P, pts.data(), order.data(), dirs.data(), w.data(), col.data(), tris.p, grid.p, S, roots.data(), normals.data(),
                            rorder, M, r * r, h, 0.5f, 0.05f, 2, margin, seed, path.data(), steps.data(), rgb.data(), contacts.data(),
                            stop.data(), log ? log->data() : nullptr);
    };
    std::vector<float> path, rgb, log, path2, rgb2;
    std::vector<int32_t> steps, contacts, steps2, contacts2;
    std::vector<uint8_t> stop, stop2;
    walk(nullptr, -1, path, steps, rgb, contacts, stop, &log);
    std::vector<int64_t> rorder(S);
    std::iota(rorder.begin(), rorder.end(), 0);
    std::reverse(rorder.begin(), rorder.end());
    walk(rorder.data(), 1 + nf / 128, path2, steps2, rgb2, contacts2, stop2, nullptr);
    KNN_CHECK(std::memcmp(path.data(), path2.data(), path.size() * 4) == 0 && std::memcmp(rgb.data(), rgb2.data(), rgb.size() * 4) == 0);
    KNN_CHECK(steps == steps2 && contacts == contacts2 && stop == stop2);
    long touched = 0, head_on = 0;
    float inscribed = radius;  // the smallest distance of a face's plane from the centre
    for (int i = 0; i < nf; i++) {
        const float *a = v.data() + 3 * f[3 * i], *b = v.data() + 3 * f[3 * i + 1], *c = v.data() + 3 * f[3 * i + 2];
        const float e0[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e1[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
        const float n[3] = {e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]};
        const float ln = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        KNN_CHECK(ln > 0.f);
        inscribed = std::min(inscribed, std::fabs(n[0] * (a[0] - .5f) + n[1] * (a[1] - .5f) + n[2] * (a[2] - .5f)) / ln);
    }
    inscribed -= 1e-4f;
    for (int s = 0; s < S; s++) {
        KNN_CHECK(steps[s] >= 0 && steps[s] <= M && contacts[s] >= 0 && contacts[s] <= M && stop[s] <= 2);
        for (int k = 0; k < 3; k++) KNN_CHECK(!std::isnan(rgb[s * 3 + k]));
        const bool finite_root = std::isfinite(roots[s * 3]);
        for (int j = 0; j <= M; j++)
            for (int k = 0; k < 3; k++) KNN_CHECK(!finite_root || !std::isnan(path[((size_t)s * (M + 1) + j) * 3 + k]));
        int rows = 1;
        for (int j = 0; j < M; j++) {
            const float* lg = log.data() + ((size_t)s * M + j) * GROW_LOG;
            if (std::isnan(lg[13]) || lg[13] < 0.f || lg[25] == 3.f) continue;
            if (lg[25] == 1.f) {  // a pushed point: margin above its closest point, so outside the inscribed sphere
                const float* x = path.data() + ((size_t)s * (M + 1) + rows) * 3;
                const float d = std::sqrt((x[0] - .5f) * (x[0] - .5f) + (x[1] - .5f) * (x[1] - .5f) + (x[2] - .5f) * (x[2] - .5f));
                KNN_CHECK(d > inscribed);
                touched++;
            }
            rows++;
        }
        head_on += stop[s] == 2;
    }
    if (S > 2) KNN_CHECK(steps[1] == 0 && stop[1] == 1 && contacts[1] == 0 && contacts[2] == 0);
    std::printf("F %d P %d S %d M %d: pushed points %ld, head-on stops %ld\n", nf, P, S, M, touched, head_on);
    return 1;
}

}  // namespace

int main()
{
    int done = 0;
    done += run(3, 3, 65, 1, 5);        // F = 12
    done += run(8, 8, 4097, 65, 12);    // F = 112
    done += run(46, 46, 4097, 130, 12); // F = 4140: a second superblock
    done += run(8, 8, 1, 65, 3);        // a cloud of one point
    std::printf("%d cases ok\n", done);
    return 0;
}
