// ghr_field_selfcheck.cpp -- TEST SCAFFOLDING: ghr_hostsim_field.cpp's walks as a program of its own, built with
// -fsanitize=address,undefined by tests/test_field_cpu.py and run directly.  Every buffer has exactly its size.  For seeded clouds of
// P = 1, 63, 64, 65, 4097 points: the pruned walk's rho, v, c, n equal, bit for bit, the sequential sums over ALL points in sorted
// order (the definition without the boxes); strands are traced and resampled; every output element is written.
#include <algorithm>
#include <cmath>
#include <numeric>
#include "ghr_hostsim_field.cpp"

namespace {

uint32_t g_state = 12345u;
float rnd() { g_state = g_state * 1664525u + 1013904223u; return (float)(g_state >> 8) / 16777216.0f; }

bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

int run(int P, int Q, float r)
{
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

    std::vector<float> x((size_t)Q * 3), t((size_t)Q * 3), rho(Q), v((size_t)Q * 3), c((size_t)Q * 3);
    std::vector<int32_t> n(Q, -1);
    std::vector<uint32_t> scanned((Q + 63) / 64);
    for (int i = 0; i < Q * 3; i++) x[i] = rnd() * 1.2f - 0.1f, t[i] = rnd() - 0.5f;
    const float r2 = r * r;
    ghrsim_field_query(P, pts.data(), order.data(), dirs.data(), w.data(), col.data(), Q, x.data(), t.data(), nullptr, r2, rho.data(),
                       v.data(), c.data(), n.data(), scanned.data());
    for (int q = 0; q < Q; q++) {  // the definition without the boxes
        ghr::FieldGather g(r2, t[q * 3], t[q * 3 + 1], t[q * 3 + 2], ghr::FieldPayload{nullptr, nullptr}, nullptr);
        const ghr::float3 qq{x[q * 3], x[q * 3 + 1], x[q * 3 + 2]};
        for (int i = 0; i < P; i++) {
            const int64_t o = order[i];
            const ghr::float4 p{pts[o * 3], pts[o * 3 + 1], pts[o * 3 + 2], 0.f};
            const float d2 = ghr::knn_dist2(p, qq);
            if (d2 < r2)
                g.add(d2, ghr::float4{dirs[o * 3], dirs[o * 3 + 1], dirs[o * 3 + 2], w[o]}, ghr::float4{col[o * 3], col[o * 3 + 1], col[o * 3 + 2], 0.f});
        }
        KNN_CHECK(same(g.rho, rho[q]) && g.n == n[q]);
        KNN_CHECK(same(g.vx, v[q * 3]) && same(g.vy, v[q * 3 + 1]) && same(g.vz, v[q * 3 + 2]));
        KNN_CHECK(same(g.cx, c[q * 3]) && same(g.cy, c[q * 3 + 1]) && same(g.cz, c[q * 3 + 2]));
    }

    const int S = Q, M = 7, L = 3;
    std::vector<float> normals((size_t)S * 3), path((size_t)S * (M + 1) * 3, NAN), rgb((size_t)S * 3, NAN), log((size_t)S * M * 14, NAN);
    std::vector<float> out((size_t)S * L * 3, NAN);
    std::vector<int32_t> steps(S, -1);
    for (int i = 0; i < S * 3; i++) normals[i] = rnd() - 0.5f;
    std::vector<int64_t> rorder(S);
    std::iota(rorder.begin(), rorder.end(), 0);
    std::reverse(rorder.begin(), rorder.end());
    ghrsim_field_trace(P, pts.data(), order.data(), dirs.data(), w.data(), col.data(), S, x.data(), normals.data(), rorder.data(), M, r2,
                       r / 2.5f, 0.5f, 0.05f, 2, path.data(), steps.data(), rgb.data(), log.data());
    ghrsim_strands_resample(S, M, L, path.data(), steps.data(), out.data());
    for (float f : path) KNN_CHECK(!std::isnan(f));
    for (float f : rgb) KNN_CHECK(!std::isnan(f));
    for (float f : out) KNN_CHECK(!std::isnan(f));
    int kept = 0;
    for (int32_t s : steps) {
        KNN_CHECK(s >= 0 && s <= M);
        kept += s > 0;
    }
    std::printf("P %d Q %d r %g: blocks scanned by the first wave %u, strands with support %d\n", P, Q, r, scanned[0], kept);
    return 1;
}

}  // namespace

int main()
{
    int done = 0;
    const int Ps[5] = {1, 63, 64, 65, 4097};
    for (int P : Ps) {
        done += run(P, 65, P < 100 ? 0.6f : 0.1f);
        done += run(P, 1, 4.0f);
    }
    std::printf("%d cases ok\n", done);
    return 0;
}
