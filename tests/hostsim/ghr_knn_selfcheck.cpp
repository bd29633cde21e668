// ghr_knn_selfcheck.cpp -- TEST SCAFFOLDING: the host walks of ghr_hostsim_knn.cpp as a program of its own, for a build with
// -fsanitize=address,undefined (tests/test_knn_cpu.py).  Every buffer has exactly the size the C ABI documents.
//
//   ghr_knn_selfcheck cases.bin
// cases.bin: per case  int32 Px Py norm | float32 x [Px 3] y [Py 3] | expected: float32 dist [Px], int32 idx [Px] (x -> y under
//   `norm`), float32 mean3 [Py] (distCUDA2 of y).  The program makes the keys (union bounds for the search, y's own for distCUDA2)
//   and their stable sorts itself and compares bits.
#include "ghr_hostsim_knn.cpp"

#include <algorithm>
#include <numeric>

namespace {

template <class T>
bool rd(std::FILE* f, std::vector<T>& v, size_t n)
{
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int fail_case(int k, const char* what)
{
    std::fprintf(stderr, "case %d: %s\n", k, what);
    return 1;
}

void grow(float* bounds, const std::vector<float>& p)
{
    for (size_t i = 0; i < p.size(); i++) {
        bounds[i % 3] = std::min(bounds[i % 3], p[i]);
        bounds[3 + i % 3] = std::max(bounds[3 + i % 3], p[i]);
    }
}

// keys over `bounds`, their stable sort: order, and the keys in that order
void key_sort(const std::vector<float>& p, const float* bounds, std::vector<int64_t>& order, std::vector<uint64_t>& sorted)
{
    const size_t P = p.size() / 3;
    std::vector<uint64_t> keys(P);
    ghrsim_knn_keys((int64_t)P, p.data(), bounds, keys.data());
    order.resize(P);
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return (int64_t)keys[a] < (int64_t)keys[b]; });
    sorted.resize(P);
    for (size_t i = 0; i < P; i++) sorted[i] = keys[order[i]];
}

bool same_bits(const std::vector<float>& a, const std::vector<float>& b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int k = 0;
    for (;; k++) {
        int32_t h[3];
        if (std::fread(h, sizeof(int32_t), 3, f) != 3) break;
        const size_t Px = h[0], Py = h[1];
        std::vector<float> x, y, want_dist, want_mean;
        std::vector<int32_t> want_idx;
        if (!rd(f, x, Px * 3) || !rd(f, y, Py * 3) || !rd(f, want_dist, Px) || !rd(f, want_idx, Px) || !rd(f, want_mean, Py))
            return fail_case(k, "short file");
        const float none[6] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
        float both[6], own[6];
        std::memcpy(both, none, sizeof(none));
        std::memcpy(own, none, sizeof(none));
        grow(both, x);
        grow(both, y);
        grow(own, y);
        std::vector<int64_t> ox, oy;
        std::vector<uint64_t> kx, ky;
        key_sort(x, both, ox, kx);
        key_sort(y, both, oy, ky);
        std::vector<float> dist(Px, NAN);
        std::vector<int32_t> idx(Px, -1);
        std::vector<uint32_t> scanned((Px + GHR_KNN_BLOCK - 1) / GHR_KNN_BLOCK, 0);
        ghrsim_nn_search((int64_t)Px, x.data(), ox.data(), kx.data(), (int64_t)Py, y.data(), oy.data(), ky.data(), h[2], dist.data(),
                         idx.data(), scanned.data());
        if (!same_bits(dist, want_dist)) return fail_case(k, "dist");
        if (idx != want_idx) return fail_case(k, "idx");
        for (uint32_t n : scanned)
            if (n < 1 || n > (Py + GHR_KNN_BLOCK - 1) / GHR_KNN_BLOCK) return fail_case(k, "blocks scanned by a wave");
        key_sort(y, own, oy, ky);
        std::vector<float> mean(Py, NAN);
        ghrsim_knn_mean_dist2((int64_t)Py, y.data(), oy.data(), mean.data(), nullptr);
        if (!same_bits(mean, want_mean)) return fail_case(k, "mean of the three nearest");
    }
    std::fclose(f);
    std::printf("%d cases ok\n", k);
    return 0;
}
