// ghr_guides_selfcheck.cpp -- TEST SCAFFOLDING: the host walks of ghr_hostsim_guides.cpp as a program of its own, for a build with
// -fsanitize=address,undefined (tests/test_guides_cpu.py).  Every buffer has exactly the size the C ABI documents.
//
//   ghr_guides_selfcheck cases.bin
// cases.bin: per case  int32 S N n C | float32 tol | float32 uvs [S 2] z_g [N C] v_g [N n 3] d_z [S C] | expected: int32
//   nbr [S 4] start [N + 1] list [4 S] | float32 z [S C] d_zg [N C]
#include "ghr_hostsim_guides.cpp"

#include <cmath>

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

bool close_all(const std::vector<float>& a, const std::vector<float>& b, float tol)
{
    for (size_t i = 0; i < a.size(); i++)
        if (!(std::fabs(a[i] - b[i]) <= tol)) return false;
    return a.size() == b.size();
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int k = 0;
    for (;; k++) {
        int32_t h[4];
        if (std::fread(h, sizeof(int32_t), 4, f) != 4) break;
        const int S = h[0], N = h[1], n = h[2], C = h[3];
        float tol;
        if (std::fread(&tol, sizeof(float), 1, f) != 1) return fail_case(k, "short file");
        std::vector<float> uvs, z_g, v_g, d_z, want_z, want_dzg;
        std::vector<int32_t> want_nbr, want_start, want_list;
        const size_t nv = (size_t)N * n * 3;
        if (!rd(f, uvs, (size_t)S * 2) || !rd(f, z_g, (size_t)N * C) || !rd(f, v_g, nv) || !rd(f, d_z, (size_t)S * C) ||
            !rd(f, want_nbr, (size_t)S * 4) || !rd(f, want_start, N + 1) || !rd(f, want_list, (size_t)S * 4) ||
            !rd(f, want_z, (size_t)S * C) || !rd(f, want_dzg, (size_t)N * C))
            return fail_case(k, "short file");
        std::vector<int32_t> nbr((size_t)S * 4, -1), count(N, -1), start(N + 1, -1), unsorted((size_t)S * 4, -1), list((size_t)S * 4, -1);
        std::vector<float> w((size_t)S * 4, NAN), csim(N, NAN), alpha(N, NAN), alpha_s(S, NAN), z((size_t)S * C, NAN);
        ghrsim_gd_blend(S, N, n, C, uvs.data(), z_g.data(), v_g.data(), nbr.data(), w.data(), csim.data(), alpha.data(), alpha_s.data(),
                        count.data(), start.data(), unsorted.data(), list.data(), z.data());
        if (nbr != want_nbr) return fail_case(k, "nbr");
        if (start != want_start || list != want_list) return fail_case(k, "inverted lists");
        if (!close_all(z, want_z, tol)) return fail_case(k, "z");
        std::vector<float> dalpha_s(S, NAN), d_csim(N, NAN), d_zg((size_t)N * C, NAN), d_vg(nv, NAN);
        ghrsim_gd_blend_backward(S, N, n, C, z_g.data(), v_g.data(), nbr.data(), w.data(), csim.data(), alpha_s.data(), start.data(),
                                 list.data(), d_z.data(), dalpha_s.data(), d_csim.data(), d_zg.data(), d_vg.data());
        if (!close_all(d_zg, want_dzg, tol)) return fail_case(k, "d_zg");
        for (float x : d_vg) if (!std::isfinite(x)) return fail_case(k, "d_vg");
    }
    std::fclose(f);
    std::printf("%d cases ok\n", k);
    return 0;
}
