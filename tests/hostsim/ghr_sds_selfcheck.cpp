// ghr_sds_selfcheck.cpp -- TEST SCAFFOLDING: the host walks of ghr_hostsim_sds.cpp as a program of its own, for a build with
// -fsanitize=address,undefined (tests/test_strand_prior_cpu.py).  Every buffer has exactly the size the C ABI documents.
//
//   ghr_sds_selfcheck cases.bin
// cases.bin: per case  int32 S N n C G inverse | float32 scale tol | dirs [S n 3] frames [S 9] | int64 idx sorted_idx order [N] each |
//   float32 uvg [N 2] centres [G] z [N C] d_texture [C G G] d_e [N (n + 1) 3] | expected: int32 nbr [G G 4] start [N + 1]
//   list [4 G G] | float32 texture [C G G] e [N (n + 1) 3]
#include "ghr_hostsim_sds.cpp"

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
        int32_t h[6];
        if (std::fread(h, sizeof(int32_t), 6, f) != 6) break;
        const int S = h[0], N = h[1], n = h[2], C = h[3], G = h[4], inv = h[5], GG = G * G;
        float sc[2];
        if (std::fread(sc, sizeof(float), 2, f) != 2) return fail_case(k, "short file");
        std::vector<float> dirs, frames, uvg, centres, z, d_tex, d_e, want_tex, want_e;
        std::vector<int64_t> idx, sidx, order;
        std::vector<int32_t> want_nbr, want_start, want_list;
        const size_t ne = (size_t)N * (n + 1) * 3, nv = (size_t)N * n * 3;
        if (!rd(f, dirs, (size_t)S * n * 3) || !rd(f, frames, (size_t)S * 9) || !rd(f, idx, N) || !rd(f, sidx, N) || !rd(f, order, N) ||
            !rd(f, uvg, (size_t)N * 2) || !rd(f, centres, G) || !rd(f, z, (size_t)N * C) || !rd(f, d_tex, (size_t)C * GG) || !rd(f, d_e, ne) ||
            !rd(f, want_nbr, (size_t)GG * 4) || !rd(f, want_start, N + 1) || !rd(f, want_list, (size_t)GG * 4) ||
            !rd(f, want_tex, (size_t)C * GG) || !rd(f, want_e, ne))
            return fail_case(k, "short file");
        std::vector<float> e(ne, NAN), v(nv, NAN);
        ghrsim_sds_local(S, N, n, dirs.data(), frames.data(), inv, idx.data(), sc[0], e.data(), v.data());
        if (!close_all(e, want_e, sc[1])) return fail_case(k, "e");
        std::vector<int32_t> nbr((size_t)GG * 4, -1), count(N, -1), start(N + 1, -1), list((size_t)GG * 4, -1);
        std::vector<float> w((size_t)GG * 4, NAN), csim(N, NAN), alpha(N, NAN), alpha_q(GG, NAN), tex((size_t)C * GG, NAN);
        ghrsim_sds_texture(N, n, C, G, uvg.data(), centres.data(), z.data(), v.data(), nbr.data(), w.data(), csim.data(), alpha.data(),
                           alpha_q.data(), count.data(), start.data(), list.data(), tex.data());
        if (nbr != want_nbr) return fail_case(k, "nbr");
        if (start != want_start || list != want_list) return fail_case(k, "inverted lists");
        if (!close_all(tex, want_tex, sc[1])) return fail_case(k, "texture");
        std::vector<float> dalpha_q(GG, NAN), d_csim(N, NAN), d_z((size_t)N * C, NAN), d_v(nv, NAN), d_dirs((size_t)S * n * 3, 0.f);
        ghrsim_sds_texture_backward(N, n, C, G, z.data(), v.data(), nbr.data(), w.data(), csim.data(), alpha_q.data(), start.data(),
                                    list.data(), d_tex.data(), dalpha_q.data(), d_csim.data(), d_z.data(), d_v.data());
        ghrsim_sds_local_backward(S, N, n, frames.data(), inv, sidx.data(), order.data(), sc[0], d_e.data(), d_v.data(), d_dirs.data());
        for (float x : d_z) if (!std::isfinite(x)) return fail_case(k, "d_z");
        for (float x : d_v) if (!std::isfinite(x)) return fail_case(k, "d_v");
        for (float x : d_dirs) if (!std::isfinite(x)) return fail_case(k, "d_dirs");
    }
    std::fclose(f);
    std::printf("%d cases ok\n", k);
    return 0;
}
