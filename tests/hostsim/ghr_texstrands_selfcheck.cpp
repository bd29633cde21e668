// ghr_texstrands_selfcheck.cpp -- TEST SCAFFOLDING: the host walks of ghr_hostsim_texstrands.cpp as a program of its own, for a
// build with -fsanitize=address,undefined (tests/test_textured_strands_cpu.py).  Every buffer has exactly the size the C ABI
// documents.
//
//   ghr_texstrands_selfcheck cases.bin
// cases.bin: per case  int32 Smax S T C n list_len | float32 inv_scale tol | float32 texture [C T T] | int32 x0 y0 [Smax] each |
//   float32 fx fy [Smax] each | int32 start [T T + 1] list [list_len] | int64 idx [S] | float32 v [S n 3] frames [Smax 9]
//   origins [Smax 3] d_z [S C] d_p d_pl [S (n + 1) 3] each | expected: float32 z [S C] d_texture [C T T] p [S (n + 1) 3]
//   d_v [S n 3] | int32 pos [Smax]
#include "ghr_hostsim_texstrands.cpp"

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
        const int Smax = h[0], S = h[1], T = h[2], C = h[3], n = h[4], len = h[5];
        const size_t TT = (size_t)T * T, np = (size_t)S * (n + 1) * 3;
        float sc[2];
        if (std::fread(sc, sizeof(float), 2, f) != 2) return fail_case(k, "short file");
        std::vector<float> tex, fx, fy, v, frames, origins, d_z, d_p, d_pl, want_z, want_dt, want_p, want_dv;
        std::vector<int32_t> x0, y0, start, list, want_pos;
        std::vector<int64_t> idx;
        if (!rd(f, tex, C * TT) || !rd(f, x0, Smax) || !rd(f, y0, Smax) || !rd(f, fx, Smax) || !rd(f, fy, Smax) || !rd(f, start, TT + 1) ||
            !rd(f, list, len) || !rd(f, idx, S) || !rd(f, v, (size_t)S * n * 3) || !rd(f, frames, (size_t)Smax * 9) ||
            !rd(f, origins, (size_t)Smax * 3) || !rd(f, d_z, (size_t)S * C) || !rd(f, d_p, np) || !rd(f, d_pl, np) ||
            !rd(f, want_z, (size_t)S * C) || !rd(f, want_dt, C * TT) || !rd(f, want_p, np) || !rd(f, want_dv, (size_t)S * n * 3) ||
            !rd(f, want_pos, Smax))
            return fail_case(k, "short file");
        std::vector<float> z((size_t)S * C, NAN), dt(C * TT, NAN), p(np, NAN), pl(np, NAN), dv((size_t)S * n * 3, NAN);
        std::vector<int32_t> pos(Smax, -7);
        ghrsim_ts_fetch(Smax, S, T, C, tex.data(), x0.data(), y0.data(), fx.data(), fy.data(), idx.data(), z.data());
        if (!close_all(z, want_z, sc[1])) return fail_case(k, "z");
        ghrsim_ts_fetch_backward(Smax, S, T, C, fx.data(), fy.data(), start.data(), list.data(), len, idx.data(), d_z.data(), pos.data(),
                                 dt.data());
        if (pos != want_pos) return fail_case(k, "pos");
        if (!close_all(dt, want_dt, sc[1])) return fail_case(k, "d_texture");
        ghrsim_ts_world(Smax, S, n, v.data(), frames.data(), origins.data(), idx.data(), sc[0], p.data(), pl.data());
        if (!close_all(p, want_p, sc[1])) return fail_case(k, "p");
        for (float x : pl) if (!std::isfinite(x)) return fail_case(k, "p_local");
        ghrsim_ts_world(Smax, S, n, v.data(), frames.data(), origins.data(), idx.data(), sc[0], p.data(), nullptr);
        ghrsim_ts_world_backward(Smax, S, n, frames.data(), idx.data(), sc[0], d_p.data(), d_pl.data(), dv.data());
        if (!close_all(dv, want_dv, sc[1])) return fail_case(k, "d_v");
        ghrsim_ts_world_backward(Smax, S, n, frames.data(), idx.data(), sc[0], d_p.data(), nullptr, dv.data());
        ghrsim_ts_world_backward(Smax, S, n, frames.data(), idx.data(), sc[0], nullptr, d_pl.data(), dv.data());
        for (float x : dv) if (!std::isfinite(x)) return fail_case(k, "d_v from d_p_local alone");
    }
    std::fclose(f);
    std::printf("%d cases ok\n", k);
    return 0;
}
