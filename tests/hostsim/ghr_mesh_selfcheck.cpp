// ghr_mesh_selfcheck.cpp -- TEST SCAFFOLDING: a stand-alone program around ghr_hostsim_mesh.cpp, for a sanitizer build
// (-fsanitize=address,undefined) of the grid builder and the per-element functions of csrc/ghr_mesh.h.
//
//   ghr_mesh_selfcheck CASES
// CASES holds, per case, five int32 {nv, nf, G, nq, np} and then vertices [nv][3] f32, faces [nf][3] i32, queries [nq][3] f32,
// expected inside [nq] u8, expected crossings [nq][3] u32, Gaussians xyz [np][3] / scaling [np][3] / rotation [np][4] f32 and
// the expected probe results [np] u8 for probe modes 0 and 1 (written by tests/test_mesh_cpu.py from the numpy model).
// Every buffer is allocated at its exact size so that an access past it is an error the sanitizer sees.
// Exit status 0: every case built, verified and matched.
#include "ghr_hostsim_mesh.cpp"

#include <vector>

namespace {
template <class T>
bool take(std::FILE* fp, std::vector<T>& out, size_t n)
{
    out.resize(n);
    return n == 0 || std::fread(out.data(), sizeof(T), n, fp) == n;
}
}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    std::FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) { std::perror(argv[1]); return 2; }
    int n_cases = 0;
    for (;;) {
        int32_t hd[5];
        const size_t got = std::fread(hd, sizeof(int32_t), 5, fp);
        if (got == 0) break;
        if (got != 5) { std::fprintf(stderr, "truncated case header\n"); return 2; }
        const size_t nv = hd[0], nf = hd[1], nq = hd[3], np = hd[4];
        std::vector<float> v, q, xyz, s, rot;
        std::vector<int32_t> f;
        std::vector<uint8_t> want_in, want_o0, want_o1;
        std::vector<uint32_t> want_c;
        if (!take(fp, v, 3 * nv) || !take(fp, f, 3 * nf) || !take(fp, q, 3 * nq) || !take(fp, want_in, nq) || !take(fp, want_c, 3 * nq) ||
            !take(fp, xyz, 3 * np) || !take(fp, s, 3 * np) || !take(fp, rot, 4 * np) || !take(fp, want_o0, np) || !take(fp, want_o1, np)) {
            std::fprintf(stderr, "case %d: truncated\n", n_cases);
            return 2;
        }
        ghr::MeshGrid h;
        char why[128] = "";
        if (ghrsim_mesh_sizes((int)nv, v.data(), (int)nf, f.data(), hd[2], &h, why)) { std::fprintf(stderr, "case %d: %s\n", n_cases, why); return 1; }
        float* blob = new float[(size_t)h.bytes / 4];  // (new[] of float: 16-B aligned, exact size)
        if (ghrsim_mesh_build((int)nv, v.data(), (int)nf, f.data(), hd[2], blob, h.bytes, why)) { std::fprintf(stderr, "case %d: %s\n", n_cases, why); return 1; }
        if (int line = ghrsim_mesh_verify(v.data(), f.data(), blob)) { std::fprintf(stderr, "case %d: verify failed at line %d\n", n_cases, line); return 1; }
        std::vector<uint8_t> in(nq), o(np);
        std::vector<uint32_t> c(3 * nq);
        ghrsim_mesh_contains(blob, (long long)nq, q.data(), in.data(), c.data());
        if (in != want_in || c != want_c) { std::fprintf(stderr, "case %d: contains differs from the model\n", n_cases); return 1; }
        for (int mode = 0; mode < 2; mode++) {
            ghrsim_mesh_probes_outside(blob, (long long)np, xyz.data(), s.data(), rot.data(), mode, o.data());
            if (o != (mode ? want_o1 : want_o0)) { std::fprintf(stderr, "case %d: probe mode %d differs from the model\n", n_cases, mode); return 1; }
        }
        delete[] blob;
        n_cases++;
    }
    std::fclose(fp);
    std::printf("ghr_mesh_selfcheck: %d cases ok\n", n_cases);
    return n_cases > 0 ? 0 : 2;
}
