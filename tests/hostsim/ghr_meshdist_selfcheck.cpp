// ghr_meshdist_selfcheck.cpp -- TEST SCAFFOLDING: a stand-alone program around ghr_hostsim_meshdist.cpp, for a sanitizer build
// (-fsanitize=address,undefined) of the triangle-blob builder, the per-element functions and the wave walk of
// csrc/ghr_meshdist.h.
//
//   ghr_meshdist_selfcheck CASES
// CASES holds, per case, three int32 {nv, nf, nq} and then vertices [nv][3] f32, faces [nf][3] i32, queries [nq][3] f32 and the
// expected dist2 [nq] f32, face [nq] i32, point [nq][3] f32 (written by tests/test_mesh_distance_cpu.py from the numpy model;
// the non-finite queries ride along).  Every buffer is allocated at its exact size so that an access past it is an error the
// sanitizer sees.  Floats are compared as bits.  Exit status 0: every case built, verified and matched.
#include "ghr_hostsim_meshdist.cpp"

namespace {
template <class T>
bool take(std::FILE* fp, std::vector<T>& out, size_t n)
{
    out.resize(n);
    return n == 0 || std::fread(out.data(), sizeof(T), n, fp) == n;
}

template <class T>
bool same_bits(const std::vector<T>& a, const std::vector<T>& b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(T) * a.size()) == 0);
}
}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    std::FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) { std::perror(argv[1]); return 2; }
    int n_cases = 0;
    for (;;) {
        int32_t hd[3];
        const size_t got = std::fread(hd, sizeof(int32_t), 3, fp);
        if (got == 0) break;
        if (got != 3) { std::fprintf(stderr, "truncated case header\n"); return 2; }
        const size_t nv = hd[0], nf = hd[1], nq = hd[2];
        std::vector<float> v, q, want_d, want_p;
        std::vector<int32_t> f, want_f;
        if (!take(fp, v, 3 * nv) || !take(fp, f, 3 * nf) || !take(fp, q, 3 * nq) || !take(fp, want_d, nq) || !take(fp, want_f, nq) ||
            !take(fp, want_p, 3 * nq)) {
            std::fprintf(stderr, "case %d: truncated\n", n_cases);
            return 2;
        }
        ghr::MeshTris h;
        char why[128] = "";
        if (ghrsim_md_sizes((int)nv, v.data(), (int)nf, f.data(), &h, why)) { std::fprintf(stderr, "case %d: %s\n", n_cases, why); return 1; }
        float* blob = new float[(size_t)h.bytes / 4];  // (new[] of float: 16-B aligned, exact size)
        if (ghrsim_md_build((int)nv, v.data(), (int)nf, f.data(), blob, h.bytes, why)) { std::fprintf(stderr, "case %d: %s\n", n_cases, why); return 1; }
        if (int line = ghrsim_md_verify(v.data(), f.data(), blob)) { std::fprintf(stderr, "case %d: verify failed at line %d\n", n_cases, line); return 1; }
        std::vector<float> d(nq), p(3 * nq), g(nq, 1.f), grad(3 * nq);
        std::vector<int32_t> face(nq);
        std::vector<uint8_t> inside(nq, 0);
        ghrsim_md_closest(blob, (int64_t)nq, q.data(), nullptr, nullptr, d.data(), face.data(), p.data(), nullptr);
        if (!same_bits(d, want_d) || !same_bits(face, want_f) || !same_bits(p, want_p)) {
            std::fprintf(stderr, "case %d: closest differs from the model\n", n_cases);
            return 1;
        }
        ghrsim_md_backward((int64_t)nq, q.data(), p.data(), d.data(), inside.data(), g.data(), grad.data());
        for (size_t i = 0; i < 3 * nq; i++)
            if (!(fabsf(grad[i]) <= FLT_MAX)) { std::fprintf(stderr, "case %d: gradient %zu is not finite\n", n_cases, i); return 1; }
        delete[] blob;
        n_cases++;
    }
    std::fclose(fp);
    std::printf("ghr_meshdist_selfcheck: %d cases ok\n", n_cases);
    return n_cases > 0 ? 0 : 2;
}
