// ghr_strandview_selfcheck.cpp -- TEST SCAFFOLDING: a stand-alone program around ghr_hostsim_strandview.cpp, for a sanitizer
// build (-fsanitize=address,undefined) of the per-element functions and the table walk of csrc/ghr_strandview.h.
//
//   ghr_strandview_selfcheck CASES
// CASES holds, per case, ten int32 {S, L, H, W, V, F, has_mesh, mode, has_base, s}, fifteen float32 {M[12], near, r, head_bias},
// the bytes of a ghr::SvShading, and then points [S][L][3] f32, (vertices [V][3] f32, faces [F][3] i32, pix_to_face [H][W] i32 when
// has_mesh), (base [S][3] f32 when has_base), and the expected pix_to_segment i32, t f32, pix_to_face_out i32, inv_depth f32
// (each [H][W]), rgb [H][W][3] u8 and the resolved [H / s][W / s][3] u8 (written by tests/test_strand_view_cpu.py from the numpy
// model; H, W are the raster's size, s times the picture's).  Every buffer is allocated at its exact size so that an access
// past it is an error the sanitizer sees.  Exit status 0: every case matched.
#include "ghr_hostsim_strandview.cpp"

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
        int32_t hd[10];
        float fl[15];
        ghr::SvShading sh;
        const size_t got = std::fread(hd, sizeof(int32_t), 10, fp);
        if (got == 0) break;
        if (got != 10 || std::fread(fl, sizeof(float), 15, fp) != 15 || std::fread(&sh, sizeof(sh), 1, fp) != 1) {
            std::fprintf(stderr, "truncated case header\n");
            return 2;
        }
        const size_t S = hd[0], L = hd[1], V = hd[4], F = hd[5], HW = (size_t)hd[2] * hd[3];
        const bool mesh = hd[6] != 0, has_base = hd[8] != 0;
        const int s = hd[9], h = hd[2] / s, w = hd[3] / s;
        std::vector<float> points, vertices, base, want_t, want_inv;
        std::vector<int32_t> faces, pix, want_seg, want_face;
        std::vector<uint8_t> want_rgb, want_small;
        if (!take(fp, points, 3 * S * L) || !take(fp, vertices, mesh ? 3 * V : 0) || !take(fp, faces, mesh ? 3 * F : 0) ||
            !take(fp, pix, mesh ? HW : 0) || !take(fp, base, has_base ? 3 * S : 0) || !take(fp, want_seg, HW) || !take(fp, want_t, HW) ||
            !take(fp, want_face, HW) || !take(fp, want_inv, HW) || !take(fp, want_rgb, 3 * HW) || !take(fp, want_small, 3 * (size_t)h * w)) {
            std::fprintf(stderr, "case %d: truncated\n", n_cases);
            return 2;
        }
        std::vector<float> qf(mesh ? HW : 0, 7.f), t(HW, 7.f), inv(HW, 7.f);
        std::vector<int32_t> seg(HW, 7), face(HW, 7);
        std::vector<uint8_t> rgb(3 * HW, 7), small(3 * (size_t)h * w, 7);
        if (mesh) ghrsim_sv_face_depth((int)V, vertices.data(), (int)F, faces.data(), fl, fl[12], hd[2], hd[3], pix.data(), qf.data());
        if (ghrsim_sv_raster((int)S, (int)L, points.data(), fl, fl[12], hd[2], hd[3], fl[13], fl[14], mesh ? pix.data() : nullptr,
                             mesh ? qf.data() : nullptr, seg.data(), t.data(), face.data(), inv.data(), nullptr, nullptr)) {
            std::fprintf(stderr, "case %d: the layout refused the sizes\n", n_cases);
            return 1;
        }
        ghrsim_sv_shade((int)S, (int)L, points.data(), mesh ? (int)V : 0, vertices.data(), mesh ? (int)F : 0, faces.data(), hd[2], hd[3],
                        seg.data(), face.data(), hd[7], &sh, has_base ? base.data() : nullptr, rgb.data());
        ghrsim_sv_resolve(h, w, s, rgb.data(), small.data());
        const bool ok = seg == want_seg && face == want_face && rgb == want_rgb && small == want_small &&
                        std::memcmp(t.data(), want_t.data(), 4 * HW) == 0 && std::memcmp(inv.data(), want_inv.data(), 4 * HW) == 0;
        if (!ok) { std::fprintf(stderr, "case %d: differs from the model\n", n_cases); return 1; }
        n_cases++;
    }
    std::fclose(fp);
    std::printf("ghr_strandview_selfcheck: %d cases ok\n", n_cases);
    return n_cases > 0 ? 0 : 2;
}
