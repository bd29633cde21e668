// ghr_strandshadow_selfcheck.cpp -- TEST SCAFFOLDING: a stand-alone program around ghr_hostsim_strandshadow.cpp, for a sanitizer
// build (-fsanitize=address,undefined) of the self-shadowing functions and the two-walk light pass of csrc/ghr_strandview.h.
//
//   ghr_strandshadow_selfcheck CASES
// CASES is a sequence of records, each led by one int32 kind (written by tests/test_strand_shadow_cpu.py from the numpy model):
//   kind 1, a light map: four int32 {S, L, Hl, Wl}, fifteen float32 {Ml[12], near, rl, layer}, points [S][L][3] f32, and the
//       expected q0 [Hl][Wl] f32 and layers [Hl][Wl][4] u32;
//   kind 2, a shadowed frame: twelve int32 {S, L, H, W, V, F, has_mesh, mode, has_base, Hl, Wl, has_qfl}, sixteen float32
//       {Ml[12], near, layer, kappa, bias}, the bytes of a ghr::SvShading, points, (vertices [V][3] f32, faces [F][3] i32 when
//       has_mesh), (base [S][3] f32 when has_base), pix_to_segment i32, pix_to_face_out i32 and t f32 (each [H][W]), q0, layers,
//       (qfl [Hl][Wl] f32 when has_qfl), and the expected rgb [H][W][3] u8.
// Every buffer is allocated at its exact size so that an access past it is an error the sanitizer sees.  Exit status 0: every
// record matched.
#include "ghr_hostsim_strandshadow.cpp"

namespace {
template <class T>
bool take(std::FILE* fp, std::vector<T>& out, size_t n)
{
    out.resize(n);
    return n == 0 || std::fread(out.data(), sizeof(T), n, fp) == n;
}

int fail(int n, const char* why)
{
    std::fprintf(stderr, "record %d: %s\n", n, why);
    return 1;
}
}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    std::FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) { std::perror(argv[1]); return 2; }
    int n_maps = 0, n_frames = 0;
    for (;;) {
        int32_t kind;
        if (std::fread(&kind, sizeof(kind), 1, fp) != 1) break;
        const int n = n_maps + n_frames;
        if (kind == 1) {
            int32_t hd[4];
            float fl[15];
            if (std::fread(hd, sizeof(int32_t), 4, fp) != 4 || std::fread(fl, sizeof(float), 15, fp) != 15) return fail(n, "truncated header");
            const size_t S = hd[0], L = hd[1], HW = (size_t)hd[2] * hd[3];
            std::vector<float> points, want_q0;
            std::vector<uint32_t> want_layers;
            if (!take(fp, points, 3 * S * L) || !take(fp, want_q0, HW) || !take(fp, want_layers, 4 * HW)) return fail(n, "truncated");
            std::vector<float> q0(HW, 7.f);
            std::vector<uint32_t> layers(4 * HW, 7u);
            if (ghrsim_ss_opacity((int)S, (int)L, points.data(), fl, fl[12], hd[2], hd[3], fl[13], fl[14], q0.data(), layers.data(), nullptr,
                                  nullptr))
                return fail(n, "the layout refused the sizes");
            if (layers != want_layers || std::memcmp(q0.data(), want_q0.data(), 4 * HW) != 0) return fail(n, "the map differs from the model");
            n_maps++;
        } else if (kind == 2) {
            int32_t hd[12];
            float fl[16];
            ghr::SvShading sh;
            if (std::fread(hd, sizeof(int32_t), 12, fp) != 12 || std::fread(fl, sizeof(float), 16, fp) != 16 ||
                std::fread(&sh, sizeof(sh), 1, fp) != 1)
                return fail(n, "truncated header");
            const size_t S = hd[0], L = hd[1], HW = (size_t)hd[2] * hd[3], V = hd[4], F = hd[5], LHW = (size_t)hd[9] * hd[10];
            const bool mesh = hd[6] != 0, has_base = hd[8] != 0, has_qfl = hd[11] != 0;
            std::vector<float> points, vertices, base, t, q0, qfl;
            std::vector<int32_t> faces, seg, face;
            std::vector<uint32_t> layers;
            std::vector<uint8_t> want_rgb;
            if (!take(fp, points, 3 * S * L) || !take(fp, vertices, mesh ? 3 * V : 0) || !take(fp, faces, mesh ? 3 * F : 0) ||
                !take(fp, base, has_base ? 3 * S : 0) || !take(fp, seg, HW) || !take(fp, face, HW) || !take(fp, t, HW) ||
                !take(fp, q0, LHW) || !take(fp, layers, 4 * LHW) || !take(fp, qfl, has_qfl ? LHW : 0) || !take(fp, want_rgb, 3 * HW))
                return fail(n, "truncated");
            std::vector<uint8_t> rgb(3 * HW, 7);
            ghrsim_ss_shade((int)S, (int)L, points.data(), mesh ? (int)V : 0, vertices.data(), mesh ? (int)F : 0, faces.data(), hd[2],
                            hd[3], seg.data(), face.data(), t.data(), hd[7], &sh, has_base ? base.data() : nullptr, fl, fl[12], hd[9],
                            hd[10], fl[13], fl[14], fl[15], q0.data(), layers.data(), has_qfl ? qfl.data() : nullptr, rgb.data());
            if (rgb != want_rgb) return fail(n, "the bytes differ from the model");
            n_frames++;
        } else {
            return fail(n, "unknown kind");
        }
    }
    std::fclose(fp);
    std::printf("ghr_strandshadow_selfcheck: %d maps and %d frames ok\n", n_maps, n_frames);
    return n_maps + n_frames > 0 ? 0 : 2;
}
