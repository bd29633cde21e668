// ghr_capture_selfcheck.cpp -- TEST SCAFFOLDING: a stand-alone program around ghr_hostsim_capture.cpp, for a sanitizer build
// (-fsanitize=address,undefined) of the per-pixel functions of csrc/ghr_capture.h.
//
//   ghr_capture_selfcheck CASES
// CASES holds the table [180][2] f32 once and then, per case, six int32 {S, L, H, W, s, F}, fourteen float32 {Ms[12], near,
// var_floor}, points [S][L][3] f32, pix_to_segment and pix_to_face_out [s H][s W] i32, and the expected mask_hair, mask_body,
// angle [H][W] u8 and var [H][W] f32 (written by tests/test_capture_cpu.py from the numpy model).  Every buffer is allocated at its
// exact size so that an access past it is an error the sanitizer sees.  Exit status 0: every case matched in both walks.
#include "ghr_hostsim_capture.cpp"

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
    std::vector<float> table;
    if (!take(fp, table, 2 * GHR_CAP_BINS)) { std::fprintf(stderr, "truncated table\n"); return 2; }
    int n_cases = 0;
    for (;;) {
        int32_t hd[6];
        float fl[14];
        const size_t got = std::fread(hd, sizeof(int32_t), 6, fp);
        if (got == 0) break;
        if (got != 6 || std::fread(fl, sizeof(float), 14, fp) != 14) { std::fprintf(stderr, "truncated case header\n"); return 2; }
        const size_t S = hd[0], L = hd[1], HW = (size_t)hd[2] * hd[3], big = HW * hd[4] * hd[4];
        std::vector<float> points, want_var;
        std::vector<int32_t> seg, face;
        std::vector<uint8_t> want_hair, want_body, want_angle;
        if (!take(fp, points, 3 * S * L) || !take(fp, seg, big) || !take(fp, face, big) || !take(fp, want_hair, HW) ||
            !take(fp, want_body, HW) || !take(fp, want_angle, HW) || !take(fp, want_var, HW)) {
            std::fprintf(stderr, "case %d: truncated\n", n_cases);
            return 2;
        }
        for (int walk = 0; walk < 2; walk++) {
            std::vector<uint8_t> hair(HW, 7), body(HW, 7), angle(HW, 7);
            std::vector<float> var(HW, 7.f);
            ghrsim_capture((int)S, (int)L, points.data(), fl, fl[12], hd[2], hd[3], hd[4], hd[5], seg.data(), face.data(), table.data(),
                           fl[13], hair.data(), body.data(), angle.data(), var.data(), walk);
            const bool ok = hair == want_hair && body == want_body && angle == want_angle &&
                            std::memcmp(var.data(), want_var.data(), 4 * HW) == 0;
            if (!ok) { std::fprintf(stderr, "case %d, walk %d: differs from the model\n", n_cases, walk); return 1; }
        }
        n_cases++;
    }
    std::fclose(fp);
    std::printf("ghr_capture_selfcheck: %d cases ok\n", n_cases);
    return n_cases > 0 ? 0 : 2;
}
