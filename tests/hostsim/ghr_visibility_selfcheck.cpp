// ghr_visibility_selfcheck.cpp -- TEST SCAFFOLDING: a stand-alone program around ghr_hostsim_visibility.cpp, for a sanitizer
// build (-fsanitize=address,undefined) of the per-element functions and the table walk of csrc/ghr_visibility.h.
//
//   ghr_visibility_selfcheck CASES
// CASES holds, per case, five int32 {V, F, H, W, has_masks}, thirteen float32 {M[12], near} and then vertices [V][3] f32,
// faces [F][3] i32, (body, hair [H][W] u8 when has_masks), and the expected pix_to_face [H][W] i32, vis [H][W] u8, seen [V] u8,
// seen_head [V] u8 and head [H][W] u8 (written by tests/test_visibility_cpu.py from the numpy model).
// Every buffer is allocated at its exact size so that an access past it is an error the sanitizer sees.
// Exit status 0: every case matched.
#include "ghr_hostsim_visibility.cpp"

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
        float mn[13];
        const size_t got = std::fread(hd, sizeof(int32_t), 5, fp);
        if (got == 0) break;
        if (got != 5 || std::fread(mn, sizeof(float), 13, fp) != 13) { std::fprintf(stderr, "truncated case header\n"); return 2; }
        const size_t V = hd[0], F = hd[1], HW = (size_t)hd[2] * hd[3], nm = hd[4] ? HW : 0;
        std::vector<float> v;
        std::vector<int32_t> f, want_pix;
        std::vector<uint8_t> body, hair, want_vis, want_seen, want_seen_head, want_head;
        if (!take(fp, v, 3 * V) || !take(fp, f, 3 * F) || !take(fp, body, nm) || !take(fp, hair, nm) || !take(fp, want_pix, HW) ||
            !take(fp, want_vis, HW) || !take(fp, want_seen, V) || !take(fp, want_seen_head, V) || !take(fp, want_head, HW)) {
            std::fprintf(stderr, "case %d: truncated\n", n_cases);
            return 2;
        }
        std::vector<int32_t> pix(HW, 7), cnt(V, 0), cnt_head(V, 0);
        std::vector<uint8_t> vis(HW, 7), head(HW, 7);
        if (ghrsim_vis_view((int)V, v.data(), (int)F, f.data(), mn, mn[12], hd[2], hd[3], hd[4] ? body.data() : nullptr,
                            hd[4] ? hair.data() : nullptr, pix.data(), vis.data(), cnt.data(), cnt_head.data(), nullptr)) {
            std::fprintf(stderr, "case %d: the layout refused the sizes\n", n_cases);
            return 1;
        }
        bool ok = pix == want_pix && vis == want_vis;
        for (size_t k = 0; k < V; k++) ok = ok && cnt[k] == want_seen[k] && cnt_head[k] == want_seen_head[k];
        if (hd[4]) {
            ghrsim_vis_head_mask(hd[2], hd[3], body.data(), hair.data(), head.data());
            ok = ok && head == want_head;
        }
        if (!ok) { std::fprintf(stderr, "case %d: differs from the model\n", n_cases); return 1; }
        n_cases++;
    }
    std::fclose(fp);
    std::printf("ghr_visibility_selfcheck: %d cases ok\n", n_cases);
    return n_cases > 0 ? 0 : 2;
}
