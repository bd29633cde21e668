// ghr_upsample_selfcheck.cpp -- TEST SCAFFOLDING: a stand-alone program over ghr_hostsim_upsample.cpp's walks of
// csrc/ghr_upsample.h, built plain and with -fsanitize=address,undefined by tests/test_strand_upsampling_cpu.py.  Three planted
// cases through the two loops, every buffer sized exactly so that an access outside it is caught.
#include "ghr_hostsim_upsample.cpp"

#include <cmath>

namespace {

unsigned g_seed = 2468u;
float rnd() { g_seed = g_seed * 1664525u + 1013904223u; return (float)(g_seed >> 8) / (float)(1u << 24); }

// a rotation about z by `a`, then about x by `b`: orthonormal up to rounding
void frame(float a, float b, float* M)
{
    const float ca = std::cos(a), sa = std::sin(a), cb = std::cos(b), sb = std::sin(b);
    const float R[9] = {ca, -sa, 0.f, cb * sa, cb * ca, -sb, sb * sa, sb * ca, cb};
    std::memcpy(M, R, sizeof(R));
}

bool run(const char* name, int G, int L, int N, int F, float r2, int gate, bool foreign)
{
    std::vector<float> gp((size_t)G * L * 3), gM((size_t)G * 9), gf((size_t)G * F), co((size_t)N * 3), cM((size_t)N * 9);
    for (int g = 0; g < G; g++) {
        frame(6.f * rnd(), 3.f * rnd(), &gM[(size_t)9 * g]);
        float p[3] = {(float)(g % 4), (float)((g / 4) % 4), (float)(g / 16)};  // roots on an integer lattice
        for (int j = 0; j < L; j++) {
            for (int x = 0; x < 3; x++) gp[((size_t)g * L + j) * 3 + x] = p[x];
            if (g != 1)  // guide 1 has zero length
                for (int x = 0; x < 3; x++) p[x] += 0.05f * (rnd() - 0.3f);
        }
    }
    for (size_t i = 0; i < gf.size(); i++) gf[i] = rnd();
    for (int c = 0; c < N; c++) {
        frame(6.f * rnd(), 3.f * rnd(), &cM[(size_t)9 * c]);
        for (int x = 0; x < 3; x++) co[(size_t)3 * c + x] = c == 0 ? 0.f : (c == 1 ? 50.f : (float)(int)(4.f * rnd()) + (c % 2 ? 0.5f : 0.f));
    }
    std::vector<int32_t> nbr((size_t)N * 4, -7);
    std::vector<float> nd2((size_t)N * 4, NAN);
    ghrsim_ups_near(G, gp.data(), 0, co.data(), r2, nbr.data(), nd2.data());  // N == 0: nothing is read or written
    if (N > 0 && nbr[0] != -7) return false;
    std::vector<float> groots((size_t)G * 3);
    for (int g = 0; g < G; g++)
        for (int x = 0; x < 3; x++) groots[(size_t)3 * g + x] = gp[(size_t)g * L * 3 + x];
    ghrsim_ups_near(G, groots.data(), N, co.data(), r2, nbr.data(), nd2.data());
    for (int c = 0; c < N; c++)
        for (int k = 0; k < 4; k++) {
            const int32_t x = nbr[(size_t)4 * c + k];
            const float d = nd2[(size_t)4 * c + k];
            if (!(x == -1 ? std::isinf(d) : (x >= 0 && x < G && d <= r2))) { std::printf("%s: nbr[%d][%d] = %d, %g\n", name, c, k, x, d); return false; }
            if (k > 0 && !(nd2[(size_t)4 * c + k - 1] <= d)) { std::printf("%s: distances not ascending\n", name); return false; }
        }
    if (foreign && N > 2) {  // entries outside [0, G) end a child's list and are never dereferenced
        nbr[4 * 2 + 1] = G;
        nbr[4 * 2 + 2] = 0;
        if (N > 3) nbr[4 * 3] = -5;
    }
    std::vector<float> out((size_t)N * L * 3, NAN), w((size_t)N * 4, NAN), of((size_t)N * F, NAN), again(out.size());
    std::vector<uint8_t> valid((size_t)N, 7);
    float* gfp = F ? gf.data() : nullptr;
    float* ofp = F ? of.data() : nullptr;
    ghrsim_ups_blend(G, L, gp.data(), gM.data(), gfp, F, N, co.data(), cM.data(), nbr.data(), nd2.data(), 1e-6f, 0.5f, gate, out.data(),
                     w.data(), ofp, valid.data());
    ghrsim_ups_blend(G, L, gp.data(), gM.data(), gfp, F, N, co.data(), cM.data(), nbr.data(), nd2.data(), 1e-6f, 0.5f, gate, again.data(),
                     w.data(), ofp, valid.data());
    if (std::memcmp(out.data(), again.data(), out.size() * 4) != 0) return false;
    int nvalid = 0;
    for (int c = 0; c < N; c++) {
        if (valid[(size_t)c] > 1) return false;
        nvalid += valid[(size_t)c];
        float sum = 0.f;
        for (int k = 0; k < 4; k++) {
            const float x = w[(size_t)4 * c + k];
            if (!(x >= 0.f && x <= 1.f)) { std::printf("%s: w[%d][%d] = %g\n", name, c, k, x); return false; }
            sum += x;
        }
        if (std::fabs(sum - (valid[(size_t)c] ? 1.f : 0.f)) > 1e-5f) { std::printf("%s: the weights of child %d sum to %g\n", name, c, sum); return false; }
        if (std::memcmp(&out[(size_t)c * L * 3], &co[(size_t)3 * c], 12) != 0) { std::printf("%s: point 0 of child %d is not its origin\n", name, c); return false; }
    }
    if (foreign && N > 3 && valid[3] != 0) return false;
    if (foreign && N > 2 && !(w[4 * 2 + 1] == 0.f && w[4 * 2 + 2] == 0.f)) return false;
    for (float x : out)
        if (!std::isfinite(x)) { std::printf("%s: a point is not finite\n", name); return false; }
    for (float x : of)
        if (!std::isfinite(x)) { std::printf("%s: a feature is not finite\n", name); return false; }
    std::printf("%s: G %d L %d N %d F %d valid %d\n", name, G, L, N, F, nvalid);
    return true;
}

}  // namespace

int main()
{
    int ok = 0;
    ok += run("lattice-cut", 20, 65, 9, 3, 2.f, 1, false);
    ok += run("tile-edge", 257, 2, 70, 0, INFINITY, 0, false);
    ok += run("foreign-entries", 5, 130, 6, 1, INFINITY, 1, true);
    std::printf("%d cases ok\n", ok);
    return ok == 3 ? 0 : 1;
}
