// ghr_shape_selfcheck.cpp -- TEST SCAFFOLDING: a stand-alone program over ghr_hostsim_shape.cpp's walks of csrc/ghr_shape.h, built
// plain and with -fsanitize=address,undefined by tests/test_strand_shape_cpu.py.  Two planted cases through the three loops
// (neighbours, forward, backward), every buffer sized exactly so that an access outside it is caught.
#include "ghr_hostsim_shape.cpp"

#include <cmath>

namespace {

unsigned g_seed = 12345u;
float rnd() { g_seed = g_seed * 1664525u + 1013904223u; return (float)(g_seed >> 8) / (float)(1u << 24); }

// per strand the entries 4 t + k with nbr[t][k] == s, ascending
void build_lists(int S, const std::vector<int32_t>& nbr, std::vector<int32_t>& start, std::vector<int32_t>& list)
{
    start.assign((size_t)S + 1, 0);
    list.clear();
    for (int s = 0; s < S; s++) {
        start[(size_t)s] = (int32_t)list.size();
        for (int e = 0; e < 4 * S; e++)
            if (nbr[(size_t)e] == s) list.push_back(e);
    }
    start[(size_t)S] = (int32_t)list.size();
}

bool run(const char* name, int S, int n, bool coincident, bool hub)
{
    std::vector<float> roots((size_t)S * 3), dirs((size_t)S * n * 3), rest((size_t)S);
    for (int s = 0; s < S; s++)
        for (int c = 0; c < 3; c++) roots[(size_t)3 * s + c] = coincident ? 0.25f : (float)((s >> (2 * c)) & 3);  // a 4 x 4 x 4 lattice
    for (size_t i = 0; i < dirs.size(); i++) dirs[i] = 0.003f * (rnd() - 0.3f);
    for (int s = 0; s < S; s++) rest[(size_t)s] = 0.002f + 0.001f * rnd();
    for (int c = 0; c < 3; c++) dirs[(size_t)c] = 0.f;                                   // a segment of length exactly 0
    dirs[((size_t)(S - 1) * n + (n - 1)) * 3] = GHR_SHAPE_DEAD * rest[(size_t)S - 1];    // one at the dead threshold
    dirs[((size_t)(S - 1) * n + (n - 1)) * 3 + 1] = 0.f;
    dirs[((size_t)(S - 1) * n + (n - 1)) * 3 + 2] = 0.f;
    std::vector<int32_t> nbr((size_t)S * 4, -7), start, list;
    ghrsim_shape_neighbours(S, roots.data(), coincident ? INFINITY : 1.5f, nbr.data());
    for (int s = 0; s < S; s++)
        for (int k = 0; k < 4; k++) {
            const int32_t x = nbr[(size_t)4 * s + k];
            if (!(x == -1 || (x >= 0 && x < S && x != s))) { std::printf("%s: nbr[%d][%d] = %d\n", name, s, k, x); return false; }
            if (coincident && x != (k < s ? k : k + 1)) { std::printf("%s: coincident roots choose the lowest indices\n", name); return false; }
        }
    if (hub)
        for (int s = 0; s < S; s++)
            for (int k = 0; k < 4; k++) nbr[(size_t)4 * s + k] = s == 0 ? -1 : 0;
    build_lists(S, nbr, start, list);
    long long M = 0;
    for (int32_t x : nbr) M += x >= 0;
    if ((long long)list.size() != M) return false;
    std::vector<float> partial((size_t)S * 3), grad((size_t)S * n * 3), again(grad.size());
    float E[3], E2[3];
    const float dE[3] = {0.7f, 1.3f, 0.45f};
    ghrsim_shape_forward(S, n, dirs.data(), rest.data(), nbr.data(), M, partial.data(), E);
    ghrsim_shape_forward(S, n, dirs.data(), rest.data(), nbr.data(), M, partial.data(), E2);
    std::vector<int32_t> one(1, 0);
    const int32_t* lp = list.empty() ? one.data() : list.data();
    ghrsim_shape_backward(S, n, dirs.data(), rest.data(), nbr.data(), start.data(), lp, (long long)list.size(), M, dE, grad.data());
    ghrsim_shape_backward(S, n, dirs.data(), rest.data(), nbr.data(), start.data(), lp, (long long)list.size(), M, dE, again.data());
    if (std::memcmp(E, E2, sizeof(E)) != 0 || std::memcmp(grad.data(), again.data(), grad.size() * 4) != 0) return false;
    for (int c = 0; c < 3; c++)
        if (!(E[c] >= 0.f) || !std::isfinite(E[c])) { std::printf("%s: E[%d] = %g\n", name, c, E[c]); return false; }
    if (M > 0 && !(E[2] <= 2.f)) return false;
    for (float g : grad)
        if (!std::isfinite(g)) { std::printf("%s: a gradient is not finite\n", name); return false; }
    std::printf("%s: S %d n %d M %lld E %.6g %.6g %.6g\n", name, S, n, M, E[0], E[1], E[2]);
    return true;
}

}  // namespace

int main()
{
    int ok = 0;
    ok += run("coincident", 70, 3, true, false);
    ok += run("lattice-hub", 64, 65, false, true);
    std::printf("%d cases ok\n", ok);
    return ok == 2 ? 0 : 1;
}
