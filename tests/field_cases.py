"""The float64 arbiter of csrc/ghr_field.h's definition (numpy, brute force) and the cases of tests/test_field_cpu.py and
tests/test_gpu_field.py.  Every case asserts its own margins in float64, so that no decision of an fp32 form is excluded from a
comparison (the cap on skipped comparisons is 0):

    |d2 - r2| >= 1e-5 r2, or an exact tie built from representable coordinates (a point at exactly r is OUTSIDE);
    |d_i . t| >= 1e-4 for every inside point, or exactly 0;
    |rho - rho_min| >= 1e-4 rho_min at every state the fp32 host walk visits.

THE BAR of the fp32 forms against the arbiter.  Measured on the CPU (tests/test_field_cpu.py::test_the_bar_is_four_times_the_
composed_forms_measured_error prints them): the composed fp32 form's largest error over all query cases below is
    rho 6.21e-07, v 4.57e-07 of rho           c 6.48e-07 of rho max|f|
and over the states of the traces (teacher-forced, one step from each)
    a next point 1.57e-06 of h   (the rounding of x + h t at |x| up to 1 with h = 0.02: half an ulp of x is 1.5e-6 h).
With the factor 4 for the forms' different orders of summation:
    BAR_FIELD = 2.6e-6  (rho, v: of rho; c: of rho max|f|)        BAR_POINT = 6.3e-6  (of h)
Where the arbiter's rho is 0 an fp32 form's rho, v, c and n are exactly 0.
The kernels sum one point after the other; the rounding of such a sum grows with the number n of inside points (at most
(n - 1) 2^-24 of rho, in practice about its square root), torch.sum's pairwise sum hardly at all.  The cases keep n <= 300, where
the host walk stays under 0.4 of the bar; at n = 4097 (a radius that reaches all of the largest cloud) the sequential sum's own
rounding, 2.6e-6 of rho, IS the bar, which is why the radius that reaches everything is given to a cloud of 300.
"""
import numpy as np

BAR_FIELD = 2.6e-6
BAR_POINT = 6.3e-6
M_D2, M_DOT, M_RHO = 1e-5, 1e-4, 1e-4


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def r2_of(r):
    """r*r formed once in fp32"""
    return np.float32(np.float32(r) * np.float32(r))


# ---- the arbiter -------------------------------------------------------------------------------------------------------------------
def field64(cloud, x, t, r2, margins=True):
    """cloud: dict(points, directions, weights, colors) of fp32 arrays; x, t [Q, 3]; r2 an fp32 value.  -> rho, v, c (float64), n.
    With ``margins`` the case's margins are asserted for these queries."""
    p, d = cloud["points"].astype(np.float64), cloud["directions"].astype(np.float64)
    m, f = cloud["weights"].astype(np.float64), cloud["colors"].astype(np.float64)
    x, t, r2 = np.asarray(x, np.float64).reshape(-1, 3), np.asarray(t, np.float64).reshape(-1, 3), float(r2)
    Q = x.shape[0]
    rho, v, c, n = np.zeros(Q), np.zeros((Q, 3)), np.zeros((Q, 3)), np.zeros(Q, np.int32)
    for s in range(0, Q, 256):
        dx = p[None, :, :] - x[s:s + 256, None, :]
        d2 = (dx[..., 0] * dx[..., 0] + dx[..., 1] * dx[..., 1]) + dx[..., 2] * dx[..., 2]
        inside = d2 < r2
        dot = (d[None, :, 0] * t[s:s + 256, None, 0] + d[None, :, 1] * t[s:s + 256, None, 1]) + d[None, :, 2] * t[s:s + 256, None, 2]
        if margins:
            assert np.all((np.abs(d2 - r2) >= M_D2 * r2) | (d2 == r2)), "a point within 1e-5 r2 of the radius"
            assert np.all(~inside | (np.abs(dot) >= M_DOT) | (dot == 0)), "an inside line within 1e-4 of perpendicular"
        u = 1 - d2 / r2
        a = np.where(inside, m[None, :] * (u * u), 0.0)
        sa = np.where(dot < 0, -a, a)
        rho[s:s + 256] = a.sum(1)
        v[s:s + 256] = (sa[..., None] * d[None]).sum(1)
        c[s:s + 256] = (a[..., None] * f[None]).sum(1)
        n[s:s + 256] = inside.sum(1)
    return rho, v, c, n


def len64(a):
    return np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])


def step64(x, t, rho, v, h, beta, rho_min):
    """One decision and the next heading / point of the definition in float64 for states x, t [N, 3].  -> supported, t', x + h t'
    (the caller applies the coast rule: whether the point is made at all)."""
    lv = len64(v)
    sup = (rho >= rho_min) & (lv > 0)
    u = v / np.where(lv > 0, lv, 1.0)[:, None]
    b = t * (1.0 - float(beta)) + u * float(beta)
    tn = np.where(sup[:, None], b / np.maximum(len64(b), 1e-8)[:, None], t)
    return sup, tn, x + float(h) * tn


def trace64(cloud, roots, normals, M, r2, h, beta, rho_min, max_coast):
    """The trace of the definition, free-running in float64 -> path [S, M+1, 3], steps [S], rgb [S, 3]."""
    x = np.asarray(roots, np.float64).copy()
    nrm = np.asarray(normals, np.float64)
    t = nrm / np.maximum(len64(nrm), 1e-8)[:, None]
    S = x.shape[0]
    path = np.repeat(x[:, None, :], M + 1, axis=1)
    live, coast, rows, steps = np.ones(S, bool), np.zeros(S, int), np.ones(S, int), np.zeros(S, int)
    C, R = np.zeros((S, 3)), np.zeros(S)
    for _ in range(M):
        if not live.any():
            break
        rho, v, c, _n = field64(cloud, x, t, r2, margins=False)
        sup, tn, xn = step64(x, t, rho, v, h, beta, rho_min)
        sup &= live
        t = np.where(sup[:, None], tn, t)
        C, R = np.where(sup[:, None], C + c, C), np.where(sup, R + rho, R)
        coast = np.where(sup, 0, coast + 1)
        live &= sup | (coast <= max_coast)
        x = np.where(live[:, None], x + float(h) * t, x)
        rows += live
        path[live, rows[live] - 1] = x[live]
        steps = np.where(sup, rows - 1, steps)
    path = np.where((np.arange(M + 1)[None, :] >= rows[:, None])[..., None], x[:, None, :], path)
    rgb = np.where((R == 0)[:, None], 0.0, C / np.where(R == 0, 1.0, R)[:, None])
    return path, steps.astype(np.int32), rgb


def spans(n, L):
    """(q, q1, rem) of the resampling for steps n [S]: integers only"""
    num = np.arange(L, dtype=np.int64)[None, :] * np.asarray(n, np.int64)[:, None]
    q, rem = num // (L - 1), num % (L - 1)
    return q, np.minimum(q + 1, np.asarray(n, np.int64)[:, None]), rem


def resample64(path, steps, L):
    q, q1, rem = spans(steps, L)
    p = np.asarray(path, np.float64)
    a, b = np.take_along_axis(p, q[..., None], 1), np.take_along_axis(p, q1[..., None], 1)
    return a + (b - a) * (rem / float(L - 1))[..., None]


# ---- clouds and queries ------------------------------------------------------------------------------------------------------------
def unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def make_cloud(P, kind, seed):
    g = np.random.default_rng(seed)
    p = g.random((P, 3))
    if kind == "plane":
        p[:, 2] = 0.25
    if kind == "duplicates":
        p = p[g.integers(0, max(1, P // 3), P)]
    d = unit(g.normal(size=(P, 3)))
    return dict(points=f32(p), directions=f32(unit(f32(d).astype(np.float64))), weights=f32(g.random(P) * 0.9 + 0.1),
                colors=f32(g.random((P, 3)) * 2 - 0.5))


def make_queries(cloud, Q, r, seed, lo=0.0, hi=1.0):
    """Q queries in [lo, hi)^3 with unit headings that meet the margins against ``cloud`` at radius r: a draw that does not is
    drawn again (the draws depend on nothing but the seed and the cloud)."""
    g = np.random.default_rng(seed)
    x, t = f32(g.random((Q, 3)) * (hi - lo) + lo), f32(unit(g.normal(size=(Q, 3))))
    r2 = r2_of(r)
    for _ in range(200):
        bad = np.zeros(Q, bool)
        for i in range(Q):
            try:
                field64(cloud, x[i], t[i], r2)
            except AssertionError:
                bad[i] = True
        if not bad.any():
            return x, t
        k = int(bad.sum())
        x[bad], t[bad] = f32(g.random((k, 3)) * (hi - lo) + lo), f32(unit(g.normal(size=(k, 3))))
    raise AssertionError("no queries with margins found")


# name: (P, Q, cloud kind, radius, (lo, hi) of the queries)
QUERY_CASES = {}
for _P in (1, 63, 64, 65, 4095, 4096, 4097):
    QUERY_CASES["P%d" % _P] = (_P, 65, "uniform", 0.6 if _P < 100 else 0.12, (0.0, 1.0))
for _Q in (1, 63, 64, 257):
    QUERY_CASES["Q%d" % _Q] = (4097 if _Q == 257 else 300, _Q, "uniform", 0.12 if _Q == 257 else 0.3, (0.0, 1.0))
QUERY_CASES.update({
    "nothing": (300, 65, "uniform", 1e-4, (0.0, 1.0)),
    "everything": (300, 65, "uniform", 4.0, (0.0, 1.0)),
    "everything_small": (65, 64, "uniform", 4.0, (0.0, 1.0)),
    "duplicates": (300, 65, "duplicates", 0.3, (0.0, 1.0)),
    "plane": (300, 65, "plane", 0.3, (0.0, 1.0)),
    "far_small_r": (300, 65, "uniform", 0.3, (50.0, 60.0)),
    "far_large_r": (300, 65, "uniform", 120.0, (50.0, 60.0)),
})


def query_case(name):
    if name == "tie":
        return tie_case()
    P, Q, kind, r, (lo, hi) = QUERY_CASES[name]
    seed = sorted(QUERY_CASES).index(name) + 1
    cloud = make_cloud(P, kind, seed)
    x, t = make_queries(cloud, Q, r, 1000 + seed, lo, hi)
    return dict(cloud=cloud, x=x, t=t, r=r, r2=r2_of(r))


def tie_case():
    """Representable coordinates: r = 0.25, points at exactly r (OUTSIDE) and just inside, lines exactly perpendicular to the
    heading (d . t = 0 counts as +) and exactly opposed."""
    pts = f32([[0.25, 0, 0], [0, -0.25, 0], [0, 0, 0.25], [0.125, 0, 0], [0, 0.125, 0], [0.75, 0.5, 0.5], [0.5, 0.5, 0.375]])
    dirs = f32([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 1, 0], [-1, 0, 0], [1, 0, 0], [0, 0, -1]])
    cloud = dict(points=pts, directions=dirs, weights=f32([1, 0.5, 0.25, 1, 0.5, 1, 2]), colors=f32(np.arange(21).reshape(7, 3) / 8))
    x = f32([[0, 0, 0], [0.5, 0.5, 0.5], [0, 0, 0]])
    t = f32([[1, 0, 0], [0, 0, 1], [0, 0, 1]])
    return dict(cloud=cloud, x=x, t=t, r=0.25, r2=r2_of(0.25))


ALL_QUERY_CASES = sorted(QUERY_CASES) + ["tie"]


# ---- scenes with a known answer ----------------------------------------------------------------------------------------------------
def helix_scene(n_curves=40, per_curve=250, S=None, seed=7, length=1.5):
    """A seeded bundle of helices about the z axis sampled as a cloud (jittered positions, noisy tangents with random signs); roots
    at the curves' starts (root i on curve i % n_curves, jittered from the second round on) with perturbed headings.  The cloud stops
    0.075 of the parameter short of the curves' ends: a strand's last kept point is one step PAST its last supported state, up to
    about r beyond the last cloud point (measured: 1.06 r with the cloud to the very end), and tips are where captures are thin.
    -> dict(cloud, roots, normals, curves [n_curves, 3000, 3] dense samples of the true curves)"""
    g = np.random.default_rng(seed)
    S = n_curves if S is None else S
    ang, rad = g.random(n_curves) * 2 * np.pi, 0.05 + 0.3 * np.sqrt(g.random(n_curves))
    base = np.stack([rad * np.cos(ang), rad * np.sin(ang), np.zeros(n_curves)], 1)
    # (gentle turns: the trace follows directions only, nothing pulls it back to a curve's centre line, so it drifts outward by about
    # curvature x h x length -- here up to 0.8 / unit length x 0.02 x 1.4)
    a, w, th = 0.02 + 0.02 * g.random(n_curves), 2 + 2 * g.random(n_curves), g.random(n_curves) * 2 * np.pi

    def curve(i, s):
        ph = w[i] * s + th[i]
        return base[i] + np.stack([a[i] * np.cos(ph), a[i] * np.sin(ph), 0.9 * s], -1)

    def tangent(i, s):
        ph = w[i] * s + th[i]
        return unit(np.stack([-a[i] * w[i] * np.sin(ph), a[i] * w[i] * np.cos(ph), 0.9 * np.ones_like(s)], -1))

    pts, dirs = [], []
    for i in range(n_curves):
        s = g.random(per_curve) * (length - 0.075)
        pts.append(curve(i, s) + g.normal(size=(per_curve, 3)) * 0.003)
        dirs.append(unit(tangent(i, s) + g.normal(size=(per_curve, 3)) * 0.1) * g.choice([-1.0, 1.0], per_curve)[:, None])
    pts, dirs = np.concatenate(pts), np.concatenate(dirs)
    P = pts.shape[0]
    cloud = dict(points=f32(pts), directions=f32(unit(f32(dirs).astype(np.float64))), weights=f32(0.5 + 0.5 * g.random(P)),
                 colors=f32(g.random((P, 3))))
    idx = np.arange(S) % n_curves
    zero = np.zeros(1)
    roots = np.stack([curve(i, zero)[0] for i in idx]) + (np.arange(S) >= n_curves)[:, None] * g.normal(size=(S, 3)) * 0.004
    normals = np.stack([tangent(i, zero)[0] for i in idx]) + g.normal(size=(S, 3)) * 0.15
    dense = np.linspace(0, length, 3000)
    return dict(cloud=cloud, roots=f32(roots), normals=f32(normals), curves=np.stack([curve(i, dense) for i in range(n_curves)]))


HELIX_R, HELIX_H = 0.05, 0.02


def distance_to_curves(points, curves):
    """the distance of every point [N, 3] to the nearest dense sample of any true curve (an upper bound of its distance to them)"""
    c = curves.reshape(-1, 3)
    out = np.empty(points.shape[0])
    for s in range(0, points.shape[0], 512):
        out[s:s + 512] = np.sqrt(((points[s:s + 512, None, :] - c[None]) ** 2).sum(-1).min(1))
    return out


def assert_grown_hair(path, steps, curves, r=HELIX_R, min_kept=30):
    """item 9: every kept point of every grown strand lies within r of some true curve, and every strand keeps >= 30 steps"""
    steps = np.asarray(steps)
    assert steps.min() >= min_kept, ("kept steps", int(steps.min()), int(steps.max()))
    kept = np.concatenate([np.asarray(path, np.float64)[s, :steps[s] + 1] for s in range(len(steps))])
    worst = float(distance_to_curves(kept, curves).max())
    print("kept steps %d..%d, worst distance %.3f r" % (steps.min(), steps.max(), worst / r))
    assert worst < r, worst / r


def small_scene(S, seed=19):
    """the trace cases' scene: 8 helices, 120 points each (the seed: one at which every state the host walk visits in
    tests/test_field_cpu.py's traces keeps the margins, as the tests assert)"""
    return helix_scene(n_curves=8, per_curve=120, S=S, seed=seed, length=1.0)


TRACE_S, TRACE_M, TRACE_COAST = (1, 64, 65), (1, 2, 7, 40), (0, 2)
TRACE_ARGS = dict(r=HELIX_R, h=HELIX_H, beta=0.5, rho_min=0.2)


def line_scene(gap_start_k, seed=3):
    """Points on the x axis at 0.0025 + 0.005 k, k < 58 (the last at 0.2875) and from k = gap_start_k on (to 0.8), lines along x
    with random signs, weight 1; one root at the origin heading +x, h = 0.02, r = 0.05, rho_min = 0.01.  A sample at x is
    unsupported iff no point is within r: 0.34, 0.36, ... until the second run is nearer than 0.05."""
    g = np.random.default_rng(seed)
    k = np.concatenate([np.arange(58), np.arange(gap_start_k, 160)])
    P = k.shape[0]
    pts = np.zeros((P, 3))
    pts[:, 0] = 0.0025 + 0.005 * k
    dirs = np.zeros((P, 3))
    dirs[:, 0] = g.choice([-1.0, 1.0], P)
    cloud = dict(points=f32(pts), directions=f32(dirs), weights=f32(np.ones(P)), colors=f32(g.random((P, 3))))
    return dict(cloud=cloud, roots=f32([[0, 0, 0]]), normals=f32([[2, 0, 0]]))


# (max_coast, k of the second run's first point, unsupported steps of the gap, whether the strand crosses it)
GAP_CASES = {"coast2_gap2": (2, 84, 2, True), "coast2_gap3": (2, 88, 3, False), "coast0_gap0": (0, 58, 0, True),
             "coast0_gap1": (0, 80, 1, False)}
LINE_ARGS = dict(r=0.05, h=0.02, beta=0.5, rho_min=0.01, M=40)

RESAMPLE_L = (2, 3, 100)


def resample_steps(L):
    return [0, 1, max(L - 2, 0), L - 1, L, 3 * L + 1]
