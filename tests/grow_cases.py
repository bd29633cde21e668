"""The float64 arbiter of csrc/ghr_grow.h's guard (numpy, brute force) and the cases of tests/test_grow_guarded_cpu.py and
tests/test_gpu_grow_guarded.py.  Every case asserts its own margins in float64 at every state an fp32 form visits, so that no
decision is excluded from a comparison:

    |sd - m| >= 1e-4 m                      (free or contact; the cube case, built from representable coordinates, also holds the
                                            exact tie sd == m, which is FREE: a strand that slides along a flat face meets it)
    d == 0 exactly, or d >= 1e-5            (inside or outside: the sign of a y on the surface is the containment's tie rule)
    |tn| >= 1e-4, or exactly 0              (slide or not)
    |l - 1e-4| >= 1e-5                      (head-on or not)
    and tests/field_cases.py's for the field (|d2 - r2|, |d . t|, |rho - rho_min|).

Teacher-forced, as tests/test_field_cpu.py: the arbiter takes the fp32 walk's (x_j, t_j) of every step, must make the same decisions
and the next point and heading under the bar.  It also takes the walk's closest point c_j, after checking it: c_j lies on the mesh
(within 1e-6 of the larger of 1 and |y|) and is as near to y as the float64 closest point (d within 1e-5 relative + 1e-12).  Which of two equally near
candidates a float32 search selects is ghr_meshdist.h's business and held to its own bar by its own tests (near the
line where an edge's region meets a face's, two points up to 2 sqrt(|d1 - d2|) apart are equally near in float32); the guard's
arithmetic is what is judged here.

THE BAR of the fp32 forms against the arbiter, 8s's convention: the composed fp32 form's largest error over the cases on the CPU
(tests/test_grow_guarded_cpu.py::test_the_bar_is_four_times_the_composed_forms_measured_error prints them), times 4.
    a next point, free or pushed: measured 4.02e-06 of h    BAR_PUSH    = 1.7e-5  (of h)
    a heading after the guard:    measured 4.37e-06 (of 1)  BAR_HEADING = 1.8e-5  (of 1)
(The point's error is largest in the "free" case, whose coordinates are about 8: half an ulp of x there is 4e-6 h at h = 0.06; on
the unit heads it is 1.1e-6 .. 2.2e-6 of h.  The heading's error is the normal's: n = (y - c) / d with d about m = 0.03 and y, c
rounded at 1, and the slide removes tn n from t; it is largest on the icosahedron, whose faces the strands meet at the steepest
angles.)
"""
import functools

import numpy as np

from tests import field_cases as fc
from tests import mesh_cases as mc

BAR_PUSH = 1.7e-5
BAR_HEADING = 1.8e-5
M_SD, M_D, M_TN, M_L = 1e-4, 1e-5, 1e-4, 1e-5
HEADON = 1e-4
FREE, PUSHED, ON_SURFACE, HEAD_ON = 0, 1, 2, 3      # the log's outcome of a guarded step
STOP_STEPS, STOP_COAST, STOP_HEADON = 0, 1, 2


# ---- the arbiter -------------------------------------------------------------------------------------------------------------------
def closest64(v, f, q, chunk=256):
    """float64 closest point of the mesh (Ericson's regions, brute force) -> d [Q], point [Q, 3]"""
    v, q = np.asarray(v, np.float64), np.asarray(q, np.float64).reshape(-1, 3)
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    dot = lambda x, y: (x * y).sum(-1)  # noqa: E731
    out_d, out_p = np.zeros(len(q)), np.zeros((len(q), 3))
    with np.errstate(all="ignore"):
        for s in range(0, len(q), chunk):
            p = q[s:s + chunk, None, :]
            ab, ac, ap = b - a, c - a, p - a
            d1, d2 = dot(ab, ap), dot(ac, ap)
            bp = p - b
            d3, d4 = dot(ab, bp), dot(ac, bp)
            cp = p - c
            d5, d6 = dot(ab, cp), dot(ac, cp)
            vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
            denom = va + vb + vc
            res = a + ab * (vb / denom)[..., None] + ac * (vc / denom)[..., None]
            m = (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)
            res = np.where(m[..., None], b + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None] * (c - b), res)
            m = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
            res = np.where(m[..., None], a + (d2 / (d2 - d6))[..., None] * ac, res)
            m = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
            res = np.where(m[..., None], a + (d1 / (d1 - d3))[..., None] * ab, res)
            res = np.where(((d6 >= 0) & (d5 <= d6))[..., None], c + 0 * p, res)
            res = np.where(((d3 >= 0) & (d4 <= d3))[..., None], b + 0 * p, res)
            res = np.where(((d1 <= 0) & (d2 <= 0))[..., None], a + 0 * p, res)
            dd = np.sqrt(dot(res - p, res - p))
            assert np.isfinite(dd).all()                                    # (the cases' meshes have no zero-area face)
            k = dd.argmin(1)
            ar = np.arange(len(k))
            out_d[s:s + chunk], out_p[s:s + chunk] = dd[ar, k], res[ar, k]
    return out_d, out_p


def inside64(v, f, q):
    """float64 containment in a CONVEX closed mesh: on the inner side of every face's plane (the cases' meshes are convex)"""
    v, q = np.asarray(v, np.float64), np.asarray(q, np.float64).reshape(-1, 3)
    a = v[f[:, 0]]
    n = np.cross(v[f[:, 1]] - a, v[f[:, 2]] - a)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    centre = v[np.unique(f)].mean(0)
    n *= np.sign(((a - centre) * n).sum(1))[:, None]                        # outward
    return (((q[:, None, :] - a[None]) * n[None]).sum(-1) < 0).all(1)


def guard64(v, f, t, y, c, m, ties=False):
    """The guard of csrc/ghr_grow.h in float64 for headings t [N, 3] (after the heading update), y [N, 3] and the closest points
    c [N, 3] an fp32 form found (checked here).  Asserts the margins; ``ties``: a case built from representable coordinates may
    also hold sd == m exactly (FREE).  -> outcome [N], the heading after, the next point, inside"""
    t, y, c, m = np.asarray(t, np.float64), np.asarray(y, np.float64), np.asarray(c, np.float64), float(m)
    fin = np.isfinite(y).all(1)
    assert fin.all(), "the cases keep every y finite"
    d_true, _ = closest64(v, f, y)
    d_on, _ = closest64(v, f, c)
    scale = max(1.0, float(np.abs(y).max()))                                 # (a projection q - k n is rounded at the query's size)
    assert np.all(d_on <= 1e-6 * scale), ("a closest point off the mesh", float(d_on.max()))
    d = fc.len64(y - c)
    assert np.all(np.abs(d - d_true) <= 1e-5 * d_true + 1e-12), ("a closest point that is not the nearest", float(np.abs(d - d_true).max()))
    inn = inside64(v, f, y)
    assert np.all((d_true == 0) | (d_true >= M_D)), "a y within 1e-5 of the surface"
    sd = np.where(inn, -d_true, d_true)
    assert np.all((np.abs(sd - m) >= M_SD * m) | (ties & (sd == m))), "a y within 1e-4 m of the margin"
    contact = sd < m
    on = contact & (d_true == 0)
    corr = contact & ~on
    n = np.where(corr[:, None], (y - c) / np.where(corr, d, 1.0)[:, None], 0.0)
    n = np.where(inn[:, None], -n, n)
    tn = (t[:, 0] * n[:, 0] + t[:, 1] * n[:, 1]) + t[:, 2] * n[:, 2]
    assert np.all(~corr | (np.abs(tn) >= M_TN) | (tn == 0)), "a heading within 1e-4 of tangent"
    slide = corr & (tn < 0)
    s = t - tn[:, None] * n
    l = fc.len64(s)
    assert np.all(~slide | (np.abs(l - HEADON) >= M_L)), "a slid heading within 1e-5 of the head-on length"
    head_on = slide & (l <= HEADON)
    t2 = np.where((slide & ~head_on)[:, None], s / np.where(l > 0, l, 1.0)[:, None], t)
    x2 = np.where(corr[:, None], c + m * n, y)
    outcome = np.where(head_on, HEAD_ON, np.where(on, ON_SURFACE, np.where(corr, PUSHED, FREE)))
    return outcome, t2, x2, inn


def check_trace(case, got):
    """Teacher-forces the arbiter along one fp32 trace ``got`` (path, steps, rgb, contacts, stop, log) of ``case``: every decision,
    ``steps``, ``contacts`` and ``stop`` exactly.  -> the largest error of a next point (of h) and of a heading (of 1)"""
    path, steps, rgb, contacts, stop, log = got
    cloud, (v, f) = case["cloud"], case["mesh"]
    S, M, coast = path.shape[0], case["M"], case["max_coast"]
    h, beta, rho_min, m = [float(np.float32(case[k])) for k in ("h", "beta", "rho_min", "margin")]
    r2 = fc.r2_of(case["r"])
    live, coast_n, rows, st = np.ones(S, bool), np.zeros(S, int), np.ones(S, int), np.zeros(S, int)
    cont, why = np.zeros(S, int), np.zeros(S, int)
    e_point = e_head = 0.0
    assert np.array_equal(path[:, 0], case["roots"])
    for j in range(M):
        made = ~np.isnan(log[:, j, 13])
        assert np.array_equal(made, live), j
        if not live.any():
            break
        i = np.nonzero(live)[0]
        x, t = log[i, j, 0:3].astype(np.float64), log[i, j, 3:6].astype(np.float64)
        assert np.array_equal(log[i, j, 0:3], path[i, rows[i] - 1])
        rho, fv, _c, _n = fc.field64(cloud, x, t, r2)                        # (asserts the field's margins)
        assert np.all(np.abs(rho - rho_min) >= fc.M_RHO * rho_min), "a state within 1e-4 of rho_min"
        sup, tn, y = fc.step64(x, t, rho, fv, h, beta, rho_min)
        assert np.array_equal(sup, log[i, j, 13] == 1), j
        coast_n[i] = np.where(sup, 0, coast_n[i] + 1)
        out = coast_n[i] > coast
        assert np.array_equal(out, log[i, j, 13] == -1), j
        why[i[out]] = STOP_COAST
        live[i[out]] = False
        i, sup, tn, y = i[~out], sup[~out], tn[~out], y[~out]
        if i.size == 0:
            continue
        e_head = max(e_head, float(np.abs(log[i, j, 14:17] - tn).max()))     # the heading update (8s's, one more look at it)
        e_point = max(e_point, float(np.abs(log[i, j, 17:20] - y).max() / h))
        outcome, t2, x2, inn = guard64(v, f, tn, y, log[i, j, 21:24], m, ties=case.get("ties", False))
        assert np.array_equal(outcome, log[i, j, 25].astype(int)), (j, outcome, log[i, j, 25])
        off = outcome != ON_SURFACE                                          # (on the surface the sign is the containment's tie rule)
        assert np.array_equal(inn[off], log[i, j, 24][off] == 1), j
        ho = outcome == HEAD_ON
        why[i[ho]] = STOP_HEADON
        live[i[ho]] = False
        go, sup = i[~ho], sup[~ho]
        rows[go] += 1
        cont[go] += (outcome[~ho] != FREE)
        st[go[sup]] = rows[go[sup]] - 1
        if go.size:
            e_point = max(e_point, float(np.abs(path[go, rows[go] - 1] - x2[~ho]).max() / h))
            e_head = max(e_head, float(np.abs(log[go, j, 26:29] - t2[~ho]).max()))
    assert np.array_equal(steps, st) and np.array_equal(contacts, cont) and np.array_equal(stop, why)
    for s in range(S):
        assert not np.isnan(path[s]).any() and np.all(path[s, rows[s]:] == path[s, rows[s] - 1])
    return e_point, e_head


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def icosphere(level):
    v, f = mc.icosphere(level)
    v.setflags(write=False); f.setflags(write=False)
    return v, f


@functools.lru_cache(maxsize=None)
def cube():
    """the dyadic axis-aligned cube [0, 1]^3 (F = 12)"""
    v, f = mc.box((0, 0, 0), (1, 1, 1))
    v.setflags(write=False); f.setflags(write=False)
    return v, f


@functools.lru_cache(maxsize=None)
def head_mesh(name):
    from gaussianhaircut_amd.mesh import HeadMesh
    v, f = cube() if name == "cube" else icosphere(int(name[3:]))
    return HeadMesh(v, f)


def surface_radius(v, f, u):
    """the distance from the origin to the surface of a convex mesh around it along the unit directions u [N, 3]"""
    v = np.asarray(v, np.float64)
    a = v[f[:, 0]]
    n = np.cross(v[f[:, 1]] - a, v[f[:, 2]] - a)
    n *= np.sign((a * n).sum(1))[:, None]
    num, den = (a * n).sum(1)[None, :], u @ n.T
    return np.where(den > 1e-12, num / np.where(den > 1e-12, den, 1.0), np.inf).min(1)


# ---- the sphere scene --------------------------------------------------------------------------------------------------------------
def _down_tangent(u):
    """the unit tangent of the sphere at u that points towards -z (the pole's is +x)"""
    d = np.stack([u[:, 0] * u[:, 2], u[:, 1] * u[:, 2], u[:, 2] ** 2 - 1.0], 1)
    l = np.linalg.norm(d, axis=1, keepdims=True)
    return np.where(l > 1e-9, d / np.where(l > 1e-9, l, 1.0), np.array([[1.0, 0.0, 0.0]]))


def sphere_scene(level, S, P, seed, shell=0.15, lean=0.3, zmin=-0.75, cap=0.6, lift=0.01, tilt=1.0):
    """A cloud of hair that lies on a head: P points over the part z >= zmin of an icosphere, between its surface and ``shell`` above
    it, lines combed down with an inward lean of ``lean`` (random signs); S roots on the cap z >= cap, ``lift`` above the surface,
    normals tilted downwards by ``tilt`` (1: 45 degrees)."""
    v, f = icosphere(level)
    g = np.random.default_rng(seed)

    def dirs(n, lo):
        z = lo + (1 - lo) * g.random(n)
        ph = 2 * np.pi * g.random(n)
        s = np.sqrt(1 - z * z)
        return np.stack([s * np.cos(ph), s * np.sin(ph), z], 1)
    u = dirs(P, zmin)
    pts = u * (surface_radius(v, f, u) + shell * g.random(P))[:, None]
    d = fc.unit(_down_tangent(u) - lean * u + 0.1 * g.normal(size=(P, 3))) * g.choice([-1.0, 1.0], P)[:, None]
    cloud = dict(points=fc.f32(pts), directions=fc.f32(fc.unit(fc.f32(d).astype(np.float64))), weights=fc.f32(0.5 + 0.5 * g.random(P)),
                 colors=fc.f32(g.random((P, 3))))
    ur = dirs(S, cap)
    roots = ur * (surface_radius(v, f, ur) + lift)[:, None]
    normals = ur + tilt * _down_tangent(ur)
    return dict(cloud=cloud, roots=fc.f32(roots), normals=fc.f32(normals), mesh=(v, f))


SPHERE_ARGS = dict(r=0.15, h=0.06, beta=0.5, rho_min=0.2, max_coast=2, margin=0.03, M=20)

# name: (icosphere level, S, P, seed).  The seeds: ones at which every state the host walk visits keeps the margins (the tests
# assert them).  F = 20, 80, 1280, 5120: one block of faces, a second block (64-face block ends), 20 blocks, a second superblock.
FREE_SEED = 5
SPHERE_CASES = {"ico0": (0, 20, 3500, 1), "ico1": (1, 33, 3500, 2), "ico3": (3, 65, 3500, 3), "ico4": (4, 40, 3500, 4)}


def _far_cloud():
    """one point far from everything: a cloud that supports nothing (the planted strands coast)"""
    return dict(points=fc.f32([[40, 40, 40]]), directions=fc.f32([[1, 0, 0]]), weights=fc.f32([1]), colors=fc.f32([[0.5, 0.5, 0.5]]))


def planted_cube():
    """Strands without support (they coast max_coast = 2 steps: two guarded steps each, and stop at the third) against the dyadic
    cube, all coordinates representable, h = 1/16, m = 1/8:
      0  y exactly on a face (d2 == 0): no correction; then inside and heading along -n: stops head-on
      1  heading exactly along -n within the margin: stops head-on at its first step
      2  tn exactly 0 in contact: pushed to exactly m above the face, heading unchanged; then sd == m exactly: free
      3  outside the mesh's bounding box: free
      4  in contact from step 1, heading (1, 0, -1) / sqrt 2: pushed, the heading slides to (1, 0, 0); then sd == m exactly: free
      5  becomes inside: h > the distance, y jumps the surface obliquely; pushed out, the heading slides
      6  free throughout"""
    q = np.float32(1) / np.sqrt(np.float32(2))
    roots = [[0.375, 0.625, 1.0625], [0.375, 0.625, 1.125], [0.375, 0.625, 1.0625], [3, 3, 3], [0.375, 0.625, 1.09375],
             [0.375, 0.625, 1.015625], [0.375, 0.625, 1.5]]
    normals = [[0, 0, -1], [0, 0, -1], [1, 0, 0], [1, 0, 0], [q, 0, -q], [q, 0, -q], [0, 1, 0]]
    return dict(cloud=_far_cloud(), roots=fc.f32(roots), normals=fc.f32(normals), mesh=cube(), mesh_name="cube", r=0.25, h=0.0625,
                beta=0.5, rho_min=0.2, max_coast=2, margin=0.125, M=3, ties=True)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "planted_cube":
        c = planted_cube()
    elif name == "free":                                                     # the mesh is far from every strand: never in contact
        c = dict(sphere_scene(1, 33, 3500, FREE_SEED), mesh_name="ico1", **SPHERE_ARGS)
        c["roots"] = fc.f32(c["roots"] + 7.0)
        c["cloud"] = dict(c["cloud"], points=fc.f32(c["cloud"]["points"] + 7.0))
    elif name == "mixed":                                                    # free, contact, coast-stopped and head-on in one wave
        level, S, P, seed = SPHERE_CASES["ico3"]
        c = dict(sphere_scene(level, S, P, seed), mesh_name="ico3", **SPHERE_ARGS)
        c["roots"], c["normals"] = c["roots"].copy(), c["normals"].copy()
        c["roots"][5] = (3.0, 3.0, 3.0)                                       # no support anywhere: coasts and stops
        c["roots"][9] *= np.float32(1.1)                                     # high in the shell: free at first
        v, f = c["mesh"]
        vv = v.astype(np.float64)
        cen = vv[f].mean(1)
        k = int(cen[:, 2].argmin())                                          # below the cloud, above the middle of a face, heading
        n = np.cross(vv[f[k, 1]] - vv[f[k, 0]], vv[f[k, 2]] - vv[f[k, 0]])    # straight at it: coasts into the head head-on
        n = fc.unit(n) * np.sign(n @ cen[k])
        c["roots"][11], c["normals"][11] = fc.f32(cen[k] + 0.01 * n), fc.f32(-n)
    elif name == "M1":
        c = dict(case("mixed"), M=1)
    else:
        level, S, P, seed = SPHERE_CASES[name]
        c = dict(sphere_scene(level, S, P, seed), mesh_name="ico%d" % level, **SPHERE_ARGS)
    return c


def sized_scene(S):
    """the mixed wave's scene with S roots (the GPU test's S = 1, 63, 64, 65, 130: a wave's tail, a second block, a third wave)"""
    return dict(sphere_scene(3, S, 3500, 100 + S), mesh_name="ico3", **SPHERE_ARGS)


ALL_CASES = ("planted_cube", "free", "mixed", "M1") + tuple(sorted(SPHERE_CASES))


# ---- the scene that fails without the feature --------------------------------------------------------------------------------------
def head_scene(S=65, P=60000, seed=11):
    """the issue's scene on the F = 1280 icosphere: 60 000 points in the shell 0 .. 0.15 above the head, lines combed down with an
    inward lean of 0.3; roots on the upper cap, normals tilted 45 degrees downwards; r = 0.06, h = r / 2.5, M = 150"""
    sc = sphere_scene(3, S, P, seed, zmin=-1.0, cap=0.7, lift=0.0)
    return dict(sc, r=0.06, h=0.024, M=150, mesh_name="ico3")
