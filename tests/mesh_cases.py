"""Shared cases of the mesh-containment tests (csrc/ghr_mesh.h): the case meshes, their query sets, the numpy float32 MODEL of
the definition (brute force over all faces, the expressions of ghr_mesh.h in their operand order) and a float64 winding-number
TRUTH for the closed meshes.  Everything is computed once per process and handed out read-only."""
import functools

import numpy as np

ICO_A, ICO_B = np.float32(0.5257), np.float32(0.8507)


# ---------------------------------------------------------------------------------------------------------------- meshes
def _f32(v):
    return np.ascontiguousarray(np.asarray(v, np.float64).astype(np.float32))


def _i32(f):
    return np.ascontiguousarray(np.asarray(f, np.int32).reshape(-1, 3))


def box(lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(hi if (i >> c) & 1 else lo)[c] for c in range(3)] for i in range(8)])
    f = [[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6],
         [1, 3, 5], [3, 7, 5]]
    return _f32(v), _i32(f)


def icosphere(level, radius=1.0):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return _f32(np.array(v) * radius), _i32(f)


def torus(nu, nv, R=1.0, r=0.4):
    a = np.arange(nu) * 2 * np.pi / nu
    b = np.arange(nv) * 2 * np.pi / nv
    A, B = np.meshgrid(a, b, indexing="ij")
    v = np.stack([(R + r * np.cos(B)) * np.cos(A), (R + r * np.cos(B)) * np.sin(A), r * np.sin(B)], -1).reshape(-1, 3)
    f = []
    for i in range(nu):
        for j in range(nv):
            p, q, s, t = i * nv + j, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            f += [(p, q, s), (p, s, t)]
    return _f32(v), _i32(f)


def uv_sphere(n_lon, n_lat, radius=1.0):
    """2 n_lon (n_lat - 1) faces: (116, 44) gives the 9976 faces of the reference's head mesh."""
    v = [(0.0, 0.0, 1.0)]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        v += [(np.sin(th) * np.cos(2 * np.pi * j / n_lon), np.sin(th) * np.sin(2 * np.pi * j / n_lon), np.cos(th)) for j in range(n_lon)]
    v.append((0.0, 0.0, -1.0))
    f, last = [], len(v) - 1
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon  # noqa: E731
    for j in range(n_lon):
        f.append((0, ring(1, j), ring(1, j + 1)))
        f.append((last, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)))
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            f += [(ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)), (ring(i, j), ring(i + 1, j + 1), ring(i, j + 1))]
    return _f32(np.array(v) * radius), _i32(f)


def nested_spheres():
    v0, f0 = icosphere(2, 1.0)
    v1, f1 = icosphere(1, 0.5)
    return np.concatenate([v0, v1]), np.concatenate([f0, f1 + len(v0)]).astype(np.int32)


def open_cylinder(n=16):
    a = np.arange(n) * 2 * np.pi / n
    v = np.concatenate([np.stack([np.cos(a), np.sin(a), np.full(n, z)], -1) for z in (-1.0, 1.0)])
    f = []
    for i in range(n):
        j = (i + 1) % n
        f += [(i, j, n + j), (i, n + j, n + i)]
    return _f32(v), _i32(f)


def single_triangle():
    """Perpendicular to z: only the +z ray can cross it, so no point has a majority and nothing is inside."""
    return _f32([[0, 0, 0.25], [1, 0.125, 0.25], [0.25, 1, 0.25]]), _i32([[0, 1, 2]])


def slanted_triangle():
    """An open sheet oblique to all axes: the points two of the three rays hit it from are "inside" by the majority rule --
    what the rule costs on open meshes; kept as a case so that every implementation gives the model's answer there too."""
    return _f32([[0, 0, 0], [1, 0, 0.25], [0, 1, 0.5]]), _i32([[0, 1, 2]])


def with_flat_triangles():
    """A closed box plus triangles that can never count: collinear vertices, a repeated index, and one that is flat along z only."""
    v, f = box((-0.5, -0.25, -0.75), (0.75, 0.5, 0.25))
    extra = _f32([[-0.25, -0.125, 0.0], [0.0, 0.0, 0.0], [0.25, 0.125, 0.0], [0.0, 0.0, -0.5]])
    n = len(v)
    return np.concatenate([v, extra]), np.concatenate([f, _i32([[n, n + 1, n + 2], [n, n, n + 1], [n + 1, n + 3, n + 1]])])


def stack(n, G=8):
    """n small horizontal triangles over ONE cell of the z grid (cell (3, 3) of a G = 8 grid over [0, 8]^2), at heights
    1 .. 7, plus two markers that pin the bounding box to [0, 8]^3: that cell's list holds exactly n faces."""
    v = [[0, 0, 0], [0.25, 0, 0], [0, 0.25, 0], [8, 8, 8], [7.75, 8, 8], [8, 7.75, 8]]
    f = [[0, 1, 2], [3, 4, 5]]
    for i in range(n):
        z = 1.0 + 6.0 * i / max(n - 1, 1)
        b = len(v)
        v += [[3.125, 3.125, z], [3.875, 3.25, z], [3.25, 3.875, z]]
        f.append([b, b + 1, b + 2] if i % 2 == 0 else [b, b + 2, b + 1])
    return _f32(v), _i32(f)


STACK_SIZES = (0, 1, 63, 64, 65, 300)
STACK_G = 8


@functools.lru_cache(maxsize=None)
def meshes():
    """name -> (vertices [V,3] f32, faces [F,3] i32, G or 0, closed)"""
    out = {
        "cube": box((0, 0, 0), (4, 4, 4)) + (0, True),
        "icosphere2": icosphere(2) + (0, True),
        "torus": torus(24, 12) + (0, True),
        "nested": nested_spheres() + (0, True),
        "cylinder": open_cylinder() + (0, False),
        "triangle": single_triangle() + (0, False),
        "slanted": slanted_triangle() + (0, False),
        "flat": with_flat_triangles() + (0, True),
        "box": box((0.1, -0.3, 0.2), (0.9, 0.7, 1.3)) + (0, True),
    }
    for n in STACK_SIZES:
        out["stack%d" % n] = stack(n) + (STACK_G, False)
    for v, f, _, _ in out.values():
        v.setflags(write=False); f.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------- queries
def mesh_box(v, f):
    used = v[f.reshape(-1)]
    return used.min(0), used.max(0)


def cube_tie_lattice():
    """For each axis the 343 queries with integer (u, v) in -1 .. 5 and a half-integer height: [3][343][3]."""
    n = np.arange(-1, 6, dtype=np.float32)
    out = []
    for a in range(3):
        u, w, h = np.meshgrid(n, n, n + np.float32(0.5), indexing="ij")
        q = np.zeros((343, 3), np.float32)
        q[:, (a + 1) % 3], q[:, (a + 2) % 3], q[:, a] = u.ravel(), w.ravel(), h.ravel()
        out.append(q)
    return np.stack(out)


def half_open_rule(q, axis):
    u, w, h = q[:, (axis + 1) % 3], q[:, (axis + 2) % 3], q[:, axis]
    return (u >= 0) & (u < 4) & (w >= 0) & (w < 4) & (h > 0) & (h < 4)


def nonfinite_queries():
    bad = [np.nan, np.inf, -np.inf, 1e30, -1e30]
    q = [[b if c == k else 0.25 for c in range(3)] for b in bad for k in range(3)] + [[np.nan] * 3, [np.inf, -np.inf, np.nan]]
    return np.asarray(q, np.float32)


@functools.lru_cache(maxsize=None)
def queries(name):
    """Finite queries of a case mesh: random ones over 1.25 x its box, its own vertices (every one a tie), vertices with another
    height, edge midpoints, the 27 points on the box's min / centre / max, points outside the box; the cube also gets the
    integer lattice and the tie lattice.  At least 1000 of them."""
    v, f, _, _ = meshes()[name]
    lo, hi = mesh_box(v, f)
    rng = np.random.default_rng(sum(map(ord, name)))
    c, e = (lo + hi) / 2, np.maximum(hi - lo, np.float32(0.5))
    parts = [(c + (rng.random((1200, 3)) - 0.5) * 1.25 * e).astype(np.float32)]
    used = v[np.unique(f)]
    parts.append(used[:200])
    shifted = used[:200].copy()
    shifted[np.arange(len(shifted)), rng.integers(0, 3, len(shifted))] -= np.float32(0.125)
    parts.append(shifted)
    parts.append(((v[f[:100, 0]] + v[f[:100, 1]]) * np.float32(0.5)).astype(np.float32))
    parts.append(np.array([[(lo, c, hi)[(i // 3 ** k) % 3][k] for k in range(3)] for i in range(27)], np.float32))
    parts.append(np.array([hi + 1, lo - 1, [hi[0] + 1, c[1], c[2]], [c[0], lo[1] - np.float32(1e-3), c[2]]], np.float32))
    if name == "cube":
        n = np.arange(-1, 6, dtype=np.float32)
        parts.append(np.stack(np.meshgrid(n, n, n, indexing="ij"), -1).reshape(-1, 3))
        parts.append(cube_tie_lattice().reshape(-1, 3))
    if name.startswith("stack"):
        parts.append(np.array([[3.375, 3.375, z] for z in (0.0, 0.5, 1.0, 3.9, 7.0, 7.5)], np.float32))
    q = np.ascontiguousarray(np.concatenate(parts).astype(np.float32))
    rng.shuffle(q[1:])  # (q[0] stays a random point)
    q.setflags(write=False)
    return q


# ---------------------------------------------------------------------------------------------------------------- the model
def model_crossings(v, f, q, chunk=2048):
    """uint32 [Q][3]: the crossing counts of the definition, float32, brute force over all faces."""
    v, q = np.asarray(v, np.float32), np.asarray(q, np.float32)
    out = np.zeros((len(q), 3), np.uint32)
    if len(f) == 0 or len(q) == 0:
        return out
    lo, hi = mesh_box(v, f)
    with np.errstate(all="ignore"):
        ok = np.all((q >= lo) & (q <= hi), axis=1)
        idx = np.nonzero(ok)[0]
        rep = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])
        for a in range(3):
            U, V = (a + 1) % 3, (a + 2) % 3
            pu_, pv_, ph_ = [[v[f[:, k], c] for k in range(3)] for c in (U, V, a)]
            never = rep | ((pu_[1] - pu_[0]) * (pv_[2] - pv_[0]) - (pv_[1] - pv_[0]) * (pu_[2] - pu_[0]) == 0)
            ulo, uhi = np.minimum(np.minimum(pu_[0], pu_[1]), pu_[2]), np.maximum(np.maximum(pu_[0], pu_[1]), pu_[2])
            vlo, vhi = np.minimum(np.minimum(pv_[0], pv_[1]), pv_[2]), np.maximum(np.maximum(pv_[0], pv_[1]), pv_[2])
            for s in range(0, len(idx), chunk):
                ii = idx[s:s + chunk]
                pu, pv, ph = q[ii, U][:, None], q[ii, V][:, None], q[ii, a][:, None]
                side, e = [], []
                for k in range(3):
                    k1 = (k + 1) % 3
                    flip = f[:, k] > f[:, k1]
                    au, av = np.where(flip, pu_[k1], pu_[k]), np.where(flip, pv_[k1], pv_[k])
                    bu, bv = np.where(flip, pu_[k], pu_[k1]), np.where(flip, pv_[k], pv_[k1])
                    dx, dy = bu - au, bv - av
                    E = dx * (pv - av) - dy * (pu - au)
                    assert E.dtype == np.float32
                    left = (E > 0) | ((E == 0) & ((dy < 0) | ((dy == 0) & (dx > 0))))
                    side.append(left != flip)
                    e.append(np.where(flip, -E, E))
                height = ((e[1] * ph_[0] + e[2] * ph_[1]) + e[0] * ph_[2]) / ((e[0] + e[1]) + e[2])
                in_box = (pu >= ulo) & (pu <= uhi) & (pv >= vlo) & (pv <= vhi)
                crossed = ~never & in_box & (side[0] == side[1]) & (side[1] == side[2]) & (height > ph)
                out[ii, a] = crossed.sum(1)
    return out


def model_contains(v, f, q):
    c = model_crossings(v, f, q)
    return ((c & 1).sum(1) >= 2), c


def ico_vertices():
    """The twelve probe directions in the order of ghr::mesh_ico_vertex."""
    out = np.zeros((12, 3), np.float32)
    for k in range(12):
        g = k >> 2
        out[k, g] = ICO_A if k & 1 else -ICO_A
        out[k, (g + 1) % 3] = -ICO_B if k & 2 else ICO_B
    return out


def model_probe_points(xyz, scaling, rotation, mode):
    """float32 [P][12][3]: ghr::mesh_probe_point, operand for operand."""
    xyz, s, r = (np.asarray(t, np.float32) for t in (xyz, scaling, rotation))
    one, two, three = np.float32(1), np.float32(2), np.float32(3)
    n = np.sqrt(((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]) + r[:, 3] * r[:, 3])
    w, x, y, z = (r[:, i] / n for i in range(4))
    R = [[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
         [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
         [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]]
    s3 = [s[:, i] * three for i in range(3)]
    ico = ico_vertices()
    out = np.zeros((len(xyz), 12, 3), np.float32)
    for k in range(12):
        v = ico[k]
        for j in range(3):
            if mode == 0:
                out[:, k, j] = ((v[0] * (s3[0] * R[j][0]) + v[1] * (s3[1] * R[j][1])) + v[2] * (s3[2] * R[j][2])) + xyz[:, j]
            else:
                out[:, k, j] = s3[j] * ((v[0] * R[0][j] + v[1] * R[1][j]) + v[2] * R[2][j]) + xyz[:, j]
    assert out.dtype == np.float32
    return out


def model_probes_outside(v, f, xyz, scaling, rotation, mode):
    p = model_probe_points(xyz, scaling, rotation, mode)
    inside, _ = model_contains(v, f, p.reshape(-1, 3))
    return ~inside.reshape(-1, 12).any(1)


def gaussians(name, P, seed=0):
    """P Gaussians around a case mesh: centres over 1.25 x its box, scales of a few percent of it, un-normalised quaternions."""
    v, f, _, _ = meshes()[name]
    lo, hi = mesh_box(v, f)
    rng = np.random.default_rng(seed + 17)
    c, e = (lo + hi) / 2, hi - lo
    xyz = (c + (rng.random((P, 3)) - 0.5) * 1.25 * e).astype(np.float32)
    scaling = (np.exp(rng.normal(-3.0, 0.7, (P, 3))) * e.max()).astype(np.float32)
    rotation = (rng.normal(0, 1, (P, 4)) * np.exp(rng.normal(0, 1, (P, 1)))).astype(np.float32)
    return xyz, scaling, rotation


# ---------------------------------------------------------------------------------------------------------------- the truth
def winding_inside(v, f, q, chunk=1024):
    """float64 generalised winding number (solid angles, van Oosterom & Strackee); inside = its rounded value is odd."""
    v, q = np.asarray(v, np.float64), np.asarray(q, np.float64)
    t = v[f]
    out = np.zeros(len(q), bool)
    for s in range(0, len(q), chunk):
        p = q[s:s + chunk, None, None, :]
        d = t[None] - p
        a, b, c = d[:, :, 0], d[:, :, 1], d[:, :, 2]
        la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
        num = np.einsum("qfi,qfi->qf", a, np.cross(b, c))
        den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        w = (2.0 * np.arctan2(num, den)).sum(1) / (4.0 * np.pi)
        out[s:s + chunk] = np.round(w).astype(np.int64) % 2 == 1
    return out
