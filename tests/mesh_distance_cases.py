"""Shared cases of the mesh-distance tests (csrc/ghr_meshdist.h): the case meshes and their query sets, the numpy float32 MODEL of
the definition (brute force over all faces in their given order, the expressions of ghr_meshdist.h in their operand order) and a
float64 TRUTH (Ericson's region algorithm, Real-Time Collision Detection 5.1.5).  Everything is computed once per process and
handed out read-only."""
import functools

import numpy as np

from tests import mesh_cases as mc

F32_MAX = np.float32(3.4028234663852886e38)
ZERO, ONE = np.float32(0), np.float32(1)
BASE = ("cube", "icosphere2", "torus", "flat", "triangle", "cylinder")
ICO4_SLICES = (63, 64, 65, 4096, 4097, 5120)
Q_SIZES = (1, 63, 64, 65, 257)


# ---------------------------------------------------------------------------------------------------------------- meshes
@functools.lru_cache(maxsize=None)
def meshes():
    """name -> (vertices [V,3] f32, faces [F,3] i32, closed)"""
    out = {n: (mc.meshes()[n][0], mc.meshes()[n][1], mc.meshes()[n][3]) for n in BASE}
    v4, f4 = mc.icosphere(4)
    assert len(f4) == 5120
    for n in ICO4_SLICES:
        out["ico4_%d" % n] = (v4, np.ascontiguousarray(f4[:n]), n == 5120)
    for v, f, _ in out.values():
        v.setflags(write=False); f.setflags(write=False)
    return out


CASES = tuple(BASE) + tuple("ico4_%d" % n for n in ICO4_SLICES)
CLOSED = ("cube", "icosphere2", "torus", "flat")
SMALL = BASE  # the meshes on which every (query, face) pair is checked against its block's bound


def nonfinite_queries():
    return mc.nonfinite_queries()


@functools.lru_cache(maxsize=None)
def queries(name):
    """Finite queries of a case: the mesh's own vertices (every one at distance 0, shared by several faces), edge midpoints, face
    centroids, points far outside (no block can be pruned before the seed is scanned), points inside, random points over 1.5 x
    the box, duplicated queries; the integer cube also gets its tie lattice, the integer lattice and its centre (exact ties
    across faces).  Shuffled (q[0] stays the first vertex), so that every prefix -- Q_SIZES -- mixes the kinds."""
    v, f, _ = meshes()[name]
    lo, hi = mc.mesh_box(v, f)
    rng = np.random.default_rng(sum(map(ord, name)) + 7)
    c, e = (lo + hi) / 2, np.maximum(hi - lo, np.float32(0.5))
    used = v[np.unique(f)]
    parts = [used if name in BASE else used[:300]]
    parts.append(((v[f[:200, 0]] + v[f[:200, 1]]) * np.float32(0.5)).astype(np.float32))
    parts.append((((v[f[:200, 0]] + v[f[:200, 1]]) + v[f[:200, 2]]) / np.float32(3)).astype(np.float32))
    far = np.array([[(-1, 1)[(i >> k) & 1] for k in range(3)] for i in range(8)], np.float32)
    parts.append((c + far * 50 * e).astype(np.float32))
    parts.append((c + (rng.random((100, 3)) - 0.5) * 0.5 * e).astype(np.float32))
    parts.append((c + (rng.random((300, 3)) - 0.5) * 1.5 * e).astype(np.float32))
    if name == "cube":
        n = np.arange(-1, 6, dtype=np.float32)
        parts.append(np.stack(np.meshgrid(n, n, n, indexing="ij"), -1).reshape(-1, 3))
        parts.append(mc.cube_tie_lattice().reshape(-1, 3))
        parts.append(np.array([[2, 2, 2]], np.float32))
    q = np.concatenate(parts).astype(np.float32)
    q = np.concatenate([q, q[:20], q[-20:]])  # duplicated queries
    rng.shuffle(q[1:])
    q = np.ascontiguousarray(q)
    q.setflags(write=False)
    return q


# ---------------------------------------------------------------------------------------------------------------- the model
def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _clamp(x, lo, hi):
    t = np.where(x > lo, x, lo)
    return np.where(t < hi, t, hi)


def _edge(P0, P1, q):
    e, w = _sub(P1, P0), _sub(q, P0)
    ee, ew = _dot(e, e), _dot(e, w)
    t = np.where(ee > 0, _clamp(ew / ee, ZERO, ONE), ZERO)
    c = [np.where(t == 1, P1[k], P0[k] + t * e[k]) for k in range(3)]
    c = [_clamp(c[k], np.minimum(P0[k], P1[k]), np.maximum(P0[k], P1[k])) for k in range(3)]
    r = _sub(c, q)
    return _dot(r, r), c


def _face(A, B, C, q):
    d, best = _edge(A, B, q)
    sel = np.zeros(d.shape, np.int8)  # which candidate answered: 0, 1, 2 the edges (A,B), (A,C), (B,C), 3 the interior
    for j, (P0, P1) in enumerate(((A, C), (B, C))):
        dk, p = _edge(P0, P1, q)
        take = dk < d
        d = np.where(take, dk, d)
        sel = np.where(take, np.int8(j + 1), sel)
        best = [np.where(take, p[k], best[k]) for k in range(3)]
    ab, ac = _sub(B, A), _sub(C, A)
    n = _cross(ab, ac)
    nn = _dot(n, n)
    s0 = _dot(_cross(_sub(C, B), _sub(q, B)), n)
    s1 = _dot(_cross(_sub(A, C), _sub(q, C)), n)
    s2 = _dot(_cross(ab, _sub(q, A)), n)
    accepted = (nn > 0) & (s0 >= 0) & (s1 >= 0) & (s2 >= 0)
    k = np.where(nn > 0, _dot(n, _sub(q, A)) / nn, ZERO)
    p = [q[i] - k * n[i] for i in range(3)]
    p = [_clamp(p[i], np.minimum(np.minimum(A[i], B[i]), C[i]), np.maximum(np.maximum(A[i], B[i]), C[i])) for i in range(3)]
    r = _sub(p, q)
    dk = _dot(r, r)
    take = accepted & (dk < d)
    d = np.where(take, dk, d)
    sel = np.where(take, np.int8(3), sel)
    best = [np.where(take, p[i], best[i]) for i in range(3)]
    assert d.dtype == np.float32 and best[0].dtype == np.float32
    return d, best, sel


def model_pairs(v, f, q, with_candidate=False):
    """d [Q][F] float32 and c [Q][F][3] of every (query, face) pair (finite queries); ``with_candidate``: also which of the
    face's four candidates answered, int8 [Q][F]."""
    v, q = np.asarray(v, np.float32), np.asarray(q, np.float32)
    fs = np.sort(np.asarray(f), axis=1)  # A, B, C: the vertices in vertex-index order
    A, B, C = ([v[fs[:, k], c][None, :] for c in range(3)] for k in range(3))
    qq = [q[:, c][:, None] for c in range(3)]
    with np.errstate(all="ignore"):
        d, c, sel = _face(A, B, C, qq)
    return (d, np.stack(c, -1), sel) if with_candidate else (d, np.stack(c, -1))


def model_closest(v, f, q, chunk_elems=1 << 20):
    """(dist2 [Q] f32, face [Q] i32, point [Q,3] f32): the definition, brute force over all faces."""
    q = np.ascontiguousarray(q, np.float32)
    Q, F = len(q), len(f)
    assert F >= 1
    dist2, face, point = np.full(Q, np.inf, np.float32), np.full(Q, -1, np.int32), q.copy()
    with np.errstate(all="ignore"):
        idx = np.nonzero(np.all(np.abs(q) <= F32_MAX, axis=1))[0]
    rows = max(1, chunk_elems // F)
    ar = np.arange(F)
    for s in range(0, len(idx), rows):
        ii = idx[s:s + rows]
        d, c = model_pairs(v, f, q[ii])
        mn = d.min(1, keepdims=True)
        assert not np.isnan(mn).any()
        w = np.where(d == mn, ar[None, :], F).min(1)  # the lowest face index among equal d
        dist2[ii], face[ii], point[ii] = d[np.arange(len(ii)), w], w, c[np.arange(len(ii)), w]
    return dist2, face, point


@functools.lru_cache(maxsize=None)
def expected(name):
    """The model's answer on queries(name) followed by the non-finite set; computed once."""
    v, f, _ = meshes()[name]
    q = np.concatenate([queries(name), nonfinite_queries()])
    out = model_closest(v, f, q)
    for a in out:
        a.setflags(write=False)
    return (q,) + out


# ---------------------------------------------------------------------------------------------------------------- the truth
def truth_distance(v, f, q, chunk=256):
    """float64 distance to the mesh by Ericson's region classification, brute force."""
    v, q = np.asarray(v, np.float64), np.asarray(q, np.float64)
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    out = np.zeros(len(q))
    dot = lambda x, y: (x * y).sum(-1)  # noqa: E731
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
            vv, ww = vb / denom, vc / denom
            res = a + ab * vv[..., None] + ac * ww[..., None]                         # interior
            m = (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)                            # edge BC
            t = ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None]
            res = np.where(m[..., None], b + t * (c - b), res)
            m = (vb <= 0) & (d2 >= 0) & (d6 <= 0)                                          # edge AC
            res = np.where(m[..., None], a + (d2 / (d2 - d6))[..., None] * ac, res)
            m = (vc <= 0) & (d1 >= 0) & (d3 <= 0)                                          # edge AB
            res = np.where(m[..., None], a + (d1 / (d1 - d3))[..., None] * ab, res)
            res = np.where(((d6 >= 0) & (d5 <= d6))[..., None], c + 0 * p, res)            # vertex C
            res = np.where(((d3 >= 0) & (d4 <= d3))[..., None], b + 0 * p, res)            # vertex B
            res = np.where(((d1 <= 0) & (d2 <= 0))[..., None], a + 0 * p, res)             # vertex A
            dd = np.sqrt(dot(res - p, res - p))
            # a zero-area face has no regions (denom == 0): its three edges answer
            deg = ~np.isfinite(dd)
            if deg.any():
                def seg(p0, p1):
                    e = p1 - p0
                    ee = dot(e, e)
                    t = np.clip(np.where(ee > 0, dot(e, p - p0) / np.where(ee > 0, ee, 1), 0), 0, 1)[..., None]
                    r = p0 + t * e - p
                    return np.sqrt(dot(r, r))
                dd = np.where(deg, np.minimum(np.minimum(seg(a, b), seg(a, c)), seg(b, c)), dd)
            out[s:s + chunk] = dd.min(1)
    return out


def max_coord_diff(v, f, q):
    """E of the tolerance: the largest absolute coordinate difference between a query and a vertex of the mesh."""
    used = np.asarray(v, np.float64)[np.unique(f)]
    q = np.asarray(q, np.float64)
    return float(max(np.abs(q.max(0) - used.min(0)).max(), np.abs(used.max(0) - q.min(0)).max()))
