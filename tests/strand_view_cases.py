"""Shared cases of the strand-preview tests (csrc/ghr_strandview.h): the case strands, meshes and views, the numpy float32 MODEL
of the definition (brute force over all segments, the expressions of ghr_strandview.h in their operand order) and a float64 TRUTH
on the same float32 screen points, with the pixels at which float32 may legitimately decide otherwise marked FRAGILE.
Everything is computed once per process and handed out read-only."""
import functools
import os
import re

import numpy as np

from gaussianhaircut_amd import visibility as vis
from tests import mesh_cases as mc
from tests import visibility_cases as vc
from tests.visibility_cases import view_front, view_inside, view_oblique, view_pixels, view_screen_w

F32 = np.float32
NEAR = vc.NEAR
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaussianhaircut_amd", "csrc", "ghr_strandview.h")


def header_constant(name):
    with open(HEADER) as fh:
        return int(re.search(r"^#define %s (\d+)" % name, fh.read(), re.M).group(1))


CHUNK = header_constant("GHR_SV_CHUNK")
BIG_RECT = header_constant("GHR_SV_BIG_RECT")
STACK_K = (1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
SIZES = ((1, 1), (15, 17), (16, 16), (17, 33), (48, 64), (130, 250))
RADII = (0.5, 0.75, 2.5)
KAJIYA, TANGENT = 0, 1
LIGHT_CAMERA = (0.45, -0.60, -0.66)
DEFAULTS = dict(ambient=0.25, kd=0.65, ks=0.35, shininess_log2=5, base_rgb=(0.45, 0.30, 0.18), head_rgb=(0.62, 0.62, 0.62),
                background_rgb=(1.0, 1.0, 1.0))
VIEWS = {"front": view_front, "oblique": view_oblique, "inside": view_inside, "pixels": view_pixels, "screen_w": view_screen_w}


def shading(M, **kw):
    """the constants of a picture as float32 (eye and light in double, rounded once); affine views have no eye: one is given"""
    M3 = np.asarray(M, np.float64).reshape(3, 4)
    lc = np.asarray(LIGHT_CAMERA, np.float64)
    lc = lc / np.linalg.norm(lc)
    if abs(np.linalg.det(M3[:, :3])) > 1e-9:
        _, R, t = vis.decompose_projection(M3)
        eye, light = -R.T @ t, R.T @ lc
    else:
        eye, light = np.array([7.3, -4.1, -30.0]), lc
    light = light / np.linalg.norm(light)
    d = dict(DEFAULTS, **kw)
    f3 = lambda x: np.asarray(x, np.float64).astype(F32)  # noqa: E731
    return dict(eye=f3(eye), light=f3(light), ambient=F32(d["ambient"]), kd=F32(d["kd"]), ks=F32(d["ks"]),
                shininess_log2=int(d["shininess_log2"]), base_rgb=f3(d["base_rgb"]), head_rgb=f3(d["head_rgb"]),
                background_rgb=f3(d["background_rgb"]))


# ---------------------------------------------------------------------------------------------------------------- strands
def _pts(a):
    return np.ascontiguousarray(np.asarray(a, np.float64).astype(F32))


def from_pixels(sxy):
    """[S, L, 2] screen positions on the half-pixel lattice -> world points of view_pixels (x' = 2 X0: exact), all at w = 1"""
    sxy = np.asarray(sxy, np.float64)
    return _pts(np.concatenate([sxy / 2, np.zeros(sxy.shape[:-1] + (1,))], -1))


def from_screen_w(sx, sy, w):
    """world points of view_screen_w: (sx w, sy w, w)"""
    sx, sy, w = np.broadcast_arrays(np.asarray(sx, np.float64), np.asarray(sy, np.float64), np.asarray(w, np.float64))
    return _pts(np.stack([sx * w, sy * w, w], -1))


def singles(H, W):
    """four strands of one segment each on the lattice: horizontal (centres at distance exactly 0.5 and 2.5 above and below it),
    vertical (it leaves the image at the bottom), diagonal, and a zero-length one (a disc); all at w = 1: ties go to the lowest k"""
    n = float(min(H, W))
    return from_pixels([[[2.0, 3.0], [W - 1.0, 3.0]], [[5.0, 1.0], [5.0, H + 3.0]], [[1.0, 1.0], [n + 2.0, n + 2.0]],
                        [[W // 2 + 0.5, H // 2 + 0.5], [W // 2 + 0.5, H // 2 + 0.5]]])


def dropped():
    """view_screen_w, L = 4: a point behind the camera, one exactly at w == near, one NaN coordinate -- every segment that touches
    them is dropped whole -- and an untouched strand behind them all"""
    sx = np.array([[5.3, 20.1, 40.7, 60.2], [4.1, 22.3, 41.9, 59.5], [6.2, 21.4, 43.3, 61.8], [3.0, 25.0, 45.0, 62.0]])
    sy = np.array([[6.1, 9.3, 12.2, 15.4], [20.2, 22.1, 24.3, 26.6], [33.3, 35.2, 37.4, 39.1], [5.0, 18.0, 30.0, 44.0]])
    w = np.array([[1.0, -0.5, 1.2, 1.1], [1.0, 1.1, float(NEAR), 1.3], [1.0, 1.1, 1.2, 1.3], [2.0, 2.1, 2.2, 2.3]])
    p = from_screen_w(sx, sy, w)
    p[1, 2] = [41.9 * float(NEAR), 24.3 * float(NEAR), float(NEAR)]
    p[2, 1, 1] = np.nan
    return p


def stack(K, duplicates):
    """K one-segment strands over tile (1, 1) of view_screen_w (pixels 17 .. 30) at distinct depths in a shuffled order -- or, with
    `duplicates`, one far segment (strand 0) and K identical copies of a nearer one"""
    if duplicates:
        a = [[17.4, 18.3, 2.0], [30.2, 29.6, 2.0]]
        b = [[17.4, 18.3, 1.5], [30.2, 29.6, 1.5]]
        seg = np.array([a] + [b] * K)
    else:
        order = np.random.default_rng(K).permutation(K)
        seg = np.array([[[17.4 + 0.02 * (i % 7), 18.3 + 0.3 * (i % 5), 1.0 + 0.01 * order[i]],
                         [30.2 - 0.02 * (i % 7), 29.6 - 0.3 * (i % 3), 1.0 + 0.01 * order[i]]] for i in range(K)])
    return from_screen_w(seg[..., 0], seg[..., 1], seg[..., 2])


def long_and_short(H, W):
    """one segment across the whole image (more tiles than BIG_RECT) in front of a row of short ones, and one behind them"""
    rng = np.random.default_rng(3)
    n = 24
    cx, cy = rng.uniform(4, W - 4, n), rng.uniform(4, H - 4, n)
    a = rng.uniform(0, np.pi, n)
    short = np.stack([np.stack([cx - 3 * np.cos(a), cy - 3 * np.sin(a), np.full(n, 1.5)], -1),
                      np.stack([cx + 3 * np.cos(a), cy + 3 * np.sin(a), np.full(n, 1.6)], -1)], 1)
    long1 = np.array([[[3.3, 5.2, 1.0], [W - 4.6, H - 9.7, 1.2]]])
    long2 = np.array([[[2.1, H - 3.4, 3.0], [W - 2.2, 4.8, 2.5]]])
    seg = np.concatenate([short[:n // 2], long1, short[n // 2:], long2])
    return from_screen_w(seg[..., 0], seg[..., 1], seg[..., 2])


def hair(S, L, seed, radius=1.0, through=True):
    """strands that grow from a sphere of `radius` about the origin: outwards with a curl (their roots ON the sphere), a few straight
    through it, and a few that start inside"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(S, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    side = np.cross(d, rng.normal(size=(S, 3)))
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    u = np.linspace(0.0, 1.0, L)[None, :, None]
    length = rng.uniform(0.3, 0.9, (S, 1, 1))
    p = d[:, None] * (radius + length * u) + side[:, None] * (0.25 * length * np.sin(5.0 * u + rng.uniform(0, 6, (S, 1, 1))) * u)
    if through:
        k = max(1, S // 6)
        p[:k] = d[:k, None] * (radius * 1.3) * (2 * u - 1) + side[:k, None] * 0.31   # chords through the sphere
        p[k:2 * k] = d[k:2 * k, None] * (radius * (0.4 + 0.9 * u))                   # from inside to outside
    return _pts(p)


@functools.lru_cache(maxsize=None)
def meshes():
    out = {"sphere": mc.uv_sphere(116, 44), "small_sphere": mc.uv_sphere(24, 10)}
    for v, f in out.values():
        v.setflags(write=False); f.setflags(write=False)
    return out


def _case_table():
    """name -> dict(points, view, H, W, r, bias, mesh, s, mode, colors)"""
    t = {}

    def add(name, points, view, size, r=0.75, bias=0.0, mesh=None, s=1, mode=KAJIYA, colors=None):
        assert name not in t, name
        t[name] = dict(points=points, view=view, H=size[0], W=size[1], r=r, bias=bias, mesh=mesh, s=s, mode=mode, colors=colors)
    for k, size in enumerate(SIZES):
        for r in RADII:
            add("singles-%dx%d-r%g" % (size + (r,)), lambda size=size: singles(*size), "pixels", size, r=r, mode=(k + int(r)) % 2,
                colors="per" if k % 2 else None)
    for size in ((17, 33), (48, 64)):
        add("dropped-%dx%d" % size, dropped, "screen_w", size, r=2.5 if size[0] == 48 else 0.75)
    for size in ((1, 1), (16, 16)):
        add("empty-%dx%d" % size, lambda: np.zeros((0, 5, 3), F32), "front", size, mesh="small_sphere" if size[0] == 16 else None)
    for K in STACK_K:
        add("stack%d" % K, lambda K=K: stack(K, False), "screen_w", (48, 64), r=0.75, mode=TANGENT)
        add("dups%d" % K, lambda K=K: stack(K, True), "screen_w", (48, 64), r=0.5)
    add("long-130x250", lambda: long_and_short(130, 250), "screen_w", (130, 250), r=0.75, colors="per")
    add("long-48x64", lambda: long_and_short(48, 64), "screen_w", (48, 64), r=2.5)
    add("hair-front-130x250", lambda: hair(16, 100, 1), "front", (130, 250), r=0.75, mesh="small_sphere", colors="per")
    add("hair-oblique-130x250", lambda: hair(12, 100, 2), "oblique", (130, 250), r=0.5, bias=0.05, mesh="small_sphere", mode=TANGENT)
    add("hair-inside-48x64", lambda: hair(24, 12, 3), "inside", (48, 64), r=2.5)
    add("hair-front-48x64", lambda: hair(30, 20, 4), "front", (48, 64), r=0.75, mesh="sphere")
    add("hair-front-48x64-bias", lambda: hair(30, 20, 4), "front", (48, 64), r=0.75, bias=0.05, mesh="sphere", colors="one")
    add("hair-front-48x64-nomesh", lambda: hair(30, 20, 4), "front", (48, 64), r=0.75)
    add("hair-oblique-17x33", lambda: hair(20, 2, 5), "oblique", (17, 33), r=0.5, mesh="sphere")
    add("hair-front-15x17", lambda: hair(12, 3, 6), "front", (15, 17), r=0.75, mesh="small_sphere", bias=0.05)
    add("hair-front-16x16", lambda: hair(12, 7, 7), "front", (16, 16), r=2.5, mesh="small_sphere", mode=TANGENT)
    add("hair-front-1x1", lambda: hair(12, 7, 8), "front", (1, 1), r=0.75, mesh="small_sphere")
    for s in (1, 2, 4):
        add("ss%d-17x33" % s, lambda: hair(24, 16, 9), "front", (17, 33), r=0.75, mesh="small_sphere", s=s,
            colors="per" if s == 2 else None)
        add("ss%d-tangent-17x33" % s, lambda: hair(24, 16, 9), "oblique", (17, 33), r=0.75, mesh="small_sphere", s=s, mode=TANGENT)
    return t


_TABLE = _case_table()
CASES = list(_TABLE)
EXACT_ONLY = ("singles", "dups", "empty")  # built from ties (or empty): not part of the comparison with the float64 truth


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: points [S, L, 3], M, H, W, r, bias, v, f (or None), s, mode, base ([S, 3] or None), sh (the shading constants)"""
    c = dict(_TABLE[name])
    c["points"] = np.ascontiguousarray(c["points"]())
    c["M"] = VIEWS[c["view"]](c["H"], c["W"])
    c["v"], c["f"] = meshes()[c["mesh"]] if c["mesh"] else (None, None)
    S = len(c["points"])
    kw = {}
    c["base"] = None
    if c["colors"] == "per":
        c["base"] = np.ascontiguousarray(np.random.default_rng(S).uniform(0.05, 0.95, (S, 3)).astype(F32))
    elif c["colors"] == "one":
        kw["base_rgb"] = (0.7, 0.55, 0.2)
    c["sh"] = shading(c["M"], **kw)
    for a in (c["points"], c["M"], c["base"]):
        if a is not None:
            a.setflags(write=False)
    return c


def supersampled(M, r, s):
    Ms = np.array(M, F32)
    Ms[:8] *= F32(s)
    return Ms, F32(r) * F32(s)


# ---------------------------------------------------------------------------------------------------------------- the model
def _segments(points, M, near):
    S, L = points.shape[:2]
    sx, sy, q, valid = vc.model_project(points.reshape(-1, 3), M, near) if S else ((np.zeros(0, F32),) * 3 + (np.zeros(0, bool),))
    sx, sy, q, valid = (a.reshape(S, L) for a in (sx, sy, q, valid))
    fl = lambda a: (a[:, :-1].reshape(-1), a[:, 1:].reshape(-1))  # noqa: E731
    (ax, bx), (ay, by), (qa, qb), (va, vb) = fl(sx), fl(sy), fl(q), fl(valid)
    return ax, ay, bx, by, qa, qb, va & vb


def model_face_depth(v, f, M, H, W, pix, near=NEAR):
    """qf [H, W] float32: 8h's inverse depth of face pix[p] at the centre of p, 0 where there is none"""
    out = np.zeros(H * W, F32)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    face = pix.reshape(-1).astype(np.int64)
    on = np.nonzero((face >= 0) & (face < len(f)))[0]
    if len(on) == 0 or len(v) == 0:
        return out.reshape(H, W)
    t = f[face[on]]
    u, w_, q, never = vc._face_tables(v, t, M, near)
    px, py = ((on % W).astype(F32) + F32(0.5)), ((on // W).astype(F32) + F32(0.5))
    with np.errstate(all="ignore"):
        side, e = [], []
        for k in range(3):
            k1 = (k + 1) % 3
            flip = t[:, k] > t[:, k1]
            au, av = np.where(flip, u[k1], u[k]), np.where(flip, w_[k1], w_[k])
            bu, bv = np.where(flip, u[k], u[k1]), np.where(flip, w_[k], w_[k1])
            dx, dy = bu - au, bv - av
            E = dx * (py - av) - dy * (px - au)
            assert E.dtype == F32
            left = (E > 0) | ((E == 0) & ((dy < 0) | ((dy == 0) & (dx > 0))))
            side.append(left != flip)
            e.append(np.where(flip, -E, E))
        d = ((e[1] * q[0] + e[2] * q[1]) + e[0] * q[2]) / ((e[0] + e[1]) + e[2])
        assert d.dtype == F32
        ulo, uhi = np.fmin(np.fmin(u[0], u[1]), u[2]), np.fmax(np.fmax(u[0], u[1]), u[2])
        vlo, vhi = np.fmin(np.fmin(w_[0], w_[1]), w_[2]), np.fmax(np.fmax(w_[0], w_[1]), w_[2])
        covers = ~never & (px >= ulo) & (px <= uhi) & (py >= vlo) & (py <= vhi) & (side[0] == side[1]) & (side[1] == side[2]) & (d > 0)
    out[on] = np.where(covers, d, F32(0))
    return out.reshape(H, W)


def model_strand_winner(points, M, H, W, r, near=NEAR, chunk_elems=1 << 21, return_cover_count=False):
    """(k int32, t, qs) [H, W] of the strand winner alone (-1, 0, 0 where none)"""
    N = H * W
    seg, tt, qq, count = np.full(N, -1, np.int32), np.zeros(N, F32), np.zeros(N, F32), np.zeros(N, np.int32)
    ax, ay, bx, by, qa, qb, exists = _segments(points, M, near)
    K = len(ax)
    if N and K:
        r = F32(r)
        with np.errstate(all="ignore"):
            ulo, uhi, vlo, vhi = np.fmin(ax, bx) - r, np.fmax(ax, bx) + r, np.fmin(ay, by) - r, np.fmax(ay, by) + r
            dx, dy, dq = bx - ax, by - ay, qb - qa
            len2 = dx * dx + dy * dy
            chunk = max(1, chunk_elems // K)
            for s0 in range(0, N, chunk):
                p = np.arange(s0, min(s0 + chunk, N))
                px = ((p % W).astype(F32) + F32(0.5))[:, None]
                py = ((p // W).astype(F32) + F32(0.5))[:, None]
                t = ((px - ax) * dx + (py - ay) * dy) / len2
                t = np.fmin(np.fmax(t, F32(0)), F32(1))
                t = np.where((len2 == 0) | np.isnan(t), F32(0), t)
                ex, ey = px - (ax + t * dx), py - (ay + t * dy)
                d2 = ex * ex + ey * ey
                assert t.dtype == F32 and d2.dtype == F32
                covers = exists & (px >= ulo) & (px <= uhi) & (py >= vlo) & (py <= vhi) & (d2 <= r * r)
                count[p] = covers.sum(1)
                qs = qa + t * dq
                assert qs.dtype == F32
                qs = np.where(covers & (qs > 0), qs, F32(0))
                best = qs.argmax(1)              # (numpy: the FIRST maximum, i.e. the lowest index among equals)
                top = qs[np.arange(len(p)), best]
                won = top > 0
                seg[p] = np.where(won, best, -1)
                tt[p] = np.where(won, t[np.arange(len(p)), best], F32(0))
                qq[p] = np.where(won, top, F32(0))
    out = seg.reshape(H, W), tt.reshape(H, W), qq.reshape(H, W)
    return out + (count.reshape(H, W),) if return_cover_count else out


def model_head_test(seg, tt, qq, pix, qf, bias):
    """the four output planes from the strand winner and the head"""
    if pix is None:
        pix, qf = np.full(seg.shape, -1, np.int32), np.zeros(seg.shape, F32)
    has_face = qf > 0
    with np.errstate(all="ignore"):
        lifted = qq * (F32(1) + F32(bias))
    assert lifted.dtype == F32
    kept = (seg >= 0) & (~has_face | (lifted >= qf))
    head = ~kept & has_face
    return (np.where(kept, seg, -1).astype(np.int32), np.where(kept, tt, F32(0)), np.where(head, pix, -1).astype(np.int32),
            np.where(kept, qq, np.where(head, qf, F32(0))))


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _normalise(x):
    with np.errstate(all="ignore"):
        ln = np.sqrt(_dot(x, x))
        assert ln.dtype == F32
        return [np.where(ln == 0, F32(0), c / ln) for c in x]


def _quant8(x):
    with np.errstate(all="ignore"):
        x = np.fmin(np.fmax(x, F32(0)), F32(1))
        y = np.fmin(np.fmax(x * F32(255) + F32(0.5), F32(0)), F32(255))
    assert y.dtype == F32
    return y.astype(np.uint8)


def model_shade(points, v, f, seg, face, mode, sh, base=None):
    """uint8 [H, W, 3]"""
    H, W = seg.shape
    S, L = points.shape[:2]
    out = np.empty((H * W, 3), np.uint8)
    out[:] = _quant8(sh["background_rgb"])
    seg, face = seg.reshape(-1), face.reshape(-1)
    on = np.nonzero(seg >= 0)[0]
    light = [sh["light"][c] for c in range(3)]
    with np.errstate(all="ignore"):
        if len(on):
            s, i = seg[on] // (L - 1), seg[on] % (L - 1)
            A, B = points[s, i], points[s, i + 1]
            T = _normalise([B[:, c] - A[:, c] for c in range(3)])
            if mode == TANGENT:
                col = [F32(0.5) + F32(0.5) * T[c] for c in range(3)]
            else:
                Vn = _normalise([sh["eye"][c] - F32(0.5) * (A[:, c] + B[:, c]) for c in range(3)])
                cl, cv = _dot(T, light), _dot(T, Vn)
                sl, sv = np.sqrt(np.fmax(F32(0), F32(1) - cl * cl)), np.sqrt(np.fmax(F32(0), F32(1) - cv * cv))
                spec = np.fmax(F32(0), cl * cv + sl * sv)
                for _ in range(sh["shininess_log2"]):
                    spec = spec * spec
                assert spec.dtype == F32
                b = base[s] if base is not None else np.broadcast_to(sh["base_rgb"], (len(on), 3))
                col = [b[:, c] * (sh["ambient"] + sh["kd"] * sl) + sh["ks"] * spec for c in range(3)]
            assert col[0].dtype == F32
            out[on] = np.stack([_quant8(c) for c in col], 1)
        on = np.nonzero((seg < 0) & (face >= 0))[0]
        if len(on):
            t = np.asarray(f, np.int64).reshape(-1, 3)[face[on]]
            v0, v1, v2 = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
            e1, e2 = [v1[:, c] - v0[:, c] for c in range(3)], [v2[:, c] - v0[:, c] for c in range(3)]
            n = _normalise([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
            c = _dot(n, light)
            lit = sh["ambient"] + sh["kd"] * np.fmax(c, -c)
            assert lit.dtype == F32
            out[on] = np.stack([_quant8(sh["head_rgb"][k] * lit) for k in range(3)], 1)
    return out.reshape(H, W, 3)


def model_resolve(src, s):
    Hs, Ws, _ = src.shape
    x = src.reshape(Hs // s, s, Ws // s, s, 3).astype(np.int64).sum((1, 3))
    return ((x + (s * s) // 2) // (s * s)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _mesh_planes(mesh, view, H, W, s):
    """(pix_to_face, qf) of a mesh under a view's s-times finer grid: shared among the cases that differ in the strands only"""
    v, f = meshes()[mesh]
    Ms, _ = supersampled(VIEWS[view](H, W), 1.0, s)
    pix = vc.model_rasterize(v, f, Ms, s * H, s * W, NEAR)
    qf = model_face_depth(v, f, Ms, s * H, s * W, pix)
    pix.setflags(write=False); qf.setflags(write=False)
    return pix, qf


@functools.lru_cache(maxsize=None)
def model_frame(name, s=1):
    """the model of one case on the s-times finer grid: dict(M, r, H, W, pix, qf, winner (k, t, qs), planes (four), rgb)"""
    c = case(name)
    Ms, rs = supersampled(c["M"], c["r"], s)
    H, W = s * c["H"], s * c["W"]
    pix, qf = _mesh_planes(c["mesh"], c["view"], c["H"], c["W"], s) if c["mesh"] else (None, None)
    winner = model_strand_winner(c["points"], Ms, H, W, rs)
    planes = model_head_test(*winner, pix, qf, c["bias"])
    rgb = model_shade(c["points"], c["v"], c["f"], planes[0], planes[2], c["mode"], c["sh"], c["base"])
    out = dict(M=Ms, r=float(rs), H=H, W=W, pix=pix, qf=qf, winner=winner, planes=planes, rgb=rgb)
    for a in (Ms, rgb) + planes + winner:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def model_picture(name):
    """uint8 [H, W, 3]: the case's picture at its own supersampling"""
    s = case(name)["s"]
    out = model_resolve(model_frame(name, s)["rgb"], s)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------- the truth
def truth_frame(name, chunk_elems=1 << 21):
    """float64 on the model's float32 screen points and the model's qf: (pix_to_segment, pix_to_face_out, fragile bool [H, W]).
    A pixel is fragile when, for an existing segment, |dist^2 - r^2| is within 2^-20 of the operands' magnitude
    r (r + 1 + |ax| + |ay| + |bx| + |by|) -- the rounding of e is a few ulp of the screen coordinates, and dist^2 moves by 2 r of it --, when the two largest qs are within 4 float32 ulp of each other, or when
    qs (1 + bias) and qf are."""
    c, m = case(name), model_frame(name)
    H, W, r, N = c["H"], c["W"], float(F32(c["r"])), c["H"] * c["W"]
    seg, fragile, top_q = np.full(N, -1, np.int32), np.zeros(N, bool), np.zeros(N)
    ax, ay, bx, by, qa, qb, exists = (a.astype(np.float64) if a.dtype == F32 else a for a in _segments(c["points"], c["M"], NEAR))
    K = len(ax)
    ulp4 = lambda x: 4 * np.spacing(np.abs(x).astype(F32)).astype(np.float64)  # noqa: E731
    if N and K:
        with np.errstate(all="ignore"):
            dx, dy = bx - ax, by - ay
            len2 = dx * dx + dy * dy
            mag = r * (r + 1.0 + np.abs(ax) + np.abs(ay) + np.abs(bx) + np.abs(by))
            chunk = max(1, chunk_elems // K)
            for s0 in range(0, N, chunk):
                p = np.arange(s0, min(s0 + chunk, N))
                px, py = ((p % W) + 0.5)[:, None], ((p // W) + 0.5)[:, None]
                t = np.where(len2 == 0, 0.0, np.clip(((px - ax) * dx + (py - ay) * dy) / np.where(len2 == 0, 1.0, len2), 0.0, 1.0))
                ex, ey = px - (ax + t * dx), py - (ay + t * dy)
                d2 = ex * ex + ey * ey
                covers = exists & (d2 <= r * r)
                near_edge = exists & (np.abs(d2 - r * r) <= 2.0 ** -20 * mag)
                qs = np.where(covers, qa + t * (qb - qa), 0.0)
                qs = np.where(qs > 0, qs, 0.0)
                order = np.sort(qs, axis=1)
                top, second = order[:, -1], (order[:, -2] if K > 1 else np.zeros(len(p)))
                best = qs.argmax(1)
                seg[p] = np.where(top > 0, best, -1)
                top_q[p] = top
                fragile[p] = near_edge.any(1) | ((second > 0) & (top - second <= ulp4(top)))
    seg, fragile, top_q = seg.reshape(H, W), fragile.reshape(H, W), top_q.reshape(H, W)
    if m["pix"] is not None:
        pix, qf = m["pix"], m["qf"].astype(np.float64)
        lifted = top_q * (1.0 + float(F32(c["bias"])))
        has_face = qf > 0
        kept = (seg >= 0) & (~has_face | (lifted >= qf))
        fragile |= (seg >= 0) & has_face & (np.abs(lifted - qf) <= ulp4(qf))
        face = np.where(~kept & has_face, pix, -1).astype(np.int32)
        seg = np.where(kept, seg, -1).astype(np.int32)
    else:
        face = np.full((H, W), -1, np.int32)
    return seg, face, fragile
