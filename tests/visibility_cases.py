"""Shared cases of the head-mesh visibility tests (csrc/ghr_visibility.h): the case meshes, views and masks, the numpy float32
MODEL of the definition (brute force over all faces, the expressions of ghr_visibility.h in their operand order) and a float64
TRUTH on the same float32 screen vertices, with the pixels at which float32 may legitimately decide otherwise marked FRAGILE.
Everything is computed once per process and handed out read-only."""
import functools
import os
import re

import numpy as np

from tests import mesh_cases as mc

F32 = np.float32
NEAR = F32(1e-3)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaussianhaircut_amd", "csrc", "ghr_visibility.h")


def header_constant(name):
    with open(HEADER) as fh:
        return int(re.search(r"^#define %s (\d+)" % name, fh.read(), re.M).group(1))


CHUNK = header_constant("GHR_VIS_CHUNK")
BIG_RECT = header_constant("GHR_VIS_BIG_RECT")
STACK_K = (1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
SIZES = ((1, 1), (15, 17), (16, 16), (17, 33), (48, 64), (130, 250))


# ---------------------------------------------------------------------------------------------------------------- views
def _look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """world-to-camera R, t of a camera at `eye` looking at `target`, x right, y down, z forward (OpenCV)"""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, -R @ eye


def _pinhole(H, W, focal=1.1):
    f = focal * max(H, W) / 2.0
    return np.array([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1.0]])


def _M(K, R, t):
    return np.ascontiguousarray((K @ np.concatenate([R, np.asarray(t, np.float64)[:, None]], 1)).astype(F32).reshape(12))


def view_front(H, W):
    return _M(_pinhole(H, W, 2.0), *_look_at((0.3, 0.2, 3.1), (0.0, 0.0, 0.0)))


def view_oblique(H, W):
    return _M(_pinhole(H, W, 1.7), *_look_at((1.9, 1.3, -1.6), (0.1, -0.05, 0.0), up=(0.1, 1.0, 0.2)))


def view_inside(H, W):
    return _M(_pinhole(H, W, 0.6), *_look_at((0.05, 0.02, 0.03), (0.4, 0.3, 1.0)))


def view_camera_space(H, W):
    """vertices are given in camera space: w = X2 exactly"""
    return _M(_pinhole(H, W, 1.0), np.eye(3), np.zeros(3))


def view_uv(H, W):
    """the affine view of scalp_uv_mask: x' = (W - 1) / 2 (u + 1) + 0.5, likewise y', w = 1"""
    return np.array([(W - 1) / 2.0, 0, 0, (W - 1) / 2.0 + 0.5, 0, (H - 1) / 2.0, 0, (H - 1) / 2.0 + 0.5, 0, 0, 0, 1], F32)


def view_pixels(H, W):
    """x' = 2 X0, y' = 2 X1, w = 1: a power-of-two scale, so that lattice vertices land exactly where they are put"""
    return np.array([2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 1], F32)


def view_screen_w(H, W):
    """x' = X0, y' = X1, w = X2: a vertex (sx w, sy w, w) projects to (sx, sy) at depth w"""
    return np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F32)


# ---------------------------------------------------------------------------------------------------------------- meshes
def lattice(n, shift):
    """(n + 1)^2 vertices two pixels apart under view_pixels, the first at pixel centre (2.5, 2.5) + shift; 2 n^2 faces with
    alternating diagonals and windings.  shift = 0: every vertex, every edge midpoint and every diagonal passes through pixel
    centres; shift = 0.5: the vertices sit on pixel corners and only the diagonals pass through centres."""
    v = [[(2 * a + 2.5 + shift) / 2, (2 * b + 2.5 + shift) / 2, 0.25 * ((a + b) % 3)] for b in range(n + 1) for a in range(n + 1)]
    f = []
    for b in range(n):
        for a in range(n):
            p, q, r, s = b * (n + 1) + a, b * (n + 1) + a + 1, (b + 1) * (n + 1) + a + 1, (b + 1) * (n + 1) + a
            if (a + b) % 2 == 0:
                f += [[p, q, r], [r, s, p] if a % 2 else [p, r, s]]
            else:
                f += [[p, q, s], [q, s, r] if b % 2 else [q, r, s]]
    return mc._f32(v), mc._i32(f)


def lattice_extent(n, shift):
    """the closed pixel-coordinate interval the lattice spans"""
    return 2.5 + shift, 2 * n + 2.5 + shift


def stack(K, duplicates):
    """K triangles over tile (1, 1) of view_screen_w (pixels 17 .. 30), behind one another at distinct depths -- or, with
    `duplicates`, one far triangle (face 0) and K identical copies of a nearer one (half of them through vertices of their own)."""
    tri = np.array([[17.3, 17.2], [30.6, 18.1], [18.4, 30.7]])
    v, f = [], []

    def add(w, jitter):
        b = len(v)
        for k in range(3):
            v.append([(tri[k, 0] + jitter) * w, (tri[k, 1] - jitter) * w, w])
        return b
    if duplicates:
        b = add(2.0, 0.0)
        f.append([b, b + 1, b + 2])
        b = add(1.5, 0.0)
        for i in range(K):
            if i % 2:
                b2 = add(1.5, 0.0)
                f.append([b2, b2 + 1, b2 + 2])
            else:
                f.append([b, b + 1, b + 2])
    else:
        order = np.random.default_rng(K).permutation(K)
        for i in range(K):
            b = add(1.0 + 0.01 * float(order[i]), 0.02 * (i % 7))
            f.append([b, b + 1, b + 2] if i % 2 == 0 else [b, b + 2, b + 1])
    return mc._f32(v), mc._i32(f)


def bad_faces():
    """A box in camera space (view_camera_space) and, around it, every kind of face that must not cover or that tests the
    binning: a repeated index, zero area, a vertex behind the camera, one exactly at w == near, one with a NaN, faces wholly off
    the screen on each side, indices outside the vertices, and one face whose box is larger than any image (behind the box)."""
    v, f = mc.box((-0.4, -0.3, 2.0), (0.5, 0.35, 2.8))
    v, f = [list(map(float, p)) for p in v], [list(map(int, t)) for t in f]

    def tri(p0, p1, p2):
        b = len(v)
        v.extend([list(p0), list(p1), list(p2)])
        f.append([b, b + 1, b + 2])
        return b
    b = tri((-0.2, -0.2, 1.5), (0.3, -0.1, 1.5), (0.0, 0.3, 1.5))
    f.append([b, b, b + 1])                                                  # a repeated index
    tri((-0.3, 0.11, 1.2), (0.0, 0.11, 1.2), (0.3, 0.11, 1.2))                 # zero area: one sy, so exactly flat in float32
    tri((-0.3, 0.2, 1.0), (0.3, 0.2, 1.0), (0.0, 0.1, -0.5))                   # a vertex behind the camera
    tri((-0.3, 0.2, 1.0), (0.3, 0.2, 1.0), (0.0, 0.0, float(NEAR)))            # a vertex exactly at w == near
    tri((-0.3, 0.2, 1.0), (0.3, 0.2, 1.0), (0.0, float("nan"), 1.0))           # a NaN
    tri((-9.0, -0.2, 1.0), (-8.0, 0.0, 1.0), (-8.5, 0.3, 1.0))                 # off-screen left
    tri((9.0, -0.2, 1.0), (8.0, 0.0, 1.0), (8.5, 0.3, 1.0))                    # right
    tri((-0.2, -9.0, 1.0), (0.0, -8.0, 1.0), (0.3, -8.5, 1.0))                 # above
    tri((-0.2, 9.0, 1.0), (0.0, 8.0, 1.0), (0.3, 8.5, 1.0))                    # below
    f.append([0, 1, 1000000])                                               # an index past the vertices
    f.append([-1, 1, 2])                                                     # a negative index
    tri((-50.0, -40.0, 4.0), (60.0, -45.0, 4.0), (5.0, 70.0, 4.0))             # a box larger than the image, behind the box
    tri((-0.45, -0.2, 1.9), (-0.1, -0.25, 1.9), (-0.3, 0.2, 1.9))              # and a small one in front of the box
    return mc._f32(v), mc._i32(f)


def uv_patch(n=7):
    """a jittered planar grid in [-0.9, 0.8]^2 (z = 0): the mesh of the affine UV view"""
    rng = np.random.default_rng(5)
    g = np.linspace(-0.9, 0.8, n + 1)
    v = [[g[a] + rng.uniform(-0.04, 0.04), g[b] + rng.uniform(-0.04, 0.04), 0.0] for b in range(n + 1) for a in range(n + 1)]
    f = []
    for b in range(n):
        for a in range(n):
            p, q, r, s = b * (n + 1) + a, b * (n + 1) + a + 1, (b + 1) * (n + 1) + a + 1, (b + 1) * (n + 1) + a
            f += [[p, q, r], [p, r, s]] if (a + b) % 2 else [[p, q, s], [q, r, s]]
    return mc._f32(v), mc._i32(f)


@functools.lru_cache(maxsize=None)
def meshes():
    out = {"box": mc.box((-0.6, -0.45, -0.5), (0.55, 0.5, 0.6)), "ico1": mc.icosphere(1), "ico2": mc.icosphere(2),
           "torus": mc.torus(24, 12), "uv_sphere": mc.uv_sphere(116, 44), "bad": bad_faces(), "uv_patch": uv_patch(),
           "latticeA": lattice(10, 0.0), "latticeB": lattice(10, 0.5)}
    for K in STACK_K:
        out["stack%d" % K] = stack(K, False)
        out["dups%d" % K] = stack(K, True)
    for v, f in out.values():
        v.setflags(write=False); f.setflags(write=False)
    return out


VIEWS = {"front": view_front, "oblique": view_oblique, "inside": view_inside, "camera": view_camera_space, "uv": view_uv,
         "pixels": view_pixels, "screen_w": view_screen_w}


def _case_table():
    """name -> (mesh, view, (H, W)); the mask kind follows from the position in the table"""
    t = []
    t += [("box", "front", s) for s in SIZES] + [("box", "oblique", (48, 64)), ("box", "inside", (48, 64))]
    t += [("ico1", "front", (15, 17)), ("ico1", "oblique", (130, 250)), ("ico1", "inside", (17, 33))]
    t += [("ico2", "front", (48, 64)), ("ico2", "oblique", (16, 16)), ("ico2", "inside", (130, 250))]
    t += [("torus", "front", (17, 33)), ("torus", "oblique", (48, 64)), ("torus", "inside", (15, 17))]
    t += [("uv_sphere", "front", (17, 33)), ("uv_sphere", "oblique", (15, 17))]
    t += [("bad", "camera", s) for s in ((1, 1), (17, 33), (48, 64), (130, 250))]
    t += [("uv_patch", "uv", s) for s in ((16, 16), (48, 64), (130, 250))]
    t += [(m, "pixels", s) for m in ("latticeA", "latticeB") for s in ((16, 16), (17, 33), (48, 64))]
    t += [("%s%d" % (kind, K), "screen_w", (48, 64)) for kind in ("stack", "dups") for K in STACK_K]
    return {"%s-%s-%dx%d" % (m, vw, s[0], s[1]): (m, vw, s) for m, vw, s in t}


CASES = _case_table()
MASK_KINDS = ("zeros", "full", "corners", "threshold", "blobs")
EXACT_ONLY = ("lattice", "dups")  # built from ties: not part of the comparison with the float64 truth


def masks(kind, H, W, seed=0):
    """(body, hair) uint8 [H, W]"""
    rng = np.random.default_rng(seed + 31 * H + W)
    body, hair = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    if kind == "full":
        body[:] = 255
    elif kind == "corners":      # one pixel lit in each corner and in the centre: the dilation's clipped window
        for i, j in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)):
            body[i, j] = 255
        hair[H - 1, W - 1] = 200
    elif kind == "threshold":    # 127 against 128
        body[:] = 127
        body[::5, ::7] = 128
        hair[:] = 0
        hair[H // 3:, W // 2:] = 127
        hair[H // 2, W // 2] = 128
    elif kind == "blobs":
        ii, jj = np.mgrid[0:H, 0:W]
        for plane, n in ((body, 5), (hair, 3)):
            for _ in range(n):
                ci, cj, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(1, max(2.0, 0.3 * max(H, W)))
                plane[(ii - ci) ** 2 + (jj - cj) ** 2 <= r * r] = rng.integers(100, 256)
    return body, hair


@functools.lru_cache(maxsize=None)
def case(name):
    """(vertices, faces, M, H, W, body, hair)"""
    m, vw, (H, W) = CASES[name]
    v, f = meshes()[m]
    kind = MASK_KINDS[list(CASES).index(name) % len(MASK_KINDS)]
    body, hair = masks(kind, H, W)
    M = VIEWS[vw](H, W)
    for a in (M, body, hair):
        a.setflags(write=False)
    return v, f, M, H, W, body, hair


# ---------------------------------------------------------------------------------------------------------------- the model
def model_project(v, M, near=NEAR):
    v, M = np.asarray(v, F32), np.asarray(M, F32)
    with np.errstate(all="ignore"):
        X = [v[:, c] for c in range(3)]
        xp = (M[0] * X[0] + M[1] * X[1]) + (M[2] * X[2] + M[3])
        yp = (M[4] * X[0] + M[5] * X[1]) + (M[6] * X[2] + M[7])
        w = (M[8] * X[0] + M[9] * X[1]) + (M[10] * X[2] + M[11])
        sx, sy, q = xp / w, yp / w, F32(1) / w
        valid = np.isfinite(w) & (w > F32(near))
    assert sx.dtype == F32 and q.dtype == F32
    return sx, sy, q, valid


def _face_tables(v, f, M, near):
    V = len(v)
    sx, sy, q, valid = model_project(v, M, near) if V else (np.zeros(1, F32),) * 3 + (np.zeros(1, bool),)
    in_range = ((f >= 0) & (f < V)).all(1)
    fi = np.where(in_range[:, None], f, 0)
    u, t, qq = [[a[fi[:, k]] for k in range(3)] for a in (sx, sy, q)]
    with np.errstate(all="ignore"):
        never = ~in_range | (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])
        never |= ~(valid[fi[:, 0]] & valid[fi[:, 1]] & valid[fi[:, 2]])
        never |= (u[1] - u[0]) * (t[2] - t[0]) - (t[1] - t[0]) * (u[2] - u[0]) == 0
    return u, t, qq, never


def model_rasterize(v, f, M, H, W, near=NEAR, chunk_elems=1 << 21, return_cover_count=False):
    """pix_to_face [H, W] int32 (and, on request, the number of faces that cover each pixel)"""
    f = np.asarray(f, np.int64).reshape(-1, 3)
    out = np.full(H * W, -1, np.int32)
    count = np.zeros(H * W, np.int32)
    Fc = len(f)
    if H * W and Fc and len(v):
        u, t, qq, never = _face_tables(v, f, M, near)
        with np.errstate(all="ignore"):
            ulo, uhi = np.fmin(np.fmin(u[0], u[1]), u[2]), np.fmax(np.fmax(u[0], u[1]), u[2])
            vlo, vhi = np.fmin(np.fmin(t[0], t[1]), t[2]), np.fmax(np.fmax(t[0], t[1]), t[2])
            chunk = max(1, chunk_elems // Fc)
            for s in range(0, H * W, chunk):
                p = np.arange(s, min(s + chunk, H * W))
                px = ((p % W).astype(F32) + F32(0.5))[:, None]
                py = ((p // W).astype(F32) + F32(0.5))[:, None]
                side, e = [], []
                for k in range(3):
                    k1 = (k + 1) % 3
                    flip = f[:, k] > f[:, k1]
                    au, av = np.where(flip, u[k1], u[k]), np.where(flip, t[k1], t[k])
                    bu, bv = np.where(flip, u[k], u[k1]), np.where(flip, t[k], t[k1])
                    dx, dy = bu - au, bv - av
                    E = dx * (py - av) - dy * (px - au)
                    assert E.dtype == F32
                    left = (E > 0) | ((E == 0) & ((dy < 0) | ((dy == 0) & (dx > 0))))
                    side.append(left != flip)
                    e.append(np.where(flip, -E, E))
                d = ((e[1] * qq[0] + e[2] * qq[1]) + e[0] * qq[2]) / ((e[0] + e[1]) + e[2])
                assert d.dtype == F32
                in_box = (px >= ulo) & (px <= uhi) & (py >= vlo) & (py <= vhi)
                covers = ~never & in_box & (side[0] == side[1]) & (side[1] == side[2])
                count[p] = covers.sum(1)
                d = np.where(covers & ~np.isnan(d), d, F32(-np.inf))
                best = d.argmax(1)              # (numpy: the FIRST maximum, i.e. the lowest index among equals)
                out[p] = np.where(d[np.arange(len(p)), best] > F32(-np.inf), best, -1)
    out = out.reshape(H, W)
    return (out, count.reshape(H, W)) if return_cover_count else out


def model_head(body, hair):
    H, W = body.shape

    def dil(a):
        p = np.zeros((H + 4, W + 4), np.uint8)
        p[2:H + 2, 2:W + 2] = a
        return np.max([p[di:di + H, dj:dj + W] for di in range(5) for dj in range(5)], axis=0)
    return (dil(body) >= 128) & ~(dil(hair) >= 128)


def model_view(v, f, M, H, W, body=None, hair=None, near=NEAR):
    """(pix_to_face, vis uint8, seen bool [V], seen_head bool [V], head bool [H, W])"""
    pix = model_rasterize(v, f, M, H, W, near)
    head = model_head(body, hair) if body is not None else np.zeros((H, W), bool)
    won = pix >= 0
    seen, seen_head = np.zeros(len(v), bool), np.zeros(len(v), bool)
    f = np.asarray(f).reshape(-1, 3)
    seen[np.unique(f[np.unique(pix[won])])] = True
    seen_head[np.unique(f[np.unique(pix[won & head])])] = True
    return pix, np.where(won & head, 255, 0).astype(np.uint8), seen, seen_head, head


@functools.lru_cache(maxsize=None)
def model_case(name):
    out = model_view(*case(name))
    for a in out:
        a.setflags(write=False)
    return out


def model_vertex_mask(cnt, cnt_head, n_views, prob_thr=0.5, n_views_thr=0.1):
    with np.errstate(all="ignore"):
        c, ch = np.asarray(cnt).astype(F32), np.asarray(cnt_head).astype(F32)
        return (F32(1) - ch / c > F32(prob_thr)) | (c / F32(n_views) < F32(n_views_thr))


# ---------------------------------------------------------------------------------------------------------------- the truth
def truth_rasterize(v, f, M, H, W, near=NEAR, chunk_elems=1 << 21):
    """float64 on the model's float32 screen vertices: (pix_to_face, fragile bool [H, W]).  A pixel is fragile when, for a face
    whose box holds it, a double edge value lies within 2^-20 (|dx| + |dy|) x the face's extent of 0, or when the two largest
    inverse depths are within 4 float32 ulp of each other."""
    f = np.asarray(f, np.int64).reshape(-1, 3)
    out, fragile = np.full(H * W, -1, np.int32), np.zeros(H * W, bool)
    Fc = len(f)
    if H * W and Fc and len(v):
        u, t, qq, never = _face_tables(v, f, M, near)
        with np.errstate(all="ignore"):
            u, t, qq = [[a.astype(np.float64) for a in x] for x in (u, t, qq)]
            ulo, uhi = np.fmin(np.fmin(u[0], u[1]), u[2]), np.fmax(np.fmax(u[0], u[1]), u[2])
            vlo, vhi = np.fmin(np.fmin(t[0], t[1]), t[2]), np.fmax(np.fmax(t[0], t[1]), t[2])
            extent = np.maximum(uhi - ulo, vhi - vlo)
            chunk = max(1, chunk_elems // Fc)
            for s in range(0, H * W, chunk):
                p = np.arange(s, min(s + chunk, H * W))
                px, py = ((p % W) + 0.5)[:, None], ((p // W) + 0.5)[:, None]
                in_box = ~never & (px >= ulo) & (px <= uhi) & (py >= vlo) & (py <= vhi)
                e, near0 = [], np.zeros((len(p), Fc), bool)
                for k in range(3):
                    k1 = (k + 1) % 3
                    dx, dy = u[k1] - u[k], t[k1] - t[k]
                    E = dx * (py - t[k]) - dy * (px - u[k])
                    near0 |= np.abs(E) <= 2.0 ** -20 * (np.abs(dx) + np.abs(dy)) * extent
                    e.append(E)
                covers = in_box & (((e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)) | ((e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0)))
                d = ((e[1] * qq[0] + e[2] * qq[1]) + e[0] * qq[2]) / ((e[0] + e[1]) + e[2])
                d = np.where(covers & ~np.isnan(d), d, -np.inf)
                order = np.sort(d, axis=1)
                top, second = order[:, -1], (order[:, -2] if Fc > 1 else np.full(len(p), -np.inf))
                best = d.argmax(1)
                out[p] = np.where(top > -np.inf, best, -1)
                close = np.isfinite(second) & (top - second <= 4 * np.spacing(np.abs(top).astype(F32)).astype(np.float64))
                fragile[p] = (in_box & near0).any(1) | close
    return out.reshape(H, W), fragile.reshape(H, W)
