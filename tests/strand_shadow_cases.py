"""Shared cases of the self-shadowing tests (csrc/ghr_strandview.h, "Self-shadowing"): the numpy float32 MODEL of
the deep opacity map, of its lookup and of the shadowed shading (brute force over all segments, the header's expressions in their
operand order), the hand-derived ladder, the light maps every form is held to, and the frames (a camera view over a light view).
Everything is computed once per process and handed out read-only."""
import functools

import numpy as np

from tests import strand_view_cases as sc
from tests import visibility_cases as vc

F32 = np.float32
NEAR = sc.NEAR
CHUNK = sc.CHUNK
STACK_K = sc.STACK_K
LIGHT_SIZES = ((1, 1), (16, 16), (17, 33), (40, 48))
LIGHT_RADII = (0.5, 1.0, 2.5)
KAPPA, BIAS = 0.2, 0.02   # the header's defaults


# ---------------------------------------------------------------------------------------------------------------- the model
def model_opacity(points, Ml, Hl, Wl, rl, layer, near=NEAR, chunk_elems=1 << 21):
    """(q0 float32 [Hl, Wl], layers uint32 [Hl, Wl, 4])"""
    N = Hl * Wl
    q0, layers = np.zeros(N, F32), np.zeros((N, 4), np.uint32)
    ax, ay, bx, by, qa, qb, exists = sc._segments(points, np.asarray(Ml, F32).reshape(12), near)
    K = len(ax)
    if N and K:
        r, d = F32(rl), F32(layer)
        with np.errstate(all="ignore"):
            ulo, uhi, vlo, vhi = np.fmin(ax, bx) - r, np.fmax(ax, bx) + r, np.fmin(ay, by) - r, np.fmax(ay, by) + r
            dx, dy, dq = bx - ax, by - ay, qb - qa
            len2 = dx * dx + dy * dy
            chunk = max(1, chunk_elems // K)
            for s0 in range(0, N, chunk):
                p = np.arange(s0, min(s0 + chunk, N))
                px = ((p % Wl).astype(F32) + F32(0.5))[:, None]
                py = ((p // Wl).astype(F32) + F32(0.5))[:, None]
                t = ((px - ax) * dx + (py - ay) * dy) / len2
                t = np.fmin(np.fmax(t, F32(0)), F32(1))
                t = np.where((len2 == 0) | np.isnan(t), F32(0), t)
                ex, ey = px - (ax + t * dx), py - (ay + t * dy)
                d2 = ex * ex + ey * ey
                covers = exists & (px >= ulo) & (px <= uhi) & (py >= vlo) & (py <= vhi) & (d2 <= r * r)
                qs = qa + t * dq
                assert qs.dtype == F32 and d2.dtype == F32
                counted = covers & (qs > 0)
                front = np.where(counted, qs, F32(0)).max(1)
                u = F32(1) / qs - (F32(1) / front)[:, None]
                assert u.dtype == F32
                lay = np.where(u < d, 0, np.where(u < F32(3) * d, 1, np.where(u < F32(7) * d, 2, 3)))
                q0[p] = front
                for k in range(4):
                    layers[p, k] = (counted & (lay == k)).sum(1)
    return q0.reshape(Hl, Wl), layers.reshape(Hl, Wl, 4)


def _count_float(c):
    return np.minimum(c, np.uint32(1 << 24)).astype(F32)


def model_lookup(P, sm, kappa=KAPPA, bias=BIAS):
    """P [n, 3] float32 world points against the map sm (dict: Ml, Hl, Wl, layer, q0, layers, qfl or None):
    (n float32, Tr float32, branch int: -1 no occluder term, 0 .. 3 the lookup's four branches, behind bool)"""
    P = np.asarray(P, F32).reshape(-1, 3)
    Hl, Wl = sm["Hl"], sm["Wl"]
    cnt = len(P)
    n, branch, behind = np.zeros(cnt, F32), np.full(cnt, -1), np.zeros(cnt, bool)
    if cnt and Hl * Wl:
        lx, ly, ql, valid = vc.model_project(P, np.asarray(sm["Ml"], F32).reshape(12), NEAR)
        with np.errstate(all="ignore"):
            inside = valid & (lx >= 0) & (lx < F32(Wl)) & (ly >= 0) & (ly < F32(Hl))
            e = np.where(inside, ly, 0).astype(np.int64) * Wl + np.where(inside, lx, 0).astype(np.int64)
            q0 = sm["q0"].reshape(-1)[e]
            n4 = sm["layers"].reshape(-1, 4)[e]
            u = F32(1) / ql - F32(1) / q0
            ok = inside & (q0 != 0) & (u > 0)
            i0 = n4[:, 0]
            i1 = i0 + n4[:, 1]
            i2 = i1 + n4[:, 2]
            assert i2.dtype == np.uint32
            c0, c1, c2 = _count_float(i0), _count_float(i1), _count_float(i2)
            d = F32(sm["layer"])
            b = np.where(u < d, 0, np.where(u < F32(3) * d, 1, np.where(u < F32(7) * d, 2, 3)))
            val = [c0 * (u / d),
                   c0 + _count_float(n4[:, 1]) * ((u - d) / (F32(2) * d)),
                   c1 + _count_float(n4[:, 2]) * ((u - F32(3) * d) / (F32(4) * d)),
                   c2 + _count_float(n4[:, 3]) * np.fmin((u - F32(7) * d) / (F32(8) * d), F32(1))]
            for k in range(4):
                assert val[k].dtype == F32
                n = np.where(ok & (b == k), val[k], n)
            branch = np.where(ok, b, -1)
            if sm.get("qfl") is not None:
                qfl = sm["qfl"].reshape(-1)[e]
                behind = inside & (qfl > 0) & (ql * (F32(1) + F32(bias)) < qfl)
    with np.errstate(all="ignore"):
        Tr = np.where(behind, F32(0), F32(1) / (F32(1) + F32(kappa) * n))
    assert Tr.dtype == F32 and n.dtype == F32
    return n, Tr, branch, behind


def model_shade_shadowed(points, v, f, seg, face, t, mode, sh, base, sm, kappa=KAPPA, bias=BIAS, return_branches=False):
    """uint8 [H, W, 3]: sc.model_shade with the transmittance on the kajiya terms; tangent mode is sc.model_shade itself"""
    if mode == sc.TANGENT:
        out = sc.model_shade(points, v, f, seg, face, mode, sh, base)
        return (out, set()) if return_branches else out
    H, W = seg.shape
    L = points.shape[1]
    out = np.empty((H * W, 3), np.uint8)
    out[:] = sc._quant8(sh["background_rgb"])
    seg, face, t = seg.reshape(-1), face.reshape(-1), t.reshape(-1)
    light = [sh["light"][c] for c in range(3)]
    seen = []
    with np.errstate(all="ignore"):
        on = np.nonzero(seg >= 0)[0]
        if len(on):
            s, i = seg[on] // (L - 1), seg[on] % (L - 1)
            A, B = points[s, i], points[s, i + 1]
            P = np.stack([A[:, c] + t[on] * (B[:, c] - A[:, c]) for c in range(3)], 1)
            assert P.dtype == F32
            _, Tr, br, bh = model_lookup(P, sm, kappa, bias)
            seen.append(np.where(bh, 4, br))
            T = sc._normalise([B[:, c] - A[:, c] for c in range(3)])
            Vn = sc._normalise([sh["eye"][c] - F32(0.5) * (A[:, c] + B[:, c]) for c in range(3)])
            cl, cv = sc._dot(T, light), sc._dot(T, Vn)
            sl, sv = np.sqrt(np.fmax(F32(0), F32(1) - cl * cl)), np.sqrt(np.fmax(F32(0), F32(1) - cv * cv))
            spec = np.fmax(F32(0), cl * cv + sl * sv)
            for _ in range(sh["shininess_log2"]):
                spec = spec * spec
            b = base[s] if base is not None else np.broadcast_to(sh["base_rgb"], (len(on), 3))
            col = [b[:, c] * (sh["ambient"] + sh["kd"] * (Tr * sl)) + sh["ks"] * (Tr * spec) for c in range(3)]
            assert col[0].dtype == F32
            out[on] = np.stack([sc._quant8(c) for c in col], 1)
        on = np.nonzero((seg < 0) & (face >= 0))[0]
        if len(on):
            tr = np.asarray(f, np.int64).reshape(-1, 3)[face[on]]
            v0, v1, v2 = v[tr[:, 0]], v[tr[:, 1]], v[tr[:, 2]]
            P = np.stack([((v0[:, c] + v1[:, c]) + v2[:, c]) / F32(3) for c in range(3)], 1)
            assert P.dtype == F32
            _, Tr, br, bh = model_lookup(P, sm, kappa, bias)
            seen.append(np.where(bh, 4, br) + 10)
            e1, e2 = [v1[:, c] - v0[:, c] for c in range(3)], [v2[:, c] - v0[:, c] for c in range(3)]
            n = sc._normalise([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
            c = sc._dot(n, light)
            lit = sh["ambient"] + sh["kd"] * (Tr * np.fmax(c, -c))
            assert lit.dtype == F32
            out[on] = np.stack([sc._quant8(sh["head_rgb"][k] * lit) for k in range(3)], 1)
    out = out.reshape(H, W, 3)
    return (out, set(np.concatenate(seen).tolist()) if seen else set()) if return_branches else out


# ---------------------------------------------------------------------------------------------------------------- the ladder
LADDER_Z = (1.0, 2.0, 4.0, 8.0, 16.0)
LADDER_M = ((4, 2, 0, 0, 0), (1, 1, 1, 1, 1), (3, 0, 5, 2, 7), (1, 2, 0, 129, 1))


def ladder(m):
    """m_z copies of the segment (0.25 z, 0.5 z, z) -- (0.75 z, 0.5 z, z) for z in LADDER_Z, under view_screen_w on a 1 x 1 map with
    d = 1: qs = 1 / z and u = z - z_first, all exact in float32"""
    segs = [[[0.25 * z, 0.5 * z, z], [0.75 * z, 0.5 * z, z]] for z, k in zip(LADDER_Z, m) for _ in range(k)]
    return np.ascontiguousarray(np.array(segs, F32).reshape(-1, 2, 3))


def ladder_point(z, sx=0.5, sy=0.5):
    return np.array([sx * z, sy * z, z], F32)


# ---------------------------------------------------------------------------------------------------------------- the maps
def _map_table():
    """name -> dict(points, view, Hl, Wl, rl, layer, mesh)"""
    t = {}

    def add(name, points, view, size, rl=1.0, layer=1.0, mesh=None):
        assert name not in t, name
        t[name] = dict(points=points, view=view, Hl=size[0], Wl=size[1], rl=rl, layer=layer, mesh=mesh)
    for k, m in enumerate(LADDER_M):
        add("ladder%d" % k, lambda m=m: ladder(m), "screen_w", (1, 1))
    for size in LIGHT_SIZES:
        for rl in LIGHT_RADII:   # all at w = 1: every covering segment ties for q0 and lands in layer 0; a zero-length segment
            add("singles-%dx%d-r%g" % (size + (rl,)), lambda size=size: sc.singles(*size), "pixels", size, rl=rl)
    for size in ((17, 33), (40, 48)):   # ends behind near, at near, a NaN
        add("dropped-%dx%d" % size, sc.dropped, "screen_w", size, rl=2.5 if size[0] == 40 else 1.0, layer=0.05)
    for size in ((1, 1), (16, 16)):
        add("empty-%dx%d" % size, lambda: np.zeros((0, 5, 3), F32), "front", size)
    for K in STACK_K:          # depths 1 .. 1 + 0.01 (K - 1): layers of 0.2, 0.4, 0.8 and the rest
        add("stack%d" % K, lambda K=K: sc.stack(K, False), "screen_w", (40, 48), rl=0.75, layer=0.2)   # (0.75: one tile)
        add("dups%d" % K, lambda K=K: sc.stack(K, True), "screen_w", (40, 48), rl=0.5, layer=0.25)
    add("long-80x96", lambda: sc.long_and_short(80, 96), "screen_w", (80, 96), layer=0.3)       # 30 tiles: the two long ones are BIG
    add("long-40x48", lambda: sc.long_and_short(40, 48), "screen_w", (40, 48), rl=2.5, layer=0.3)
    add("hair-L2-17x33", lambda: sc.hair(40, 2, 5), "oblique", (17, 33), rl=0.5, layer=0.05)
    add("hair-L100-40x48", lambda: sc.hair(16, 100, 1), "front", (40, 48), layer=0.05, mesh="small_sphere")
    add("hair-inside-16x16", lambda: sc.hair(24, 12, 3), "inside", (16, 16), rl=2.5, layer=0.02)
    add("hair-sphere-17x33", lambda: sc.hair(30, 20, 4), "oblique", (17, 33), layer=0.05, mesh="sphere")
    return t


_MAPS = _map_table()
MAPS = list(_MAPS)


@functools.lru_cache(maxsize=None)
def light_map(name):
    """dict: points, Ml, Hl, Wl, rl, layer, v, f (or None), pix, qfl (or None), q0, layers -- the model's map of one case"""
    c = dict(_MAPS[name])
    c["points"] = np.ascontiguousarray(c["points"]())
    c["Ml"] = np.ascontiguousarray(sc.VIEWS[c["view"]](c["Hl"], c["Wl"]))
    c["v"], c["f"] = sc.meshes()[c["mesh"]] if c["mesh"] else (None, None)
    c["pix"] = c["qfl"] = None
    if c["mesh"]:
        c["pix"], c["qfl"] = sc._mesh_planes(c["mesh"], c["view"], c["Hl"], c["Wl"], 1)
    c["q0"], c["layers"] = model_opacity(c["points"], c["Ml"], c["Hl"], c["Wl"], c["rl"], c["layer"])
    for a in (c["points"], c["Ml"], c["q0"], c["layers"]):
        a.setflags(write=False)
    return c


# ---------------------------------------------------------------------------------------------------------------- the frames
def _frame_table():
    """name -> dict(points, camera view, H, W, s, r, mesh, mode, colors, light map: view, size, rl, layer; kappa, bias, qfl)"""
    t = {}

    def add(name, points, view, size, light, lsize, s=1, r=0.75, mesh=None, mode=sc.KAJIYA, colors=None, rl=1.0, layer=0.05,
            kappa=KAPPA, bias=BIAS, qfl=True):
        t[name] = dict(points=points, view=view, H=size[0], W=size[1], s=s, r=r, mesh=mesh, mode=mode, colors=colors, light=light,
                       Hl=lsize[0], Wl=lsize[1], rl=rl, layer=layer, kappa=kappa, bias=bias, qfl=qfl)
    hair = lambda: sc.hair(30, 20, 4, through=False)  # noqa: E731
    add("sphere-48x64-ss2", hair, "front", (48, 64), "oblique", (17, 33), s=2, mesh="sphere")
    add("sphere-48x64-noqfl", hair, "front", (48, 64), "oblique", (17, 33), mesh="sphere", qfl=False, kappa=0.5)
    add("small-17x33", lambda: sc.hair(24, 16, 9), "oblique", (17, 33), "front", (40, 48), mesh="small_sphere", colors="per", rl=2.5,
        layer=0.03, kappa=1.0, bias=0.0)
    add("nomesh-16x16", lambda: sc.hair(12, 7, 7), "front", (16, 16), "oblique", (16, 16), rl=0.5, layer=0.1)
    add("tangent-17x33", lambda: sc.hair(24, 16, 9), "oblique", (17, 33), "front", (16, 16), mesh="small_sphere", mode=sc.TANGENT)
    add("empty-map-15x17", lambda: sc.hair(12, 3, 6), "front", (15, 17), "front", (0, 0), mesh="small_sphere")
    return t


_FRAMES = _frame_table()
FRAMES = list(_FRAMES)


@functools.lru_cache(maxsize=None)
def frame(name):
    """dict of one frame: the inputs (points, M, H, W, s, r, v, f, mode, base, sh, kappa, bias), the light map `sm` (dict as
    model_lookup takes it, with rl), the camera planes on the s-times finer grid (seg, t, face), the bytes on that grid `rgb`, the
    branches of the lookup met (`branches`: 0 .. 4 strand pixels, 10 .. 14 head pixels; 4: behind the head; -1 / 9: no occluder
    term) and the resolved `picture`"""
    c = dict(_FRAMES[name])
    pts = c["points"] = np.ascontiguousarray(c["points"]())
    M = c["M"] = sc.VIEWS[c["view"]](c["H"], c["W"])
    c["v"], c["f"] = sc.meshes()[c["mesh"]] if c["mesh"] else (None, None)
    S = len(pts)
    c["base"] = np.ascontiguousarray(np.random.default_rng(S).uniform(0.05, 0.95, (S, 3)).astype(F32)) if c["colors"] == "per" else None
    c["sh"] = sc.shading(M)
    Hl, Wl = c["Hl"], c["Wl"]
    Ml = np.ascontiguousarray(sc.VIEWS[c["light"]](max(Hl, 1), max(Wl, 1)))
    qfl = None
    if c["mesh"] and c["qfl"] and Hl * Wl:
        qfl = sc._mesh_planes(c["mesh"], c["light"], Hl, Wl, 1)[1]
    q0, layers = model_opacity(pts, Ml, Hl, Wl, c["rl"], c["layer"])
    c["sm"] = dict(Ml=Ml, Hl=Hl, Wl=Wl, rl=c["rl"], layer=c["layer"], q0=q0, layers=layers, qfl=qfl)
    s = c["s"]
    Ms, rs = sc.supersampled(M, c["r"], s)
    H, W = s * c["H"], s * c["W"]
    pix, qf = sc._mesh_planes(c["mesh"], c["view"], c["H"], c["W"], s) if c["mesh"] else (None, None)
    seg, t, face, _ = sc.model_head_test(*sc.model_strand_winner(pts, Ms, H, W, rs), pix, qf, 0.0)
    c["Ms"], c["rs"], c["planes"] = Ms, float(rs), (seg, t, face)
    c["rgb"], c["branches"] = model_shade_shadowed(pts, c["v"], c["f"], seg, face, t, c["mode"], c["sh"], c["base"], c["sm"], c["kappa"],
                                                   c["bias"], return_branches=True)
    c["plain"] = sc.model_shade(pts, c["v"], c["f"], seg, face, c["mode"], c["sh"], c["base"])
    c["picture"] = sc.model_resolve(c["rgb"], s)
    for a in (pts, M, Ml, q0, layers, c["rgb"], c["plain"], c["picture"], seg, t, face):
        a.setflags(write=False)
    return c
