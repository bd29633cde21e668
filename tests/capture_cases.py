"""Shared cases of the synthetic-capture tests (csrc/ghr_capture.h): the numpy float32 MODEL of the definition (the
expressions of ghr_capture.h in their operand order, on the index planes of the strand-preview model of tests/strand_view_cases.py),
a float64 TRUTH on the same float32 screen points, every case of strand_view_cases.CASES at s = 1, 2, 4 and the planted cases.
Everything is computed once per process and handed out read-only."""
import functools

import numpy as np

from tests import strand_view_cases as sc
from tests import visibility_cases as vc

F32 = np.float32
NEAR = sc.NEAR
BINS = 180
SUPERSAMPLES = (1, 2, 4)


def table():
    """T [180, 2] float32 restated: (cos 2 th_k, sin 2 th_k) in float64, rounded once"""
    th = np.arange(BINS, dtype=np.float64) * np.pi / 180.0
    return np.ascontiguousarray(np.stack([np.cos(2 * th), np.sin(2 * th)], 1).astype(F32))


# ---------------------------------------------------------------------------------------------------------------- planted
def _comb(H, W):
    """a few straight strands of two segments across the frame, on no lattice: every size gets hair and background"""
    n = 3
    y0 = np.linspace(0.3, H - 0.4, n)
    sxy = np.array([[[-1.0, y], [W / 2.0 + 0.3, y + 0.37 * (k + 1)], [W + 1.0, y - 0.2]] for k, y in enumerate(y0)])
    sxy = np.concatenate([sxy, [[[W / 3.0, -1.0], [W / 3.0 + 0.4, H / 2.0], [W / 2.0, H + 1.0]]]])
    return sc.from_pixels(sxy)


def _front_and_behind():
    """two straight strands across the small sphere's silhouette under view_front (camera near z = 3.1): one in front of the head
    (z = 1.2), one behind it (z = -1.2), four segments each"""
    x = np.linspace(-1.6, 1.6, 5)
    a = np.stack([x, np.full(5, 0.15), np.full(5, 1.2)], 1)
    b = np.stack([x, np.full(5, -0.2) + 0.1 * x, np.full(5, -1.2)], 1)
    return np.ascontiguousarray(np.stack([a, b]).astype(F32))


def _thin():
    return sc.from_pixels([[[0.7, 0.9], [15.2, 9.1], [31.6, 15.3]]])


def _crossing():
    """s = 4, view_pixels, output pixel (1, 1) (fine rows and columns 4 .. 7): strand 0 lies along the fine row y = 5.5 from x = 4.3
    to 6.7 (the centres 4.5, 5.5, 6.5), strand 1 along the fine column x = 5.5 from y = 4.3 to 7.7 (the centres 4.5 .. 7.5); all at
    w = 1, so the crossing goes to the lower index: three subsamples each, c2 = -1 and +1: C = S = 0"""
    return sc.from_pixels(np.array([[[4.3, 5.5], [6.7, 5.5]], [[5.5, 4.3], [5.5, 7.7]]]) / 4.0)


def _along_the_ray():
    """view_pixels ignores X2: the two ends of the segment project to one point (len2 == 0, a disc), next to an ordinary strand"""
    p = sc.from_pixels([[[2.5, 2.5], [2.5, 2.5]], [[0.5, 0.4], [4.6, 0.9]]])
    p[0, 1, 2] = 1.0
    return p


THETAS_ON = (0, 1, 30, 45, 60, 89, 90, 91, 120, 135, 150, 179)


def _directions(offsets):
    """one two-point strand per angle under view_pixels, direction (sin th, cos th) (x right, y down), half-length 3 pixels, on a
    6 x 2 grid of centres 8 and 10 pixels apart; returns (points, theta in radians float64)"""
    th = np.array([np.deg2rad(k) + o for k, o in offsets], np.float64)
    pts = []
    for n, t in enumerate(th):
        cx, cy = 5.0 + 8.0 * (n % 6), 5.0 + 10.0 * (n // 6)
        d = 3.0 * np.array([np.sin(t), np.cos(t)])
        pts.append([[cx - d[0], cy - d[1]], [cx + d[0], cy + d[1]]])
    return sc.from_pixels(np.array(pts)), th


def _on_bins():
    return _directions([(k, 0.0) for k in THETAS_ON])[0]


def _near_boundaries():
    return _directions([(k + 0.5, o) for k in (0, 29, 44, 89, 134, 178) for o in (-1e-6, 1e-6)])[0]


def _planted():
    t = {}

    def add(name, points, view, size, r=0.75, bias=0.0, mesh=None, ss=SUPERSAMPLES, var_floor=0.0):
        assert name not in t, name
        t[name] = dict(points=points, view=view, H=size[0], W=size[1], r=r, bias=bias, mesh=mesh, ss=tuple(ss), var_floor=var_floor)
    for size in ((1, 1), (3, 5), (4, 9), (3, 6), (5, 7), (17, 33)):      # widths 4 m + 1, + 2, + 3; one pixel; more than one quad row
        add("comb-%dx%d" % size, lambda size=size: _comb(*size), "pixels", size, var_floor=0.094 if size == (3, 5) else 0.0)
    add("empty-3x5", lambda: np.zeros((0, 2, 3), F32), "pixels", (3, 5))
    add("head-only-17x33", lambda: np.zeros((0, 3, 3), F32), "front", (17, 33), mesh="small_sphere")
    add("front-and-behind-17x33", _front_and_behind, "front", (17, 33), mesh="small_sphere")
    add("thin-17x33", _thin, "pixels", (17, 33), r=0.1)                   # at s = 1 the strand is 0.2 subsamples wide
    add("crossing-3x3", _crossing, "pixels", (3, 3), r=0.075, ss=(4,))
    add("along-the-ray-5x6", _along_the_ray, "pixels", (5, 6), r=0.75)
    add("dropped-48x66", sc.dropped, "screen_w", (48, 66), r=1.0, ss=(1, 2))
    add("on-bins-20x50", _on_bins, "pixels", (20, 50), r=0.75)
    add("near-boundaries-20x50", _near_boundaries, "pixels", (20, 50), r=0.75)
    return t


_PLANTED = _planted()
PLANTED = [(name, s) for name, c in _PLANTED.items() for s in c["ss"]]
FROM_PREVIEW = [(name, s) for name in sc.CASES for s in SUPERSAMPLES]
CASES = FROM_PREVIEW + PLANTED
IDS = ["%s-s%d" % c for c in CASES]
SMALL = [(name, s) for name, s in CASES if s * (_PLANTED[name]["H"] if name in _PLANTED else sc.case(name)["H"]) <= 68]  # the sanitized run's


@functools.lru_cache(maxsize=None)
def case(name, s):
    """dict: points [S, L, 3], M (the view's), Ms (the finer grid's), H, W, s, r, bias, v, f (or None), F, var_floor, and the
    model's planes seg, face [s H, s W] of the finer grid"""
    if name in _PLANTED:
        p = _PLANTED[name]
        pts = np.ascontiguousarray(p["points"]())
        M = sc.VIEWS[p["view"]](p["H"], p["W"])
        v, f = sc.meshes()[p["mesh"]] if p["mesh"] else (None, None)
        Ms, rs = sc.supersampled(M, p["r"], s)
        H, W = s * p["H"], s * p["W"]
        pix = qf = None
        if v is not None:
            pix = vc.model_rasterize(v, f, Ms, H, W, NEAR)
            qf = sc.model_face_depth(v, f, Ms, H, W, pix)
        planes = sc.model_head_test(*sc.model_strand_winner(pts, Ms, H, W, rs), pix, qf, p["bias"])
        c = dict(points=pts, M=M, Ms=Ms, H=p["H"], W=p["W"], s=s, r=p["r"], bias=p["bias"], v=v, f=f, var_floor=p["var_floor"],
                 seg=planes[0], face=planes[2])
    else:
        b, m = sc.case(name), sc.model_frame(name, s)
        c = dict(points=b["points"], M=b["M"], Ms=m["M"], H=b["H"], W=b["W"], s=s, r=b["r"], bias=b["bias"], v=b["v"], f=b["f"],
                 var_floor=0.0, seg=m["planes"][0], face=m["planes"][2])
    c["F"] = 0 if c["f"] is None else len(c["f"])
    c["seg"], c["face"] = np.ascontiguousarray(c["seg"]), np.ascontiguousarray(c["face"])
    for a in (c["points"], c["Ms"], c["seg"], c["face"]):
        a.setflags(write=False)
    return c


# ---------------------------------------------------------------------------------------------------------------- the model
def _directions_of(points, Ms, seg, K):
    """per subsample: (hair bool, ok bool, ax, ay, bx, by float32) -- the segment's projected ends where the entry is in its table"""
    S, L = points.shape[:2]
    hair = (seg >= 0) & (seg.astype(np.int64) < K)
    z = np.zeros(seg.shape, F32)
    if not K:
        return hair, np.zeros(seg.shape, bool), z, z, z, z
    k = np.where(hair, seg, 0).astype(np.int64)
    si, ii = k // (L - 1), k % (L - 1)
    sx, sy, _, valid = vc.model_project(points.reshape(-1, 3), Ms, NEAR)
    sx, sy, valid = sx.reshape(S, L), sy.reshape(S, L), valid.reshape(S, L)
    ok = hair & valid[si, ii] & valid[si, ii + 1]
    return hair, ok, sx[si, ii], sy[si, ii], sx[si, ii + 1], sy[si, ii + 1]


def model_capture(points, Ms, H, W, s, F, seg, face, var_floor=0.0):
    """(mask_hair u8, mask_body u8, angle u8, var f32, C f32, S f32) [H, W] of the definition; seg / face [s H, s W]"""
    S_, L = points.shape[:2]
    K, n = S_ * (L - 1), s * s
    hair, ok, ax, ay, bx, by = _directions_of(points, Ms, seg, K)
    head = ~hair & (face >= 0) & (face < F)
    with np.errstate(all="ignore"):
        dx, dy = bx - ax, by - ay
        len2 = dx * dx + dy * dy
        c2 = (dy * dy - dx * dx) / len2
        s2 = (F32(2) * (dx * dy)) / len2
        assert c2.dtype == F32 and s2.dtype == F32
        ok = ok & (len2 > 0) & np.isfinite(c2) & np.isfinite(s2)
        C, Sm = np.zeros((H, W), F32), np.zeros((H, W), F32)
        for a in range(s):
            for b in range(s):
                m = ok[a::s, b::s]
                C = np.where(m, C + c2[a::s, b::s], C)
                Sm = np.where(m, Sm + s2[a::s, b::s], Sm)
        assert C.dtype == F32 and Sm.dtype == F32
        n_hair = hair.reshape(H, s, W, s).sum((1, 3)).astype(np.int64)
        n_face = head.reshape(H, s, W, s).sum((1, 3)).astype(np.int64)
        mask_hair = ((255 * n_hair + n // 2) // n).astype(np.uint8)
        mask_body = ((255 * (n_hair + n_face) + n // 2) // n).astype(np.uint8)
        T = table()
        score = C[..., None] * T[:, 0] + Sm[..., None] * T[:, 1]
        assert score.dtype == F32
        score = np.where(np.isnan(score), -np.inf, score)
        angle = np.where(np.isneginf(score).all(-1), 0, score.argmax(-1)).astype(np.uint8)    # (argmax: the FIRST maximum)
        var = F32(var_floor) + F32(0.5) * np.fmax(F32(0), F32(1) - np.sqrt(C * C + Sm * Sm) / F32(n))
        assert var.dtype == F32
    return mask_hair, mask_body, angle, var, C, Sm


@functools.lru_cache(maxsize=None)
def model(name, s):
    c = case(name, s)
    out = model_capture(c["points"], c["Ms"], c["H"], c["W"], s, c["F"], c["seg"], c["face"], c["var_floor"])
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------- the truth
def truth_capture(points, Ms, H, W, s, seg, var_floor=0.0):
    """float64 on the model's float32 screen points: (theta in [0, pi) by atan2, var, resultant |Sigma|) [H, W]"""
    S_, L = points.shape[:2]
    K, n = S_ * (L - 1), s * s
    hair, ok, ax, ay, bx, by = _directions_of(points, Ms, seg, K)
    with np.errstate(all="ignore"):
        dx, dy = bx.astype(np.float64) - ax.astype(np.float64), by.astype(np.float64) - ay.astype(np.float64)
        len2 = dx * dx + dy * dy
        ok = ok & (len2 > 0)
        c2 = np.where(ok, (dy * dy - dx * dx) / np.where(ok, len2, 1.0), 0.0)
        s2 = np.where(ok, 2.0 * dx * dy / np.where(ok, len2, 1.0), 0.0)
    C = c2.reshape(H, s, W, s).sum((1, 3))
    Sm = s2.reshape(H, s, W, s).sum((1, 3))
    R = np.sqrt(C * C + Sm * Sm)
    theta = np.mod(0.5 * np.arctan2(Sm, C), np.pi)
    return theta, float(F32(var_floor)) + 0.5 * np.maximum(0.0, 1.0 - R / n), R
