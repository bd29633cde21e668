"""A preview of the groom: strands drawn as depth-tested polylines over the head mesh (csrc/ghr_strandview.h) --
the last step of the reference's ``run.sh``, ``src/postprocessing/render_video.py``, without Blender.

``rasterize_strands`` gives the four planes of one view (``pix_to_segment``, ``t``, ``pix_to_face``, ``inv_depth``),
``render_strands`` the shaded uint8 picture, ``camera_path`` the script's interpolated cameras as 3 x 4 pixel matrices.
``fused=True`` launches the HIP kernels (ROCm tensors only: there is no CPU path); ``fused=False`` evaluates the PyTorch-composed
comparator on any device: the same float32 expressions in the same operand order, brute force in pixel chunks over all segments
whose widened box meets the chunk's pixel range -- the tile lists change which segments a pixel looks at, never the winner.
The definition is this package's own and is stated at the top of ``csrc/ghr_strandview.h``.  A view is ``(M, H, W)`` as in
``visibility.py``.

Self-shadowing is a deep opacity map of a light view: ``light_view`` fits a perspective light camera to the groom,
``strand_shadow_map`` makes the map (``ghr_strandview_opacity``, or the composed form), and ``render_strands(shadows=...)`` shades
with the transmittance it gives.  ``shadows=False`` (the default) is the unshadowed path, launch for launch.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from . import visibility as vis
from .visibility import NEAR

MODES = {"kajiya": _lib.STRANDVIEW_KAJIYA, "tangent": _lib.STRANDVIEW_TANGENT}
# the defaults of csrc/ghr_strandview.h
AMBIENT, KD, KS, SHININESS_LOG2 = 0.25, 0.65, 0.35, 5
HAIR_RGB, HEAD_RGB, BACKGROUND_RGB = (0.45, 0.30, 0.18), (0.62, 0.62, 0.62), (1.0, 1.0, 1.0)
LIGHT_CAMERA = (0.45, -0.60, -0.66)  # camera axes (x right, y down, z forward): above and to the right of the camera
# the look constants of the shadows (chosen, not measured): the light map's size, the half-width in texels, kappa, the bias of the
# head's shadow, and the layer depth as a fraction of the bounding sphere's radius
SHADOW_SIZE, SHADOW_HALF_WIDTH, SHADOW_KAPPA, SHADOW_BIAS, SHADOW_LAYERS_PER_RADIUS = 1024, 1.0, 0.2, 0.02, 32


# ---------------------------------------------------------------------------------------------------------------- helpers
def _m12(M):
    return np.ascontiguousarray(np.asarray(M, np.float32).reshape(12))


def _points(points, dev):
    p = points if isinstance(points, torch.Tensor) else torch.from_numpy(np.array(points, np.float32))
    assert p.dim() == 3 and p.shape[2] == 3, tuple(p.shape)
    if p.shape[1] < 2:
        raise ValueError("strand_view: a strand needs two points (L >= 2), got L = %d" % p.shape[1])
    return p.detach().to(device=dev, dtype=torch.float32).contiguous()


def _check_scalars(half_width, head_bias):
    if not (np.isfinite(half_width) and half_width > 0):
        raise ValueError("strand_view: half_width must be finite and > 0")
    if not (np.isfinite(head_bias) and head_bias >= 0):
        raise ValueError("strand_view: head_bias must be finite and >= 0")


def supersampled(M, half_width, s):
    """(M, r) of the s-times finer grid: rows 0 and 1 of M and r times s (exact: s is a power of two)"""
    if s not in (1, 2, 4):
        raise ValueError("strand_view: supersample must be 1, 2 or 4")
    Ms = _m12(M).copy()
    Ms[:8] *= np.float32(s)
    return Ms, float(np.float32(half_width) * np.float32(s))


def shading_for_view(M, ambient=AMBIENT, kd=KD, ks=KS, shininess_log2=SHININESS_LOG2, hair_rgb=HAIR_RGB, head_rgb=HEAD_RGB,
                     background_rgb=BACKGROUND_RGB, light_camera=LIGHT_CAMERA, eye=None, light=None) -> dict:
    """The constants of one picture as float32: ``eye`` (the camera centre) and ``light`` (a world-space unit vector towards the
    light: ``light_camera`` rotated to world) come from ``decompose_projection`` of M in double, rounded once."""
    if eye is None or light is None:
        _, R, t = vis.decompose_projection(np.asarray(M, np.float64).reshape(3, 4))
        if eye is None:
            eye = -R.T @ t
        if light is None:
            lc = np.asarray(light_camera, np.float64)
            light = R.T @ (lc / np.linalg.norm(lc))
            light = light / np.linalg.norm(light)
    if not 0 <= int(shininess_log2) <= 16:
        raise ValueError("strand_view: shininess_log2 must be in 0 .. 16")
    f3 = lambda x: np.asarray(x, np.float64).reshape(3).astype(np.float32)  # noqa: E731
    return dict(eye=f3(eye), light=f3(light), ambient=np.float32(ambient), kd=np.float32(kd), ks=np.float32(ks),
                shininess_log2=int(shininess_log2), base_rgb=f3(hair_rgb), head_rgb=f3(head_rgb), background_rgb=f3(background_rgb))


def _shading_struct(sh):
    s = _lib.StrandViewShading()
    for name in ("eye", "light", "base_rgb", "head_rgb", "background_rgb"):
        setattr(s, name, (ctypes.c_float * 3)(*[float(x) for x in sh[name]]))
    s.ambient, s.kd, s.ks, s.shininess_log2 = float(sh["ambient"]), float(sh["kd"]), float(sh["ks"]), int(sh["shininess_log2"])
    return s


def strandview_workspace_bytes(S: int, L: int, H: int, W: int) -> int:
    b = ctypes.c_size_t(0)
    _lib.check(_lib.lib().ghr_strandview_sizes(int(S), int(L), int(H), int(W), ctypes.byref(b)))
    return int(b.value)


# ---------------------------------------------------------------------------------------------------------------- composed
def _project_torch(X, m, nr):
    x = [X[..., c] for c in range(3)]
    xp = (m[0] * x[0] + m[1] * x[1]) + (m[2] * x[2] + m[3])
    yp = (m[4] * x[0] + m[5] * x[1]) + (m[6] * x[2] + m[7])
    w = (m[8] * x[0] + m[9] * x[1]) + (m[10] * x[2] + m[11])
    return xp / w, yp / w, torch.ones_like(w) / w, torch.isfinite(w) & (w > nr)   # (divisions: correctly rounded)


def _sqrt(x):
    """sqrtf, correctly rounded whatever the device's float32 sqrt does: the double root rounded once (53 >= 2 x 24 + 2 bits)"""
    return torch.sqrt(x.double()).float()


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _normalise(x):
    ln = _sqrt(_dot(x, x))
    zero = torch.zeros_like(ln)
    return [torch.where(ln == 0, zero, c / ln) for c in x]


def _face_depth_torch(v, f, M, H, W, near, pix):
    """qf [H, W] float32 of the definition; v [V, 3] float32, f [F, 3] int64, pix [H, W] int32 on one device"""
    dev = pix.device
    out = torch.zeros(H * W, dtype=torch.float32, device=dev)
    V, Fc = v.shape[0], f.shape[0]
    if H * W == 0 or Fc == 0 or V == 0:
        return out.reshape(H, W)
    m = [float(x) for x in _m12(M)]
    nr = float(np.float32(near))
    face = pix.reshape(-1).long()
    has = (face >= 0) & (face < Fc)
    t = f[torch.where(has, face, torch.zeros_like(face))]                       # [N, 3]
    in_range = ((t >= 0) & (t < V)).all(dim=1)
    ti = torch.where(in_range[:, None], t, torch.zeros_like(t))
    u, w_, q, ok = [], [], [], has & in_range & (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    for k in range(3):
        sx, sy, qq, valid = _project_torch(v[ti[:, k]], m, nr)
        u.append(sx); w_.append(sy); q.append(qq)
        ok = ok & valid
    ok = ok & ~((u[1] - u[0]) * (w_[2] - w_[0]) - (w_[1] - w_[0]) * (u[2] - u[0]) == 0)
    p = torch.arange(H * W, device=dev)
    px, py = (p % W).float() + 0.5, (p // W).float() + 0.5
    side, e = [], []
    for k in range(3):
        k1 = (k + 1) % 3
        flip = t[:, k] > t[:, k1]
        au, av = torch.where(flip, u[k1], u[k]), torch.where(flip, w_[k1], w_[k])
        bu, bv = torch.where(flip, u[k], u[k1]), torch.where(flip, w_[k], w_[k1])
        dx, dy = bu - au, bv - av
        E = dx * (py - av) - dy * (px - au)
        left = (E > 0) | ((E == 0) & ((dy < 0) | ((dy == 0) & (dx > 0))))
        side.append(left != flip)
        e.append(torch.where(flip, -E, E))
    d = ((e[1] * q[0] + e[2] * q[1]) + e[0] * q[2]) / ((e[0] + e[1]) + e[2])
    ulo, uhi = torch.fmin(torch.fmin(u[0], u[1]), u[2]), torch.fmax(torch.fmax(u[0], u[1]), u[2])
    vlo, vhi = torch.fmin(torch.fmin(w_[0], w_[1]), w_[2]), torch.fmax(torch.fmax(w_[0], w_[1]), w_[2])
    covers = ok & (px >= ulo) & (px <= uhi) & (py >= vlo) & (py <= vhi) & (side[0] == side[1]) & (side[1] == side[2]) & (d > 0)
    return torch.where(covers, d, out).reshape(H, W)


def _rasterize_torch(points, M, H, W, r, head_bias, near, pix_to_face=None, qf=None, chunk_elems=None):
    """The four planes of the definition, brute force; points [S, L, 3] float32, pix_to_face / qf [H, W] or None"""
    dev = points.device
    N = H * W
    seg = torch.full((N,), -1, dtype=torch.int32, device=dev)
    tt = torch.zeros(N, dtype=torch.float32, device=dev)
    qq = torch.zeros(N, dtype=torch.float32, device=dev)
    S, L = points.shape[0], points.shape[1]
    K = S * (L - 1)
    if N and K:
        if chunk_elems is None:
            chunk_elems = 1 << (25 if dev.type == "cuda" else 21)
        m = [float(x) for x in _m12(M)]
        r32 = float(np.float32(r))
        rr = float(np.float32(r) * np.float32(r))
        sx, sy, q, valid = _project_torch(points, m, float(np.float32(near)))
        ax, ay, qa = sx[:, :-1].reshape(-1), sy[:, :-1].reshape(-1), q[:, :-1].reshape(-1)
        bx, by, qb = sx[:, 1:].reshape(-1), sy[:, 1:].reshape(-1), q[:, 1:].reshape(-1)
        exists = (valid[:, :-1] & valid[:, 1:]).reshape(-1)
        ulo, uhi = torch.fmin(ax, bx) - r32, torch.fmax(ax, bx) + r32
        vlo, vhi = torch.fmin(ay, by) - r32, torch.fmax(ay, by) + r32
        dx, dy, dq = bx - ax, by - ay, qb - qa
        len2 = dx * dx + dy * dy
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        chunk = max(1, chunk_elems // K)
        for s0 in range(0, N, chunk):
            p = torch.arange(s0, min(s0 + chunk, N), device=dev)
            px = ((p % W).float() + 0.5)[:, None]
            py = ((p // W).float() + 0.5)[:, None]
            # the closed widened box is part of the coverage rule: a segment whose box misses the chunk's pixel range covers none
            # of its centres (an exact cull; a NaN bound fails here as it fails there)
            sid = torch.nonzero(exists & (uhi >= px.min()) & (ulo <= px.max()) & (vhi >= py.min()) & (vlo <= py.max()))[:, 0]
            if sid.numel() == 0:
                continue
            cax, cay, cdx, cdy, cl2 = ax[sid], ay[sid], dx[sid], dy[sid], len2[sid]
            t = ((px - cax) * cdx + (py - cay) * cdy) / cl2
            t = torch.fmin(torch.fmax(t, zero), zero + 1)
            t = torch.where((cl2 == 0) | torch.isnan(t), zero, t)
            ex, ey = px - (cax + t * cdx), py - (cay + t * cdy)
            covers = (px >= ulo[sid]) & (px <= uhi[sid]) & (py >= vlo[sid]) & (py <= vhi[sid]) & (ex * ex + ey * ey <= rr)
            qs = qa[sid] + t * dq[sid]
            qs = torch.where(covers & (qs > 0), qs, zero)
            qmax = qs.max(dim=1).values
            first = torch.where(qs == qmax[:, None], sid, K).min(dim=1).values   # the lowest index among the equals
            won = qmax > 0
            col = torch.searchsorted(sid, torch.where(won, first, sid[0]))[:, None]
            seg[p] = torch.where(won, first, -1).to(torch.int32)
            tt[p] = torch.where(won, t.gather(1, col)[:, 0], zero)
            qq[p] = torch.where(won, qmax, zero)
    if pix_to_face is not None:
        face, qfv = pix_to_face.reshape(-1).to(torch.int32), qf.reshape(-1)
    else:
        face, qfv = torch.full((N,), -1, dtype=torch.int32, device=dev), torch.zeros(N, dtype=torch.float32, device=dev)
    has_face = qfv > 0
    hb1 = float(np.float32(1) + np.float32(head_bias))
    kept = (seg >= 0) & (~has_face | (qq * hb1 >= qfv))
    head = ~kept & has_face
    minus = torch.full_like(seg, -1)
    z = torch.zeros_like(tt)
    return (torch.where(kept, seg, minus).reshape(H, W), torch.where(kept, tt, z).reshape(H, W),
            torch.where(head, face, minus).reshape(H, W), torch.where(kept, qq, torch.where(head, qfv, z)).reshape(H, W))


def _quant8(x):
    zero = torch.zeros((), dtype=torch.float32, device=x.device)
    x = torch.fmin(torch.fmax(x, zero), zero + 1)
    return torch.fmin(torch.fmax(x * 255.0 + 0.5, zero), zero + 255).to(torch.uint8)


def _shade_torch(points, v, f, H, W, seg, face, mode, sh, base=None, t=None, shadow=None, kappa=0.0, bias=0.0):
    """uint8 [H, W, 3] of the definition; v / f may be None (no mesh).  ``shadow``: a ShadowMap (with ``t``, the raster's t plane):
    the kajiya terms are multiplied by the transmittance; None: the unshadowed expressions."""
    dev = seg.device
    N = H * W
    S, L = points.shape[0], points.shape[1]
    out = torch.empty((N, 3), dtype=torch.uint8, device=dev)
    if N == 0:
        return out.reshape(H, W, 3)
    sc = {k: (torch.tensor(val, dtype=torch.float32, device=dev) if isinstance(val, np.ndarray) else float(val)) for k, val in sh.items()}
    out[:] = _quant8(sc["background_rgb"])[None]
    seg, face = seg.reshape(-1).long(), face.reshape(-1).long()
    on = torch.nonzero((seg >= 0) & (seg < S * (L - 1)))[:, 0]
    if on.numel():
        k = seg[on]
        s, i = k // (L - 1), k % (L - 1)
        A, B = points[s, i], points[s, i + 1]
        T = _normalise([B[:, c] - A[:, c] for c in range(3)])
        if mode == _lib.STRANDVIEW_TANGENT:
            col = [0.5 + 0.5 * T[c] for c in range(3)]
        else:
            Vn = _normalise([sc["eye"][c] - 0.5 * (A[:, c] + B[:, c]) for c in range(3)])
            Lw = [sc["light"][c] for c in range(3)]
            cl, cv = _dot(T, Lw), _dot(T, Vn)
            zero = torch.zeros_like(cl)
            sl, sv = _sqrt(torch.fmax(zero, 1.0 - cl * cl)), _sqrt(torch.fmax(zero, 1.0 - cv * cv))
            spec = torch.fmax(zero, cl * cv + sl * sv)
            for _ in range(int(sh["shininess_log2"])):
                spec = spec * spec
            b = base[s] if base is not None else sc["base_rgb"][None].expand(len(on), 3)
            if shadow is not None:
                tk = t.reshape(-1)[on]
                Tr = _transmittance_torch([A[:, c] + tk * (B[:, c] - A[:, c]) for c in range(3)], shadow, kappa, bias)
                col = [b[:, c] * (sc["ambient"] + sc["kd"] * (Tr * sl)) + sc["ks"] * (Tr * spec) for c in range(3)]
            else:
                col = [b[:, c] * (sc["ambient"] + sc["kd"] * sl) + sc["ks"] * spec for c in range(3)]
        out[on] = torch.stack([_quant8(c) for c in col], dim=1)
    if v is not None and f is not None and f.shape[0] and v.shape[0]:
        hd = ~((seg >= 0) & (seg < S * (L - 1))) & (face >= 0) & (face < f.shape[0])
        t = f[torch.where(hd, face, torch.zeros_like(face))]
        hd = hd & ((t >= 0) & (t < v.shape[0])).all(dim=1)
        on = torch.nonzero(hd)[:, 0]
        if on.numel():
            t = t[on]
            v0, v1, v2 = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
            e1, e2 = [v1[:, c] - v0[:, c] for c in range(3)], [v2[:, c] - v0[:, c] for c in range(3)]
            n = _normalise([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
            c = _dot(n, [sc["light"][k] for k in range(3)])
            if shadow is not None and mode != _lib.STRANDVIEW_TANGENT:
                Tr = _transmittance_torch([_div((v0[:, k] + v1[:, k]) + v2[:, k], 3.0) for k in range(3)], shadow, kappa, bias)
                lit = sc["ambient"] + sc["kd"] * (Tr * torch.fmax(c, -c))
            else:
                lit = sc["ambient"] + sc["kd"] * torch.fmax(c, -c)
            out[on] = torch.stack([_quant8(sc["head_rgb"][k] * lit) for k in range(3)], dim=1)
    return out.reshape(H, W, 3)


def _div(a, b):
    """a / b for a float b as a tensor division (a division by a host scalar may be evaluated as a product with 1 / b)"""
    return a / torch.full_like(a, float(np.float32(b)))


def _opacity_torch(points, Ml, Hl, Wl, rl, layer, near, chunk_elems=None):
    """(q0 float32 [Hl, Wl], layers int32 [Hl, Wl, 4]) of the definition, brute force like _rasterize_torch: integer sums over
    the covering mask, texel chunk by texel chunk"""
    dev = points.device
    N = Hl * Wl
    q0 = torch.zeros(N, dtype=torch.float32, device=dev)
    layers = torch.zeros((N, 4), dtype=torch.int32, device=dev)
    S, L = points.shape[0], points.shape[1]
    K = S * (L - 1)
    if N and K:
        if chunk_elems is None:
            chunk_elems = 1 << (25 if dev.type == "cuda" else 21)
        m = [float(x) for x in _m12(Ml)]
        r32 = float(np.float32(rl))
        rr = float(np.float32(rl) * np.float32(rl))
        d1 = np.float32(layer)
        d1, d3, d7 = float(d1), float(np.float32(3) * d1), float(np.float32(7) * d1)
        sx, sy, q, valid = _project_torch(points, m, float(np.float32(near)))
        ax, ay, qa = sx[:, :-1].reshape(-1), sy[:, :-1].reshape(-1), q[:, :-1].reshape(-1)
        bx, by, qb = sx[:, 1:].reshape(-1), sy[:, 1:].reshape(-1), q[:, 1:].reshape(-1)
        exists = (valid[:, :-1] & valid[:, 1:]).reshape(-1)
        ulo, uhi = torch.fmin(ax, bx) - r32, torch.fmax(ax, bx) + r32
        vlo, vhi = torch.fmin(ay, by) - r32, torch.fmax(ay, by) + r32
        dx, dy, dq = bx - ax, by - ay, qb - qa
        len2 = dx * dx + dy * dy
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        chunk = max(1, chunk_elems // K)
        for s0 in range(0, N, chunk):
            p = torch.arange(s0, min(s0 + chunk, N), device=dev)
            px = ((p % Wl).float() + 0.5)[:, None]
            py = ((p // Wl).float() + 0.5)[:, None]
            sid = torch.nonzero(exists & (uhi >= px.min()) & (ulo <= px.max()) & (vhi >= py.min()) & (vlo <= py.max()))[:, 0]
            if sid.numel() == 0:
                continue
            cax, cay, cdx, cdy, cl2 = ax[sid], ay[sid], dx[sid], dy[sid], len2[sid]
            t = ((px - cax) * cdx + (py - cay) * cdy) / cl2
            t = torch.fmin(torch.fmax(t, zero), zero + 1)
            t = torch.where((cl2 == 0) | torch.isnan(t), zero, t)
            ex, ey = px - (cax + t * cdx), py - (cay + t * cdy)
            covers = (px >= ulo[sid]) & (px <= uhi[sid]) & (py >= vlo[sid]) & (py <= vhi[sid]) & (ex * ex + ey * ey <= rr)
            qs = qa[sid] + t * dq[sid]
            counted = covers & (qs > 0)
            qs = torch.where(counted, qs, zero + 1)
            front = torch.where(counted, qs, zero).max(dim=1).values
            u = torch.ones_like(qs) / qs - (torch.ones_like(front) / front)[:, None]
            lay = torch.where(u < d1, 0, torch.where(u < d3, 1, torch.where(u < d7, 2, 3)))
            q0[p] = front
            layers[p] = torch.stack([(counted & (lay == k)).sum(dim=1) for k in range(4)], dim=1).to(torch.int32)
    return q0.reshape(Hl, Wl), layers.reshape(Hl, Wl, 4)


def _occluders_torch(P, shadow):
    """(n float32, ql, the texel's index, inside) of the lookup for the world points P = [x, y, z] (three float32 tensors)"""
    Hl, Wl = shadow.Hl, shadow.Wl
    dev = P[0].device
    m = [float(x) for x in _m12(shadow.Ml)]
    lx, ly, ql, valid = _project_torch(torch.stack(P, dim=-1), m, float(np.float32(shadow.near)))
    zero = torch.zeros_like(ql)
    if Hl * Wl == 0:
        return zero, ql, torch.zeros_like(ql, dtype=torch.int64), torch.zeros_like(valid)
    inside = valid & (lx >= 0) & (lx < float(np.float32(Wl))) & (ly >= 0) & (ly < float(np.float32(Hl)))
    e = torch.where(inside, ly, zero).long() * Wl + torch.where(inside, lx, zero).long()
    q0 = shadow.q0.reshape(-1)[e]
    n4 = shadow.layers.reshape(-1, 4)[e].long() & 0xffffffff
    u = torch.ones_like(ql) / ql - torch.ones_like(q0) / q0
    ok = inside & (q0 != 0) & (u > 0)
    cnt = lambda x: torch.clamp(x, max=1 << 24).float()  # noqa: E731
    i0 = n4[:, 0]
    i1 = (i0 + n4[:, 1]) & 0xffffffff
    i2 = (i1 + n4[:, 2]) & 0xffffffff
    c0, c1, c2 = cnt(i0), cnt(i1), cnt(i2)
    d = np.float32(shadow.layer)
    k = lambda x: float(np.float32(x) * d)  # noqa: E731
    d1, d3, d7 = float(d), k(3), k(7)
    n = torch.where(u < d1, c0 * _div(u, d1),
                    torch.where(u < d3, c0 + cnt(n4[:, 1]) * _div(u - d1, k(2)),
                                torch.where(u < d7, c1 + cnt(n4[:, 2]) * _div(u - d3, k(4)),
                                            c2 + cnt(n4[:, 3]) * torch.fmin(_div(u - d7, k(8)), zero + 1))))
    return torch.where(ok, n, zero), ql, e, inside


def _transmittance_torch(P, shadow, kappa, bias):
    n, ql, e, inside = _occluders_torch(P, shadow)
    Tr = torch.ones_like(n) / (1.0 + float(np.float32(kappa)) * n)
    if shadow.qfl is not None and shadow.Hl * shadow.Wl:
        qfl = shadow.qfl.reshape(-1)[e]
        behind = inside & (qfl > 0) & (ql * float(np.float32(1) + np.float32(bias)) < qfl)
        Tr = torch.where(behind, torch.zeros_like(Tr), Tr)
    return Tr


def _resolve_torch(src, H, W, s):
    if s == 1:
        return src.clone()
    x = src.reshape(H, s, W, s, 3).to(torch.int32).sum(dim=(1, 3))
    return ((x + (s * s) // 2) // (s * s)).to(torch.uint8)


# ---------------------------------------------------------------------------------------------------------------- fused
class _Frames:
    """The device buffers of a run of frames: allocated once per (S, L, H, W, V, F) and device, reused across a camera path"""
    key = None

    def __init__(self, key, dev):
        S, L, H, W, V, Fc = key[:6]
        self.key = key
        self.ws = torch.empty(strandview_workspace_bytes(S, L, H, W), dtype=torch.uint8, device=dev)
        self.vis_ws = torch.empty(vis.vis_workspace_bytes(V, Fc, H, W), dtype=torch.uint8, device=dev) if Fc else None
        self.qf = torch.empty((H, W), dtype=torch.float32, device=dev) if Fc else None


_frames = None


def _frames_for(S, L, H, W, V, Fc, dev):
    global _frames
    key = (S, L, H, W, V, Fc, str(dev))
    if _frames is None or _frames.key != key:
        _frames = None            # (the old buffers go before the new ones come)
        _frames = _Frames(key, dev)
    return _frames


def _mc(M):
    return (ctypes.c_float * 12)(*[float(x) for x in _m12(M)])


def _raster_fused(pts, v, f32, M, H, W, r, head_bias, near):
    from .diff_gaussian_rasterization import _on_device, _ptr, _stream
    dev = pts.device
    S, L = pts.shape[0], pts.shape[1]
    V, Fc = (v.shape[0], f32.shape[0]) if v is not None else (0, 0)
    fr = _frames_for(S, L, H, W, V, Fc, dev)
    seg = torch.empty((H, W), dtype=torch.int32, device=dev)
    face_out = torch.empty((H, W), dtype=torch.int32, device=dev)
    t = torch.empty((H, W), dtype=torch.float32, device=dev)
    inv = torch.empty((H, W), dtype=torch.float32, device=dev)
    Mc = _mc(M)
    pix = None
    if Fc and H * W:
        pix, _ = vis._view_fused(v, f32, M, H, W, near, None, None, fr.vis_ws, None, None)
    with _on_device(dev):
        L_ = _lib.lib()
        if pix is not None:
            _lib.check(L_.ghr_strandview_face_depth(_stream(), V, _ptr(v) if V else None, Fc, _ptr(f32), ctypes.byref(Mc), float(near),
                                                    H, W, _ptr(pix), _ptr(fr.qf)))
        _lib.check(L_.ghr_strandview_raster(_stream(), S, L, _ptr(pts) if S else None, ctypes.byref(Mc), float(near), H, W, float(r),
                                            float(head_bias), _ptr(pix) if pix is not None else None,
                                            _ptr(fr.qf) if pix is not None else None, _ptr(fr.ws), _ptr(seg) if H * W else None,
                                            _ptr(t) if H * W else None, _ptr(face_out) if H * W else None,
                                            _ptr(inv) if H * W else None))
    return seg, t, face_out, inv


def _shade_fused(pts, v, f32, H, W, seg, face, mode, sh, base):
    from .diff_gaussian_rasterization import _on_device, _ptr, _stream
    dev = pts.device
    S, L = pts.shape[0], pts.shape[1]
    V, Fc = (v.shape[0], f32.shape[0]) if v is not None else (0, 0)
    rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    st = _shading_struct(sh)
    with _on_device(dev):
        _lib.check(_lib.lib().ghr_strandview_shade(_stream(), S, L, _ptr(pts) if S else None, V, _ptr(v) if V else None, Fc,
                                                   _ptr(f32) if Fc else None, H, W, _ptr(seg) if H * W else None,
                                                   _ptr(face) if H * W else None, int(mode), ctypes.byref(st),
                                                   _ptr(base) if base is not None else None, _ptr(rgb) if H * W else None))
    return rgb


_light_frames = None   # the light pass's buffers, cached per (S, L, Hl, Wl, V, F) and device like the camera's


def _light_frames_for(S, L, Hl, Wl, V, Fc, dev):
    global _light_frames
    key = (S, L, Hl, Wl, V, Fc, str(dev))
    if _light_frames is None or _light_frames.key != key:
        _light_frames = None
        _light_frames = _Frames(key, dev)
    return _light_frames


def _opacity_fused(pts, v, f32, Ml, Hl, Wl, rl, layer, near):
    """(q0, layers, qfl or None) of the light view on the device"""
    from .diff_gaussian_rasterization import _on_device, _ptr, _stream
    dev = pts.device
    S, L = pts.shape[0], pts.shape[1]
    V, Fc = (v.shape[0], f32.shape[0]) if v is not None else (0, 0)
    fr = _light_frames_for(S, L, Hl, Wl, V, Fc, dev)
    q0 = torch.empty((Hl, Wl), dtype=torch.float32, device=dev)
    layers = torch.empty((Hl, Wl, 4), dtype=torch.int32, device=dev)
    Mc = _mc(Ml)
    qfl = None
    pix = None
    if Fc and Hl * Wl:
        pix, _ = vis._view_fused(v, f32, Ml, Hl, Wl, near, None, None, fr.vis_ws, None, None)
    with _on_device(dev):
        L_ = _lib.lib()
        if pix is not None:
            qfl = torch.empty((Hl, Wl), dtype=torch.float32, device=dev)
            _lib.check(L_.ghr_strandview_face_depth(_stream(), V, _ptr(v) if V else None, Fc, _ptr(f32), ctypes.byref(Mc), float(near),
                                                    Hl, Wl, _ptr(pix), _ptr(qfl)))
        _lib.check(L_.ghr_strandview_opacity(_stream(), S, L, _ptr(pts) if S else None, ctypes.byref(Mc), float(near), Hl, Wl, float(rl),
                                             float(layer), _ptr(fr.ws), fr.ws.numel(), _ptr(q0) if Hl * Wl else None,
                                             _ptr(layers) if Hl * Wl else None))
    return q0, layers, qfl


def _shadow_struct(shadow, kappa, bias):
    from .diff_gaussian_rasterization import _ptr
    s = _lib.StrandViewShadow()
    s.Ml = (ctypes.c_float * 12)(*[float(x) for x in _m12(shadow.Ml)])
    s.near_w, s.Hl, s.Wl = float(shadow.near), int(shadow.Hl), int(shadow.Wl)
    s.layer, s.kappa, s.bias = float(shadow.layer), float(kappa), float(bias)
    n = shadow.Hl * shadow.Wl
    s.q0 = _ptr(shadow.q0) if n else None
    s.layers = _ptr(shadow.layers) if n else None
    s.qfl = _ptr(shadow.qfl) if n and shadow.qfl is not None else None
    return s


def _shade_shadowed_fused(pts, v, f32, H, W, seg, face, t, mode, sh, base, shadow, kappa, bias):
    from .diff_gaussian_rasterization import _on_device, _ptr, _stream
    dev = pts.device
    S, L = pts.shape[0], pts.shape[1]
    V, Fc = (v.shape[0], f32.shape[0]) if v is not None else (0, 0)
    rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    st, sd = _shading_struct(sh), _shadow_struct(shadow, kappa, bias)
    with _on_device(dev):
        _lib.check(_lib.lib().ghr_strandview_shade_shadowed(
            _stream(), S, L, _ptr(pts) if S else None, V, _ptr(v) if V else None, Fc, _ptr(f32) if Fc else None, H, W,
            _ptr(seg) if H * W else None, _ptr(face) if H * W else None, _ptr(t) if H * W else None, int(mode), ctypes.byref(st),
            _ptr(base) if base is not None else None, ctypes.byref(sd), _ptr(rgb) if H * W else None))
    return rgb


def _resolve_fused(src, H, W, s):
    from .diff_gaussian_rasterization import _on_device, _ptr, _stream
    dst = torch.empty((H, W, 3), dtype=torch.uint8, device=src.device)
    with _on_device(src.device):
        _lib.check(_lib.lib().ghr_strandview_resolve(_stream(), H, W, int(s), _ptr(src) if H * W else None, _ptr(dst) if H * W else None))
    return dst


# ---------------------------------------------------------------------------------------------------------------- public
def _mesh_tensors(mesh, dev):
    if mesh is None:
        return None, None
    if isinstance(mesh, tuple) and all(isinstance(x, torch.Tensor) and x.device == dev and x.is_contiguous() for x in mesh) and \
            mesh[0].dtype == torch.float32 and mesh[1].dtype == torch.int32:
        return mesh                  # already on the device in the kernels' types: a path of frames uploads its mesh once
    va, fa = vis._mesh_arrays(mesh)
    return torch.from_numpy(va).to(dev), torch.from_numpy(fa).to(dev)


def _rasterize(pts, v, f32, M, H, W, r, head_bias, near, fused):
    if fused:
        return _raster_fused(pts, v, f32, M, H, W, r, head_bias, near)
    pix = qf = None
    if v is not None and f32.shape[0]:
        f64 = f32.long()
        pix = vis._rasterize_torch(v, f64, M, H, W, near)
        qf = _face_depth_torch(v, f64, M, H, W, near, pix)
    return _rasterize_torch(pts, M, H, W, r, head_bias, near, pix, qf)


@torch.no_grad()
def rasterize_strands(points, M, H, W, mesh=None, half_width: float = 0.75, head_bias: float = 0.0, near: float = NEAR,
                      fused: bool = True, device=None):
    """``points`` [S, L, 3] under the view (M, H, W), over ``mesh`` (a HeadMesh, (vertices, faces) or None).  Returns
    (pix_to_segment int32, t float32, pix_to_face int32, inv_depth float32), each [H, W], on the device."""
    dev = vis._device(device, fused)
    if fused and dev.type != "cuda":
        raise RuntimeError("rasterize_strands(fused=True) needs a ROCm device: the kernels have no CPU path (fused=False is the "
                           "PyTorch form)")
    _check_scalars(half_width, head_bias)
    pts = _points(points, dev)
    v, f32 = _mesh_tensors(mesh, dev)
    return _rasterize(pts, v, f32, M, int(H), int(W), half_width, head_bias, near, fused)


def _bounding_sphere(points, mesh):
    """(centre float64 [3], radius) of the finite points and mesh vertices: the centre of their bounds, the largest distance from
    it; (0, 1) when there is nothing (or a single place)"""
    parts = [points if isinstance(points, torch.Tensor) else torch.from_numpy(np.array(points, np.float32))]
    if mesh is not None:
        mv = mesh.vertices if hasattr(mesh, "vertices") else mesh[0]
        parts.append(mv if isinstance(mv, torch.Tensor) else torch.from_numpy(np.array(mv, np.float32)))
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    kept = []
    for p in parts:
        p = p.detach().reshape(-1, 3)
        p = p[torch.isfinite(p).all(dim=1)].double()
        if p.shape[0]:
            kept.append(p)
            lo, hi = np.minimum(lo, p.min(dim=0).values.cpu().numpy()), np.maximum(hi, p.max(dim=0).values.cpu().numpy())
    if not kept:
        return np.zeros(3), 1.0
    c = (lo + hi) / 2
    rho = max(float(((p - torch.from_numpy(c).to(p.device)) ** 2).sum(dim=1).max().sqrt()) for p in kept)
    return c, (rho if np.isfinite(rho) and rho > 0 else 1.0)


def light_view(points, mesh=None, light=None, view=None, size=SHADOW_SIZE, distance: float = 8.0):
    """A perspective light camera fitted to the groom: ``(Ml float32 [3, 4], Hl, Wl, rho)``.  The finite points and mesh vertices
    get a bounding sphere (the centre of their bounds, radius ``rho``); the camera sits ``distance * rho`` from the centre along
    ``light`` (a world vector towards the light; default: ``shading_for_view(view)["light"]``, the vector the shading uses) and
    looks at the centre; the focal length makes the sphere fit the map with a margin of two texels.  ``size``: the map's side, or
    (Hl, Wl).  In double on the host, rounded once."""
    Hl, Wl = (int(size), int(size)) if np.ndim(size) == 0 else (int(size[0]), int(size[1]))
    if min(Hl, Wl) < 6:
        raise ValueError("light_view: the light map needs at least 6 texels a side (a margin of two on either side)")
    if not distance > 1.0:
        raise ValueError("light_view: distance must be > 1 (the camera sits outside the bounding sphere)")
    if light is None:
        if view is None:
            raise ValueError("light_view: give light, or view for the shading's own light")
        light = shading_for_view(view[0] if isinstance(view, (tuple, list)) and len(view) == 3 else view)["light"]
    lw = np.asarray(light, np.float64).reshape(3)
    lw = lw / np.linalg.norm(lw)
    c, rho = _bounding_sphere(points, mesh)
    z = -lw                                        # the camera looks from the light at the centre
    up = np.eye(3)[int(np.argmin(np.abs(lw)))]     # the world axis farthest from the light's direction
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    eye = c + distance * rho * lw
    f = (min(Hl, Wl) / 2.0 - 2.0) * np.sqrt(distance * distance - 1.0)   # the sphere's outline: radius f / sqrt(distance^2 - 1)
    K = np.array([[f, 0, Wl / 2.0], [0, f, Hl / 2.0], [0, 0, 1.0]])
    return vis.view_matrix(K, R, -R @ eye).reshape(3, 4), Hl, Wl, rho


class ShadowMap:
    """The deep opacity map of one light view: ``Ml`` float32 [12], ``Hl``, ``Wl``, ``near``, ``q0`` float32 [Hl, Wl], ``layers``
    int32 [Hl, Wl, 4] (the bits of the uint32 counts), ``qfl`` float32 [Hl, Wl] or None (no mesh), and ``layer``."""
    __slots__ = ("Ml", "Hl", "Wl", "near", "q0", "layers", "qfl", "layer")

    def __init__(self, Ml, Hl, Wl, near, q0, layers, qfl, layer):
        self.Ml, self.Hl, self.Wl, self.near, self.q0, self.layers, self.qfl, self.layer = _m12(Ml), Hl, Wl, near, q0, layers, qfl, layer


def _check_shadow_scalars(half_width, layer, kappa, bias):
    if not (np.isfinite(half_width) and half_width > 0):
        raise ValueError("strand_view: the shadow half_width must be finite and > 0")
    if not (np.isfinite(layer) and layer > 0):
        raise ValueError("strand_view: the shadow layer must be finite and > 0")
    if not (np.isfinite(kappa) and kappa >= 0):
        raise ValueError("strand_view: shadow_kappa must be finite and >= 0")
    if not (np.isfinite(bias) and bias >= 0):
        raise ValueError("strand_view: shadow_bias must be finite and >= 0")


def _shadow_map(pts, v, f32, Ml, Hl, Wl, half_width, layer, near, fused):
    if fused:
        q0, layers, qfl = _opacity_fused(pts, v, f32, Ml, Hl, Wl, half_width, layer, near)
    else:
        qfl = None
        if v is not None and f32.shape[0] and Hl * Wl:
            f64 = f32.long()
            qfl = _face_depth_torch(v, f64, Ml, Hl, Wl, near, vis._rasterize_torch(v, f64, Ml, Hl, Wl, near))
        q0, layers = _opacity_torch(pts, Ml, Hl, Wl, half_width, layer, near)
    return ShadowMap(Ml, Hl, Wl, float(near), q0, layers, qfl, float(np.float32(layer)))


@torch.no_grad()
def strand_shadow_map(points, Ml, Hl, Wl, mesh=None, half_width: float = SHADOW_HALF_WIDTH, layer=None, near: float = NEAR,
                      fused: bool = True, device=None) -> ShadowMap:
    """The deep opacity map of ``points`` [S, L, 3] under the light view (Ml, Hl, Wl): the front plane, the four layer counts
    behind it and, with a ``mesh``, the head's inverse depth (the mesh goes through the mesh raster and the face depth in the light
    view).  ``layer``: the depth of the first layer in the light's w units (default: the bounding sphere's radius / 32)."""
    dev = vis._device(device, fused)
    if fused and dev.type != "cuda":
        raise RuntimeError("strand_shadow_map(fused=True) needs a ROCm device: the kernels have no CPU path (fused=False is the "
                           "PyTorch form)")
    if layer is None:
        layer = _bounding_sphere(points, mesh)[1] / SHADOW_LAYERS_PER_RADIUS
    _check_shadow_scalars(half_width, layer, 0.0, 0.0)
    pts = _points(points, dev)
    v, f32 = _mesh_tensors(mesh, dev)
    return _shadow_map(pts, v, f32, Ml, int(Hl), int(Wl), half_width, layer, near, fused)


@torch.no_grad()
def render_strands(points, view, mesh=None, colors=None, mode: str = "kajiya", supersample: int = 2, half_width: float = 0.75,
                   head_bias: float = 0.0, near: float = NEAR, fused: bool = True, device=None, shadows=False,
                   shadow_size=SHADOW_SIZE, shadow_half_width: float = SHADOW_HALF_WIDTH, shadow_layer=None,
                   shadow_kappa: float = SHADOW_KAPPA, shadow_bias: float = SHADOW_BIAS, **shading):
    """The picture of ``points`` [S, L, 3] under ``view`` = (M, H, W): uint8 [H, W, 3] on the device.  ``colors``: [S, 3] per-strand
    base colours, one colour, or None (the default hair colour); ``shading``: the keywords of ``shading_for_view``.
    ``shadows``: False (the unshadowed picture), True (a deep opacity map of ``shadow_size`` is made for this call, from the
    shading's own light: it follows the camera unless ``light=`` is given) or a ``ShadowMap`` (reused: a light fixed in the world
    along a path).  The light map is not supersampled.  Tangent mode has no shadows."""
    dev = vis._device(device, fused)
    if fused and dev.type != "cuda":
        raise RuntimeError("render_strands(fused=True) needs a ROCm device: the kernels have no CPU path (fused=False is the "
                           "PyTorch form)")
    if mode not in MODES:
        raise ValueError("render_strands: mode must be one of %s" % sorted(MODES))
    _check_scalars(half_width, head_bias)
    M, H, W = view
    H, W, s = int(H), int(W), int(supersample)
    Ms, rs = supersampled(M, half_width, s)
    pts = _points(points, dev)
    base = None
    if colors is not None:
        c = colors.detach().cpu().numpy() if isinstance(colors, torch.Tensor) else np.asarray(colors)
        c = np.array(c, np.float32)
        if c.size == 3:
            shading = dict(shading, hair_rgb=c.reshape(3))
        else:
            assert c.shape == (pts.shape[0], 3), (c.shape, tuple(pts.shape))
            base = torch.from_numpy(c).to(dev).contiguous()
    sh = shading_for_view(M, **shading)
    v, f32 = _mesh_tensors(mesh, dev)
    shadow = None
    if shadows is not False and shadows is not None and mode == "kajiya":
        if isinstance(shadows, ShadowMap):
            shadow = shadows
            _check_shadow_scalars(1.0, shadow.layer, shadow_kappa, shadow_bias)
            if shadow.q0.device != dev:
                raise ValueError("render_strands: the ShadowMap is on %s, the picture on %s" % (shadow.q0.device, dev))
        else:
            Ml, Hl, Wl, rho = light_view(pts, None if v is None else (v, f32), light=sh["light"], size=shadow_size)
            layer = rho / SHADOW_LAYERS_PER_RADIUS if shadow_layer is None else shadow_layer
            _check_shadow_scalars(shadow_half_width, layer, shadow_kappa, shadow_bias)
            shadow = _shadow_map(pts, v, f32, Ml, Hl, Wl, shadow_half_width, layer, near, fused)
    seg, t, face, _ = _rasterize(pts, v, f32, Ms, s * H, s * W, rs, head_bias, near, fused)
    if fused:
        if shadow is not None:
            big = _shade_shadowed_fused(pts, v, f32, s * H, s * W, seg, face, t, MODES[mode], sh, base, shadow, shadow_kappa, shadow_bias)
        else:
            big = _shade_fused(pts, v, f32, s * H, s * W, seg, face, MODES[mode], sh, base)
        return _resolve_fused(big, H, W, s)
    big = _shade_torch(pts, v, None if f32 is None else f32.long(), s * H, s * W, seg, face, MODES[mode], sh, base, t=t, shadow=shadow,
                       kappa=shadow_kappa, bias=shadow_bias)
    return _resolve_torch(big, H, W, s)


def camera_path(P_by_frame, speed_up: int = 4, max_frames: int = 200) -> np.ndarray:
    """The interpolated cameras of ``render_video.py`` (its lines 109-175) as [n, 3, 4] float64 pixel matrices K [R | T].
    ``P_by_frame``: frame number -> 3 x 4 projection of a key camera.  Every key is decomposed into K, R, T; the rotations go
    through scipy's RotationSpline over the frame numbers, K and T are blended linearly between neighbouring keys with the
    script's ``alpha``; of the frames frames[0] .. frames[-1] - 1 every ``speed_up``-th is kept, ``max_frames`` at the most.
    The Blender-only parts of the script (the halved intrinsics, its 1080 / 1920 scaling matrix, the (x, -z, y) axis swap) are
    not reproduced: the matrices are in the pixels of the keys."""
    from scipy.spatial.transform import Rotation, RotationSpline
    frames = sorted(int(k) for k in P_by_frame)
    if len(frames) < 2:
        raise ValueError("camera_path: at least two key frames are needed")
    Ks, Rs, Ts = [], [], []
    for fr in frames:
        K, R, t = vis.decompose_projection(np.asarray(P_by_frame[fr], np.float64)[:3, :4])
        Ks.append(K); Rs.append(R); Ts.append(t)
    spline = RotationSpline(frames, Rotation.from_matrix(np.stack(Rs)))
    idx = list(range(frames[0], frames[-1]))
    R_interp = spline(idx).as_matrix()
    out, j = [], 0
    for n, i in enumerate(idx):
        while i >= frames[j + 1]:
            j += 1
        alpha = 1 - (i - frames[j]) / (frames[j + 1] - frames[j])
        K_cur = Ks[j] * alpha + Ks[j + 1] * (1 - alpha)
        T_cur = Ts[j] * alpha + Ts[j + 1] * (1 - alpha)
        out.append(K_cur @ np.concatenate([R_interp[n], T_cur[:, None]], axis=1))
    return np.stack(out)[::int(speed_up)][:int(max_frames)]
