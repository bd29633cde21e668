"""A preview of the groom: strands drawn as depth-tested polylines over the head mesh (csrc/ghr_strandview.h) --
the last step of the reference's ``run.sh``, ``src/postprocessing/render_video.py``, without Blender.

``rasterize_strands`` gives the four planes of one view (``pix_to_segment``, ``t``, ``pix_to_face``, ``inv_depth``),
``render_strands`` the shaded uint8 picture, ``camera_path`` the script's interpolated cameras as 3 x 4 pixel matrices.
``fused=True`` launches the HIP kernels (ROCm tensors only: there is no CPU path); ``fused=False`` evaluates the PyTorch-composed
comparator on any device: the same float32 expressions in the same operand order, brute force in pixel chunks over all segments
whose widened box meets the chunk's pixel range -- the tile lists change which segments a pixel looks at, never the winner.
The definition is this package's own and is stated at the top of ``csrc/ghr_strandview.h``.  A view is ``(M, H, W)`` as in
``visibility.py``.
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


def _shade_torch(points, v, f, H, W, seg, face, mode, sh, base=None):
    """uint8 [H, W, 3] of the definition; v / f may be None (no mesh)"""
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
            lit = sc["ambient"] + sc["kd"] * torch.fmax(c, -c)
            out[on] = torch.stack([_quant8(sc["head_rgb"][k] * lit) for k in range(3)], dim=1)
    return out.reshape(H, W, 3)


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


@torch.no_grad()
def render_strands(points, view, mesh=None, colors=None, mode: str = "kajiya", supersample: int = 2, half_width: float = 0.75,
                   head_bias: float = 0.0, near: float = NEAR, fused: bool = True, device=None, **shading):
    """The picture of ``points`` [S, L, 3] under ``view`` = (M, H, W): uint8 [H, W, 3] on the device.  ``colors``: [S, 3] per-strand
    base colours, one colour, or None (the default hair colour); ``shading``: the keywords of ``shading_for_view``."""
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
    seg, _, face, _ = _rasterize(pts, v, f32, Ms, s * H, s * W, rs, head_bias, near, fused)
    if fused:
        big = _shade_fused(pts, v, f32, s * H, s * W, seg, face, MODES[mode], sh, base)
        return _resolve_fused(big, H, W, s)
    big = _shade_torch(pts, v, None if f32 is None else f32.long(), s * H, s * W, seg, face, MODES[mode], sh, base)
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
