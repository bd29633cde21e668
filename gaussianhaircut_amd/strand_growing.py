"""A network-free initial groom: strands grown from scalp roots through the orientation field of stage 1's strand-aligned hair
Gaussians, over the ``ghr_field_*`` / ``ghr_strands_resample`` entry points of ``libghr_hip.so`` (``csrc/ghr_field.h`` holds the
definition).

The cloud: hair points with a unit line direction (its sign is meaningless), a weight and a colour.  The field at ``x`` under
heading ``t`` sums, over the points with ``d2 < r2``, ``a = m (1 - d2 / r2)^2`` into ``rho``, ``a s d`` into ``v`` (``s`` the sign
that aligns the line ``d`` with ``t``) and ``a f`` into ``c``; ``n`` counts them.  A strand starts at its root along the scalp
normal, blends its heading with ``v / |v|`` by ``beta`` where ``rho >= rho_min``, coasts straight on for at most ``max_coast``
unsupported steps and stops after; ``steps`` is the last point reached by a supported step.  ``resample_strands`` brings the kept
part to ``L`` points with integer spans.

``grow_strands(..., mesh=, avoid=True)`` grows the strands AROUND the head (``csrc/ghr_grow.h``): where the trace
would set ``x += h t`` it asks the head mesh for the closest point and the containment of ``y = x + h t``; a ``y`` whose signed
distance is below ``margin`` is projected to ``margin`` above its closest point, and the part of the heading that points into the
surface is removed (a heading that has nothing else stops the strand head-on).

``fused=False`` is the PyTorch-composed comparator: brute force over all points in chunks, the same expressions elementwise with
``torch.sum`` (another order of summation), for any floating dtype and the only form for CPU tensors.  ``fused=None`` takes the
HIP kernels for contiguous fp32 ROCm tensors and the comparator otherwise; ``fused=True`` raises where HIP does not apply.  The
HIP form's bits depend on nothing but the cloud and a query's (a strand's) own arguments: not on the other queries, their order
or the launch.

The defaults of ``grow_strands`` are look constants, chosen and not measured: ``radius`` twice the median nearest-neighbour
spacing of the cloud (``sqrt(distCUDA2)``), ``step = radius / 2.5``, ``rho_min`` 0.05 of the median ``rho`` at the cloud's own
points, ``beta = 0.5``, ``max_coast = 4``, ``min_steps = 8``, and with ``avoid`` ``margin = step``.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib
from .simple_knn import _C as _knn
from .simple_knn._C import _ptr, _stream
from .utils.general_utils import build_rotation

PAIR_CHUNK = 2 ** 24  # pairs per brute-force chunk of the comparator
NORM_EPS = 1e-8       # GHR_FIELD_NORM_EPS
HEADON_EPS = 1e-4     # GHR_GROW_HEADON_EPS


def _f32(v) -> float:
    """``v`` rounded to fp32, as the Python float the C entry points take and the comparator uses."""
    return float(np.float32(v))


def _hip_applies(*tensors: torch.Tensor) -> bool:
    return all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in tensors)


def _rows3(t, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != 3 or not t.is_floating_point():
        raise ValueError("%s must be a [N, 3] floating tensor" % name)
    return t.detach()


# ---- PyTorch-composed comparator -------------------------------------------------------------------------------------------------

def field_composed(points, directions, weights, colors, x, t, r2: float):
    """The field of the module's definition at ``x [Q, 3]`` under ``t [Q, 3]`` by brute force -> ``rho [Q]``, ``v [Q, 3]``,
    ``c [Q, 3]``, ``n [Q]`` int32.  ``r2`` is used as given, in the tensors' dtype."""
    Q, P = x.shape[0], points.shape[0]
    rows = max(1, PAIR_CHUNK // max(P, 1))
    rho, v, c, n = [], [], [], []
    for s in range(0, Q, rows):
        d = points[None, :, :] - x[s:s + rows, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        inside = d2 < r2
        u = 1 - d2 / r2
        a = torch.where(inside, weights[None, :] * (u * u), torch.zeros((), dtype=d2.dtype, device=d2.device))
        tt = t[s:s + rows, None, :]
        dot = (directions[None, :, 0] * tt[..., 0] + directions[None, :, 1] * tt[..., 1]) + directions[None, :, 2] * tt[..., 2]
        sa = torch.where(dot < 0, -a, a)
        rho.append(a.sum(dim=1))
        v.append((sa[..., None] * directions[None]).sum(dim=1))
        c.append((a[..., None] * colors[None]).sum(dim=1))
        n.append(inside.sum(dim=1).to(torch.int32))
    if not rho:
        z = x.new_zeros(0)
        return z, x.new_zeros(0, 3), x.new_zeros(0, 3), torch.zeros(0, dtype=torch.int32, device=x.device)
    return torch.cat(rho), torch.cat(v), torch.cat(c), torch.cat(n)


def _len3(a: torch.Tensor) -> torch.Tensor:
    return torch.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])


def trace_composed(field_fn, roots, normals, M: int, h: float, beta: float, rho_min: float, max_coast: int):
    """The trace of the module's definition for every root at once; ``field_fn(x, t) -> (rho, v, c, n)``.
    -> ``path [S, M + 1, 3]``, ``steps [S]`` int32, ``rgb [S, 3]``."""
    S, dev, dt = roots.shape[0], roots.device, roots.dtype
    x = roots.clone()
    t = normals / _len3(normals).clamp_min(NORM_EPS)[:, None]
    path = roots[:, None, :].repeat(1, M + 1, 1)
    live = torch.ones(S, dtype=torch.bool, device=dev)
    coast = torch.zeros(S, dtype=torch.int64, device=dev)
    rows = torch.ones(S, dtype=torch.int64, device=dev)
    steps = torch.zeros(S, dtype=torch.int64, device=dev)
    C, R = torch.zeros(S, 3, dtype=dt, device=dev), torch.zeros(S, dtype=dt, device=dev)
    omb = float(torch.tensor(1.0, dtype=dt) - torch.tensor(beta, dtype=dt))   # 1 - beta formed once in the tensors' dtype
    for _ in range(M):
        if not bool(live.any()):
            break
        rho, v, c, _n = field_fn(x, t)
        lv = _len3(v)
        sup = live & (rho >= rho_min) & (lv > 0)
        u = v / torch.where(lv > 0, lv, torch.ones_like(lv))[:, None]
        b = t * omb + u * beta
        tn = b / _len3(b).clamp_min(NORM_EPS)[:, None]
        t = torch.where(sup[:, None], tn, t)
        C = torch.where(sup[:, None], C + c, C)
        R = torch.where(sup, R + rho, R)
        coast = torch.where(sup, torch.zeros_like(coast), coast + 1)
        live = live & (sup | (coast <= max_coast))
        x = torch.where(live[:, None], x + h * t, x)
        rows = rows + live.to(torch.int64)
        idx = torch.nonzero(live)[:, 0]
        path[idx, rows[idx] - 1] = x[idx]
        steps = torch.where(sup, rows - 1, steps)
    ar = torch.arange(M + 1, device=dev)[None, :]
    path = torch.where((ar >= rows[:, None])[..., None], x[:, None, :], path)
    rgb = torch.where((R == 0)[:, None], torch.zeros_like(C), C / torch.where(R == 0, torch.ones_like(R), R)[:, None])
    return path, steps.to(torch.int32), rgb


def trace_guarded_composed(field_fn, mesh, roots, normals, M: int, h: float, beta: float, rho_min: float, max_coast: int,
                           margin: float, headings: bool = False):
    """The guarded trace of ``csrc/ghr_grow.h`` for every root at once: ``trace_composed``'s loop with the head asked at every step
    through ``mesh.closest_point(fused=False)`` and ``mesh.contains(fused=False)`` (both float32) -- the only form on CPU tensors.
    -> ``path [S, M + 1, 3]``, ``steps [S]`` int32, ``rgb [S, 3]``, ``contacts [S]`` int32, ``stop [S]`` uint8 (0 ran out of
    ``M``, 1 coasted out of support, 2 met the head head-on); with ``headings`` also the strands' last headings ``[S, 3]``."""
    from .mesh import _sqrt32
    S, dev, dt = roots.shape[0], roots.device, roots.dtype
    x = roots.clone()
    t = normals / _len3(normals).clamp_min(NORM_EPS)[:, None]
    path = roots[:, None, :].repeat(1, M + 1, 1)
    live = torch.ones(S, dtype=torch.bool, device=dev)
    coast = torch.zeros(S, dtype=torch.int64, device=dev)
    rows = torch.ones(S, dtype=torch.int64, device=dev)
    steps = torch.zeros(S, dtype=torch.int64, device=dev)
    contacts = torch.zeros(S, dtype=torch.int64, device=dev)
    stop = torch.zeros(S, dtype=torch.uint8, device=dev)
    C, R = torch.zeros(S, 3, dtype=dt, device=dev), torch.zeros(S, dtype=dt, device=dev)
    omb = float(torch.tensor(1.0, dtype=dt) - torch.tensor(beta, dtype=dt))   # 1 - beta formed once in the tensors' dtype
    one = torch.ones((), dtype=dt, device=dev)
    for _ in range(M):
        if not bool(live.any()):
            break
        rho, v, c, _n = field_fn(x, t)
        lv = _len3(v)
        sup = live & (rho >= rho_min) & (lv > 0)
        u = v / torch.where(lv > 0, lv, torch.ones_like(lv))[:, None]
        b = t * omb + u * beta
        tn = b / _len3(b).clamp_min(NORM_EPS)[:, None]
        t = torch.where(sup[:, None], tn, t)
        C = torch.where(sup[:, None], C + c, C)
        R = torch.where(sup, R + rho, R)
        coast = torch.where(sup, torch.zeros_like(coast), coast + 1)
        coasted_out = live & ~(sup | (coast <= max_coast))
        stop = torch.where(coasted_out, torch.ones_like(stop), stop)
        live = live & ~coasted_out
        # the guard: y asked of the mesh (a row that is not live asks too; its answer is not used)
        y = x + h * t
        d2, _face, cpt = mesh.closest_point(y, fused=False)
        inside = mesh.contains(y, fused=False)
        d = _sqrt32(d2).to(dt)
        cpt = cpt.to(dt)
        sd = torch.where(inside, -d, d)
        contact = live & (sd < margin)
        corrected = contact & (d2 != 0)
        un = (y - cpt) / torch.where(corrected, d, one)[:, None]
        nrm = torch.where(inside[:, None], -un, un)
        dot = (t[:, 0] * nrm[:, 0] + t[:, 1] * nrm[:, 1]) + t[:, 2] * nrm[:, 2]
        slide = corrected & (dot < 0)
        sl = t - dot[:, None] * nrm
        ln = _len3(sl)
        head_on = slide & (ln <= HEADON_EPS)
        t = torch.where((slide & ~head_on)[:, None], sl / torch.where(ln > 0, ln, one)[:, None], t)
        stop = torch.where(head_on, torch.full_like(stop, 2), stop)
        live = live & ~head_on
        xn = torch.where(corrected[:, None], cpt + margin * nrm, y)
        x = torch.where(live[:, None], xn, x)
        contacts = contacts + (contact & live).to(torch.int64)
        rows = rows + live.to(torch.int64)
        idx = torch.nonzero(live)[:, 0]
        path[idx, rows[idx] - 1] = x[idx]
        steps = torch.where(sup & live, rows - 1, steps)
    ar = torch.arange(M + 1, device=dev)[None, :]
    path = torch.where((ar >= rows[:, None])[..., None], x[:, None, :], path)
    rgb = torch.where((R == 0)[:, None], torch.zeros_like(C), C / torch.where(R == 0, torch.ones_like(R), R)[:, None])
    out = (path, steps.to(torch.int32), rgb, contacts.to(torch.int32), stop)
    return out + (t,) if headings else out


def resample_composed(path: torch.Tensor, steps: torch.Tensor, L: int) -> torch.Tensor:
    """``path [S, M + 1, 3]``, ``steps [S]`` -> ``[S, L, 3]`` by the module's integer spans."""
    S, M = path.shape[0], path.shape[1] - 1
    n = steps.to(torch.int64).clamp(0, M)[:, None]
    num = torch.arange(L, device=path.device, dtype=torch.int64)[None, :] * n
    q, rem = torch.div(num, L - 1, rounding_mode="floor"), num % (L - 1)
    q1 = torch.minimum(q + 1, n)
    a = torch.gather(path, 1, q[..., None].expand(S, L, 3))
    b = torch.gather(path, 1, q1[..., None].expand(S, L, 3))
    w = rem.to(path.dtype) / torch.tensor(float(L - 1), dtype=path.dtype, device=path.device)
    return a + (b - a) * w[..., None]


def _mean_dist2_composed(points: torch.Tensor) -> torch.Tensor:
    """distCUDA2's value by brute force (the comparator's spacing of the cloud)."""
    P = points.shape[0]
    rows = max(1, PAIR_CHUNK // max(P, 1))
    out = []
    for s in range(0, P, rows):
        d = points[None, :, :] - points[s:s + rows, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        ar = torch.arange(s, min(s + rows, P), device=points.device)
        d2[torch.arange(ar.shape[0], device=points.device), ar] = float("inf")
        k = min(3, P)
        out.append(torch.topk(d2, k, dim=1, largest=False).values.sum(dim=1) / 3)
    return torch.cat(out)


# ---- the field ---------------------------------------------------------------------------------------------------------------------

class HairField:
    """The orientation field of a hair-point cloud: ``points [P, 3]``, ``directions [P, 3]`` (normalised here; a zero row stays
    zero), ``weights [P]`` (>= 0), ``colors [P, 3]``, all on one device.  On a ROCm device with fp32 tensors the key-ordered cloud
    and its payload (``ghr_field_build``) are built on first use and kept."""

    def __init__(self, points, directions, weights, colors):
        points, directions, colors = _rows3(points, "points"), _rows3(directions, "directions"), _rows3(colors, "colors")
        weights = weights.detach().reshape(-1)
        P = points.shape[0]
        if P < 1:
            raise ValueError("HairField: the cloud is empty")
        if directions.shape[0] != P or colors.shape[0] != P or weights.shape[0] != P:
            raise ValueError("HairField: points, directions, weights and colors must have one row per point")
        dt = points.dtype
        self.points = points.contiguous()
        d = directions.to(dt)
        self.directions = (d / torch.linalg.norm(d, dim=-1, keepdim=True).clamp_min(1e-20)).contiguous()
        self.weights = weights.to(dt).contiguous()
        self.colors = colors.to(dt).contiguous()
        for name in ("points", "directions", "weights", "colors"):
            if not bool(torch.isfinite(getattr(self, name)).all()):
                raise ValueError("HairField: %s hold non-finite values" % name)
        if bool((self.weights < 0).any()):
            raise ValueError("HairField: weights must be >= 0")
        self._ws = None
        self.bounds = None
        self.order = None

    @classmethod
    def from_model(cls, gaussians, label_threshold: float = 0.5) -> "HairField":
        """The hair Gaussians of a stage-1 model: rows with ``get_label[:, 0] >= label_threshold``, direction the unit longest
        axis, weight ``get_opacity``, colour ``_features_dc``.  Non-finite rows raise ``ValueError`` (as ``distCUDA2`` does)."""
        with torch.no_grad():
            hair = gaussians.get_label[:, 0] >= label_threshold
            xyz = gaussians.get_xyz.detach()[hair]
            scaling = gaussians.get_scaling.detach()[hair]
            R = build_rotation(gaussians._rotation.detach()[hair])
            j = scaling.argsort(dim=-1, descending=True)[:, 0]
            axis = R[torch.arange(R.shape[0], device=R.device), j]
            opacity = gaussians.get_opacity.detach()[hair][:, 0]
            dc = gaussians._features_dc.detach()[hair].reshape(-1, 3)
            for name, t in (("positions", xyz), ("axes", axis), ("opacities", opacity), ("colours", dc)):
                if not bool(torch.isfinite(t).all()):
                    raise ValueError("HairField.from_model: the hair Gaussians' %s hold non-finite values" % name)
            if xyz.shape[0] == 0:
                raise ValueError("HairField.from_model: no Gaussian has label >= %g" % label_threshold)
            return cls(xyz.float(), axis.float(), opacity.float(), dc.float())

    # -- HIP
    @property
    def P(self) -> int:
        return int(self.points.shape[0])

    def hip_applies(self, *more: torch.Tensor) -> bool:
        return _hip_applies(self.points, self.directions, self.weights, self.colors, *more)

    def _use_hip(self, fused: Optional[bool], who: str, *more: torch.Tensor) -> bool:
        if fused is False:
            return False
        ok = self.hip_applies(*more) and all(t.device == self.points.device for t in more)
        if fused and not ok:
            raise ValueError("%s: fused=True needs contiguous float32 tensors on the field's ROCm device" % who)
        return ok

    def workspace(self) -> torch.Tensor:
        """The built cloud (``ghr_field_build``): key order over the points' own bounds, block boxes, payload."""
        if self._ws is None:
            with torch.cuda.device(self.points.device):
                self.bounds = torch.cat(torch.aminmax(self.points, dim=0))
                self.order = _knn.sort_order(_knn.keys(self.points, self.bounds))
                ws = torch.empty(_lib.field_workspace_size(self.P), dtype=torch.uint8, device=self.points.device)
                _lib.check(_lib.lib().ghr_field_build(_stream(), self.P, _ptr(self.points), _ptr(self.order), _ptr(self.directions),
                                                      _ptr(self.weights), _ptr(self.colors), _ptr(ws)))
                self._ws = ws
        return self._ws

    def _key_order(self, rows: torch.Tensor) -> Optional[torch.Tensor]:
        """The permutation that brings ``rows [N, 3]`` into the key order of the cloud's bounds (speed only); None for one wave."""
        if rows.shape[0] <= 64:
            return None
        return _knn.sort_order(_knn.keys(rows, self.bounds))

    def query_hip(self, x: torch.Tensor, t: torch.Tensor, r2: float, sort: bool = True):
        Q, dev = x.shape[0], x.device
        with torch.cuda.device(dev):
            rho = torch.empty(Q, dtype=torch.float32, device=dev)
            v, c = torch.empty(Q, 3, dtype=torch.float32, device=dev), torch.empty(Q, 3, dtype=torch.float32, device=dev)
            n = torch.empty(Q, dtype=torch.int32, device=dev)
            if Q:
                ws = self.workspace()
                order = self._key_order(x) if sort else None
                _lib.check(_lib.lib().ghr_field_query(_stream(), self.P, _ptr(ws), Q, _ptr(x), _ptr(t), _ptr(order), r2, _ptr(rho),
                                                      _ptr(v), _ptr(c), _ptr(n)))
        return rho, v, c, n

    def trace_hip(self, roots, normals, M: int, r2: float, h: float, beta: float, rho_min: float, max_coast: int, sort: bool = True):
        S, dev = roots.shape[0], roots.device
        with torch.cuda.device(dev):
            path = torch.empty(S, M + 1, 3, dtype=torch.float32, device=dev)
            steps = torch.empty(S, dtype=torch.int32, device=dev)
            rgb = torch.empty(S, 3, dtype=torch.float32, device=dev)
            if S:
                ws = self.workspace()
                order = self._key_order(roots) if sort else None
                _lib.check(_lib.lib().ghr_field_trace(_stream(), self.P, _ptr(ws), S, _ptr(roots), _ptr(normals), _ptr(order), M, r2, h,
                                                      beta, rho_min, max_coast, _ptr(path), _ptr(steps), _ptr(rgb)))
        return path, steps, rgb

    def trace_guarded_hip(self, mesh, roots, normals, M: int, r2: float, h: float, beta: float, rho_min: float, max_coast: int,
                          margin: float, sort: bool = True):
        """``ghr_field_trace_guarded``: ``trace_hip`` with ``mesh`` (a ``HeadMesh``) asked at every step.
        -> ``path, steps, rgb, contacts [S] int32, stop [S] uint8``."""
        S, dev = roots.shape[0], roots.device
        with torch.cuda.device(dev):
            path = torch.empty(S, M + 1, 3, dtype=torch.float32, device=dev)
            steps = torch.empty(S, dtype=torch.int32, device=dev)
            rgb = torch.empty(S, 3, dtype=torch.float32, device=dev)
            contacts = torch.empty(S, dtype=torch.int32, device=dev)
            stop = torch.empty(S, dtype=torch.uint8, device=dev)
            if S:
                ws = self.workspace()
                order = self._key_order(roots) if sort else None
                tris, _bounds = mesh._tris_tables(dev)
                grid = mesh._tables(dev)
                _lib.check(_lib.lib().ghr_field_trace_guarded(
                    _stream(), self.P, _ptr(ws), ctypes.byref(mesh._tris_header), _ptr(tris), ctypes.byref(mesh.header), _ptr(grid), S,
                    _ptr(roots), _ptr(normals), _ptr(order), M, r2, h, beta, rho_min, max_coast, margin, _ptr(path), _ptr(steps),
                    _ptr(rgb), _ptr(contacts), _ptr(stop)))
        return path, steps, rgb, contacts, stop

    # -- public
    def query(self, points, headings, radius: Optional[float] = None, fused: Optional[bool] = None):
        """``points [Q, 3]``, ``headings [Q, 3]`` -> ``(rho [Q], v [Q, 3], c [Q, 3], n [Q] int32)``, none normalised.
        ``radius=None``: ``default_radius()``."""
        x, t = _rows3(points, "points").contiguous(), _rows3(headings, "headings").contiguous()
        if x.shape != t.shape:
            raise ValueError("HairField.query: points and headings must have the same shape")
        r = _f32(self.default_radius(fused) if radius is None else radius)
        if not (r > 0 and np.isfinite(r)):
            raise ValueError("HairField.query: radius must be positive and finite")
        r2 = _f32(np.float32(r) * np.float32(r))
        if self._use_hip(fused, "HairField.query", x, t):
            return self.query_hip(x, t, r2)
        dt = self.points.dtype
        return field_composed(self.points, self.directions, self.weights, self.colors, x.to(dt), t.to(dt), r2)

    def default_radius(self, fused: Optional[bool] = None) -> float:
        """Twice the median of ``sqrt(distCUDA2(points))``: two nearest-neighbour spacings of the cloud."""
        if self.P < 2:
            raise ValueError("HairField: a cloud of one point has no spacing; give radius")
        if self._use_hip(fused, "HairField.default_radius"):
            d2 = _knn.distCUDA2(self.points)
        else:
            d2 = _mean_dist2_composed(self.points)
        d2 = d2[torch.isfinite(d2)]
        if d2.numel() == 0:
            raise ValueError("HairField: the cloud has fewer than four points; give radius")
        return _f32(2.0 * float(torch.sqrt(d2).median()))

    def default_rho_min(self, radius: float, fused: Optional[bool] = None) -> float:
        """0.05 of the median ``rho`` at the cloud's own points under their own directions (one query)."""
        rho = self.query(self.points, self.directions, radius=radius, fused=fused)[0]
        return _f32(0.05 * float(rho.median()))


def resample_strands(path: torch.Tensor, steps: torch.Tensor, L: int, fused: Optional[bool] = None) -> torch.Tensor:
    """``path [S, M + 1, 3]``, ``steps [S]`` (integers in 0 .. M) -> ``[S, L, 3]``: point ``k`` lies ``k steps / (L - 1)`` path
    segments from the root, spans by integer division; ``steps == 0`` gives ``L`` copies of the root."""
    if path.dim() != 3 or path.shape[2] != 3 or path.shape[1] < 2 or steps.shape != path.shape[:1]:
        raise ValueError("resample_strands: path must be [S, M + 1, 3] with M >= 1 and steps [S]")
    if L < 2:
        raise ValueError("resample_strands: L must be at least 2")
    S, M = int(path.shape[0]), int(path.shape[1]) - 1
    hip = fused is not False and _hip_applies(path) and steps.is_cuda
    if fused and not hip:
        raise ValueError("resample_strands: fused=True needs a contiguous float32 path on a ROCm device")
    if not hip:
        return resample_composed(path, steps, L)
    with torch.cuda.device(path.device):
        st = steps.to(torch.int32).contiguous()
        out = torch.empty(S, L, 3, dtype=torch.float32, device=path.device)
        if S:
            _lib.check(_lib.lib().ghr_strands_resample(_stream(), S, M, L, _ptr(path), _ptr(st), _ptr(out)))
    return out


@torch.no_grad()
def grow_strands(field: HairField, roots, normals, L: int = 100, radius: Optional[float] = None, step: Optional[float] = None,
                 max_steps: int = 400, rho_min: Optional[float] = None, beta: float = 0.5, max_coast: int = 4, min_steps: int = 8,
                 mesh=None, fused: Optional[bool] = None, avoid: bool = False, margin: Optional[float] = None) -> dict:
    """Grow one strand from every root ``roots [S, 3]`` along ``normals [S, 3]`` through ``field`` and resample it to ``L`` points.

    -> ``dict(points [S', L, 3], keep [S] bool, steps [S] int32, rgb [S', 3], path [S, max_steps + 1, 3], radius, step, rho_min)``:
    ``keep`` marks the strands with ``steps >= min_steps`` that, with ``mesh`` (a ``HeadMesh``), also pass
    ``between_stages.prune_strands``; ``points`` and ``rgb`` hold those, in the roots' order.

    ``avoid=False``: the trace itself knows no mesh; ``mesh`` only prunes afterwards.  ``avoid=True`` (needs ``mesh``): the guarded
    trace of ``csrc/ghr_grow.h`` keeps every step at least ``margin`` off the head (``margin=None``: the step ``h``, a look constant,
    chosen and not measured); the result gains ``contacts [S]`` int32 (contact steps), ``stop [S]`` uint8 (0 ran out of
    ``max_steps``, 1 coasted out of support, 2 met the head head-on) and ``margin``.  ``mesh`` still prunes afterwards."""
    roots, normals = _rows3(roots, "roots").contiguous(), _rows3(normals, "normals").contiguous()
    if roots.shape != normals.shape:
        raise ValueError("grow_strands: roots and normals must have the same shape")
    if L < 2 or max_steps < 1 or max_coast < 0 or not 0.0 <= beta <= 1.0:
        raise ValueError("grow_strands: needs L >= 2, max_steps >= 1, max_coast >= 0 and beta in [0, 1]")
    if avoid and mesh is None:
        raise ValueError("grow_strands: avoid=True needs mesh")
    if margin is not None and not avoid:
        raise ValueError("grow_strands: margin is the guarded trace's; give avoid=True")
    hip = field._use_hip(fused, "grow_strands", roots, normals)
    use = bool(hip)
    r = _f32(field.default_radius(use) if radius is None else radius)
    h = _f32(r / 2.5 if step is None else step)
    rmin = _f32(field.default_rho_min(r, use) if rho_min is None else rho_min)
    if not (r > 0 and h > 0 and rmin > 0):
        raise ValueError("grow_strands: radius, step and rho_min must be positive (got %g, %g, %g)" % (r, h, rmin))
    r2, beta = _f32(np.float32(r) * np.float32(r)), _f32(beta)
    extra = {}
    if avoid:
        m = _f32(h if margin is None else margin)
        if not (m > 0 and np.isfinite(m)):
            raise ValueError("grow_strands: margin must be positive and finite (got %g)" % m)
    if hip and avoid:
        path, steps, rgb, contacts, stop = field.trace_guarded_hip(mesh, roots, normals, int(max_steps), r2, h, beta, rmin,
                                                                   int(max_coast), m)
    elif hip:
        path, steps, rgb = field.trace_hip(roots, normals, int(max_steps), r2, h, beta, rmin, int(max_coast))
    else:
        dt = field.points.dtype

        def fn(x, t):
            return field_composed(field.points, field.directions, field.weights, field.colors, x, t, r2)
        if avoid:
            path, steps, rgb, contacts, stop = trace_guarded_composed(fn, mesh, roots.to(dt), normals.to(dt), int(max_steps), h, beta,
                                                                      rmin, int(max_coast), m)
        else:
            path, steps, rgb = trace_composed(fn, roots.to(dt), normals.to(dt), int(max_steps), h, beta, rmin, int(max_coast))
    if avoid:
        extra = dict(contacts=contacts, stop=stop, margin=m)
    keep = steps >= min_steps
    points = resample_strands(path[keep].contiguous(), steps[keep].contiguous(), L, fused=use)
    if mesh is not None:
        from .between_stages import prune_strands
        points, outside = prune_strands(points, mesh, fused=use)   # (the comparator where the trace was composed)
        keep = keep.clone()
        keep[keep.clone()] = outside
    return dict(points=points, keep=keep, steps=steps, rgb=rgb[keep], path=path, radius=r, step=h, rho_min=rmin, **extra)
