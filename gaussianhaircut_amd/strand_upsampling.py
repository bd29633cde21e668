"""Groom upsampling: child strands blended from guide strands.

A groom from ``grow_strands`` has only as many strands as traces that survived, and the strand stage optimises about 30 000 strands
because that is what an iteration can afford.  The reference fills its scalp from 50 000 roots through a latent texture and two
networks; on ``create_from_polylines`` grooms there are no networks.  The geometric answer: the optimised strands are GUIDES, and
every other scalp root gets a strand that is a blend of its 4 nearest guides, each expressed in its own scalp-local frame and
weighted by inverse squared root distance times a shape-similarity gate, so that strands on two sides of a parting are not averaged
into one that stands up between them.  The definition -- every expression and the order of every sum -- is at the top of
csrc/ghr_upsample.h.  Forward only.

    guide_neighbours(guide_roots, child_origins, radius)            -> (nbr [N, 4] int32, nd2 [N, 4])
    upsample_strands(points, guide_frames, child_origins, child_frames, ...) -> dict(points, features, weights, nbr, valid, keep, eps2)
    frames_at(scalp_mesh, face_frames, points)                      -> [..., 3, 3]: the frame of each point's closest scalp face
    frames_from_normals(normals, up)                                -> [..., 3, 3]: a deterministic fallback without UVs

On a ROCm tensor with ``fused=True`` (the default there) the search and the blend are one HIP call each (``ghr_upsample_neighbours``:
brute force through LDS; ``ghr_upsample_blend``: a wave per child, no ``[N, 4, L, 3]`` gather).  ``fused=False`` is the
PyTorch-composed comparator -- the same float32 expressions, a chunked ``[N, G]`` distance with a stable sort, torch's reductions for
the similarity sums -- and the only form for CPU tensors."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _lib

K = 4
TAU = 0.5          # the gate's default threshold: a look constant, chosen and not measured
EPS2_FACTOR = 1e-6  # eps2 = EPS2_FACTOR x median squared nearest-guide-root distance: a look constant, chosen and not measured
EPS2_FLOOR = 1e-12  # where the guides have no such distance (one guide, coincident roots)
_ELEMS = 1 << 22   # elements of the composed form's largest temporary per pass


def _use_fused(fused, t) -> bool:
    if fused is None:
        return bool(t.is_cuda)
    if fused and not t.is_cuda:
        raise RuntimeError("strand_upsampling: the HIP form has no CPU path (fused=False is the composed form)")
    return bool(fused)


def _f32(v) -> float:
    return float(np.float32(v))


def _r2(radius) -> float:
    r2 = math.inf if radius is None else _f32(np.float32(radius) * np.float32(radius))
    if not r2 > 0:
        raise ValueError("strand_upsampling: radius must be positive, got %r" % (radius,))
    return r2


def _rows(t, tail, name) -> torch.Tensor:
    t = torch.as_tensor(t).detach()
    if t.dim() != 1 + len(tail) or tuple(t.shape[1:]) != tuple(tail):
        raise ValueError("strand_upsampling: %s must be [*, %s], got %s" % (name, ", ".join(map(str, tail)), tuple(t.shape)))
    return t.float().contiguous()


def _on(device, **tensors):
    for name, t in tensors.items():
        if t.device != device:
            raise ValueError("strand_upsampling: %s on %s, the guides on %s" % (name, t.device, device))


# ---- neighbours ---------------------------------------------------------------------------------------------------------------------
def _neighbours_composed(gr, co, r2):
    G, N = int(gr.shape[0]), int(co.shape[0])
    dev = gr.device
    nbr = torch.full((N, K), -1, dtype=torch.int32, device=dev)
    nd2 = torch.full((N, K), math.inf, dtype=torch.float32, device=dev)
    inf = torch.tensor(math.inf, dtype=torch.float32, device=dev)
    rows = max(1, _ELEMS // max(G, 1))
    for lo in range(0, N, rows):
        q = co[lo:lo + rows]
        dx, dy, dz = (gr[None, :, c] - q[:, None, c] for c in range(3))
        d2 = ((dx * dx) + (dy * dy)) + (dz * dz)
        d2 = torch.where(d2 < inf, d2, inf)  # a candidate at +inf or NaN is never taken
        d, j = torch.sort(d2, dim=1, stable=True)
        d, j = d[:, :K], j[:, :K]
        keep = (d < inf) & ~(d > r2)
        nbr[lo:lo + rows, :d.shape[1]] = torch.where(keep, j, torch.full_like(j, -1)).to(torch.int32)
        nd2[lo:lo + rows, :d.shape[1]] = torch.where(keep, d, inf)
    return nbr, nd2


def guide_neighbours(guide_roots, child_origins, radius=None, fused: Optional[bool] = None):
    """``guide_roots [G, 3]``, ``child_origins [N, 3]`` -> ``nbr [N, 4]`` int32: the 4 nearest guides of every child by
    ``((dx*dx)+(dy*dy))+(dz*dz)``, ascending, equal distances to the lower index, and ``nd2 [N, 4]`` float32 their squared
    distances; ``-1`` and ``+inf`` where the squared distance exceeds ``radius**2`` (float32) or fewer than 4 guides exist."""
    gr, co = _rows(guide_roots, (3,), "guide_roots"), _rows(child_origins, (3,), "child_origins")
    _on(gr.device, child_origins=co)
    if gr.shape[0] < 1:
        raise ValueError("strand_upsampling: no guides")
    r2 = _r2(radius)
    if not _use_fused(fused, gr):
        return _neighbours_composed(gr, co, r2)
    from .diff_gaussian_rasterization import _on_device, _ptr, _stream
    N = int(co.shape[0])
    nbr = torch.empty((N, K), dtype=torch.int32, device=gr.device)
    nd2 = torch.empty((N, K), dtype=torch.float32, device=gr.device)
    with _on_device(gr.device):
        _lib.check(_lib.lib().ghr_upsample_neighbours(_stream(), int(gr.shape[0]), _ptr(gr), N, _ptr(co), r2, _ptr(nbr), _ptr(nd2)))
    return nbr, nd2


def default_eps2(guide_roots, fused: Optional[bool] = None) -> float:
    """``1e-6`` times the median squared distance from a guide root to its nearest other guide root (float32 expressions,
    ``strand_shape.nearest_roots``); ``1e-12`` where no such distance exists or the median is 0.  The factor is a look constant,
    chosen and not measured: it only keeps a child that sits on a guide's root from dividing by 0, and a child nearer to a guide
    than a thousandth of the guide spacing takes that guide alone."""
    from .strand_shape import nearest_roots
    gr = _rows(guide_roots, (3,), "guide_roots")
    first = nearest_roots(gr, None, fused=_use_fused(fused, gr))[:, 0].long()
    has = first >= 0
    if not bool(has.any()):
        return EPS2_FLOOR
    a, b = gr[has], gr[first[has]]
    dx, dy, dz = (b[:, c] - a[:, c] for c in range(3))
    med = float(torch.median(((dx * dx) + (dy * dy)) + (dz * dz)))
    e = _f32(np.float32(EPS2_FACTOR) * np.float32(med))
    return e if e > 0 and math.isfinite(e) else EPS2_FLOOR


# ---- the blend ----------------------------------------------------------------------------------------------------------------------
def _mtv(M, x):
    """M^T x with sds_mtv's bracketing; M [..., 3, 3], x [..., 3]"""
    return torch.stack([(M[..., 0, c] * x[..., 0] + M[..., 1, c] * x[..., 1]) + M[..., 2, c] * x[..., 2] for c in range(3)], dim=-1)


def _mv(M, x):
    return torch.stack([(M[..., r, 0] * x[..., 0] + M[..., r, 1] * x[..., 1]) + M[..., r, 2] * x[..., 2] for r in range(3)], dim=-1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _blend_composed(gp, gM, gf, co, cM, nbr, nd2, eps2, tau):
    G, L = int(gp.shape[0]), int(gp.shape[1])
    N, F = int(co.shape[0]), (0 if gf is None else int(gf.shape[1]))
    dev = gp.device
    out = torch.empty((N, L, 3), dtype=torch.float32, device=dev)
    w_out = torch.empty((N, K), dtype=torch.float32, device=dev)
    of = torch.empty((N, F), dtype=torch.float32, device=dev)
    valid = torch.empty(N, dtype=torch.uint8, device=dev)
    eps2_t = torch.tensor(eps2, dtype=torch.float32, device=dev)
    rows = max(1, _ELEMS // (K * L * 3))
    for lo in range(0, N, rows):
        e4, d4 = nbr[lo:lo + rows].long(), nd2[lo:lo + rows]
        ok = ((e4 >= 0) & (e4 < G)).to(torch.int32).cumprod(dim=1).bool()    # the leading entries inside [0, G)
        g = torch.where(ok, e4, torch.zeros_like(e4))
        P, M = gp[g], gM[g]                                                    # [n, 4, L, 3], [n, 4, 3, 3]
        e = _mtv(M[:, :, None], P[:, :, 1:] - P[:, :, :-1])                    # [n, 4, L - 1, 3]
        D, A = _dot(e, e[:, :1]).sum(-1), _dot(e, e).sum(-1)                   # [n, 4]
        den = torch.sqrt(A) * torch.sqrt(A[:, :1])
        pos = den > 0
        s = torch.where(pos, D / torch.where(pos, den, torch.ones_like(den)), torch.zeros_like(den))
        if tau is None:
            q = torch.ones_like(s)
        else:
            t = torch.tensor(tau, dtype=torch.float32, device=dev)
            x = (s - t) / (1.0 - t)
            q = torch.where(x < 0, torch.zeros_like(x), torch.where(x > 1, torch.ones_like(x), x))
        q = torch.cat([torch.ones_like(q[:, :1]), q[:, 1:]], dim=1)
        a = torch.where(ok, q / (torch.where(ok, d4, torch.zeros_like(d4)) + eps2_t), torch.zeros_like(q))
        W = ((a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3]                          # (a_k = +0 beyond the list: the sum in k order)
        has = ok[:, 0]
        w = torch.where(has[:, None], a / torch.where(has, W, torch.ones_like(W))[:, None], torch.zeros_like(a))
        r = _mtv(M[:, :, None], P - P[:, :, :1])                               # [n, 4, L, 3]
        terms = torch.where(ok[:, :, None, None], w[:, :, None, None] * r, torch.zeros_like(r))
        Pl = ((terms[:, 0] + terms[:, 1]) + terms[:, 2]) + terms[:, 3]
        o = co[lo:lo + rows]
        pts = o[:, None] + _mv(cM[lo:lo + rows, None], Pl)
        pts[:, 0] = o
        out[lo:lo + rows] = torch.where(has[:, None, None], pts, o[:, None].expand_as(pts))
        if F:
            ft = torch.where(ok[:, :, None], w[:, :, None] * gf[g], torch.zeros((), dtype=torch.float32, device=dev))
            of[lo:lo + rows] = ((ft[:, 0] + ft[:, 1]) + ft[:, 2]) + ft[:, 3]
        w_out[lo:lo + rows] = w
        valid[lo:lo + rows] = has.to(torch.uint8)
    return out, w_out, of, valid


def _blend_fused(gp, gM, gf, co, cM, nbr, nd2, eps2, tau):
    from .diff_gaussian_rasterization import _on_device, _ptr, _stream
    G, L = int(gp.shape[0]), int(gp.shape[1])
    N, F = int(co.shape[0]), (0 if gf is None else int(gf.shape[1]))
    dev = gp.device
    out = torch.empty((N, L, 3), dtype=torch.float32, device=dev)  # (every element is written)
    w = torch.empty((N, K), dtype=torch.float32, device=dev)
    of = torch.empty((N, F), dtype=torch.float32, device=dev)
    valid = torch.empty(N, dtype=torch.uint8, device=dev)
    with _on_device(dev):
        _lib.check(_lib.lib().ghr_upsample_blend(_stream(), G, L, _ptr(gp), _ptr(gM), _ptr(gf) if F else None, F, N, _ptr(co), _ptr(cM),
                                                 _ptr(nbr), _ptr(nd2), eps2, 0.0 if tau is None else tau, 0 if tau is None else 1,
                                                 _ptr(out), _ptr(w), _ptr(of) if F else None, _ptr(valid)))
    return out, w, of, valid


@torch.no_grad()
def upsample_strands(points, guide_frames, child_origins, child_frames, features=None, radius=None, eps2=None, tau=TAU,
                     neighbours=None, mesh=None, fused: Optional[bool] = None) -> dict:
    """Blend a child strand for every root ``child_origins [N, 3]`` (frames ``child_frames [N, 3, 3]``, ``local2world`` with columns
    tangent, bitangent, normal) from the guides ``points [G, L, 3]`` (frames ``guide_frames [G, 3, 3]``; see ``frames_at``).

    -> ``dict(points [N, L, 3], features [N, F], weights [N, 4], nbr [N, 4] int32, valid [N] bool, keep [N] bool, eps2)``, every row
    in the children's order.  ``valid`` marks the children with a guide inside ``radius`` (``None``: no cut); an invalid child's
    strand is its origin repeated, its weights and features 0.  ``keep`` marks the valid children that, with ``mesh`` (a
    ``HeadMesh``), also pass ``between_stages.prune_strands``: ``points[keep]`` is the groom to export.

    ``features [G, F]`` (for instance the ``rgb`` that ``grow_strands`` returns) are blended with the strands' weights.
    ``neighbours=(nbr, nd2)`` reuses a table of ``guide_neighbours``.  ``tau`` in ``[-1, 1)`` gates a later neighbour by the cosine
    ``s`` between its segments and the nearest guide's, in the two guides' own frames: weight ``clamp((s - tau) / (1 - tau), 0, 1)``;
    ``tau=None`` switches the gate off.  ``eps2=None``: ``default_eps2``.  ``tau = 0.5`` and the ``1e-6`` of ``eps2`` are look
    constants, chosen and not measured."""
    gp = torch.as_tensor(points).detach()
    if gp.dim() != 3 or gp.shape[-1] != 3 or gp.shape[1] < 2 or gp.shape[0] < 1:
        raise ValueError("upsample_strands: points must be [G, L, 3] with G >= 1 and L >= 2, got %s" % (tuple(gp.shape),))
    gp = gp.float().contiguous()
    G = int(gp.shape[0])
    gM, co, cM = _rows(guide_frames, (3, 3), "guide_frames"), _rows(child_origins, (3,), "child_origins"), _rows(child_frames, (3, 3), "child_frames")
    if gM.shape[0] != G or cM.shape[0] != co.shape[0]:
        raise ValueError("upsample_strands: one frame per guide and per child")
    gf = None
    if features is not None:
        gf = torch.as_tensor(features).detach().float().reshape(G, -1).contiguous()
        if gf.shape[1] == 0:
            gf = None
    _on(gp.device, guide_frames=gM, child_origins=co, child_frames=cM, **({} if gf is None else dict(features=gf)))
    use = _use_fused(fused, gp)
    if tau is not None:
        tau = _f32(tau)
        if not -1.0 <= tau < 1.0:
            raise ValueError("upsample_strands: tau must lie in [-1, 1) (None: no gate), got %r" % (tau,))
    roots = gp[:, 0].contiguous()
    e2 = default_eps2(roots, fused=use) if eps2 is None else _f32(eps2)
    if not (e2 > 0 and math.isfinite(e2)):
        raise ValueError("upsample_strands: eps2 must be positive and finite, got %r" % (eps2,))
    if neighbours is None:
        nbr, nd2 = guide_neighbours(roots, co, radius, fused=use)
    else:
        nbr, nd2 = neighbours
        nbr, nd2 = nbr.to(torch.int32).contiguous(), nd2.float().contiguous()
        _on(gp.device, nbr=nbr, nd2=nd2)
        if tuple(nbr.shape) != (co.shape[0], K) or nbr.shape != nd2.shape:
            raise ValueError("upsample_strands: neighbours must be (nbr [N, 4], nd2 [N, 4])")
    if co.shape[0] == 0:
        dev = gp.device
        out, w = gp.new_zeros((0, gp.shape[1], 3)), gp.new_zeros((0, K))
        of, valid = gp.new_zeros((0, 0 if gf is None else gf.shape[1])), torch.zeros(0, dtype=torch.uint8, device=dev)
    else:
        out, w, of, valid = (_blend_fused if use else _blend_composed)(gp, gM, gf, co, cM, nbr, nd2, e2, tau)
    valid = valid.bool()
    keep = valid
    if mesh is not None and int(out.shape[0]) > 0:
        from .between_stages import prune_strands
        keep = valid & prune_strands(out, mesh, fused=use)[1]
    return dict(points=out, features=of, weights=w, nbr=nbr, valid=valid, keep=keep, eps2=e2)


# ---- frames -------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def frames_at(scalp_mesh, face_frames, points, fused: Optional[bool] = None) -> torch.Tensor:
    """``[..., 3, 3]``: for every point the frame ``face_frames[f]`` (``strand_generator.scalp_frames`` of the same mesh) of the
    scalp face ``f`` that holds its closest point (``HeadMesh.closest_point``'s face output: the lowest index among the faces at
    that distance).  The guides' roots get their frames this way.  A point with a non-finite coordinate gets the identity."""
    pts = torch.as_tensor(points).detach().float()
    face_frames = torch.as_tensor(face_frames).float().to(pts.device)
    if face_frames.dim() != 3 or tuple(face_frames.shape[1:]) != (3, 3) or face_frames.shape[0] != len(scalp_mesh.faces):
        raise ValueError("frames_at: face_frames must be [F, 3, 3] with one frame per face of the mesh")
    _, face, _ = scalp_mesh.closest_point(pts, fused=_use_fused(fused, pts))
    face = face.long()
    eye = torch.eye(3, dtype=torch.float32, device=pts.device)
    return torch.where((face >= 0)[..., None, None], face_frames[face.clamp(min=0)], eye).contiguous()


def frames_from_normals(normals, up=(0.0, 1.0, 0.0)) -> torch.Tensor:
    """``[..., 3, 3]`` float32 frames (columns tangent, bitangent, normal) from normals alone, for a scalp without UVs: on the host
    in float64, then rounded.  ``n`` is the normalised normal, ``t = normalise(up x n)``, ``b = n x t``.  Where ``up`` and ``n`` are
    parallel (``|up x n| < 1e-8``) the second axis is the unit axis in which ``|n|`` is smallest (the lowest index among equals).
    A zero or non-finite normal gets the identity.  Frames made this way turn about the normal from root to root only as ``up x n``
    does: use ``scalp_frames`` where the scalp has UVs."""
    nrm = torch.as_tensor(normals).detach()
    dev = nrm.device
    n = nrm.double().cpu()
    if n.shape[-1] != 3:
        raise ValueError("frames_from_normals: normals must be [..., 3]")
    u = torch.tensor([float(x) for x in up], dtype=torch.float64)
    if not float(u.norm()) > 0:
        raise ValueError("frames_from_normals: up must not be zero")
    u = u / u.norm()
    ln = n.norm(dim=-1, keepdim=True)
    good = ((ln > 0) & torch.isfinite(ln))[..., 0]
    n = torch.where(good[..., None], n / torch.where(good[..., None], ln, torch.ones_like(ln)), torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand_as(n))
    t = torch.linalg.cross(u.expand_as(n), n)
    par = t.norm(dim=-1) < 1e-8
    a = n.abs()
    first = torch.where((a[..., 0] <= a[..., 1]) & (a[..., 0] <= a[..., 2]), 0, torch.where(a[..., 1] <= a[..., 2], 1, 2))
    axis = torch.nn.functional.one_hot(first, 3).double()
    t = torch.where(par[..., None], torch.linalg.cross(axis, n), t)
    t = t / t.norm(dim=-1, keepdim=True)
    b = torch.linalg.cross(n, t)
    frames = torch.stack([t, b, n], dim=-1)
    frames = torch.where(good[..., None, None], frames, torch.eye(3, dtype=torch.float64).expand_as(frames))
    return frames.float().contiguous().to(dev)
