"""Nearest neighbour between two point clouds: ``knn_points`` / ``knn_gather`` for K = 1, the two functions the reference's
``src/utils/loss_chamfer_utils.py`` takes from pytorch3d, over the ``ghr_nn_*`` / ``ghr_chamfer_point*`` entry points of
``libghr_hip.so`` (``csrc/ghr_nn.h``).

Contract: for query ``x_i`` and every candidate ``y_j``, ``d = (dx*dx + dy*dy) + dz*dz`` (``norm=2``: the SQUARED distance, as
pytorch3d returns it) or ``d = (|dx| + |dy|) + |dz|`` (``norm=1``) with ``dx = y_j.x - x_i.x``, in fp32 without contraction.
``dists[i]`` is the smallest ``d``, ``idx[i]`` the LOWEST index ``j`` among the candidates that reach it.  That is a total order
when no ``d`` is NaN, so both are the same bits for any launch schedule and any permutation of either cloud (permuting ``p2``
renames the indices; on ties the lowest original one still wins).  ``idx`` is always a valid row of ``p2``.  Non-finite
coordinates are the caller's responsibility: the values are then unspecified.  An empty ``p2`` cloud (``lengths2 == 0``) gives
distance 0 and index 0, as do padded query rows.

``fused=False`` is the PyTorch-composed comparator: the same expressions elementwise (no matmul expansion), brute force in chunks
of at most 2^26 pairs, the winner ``torch.where(d == min, arange, P2).min(-1)`` -- the lowest index explicitly, not a property of
``torch.min`` -- for any ``D`` and dtype, CPU tensors too.  ``fused=None`` takes the HIP kernels for contiguous fp32 ROCm tensors
with ``D == 3`` and the comparator otherwise; ``fused=True`` raises where HIP does not apply.  Both are differentiable in ``p1``
and ``p2``: the HIP backward is gather-form (inverted lists in ascending query order, no floating-point atomics), so two runs
give the same bits.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from . import _lib
from .simple_knn import _C as _knn
from .simple_knn._C import _ptr, _stream

KNN = namedtuple("KNN", "dists idx knn")
PAIR_CHUNK = 2 ** 26  # pairs per brute-force chunk of the comparator


def hip_applies(*tensors: Optional[torch.Tensor]) -> bool:
    """Whether the HIP kernels take these clouds: contiguous fp32 ROCm tensors whose last dimension is 3."""
    ts = [t for t in tensors if t is not None]
    return bool(ts) and all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape[-1] == 3 for t in ts)


def _use_hip(fused: Optional[bool], who: str, *tensors: Optional[torch.Tensor]) -> bool:
    if fused is False:
        return False
    ok = hip_applies(*tensors)
    if fused and not ok:
        raise ValueError("%s: fused=True needs contiguous float32 tensors on a ROCm device with D == 3" % who)
    return ok


# ---- PyTorch-composed comparator ---------------------------------------------------------------------------------------------

def _pair_dist(diff: torch.Tensor, norm: int) -> torch.Tensor:
    """d of the contract over the last dimension of ``diff``, summed left to right: (t0 + t1) + t2 for D == 3."""
    t = diff * diff if norm == 2 else diff.abs()
    d = t[..., 0]
    for k in range(1, t.shape[-1]):
        d = d + t[..., k]
    return d


def nearest_composed(x: torch.Tensor, y: torch.Tensor, norm: int = 2) -> Tuple[torch.Tensor, torch.Tensor]:
    """One cloud pair ``x [Px, D]``, ``y [Py, D]`` (Py >= 1) -> ``dists [Px]`` (differentiable in both), ``idx [Px]`` int64."""
    Px, Py = x.shape[0], y.shape[0]
    with torch.no_grad():
        rows = max(1, PAIR_CHUNK // max(Py, 1))
        ar = torch.arange(Py, device=x.device)
        parts = []
        for s in range(0, Px, rows):
            d = _pair_dist(y[None, :, :] - x[s:s + rows, None, :], norm)
            mn = d.min(dim=-1, keepdim=True).values
            parts.append(torch.where(d == mn, ar[None, :], Py).min(dim=-1).values)
        idx = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int64, device=x.device)
        idx = idx.clamp(max=Py - 1)  # every d NaN: unspecified, but a valid row
    return _pair_dist(y[idx] - x, norm), idx


def cosine_term_composed(a: torch.Tensor, b: torch.Tensor, abs_cosine: bool) -> torch.Tensor:
    cos = F.cosine_similarity(a, b, dim=-1, eps=1e-6)
    return 1 - (torch.abs(cos) if abs_cosine else cos)


# ---- HIP -----------------------------------------------------------------------------------------------------------------------

def union_keys(x: torch.Tensor, y: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """63-bit Morton codes of both clouds over the bounds of their union (int64): equal keys mean equal places."""
    xmn, xmx = torch.aminmax(x, dim=0)
    ymn, ymx = torch.aminmax(y, dim=0)
    bounds = torch.cat((torch.minimum(xmn, ymn), torch.maximum(xmx, ymx)))
    return _knn.keys(x, bounds), _knn.keys(y, bounds)


def search_hip(x: torch.Tensor, y: torch.Tensor, norm: int = 2) -> Tuple[torch.Tensor, torch.Tensor]:
    """``ghr_nn_search`` on contiguous fp32 ROCm ``x [Px, 3]``, ``y [Py, 3]`` (Py >= 1): ``dist [Px]`` fp32, ``idx [Px]`` int32."""
    Px, Py = x.shape[0], y.shape[0]
    with torch.cuda.device(x.device):
        dist = torch.empty(Px, dtype=torch.float32, device=x.device)
        idx = torch.empty(Px, dtype=torch.int32, device=x.device)
        if Px == 0:
            return dist, idx
        kx, ky = union_keys(x, y)
        sx, sy = _knn.sort_keys(kx), _knn.sort_keys(ky)
        ws = torch.empty(_lib.nn_workspace_size(Px, Py), dtype=torch.uint8, device=x.device)
        _lib.check(_lib.lib().ghr_nn_search(_stream(), Px, _ptr(x), _ptr(sx.indices), _ptr(sx.values), Py, _ptr(y), _ptr(sy.indices),
                                            _ptr(sy.values), norm, _ptr(ws), _ptr(dist), _ptr(idx)))
    return dist, idx


def inverted_lists(idx: torch.Tensor, Py: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """``start [Py + 1]``, ``members [Px]`` (int64): the queries that chose candidate j are ``members[start[j]:start[j + 1]]`` in
    ascending order.  A stable sort and a search over integers: no floating point decides anything."""
    s = torch.sort(idx.to(torch.int64), stable=True)
    start = torch.searchsorted(s.values, torch.arange(Py + 1, device=idx.device))
    return start.contiguous(), s.indices.contiguous()


def _point_backward(norm, x, y, idx32, g_dist, xn, yn, abs_cosine, g_cos):
    """(d_x, d_y, d_xn, d_yn) of ``ghr_chamfer_point_backward``; the pair whose upstream gradient is None stays None."""
    Px, Py = idx32.shape[0], (y if y is not None else yn).shape[0]
    dev = idx32.device

    def out(rows, want):
        return torch.empty(rows, 3, dtype=torch.float32, device=dev) if want else None

    d_x, d_y = out(Px, g_dist is not None), out(Py, g_dist is not None)
    d_xn, d_yn = out(Px, g_cos is not None), out(Py, g_cos is not None)
    if Px == 0:
        for t in (d_y, d_yn):
            if t is not None:
                t.zero_()
        return d_x, d_y, d_xn, d_yn
    with torch.cuda.device(dev):
        start, members = inverted_lists(idx32, Py)
        g_dist = None if g_dist is None else g_dist.to(torch.float32).contiguous()
        g_cos = None if g_cos is None else g_cos.to(torch.float32).contiguous()
        _lib.check(_lib.lib().ghr_chamfer_point_backward(
            _stream(), Px, Py, norm, _ptr(x if g_dist is not None else None), _ptr(y if g_dist is not None else None), _ptr(idx32),
            _ptr(start), _ptr(members), _ptr(g_dist), _ptr(xn if g_cos is not None else None),
            _ptr(yn if g_cos is not None else None), int(bool(abs_cosine)), _ptr(g_cos), _ptr(d_x), _ptr(d_y), _ptr(d_xn), _ptr(d_yn)))
    return d_x, d_y, d_xn, d_yn


class _NearestHip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, norm):
        dist, idx32 = search_hip(x, y, norm)
        idx = idx32.to(torch.int64)
        ctx.save_for_backward(x, y, idx32)
        ctx.norm = norm
        ctx.mark_non_differentiable(idx)
        return dist, idx

    @staticmethod
    def backward(ctx, g_dist, _g_idx):
        x, y, idx32 = ctx.saved_tensors
        d_x, d_y, _, _ = _point_backward(ctx.norm, x, y, idx32, g_dist, None, None, False, None)
        return d_x, d_y, None


class _CosineHip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xn, yn, idx32, abs_cosine):
        Px, Py = xn.shape[0], yn.shape[0]
        term = torch.empty(Px, dtype=torch.float32, device=xn.device)
        if Px:
            with torch.cuda.device(xn.device):
                _lib.check(_lib.lib().ghr_chamfer_point(_stream(), Px, Py, _ptr(idx32), _ptr(xn), _ptr(yn), int(bool(abs_cosine)),
                                                        None, _ptr(term), None))
        ctx.save_for_backward(xn, yn, idx32)
        ctx.abs_cosine = bool(abs_cosine)
        return term

    @staticmethod
    def backward(ctx, g_cos):
        xn, yn, idx32 = ctx.saved_tensors
        _, _, d_xn, d_yn = _point_backward(2, None, None, idx32, None, xn, yn, ctx.abs_cosine, g_cos)
        return d_xn, d_yn, None, None


def gather_weights_hip(y_weights: torch.Tensor, idx32: torch.Tensor) -> torch.Tensor:
    """``y_weights[idx]`` by ``ghr_chamfer_point`` (no gradient: weights carry none)."""
    Px, Py = idx32.shape[0], y_weights.shape[0]
    w = torch.empty(Px, dtype=torch.float32, device=idx32.device)
    if Px:
        with torch.cuda.device(idx32.device):
            _lib.check(_lib.lib().ghr_chamfer_point(_stream(), Px, Py, _ptr(idx32), None, None, 0, _ptr(y_weights), None, _ptr(w)))
    return w


# ---- public ----------------------------------------------------------------------------------------------------------------------

def _lengths(lengths, N, P, device, name):
    if lengths is None:
        return [P] * N
    if lengths.dim() != 1 or lengths.shape[0] != N:
        raise ValueError("%s must be of shape (N,)" % name)
    out = [int(v) for v in lengths.tolist()]
    if any(v < 0 or v > P for v in out):
        raise ValueError("%s holds a length outside [0, P]" % name)
    return out


def knn_points(p1: torch.Tensor, p2: torch.Tensor, lengths1=None, lengths2=None, norm: int = 2, K: int = 1,
               fused: Optional[bool] = None) -> KNN:
    """``p1 [N, P1, D]``, ``p2 [N, P2, D]`` -> ``KNN(dists [N, P1, 1], idx [N, P1, 1] int64, knn=None)``, the nearest row of
    ``p2[n, :lengths2[n]]`` for every row of ``p1[n, :lengths1[n]]`` under the module's contract.  Rows of ``p1`` at or past
    ``lengths1[n]`` get distance 0 and index 0.  Only ``K == 1``.  The batch is a Python loop."""
    if K != 1:
        raise NotImplementedError("knn_points: only K == 1 is built (got K = %r)" % (K,))
    if norm not in (1, 2):
        raise ValueError("Support for 1 or 2 norm.")
    if p1.dim() != 3 or p2.dim() != 3 or p1.shape[0] != p2.shape[0] or p1.shape[2] != p2.shape[2]:
        raise ValueError("knn_points: p1 and p2 must be [N, P1, D] and [N, P2, D], got %s and %s" % (tuple(p1.shape), tuple(p2.shape)))
    N, P1, _ = p1.shape
    P2 = p2.shape[1]
    use_hip = _use_hip(fused, "knn_points", p1, p2)
    l1, l2 = _lengths(lengths1, N, P1, p1.device, "lengths1"), _lengths(lengths2, N, P2, p1.device, "lengths2")
    dists, idxs = [], []
    for n in range(N):
        if l1[n] == 0 or l2[n] == 0:
            dists.append(p1.new_zeros(P1))
            idxs.append(torch.zeros(P1, dtype=torch.int64, device=p1.device))
            continue
        x, y = p1[n, :l1[n]], p2[n, :l2[n]]
        d, i = _NearestHip.apply(x, y, norm) if use_hip else nearest_composed(x, y, norm)
        if l1[n] < P1:
            d = torch.cat((d, d.new_zeros(P1 - l1[n])))
            i = torch.cat((i, i.new_zeros(P1 - l1[n])))
        dists.append(d)
        idxs.append(i)
    if N == 0:
        return KNN(p1.new_zeros(0, P1, 1), torch.zeros(0, P1, 1, dtype=torch.int64, device=p1.device), None)
    return KNN(torch.stack(dists)[..., None], torch.stack(idxs)[..., None], None)


def knn_gather(x: torch.Tensor, idx: torch.Tensor, lengths=None) -> torch.Tensor:
    """``x [N, M, U]``, ``idx [N, L, K]`` -> ``[N, L, K, U]`` with ``out[n, l, k] = x[n, idx[n, l, k]]``; where ``k`` is at or
    past ``lengths[n]`` (fewer than K candidates existed) the row is zero."""
    N, M, U = x.shape
    _, L, K = idx.shape
    if idx.shape[0] != N:
        raise ValueError("knn_gather: x and idx must share the batch dimension")
    out = x[:, :, None].expand(N, M, K, U).gather(1, idx[:, :, :, None].expand(N, L, K, U))
    if lengths is not None:
        short = torch.arange(K, device=x.device)[None, :] >= lengths[:, None]  # [N, K]
        out = torch.where(short[:, None, :, None], torch.zeros((), dtype=out.dtype, device=out.device), out)
    return out


def point_terms(idx: torch.Tensor, x_normals=None, y_normals=None, abs_cosine: bool = True, y_weights=None,
                fused: Optional[bool] = None):
    """The per-point terms of a chamfer direction from ``idx [N, P1, 1]`` (``knn_points``'): ``1 - cos`` or ``1 - |cos|`` between
    ``x_normals [N, P1, 3]`` and ``y_normals[n, idx]`` (differentiable in both; ``cos = a.b / (max(|a|, eps) max(|b|, eps))``,
    ``eps = 1e-6``) and ``y_weights[n, idx]`` (``[N, P2]``, no gradient) -> ``(term [N, P1] or None, weight [N, P1] or None)``."""
    idx = idx.reshape(idx.shape[0], idx.shape[1])
    N = idx.shape[0]
    normals = x_normals is not None and y_normals is not None
    term = weight = None
    if normals:
        if _use_hip(fused, "point_terms", x_normals, y_normals) and idx.is_cuda:
            i32 = idx.to(torch.int32)
            term = torch.stack([_CosineHip.apply(x_normals[n], y_normals[n], i32[n], abs_cosine) for n in range(N)])
        else:
            near = torch.stack([y_normals[n][idx[n]] for n in range(N)])
            term = cosine_term_composed(x_normals, near, abs_cosine)
    if y_weights is not None:
        w = y_weights.detach()
        if fused is not False and w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and idx.is_cuda:
            i32 = idx.to(torch.int32)
            weight = torch.stack([gather_weights_hip(w[n], i32[n]) for n in range(N)])
        elif fused:
            raise ValueError("point_terms: fused=True needs contiguous float32 weights on a ROCm device")
        else:
            weight = torch.gather(w, 1, idx)
    return term, weight
