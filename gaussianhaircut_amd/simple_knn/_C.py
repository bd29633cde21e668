"""``distCUDA2(points) -> Tensor[P]``: the mean squared distance of every point to its 3 nearest neighbours, the initial
Gaussian scale of ``create_from_pcd`` (reference ``src/scene/gaussian_model.py:409``), computed exactly on the GPU by the
``ghr_knn_*`` entry points of ``libghr_hip.so`` (``csrc/ghr_knn.h``).

Contract: for point i and every j != i (by index: a duplicate point is a neighbour at distance 0),
d = (dx*dx + dy*dy) + dz*dz in fp32 with dx = p_j.x - p_i.x; three slots b0 <= b1 <= b2 start at FLT_MAX and take d only
when d is strictly smaller than b2, so a d >= FLT_MAX (overflow to inf included) never enters; the result is
((b0 + b1) + b2) / 3.  That is +inf for P = 1 and 2, about FLT_MAX / 3 for P = 3, an empty tensor for P = 0.  The bits do
not depend on the launch schedule, the stream or the order of the input (permuting the points permutes the result), so
data-parallel ranks that build their models apart get identical models.

Kernels run on the current stream of the points' device.  There is no CPU path.  Non-finite coordinates raise ValueError
(one host read-back: this runs once per model).
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

try:  # imported as gaussianhaircut_amd.simple_knn._C
    from .. import _lib
except ImportError:  # imported as top-level `simple_knn._C` (reference-style sys.path layout)
    from gaussianhaircut_amd import _lib


def _ptr(t: Optional[torch.Tensor]) -> ctypes.c_void_p:
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def _stream() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def prepare(points: torch.Tensor) -> torch.Tensor:
    """Checks ``points`` and returns them as a contiguous fp32 [P, 3] tensor on the same device."""
    if not isinstance(points, torch.Tensor):
        raise TypeError("distCUDA2: points must be a torch.Tensor, got %s" % type(points).__name__)
    if not points.is_cuda:
        raise RuntimeError("gaussianhaircut_amd: distCUDA2 points are on %s; the HIP kNN has no CPU path "
                           "(tensors must be on a ROCm device)" % points.device)
    if points.dim() != 2 or points.shape[1] != 3 or not points.is_floating_point():
        raise ValueError("distCUDA2: points must be a [P, 3] floating tensor, got %s %s"
                         % (tuple(points.shape), points.dtype))
    if points.shape[0] >= 2 ** 31:
        raise ValueError("distCUDA2: at most 2^31 - 1 points")
    return points.detach().to(torch.float32).contiguous()


def keys(pts: torch.Tensor, bounds: Optional[torch.Tensor] = None) -> torch.Tensor:
    """63-bit Morton codes of ``prepare``d points (int64 [P]) over ``bounds`` (fp32 [6] on their device: min x, y, z, max x, y, z;
    None: the points' own); they steer the search's speed only."""
    if bounds is None:
        bounds = torch.cat(torch.aminmax(pts, dim=0))
    k = torch.empty(pts.shape[0], dtype=torch.int64, device=pts.device)
    _lib.check(_lib.lib().ghr_knn_keys(_stream(), pts.shape[0], _ptr(pts), _ptr(bounds), _ptr(k)))
    return k


def sort_keys(k: torch.Tensor):
    """The stable sort of the keys: ``.values`` the sorted keys, ``.indices`` the int64 permutation."""
    return torch.sort(k, stable=True)


def sort_order(k: torch.Tensor) -> torch.Tensor:
    """The int64 permutation that sorts the keys."""
    return sort_keys(k).indices


def mean_dist2(pts: torch.Tensor, order: torch.Tensor) -> torch.Tensor:
    """Block boxes and the pruned exact search (``ghr_knn_mean_dist2``) for ``prepare``d points in key ``order``."""
    P = pts.shape[0]
    out = torch.empty(P, dtype=torch.float32, device=pts.device)
    ws = torch.empty(_lib.knn_workspace_size(P), dtype=torch.uint8, device=pts.device)
    _lib.check(_lib.lib().ghr_knn_mean_dist2(_stream(), P, _ptr(pts), _ptr(order), _ptr(ws), _ptr(out)))
    return out


def distCUDA2(points: torch.Tensor) -> torch.Tensor:
    """[P, 3] floating points on a ROCm device -> [P] float32 mean squared distance to the 3 nearest other points."""
    pts = prepare(points)
    with torch.cuda.device(pts.device):
        if pts.shape[0] == 0:
            return torch.empty(0, dtype=torch.float32, device=pts.device)
        if not bool(torch.isfinite(pts).all()):
            raise ValueError("distCUDA2: points hold non-finite coordinates")
        return mean_dist2(pts, sort_order(keys(pts)))
