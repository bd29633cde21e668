"""``chamfer_distance`` with the signature, defaults, return structure and error messages of the reference's
``src/utils/loss_chamfer_utils.py`` (which both strand scripts import), without pytorch3d: the nearest-neighbour search and the
per-point terms are ``gaussianhaircut_amd.nearest`` (HIP kernels of ``csrc/ghr_nn.h``, or their PyTorch-composed comparator with
``fused=False``).  The reductions after the per-point values are plain torch operations.

What the reference does and a reader might not expect, kept because it changes values:

* distances are SQUARED for ``norm=2``; ties go to the lowest index (``nearest``'s contract);
* when ``y_weights`` is given, ``x_weights`` is multiplied IN PLACE by ``y_weights[idx]`` (a tensor of ones is made when only
  ``y_weights`` was passed); the second direction then reads the already-multiplied tensor and multiplies the caller's
  ``y_weights`` in place the same way; the weights returned ARE those tensors;
* ``batch_reduction="mean"`` divides by the sum of the (multiplied) weights when there are weights, by ``max(N, 1)`` otherwise;
* a weight tensor that sums to zero ends its direction early with a PAIR ``(0 * sum, 0 * sum)``; ``chamfer_distance`` unpacks
  four values from every direction, so that case raises ``ValueError`` there, as it does in the reference;
* the second direction passes the features through, the first does not; ``abs_cosine`` defaults to True;
* weights carry no gradient.  A pytorch3d ``Pointclouds`` object is refused: pytorch3d is not a dependency.
"""
from __future__ import annotations

from typing import Optional

import torch

try:  # imported as gaussianhaircut_amd.utils.loss_chamfer_utils
    from .. import nearest
except ImportError:  # imported as top-level `utils.loss_chamfer_utils` (reference-style sys.path layout)
    from gaussianhaircut_amd import nearest


def _check_reductions(batch_reduction, point_reduction) -> None:
    for name, value in (("batch_reduction", batch_reduction), ("point_reduction", point_reduction)):
        if value is not None and value not in ("mean", "sum"):
            raise ValueError('%s must be one of ["mean", "sum"] or None' % name)
    if point_reduction is None and batch_reduction is not None:
        raise ValueError("Batch reduction must be None if point_reduction is None")


def _cloud(points, lengths, normals):
    """A padded cloud ``[N, P, D]``, its per-cloud lengths (all P when none were given) and its normals."""
    if type(points).__name__ == "Pointclouds" or hasattr(points, "points_padded"):
        raise TypeError("chamfer_distance: Pointclouds objects are not supported (pytorch3d is not a dependency of "
                        "gaussianhaircut_amd); pass points_padded(), num_points_per_cloud() and normals_padded()")
    if not torch.is_tensor(points):
        raise ValueError("The input pointclouds should be either Pointclouds objects or torch.Tensor of shape "
                         "(minibatch, num_points, 3).")
    if points.ndim != 3:
        raise ValueError("Expected points to be of shape (N, P, D)")
    if lengths is None:
        lengths = torch.full((points.shape[0],), points.shape[1], dtype=torch.int64, device=points.device)
    else:
        if lengths.ndim != 1 or lengths.shape[0] != points.shape[0]:
            raise ValueError("Expected lengths to be of shape (N,)")
        if lengths.max() > points.shape[1]:
            raise ValueError("A length value was too long")
    if normals is not None and normals.ndim != 3:
        raise ValueError("Expected normals to be of shape (N, P, 3")
    return points, lengths, normals


def _check_weights(w, N, P, name, size):
    if w.shape[0] != N or w.shape[1] != P:
        raise ValueError("%s must be of shape (N, %s)." % (name, size))
    if not (w >= 0).all():
        raise ValueError("%s cannot be negative." % name)
    return bool(w.sum() == 0.0)


def _one_direction(x, y, x_lengths, y_lengths, x_normals=None, y_normals=None, x_features=None, y_features=None,
                   x_weights=None, y_weights=None, batch_reduction=None, point_reduction=None, norm: int = 2,
                   abs_cosine: bool = False, norm_features: int = 2, fused: Optional[bool] = None):
    """From every point of x to its nearest point of y: ``(distance, normals term or None, features term or None, weights)``."""
    with_normals = x_normals is not None and y_normals is not None
    with_features = x_features is not None and y_features is not None
    N, P1, D = x.shape
    P2 = y.shape[1]
    ragged = bool((x_lengths != P1).any())
    padded = torch.arange(P1, device=x.device)[None] >= x_lengths[:, None]  # [N, P1]
    if y.shape[0] != N or y.shape[2] != D:
        raise ValueError("y does not have the correct shape.")

    for w, P, name, size in ((x_weights, P1, "x_weights", "P1"), (y_weights, P2, "y_weights", "P2")):
        if w is not None and _check_weights(w, N, P, name, size):
            # nothing has weight: zero, still attached to x (x_weights is None here only when y_weights sums to zero)
            nothing = x.sum(2) * x_weights
            if batch_reduction in ("mean", "sum"):
                return nothing.sum() * 0.0, nothing.sum() * 0.0
            return nothing * 0.0, nothing * 0.0

    nn = nearest.knn_points(x, y, lengths1=x_lengths, lengths2=y_lengths, norm=norm, K=1, fused=fused)
    cham = nn.dists[..., 0]  # [N, P1]
    term, gathered = nearest.point_terms(nn.idx, x_normals if with_normals else None, y_normals if with_normals else None,
                                         abs_cosine, y_weights, fused=fused)
    if ragged:
        cham = cham.masked_fill(padded, 0.0)

    if y_weights is not None:
        if x_weights is None:
            x_weights = torch.ones(N, P1, device=y_weights.device)
        gathered = gathered.masked_fill((y_lengths <= 0)[:, None], 0.0)  # an empty cloud has no weight to give
        x_weights *= gathered.view(N, P1)  # in place: the caller's tensor
    if x_weights is not None:
        cham = cham * x_weights.view(N, P1)

    cham_normals = x.new_zeros(())
    if with_normals:
        cham_normals = term
        if ragged:
            cham_normals = cham_normals.masked_fill(padded, 0.0)
        if x_weights is not None:
            cham_normals = cham_normals * x_weights.view(N, P1)

    cham_features = None
    if with_features:
        near = nearest.knn_gather(y_features, nn.idx, y_lengths)[..., 0, :]
        if norm_features == 2:
            cham_features = ((x_features - near) ** 2).mean(dim=2)
        elif norm_features == 1:
            cham_features = (x_features - near).abs().mean(dim=2)
        else:
            raise RuntimeError("No active exception to reraise")  # what the reference's bare `raise` gives: 1 or 2 only
        if ragged:
            cham_features = cham_features.masked_fill(padded, 0.0)
        if x_weights is not None:
            cham_features = cham_features * x_weights.view(N, P1)

    terms = [cham, cham_normals if with_normals else None, cham_features]
    if point_reduction is not None:
        terms = [None if t is None else t.sum(1) for t in terms]  # [N]
        if point_reduction == "mean":
            per_cloud = x_lengths.clamp(min=1)
            terms = [None if t is None else t / per_cloud for t in terms]
        if batch_reduction is not None:
            terms = [None if t is None else t.sum() for t in terms]
            if batch_reduction == "mean":
                div = x_weights.sum() if x_weights is not None else max(N, 1)
                terms = [None if t is None else t / div for t in terms]
    return terms[0], terms[1], terms[2], x_weights


def chamfer_distance(x, y, x_lengths=None, y_lengths=None, x_normals=None, y_normals=None, x_features=None, y_features=None,
                     x_weights=None, y_weights=None, batch_reduction: Optional[str] = "mean",
                     point_reduction: Optional[str] = "mean", norm: int = 2, single_directional=False, abs_cosine: bool = True,
                     fused: Optional[bool] = None):
    """Chamfer distance between the padded clouds ``x [N, P1, D]`` and ``y [N, P2, D]``.

    ``*_lengths [N]``: points per cloud; ``*_normals [N, P, D]``: adds ``1 - |cos|`` (``1 - cos`` with ``abs_cosine=False``) to the
    nearest point's normal; ``*_features [N, P, C]``: adds the mean squared difference to the nearest point's features (second
    direction only); ``*_weights [N, P]``: see the module text.  ``point_reduction`` / ``batch_reduction``: "mean", "sum" or None
    (per-point values ``[N, P1]`` / ``[N, P2]``).  ``norm``: 1 or 2.  ``fused``: None (HIP where it applies), True or False.

    Returns four pairs ``(x to y, y to x)``: distance, normals term, features term, weights -- a term that was not asked for is
    None, and with ``single_directional`` the second slot of every pair is None."""
    _check_reductions(batch_reduction, point_reduction)
    if not (norm == 1 or norm == 2):
        raise ValueError("Support for 1 or 2 norm.")
    x, x_lengths, x_normals = _cloud(x, x_lengths, x_normals)
    y, y_lengths, y_normals = _cloud(y, y_lengths, y_normals)

    cham_x, norm_x, feat_x, weight_x = _one_direction(x, y, x_lengths, y_lengths, x_normals, y_normals, None, None, x_weights,
                                                      y_weights, batch_reduction, point_reduction, norm, abs_cosine, fused=fused)
    if single_directional:
        return (cham_x, None), (norm_x, None), (feat_x, None), (weight_x, None)
    cham_y, norm_y, feat_y, weight_y = _one_direction(y, x, y_lengths, x_lengths, y_normals, x_normals, y_features, x_features,
                                                      y_weights, x_weights, batch_reduction, point_reduction, norm, abs_cosine,
                                                      fused=fused)
    return (cham_x, cham_y), (norm_x, norm_y), (feat_x, feat_y), (weight_x, weight_y)
