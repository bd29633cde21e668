"""The steps the reference's ``run.sh`` takes BETWEEN its training stages, on this package's own models:

* ``hair_sphere`` / ``crop_to_sphere`` / ``write_scale_pickle``  -- src/preprocessing/scale_scene_into_sphere.py:38-70: find the
  sphere of the hair Gaussians, crop the stage-1 model to it, write ``scale.pickle`` (both strand models read their segment
  width from it);
* ``filter_head_intersections``  -- src/preprocessing/filter_flame_intersections.py:88,109-120: drop the hair Gaussians whose
  3-sigma probe touches the inside of the head mesh;
* ``prune_strands`` / ``export_strands``  -- src/preprocessing/export_strands.py:58-79: drop the strands of which less than half
  the points lie outside the head mesh, write ``<name>_strands.pkl`` and ``<name>_strands.ply``.

All three are restated, none uses a learned model; the only arithmetic of substance is ``mesh.HeadMesh`` (HIP).
"""
from __future__ import annotations

import os
import pickle

import numpy as np
import torch
from torch import nn

from .mesh import HeadMesh
from .scene import ply_io

_ROW_TENSORS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_label", "_scaling", "_rotation", "_orient_conf")


def _keep_rows(model, keep: torch.Tensor) -> None:
    """Keep the rows where ``keep`` is True.  A model that owns an optimizer goes through its own row surgery
    (``prune_points``: the parameters and the Adam moments are re-laid together); a bare model is indexed."""
    if model.optimizer is not None:
        model.prune_points(~keep)
        return
    P = model.get_xyz.shape[0]
    for name in _ROW_TENSORS:
        t = getattr(model, name)
        if t.shape[0] == P:
            setattr(model, name, nn.Parameter(t.detach()[keep].contiguous().requires_grad_(t.requires_grad)))
    for name in ("max_radii2D", "xyz_gradient_accum", "denom"):
        t = getattr(model, name)
        if t.dim() and t.shape[0] == P:
            setattr(model, name, t[keep])


@torch.no_grad()
def hair_sphere(model):
    """(translation [3], scale []) of the hair: the Gaussians with label >= 0.5 and opacity >= 0.5, then five rounds of: the
    norms about the current centre, threshold = 5 x their (lower) median, keep the strictly nearer, centre = their mean,
    scale = their largest norm."""
    hair = torch.logical_and((model.get_label >= 0.5)[:, 0], (model.get_opacity >= 0.5)[:, 0])
    xyz = model.get_xyz.detach()[hair]
    if xyz.shape[0] == 0:
        raise ValueError("hair_sphere: no Gaussian has label >= 0.5 and opacity >= 0.5")
    tr = torch.zeros(3, device=xyz.device, dtype=xyz.dtype)
    s = None
    for _ in range(5):
        norm = torch.linalg.norm(xyz - tr, dim=-1)
        threshold = torch.median(norm, dim=0).values * 5
        near = norm < threshold
        xyz = xyz[near]
        tr = xyz.mean(dim=0)
        s = norm[near].max()
    return tr, s


@torch.no_grad()
def crop_to_sphere(model, translation, scale) -> torch.Tensor:
    """Drops the Gaussians at ``scale`` or farther from ``translation`` (strict <, as the script); returns the keep mask."""
    tr = torch.as_tensor(translation, dtype=model.get_xyz.dtype, device=model.get_xyz.device)
    keep = torch.linalg.norm(model.get_xyz.detach() - tr, dim=-1) < scale
    _keep_rows(model, keep)
    return keep


def write_scale_pickle(path: str, translation, scale) -> dict:
    """``scale.pickle`` as the script writes it: {'scale': float, 'translation': [float, float, float]}."""
    d = {"scale": float(scale), "translation": [float(x) for x in translation]}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        pickle.dump(d, f)
    return d


@torch.no_grad()
def filter_head_intersections(model, mesh: HeadMesh, probe: str = "reference", fused: bool = True) -> torch.Tensor:
    """Keeps a Gaussian iff all twelve of its probes are outside ``mesh`` or its label is <= 0.5; returns the keep mask.
    ``probe``: see ``HeadMesh.probe_points`` (the default gives the script's points).  ``fused=False``: the composed form."""
    outside = mesh.probes_outside(model.get_xyz, model.get_scaling, model._rotation, probe=probe, fused=fused)
    keep = torch.logical_or(outside, model.get_label.detach().reshape(-1) <= 0.5)
    _keep_rows(model, keep)
    return keep


@torch.no_grad()
def prune_strands(points, mesh: HeadMesh, fused: bool = True):
    """points [S, L, 3] -> (points[keep], keep [S]): a strand stays iff 2 x (its points outside the mesh) >= L -- the exact
    integer form of ``(sdf < 0).mean(axis=1) >= 0.5``."""
    assert points.dim() == 3 and points.shape[-1] == 3, points.shape
    L = points.shape[1]
    outside = ~mesh.contains(points, fused=fused)
    keep = 2 * outside.sum(dim=1) >= L
    return points[keep], keep


def export_strands(points, directory: str, name) -> tuple:
    """Writes ``<name>_strands.pkl`` (the [S, L, 3] float32 array, pickled) and ``<name>_strands.ply`` (one vertex per point:
    x y z nx ny nz float32, zero normals) into ``directory``; returns the two paths."""
    p = points.detach().cpu().numpy() if isinstance(points, torch.Tensor) else np.asarray(points)
    p = np.ascontiguousarray(p, np.float32)
    os.makedirs(directory, exist_ok=True)
    pkl, ply = os.path.join(directory, "%s_strands.pkl" % name), os.path.join(directory, "%s_strands.ply" % name)
    with open(pkl, "wb") as f:
        pickle.dump(p, f)
    xyz = p.reshape(-1, 3)
    ply_io.write_ply_vertices(ply, ["x", "y", "z", "nx", "ny", "nz"], np.concatenate([xyz, np.zeros_like(xyz)], axis=1))
    return pkl, ply
