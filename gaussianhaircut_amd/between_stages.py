"""The steps the reference's ``run.sh`` takes BETWEEN its training stages, on this package's own models:

* ``hair_sphere`` / ``crop_to_sphere`` / ``write_scale_pickle``  -- src/preprocessing/scale_scene_into_sphere.py:38-70: find the
  sphere of the hair Gaussians, crop the stage-1 model to it, write ``scale.pickle`` (both strand models read their segment
  width from it);
* ``filter_head_intersections``  -- src/preprocessing/filter_flame_intersections.py:88,109-120: drop the hair Gaussians whose
  3-sigma probe touches the inside of the head mesh;
* ``prune_strands`` / ``export_strands``  -- src/preprocessing/export_strands.py:58-79: drop the strands of which less than half
  the points lie outside the head mesh, write ``<name>_strands.pkl`` and ``<name>_strands.ply``.

* ``split_strands``  -- a definition of our own in the place of the commented-out block of src/preprocessing/export_curves.py:48-101:
  cut a strand where it enters the head mesh and re-root what follows on the scalp (``HeadMesh.closest_point``);

* ``cut_scalp`` / ``scalp_uv_mask`` / ``write_scalp_data``  -- src/preprocessing/extract_non_visible_head_scalp.py:177-229: cut
  the scalp mesh to the vertices the views do not see as bare head (``visibility.vertex_visibility``), write
  ``scalp_data/`` (stage 2's strand generator starts from it).

All are restated, none uses a learned model; the arithmetic of substance is ``mesh.HeadMesh`` and ``visibility`` (HIP).
"""
from __future__ import annotations

import os
import pickle

import numpy as np
import torch
from torch import nn

from . import visibility
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


@torch.no_grad()
def split_strands(points, head: HeadMesh, scalp: HeadMesh = None, max_root_dist: float = 0.1, fused: bool = True):
    """points [S, L, 3] -> (pieces [S', L, 3] float32, source [S'] int64: the strand every piece came from), on the points' device.

    1. a strand of which fewer than half the points are outside ``head`` is dropped (``prune_strands``' rule);
    2. every kept strand is cut into its maximal runs of consecutive outside points.  The run that holds point 0 stays rooted
       where it is.  A later run is dropped when ``scalp`` is None; otherwise the scalp's closest point to the run's first point
       (``scalp.closest_point``; every such root in ONE query) is prepended as its root when ``sqrtf(dist2) < max_root_dist``,
       and the run is dropped when it is not;
    3. pieces of fewer than 2 points are dropped;
    4. a piece of n < L points is brought back to L by replacing its first segment (p0, p1) with
       ``np.linspace(p0, p1, L - n + 2)`` (evaluated in float64, stored as float32; both ends exact), followed by ``piece[2:]``.
       (The reference's commented-out code resamples by duplicating p1; this does not.)
    Pieces are ordered by (strand, position along it).  Everything after the two queries is numpy on the host."""
    assert points.dim() == 3 and points.shape[-1] == 3, points.shape
    S, L = int(points.shape[0]), int(points.shape[1])
    outside = (~head.contains(points, fused=fused)).cpu().numpy()
    p = np.ascontiguousarray(points.detach().cpu().numpy(), np.float32)
    keep = 2 * outside.sum(axis=1) >= L
    runs = []  # (strand, first, end)
    for s in np.nonzero(keep)[0]:
        o = outside[s]
        edge = np.flatnonzero(np.diff(np.concatenate(([False], o, [False])).astype(np.int8)))
        runs += [(int(s), int(a), int(b)) for a, b in zip(edge[0::2], edge[1::2])]
    later = [i for i, (_, a, _) in enumerate(runs) if a > 0]
    roots = {}
    if scalp is not None and later:
        firsts = torch.from_numpy(np.stack([p[runs[i][0], runs[i][1]] for i in later])).to(points.device)
        d2, _, c = scalp.closest_point(firsts, fused=fused)
        d2, c = d2.cpu().numpy(), c.cpu().numpy()
        for j, i in enumerate(later):
            if np.sqrt(d2[j]) < max_root_dist:
                roots[i] = c[j]
    pieces, source = [], []
    for i, (s, a, b) in enumerate(runs):
        piece = p[s, a:b]
        if a > 0:
            if i not in roots:
                continue
            piece = np.concatenate([roots[i][None, :], piece])
        n = len(piece)
        if n < 2:
            continue
        if n < L:
            head_seg = np.linspace(piece[0].astype(np.float64), piece[1].astype(np.float64), L - n + 2).astype(np.float32)
            piece = np.concatenate([head_seg, piece[2:]])
        pieces.append(piece)
        source.append(s)
    out = np.stack(pieces).astype(np.float32) if pieces else np.zeros((0, L, 3), np.float32)
    return torch.from_numpy(out).to(points.device), torch.tensor(source, dtype=torch.int64, device=points.device)


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


def load_seam_pairs(path: str) -> list:
    """The seam groups of a scalp template from a JSON file ``{"groups": [[i, j, ...], ...]}``: scalp-vertex indices that lie on
    the same seam of the UV map and must be kept or cut together."""
    import json
    with open(path, "r") as f:
        d = json.load(f)
    return [[int(i) for i in g] for g in (d["groups"] if isinstance(d, dict) else d)]


def cut_scalp(vertex_mask, scalp_vert_idx, scalp_faces, seam_pairs=()):
    """The script's lines 177-218.  ``vertex_mask`` bool [V_head] (``visibility.visible_vertex_mask``), ``scalp_vert_idx`` [S] the
    head-mesh vertices that form the scalp, ``scalp_faces`` [F, 3] over 0 .. S - 1, ``seam_pairs`` groups of scalp indices: one
    after the other, every member of a group gets the minimum over the group.  Returns (kept [n] int64: the surviving scalp
    indices, ascending; faces [m, 3] int64: the faces whose three vertices survive, renumbered)."""
    mask = np.asarray(torch.as_tensor(vertex_mask).cpu()).astype(bool)
    idx = np.asarray(torch.as_tensor(scalp_vert_idx).cpu()).astype(np.int64).reshape(-1)
    faces = np.asarray(torch.as_tensor(scalp_faces).cpu()).astype(np.int64).reshape(-1, 3)
    m = mask[idx].copy()
    for group in seam_pairs:
        g = np.asarray(list(group), np.int64)
        m[g] = m[g].min()
    kept = np.nonzero(m)[0]
    new_id = np.full(len(idx), -1, np.int64)
    new_id[kept] = np.arange(len(kept))
    alive = m[faces].all(axis=1)
    return kept, new_id[faces[alive]]


def scalp_uv_mask(uvs, faces, size: int = 256, fused: bool = True, device=None) -> np.ndarray:
    """The script's ``create_scalp_mask``: uint8 [size, size, 1], 255 where a face of the UV map ``uvs`` [n, 2] (in [-1, 1]) covers.
    Computed by the mesh rasterizer on the affine view x' = (size - 1) / 2 (u + 1) + 0.5, likewise y', w = 1 -- the script's
    integer sample (r, c) = (size - 1) / 2 (uv + 1) is this view's pixel centre -- followed by the script's transpose and flip.
    skimage's ``polygon`` decides pixels that lie exactly on a polygon's boundary by its own rule: such pixels may differ."""
    uv = np.asarray(torch.as_tensor(uvs).cpu(), np.float32).reshape(-1, 2)
    v = np.concatenate([uv, np.zeros((len(uv), 1), np.float32)], axis=1)
    h = (size - 1) / 2.0
    M = np.array([h, 0, 0, h + 0.5, 0, h, 0, h + 0.5, 0, 0, 0, 1], np.float32)
    pix = visibility.rasterize_mesh((v, np.asarray(torch.as_tensor(faces).cpu())), M, size, size, fused=fused, device=device)
    # ours[i][j] samples (r, c) = (j, i): the script's img transposed, which is what it then forms itself before flipping
    return np.ascontiguousarray(np.flipud((pix >= 0).cpu().numpy()).astype(np.uint8) * 255)[:, :, None]


def write_scalp_data(directory: str, scalp_vertices, kept, faces, vis_planes=None, dif_mask=None) -> str:
    """``<directory>/scalp_data`` in the script's layout: ``scalp.obj`` (the kept scalp vertices and the renumbered faces),
    ``cut_scalp_verts.pickle`` (the list of kept scalp indices), ``vis/<name>.jpg`` for every entry of the dict ``vis_planes``
    (uint8 [H, W]) and ``dif_mask.png`` ([size, size, 1] or [size, size]).  Returns the path of ``scalp_data``."""
    from PIL import Image
    out = os.path.join(directory, "scalp_data")
    os.makedirs(os.path.join(out, "vis"), exist_ok=True)
    sv = np.asarray(torch.as_tensor(scalp_vertices).cpu(), np.float32).reshape(-1, 3)
    kept, faces = np.asarray(kept, np.int64), np.asarray(faces, np.int64).reshape(-1, 3)
    with open(os.path.join(out, "scalp.obj"), "w") as f:
        for p in sv[kept]:
            f.write("v %f %f %f\n" % (p[0], p[1], p[2]))
        for t in faces:
            f.write("f %d %d %d\n" % (t[0] + 1, t[1] + 1, t[2] + 1))
    with open(os.path.join(out, "cut_scalp_verts.pickle"), "wb") as f:
        pickle.dump(list(kept), f)
    for name, plane in (vis_planes or {}).items():
        p = plane.cpu().numpy() if isinstance(plane, torch.Tensor) else np.asarray(plane)
        Image.fromarray(np.ascontiguousarray(p, np.uint8)).save(os.path.join(out, "vis", "%s.jpg" % name))
    if dif_mask is not None:
        d = np.asarray(dif_mask, np.uint8)
        Image.fromarray(d[:, :, 0] if d.ndim == 3 else d).save(os.path.join(out, "dif_mask.png"))
    return out
