"""What the fused-projection tests share (tests/test_gpu_fused.py, tests/test_gpu_fused_fullsize.py,
tests/projection_cases.py, tests/test_gpu_projection_shapes.py): the two pipes, the named-pixel mask, the row criterion
and the camera whose tensors are functions of trainable leaves.  Importable without a GPU."""
from types import SimpleNamespace

import numpy as np
import torch

from gaussianhaircut_amd.utils import synthetic as syn
from tests import helpers as hp

FUSED = SimpleNamespace(debug=False, fused_projection=True)
GENERIC = SimpleNamespace(debug=False, fused_projection=False)
PARAMS = ("_xyz", "_scaling", "_rotation", "_opacity", "_label", "_orient_conf", "_features_dc", "_features_rest")
FLOOR = 2e-6  # of the tensor's largest |ref|: fp32 cancellation noise of rows whose own gradient is ~0


def _pixel_mask(state, H, W, radii_a, radii_b, means2d):
    """Pixels left out of a comparison between two chains, EXPLICITLY: the oracle's fragile pixels (a discrete decision
    -- alpha >= 1/255, T < 1e-4 -- within 2e-5 of its threshold) and a box around every Gaussian whose radius differs
    between the chains (differently rounded projection arithmetic may flip the ceil): its 3-sigma square + one tile.
    Returns (mask [H, W] bool, number of flipped Gaussians)."""
    mask = np.asarray(state.fragile).reshape(H, W).astype(bool).copy()
    flipped = np.nonzero(np.asarray(radii_a) != np.asarray(radii_b))[0]
    for i in flipped:
        r = int(max(radii_a[i], radii_b[i])) + 17
        x, y = float(means2d[i, 0]), float(means2d[i, 1])
        mask[max(0, int(y) - r):int(y) + r + 1, max(0, int(x) - r):int(x) + r + 1] = True
    return mask, int(flipped.size)


def row_unit(ref, tol=hp.TOL, floor=FLOOR):
    """The right-hand side of the row criterion for a reference tensor, [rows, -1], in the reference's own precision:
    tol (|ref| + largest |ref| of the ROW) + floor * largest |ref| of the tensor."""
    r = np.asarray(ref)
    r = r.reshape(len(r), -1)
    rows = np.abs(r).max(axis=1, keepdims=True)
    return tol * (np.abs(r) + rows) + floor * np.abs(r).max()


def _row_close(a, b, tol=hp.TOL, floor=FLOOR):
    """The row criterion, per element: |a - b| <= row_unit(b)."""
    a, b = a.reshape(len(a), -1), b.reshape(len(b), -1)
    return np.abs(a - b) <= row_unit(b, tol, floor)


def make_trainable(cam, split=False):
    """Turns a camera into one whose pose and FoV are being optimised, like the reference's (src/scene/cameras.py:83-151):
    the view matrix is a leaf, the full projection / centre are functions of it, the FoV tensors are leaves.
    ``split``: the projection reads a copy of the leaf that retains its own gradient, so that the DIRECT path (what the view
    matrix receives as the projection's input: column 3 is never read) can be told from the leaf's total (``cam.view_leaf``),
    which also collects the paths through full_proj_transform and through the inverse behind camera_center."""
    leaf = cam.world_view_transform.detach().clone().requires_grad_(True)
    cam.world_view_transform = leaf
    if split:
        cam.view_leaf = leaf
        cam.world_view_transform = leaf.clone()
        cam.world_view_transform.retain_grad()
    cam.full_proj_transform = leaf @ cam.projection_matrix
    cam.camera_center = torch.inverse(leaf)[3, :3]
    cam.FoVx = cam.FoVx.detach().clone().requires_grad_(True)
    cam.FoVy = cam.FoVy.detach().clone().requires_grad_(True)
    return cam


def _trainable_camera(spec, dev):
    return make_trainable(syn.make_view(spec, dev))
