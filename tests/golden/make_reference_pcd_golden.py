"""Generates tests/golden/reference_pcd_golden.npz by running THE REFERENCE'S OWN ``GaussianModel.create_from_pcd``
(src/scene/gaussian_model.py:399-424, imported read-only from /root/reference/src) on a seeded COLMAP-like cloud.  Run once
in the build container (the GPU box only reads the committed .npz):

    python tests/golden/make_reference_pcd_golden.py

The reference module imports ``plyfile`` and ``simple_knn`` and hard-codes device="cuda": ``plyfile`` is stubbed, the "cuda"
tensor factories are redirected to the CPU (make_reference_golden.py), and ``distCUDA2`` is a numpy float32 brute force
of the contract (gaussianhaircut_amd/simple_knn/_C.py): every other point by index, d = (dx*dx + dy*dy) + dz*dz with
dx = neighbour - query, three FLT_MAX slots taking d only when strictly smaller, ((b0 + b1) + b2) / 3.  Saved: the
points, colours, dist2 and the eight parameter tensors the reference builds.  Nothing from the reference is copied into
the repository -- only numeric outputs.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

OUT = os.path.join(HERE, "reference_pcd_golden.npz")
P, SEED, DUPLICATES = 2500, 11, 24
FIELDS = ("xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity", "label", "orient_conf")


def dist2_numpy(points: np.ndarray) -> np.ndarray:
    """float32 brute force of the distCUDA2 contract (no FMA: numpy rounds every operation)."""
    p = np.ascontiguousarray(points, dtype=np.float32)
    n = p.shape[0]
    out = np.empty(n, dtype=np.float32)
    fmax = np.float32(np.finfo(np.float32).max)
    with np.errstate(over="ignore"):
        for i in range(n):
            dx, dy, dz = p[:, 0] - p[i, 0], p[:, 1] - p[i, 1], p[:, 2] - p[i, 2]
            d = (dx * dx + dy * dy) + dz * dz
            d[i] = np.inf
            d = np.minimum(d, fmax)
            b = np.sort(np.concatenate((d, np.full(3, fmax, np.float32))))[:3]
            out[i] = ((b[0] + b[1]) + b[2]) / np.float32(3.0)
    return out


def main():
    from make_reference_golden import REF, _load, _patch_cuda_factories
    assert os.path.isdir(REF), "run in the build container (needs /root/reference)"
    from gaussianhaircut_amd.utils import synthetic as syn  # our generator only supplies the INPUT cloud
    xyz, rgb = syn.colmap_like_cloud(P, SEED, n_duplicates=DUPLICATES)
    points = xyz.numpy()
    colors = rgb.numpy() / 255.0
    dist2 = dist2_numpy(points)

    _patch_cuda_factories()
    sys.modules["plyfile"] = types.SimpleNamespace(PlyData=None, PlyElement=None)
    knn = types.ModuleType("simple_knn")
    knn_c = types.ModuleType("simple_knn._C")
    knn_c.distCUDA2 = lambda t: torch.from_numpy(dist2_numpy(t.numpy()))
    sys.modules["simple_knn"], sys.modules["simple_knn._C"] = knn, knn_c
    sys.path.insert(0, REF)
    for m in [k for k in sys.modules if k == "utils" or k.startswith("utils.")]:
        del sys.modules[m]
    ref_graphics = __import__("utils.graphics_utils", fromlist=["BasicPointCloud"])
    ref_gm = _load("ref_gaussian_model", os.path.join(REF, "scene", "gaussian_model.py"))
    m = ref_gm.GaussianModel(3)
    m.create_from_pcd(ref_graphics.BasicPointCloud(points=points, colors=colors, normals=np.zeros_like(points)), 2.5)
    out = dict(points=points, colors=colors, dist2=dist2, spatial_lr_scale=np.float64(m.spatial_lr_scale),
               max_radii2D=m.max_radii2D.numpy())
    for f in FIELDS:
        out[f] = getattr(m, "_" + f).detach().numpy()
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
