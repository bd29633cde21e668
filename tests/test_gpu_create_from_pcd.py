"""create_from_pcd on the MI355X: against the reference's own create_from_pcd (tests/golden/reference_pcd_golden.npz), and a
COLMAP-style points3D.ply taken through fetch_ply -> create_from_pcd -> training_setup -> training_step -> save_ply /
load_ply with no stub anywhere."""
import os

import numpy as np
import pytest
import torch

from gaussianhaircut_amd.scene.gaussian_model import GaussianModel, OptimizationParams
from gaussianhaircut_amd.scene.ply_io import fetch_ply
from gaussianhaircut_amd.simple_knn import distCUDA2
from gaussianhaircut_amd.utils import synthetic as syn
from gaussianhaircut_amd.utils.graphics_utils import BasicPointCloud
from tests.test_create_from_pcd import COLMAP_DTYPE, FIELDS, GOLD, _assert_matches_gold, _write_ply

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_create_from_pcd_matches_the_reference(gold):
    pcd = BasicPointCloud(points=gold["points"], colors=gold["colors"], normals=np.zeros_like(gold["points"]))
    dist2 = distCUDA2(torch.tensor(gold["points"]).to(DEV)).cpu().numpy()
    np.testing.assert_array_equal(dist2.view(np.int32), gold["dist2"].view(np.int32))
    m = GaussianModel(3).create_from_pcd(pcd, float(gold["spatial_lr_scale"]))
    assert all(getattr(m, "_" + f).device.type == "cuda" for f in FIELDS)
    _assert_matches_gold(m, gold, ulp_fields=("scaling", "features_dc", "opacity", "label"))


def test_points3d_ply_to_training_steps_and_back(tmp_path):
    from gaussianhaircut_amd.scene.cameras import ring_cameras
    from gaussianhaircut_amd.trainer import make_ground_truth, training_step
    xyz, rgb = syn.colmap_like_cloud(200_000, 21, n_duplicates=50)
    v = np.zeros(xyz.shape[0], dtype=COLMAP_DTYPE)
    for i, n in enumerate("xyz"):
        v[n] = xyz[:, i].numpy()
    for i, n in enumerate(("red", "green", "blue")):
        v[n] = rgb[:, i].numpy()
    path = str(tmp_path / "sparse" / "0" / "points3D.ply")
    os.makedirs(os.path.dirname(path))
    _write_ply(path, v, ascii_format=False)

    pcd = fetch_ply(path)
    model = GaussianModel(3).create_from_pcd(pcd, 1.0)
    assert model._xyz.shape == (200_000, 3) and torch.isfinite(model._scaling).all()
    cams = ring_cameras(3, 256, 256, radius=0.6, device=DEV)
    bg = syn.background(DEV)
    gt = GaussianModel(3).create_from_pcd(pcd, 1.0)
    with torch.no_grad():
        gt._features_dc.add_(0.25)
    make_ground_truth(gt, cams, bg)
    opt = OptimizationParams()
    model.training_setup(opt)
    losses = [float(training_step(model, cams, bg, opt, it + 1)) for it in range(5)]
    assert all(np.isfinite(losses)), losses

    out = str(tmp_path / "point_cloud" / "iteration_5" / "point_cloud.ply")
    model.save_ply(out)
    back = GaussianModel(3)
    back.load_ply(os.path.join(os.path.dirname(out), "raw_point_cloud.ply"), device=DEV)
    for f in FIELDS:
        assert torch.equal(getattr(model, "_" + f).detach(), getattr(back, "_" + f).detach()), f
