"""gaussianhaircut_amd/between_stages.py on CPU tensors, with the PyTorch-composed containment (fused=False):
the hair sphere and the crop against a float64 restatement of src/preprocessing/scale_scene_into_sphere.py:38-70 (lower median
at an even count, a point at exactly the threshold), the head-mesh filter and the strand pruning on a sphere with Gaussians and
strands placed inside, outside and across it, and the round trips of the three files."""
import pickle

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import between_stages as bs
from gaussianhaircut_amd.mesh import HeadMesh
from gaussianhaircut_amd.scene import ply_io
from gaussianhaircut_amd.scene.gaussian_model import GaussianModel, OptimizationParams
from tests import mesh_cases as mc


def _model(xyz, label=None, opacity=None, scale=0.01, rotation=None):
    xyz = torch.as_tensor(np.asarray(xyz, np.float32))
    P = xyz.shape[0]
    logit = lambda p: torch.log(torch.as_tensor(p, dtype=torch.float32) / (1 - torch.as_tensor(p, dtype=torch.float32)))  # noqa: E731
    lab = logit(np.full(P, 0.9, np.float32) if label is None else np.asarray(label, np.float32))
    opa = logit(np.full(P, 0.9, np.float32) if opacity is None else np.asarray(opacity, np.float32))
    rot = torch.tensor([[1.0, 0, 0, 0]]).repeat(P, 1) if rotation is None else torch.as_tensor(np.asarray(rotation, np.float32))
    sc = torch.log(torch.as_tensor(np.broadcast_to(np.asarray(scale, np.float32), (P, 3)).copy()))
    feats = torch.arange(P * 16 * 3, dtype=torch.float32).reshape(P, 16, 3) * 1e-3
    return GaussianModel(3).create_from_tensors(xyz, feats, sc, rot, opa, lab)


def _sphere64(xyz, label, opacity):
    """float64 restatement of the script's loop (torch.median = the LOWER median; strict <)"""
    pts = np.asarray(xyz, np.float64)[(np.asarray(label) >= 0.5) & (np.asarray(opacity) >= 0.5)]
    tr = np.zeros(3)
    for _ in range(5):
        norm = np.linalg.norm(pts - tr, axis=-1)
        thr = np.sort(norm)[(len(norm) - 1) // 2] * 5
        near = norm < thr
        pts = pts[near]
        tr = pts.mean(0)
        s = norm[near].max()
    return tr, s


def test_hair_sphere_keeps_the_lower_median_and_the_strict_threshold():
    # eight hair points (an even count): norms 1 1 2 2 3 3 10 50 -> lower median 2, threshold 10: the point AT 10 goes, and the
    # six left are symmetric about 0 (every later round repeats the first).  The upper median (3 -> 15) would keep it.
    xyz = [[1, 0, 0], [-1, 0, 0], [0, 2, 0], [0, -2, 0], [0, 0, 3], [0, 0, -3], [10, 0, 0], [0, 50, 0],
           [0.5, 0.5, 0.5], [2.5, 0, 0], [40, 0, 0]]                     # not hair: label or opacity below 0.5
    label = [0.9] * 8 + [0.1, 0.9, 0.1]
    opacity = [0.9] * 8 + [0.9, 0.1, 0.9]
    m = _model(xyz, label, opacity)
    tr, s = bs.hair_sphere(m)
    assert tr.tolist() == [0.0, 0.0, 0.0] and float(s) == 3.0
    tr64, s64 = _sphere64(xyz, label, opacity)
    assert np.array_equal(tr64, np.zeros(3)) and s64 == 3.0
    keep = bs.crop_to_sphere(m, tr, s)
    # strict <: the hair points AT the scale go too; the non-hair Gaussians inside the sphere stay
    assert keep.tolist() == [True, True, True, True, False, False, False, False, True, True, False]
    assert m.get_xyz.shape[0] == 6 and m._features_dc.shape == (6, 1, 3) and m._features_rest.shape == (6, 15, 3)
    assert torch.equal(m.get_xyz, torch.tensor(xyz, dtype=torch.float32)[keep])


@pytest.mark.parametrize("n", [200, 201])
def test_hair_sphere_and_crop_against_the_float64_restatement(n):
    rng = np.random.default_rng(n)
    xyz = np.concatenate([rng.normal(0.3, 0.2, (n, 3)), rng.normal(0, 8.0, (n // 4, 3))]).astype(np.float32)
    label = rng.choice([0.2, 0.5, 0.8], len(xyz)).astype(np.float32)      # 0.5 counts as hair (>=)
    opacity = rng.choice([0.3, 0.5, 0.95], len(xyz)).astype(np.float32)
    m = _model(xyz, label, opacity)
    got_label, got_opacity = m.get_label.detach()[:, 0].numpy(), m.get_opacity.detach()[:, 0].numpy()
    tr, s = bs.hair_sphere(m)
    tr64, s64 = _sphere64(xyz, got_label, got_opacity)
    # float32 norms and means of O(1) values over a few hundred points: 1e-5 is far above their rounding, far below any change
    # of the selected set (which would move the scale by the spacing of the outliers)
    assert np.abs(tr.numpy() - tr64).max() < 1e-5 and abs(float(s) - s64) < 1e-5 * s64
    want = np.linalg.norm(xyz.astype(np.float64) - tr64, axis=-1) < s64
    margin = np.abs(np.linalg.norm(xyz.astype(np.float64) - tr64, axis=-1) - s64) > 1e-4
    keep = bs.crop_to_sphere(m, tr, s)
    assert np.array_equal(keep.numpy()[margin], want[margin]) and 0 < keep.sum() < len(xyz)
    assert m.get_xyz.shape[0] == int(keep.sum())


def test_crop_with_an_optimizer_goes_through_the_models_row_surgery():
    rng = np.random.default_rng(5)
    xyz = rng.normal(0, 1.0, (60, 3)).astype(np.float32)
    m = _model(xyz)
    m.training_setup(OptimizationParams(), fused=False)
    for p in m.leaf_parameters():
        p.grad = torch.ones_like(p) * 0.5
    m.optimizer.step()
    moments = {g["name"]: m.optimizer.state[g["params"][0]]["exp_avg"].clone() for g in m.optimizer.param_groups}
    before = m.get_xyz.detach().clone()
    keep = bs.crop_to_sphere(m, [0.0, 0.0, 0.0], 1.5)
    assert 0 < keep.sum() < 60 and torch.equal(m.get_xyz.detach(), before[keep])
    for g in m.optimizer.param_groups:
        assert g["params"][0].shape[0] == int(keep.sum())
        assert torch.equal(m.optimizer.state[g["params"][0]]["exp_avg"], moments[g["name"]][keep])
    assert m.xyz_gradient_accum.shape[0] == int(keep.sum())


def test_scale_pickle_round_trip(tmp_path):
    d = bs.write_scale_pickle(str(tmp_path / "data" / "scale.pickle"), torch.tensor([0.25, -1.5, 3.0]), torch.tensor(2.75))
    back = pickle.load(open(tmp_path / "data" / "scale.pickle", "rb"))
    assert back == d == {"scale": 2.75, "translation": [0.25, -1.5, 3.0]}
    assert type(back["scale"]) is float and all(type(x) is float for x in back["translation"])


@pytest.fixture(scope="module")
def sphere():
    return HeadMesh(*mc.icosphere(2))  # radius 1 (inscribed radius about 0.97)


def test_filter_head_intersections_on_a_sphere(sphere):
    xyz = [[0, 0, 0], [0.1, 0.1, 0], [3, 0, 0], [0, -2.5, 1], [1.2, 0, 0], [1.2, 0, 0], [0, 0, 0], [0.2, 0, 0], [0, 0.5, 0]]
    scale = [[0.01] * 3, [0.05] * 3, [0.01] * 3, [0.1] * 3, [0.2] * 3, [0.01] * 3, [0.01] * 3, [0.01] * 3, [0.01] * 3]
    label = [0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.1, 0.5, 0.51]
    #        inside, inside, outside, outside, straddling, near but clear, inside head-labelled, inside at exactly 0.5, inside
    want = [False, False, True, True, False, True, True, True, False]
    rot = np.random.default_rng(1).normal(0, 2.0, (len(xyz), 4)).astype(np.float32)
    for probe in ("reference", "axis_scaled"):
        m = _model(xyz, label=label, scale=scale, rotation=rot)
        keep = bs.filter_head_intersections(m, sphere, probe=probe, fused=False)
        assert keep.tolist() == want, probe
        assert torch.equal(m.get_xyz, torch.tensor(xyz)[keep]) and m._rotation.shape == (int(sum(want)), 4)
    # an anisotropic Gaussian whose long axis, ROTATED, reaches the sphere: the two conventions part (90 degrees about z turns
    # the long x axis onto y, towards the sphere; scaled along the world axes it stays on x and misses)
    q = [[np.sqrt(0.5), 0, 0, np.sqrt(0.5)]]
    for probe, kept in (("reference", False), ("ellipsoid", False), ("axis_scaled", True)):
        m = _model([[0, 2.0, 0]], scale=[[0.5, 0.01, 0.01]], rotation=q)
        assert bs.filter_head_intersections(m, sphere, probe=probe, fused=False).tolist() == [kept], probe


def test_prune_strands_keeps_exactly_half_outside(sphere):
    inside, outside = [0.0, 0.1, 0.0], [0.0, 2.0, 0.5]
    def strand(n_out, L):  # noqa: E306
        return [outside] * n_out + [inside] * (L - n_out)
    even = torch.tensor([strand(k, 4) for k in range(5)], dtype=torch.float32)
    kept, keep = bs.prune_strands(even, sphere, fused=False)
    assert keep.tolist() == [False, False, True, True, True]           # 2 of 4 outside stays
    assert torch.equal(kept, even[2:])
    odd = torch.tensor([strand(k, 5) for k in range(6)], dtype=torch.float32)
    assert bs.prune_strands(odd, sphere, fused=False)[1].tolist() == [False, False, False, True, True, True]  # 2 of 5 goes
    q = torch.from_numpy(mc.queries("icosphere2")[:990].reshape(10, 99, 3).copy())
    v, f = mc.icosphere(2)
    out = ~mc.model_contains(v, f, q.reshape(-1, 3).numpy())[0].reshape(10, 99)
    assert bs.prune_strands(q, sphere, fused=False)[1].tolist() == (out.mean(axis=1) >= 0.5).tolist()


def test_export_strands_round_trip(tmp_path):
    p = torch.from_numpy(np.random.default_rng(2).normal(0, 1, (7, 5, 3)).astype(np.float32))
    pkl, ply = bs.export_strands(p, str(tmp_path / "strands"), 30000)
    assert pkl.endswith("30000_strands.pkl") and ply.endswith("30000_strands.ply")
    back = pickle.load(open(pkl, "rb"))
    assert isinstance(back, np.ndarray) and back.dtype == np.float32 and np.array_equal(back, p.numpy())
    names, data = ply_io.read_ply_vertices(ply)
    assert names == ["x", "y", "z", "nx", "ny", "nz"] and len(data) == 35
    assert np.array_equal(np.stack([data["x"], data["y"], data["z"]], -1), p.numpy().reshape(-1, 3))
    assert not data["nx"].any() and not data["ny"].any() and not data["nz"].any()


def test_command_line_tool_on_the_reference_layout(tmp_path, capsys):
    """tools/between_stages.py crop | filter | export with --composed, in this process, on the reference's directories."""
    import importlib.util
    import os
    from tests import helpers as hp
    spec = importlib.util.spec_from_file_location("between_stages_tool", os.path.join(hp.ROOT, "tools", "between_stages.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.default_rng(11)
    xyz = np.concatenate([rng.normal(0, 0.8, (300, 3)), rng.normal(0, 30.0, (20, 3))]).astype(np.float32)
    m = _model(xyz, scale=0.02)
    mp, data = str(tmp_path / "model"), str(tmp_path / "data")
    m.save_ply(os.path.join(mp, "point_cloud", "iteration_7", "point_cloud.ply"))
    v, f = mc.icosphere(1, 0.5)
    obj = tmp_path / "head.obj"
    obj.write_text("".join("v %r %r %r\n" % tuple(map(float, p)) for p in v) + "".join("f %d %d %d\n" % tuple(t + 1) for t in f))
    tool.main(["crop", "--model_path", mp, "--path_to_data", data, "--iter", "7", "--composed"])
    d = pickle.load(open(os.path.join(data, "scale.pickle"), "rb"))
    assert set(d) == {"scale", "translation"} and 1.0 < d["scale"] < 10.0
    cropped = GaussianModel(3)
    cropped.load_ply(os.path.join(mp, "point_cloud_cropped", "iteration_7", "raw_point_cloud.ply"))
    n_c = cropped.get_xyz.shape[0]
    assert 250 < n_c <= 300 and os.path.exists(os.path.join(mp, "point_cloud_cropped", "iteration_7", "point_cloud.ply"))
    tool.main(["filter", "--model_path", mp, "--mesh", str(obj), "--iter", "7", "--composed"])
    filtered = GaussianModel(3)
    filtered.load_ply(os.path.join(mp, "point_cloud_filtered", "iteration_7", "raw_point_cloud.ply"))
    n_f = filtered.get_xyz.shape[0]
    assert 0 < n_f < n_c and float(filtered.get_xyz.detach().norm(dim=1).min()) > 0.35    # nothing is left deep inside the head
    pts = np.cumsum(rng.normal(0, 0.1, (12, 9, 3)), axis=1).astype(np.float32)
    np.save(tmp_path / "p.npy", pts)
    tool.main(["export", "--points", str(tmp_path / "p.npy"), "--mesh", str(obj), "--out_dir", str(tmp_path / "strands"), "--iter", "7",
               "--composed"])
    back = pickle.load(open(tmp_path / "strands" / "7_strands.pkl", "rb"))
    assert back.shape[1:] == (9, 3) and 0 < back.shape[0] <= 12
    assert "Pruning %d strands" % (12 - back.shape[0]) in capsys.readouterr().out
