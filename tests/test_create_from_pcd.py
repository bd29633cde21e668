"""create_from_pcd without a GPU: ``fetch_ply`` on COLMAP-layout PLY files, ``create_from_points`` against the reference's
own ``create_from_pcd`` (tests/golden/reference_pcd_golden.npz, made by tests/golden/make_reference_pcd_golden.py), the
``simple_knn`` drop-in layout, the C ABI's argument checks of the ``ghr_knn_*`` entry points and their kernels' resources.
The kNN itself: tests/test_knn_cpu.py (a host walk of the kernels) and tests/test_gpu_knn.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd.scene.gaussian_model import GaussianModel
from gaussianhaircut_amd.scene.ply_io import fetch_ply
from gaussianhaircut_amd.utils.graphics_utils import BasicPointCloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "reference_pcd_golden.npz")
REF_SRC = "/root/reference/src"
FIELDS = ("xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity", "label", "orient_conf")
# the vertex layout COLMAP's points3D.ply has (and the reference's storePly writes, src/scene/dataset_readers.py:127-131)
COLMAP_DTYPE = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                ("red", "u1"), ("green", "u1"), ("blue", "u1")]
TYPE_NAMES = {"<f4": "float", "u1": "uchar"}


def _colmap_vertices(n, seed):
    g = np.random.default_rng(seed)
    v = np.zeros(n, dtype=COLMAP_DTYPE)
    for name in ("x", "y", "z", "nx", "ny", "nz"):
        v[name] = g.standard_normal(n).astype(np.float32)
    for name in ("red", "green", "blue"):
        v[name] = g.integers(0, 256, n)
    return v


def _write_ply(path, v, ascii_format):
    header = ["ply", "format %s 1.0" % ("ascii" if ascii_format else "binary_little_endian"), "element vertex %d" % len(v)]
    header += ["property %s %s" % (TYPE_NAMES[t], n) for n, t in COLMAP_DTYPE]
    header.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        if ascii_format:
            for row in v:
                f.write((" ".join(repr(float(row[n])) if t == "<f4" else str(int(row[n])) for n, t in COLMAP_DTYPE)
                         + "\n").encode("ascii"))
        else:
            f.write(v.tobytes())


@pytest.mark.parametrize("ascii_format", [False, True])
def test_fetch_ply_reads_a_colmap_points3d_file(tmp_path, ascii_format):
    v = _colmap_vertices(37, 3)
    path = str(tmp_path / "points3D.ply")
    _write_ply(path, v, ascii_format)
    pcd = fetch_ply(path)
    assert isinstance(pcd, BasicPointCloud)
    assert pcd.points.dtype == np.float32 and pcd.normals.dtype == np.float32 and pcd.colors.dtype == np.float64
    np.testing.assert_array_equal(pcd.points, np.stack([v["x"], v["y"], v["z"]], 1))
    np.testing.assert_array_equal(pcd.normals, np.stack([v["nx"], v["ny"], v["nz"]], 1))
    np.testing.assert_array_equal(pcd.colors, np.stack([v["red"], v["green"], v["blue"]], 1) / 255.0)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _assert_matches_gold(m, gold, ulp_fields=("scaling",)):
    """``ulp_fields`` may differ by 2 ulp: log(sqrt(.)) of the scaling goes through the CPU or the GPU math library, and
    on the GPU torch also divides by a Python scalar (RGB2SH's C0) as a multiplication by its reciprocal."""
    for f in FIELDS:
        got = getattr(m, "_" + f).detach().cpu().numpy()
        ref = gold[f]
        assert got.shape == ref.shape and got.dtype == ref.dtype, f
        if f in ulp_fields:
            ulp = np.spacing(np.abs(ref).astype(np.float32))
            assert (np.abs(got - ref) <= 2 * ulp).all(), (f, np.abs(got - ref).max())
        else:
            np.testing.assert_array_equal(got, ref, err_msg=f)
    np.testing.assert_array_equal(m.max_radii2D.cpu().numpy(), gold["max_radii2D"])
    assert m.spatial_lr_scale == float(gold["spatial_lr_scale"])
    for f in FIELDS:
        assert getattr(m, "_" + f).requires_grad


def test_create_from_points_on_the_cpu_matches_the_reference_create_from_pcd(gold):
    m = GaussianModel(3).create_from_points(torch.tensor(gold["points"]), torch.tensor(gold["colors"]).float(),
                                            torch.tensor(gold["dist2"]), float(gold["spatial_lr_scale"]))
    _assert_matches_gold(m, gold)


def test_the_golden_cloud_holds_duplicates_and_outliers(gold):
    pts = gold["points"]
    _, inv, counts = np.unique(pts, axis=0, return_inverse=True, return_counts=True)
    assert (counts[inv.reshape(-1)] > 1).sum() >= 2
    assert (np.abs(pts).max(1) > 1.0).sum() >= 10
    assert np.isfinite(gold["dist2"]).all() and (gold["dist2"] > 0).all()


def _run(code, **kw):
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300, **kw)


def test_simple_knn_resolves_to_this_package_under_the_dropin_path():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from simple_knn._C import distCUDA2\n"
            "import simple_knn, gaussianhaircut_amd.simple_knn._C as ours\n"
            "assert distCUDA2.__code__.co_filename == ours.distCUDA2.__code__.co_filename, distCUDA2.__code__.co_filename\n"
            "assert simple_knn.distCUDA2 is distCUDA2\n"
            "print('ok')\n" % os.path.join(ROOT, "gaussianhaircut_amd"))
    r = _run(code)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF_SRC, "scene", "gaussian_model.py")),
                    reason="needs /root/reference (build container)")
def test_reference_gaussian_model_imports_with_only_plyfile_stubbed():
    # the reference's src ahead of gaussianhaircut_amd: its own `utils` wins, `simple_knn` is found in ours.  The reference's
    # utils/ has no __init__.py, and a namespace package loses to a regular one ANYWHERE on sys.path (gaussianhaircut_amd/
    # utils), so it is bound to its directory first -- the reference's real modules, nothing stubbed
    code = ("import sys, types, importlib.util\n"
            "sys.path[0:0] = [%r, %r]\n"
            "utils = types.ModuleType('utils'); utils.__path__ = [sys.path[0] + '/utils']; sys.modules['utils'] = utils\n"
            "sys.modules['plyfile'] = types.SimpleNamespace(PlyData=None, PlyElement=None)\n"
            "spec = importlib.util.spec_from_file_location('ref_gm', %r)\n"
            "mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)\n"
            "import utils.general_utils\n"
            "assert utils.general_utils.__file__.startswith(%r), utils.general_utils.__file__\n"
            "assert mod.distCUDA2.__module__ == 'simple_knn._C', mod.distCUDA2.__module__\n"
            "assert mod.distCUDA2.__code__.co_filename.startswith(%r), mod.distCUDA2.__code__.co_filename\n"
            "print('ok')\n" % (REF_SRC, os.path.join(ROOT, "gaussianhaircut_amd"),
                              os.path.join(REF_SRC, "scene", "gaussian_model.py"), REF_SRC,
                              os.path.join(ROOT, "gaussianhaircut_amd", "simple_knn")))
    r = _run(code)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_distcuda2_refuses_cpu_tensors():
    from gaussianhaircut_amd.simple_knn import distCUDA2
    with pytest.raises(RuntimeError, match="no CPU path"):
        distCUDA2(torch.zeros(5, 3))


def test_create_from_pcd_refuses_a_cpu_device():
    pcd = BasicPointCloud(points=np.zeros((4, 3), np.float32), colors=np.zeros((4, 3)), normals=np.zeros((4, 3), np.float32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        GaussianModel(3).create_from_pcd(pcd, 1.0, device="cpu")


def test_knn_entry_points_check_their_arguments_before_any_launch():
    L = _lib.lib()
    b = ctypes.c_size_t(0)
    assert L.ghr_knn_workspace_size(0, ctypes.byref(b)) == _lib.GHR_OK
    assert L.ghr_knn_workspace_size(4097, ctypes.byref(b)) == _lib.GHR_OK
    # sorted float4 points, then one (min, max) float4 pair per block of 64 and per superblock of 4096
    assert b.value >= 4097 * 16 + 65 * 32 + 2 * 32
    assert L.ghr_knn_workspace_size(-1, ctypes.byref(b)) == _lib.GHR_E_INVALID
    assert L.ghr_knn_workspace_size(2 ** 31, ctypes.byref(b)) == _lib.GHR_E_INVALID
    assert L.ghr_knn_workspace_size(5, None) == _lib.GHR_E_INVALID
    dummy = ctypes.c_void_p(0x1000)  # never dereferenced: every call below fails or returns before a launch
    assert L.ghr_knn_keys(None, 0, None, None, None) == _lib.GHR_OK
    assert L.ghr_knn_mean_dist2(None, 0, None, None, None, None) == _lib.GHR_OK
    assert L.ghr_knn_keys(None, 5, None, dummy, dummy) == _lib.GHR_E_INVALID
    assert L.ghr_knn_keys(None, 5, dummy, dummy, None) == _lib.GHR_E_INVALID
    assert L.ghr_knn_keys(None, 2 ** 31, dummy, dummy, dummy) == _lib.GHR_E_INVALID
    assert L.ghr_knn_mean_dist2(None, 5, dummy, None, dummy, dummy) == _lib.GHR_E_INVALID
    assert L.ghr_knn_mean_dist2(None, 5, dummy, dummy, None, dummy) == _lib.GHR_E_INVALID
    assert L.ghr_knn_mean_dist2(None, -3, dummy, dummy, dummy, dummy) == _lib.GHR_E_INVALID
    assert L.ghr_knn_mean_dist2(None, 2 ** 31, dummy, dummy, dummy, dummy) == _lib.GHR_E_INVALID
    assert b"ghr_knn_mean_dist2" in L.ghr_last_error()


def test_knn_kernels_compile_without_scratch_or_spills():
    from tests.test_kernel_resources import _descriptors
    meta = _descriptors()
    for sub in ("k_knn_keys", "k_knn_boxes", "k_knn_search"):
        ks = [v for k, v in meta.items() if sub in k]
        assert len(ks) == 1, (sub, [k for k in meta if sub in k])
        k = ks[0]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (sub, k)
        assert k["vgpr_count"] <= 64, (sub, k)  # eight waves per SIMD at the 256-thread workgroups they are declared for
    assert [v for k, v in meta.items() if "k_knn_search" in k][0]["group_segment_fixed_size"] <= 4096
    nn = [v for k, v in meta.items() if "k_nn_search" in k]   # the same walk (knn_walk) in the cross-cloud search, norm 1 and 2
    assert len(nn) == 2, [k for k in meta if "k_nn_search" in k]
    for k in nn:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
        assert k["group_segment_fixed_size"] <= 4096, k
