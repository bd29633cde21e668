"""The orientation maps without a GPU: the host-side bank and taps, the `__host__ __device__` functions of csrc/ghr_orient.h on
the CPU through tests/hostsim/ghr_hostsim_orient.cpp, the PyTorch-composed comparator of gaussianhaircut_amd.orientation
(``fused=False``), the loader, the C ABI's refusals and the writer tool -- against the reference's golden
(tests/golden/make_reference_orient_golden.py).

Bars (shared with tests/test_gpu_orient.py, which runs the same cases through the C ABI on the device).
DoG plane: ``|got - ref32| <= 2^-23 |ref32| + 1e-12`` at every pixel.  A pixel is *decided* when the two largest float64
responses differ by ``m >= 1e-5`` of the larger: there ``deg`` must equal the reference's; elsewhere the returned ``k`` must
satisfy ``F64[k] >= (1 - 1e-5) F1``, F64 recomputed here in double from the golden plane and bank.  Variance, decided pixels:
``|got - var64| <= 1e-5 max(var64) + 3 |var32 - var64|``; undecided: finite and >= 0."""
import ctypes
import importlib.util
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import helpers as hp
from tests.golden import make_reference_orient_golden as mk

GOLDEN = os.path.join(hp.ROOT, "tests", "golden", "reference_orient_golden.npz")
MARGIN = 1e-5
N_CASES = 4


@pytest.fixture(scope="module")
def gold():
    G = dict(np.load(GOLDEN))
    assert int(G["n_cases"]) == N_CASES
    for i in range(N_CASES):   # the float64 responses of every case, once
        F64, k64, var64, margin = mk.restate64(G["c%d/dog32" % i], G["bank"], G["thetas"])
        assert np.array_equal(k64, G["c%d/k64" % i]) and np.allclose(var64, G["c%d/var64" % i], rtol=1e-12, atol=0)
        G["c%d/F64" % i] = F64
    return G


def case_ref(G, i):
    return dict(F64=G["c%d/F64" % i], k=G["c%d/deg" % i], var64=G["c%d/var64" % i], var32=G["c%d/var" % i], margin=G["c%d/margin" % i])


def check_plane(got, ref32, what):
    got, ref32 = np.asarray(got), np.asarray(ref32)
    assert got.dtype == np.float32 and got.shape == ref32.shape, (what, got.dtype, got.shape)
    err = np.abs(got.astype(np.float64) - ref32.astype(np.float64))
    bar = 2.0 ** -23 * np.abs(ref32.astype(np.float64)) + 1e-12
    print("%s plane: %d of %d pixels differ from the reference's float32, worst err / bar %.3g" % (what, int((got != ref32).sum()), got.size, float((err / bar).max())))
    assert (err <= bar).all(), (what, float((err / bar).max()))


def check_maps(deg, var, ref, what):
    """ref: dict(F64 [F,H,W], k, var64, var32, margin); deg integer [H,W], var float32 [H,W]"""
    deg, var = np.asarray(deg), np.asarray(var)
    F64, margin, var64 = ref["F64"], ref["margin"], ref["var64"]
    assert deg.shape == margin.shape and var.shape == margin.shape and var.dtype == np.float32, (what, deg.shape, var.shape, var.dtype)
    decided = margin >= MARGIN
    k = deg.astype(np.int64)
    assert (k >= 0).all() and (k < F64.shape[0]).all(), what
    wrong = (k != ref["k"].astype(np.int64)) & decided
    picked = np.take_along_axis(F64, k[None], axis=0)[0]
    F1 = F64.max(0)
    err = np.abs(var.astype(np.float64) - var64)
    bar = 1e-5 * var64.max() + 3.0 * np.abs(ref["var32"].astype(np.float64) - var64)
    print("%s: undecided %.2f %%, wrong decided picks %d, variance worst err / bar %.3g (decided)"
          % (what, 100 * (1 - decided.mean()), int(wrong.sum()), float((err / bar)[decided].max()) if decided.any() else 0.0))
    assert not wrong.any(), (what, int(wrong.sum()))
    assert (picked[~decided] >= (1 - MARGIN) * F1[~decided]).all(), what
    assert (err[decided] <= bar[decided]).all(), (what, float((err / bar)[decided].max()))
    assert np.isfinite(var[~decided]).all() and (var[~decided] >= 0).all(), what


def conf_numpy(var):
    """camera_utils.py:67-68 in numpy, in the float32 the loader works in: ``.float() / pi^2``, ``1 / (x^2 + 1e-7)``"""
    q = np.asarray(var).astype(np.float32) / np.float32(math.pi ** 2)
    return np.float32(1) / (q * q + np.float32(1e-7))


# ---- bank and taps ----------------------------------------------------------------------------------------------------------------

def test_gabor_bank_equals_the_references_bank(gold):
    from gaussianhaircut_amd import orientation as ori
    w, th = ori.gabor_bank()
    g = gold["bank"]
    assert w.dtype == np.float32 and w.shape == g.shape == (180, 17, 17) and th.dtype == np.float64
    assert np.array_equal(w != 0, g != 0)
    assert (np.abs(w.astype(np.float64) - g) <= np.spacing(np.abs(g))).all()
    assert np.array_equal(th, gold["thetas"])
    assert 0.62 < (w != 0).mean() < 0.64


def test_dog_taps():
    from gaussianhaircut_amd import orientation as ori
    lo, hi = ori.dog_taps(0.4), ori.dog_taps(10)
    assert lo.dtype == hi.dtype == np.float64 and len(lo) == 5 and len(hi) == 81
    assert abs(lo.sum() - 1) <= 1e-15 and abs(hi.sum() - 1) <= 1e-15
    assert np.array_equal(lo, lo[::-1]) and np.array_equal(hi, hi[::-1]) and lo.argmax() == 2 and hi.argmax() == 40


def test_a_second_bank_and_what_is_not_built():
    from gaussianhaircut_amd import orientation as ori
    w, th = ori.gabor_bank(num_filters=45, sigma_x=1.0, sigma_y=1.5)
    assert w.shape == (45, 11, 11) and w.dtype == np.float32
    assert np.array_equal(w, w[:, ::-1, ::-1])
    assert np.allclose(th, np.pi * np.arange(45) / 45, rtol=0, atol=1e-15) and th.shape == (45,)
    for kw in (dict(sigma_x=[1.0, 2.0]), dict(sigma_y=[1.0, 2.0]), dict(offset=[0.0, 1.0]), dict(frequency=[0.23, 0.1])):
        with pytest.raises(ValueError):
            ori.gabor_bank(**kw)
        with pytest.raises(ValueError):
            ori.orientation_maps(np.zeros((4, 4, 3), np.uint8), **kw)
    p = ori.pack_bank(w)   # 45 filters: 3 tiles of 16, dealt over 4 waves; 121 taps: 31 steps of 4
    assert p.shape == (4 * 31 * 64,) and p.dtype == np.float32
    p = p.reshape(4, 31, 4, 16)
    assert p[2, 30, 0, 12] == w.reshape(45, -1)[44, 120] and not p[2, 30, 1:].any() and not p[2, :, :, 13:].any() and not p[3].any()
    assert p[1, 7, 3, 5] == w.reshape(45, -1)[21, 31]


# ---- host simulator -----------------------------------------------------------------------------------------------------------------

def _build():
    """as tests/test_hostsim_camera.py builds its file"""
    src = os.path.join(hp.ROOT, "tests", "hostsim", "ghr_hostsim_orient.cpp")
    out_dir = os.path.join(hp.ROOT, "tests", "hostsim", "_build")
    so = os.path.join(out_dir, "libghr_hostsim_orient.so")
    csrc = os.path.join(hp.ROOT, "gaussianhaircut_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(out_dir, exist_ok=True)
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-x", "hip", "-O2", "-std=c++17", "-ffp-contract=off",
                        "-fPIC", "-shared", "-o", so, src], check=True)
    return so


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def sim():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    return ctypes.CDLL(_build())


def sim_dog(sim, image):
    from gaussianhaircut_amd import orientation as ori
    image = np.ascontiguousarray(image)
    H, W = image.shape[:2]
    lo, hi = ori.dog_taps(0.4), ori.dog_taps(10)
    scratch, out = np.empty(2 * H * W, np.float64), np.full((H, W), np.nan, np.float32)
    sim.ghrsim_orient_dog(W, H, 1 if image.ndim == 2 else 3, int(image.dtype == np.uint8), _p(image), 2, _p(lo), 40, _p(hi), _p(scratch), _p(out))
    return out


def sim_gabor(sim, plane, w, th, via_half=1):
    H, W = plane.shape
    deg, var, conf = np.full((H, W), -1, np.int32), np.full((H, W), np.nan, np.float32), np.full((H, W), np.nan, np.float32)
    th32 = np.asarray(th, np.float64).astype(np.float32)
    sim.ghrsim_orient_gabor(W, H, _p(np.ascontiguousarray(plane, np.float32)), w.shape[0], w.shape[-1], _p(np.ascontiguousarray(w)), _p(th32), _p(deg),
                            _p(var), _p(conf), via_half)
    return deg, var, conf


@pytest.mark.parametrize("i", range(N_CASES))
def test_hostsim_reproduces_the_reference(sim, gold, i):
    plane = sim_dog(sim, gold["c%d/image" % i])
    check_plane(plane, gold["c%d/dog32" % i], "host-sim case %d" % i)
    deg, var, conf = sim_gabor(sim, plane, gold["bank"], gold["thetas"])
    check_maps(deg, var, case_ref(gold, i), "host-sim case %d" % i)
    exp = conf_numpy(var.astype(np.float16))
    assert (np.abs(conf - exp) <= 2 * np.spacing(exp)).all()


def test_hostsim_grey_and_float_inputs(sim, gold):
    img = gold["c2/image"]
    grey = (0.2989 * img[:, :, 0] + 0.5870 * img[:, :, 1] + 0.1140 * img[:, :, 2])
    g8 = np.ascontiguousarray(img[:, :, 1])
    ref = mk.difference_of_gaussians(g8.astype(np.float64), 0.4, 10)
    check_plane(sim_dog(sim, g8), ref.astype(np.float32), "host-sim grey uint8")
    check_plane(sim_dog(sim, g8.astype(np.float32)), ref.astype(np.float32), "host-sim grey float32")
    check_plane(sim_dog(sim, img.astype(np.float32)), gold["c2/dog32"], "host-sim rgb float32")
    assert grey.shape == g8.shape


def test_hostsim_zero_plane_gives_the_first_filter_and_zero_variance(sim, gold):
    deg, var, conf = sim_gabor(sim, np.zeros((6, 9), np.float32), gold["bank"], gold["thetas"])
    assert not deg.any() and not var.any() and np.allclose(conf, 1e7, rtol=1e-6)


# ---- comparator -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(N_CASES))
def test_comparator_reproduces_the_reference(gold, i):
    from gaussianhaircut_amd import orientation as ori
    m = ori.orientation_maps(gold["c%d/image" % i], fused=False)
    assert isinstance(m, ori.OrientationMaps) and isinstance(m.deg, np.ndarray) and m.deg.dtype == np.uint8
    check_plane(m.filtered, gold["c%d/dog32" % i], "comparator case %d" % i)
    check_maps(m.deg, m.var, case_ref(gold, i), "comparator case %d" % i)
    if i == int(gold["patch_case"]):
        t = ori.orientation_maps(torch.from_numpy(gold["c%d/image" % i]), fused=False, patch_size=32)
        assert isinstance(t.deg, torch.Tensor) and np.array_equal(t.deg.numpy(), m.deg) and np.array_equal(t.var.numpy(), m.var)
        deg, var = ori.gabor_orientation(gold["c%d/dog32" % i], fused=False)
        check_maps(deg, var, case_ref(gold, i), "comparator case %d, bank alone" % i)
    with pytest.raises(ValueError):
        ori.orientation_maps(gold["c%d/image" % i], fused=True)   # the kernels have no CPU path


# ---- loader --------------------------------------------------------------------------------------------------------------------------

def test_ground_truth_from_maps(gold):
    from gaussianhaircut_amd import orientation as ori
    deg, var = gold["c3/deg"], gold["c3/var"]
    angle, conf = ori.ground_truth_from_maps(deg, var)
    assert angle.shape == conf.shape == (1,) + deg.shape and angle.dtype == conf.dtype == np.float32
    assert np.array_equal(angle[0], (deg.astype(np.float32) / np.float32(180.0)))
    exp = conf_numpy(var.astype(np.float16))
    assert (np.abs(conf[0] - exp) <= 2 * np.spacing(exp)).all()
    _, conf_full = ori.ground_truth_from_maps(torch.from_numpy(deg), torch.from_numpy(var), via_float16=False)
    exp = conf_numpy(var)
    assert isinstance(conf_full, torch.Tensor) and (np.abs(conf_full[0].numpy() - exp) <= 2 * np.spacing(exp)).all()


def test_attach_on_cpu_cameras_fills_only_what_is_missing(gold):
    from gaussianhaircut_amd import orientation as ori
    from gaussianhaircut_amd.scene.cameras import ring_cameras
    img = gold["c1/image"]
    cams = ring_cameras(2, img.shape[1], img.shape[0])
    keep = torch.zeros(1, *img.shape[:2])
    cams[1].original_orient_angle, cams[1].original_orient_conf = keep, keep
    done = ori.attach_orientation_ground_truth(cams, [img, img])
    assert done == [cams[0]] and cams[1].original_orient_angle is keep
    a, c = ori.ground_truth_from_maps(*ori.orientation_maps(img, fused=False)[:2])
    assert np.array_equal(cams[0].original_orient_angle.numpy(), a) and np.array_equal(cams[0].original_orient_conf.numpy(), c)
    assert ori.attach_orientation_ground_truth(cams, [img, img], overwrite=True) == cams and cams[1].original_orient_angle is not keep
    with pytest.raises(ValueError):
        ori.attach_orientation_ground_truth(cams, [img[:-1], img], overwrite=True)


def test_vis_orientation_is_the_references_wheel():
    from gaussianhaircut_amd import orientation as ori
    deg = np.array([[0, 45, 90], [135, 179, 22]], np.uint8)
    v = ori.vis_orientation(deg, np.array([[1, 1, 1], [1, 1, 0.5]]))
    assert v.dtype == np.uint8 and v.shape == (2, 3, 3)
    assert v[0].tolist() == [[0, 0, 255], [255, 0, 255], [0, 255, 0]] and v[1, 0].tolist() == [255, 255, 0]
    assert v[1, 1].tolist() == [int(255 * (1 - 44 / 45.)), int(255 * (1 - 44 / 45.)), int(255 * (1 - 1 / 45.))]
    assert v[1, 2].tolist() == [int(0.5 * 255 * (22 / 45.)), 0, 127]


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------

def test_c_abi_refuses_bad_arguments_before_any_launch():
    from gaussianhaircut_amd import _lib
    L = _lib.lib()
    for name in ("ghr_orient_dog_scratch_bytes", "ghr_orient_dog", "ghr_orient_bank_floats", "ghr_orient_gabor"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert int(L.ghr_abi_version()) == _lib.ABI_VERSION
    assert L.ghr_orient_dog_scratch_bytes(7, 5) == 2 * 8 * 35 and L.ghr_orient_dog_scratch_bytes(0, 5) == 0
    assert L.ghr_orient_bank_floats(180, 17) == 12 * 73 * 64 and L.ghr_orient_bank_floats(45, 11) == 4 * 31 * 64
    assert L.ghr_orient_bank_floats(256, 25) == 16 * 157 * 64
    for bad in ((0, 17), (257, 17), (180, 16), (180, 27), (180, -1)):
        assert L.ghr_orient_bank_floats(*bad) == 0
    X = 0x1000   # stands for a buffer: a refused call touches none

    def dog(W=8, H=8, ch=3, image=X, r_low=2, w_low=X, r_high=40, w_high=X, scratch=X, out=X):
        return L.ghr_orient_dog(None, W, H, ch, 1, image, r_low, w_low, r_high, w_high, scratch, out)

    def gabor(W=8, H=8, plane=X, F=180, K=17, w=X, th=X):
        return L.ghr_orient_gabor(None, W, H, plane, F, K, w, th, X, X, None, None, 1)

    bad_calls = [lambda: dog(W=0), lambda: dog(H=0), lambda: dog(W=-3), lambda: dog(ch=2), lambda: dog(image=None), lambda: dog(w_low=None),
                 lambda: dog(w_high=None), lambda: dog(scratch=None), lambda: dog(out=None), lambda: dog(r_low=-1), lambda: dog(scratch=X + 4),
                 lambda: gabor(W=0), lambda: gabor(H=0), lambda: gabor(plane=None), lambda: gabor(w=None), lambda: gabor(th=None),
                 lambda: gabor(K=16), lambda: gabor(K=27), lambda: gabor(K=0), lambda: gabor(F=0), lambda: gabor(F=257)]
    for n, call in enumerate(bad_calls):
        assert call() == _lib.GHR_E_INVALID, n
        assert b"ghr_orient_" in L.ghr_last_error(), n


# ---- kernel resources ---------------------------------------------------------------------------------------------------------------

def test_orientation_kernels_compile_without_scratch_or_spills(tmp_path):
    """every form of the bank kernel keeps its accumulators in registers (no private segment, no spill), and the 180-filter form
    (three tiles per wave) leaves room for two waves per SIMD"""
    import re
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    src = tmp_path / "orient_only.hip"
    src.write_text('#include "%s"\n' % os.path.join(hp.ROOT, "gaussianhaircut_amd", "csrc", "ghr_orient.h") +
                   "".join("template __global__ void ghr::k_orient_gabor<%d>(ghr::OrientGaborArgs);\n" % n for n in (1, 2, 3, 4)) +
                   "".join("template __global__ void ghr::k_orient_dog<%d>(ghr::OrientDogArgs);\n" % n for n in (0, 1)))
    res = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only",
                          "-c", "-o", str(tmp_path / "o.o"), "-Rpass-analysis=kernel-resource-usage", str(src)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    blocks = re.split(r"Function Name: ", res.stderr)[1:]
    seen = {}
    for b in blocks:
        name = b.split()[0]
        get = lambda key: int(re.search(re.escape(key) + r": (\d+)", b).group(1))   # noqa: E731
        assert get("ScratchSize [bytes/lane]") == 0 and get("VGPRs Spill") == 0 and get("SGPRs Spill") == 0, b
        seen[name] = (get("VGPRs") + get("AGPRs"), get("Occupancy [waves/SIMD]"))
    assert len(seen) == 6, seen
    gabor3 = [v for k, v in seen.items() if "k_orient_gaborILi3E" in k]
    assert len(gabor3) == 1 and gabor3[0][0] <= 256 and gabor3[0][1] >= 2, seen


# ---- writer tool ----------------------------------------------------------------------------------------------------------------------

def test_writer_tool_writes_the_references_four_directories(gold, tmp_path):
    from PIL import Image
    from gaussianhaircut_amd import orientation as ori
    spec = importlib.util.spec_from_file_location("tool_orientation_maps", os.path.join(hp.ROOT, "tools", "orientation_maps.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    img_dir, mask_dir, out = tmp_path / "image", tmp_path / "mask", tmp_path / "out"
    img_dir.mkdir()
    mask_dir.mkdir()
    imgs = {"a": gold["c2/image"], "b": gold["c1/image"]}
    for name, im in imgs.items():
        Image.fromarray(im).save(img_dir / (name + ".png"))
        m = np.zeros(im.shape[:2], np.uint8)
        m[:, : im.shape[1] // 2] = 255
        Image.fromarray(m).save(mask_dir / (name + ".png"))
    assert tool.main(["--img_path", str(img_dir), "--mask_path", str(mask_dir), "--out_dir", str(out), "--torch", "--device", "cpu"]) == 2
    for name, im in imgs.items():
        m = ori.orientation_maps(im, fused=False)
        H, W = im.shape[:2]
        ang = np.asarray(Image.open(out / "angles" / (name + ".png")))
        assert ang.dtype == np.uint8 and ang.shape == (H, W) and np.array_equal(ang, m.deg)
        var = np.load(out / "vars" / (name + ".npy"))
        assert var.dtype == np.float16 and var.shape == (H, W) and np.array_equal(var, m.var.astype(np.float16))
        fil = np.asarray(Image.open(out / "filtered_imgs" / (name + ".png")))
        assert fil.dtype == np.uint8 and fil.shape == (H, W) and fil.min() == 0 and fil.max() == 255
        vis = np.asarray(Image.open(out / "vis_imgs" / (name + ".png")))
        mask = np.zeros((H, W))
        mask[:, : W // 2] = 1
        assert vis.dtype == np.uint8 and vis.shape == (H, W, 3)
        assert np.array_equal(vis, ori.vis_orientation(m.deg, mask)[:, :, ::-1])   # cv2.imwrite takes the array as B, G, R
        assert not vis[:, W // 2:].any() and vis[:, : W // 2].any()
