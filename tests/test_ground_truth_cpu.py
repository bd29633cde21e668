"""The ground-truth loader without a GPU: Pillow's coefficients and the torch-composed comparator of
gaussianhaircut_amd.ground_truth (``fused=False``), the `__host__ __device__` functions of csrc/ghr_gt.h on the CPU through
tests/hostsim/ghr_hostsim_gt.cpp, ``training_resolution``, ``view_ground_truth`` on the CPU, the C ABI's refusals, the kernels'
resources and the writer tool -- against the reference's golden (tests/golden/make_reference_loader_golden.py: the reference's
own loadCam / Camera and resize_images.py, Pillow 12.2.0).

Bars (shared with tests/test_gpu_ground_truth.py).  Everything integer and every float plane except a resized variance is
bit-identical: the arithmetic is integer, or a fixed sequence of single correctly rounded float32 operations from table values.
A resized variance: per element ``|got - f64| <= 3 |torch32 - f64| + 9 * 2^-24 * max|v|``, f64 the same blend in double from the
same float32 lambdas (``bilinear64`` of the golden's generator), torch32 F.interpolate on the CPU (its distance is in the
golden), the second term the blend's worst case: nine roundings of magnitudes <= max|v|.  No quantiles, no excluded pixels.
Measured on the CPU: the host simulator's worst distance to f64 is 1.84 * 2^-24 max|v| (case 14, the upscale), a fifth of
the bar's second term alone; the comparator's variance is torch32 itself, up to 14.9 * 2^-24 max|v| from f64 there (its source
coordinates differ from the float32 ones in the last place), 0 at the exact ``/ 2``."""
import ast
import ctypes
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import gt_cases as gc
from tests import helpers as hp
from tests.golden import make_reference_loader_golden as mk

GOLDEN = os.path.join(hp.ROOT, "tests", "golden", "reference_loader_golden.npz")


@pytest.fixture(scope="module")
def gold():
    G = dict(np.load(GOLDEN))
    assert int(G["n_cases"]) == len(mk.CASES) and str(G["pillow"]) == "12.2.0"
    return G


def case_inputs(G, i):
    """(view dict, (w, h), resolution, binarize, white) of golden case i"""
    v, r, b, wb = (int(x) for x in G["cases"][i])
    view = {n: G["view/%s/%s" % (chr(v), n)] for n in ("image", "hair", "body", "angle", "var")}
    w, h = (int(x) for x in G["%d/size" % i])
    return view, (w, h), r, bool(b), bool(wb)


def check_variance(got, G, i, what):
    """the bar of the module docstring; returns the worst distance in units of 2^-24 max|v|"""
    view, (w, h), _, _, _ = case_inputs(G, i)
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == (h, w), (what, got.dtype, got.shape)
    f64 = mk.bilinear64(view["var"], w, h)
    vmax = float(view["var"].astype(np.float64).max())
    err = np.abs(got.astype(np.float64) - f64)
    bar = 3.0 * G["%d/var_dist" % i].astype(np.float64) + 9 * 2.0 ** -24 * vmax
    print("%s case %d: resized variance worst |got - f64| = %.3g = %.2f x 2^-24 max|v|, worst err / bar %.3g"
          % (what, i, float(err.max()), float(err.max() / (2.0 ** -24 * vmax)), float((err / bar).max())))
    assert (err <= bar).all(), (what, i, float((err / bar).max()))
    return float(err.max() / (2.0 ** -24 * vmax))


def conf_numpy(var):
    """camera_utils.py:67-68 in numpy float32: ``/ pi^2``, ``1 / (x^2 + 1e-7)``"""
    q = np.asarray(var, np.float32) / np.float32(np.pi ** 2)
    return np.float32(1) / (q * q + np.float32(1e-7))


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- 1. coefficients and comparator ------------------------------------------------------------------------------------------

def test_coefficients_are_pillows_windows():
    from gaussianhaircut_amd import ground_truth as gt
    b, k = gt.resample_coefficients(37, 18)
    assert b.dtype == k.dtype == np.int32 and b.shape == (18, 2) and k.shape == (18, 11)      # // 2: 11 taps
    assert gt.resample_coefficients(53, 13)[1].shape == (13, 19) and gt.resample_coefficients(16, 33)[1].shape == (33, 5)
    assert gt.resample_coefficients(200, 25)[1].shape == (25, 33)
    for a, o in ((37, 18), (53, 13), (16, 33), (5, 1), (1, 4), (200, 25), (31, 30)):
        b, k = gt.resample_coefficients(a, o)
        assert (b[:, 0] >= 0).all() and (b[:, 1] >= 1).all() and (b[:, 0] + b[:, 1] <= a).all() and (b[:, 1] <= k.shape[1]).all()
        assert (np.abs(k.sum(1) - (1 << 22)) <= k.shape[1]).all()                                 # normalised, rounded per tap
        # a window clipped at the border loses a negative lobe and normalises a weight above 1.0 (1.09 here): what matters is
        # that the 32-bit accumulator cannot overflow
        assert (255 * np.abs(k.astype(np.int64)).sum(1) + (1 << 21) < (1 << 31)).all()
        assert not np.where(np.arange(k.shape[1])[None] >= b[:, 1:2], k, 0).any()
    b, k = gt.resample_coefficients(5, 1)
    assert b.tolist() == [[0, 5]] and k.shape == (1, 21) and (k[0, :5] > 0).all()
    with pytest.raises(ValueError):
        gt.resample_coefficients(0, 4)


def test_comparator_reproduces_the_goldens_bytes(gold):
    from gaussianhaircut_amd import ground_truth as gt
    n = 0
    for i in range(len(mk.CASES)):
        view, (w, h), _, _, _ = case_inputs(gold, i)
        for name in ("image", "hair", "body", "angle"):
            if "%d/%s_u8" % (i, name) in gold:
                got = gt.resize_u8(view[name], (w, h), fused=False)
                assert isinstance(got, np.ndarray) and same_bits(got, gold["%d/%s_u8" % (i, name)]), (i, name)
                n += 1
    assert n >= 4 * 12
    for k in ("a", "b"):
        W, H = mk.VIEWS[k][:2]
        for f in (2, 4):
            for name in ("image", "hair", "body"):
                got = gt.resize_u8(torch.from_numpy(gold["view/%s/%s" % (k, name)]), (W // f, H // f), fused=False)
                assert isinstance(got, torch.Tensor) and same_bits(got.numpy(), gold["pyr/%s/%d/%s" % (k, f, name)]), (k, f, name)


@pytest.mark.parametrize("case", gc.SHAPES, ids=gc.case_id)
def test_comparator_equals_live_pillow_on_the_shape_table(case):
    Image = pytest.importorskip("PIL.Image")
    from gaussianhaircut_amd import ground_truth as gt
    img = gc.make_input(case)
    if gc.has_negative_weights(case):
        assert gc.saturates(case, img) == (True, True)
    ref = np.asarray(Image.fromarray(img).resize(case[2], Image.BICUBIC))
    assert same_bits(gt.resize_u8(img, case[2], fused=False), ref)
    assert same_bits(np.asarray(Image.fromarray(img).resize(case[2])), ref)   # PILtoTorch's default filter is this one


def test_what_is_not_built_raises():
    from gaussianhaircut_amd import ground_truth as gt
    ok = np.zeros((4, 5, 3), np.uint8)
    for bad, kw in ((np.zeros((4, 5, 4), np.uint8), {}), (np.zeros((4, 5, 3), np.float32), {}), (np.zeros((4, 5, 2), np.uint8), {}),
                    (ok, dict(filter="lanczos")), (np.zeros((4, 5), np.uint16), {})):
        with pytest.raises(ValueError, match="not built|must be"):
            gt.resize_u8(bad, (2, 2), fused=False, **kw)
    with pytest.raises(ValueError):
        gt.resize_u8(ok, (0, 2), fused=False)
    with pytest.raises(ValueError):
        gt.resize_u8(ok, (2, 2), fused=True)   # the kernels have no CPU path
    same = gt.resize_u8(ok, (5, 4), fused=False)
    assert same is not ok and same_bits(same, ok)


def test_module_imports_without_pillow():
    for name in ("ground_truth.py",):
        tree = ast.parse(open(os.path.join(hp.ROOT, "gaussianhaircut_amd", name)).read())
        mods = [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names] + \
               [n.module or "" for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
        assert not any(m.split(".")[0] == "PIL" for m in mods), mods


# ---- 2. host simulator -------------------------------------------------------------------------------------------------------

def _build():
    """as tests/test_orient_cpu.py builds its file"""
    src = os.path.join(hp.ROOT, "tests", "hostsim", "ghr_hostsim_gt.cpp")
    out_dir = os.path.join(hp.ROOT, "tests", "hostsim", "_build")
    so = os.path.join(out_dir, "libghr_hostsim_gt.so")
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


def sim_resize(sim, img, size):
    from gaussianhaircut_amd import ground_truth as gt
    img = np.ascontiguousarray(img)
    H, W = img.shape[:2]
    C = 1 if img.ndim == 2 else 3
    w, h = size
    out = np.full((h, w) + img.shape[2:], 0xAB, np.uint8)
    bx, cx = gt.resample_coefficients(W, w) if W != w else (None, np.zeros((1, 0), np.int32))
    by, cy = gt.resample_coefficients(H, h) if H != h else (None, np.zeros((1, 0), np.int32))
    sim.ghrsim_resample_u8(W, H, C, _p(img), w, h, _p(out), _p(bx), _p(cx) if bx is not None else None, cx.shape[1],
                           _p(by), _p(cy) if by is not None else None, cy.shape[1])
    return out


def sim_assemble(sim, image, hair, body, angle, var, white, binarize, via_half=1):
    H, W = hair.shape
    t255 = (torch.arange(256, dtype=torch.int32).to(torch.uint8) / 255.0).numpy()
    t180 = (torch.arange(256, dtype=torch.int32).to(torch.uint8) / 180.0).numpy()
    o = [np.full((c, H, W), np.nan, np.float32) for c in (3, 2, 1, 1, 1)]
    var = np.ascontiguousarray(var, np.float32)
    sim.ghrsim_gt_assemble(W, H, _p(np.ascontiguousarray(image)), _p(np.ascontiguousarray(hair)), _p(np.ascontiguousarray(body)),
                           _p(np.ascontiguousarray(angle)), _p(var), var.shape[1], var.shape[0], _p(t255), _p(t180), int(white), int(binarize),
                           via_half, *(_p(x) for x in o))
    return o


@pytest.mark.parametrize("i", range(len(mk.CASES)))
def test_hostsim_reproduces_the_reference(sim, gold, i):
    view, (w, h), _, binarize, white = case_inputs(gold, i)
    small = {}
    for name in ("image", "hair", "body", "angle"):
        small[name] = sim_resize(sim, view[name], (w, h))
        key = "%d/%s_u8" % (i, name)
        assert same_bits(small[name], gold[key] if key in gold else view[name]), (i, name)
    img, mask, angle, conf, var = sim_assemble(sim, small["image"], small["hair"], small["body"], small["angle"], view["var"], white, binarize)
    assert same_bits(img, gold["%d/image" % i]) and same_bits(mask, gold["%d/mask" % i]) and same_bits(angle, gold["%d/angle" % i]), i
    if view["var"].shape == (h, w):
        assert same_bits(conf, gold["%d/conf" % i]) and same_bits(var[0], view["var"].astype(np.float32)), i
    else:
        check_variance(var[0], gold, i, "host-sim")
        assert same_bits(conf[0], conf_numpy(var[0])), i


@pytest.mark.parametrize("case", gc.SHAPES, ids=gc.case_id)
def test_hostsim_equals_the_comparator_on_the_shape_table(sim, case):
    from gaussianhaircut_amd import ground_truth as gt
    img = gc.make_input(case)
    assert same_bits(sim_resize(sim, img, case[2]), gt.resize_u8(img, case[2], fused=False))


# ---- 3. sizes -----------------------------------------------------------------------------------------------------------------

def test_training_resolution_is_loadcams_rule(gold, capsys):
    from gaussianhaircut_amd import ground_truth as gt
    gt._WARNED = False
    for i, (k, r, _, _) in enumerate(mk.CASES):
        W, H = mk.VIEWS[k][:2]
        assert gt.training_resolution(W, H, r) == tuple(int(x) for x in gold["%d/size" % i]), (k, r)
    for (W, H, r, w, h), rs in zip(gold["sizes"].tolist(), gold["size_scales"].tolist()):
        assert gt.training_resolution(W, H, r, rs) == (w, h), (W, H, r, rs)
    assert gt.training_resolution(37, 53, 2) == (18, 26) and gt.training_resolution(37, 53, 4) == (9, 13)   # Python's rounding
    assert gt.training_resolution(1700, 2, -1) == (1600, 1) and gt.training_resolution(1600, 900, -1) == (1600, 900)
    assert capsys.readouterr().out.count("rescaling to 1.6K") == 1   # the notice comes once


# ---- 4. view_ground_truth on the CPU --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(mk.CASES)))
def test_view_ground_truth_on_the_cpu_equals_the_reference_camera(gold, i):
    from gaussianhaircut_amd import ground_truth as gt
    view, (w, h), r, binarize, white = case_inputs(gold, i)
    v = gt.view_ground_truth(view["image"], view["hair"], view["body"], view["angle"], view["var"], resolution=r,
                             white_background=white, binarize_masks=binarize, fused=False)
    assert isinstance(v, gt.ViewGroundTruth) and all(isinstance(x, np.ndarray) for x in v)
    assert same_bits(v.original_image, gold["%d/image" % i]) and same_bits(v.original_mask, gold["%d/mask" % i])
    assert same_bits(v.original_orient_angle, gold["%d/angle" % i])
    assert same_bits(v.original_mask_hair, gold["%d/mask" % i][0:1]) and same_bits(v.original_mask_body, gold["%d/mask" % i][1:2])
    if view["var"].shape == (h, w):
        assert same_bits(v.original_orient_conf, gold["%d/conf" % i])
    else:
        var = gt.resize_variance(view["var"], (w, h), fused=False)
        check_variance(var, gold, i, "comparator")
        assert same_bits(v.original_orient_conf[0], conf_numpy(var))
    t = gt.view_ground_truth(*(torch.from_numpy(view[n]) for n in ("image", "hair", "body", "angle", "var")), resolution=(w, h),
                             white_background=white, binarize_masks=binarize, fused=False)
    assert all(isinstance(x, torch.Tensor) for x in t) and all(same_bits(a.numpy(), b) for a, b in zip(t, v))


def test_attach_ground_truth_on_cpu_cameras(gold):
    from gaussianhaircut_amd import ground_truth as gt
    from gaussianhaircut_amd.scene.cameras import ring_cameras
    i = 2   # view a at -r 2
    view, (w, h), r, binarize, white = case_inputs(gold, i)
    cams = ring_cameras(2, w, h)
    views = [dict(image=view["image"], mask_hair=view["hair"], mask_body=view["body"], angle=view["angle"], var=view["var"]),
             (view["image"], view["hair"], view["body"], view["angle"], view["var"])]
    assert gt.attach_ground_truth(cams, views, resolution=r, fused=False) == cams
    for cam in cams:
        for t, key in ((cam.original_image, "image"), (cam.original_mask, "mask"), (cam.original_orient_angle, "angle")):
            assert isinstance(t, torch.Tensor) and same_bits(t.numpy(), gold["%d/%s" % (i, key)])
        assert tuple(cam.original_orient_conf.shape) == (1, h, w)
    with pytest.raises(ValueError):
        gt.attach_ground_truth(cams, views, resolution=1, fused=False)    # 37 x 53 tensors for 18 x 26 cameras
    with pytest.raises(ValueError):
        gt.attach_ground_truth(cams, views[:1], resolution=r, fused=False)


def test_frame_is_skipped_is_the_scripts_rule(gold):
    from gaussianhaircut_amd import ground_truth as gt
    a, b = ({n: gold["view/%s/%s" % (k, n)] for n in ("hair", "body", "face")} for k in ("a", "b"))
    assert [chr(c) for c in gold["pyr/skipped"]] == ["b"]
    assert not gt.frame_is_skipped(a["hair"], a["body"], a["face"])
    assert gt.frame_is_skipped(b["hair"], b["body"], gold["view/b/face_skip"])
    assert gt.frame_is_skipped(*(torch.from_numpy(x) for x in (b["hair"], b["body"], gold["view/b/face_skip"])))


# ---- 5. C ABI -----------------------------------------------------------------------------------------------------------------

def test_c_abi_refuses_bad_arguments_before_any_launch():
    """The refusals the host can decide from the arguments.  ``n > ksize`` and ``xmin + n > in`` are properties of the bounds, which
    live on the device: tests/test_gpu_ground_truth.py hands the C ABI such bounds and checks that it refuses and writes nothing."""
    from gaussianhaircut_amd import _lib
    L = _lib.lib()
    for name in ("ghr_resample_scratch_bytes", "ghr_resample_u8", "ghr_gt_assemble", "ghr_gt_resize_variance"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert int(L.ghr_abi_version()) == _lib.ABI_VERSION == 20
    assert "ghr_gt.h" in _lib.HEADERS
    assert L.ghr_resample_scratch_bytes(37, 53, 18, 26, 3) == 53 * 18 * 3 and L.ghr_resample_scratch_bytes(37, 53, 18, 26, 1) == 53 * 18
    for one_pass in ((64, 48, 64, 24, 3), (64, 48, 32, 48, 3), (8, 8, 8, 8, 1)):
        assert L.ghr_resample_scratch_bytes(*one_pass) == 0
    for bad in ((0, 5, 2, 2, 3), (5, 0, 2, 2, 3), (5, 5, 0, 2, 3), (5, 5, 2, -1, 3), (5, 5, 2, 2, 2), (5, 5, 2, 2, 4)):
        assert L.ghr_resample_scratch_bytes(*bad) == 0
    X = 0x1000   # stands for a buffer: a refused call touches none

    def resample(in_w=37, in_h=53, ch=3, src=X, out_w=18, out_h=26, dst=X + 0x100000, bx=X, cx=X, kx=11, by=X, cy=X, ky=11, scratch=X):
        return L.ghr_resample_u8(None, in_w, in_h, ch, src, out_w, out_h, dst, bx, cx, kx, by, cy, ky, scratch)

    def assemble(W=8, H=8, image=X, hair=X, body=X, angle=X, var=X, vw=8, vh=8, t255=X, t180=X, white=0, o_img=X, o_mask=X, o_ang=X, o_conf=X):
        return L.ghr_gt_assemble(None, W, H, image, hair, body, angle, var, vw, vh, t255, t180, white, 0, 1, o_img, o_mask, o_ang, o_conf)

    def variance(W=8, H=8, var=X, vw=8, vh=8, out=X):
        return L.ghr_gt_resize_variance(None, W, H, var, vw, vh, 1, out)

    bad_calls = [lambda: resample(in_w=0), lambda: resample(in_h=0), lambda: resample(out_w=0), lambda: resample(out_h=-2),
                 lambda: resample(ch=2), lambda: resample(ch=4), lambda: resample(ch=0), lambda: resample(src=None), lambda: resample(dst=None),
                 lambda: resample(bx=None), lambda: resample(cx=None), lambda: resample(by=None), lambda: resample(cy=None),
                 lambda: resample(kx=0), lambda: resample(ky=0), lambda: resample(scratch=None), lambda: resample(dst=X),
                 lambda: resample(out_w=37, by=None), lambda: resample(out_h=53, cx=None),
                 lambda: assemble(W=0), lambda: assemble(H=-1), lambda: assemble(image=None), lambda: assemble(hair=None),
                 lambda: assemble(body=None), lambda: assemble(t255=None), lambda: assemble(o_img=None), lambda: assemble(o_mask=None),
                 lambda: assemble(angle=None), lambda: assemble(o_ang=None), lambda: assemble(var=None), lambda: assemble(o_conf=None),
                 lambda: assemble(t180=None), lambda: assemble(vw=0), lambda: assemble(vh=0), lambda: assemble(white=2),
                 lambda: variance(W=0), lambda: variance(vh=0), lambda: variance(var=None), lambda: variance(out=None)]
    for n, call in enumerate(bad_calls):
        assert call() == _lib.GHR_E_INVALID, n
        assert b"ghr_resample_u8" in L.ghr_last_error() or b"ghr_gt_" in L.ghr_last_error(), n


# ---- 6. kernel resources ------------------------------------------------------------------------------------------------------

def test_ground_truth_kernels_compile_without_scratch_or_spills(tmp_path):
    """every form of the resize kernels keeps its accumulators in registers: no private segment, no spill"""
    import re
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    src = tmp_path / "gt_only.hip"
    src.write_text('#include "%s"\n' % os.path.join(hp.ROOT, "gaussianhaircut_amd", "csrc", "ghr_gt.h") +
                   "".join("template __global__ void ghr::k_resample_u8_h<%d>(ghr::ResampleArgs);\n" % n for n in (1, 3)) +
                   "".join("template __global__ void ghr::k_resample_u8_h_lds<%d>(ghr::ResampleArgs);\n" % n for n in (1, 3)) +
                   "".join("template __global__ void ghr::k_resample_u8_v<%s>(ghr::ResampleArgs);\n" % n for n in ("true", "false")))
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
    assert len(seen) == 8 and sum("k_resample_u8" in k for k in seen) == 6, seen
    assert sum("k_gt_assemble" in k for k in seen) == 1 and sum("k_gt_resize_var" in k for k in seen) == 1, seen
    assert all(occ >= 4 for _, occ in seen.values()), seen   # streaming kernels: nothing here needs more than 128 registers


# ---- 7. writer tool -----------------------------------------------------------------------------------------------------------

def test_writer_tool_writes_the_six_folders_with_the_goldens_bytes(gold, tmp_path, capsys):
    import pickle
    from PIL import Image
    spec = importlib.util.spec_from_file_location("tool_resize_images", os.path.join(hp.ROOT, "tools", "resize_images.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    data = tmp_path / "data"
    for sub in ("images", "masks/hair", "masks/body", "masks/face"):
        (data / sub).mkdir(parents=True)
    for k, face in (("a", gold["view/a/face"]), ("b", gold["view/b/face_skip"])):
        Image.fromarray(gold["view/%s/image" % k]).save(data / "images" / (k + ".png"))
        Image.fromarray(gold["view/%s/hair" % k]).save(data / "masks/hair" / (k + ".png"))
        Image.fromarray(gold["view/%s/body" % k]).save(data / "masks/body" / (k + ".png"))
        Image.fromarray(face).save(data / "masks/face" / (k + ".png"))
    assert tool.main(["--data_path", str(data), "--fused", "0", "--device", "cpu"]) == 1
    assert "Skipping frame b.png" in capsys.readouterr().out
    for f in (2, 4):
        for sub, name in (("images_%d" % f, "image"), ("masks_%d/hair" % f, "hair"), ("masks_%d/body" % f, "body")):
            assert sorted(os.listdir(data / sub)) == ["a.png"], sub
            assert same_bits(np.asarray(Image.open(data / sub / "a.png")), gold["pyr/a/%d/%s" % (f, name)]), (f, name)
    # without the face mask nothing is skipped, and the list of names is honoured
    os.remove(data / "masks/face/b.png")
    with open(data / "iqa_filtered_names.pkl", "wb") as fh:
        pickle.dump(["b.png"], fh)
    os.remove(data / "images_2/a.png")
    assert tool.main(["--data_path", str(data), "--fused", "0", "--device", "cpu"]) == 1
    assert not os.path.exists(data / "images_2/a.png")
    for f in (2, 4):
        for sub, name in (("images_%d" % f, "image"), ("masks_%d/hair" % f, "hair"), ("masks_%d/body" % f, "body")):
            assert same_bits(np.asarray(Image.open(data / sub / "b.png")), gold["pyr/b/%d/%s" % (f, name)]), (f, name)
