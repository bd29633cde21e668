"""The evaluation pass without a GPU: the per-pixel functions of csrc/ghr_eval.h (eval_pixel, product_pixel -- `__host__
__device__`) on the CPU through tests/hostsim/ghr_hostsim_eval.cpp, and the PyTorch-composed comparator of
gaussianhaircut_amd.evaluation (``fused=False``), both against the reference's golden
(tests/golden/make_reference_eval_golden.py).

Bars.  Float metrics, the camera bank's: ``|got - f64| <= 1e-5 max(1, |f64|) + 3 |ref32 - f64|`` (NaN and inf must match as
such).  8-bit products: an element is *fragile* when ``255 v64 + 0.5`` lies within 0.01 of an integer (4e-5 in value); every other
element is exact, a fragile one may be off by one level; at most 3 % of a product may be fragile.  The helpers here are shared
with tests/test_gpu_eval.py, which runs the same cases through the C ABI on the device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import helpers as hp

METRICS = ("l1", "ce", "or", "psnr", "ssim")
IMAGE_PRODUCTS = ("render", "hair_mask", "head_mask", "orient", "orient_vis", "orient_conf_vis")
FRAGILE_MARGIN, FRAGILE_SHARE = 0.01, 0.03
GOLDEN = os.path.join(hp.ROOT, "tests", "golden", "reference_eval_golden.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


def case(G, i):
    """inputs of golden case i (the special cases share case 1's render)"""
    c = {k: G["c%d/%s" % (i, k)] for k in ("gt_image", "gt_mask", "gt_angle", "gt_conf")}
    c["packed"] = G["c%d/packed" % i] if "c%d/packed" % i in G else G["c1/packed"]
    return c


def check_metrics(got, f64, ref32, what, names=METRICS):
    """the camera bank's bar; returns the worst err / bar"""
    worst = 0.0
    for k, name in enumerate(METRICS):
        if name not in names:
            continue
        g, e, r = float(got[k]), float(f64[k]), float(ref32[k])
        if np.isnan(e) or np.isinf(e):
            assert (np.isnan(g) and np.isnan(e)) or g == e, (what, name, g, e)
            continue
        bar = 1e-5 * max(1.0, abs(e)) + 3.0 * abs(r - e)
        print("%s %-5s got %.12g f64 %.12g err %.3g bar %.3g" % (what, name, g, e, abs(g - e), bar))
        assert abs(g - e) <= bar, (what, name, g, e, abs(g - e), bar)
        worst = max(worst, abs(g - e) / bar)
    return worst


def expected_levels(v64):
    """CHW float64 product values -> (HWC levels as save_image quantises them, fragile mask)"""
    x = np.moveaxis(np.asarray(v64, np.float64), 0, -1) * 255 + 0.5
    return np.floor(np.clip(x, 0, 255)).astype(np.int64), np.abs(x - np.round(x)) < FRAGILE_MARGIN


def check_products(got, vals64, what, share=True):
    """got: the arrays of evaluation.products_torch / split_product_block; vals64: name -> CHW float64 values.  share: also hold
    the fragile elements to FRAGILE_SHARE of the product (the random inputs of the golden's distribution)"""
    for name in IMAGE_PRODUCTS:
        exp, fragile = expected_levels(vals64[name])
        g = got[name]
        assert g.dtype == np.uint8, (what, name, g.dtype)
        if g.ndim == 2:
            g = g[:, :, None]
        assert g.shape == exp.shape, (what, name, g.shape, exp.shape)
        frac = fragile.mean()
        d = np.abs(g.astype(np.int64) - exp)
        print("%s %-16s fragile %.2f %%, off by one at %d fragile elements" % (what, name, 100 * frac, int((d > 0).sum())))
        assert not share or frac <= FRAGILE_SHARE, (what, name, frac)
        assert (d[~fragile] == 0).all(), (what, name, int((d[~fragile] != 0).sum()))
        assert (d[fragile] <= 1).all(), (what, name, int(d.max()))
    c, e = got["orient_conf"].astype(np.float64), np.asarray(vals64["orient_conf"], np.float64)[0]
    assert got["orient_conf"].dtype == np.float32 and c.shape == e.shape
    assert (np.abs(c - e) <= 1e-6 * np.maximum(1.0, np.abs(e))).all(), (what, float(np.abs(c - e).max()))


def _build():
    """as tests/test_hostsim_camera.py builds its file"""
    src = os.path.join(hp.ROOT, "tests", "hostsim", "ghr_hostsim_eval.cpp")
    out_dir = os.path.join(hp.ROOT, "tests", "hostsim", "_build")
    so = os.path.join(out_dir, "libghr_hostsim_eval.so")
    csrc = os.path.join(hp.ROOT, "gaussianhaircut_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(out_dir, exist_ok=True)
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-x", "hip", "-O2", "-std=c++17", "-ffp-contract=off",
                        "-fPIC", "-shared", "-o", so, src], check=True)
    return so


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


class SimApi:
    """numpy in, numpy out: the two calls of include/ghr.h's evaluation pass on the CPU (no SSIM: the window is device code)"""

    def __init__(self):
        self.L = ctypes.CDLL(_build())

    def metrics(self, c):
        from gaussianhaircut_amd import evaluation as ev
        _, H, W = c["packed"].shape
        row = np.full(8, np.nan, np.float64)
        arrs = [np.ascontiguousarray(c[k], np.float32) for k in ("packed", "gt_image", "gt_mask", "gt_angle", "gt_conf")]
        self.L.ghrsim_eval_metrics(W, H, *[_p(a) for a in arrs], _p(row))
        return ev.metrics_from_table(row[None])[0]

    def products(self, packed):
        from gaussianhaircut_amd import evaluation as ev
        _, H, W = packed.shape
        block = np.full(16 * H * W, 0xAB, np.uint8)
        packed = np.ascontiguousarray(packed, np.float32)
        self.L.ghrsim_eval_products(W, H, _p(packed), _p(block), ctypes.c_void_p(block.ctypes.data + 12 * H * W))
        return ev.split_product_block(block, W, H)


@pytest.fixture(scope="module")
def sim():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    import torch  # noqa: F401  (one HIP runtime for every HIP-linked library of the process)
    return SimApi()


def test_golden_has_the_cases_and_few_fragile_elements(gold):
    n = int(gold["n_cases"])
    assert n == 5 and int(gold["n_product_cases"]) == 3
    assert [case(gold, i)["packed"].shape[1:] for i in range(3)] == [(5, 7), (23, 37), (48, 64)]
    assert np.isnan(gold["c3/ref64"][2]) and np.isnan(gold["c3/ref32"][2]) and not case(gold, 3)["gt_conf"].any()
    assert np.isinf(gold["c4/ref64"][3]) and gold["c4/ref64"][0] == 0.0
    for i in range(3):
        c = case(gold, i)
        assert c["packed"][0:3].min() < -0.1 and c["packed"][0:3].max() > 1.1 and c["packed"][3:5].min() < 0 < 1 < c["packed"][3:5].max()
        assert (c["packed"][8] > 0).all() and (c["gt_conf"] > 0).all()
        for name in IMAGE_PRODUCTS:
            _, fragile = expected_levels(gold["c%d/prod64/%s" % (i, name)])
            assert fragile.mean() <= FRAGILE_SHARE, (i, name, fragile.mean())


@pytest.mark.parametrize("i", range(5))
def test_hostsim_eval_pixel_matches_the_reference_metrics(sim, gold, i):
    got = sim.metrics(case(gold, i))
    check_metrics(got, gold["c%d/ref64" % i], gold["c%d/ref32" % i], "hostsim case %d" % i, names=("l1", "ce", "or", "psnr"))


@pytest.mark.parametrize("i", range(3))
def test_hostsim_product_pixel_matches_the_reference_products(sim, gold, i):
    got = sim.products(case(gold, i)["packed"])
    check_products(got, {k: gold["c%d/prod64/%s" % (i, k)] for k in IMAGE_PRODUCTS + ("orient_conf",)}, "hostsim case %d" % i)


@pytest.mark.parametrize("i", range(5))
def test_torch_comparator_matches_the_reference_metrics(gold, i):
    from gaussianhaircut_amd import evaluation as ev
    c = {k: torch.from_numpy(v) for k, v in case(gold, i).items()}
    got = ev.metrics_torch(c["packed"], c["gt_image"], c["gt_mask"], c["gt_angle"], c["gt_conf"]).numpy()
    check_metrics(got, gold["c%d/ref64" % i], gold["c%d/ref32" % i], "comparator case %d" % i)


@pytest.mark.parametrize("i", range(3))
def test_torch_comparator_matches_the_reference_products(gold, i):
    from gaussianhaircut_amd import evaluation as ev
    got = ev.products_torch(torch.from_numpy(case(gold, i)["packed"]))
    check_products(got, {k: gold["c%d/prod64/%s" % (i, k)] for k in IMAGE_PRODUCTS + ("orient_conf",)}, "comparator case %d" % i)
    vals = ev.product_values_torch(torch.from_numpy(case(gold, i)["packed"]).double())
    for k in IMAGE_PRODUCTS + ("orient_conf",):
        np.testing.assert_allclose(vals[k].numpy(), gold["c%d/prod64/%s" % (i, k)], rtol=0, atol=1e-12)


def test_metrics_from_table_keeps_the_reference_edge_semantics():
    from gaussianhaircut_amd import evaluation as ev
    t = np.array([[0.1, 0.2, 0.0, 0.0, 0.01, 0.01, 0.01, 0.5],      # no orientation weight
                  [0.0, 0.0, 1.0, 4.0, 0.0, 0.0, 0.0, 1.0]])         # exact match
    m = ev.metrics_from_table(t)
    assert np.isnan(m[0, 2]) and m[0, 3] == pytest.approx(20.0) and m[1, 2] == 0.25 and np.isinf(m[1, 3]) and m[1, 3] > 0
    res = ev._result(m, [None, None])
    assert np.isnan(res["mean"]["or"]) and np.isinf(res["mean"]["psnr"]) and res["mean"]["ssim"] == 0.75
    cams = ev.validation_cameras(list(range(7)), ["t0"])
    assert cams == {"test": ["t0"], "train": [5, 3, 1, 6, 4]}


def test_eval_abi_refuses_null_and_mismatched_arguments_before_any_launch():
    from gaussianhaircut_amd import _lib
    L = _lib.lib()
    fake = 0x1000   # never dereferenced: every call below is refused by the argument checks
    assert _lib.EVAL_TERMS == 8 and L.ghr_eval_scratch_floats(0, 5) == 0 and L.ghr_eval_scratch_floats(64, 48) > 0

    def args(**kw):
        a = _lib.EvalArgs()
        a.W, a.H, a.with_ssim = 64, 48, 1
        a.renders = a.gt_image = a.gt_mask = a.gt_orient_angle = a.gt_orient_conf = fake
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    bad = [(None, fake, fake), (args(), None, fake), (args(), fake, None), (args(W=0), fake, fake), (args(H=-1), fake, fake),
           (args(renders=None), fake, fake), (args(gt_image=None), fake, fake), (args(gt_mask=None), fake, fake),
           (args(gt_orient_angle=None), fake, fake), (args(gt_orient_conf=None), fake, fake), (args(), fake, fake + 4)]
    for a, scratch, row in bad:
        rc = L.ghr_eval_metrics(None, None if a is None else ctypes.byref(a), scratch, row)
        assert rc == _lib.GHR_E_INVALID and b"ghr_eval_metrics" in L.ghr_last_error(), (rc, L.ghr_last_error())
    for w, h, r, b, c in ((0, 4, fake, fake, fake), (4, 0, fake, fake, fake), (4, 4, None, fake, fake), (4, 4, fake, None, fake),
                          (4, 4, fake, fake, None)):
        assert L.ghr_eval_products(None, w, h, r, b, c) == _lib.GHR_E_INVALID and b"ghr_eval_products" in L.ghr_last_error()
    from gaussianhaircut_amd import evaluation as ev
    with pytest.raises(AssertionError, match="no CPU path"):
        ev.metrics_fused(torch.zeros(10, 4, 4), torch.zeros(3, 4, 4), torch.zeros(2, 4, 4))
    with pytest.raises(AssertionError, match="no CPU path"):
        ev.products_fused(torch.zeros(10, 4, 4))


def test_render_views_tool_writes_the_reference_layout(gold, tmp_path):
    """tools/render_views.py: seven directories, single-channel products replicated to RGB, the float plane as a [1,H,W] tensor"""
    import importlib.util
    from PIL import Image
    from gaussianhaircut_amd import evaluation as ev
    spec = importlib.util.spec_from_file_location("render_views", os.path.join(hp.ROOT, "tools", "render_views.py"))
    rv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rv)
    p = ev.products_torch(torch.from_numpy(case(gold, 1)["packed"]))
    p["name"] = "img_007.png"
    assert rv.write_products(str(tmp_path), "test", 30000, [p], scene_suffix="_x") == 1
    base = tmp_path / "test_x" / "ours_30000"
    assert sorted(d.name for d in base.iterdir()) == sorted(["renders", "hair_masks", "head_masks", "orients", "orients_vis",
                                                              "orient_confs", "orient_confs_vis"])
    hair = np.array(Image.open(base / "hair_masks" / "img_007.png"))
    assert hair.shape == (23, 37, 3) and all((hair[:, :, c] == p["hair_mask"]).all() for c in range(3))
    assert (np.array(Image.open(base / "orients_vis" / "img_007.png")) == p["orient_vis"]).all()
    conf = torch.load(base / "orient_confs" / "img_007.pth")
    assert tuple(conf.shape) == (1, 23, 37) and conf.dtype == torch.float32 and (conf[0].numpy() == p["orient_conf"]).all()
