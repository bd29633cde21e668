"""`-m gpu`: the evaluation pass on the device -- ghr_eval_metrics / ghr_eval_products through the C ABI on the golden cases
of tests/test_eval_cpu.py (same bars), a (130, 200) image against the PyTorch-composed comparator, the two forms of
k_eval_points against each other, and evaluate_views / render_products of gaussianhaircut_amd.evaluation on the tiny scenes.

Shapes: (5, 7) is smaller than the 11 x 11 window; (23, 37) has unaligned rows (tile form of the SSIM kernel, scalar loads,
2 x 2 tiles); (48, 64) aligned rows with two strips and two segments (marching form, float4 loads, three workgroups of
k_eval_points); (130, 200) seven strips x five segments and 26 workgroups."""
import numpy as np
import pytest
import torch

from gaussianhaircut_amd.utils import synthetic as syn
from tests.golden.make_reference_eval_golden import make_inputs
from tests.test_eval_cpu import IMAGE_PRODUCTS, case, check_metrics, check_products, gold  # noqa: F401  (gold: fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ALL_PRODUCTS = IMAGE_PRODUCTS + ("orient_conf",)


def _dev(c):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in c.items()}


def _table(c, with_ssim=True):
    """one view through the C ABI -> the raw row of 8 doubles (host)"""
    from gaussianhaircut_amd import evaluation as ev
    row = torch.full((8,), float("nan"), dtype=torch.float64, device=DEV)
    ev.metrics_fused(c["packed"], c["gt_image"], c["gt_mask"], c["gt_angle"], c["gt_conf"], with_ssim, row=row)
    return row.cpu().numpy()


def _products(packed):
    from gaussianhaircut_amd import evaluation as ev
    _, H, W = packed.shape
    block = torch.full((16 * H * W,), 0xAB, dtype=torch.uint8, device=DEV)
    ev.products_fused(packed, block)
    return ev.split_product_block(block.cpu().numpy(), W, H)


@pytest.fixture(scope="module")
def big():
    """(130, 200): inputs, the comparator's metrics in float32 and float64, its float64 product values -- computed once"""
    from gaussianhaircut_amd import evaluation as ev
    c = make_inputs(130, 200, 7)
    t = {k: torch.from_numpy(v) for k, v in c.items()}
    m32 = ev.metrics_torch(t["packed"], t["gt_image"], t["gt_mask"], t["gt_angle"], t["gt_conf"]).numpy()
    d = {k: v.double() for k, v in t.items()}
    m64 = ev.metrics_torch(d["packed"], d["gt_image"], d["gt_mask"], d["gt_angle"], d["gt_conf"]).numpy()
    vals64 = {k: v.numpy() for k, v in ev.product_values_torch(d["packed"]).items()}
    return dict(c=c, m32=m32, m64=m64, vals64=vals64)


@pytest.mark.parametrize("i", range(5))
def test_metric_kernels_match_the_reference_golden(gold, i):
    from gaussianhaircut_amd import evaluation as ev
    got = ev.metrics_from_table(_table(_dev(case(gold, i))))[0]
    check_metrics(got, gold["c%d/ref64" % i], gold["c%d/ref32" % i], "gpu case %d" % i)


@pytest.mark.parametrize("i", range(3))
def test_product_kernel_matches_the_reference_golden(gold, i):
    got = _products(_dev(case(gold, i))["packed"])
    check_products(got, {k: gold["c%d/prod64/%s" % (i, k)] for k in ALL_PRODUCTS}, "gpu case %d" % i)


def test_kernels_match_the_comparator_at_130_by_200(big):
    from gaussianhaircut_amd import evaluation as ev
    c = _dev(big["c"])
    check_metrics(ev.metrics_from_table(_table(c))[0], big["m64"], big["m32"], "gpu 130x200")
    check_products(_products(c["packed"]), big["vals64"], "gpu 130x200")


def test_scalar_and_float4_forms_of_the_points_kernel_give_the_same_bits(gold, big):
    """the same values at a 16-B aligned and at a 4-B offset base: the second call takes the scalar form"""
    for c in (case(gold, 2), big["c"]):
        a = _dev(c)
        b = {}
        for k, v in a.items():
            buf = torch.empty(v.numel() + 1, dtype=torch.float32, device=DEV)
            b[k] = buf[1:].view(v.shape)
            b[k].copy_(v)
            assert a[k].data_ptr() % 16 == 0 and b[k].data_ptr() % 16 == 4
        ta, tb = _table(a, with_ssim=False), _table(b, with_ssim=False)
        assert np.array_equal(ta.view(np.uint64), tb.view(np.uint64)), (ta, tb)
        assert ta[7] == 0.0 and (ta[:2] > 0).all()
        pa, pb = _products(a["packed"]), _products(b["packed"])   # and the two forms of the product kernel
        for k in ALL_PRODUCTS:
            assert np.array_equal(pa[k], pb[k]), k


def test_two_calls_give_bit_identical_tables(big):
    c = _dev(big["c"])
    t0, t1 = _table(c), _table(c)
    assert np.array_equal(t0.view(np.uint64), t1.view(np.uint64)) and np.isfinite(t0).all()


def _tiny_scene():
    """three views of the tiny model: [0] supervised by a perturbed model, [1] the same with all-zero orientation weights,
    [2] supervised by its own render"""
    from gaussianhaircut_amd.trainer import make_ground_truth
    spec = syn.CONFIGS["tiny"]
    model = syn.make_model(spec, DEV)
    other = syn.make_model(spec, DEV)
    with torch.no_grad():
        other._xyz += 0.02 * torch.randn(other._xyz.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
        other._features_dc += 0.1
    cams = [syn.make_view(spec, DEV, n) for n in ("front", "ring5", "ring13roll")]
    bg = syn.background(DEV)
    make_ground_truth(other, cams[:2], bg)
    make_ground_truth(model, cams[2:], bg)
    cams[1].original_orient_conf = torch.zeros_like(cams[1].original_orient_conf)
    for k, cam in enumerate(cams):
        cam.image_name = "view%d" % k
    return model, cams, bg


def _comparator64(packed, cam):
    from gaussianhaircut_amd import evaluation as ev
    d = [t.double().cpu() for t in (packed, cam.original_image, cam.original_mask, cam.original_orient_angle,
                                    cam.original_orient_conf)]
    return ev.metrics_torch(*d).numpy()


def _check_views(got, ref, f64s, what):
    assert [v["name"] for v in got["views"]] == [v["name"] for v in ref["views"]]
    for k, (g, r, f64) in enumerate(zip(got["views"], ref["views"], f64s)):
        check_metrics([g[m] for m in ("l1", "ce", "or", "psnr", "ssim")], f64, [r[m] for m in ("l1", "ce", "or", "psnr", "ssim")],
                      "%s view %d" % (what, k))


def test_evaluate_views_on_the_tiny_scene():
    from gaussianhaircut_amd import evaluation as ev
    from gaussianhaircut_amd.gaussian_renderer import render
    from gaussianhaircut_amd.trainer import PIPE
    model, cams, bg = _tiny_scene()
    n0 = ev.evaluate_views.table_reads
    got = ev.evaluate_views(model, cams, bg)
    assert ev.evaluate_views.table_reads == n0 + 1   # one device-to-host transfer of the table
    ref = ev.evaluate_views(model, cams, bg, fused=False)
    with torch.no_grad():
        f64s = [_comparator64(render(cam, model, PIPE, bg).renders_packed, cam) for cam in cams]
    _check_views(got, ref, f64s, "tiny")
    v = got["views"]
    assert np.isnan(v[1]["or"]) and np.isfinite(v[0]["or"]) and v[0]["or"] > 0
    assert v[2]["psnr"] == float("inf") and abs(v[2]["ssim"] - 1.0) <= 1e-6 and v[2]["l1"] == 0.0
    assert 0 < v[0]["psnr"] < 100 and v[0]["ssim"] < 0.9999
    assert np.isnan(got["mean"]["or"]) and got["mean"]["psnr"] == float("inf")
    assert got["mean"]["l1"] == pytest.approx(np.mean([x["l1"] for x in v]), rel=1e-12)
    rep = ev.validation_report(model, cams, cams[:1], bg, with_ssim=False)
    assert set(rep) == {"test", "train"} and len(rep["train"]["views"]) == 5 and rep["test"]["views"][0]["ssim"] == 0.0
    assert [x["name"] for x in rep["train"]["views"]] == ["view2", "view1", "view0", "view2", "view1"]


def test_evaluate_views_through_render_hair():
    from gaussianhaircut_amd import evaluation as ev
    from gaussianhaircut_amd.gaussian_renderer import render_hair
    from gaussianhaircut_amd.trainer import PIPE
    from tests.test_api_cpu import _hair_scene
    spec, head, hair, cam = _hair_scene(DEV, "ring5")
    bg = syn.background(DEV)
    with torch.no_grad():
        pkg = render_hair(cam, head, hair, PIPE, bg)
        g = torch.Generator().manual_seed(5)
        cam.original_image = (pkg["render"] + 0.1 * torch.randn(pkg["render"].shape, generator=g).to(DEV)).clamp(0, 1)
        cam.original_mask = pkg["mask"].clamp(0, 1).flip(2)
        cam.original_orient_angle = pkg["orient_angle"].flip(1)
        cam.original_orient_conf = torch.rand(pkg["orient_conf"].shape, generator=g).to(DEV)
        cam.image_name = "hair0"
        f64 = _comparator64(pkg.renders_packed, cam)
    got = ev.evaluate_views(head, [cam], bg, gaussians_hair=hair)
    ref = ev.evaluate_views(head, [cam], bg, gaussians_hair=hair, fused=False)
    _check_views(got, ref, [f64], "hair")
    assert np.isfinite(list(got["mean"][m] for m in ("l1", "ce", "or", "psnr", "ssim"))).all() and got["mean"]["ce"] > 0


def test_render_products_on_the_tiny_scene():
    from gaussianhaircut_amd import evaluation as ev
    from gaussianhaircut_amd.gaussian_renderer import render
    from gaussianhaircut_amd.trainer import PIPE
    model, cams, bg = _tiny_scene()
    spec = syn.CONFIGS["tiny"]
    H, W = spec.H, spec.W
    got = list(ev.render_products(model, cams, bg))
    ref = list(ev.render_products(model, cams, bg, fused=False))
    assert len(got) == len(ref) == 3 and [g["name"] for g in got] == ["view0", "view1", "view2"]
    for k, (g, r, cam) in enumerate(zip(got, ref, cams)):
        with torch.no_grad():
            vals64 = {n: v.cpu().numpy() for n, v in ev.product_values_torch(render(cam, model, PIPE, bg).renders_packed.double()).items()}
        for n in ALL_PRODUCTS:
            assert g[n].shape == r[n].shape == ((H, W, 3) if n in ("render", "orient_vis", "orient_conf_vis") else (H, W)), n
            assert g[n].dtype == r[n].dtype == (np.float32 if n == "orient_conf" else np.uint8), n
        check_products(g, vals64, "tiny view %d" % k, share=False)
        check_products(r, vals64, "tiny view %d comparator" % k, share=False)
        assert np.abs(g["orient_conf"].astype(np.float64) - r["orient_conf"]).max() <= 1e-6
        assert g["render"].max() > 100 and g["hair_mask"].max() > 100 and g["orient_vis"].max() > 50
    assert not np.array_equal(got[0]["render"], got[2]["render"])   # the two pinned buffers did not overwrite each other
