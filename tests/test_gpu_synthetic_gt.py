"""`-m gpu`: the synthetic ground truth on the device -- ghr_gt_from_render (one launch from the packed render) against the device
composition it replaces (ghr_eval_products, then ghr_gt_assemble with the / 255 table), against the torch-composed comparator
and a float64 model, over the shapes of tests/synth_cases.py in both kernel forms; the resized route; the array form on the
reference's golden; the camera hook on the tiny scene with a strand-stage step behind it.  Neither the reference nor Pillow is
needed here.

Bars: tests/synth_cases.py.  The direct launch and the device composition run the same device functions: all seven planes bit
for bit.  Against the comparator (computed once per shape on the CPU, where torch rounds ``v * 255 + 0.5`` in two steps as the
kernels do) image, mask and confidence are bit for bit; the angle plane, whose sqrt / reciprocal / acos differ in the last places,
is held to the fragile rule against float64.  A resized confidence: ``|got - f64| <= 3 |torch32 - f64| + 9 * 2^-24 max|v|``."""
import functools

import numpy as np
import pytest
import torch

from tests import synth_cases as sc
from tests.golden import make_reference_synthetic_golden as mk
from tests.synth_cases import same_bits
from tests.test_synthetic_gt_cpu import build, check_case, gold  # noqa: F401  (gold: fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = 0xAB
MODES = ((False, False), (True, False), (False, True), (True, True))   # (white_background, binarize_masks)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(v):
    return [x.cpu().numpy() for x in v]


@functools.lru_cache(maxsize=None)
def comparator(shape, white, binarize):
    """the comparator's four tensors for a shape's case, computed once on the CPU and shared"""
    from gaussianhaircut_amd import ground_truth as gt
    packed, _ = sc.make_packed(*shape)
    return tuple(gt.ground_truth_from_render(packed, white_background=white, binarize_masks=binarize, fused=False)[:4])


def composition(packed, white, binarize, fill=None):
    """products_fused followed by the assembly with the / 255 table: two launches"""
    from gaussianhaircut_amd import ground_truth as gt
    img, hair, head, orient, conf = gt.core_products_fused(packed)
    o_img, o_mask, o_ang, _ = gt._assemble_launch(img, hair, head, orient, None, white, binarize, False, fill, 255)
    return o_img, o_mask, o_ang, conf.clone()[None]


def check_against_comparator(got, shape, white, binarize, what):
    packed, planted = sc.make_packed(*shape)
    ref = comparator(shape, white, binarize)
    img, mask, angle, conf = _np(got)
    assert same_bits(img, ref[0]), (what, "image")
    assert same_bits(mask, ref[1]), (what, "mask")
    assert same_bits(conf, ref[3]), (what, "conf")
    sc.check_angle(angle, packed, planted, what)


@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_direct_launch_equals_the_composition_and_the_comparator(shape):
    from gaussianhaircut_amd import ground_truth as gt
    packed = _dev(sc.make_packed(*shape)[0])
    for white, binarize in MODES:
        what = "gpu %dx%d white %d binarize %d" % (shape + (white, binarize))
        direct = gt.from_render_fused(packed, white, binarize, fill=SENTINEL)
        comp = composition(packed, white, binarize, fill=0x5C)
        for a, b, name in zip(direct, comp, ("image", "mask", "angle", "conf")):
            assert a.shape == b.shape and a.is_contiguous() and torch.equal(a.view(torch.int32), b.view(torch.int32)), (what, name)
        check_against_comparator(direct, shape, white, binarize, what)
        again = gt.from_render_fused(packed, white, binarize, fill=0x5C)   # another sentinel: an unwritten element would differ
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(direct, again)), what
    v = gt.ground_truth_from_render(packed)   # fused=None on a ROCm tensor: the kernel
    ref = gt.from_render_fused(packed)
    assert all(x.is_cuda and x.dtype == torch.float32 for x in v) and all(torch.equal(a, b) for a, b in zip(v[:4], ref))
    assert torch.equal(v.original_mask_hair, v.original_mask[0:1]) and torch.equal(v.original_mask_body, v.original_mask[1:2])
    H, W = shape
    assert all(torch.equal(a, b) for a, b in zip(gt.ground_truth_from_render(packed, size=(W, H)), v))


@pytest.mark.parametrize("shape", [(3, 64), (64, 64), (1, 4)], ids=lambda s: "%dx%d" % s)
def test_unaligned_and_strided_inputs_take_the_scalar_form_and_a_copy(shape):
    """H * W % 4 == 0 here, so the aligned tensor runs the float4 form; a view one float into its storage is 4-B aligned only and
    runs the scalar form: the same bits.  A non-contiguous ``packed`` is made contiguous first."""
    from gaussianhaircut_amd import ground_truth as gt
    H, W = shape
    host = sc.make_packed(*shape)[0]
    packed = _dev(host)
    assert packed.data_ptr() % 16 == 0 and (H * W) % 4 == 0
    buf = torch.empty(10 * H * W + 1, dtype=torch.float32, device=DEV)
    off = buf[1:].view(10, H, W)
    off.copy_(packed)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    wide = torch.full((10, H, 2 * W), float("nan"), dtype=torch.float32, device=DEV)
    wide[:, :, ::2] = packed
    strided = wide[:, :, ::2]
    assert not strided.is_contiguous()
    for white, binarize in ((False, False), (True, True)):
        aligned = gt.from_render_fused(packed, white, binarize, fill=SENTINEL)
        for other, what in ((gt.from_render_fused(off, white, binarize, fill=SENTINEL), "unaligned"),
                            (gt.from_render_fused(strided, white, binarize, fill=SENTINEL), "strided")):
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(aligned, other)), (what, white, binarize)
        check_against_comparator(gt.from_render_fused(off, white, binarize, fill=0x5C), shape, white, binarize, "unaligned %dx%d" % shape)


@pytest.mark.parametrize("shape,size", [((53, 37), (18, 26)), ((20, 16), (33, 41))], ids=["down", "up"])
def test_resized_route_equals_the_comparator_on_the_resized_bytes(shape, size):
    from gaussianhaircut_amd import ground_truth as gt
    w, h = size
    host = sc.make_packed(*shape)[0]
    packed = _dev(host)
    render, hair, head, orient, conf = (x.cpu().numpy() for x in gt.core_products_fused(packed))
    for white, binarize in ((False, False), (True, True)):
        got = gt.ground_truth_from_render(packed, size=size, white_background=white, binarize_masks=binarize)
        assert all(x.is_cuda and x.is_contiguous() for x in got[:4]) and tuple(got.original_image.shape) == (3, h, w)
        ref = gt.synthetic_view_ground_truth(render, head, hair, orient, conf, size=size, white_background=white, binarize_masks=binarize,
                                             fused=False)
        img, mask, angle, c = _np(got[:4])
        assert same_bits(img, ref.original_image) and same_bits(mask, ref.original_mask) and same_bits(angle, ref.original_orient_angle)
        sc.check_resized_plane(c, conf, sc.torch32_dist(conf, w, h), "gpu %dx%d -> %dx%d" % (shape + (h, w)))
        files = gt.synthetic_view_ground_truth(*(_dev(x) for x in (render, head, hair, orient, conf)), size=size, white_background=white,
                                               binarize_masks=binarize)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got[:4], files[:4]))


@pytest.mark.parametrize("i", range(len(mk.CASES)))
def test_array_form_on_the_device_equals_the_reference_camera(gold, i):
    from gaussianhaircut_amd import ground_truth as gt
    v = build(gold, i, fused=None, to=_dev)
    assert all(x.is_cuda and x.dtype == torch.float32 for x in v)
    check_case(gold, i, gt.ViewGroundTruth(*_np(v)), "gpu",
               lambda var, size: gt.resize_variance(_dev(var.astype(np.float32)), size).cpu().numpy())


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_attach_synthetic_ground_truth_on_the_tiny_scene_and_a_strand_step():
    from types import SimpleNamespace
    from gaussianhaircut_amd import evaluation as ev
    from gaussianhaircut_amd import ground_truth as gt
    from gaussianhaircut_amd.gaussian_renderer import render, render_hair
    from gaussianhaircut_amd.scene.cameras import CameraBank, ring_cameras
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    from gaussianhaircut_amd.trainer import PIPE, make_ground_truth, strand_training_step
    from gaussianhaircut_amd.utils import synthetic as syn
    from tests.test_api_cpu import _hair_scene
    names = ("original_image", "original_mask", "original_orient_angle", "original_orient_conf")
    spec = syn.CONFIGS["tiny"]
    model, bg = syn.make_model(spec, DEV), syn.background(DEV)
    cams = ring_cameras(3, spec.W, spec.H, device=DEV)
    make_ground_truth(model, cams, bg)                       # the cameras' previous ground truth
    previous = [[getattr(c, n) for n in names] for c in cams]
    fused_pipe = SimpleNamespace(debug=False, fused_projection=True)
    opt = OptimizationParams()
    opt.lambda_dorient, opt.lambda_dmask = 0.1, 0.1

    def one_step(cam):
        _, head, hair, _ = _hair_scene(DEV)
        hair.training_setup(opt, fused=True)
        return float(strand_training_step(head, hair, [cam], bg, opt, 1, pipe=fused_pipe))
    loss_before = one_step(cams[0])
    assert cams[0]._ghr_gt_stats[0] is previous[0][0]        # the SSIM moments of the previous image are cached on the camera

    assert gt.attach_synthetic_ground_truth(cams, model, bg, binarize_masks=True) == cams
    files = list(ev.render_products(model, cams, bg))
    for cam, prev, f in zip(cams, previous, files):
        with torch.no_grad():
            fresh = gt.ground_truth_from_render(render(cam, model, PIPE, bg).renders_packed, binarize_masks=True)
        route = gt.synthetic_view_ground_truth(*(_dev(f[n]) for n in ("render", "head_mask", "hair_mask", "orient", "orient_conf")),
                                               binarize_masks=True)
        for n, c, p in zip(names, (3, 2, 1, 1), prev):
            t = getattr(cam, n)
            assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (c, spec.H, spec.W) and t.is_contiguous() and not t.requires_grad
            assert t is not p and t.data_ptr() != p.data_ptr()                 # replaced, not written into
            assert _bits(t, getattr(fresh, n)) and _bits(t, getattr(route, n)), n
        assert cam.original_image.min() < cam.original_image.max() and cam.original_mask[0].min() < cam.original_mask[0].max()
        assert cam.original_mask[1].min() < cam.original_mask[1].max() and torch.isfinite(cam.original_orient_conf).all()
    loss_after = one_step(cams[0])
    assert np.isfinite(loss_after) and loss_after > 0 and loss_after != loss_before
    assert cams[0]._ghr_gt_stats[0] is cams[0].original_image                  # the cache followed the replacement

    # head + hair through render_hair, and a BankCamera
    _, head, hair, cam = _hair_scene(DEV)
    with torch.no_grad():
        hair.initialize_gaussians_hair()
        gt.attach_synthetic_ground_truth([cam], head, bg, gaussians_hair=hair, white_background=True)
        fresh = gt.ground_truth_from_render(render_hair(cam, head, hair, PIPE, bg).renders_packed, white_background=True)
    assert all(_bits(getattr(cam, n), getattr(fresh, n)) for n in names)
    bank = CameraBank(ring_cameras(2, spec.W, spec.H, device=DEV), device=DEV)
    gt.attach_synthetic_ground_truth([bank[0], bank[1]], model, bg)
    with torch.no_grad():
        fresh = gt.ground_truth_from_render(render(bank[1], model, PIPE, bg).renders_packed)
    assert all(_bits(getattr(bank[1], n), getattr(fresh, n)) for n in names)
    with pytest.raises(ValueError):
        gt.ground_truth_from_render(torch.zeros(10, 4, 4, device=DEV), size=(0, 4))
