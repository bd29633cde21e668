"""`-m gpu`: the ground-truth loader on the device -- ghr_resample_u8 through the C ABI over the shape table of tests/gt_cases.py
(bit-identical to the comparator run on the same device tensor, to the host-side comparator that tests/test_ground_truth_cpu.py
pins to Pillow, and to the golden where it holds the case), into sentinel-filled buffers with guard bytes; the refusal of bad
device-resident bounds; ghr_gt_assemble on the golden's cases; the view and camera hooks; one training step on the attached
tensors.  Neither the reference nor Pillow is needed here.

Bars: those of tests/test_ground_truth_cpu.py.  Everything is bit-identical except a resized variance, whose bar is
``|got - f64| <= 3 |torch32 - f64| + 9 * 2^-24 * max|v|``; conf off the equal size is compared bit for bit with the conf
formula applied to the kernel's own resized variance (ghr_gt_resize_variance: the same device function), which keeps the 1e7
amplification at var ~ 0 out of the comparison.
Measured on an MI355X: the kernel's worst distance to f64 is 1.84 * 2^-24 max|v| (case 14, the upscale) -- the host simulator's
figure, bit for bit."""
import numpy as np
import pytest
import torch

from tests import gt_cases as gc
from tests.golden import make_reference_loader_golden as mk
from tests.test_ground_truth_cpu import case_inputs, check_variance, conf_numpy, gold, same_bits  # noqa: F401  (gold: fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD, SENTINEL = 64, 0xAB


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _resize_guarded(t, size):
    """ghr_resample_u8 into the middle of a sentinel-filled buffer; returns (result, guards intact)"""
    from gaussianhaircut_amd import ground_truth as gt
    w, h = size
    n = w * h * (1 if t.dim() == 2 else 3)
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    out = gt.resize_u8_fused(t, w, h, out=buf[GUARD:GUARD + n])
    intact = bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())
    return out.reshape((h, w) + tuple(t.shape[2:])), intact


@pytest.mark.parametrize("case", gc.SHAPES, ids=gc.case_id)
def test_resample_equals_the_comparator_bit_for_bit(case):
    from gaussianhaircut_amd import ground_truth as gt
    img = gc.make_input(case)
    if gc.has_negative_weights(case):
        assert gc.saturates(case, img) == (True, True)
    t = _dev(img)
    got, intact = _resize_guarded(t, case[2])
    assert intact and got.dtype == torch.uint8
    on_device = gt.resize_u8(t, case[2], fused=False)
    on_host = gt.resize_u8(img, case[2], fused=False)
    assert on_device.is_cuda and torch.equal(got, on_device) and same_bits(got.cpu().numpy(), on_host)
    again, intact = _resize_guarded(t, case[2])
    assert intact and torch.equal(got, again)
    assert torch.equal(gt.resize_u8(t, case[2]), got)   # fused=None on a ROCm tensor: the kernels


def test_resample_equals_the_golden(gold):
    from gaussianhaircut_amd import ground_truth as gt
    n = 0
    for i in range(len(mk.CASES)):
        view, (w, h), _, _, _ = case_inputs(gold, i)
        for name in ("image", "hair", "body", "angle"):
            key = "%d/%s_u8" % (i, name)
            if key in gold:
                got, intact = _resize_guarded(_dev(view[name]), (w, h))
                assert intact and same_bits(got.cpu().numpy(), gold[key]), key
                n += 1
    assert n >= 48
    img, hair, body = (_dev(gold["view/a/%s" % n]) for n in ("image", "hair", "body"))
    pyr = gt.resize_pyramid(img, hair, body)
    assert sorted(pyr) == [2, 4]
    for f, planes in pyr.items():
        for name, t in zip(("image", "hair", "body"), planes):
            assert t.is_cuda and same_bits(t.cpu().numpy(), gold["pyr/a/%d/%s" % (f, name)]), (f, name)


def test_bad_bounds_on_the_device_are_refused_and_nothing_is_written():
    """``n > ksize`` and ``xmin + n > in`` are properties of device-resident arrays: the C ABI reads them back and refuses"""
    from gaussianhaircut_amd import _lib
    from gaussianhaircut_amd import ground_truth as gt
    from gaussianhaircut_amd.diff_gaussian_rasterization import _ptr
    L = _lib.lib()
    case = ((37, 53), 1, (18, 26))
    t = _dev(gc.make_input(case))
    bx, cx = gt.resample_coefficients(37, 18)
    by, cy = gt.resample_coefficients(53, 26)
    scratch = torch.empty(53 * 18, dtype=torch.uint8, device=DEV)

    def call(bx_, by_):
        out = torch.full((26, 18), SENTINEL, dtype=torch.uint8, device=DEV)
        dbx, dcx, dby, dcy = _dev(bx_), _dev(cx), _dev(by_), _dev(cy)
        torch.cuda.synchronize()
        rc = L.ghr_resample_u8(None, 37, 53, 1, _ptr(t), 18, 26, _ptr(out), _ptr(dbx), _ptr(dcx), cx.shape[1], _ptr(dby), _ptr(dcy),
                               cy.shape[1], _ptr(scratch))
        torch.cuda.synchronize()
        return rc, out
    rc, out = call(bx, by)
    assert rc == _lib.GHR_OK and same_bits(out.cpu().numpy(), gt.resize_u8(t.cpu().numpy(), (18, 26), fused=False))
    for axis, row, pair in (("x", 3, (0, 12)), ("x", 17, (30, 8)), ("y", 0, (-1, 3)), ("y", 25, (50, 4)), ("y", 5, (2, -1))):
        b2x, b2y = bx.copy(), by.copy()
        (b2x if axis == "x" else b2y)[row] = pair
        rc, out = call(b2x, b2y)
        assert rc == _lib.GHR_E_INVALID and b"bounds_" + axis.encode() in L.ghr_last_error(), (axis, row, pair)
        assert bool((out == SENTINEL).all()), (axis, row, pair)


def test_bounds_that_do_not_ascend_take_the_direct_kernel():
    """the C ABI takes any windows that fit: mirrored ones (the staged horizontal kernel needs ascending windows, so the direct one
    runs) give what the comparator gives from the same arrays"""
    from gaussianhaircut_amd import _lib
    from gaussianhaircut_amd import ground_truth as gt
    from gaussianhaircut_amd.diff_gaussian_rasterization import _ptr
    L = _lib.lib()
    img = gc.make_input(((150, 11), 3, (70, 11)))
    t = _dev(img)
    bx, cx = gt.resample_coefficients(150, 70)
    bx, cx = np.ascontiguousarray(bx[::-1]), np.ascontiguousarray(cx[::-1])
    out = torch.full((11, 70, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    dbx, dcx = _dev(bx), _dev(cx)
    torch.cuda.synchronize()
    _lib.check(L.ghr_resample_u8(None, 150, 11, 3, _ptr(t), 70, 11, _ptr(out), _ptr(dbx), _ptr(dcx), cx.shape[1], None, None, 0, None))
    torch.cuda.synchronize()
    ref = gt.resample_axis_torch(torch.from_numpy(img), 1, bx, cx)
    assert same_bits(out.cpu().numpy(), ref.numpy())
    assert same_bits(ref.numpy(), gt.resize_u8(img, (70, 11), fused=False)[:, ::-1])


def test_resize_keeps_its_constants_while_the_shared_cache_turns_over():
    """bounds and coefficients live in the package's small per-device cache, which drops its entries when full: a resize holds its
    own until its call is made (64 new entries here, twice the cache's size)"""
    from gaussianhaircut_amd import ground_truth as gt
    img = gc.make_input(((37, 53), 1, (18, 26)))
    t = _dev(img)
    for w, h in zip(range(5, 21), range(40, 24, -1)):
        got, intact = _resize_guarded(t, (w, h))
        assert intact and same_bits(got.cpu().numpy(), gt.resize_u8(img, (w, h), fused=False)), (w, h)


def test_equal_sizes_are_a_copy():
    from gaussianhaircut_amd import ground_truth as gt
    t = _dev(gc.make_input(((37, 53), 3, (37, 53))))
    got, intact = _resize_guarded(t, (37, 53))
    assert intact and torch.equal(got, t) and got.data_ptr() != t.data_ptr()
    assert torch.equal(gt.resize_u8(t, (37, 53)), t)


@pytest.mark.parametrize("i", range(len(mk.CASES)))
def test_assemble_equals_the_reference_camera(gold, i):
    from gaussianhaircut_amd import ground_truth as gt
    view, (w, h), _, binarize, white = case_inputs(gold, i)
    small = [gt.resize_u8(_dev(view[n]), (w, h)) for n in ("image", "hair", "body", "angle")]
    var = _dev(view["var"].astype(np.float32))
    outs = gt.assemble_fused(*small, var, white_background=white, binarize_masks=binarize, fill=SENTINEL)
    img, mask, angle, conf = (x.cpu().numpy() for x in outs)
    assert same_bits(img, gold["%d/image" % i]) and same_bits(mask, gold["%d/mask" % i]) and same_bits(angle, gold["%d/angle" % i])
    if view["var"].shape == (h, w):
        assert same_bits(conf, gold["%d/conf" % i])
    else:
        rv = gt.resize_variance(var, (w, h))
        assert rv.is_cuda
        check_variance(rv.cpu().numpy(), gold, i, "gpu")
        assert same_bits(conf[0], conf_numpy(rv.cpu().numpy()))
    again = gt.assemble_fused(*small, var, white_background=white, binarize_masks=binarize, fill=0x5C)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs, again))
    # without the orientation files' pair the other two outputs are the same and nothing else is written
    img2, mask2, none_a, none_c = gt.assemble_fused(*small[:3], white_background=white, binarize_masks=binarize)
    assert none_a is None and none_c is None and torch.equal(img2, outs[0]) and torch.equal(mask2, outs[1])


@pytest.mark.parametrize("i", (0, 3, 9, 14))
def test_view_ground_truth_fused_equals_the_reference_camera(gold, i):
    from gaussianhaircut_amd import ground_truth as gt
    view, (w, h), r, binarize, white = case_inputs(gold, i)
    v = gt.view_ground_truth(*(_dev(view[n]) for n in ("image", "hair", "body", "angle", "var")), resolution=r,
                             white_background=white, binarize_masks=binarize)
    assert all(x.is_cuda and x.dtype == torch.float32 for x in v)
    assert same_bits(v.original_image.cpu().numpy(), gold["%d/image" % i]) and same_bits(v.original_mask.cpu().numpy(), gold["%d/mask" % i])
    assert same_bits(v.original_orient_angle.cpu().numpy(), gold["%d/angle" % i])
    assert torch.equal(v.original_mask_hair, v.original_mask[0:1]) and torch.equal(v.original_mask_body, v.original_mask[1:2])
    if view["var"].shape == (h, w):
        assert same_bits(v.original_orient_conf.cpu().numpy(), gold["%d/conf" % i])
    c = gt.view_ground_truth(*(_dev(view[n]) for n in ("image", "hair", "body", "angle", "var")), resolution=r,
                             white_background=white, binarize_masks=binarize, fused=False)   # the comparator on the device
    for a, b in zip(v[:3], c[:3]):
        assert torch.equal(a, b)


def test_maps_computed_from_the_image_equal_the_orientation_hook_at_equal_size(gold):
    from gaussianhaircut_amd import ground_truth as gt
    from gaussianhaircut_amd import orientation as ori
    from gaussianhaircut_amd.scene.cameras import ring_cameras
    view = {n: _dev(gold["view/a/%s" % n]) for n in ("image", "hair", "body")}
    H, W = view["image"].shape[:2]
    cams = ring_cameras(1, W, H, device=DEV)
    ori.attach_orientation_ground_truth(cams, [view["image"]])
    v = gt.view_ground_truth(view["image"], view["hair"], view["body"])
    assert torch.equal(v.original_orient_angle.view(torch.int32), cams[0].original_orient_angle.view(torch.int32))
    assert torch.equal(v.original_orient_conf.view(torch.int32), cams[0].original_orient_conf.view(torch.int32))
    half = gt.view_ground_truth(view["image"], view["hair"], view["body"], resolution=2)   # maps at the image's size, resized after
    assert tuple(half.original_orient_angle.shape) == (1, 26, 18) and torch.isfinite(half.original_orient_conf).all()
    deg, _ = ori.gabor_fused(ori.dog_fused(view["image"]))
    assert torch.equal(half.original_orient_angle[0], gt.view_ground_truth(view["image"], view["hair"], view["body"], deg, torch.zeros_like(deg).float(),
                                                                           resolution=2).original_orient_angle[0])


def test_attach_ground_truth_then_one_training_step():
    from gaussianhaircut_amd import ground_truth as gt
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    from gaussianhaircut_amd.trainer import training_step
    from gaussianhaircut_amd.utils import synthetic as syn
    spec = syn.CONFIGS["tiny"]
    model, cam, bg = syn.make_model(spec, DEV), syn.make_view(spec, DEV), syn.background(DEV)
    W, H = cam.image_width, cam.image_height
    g = np.random.default_rng(5)
    y, x = np.meshgrid(np.arange(2 * H), np.arange(2 * W), indexing="ij")
    disc = np.clip(300 - 2.5 * np.hypot(x - W, y - H), 0, 255).astype(np.uint8)
    view = dict(image=_dev(g.integers(0, 256, (2 * H, 2 * W, 3), dtype=np.uint8)), mask_hair=_dev(disc), mask_body=_dev(np.maximum(disc, 90)),
                angle=_dev(g.integers(0, 180, (2 * H, 2 * W)).astype(np.uint8)), var=_dev((g.random((2 * H, 2 * W)) * 2).astype(np.float16)))
    with pytest.raises(ValueError):
        gt.attach_ground_truth([cam], [view], resolution=1)
    assert gt.attach_ground_truth([cam], [view], resolution=2, binarize_masks=True) == [cam]
    for t, c in ((cam.original_image, 3), (cam.original_mask, 2), (cam.original_orient_angle, 1), (cam.original_orient_conf, 1)):
        assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (c, H, W) and t.is_contiguous() and torch.isfinite(t).all()
    opt = OptimizationParams()
    model.training_setup(opt)
    loss = float(training_step(model, [cam], bg, opt, 1))
    checksum = sum(float(p.detach().double().sum()) for p in (model._xyz, model._scaling, model._rotation, model._opacity, model._features_dc))
    assert np.isfinite(loss) and loss > 0 and np.isfinite(checksum)
