"""`-m gpu`: the orientation maps on the device -- ghr_orient_dog / ghr_orient_gabor through the C ABI on the golden cases of
tests/test_orient_cpu.py (same bars), the bank alone on the golden planes, a (130, 200) image and a second bank against a float64
restatement, the zero plane, the ground-truth tensors of the same launch, the camera hook, and the fused form against the
PyTorch-composed comparator on the device.

Shapes: (5, 7) is smaller than the 17-tap window, the DoG's radius 40 and one 16 x 8 workgroup tile; (16, 17) is one pixel past
a tile's width with two tile rows; (33, 47) odd, unaligned rows, 3 x 5 workgroups; (70, 90) 6 x 9 workgroups and two DoG
blocks along x; (130, 200) four DoG blocks along x and 13 x 17 workgroups.  The 45-filter bank of 11 x 11 taps takes the kernel's
one-tile-per-wave form with an idle wave, a tap count that is no multiple of 4 and another halo."""
import math

import numpy as np
import pytest
import torch

from tests.golden import make_reference_orient_golden as mk
from tests.test_orient_cpu import N_CASES, case_ref, check_maps, check_plane, conf_numpy, gold  # noqa: F401  (gold: fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _dog(image):
    """through the C ABI into a buffer pre-filled with NaN"""
    from gaussianhaircut_amd import orientation as ori
    t = _dev(image)
    out = torch.full(t.shape[:2], float("nan"), dtype=torch.float32, device=DEV)
    ori.dog_fused(t, out=out)
    return out


def _gabor(plane, bank=None, **kw):
    """through the C ABI into buffers pre-filled with 0xAB bytes; host arrays"""
    from gaussianhaircut_amd import orientation as ori
    return tuple(t.cpu().numpy() for t in ori.gabor_fused(plane, bank, fill=0xAB, **kw))


def _restated(image, bank):
    """the test's own float64 restatement of a case the golden does not hold: scipy's DoG, then the responses in double; var32
    from the comparator's float32 run on the CPU"""
    from gaussianhaircut_amd import orientation as ori
    w, th = bank
    grey = 0.2989 * image[:, :, 0] + 0.5870 * image[:, :, 1] + 0.1140 * image[:, :, 2]
    dog32 = mk.difference_of_gaussians(grey, 0.4, 10).astype(np.float32)
    F64, k64, var64, margin = mk.restate64(dog32, w, th)
    _, var32 = ori.gabor_orientation(dog32, bank, fused=False)
    return dict(image=image, dog32=dog32, F64=F64, k=k64, var64=var64, var32=var32, margin=margin)


@pytest.fixture(scope="module")
def big():
    from gaussianhaircut_amd import orientation as ori
    return _restated(mk.make_image(130, 200, 7), ori.gabor_bank())


@pytest.fixture(scope="module")
def bank45():
    from gaussianhaircut_amd import orientation as ori
    return ori.gabor_bank(num_filters=45, sigma_x=1.0, sigma_y=1.5)


@pytest.mark.parametrize("i", range(N_CASES))
def test_kernels_match_the_reference_golden(gold, i):
    plane = _dog(gold["c%d/image" % i])
    check_plane(plane.cpu().numpy(), gold["c%d/dog32" % i], "gpu case %d" % i)
    deg, var = _gabor(plane)
    assert deg.dtype == np.uint8
    check_maps(deg, var, case_ref(gold, i), "gpu case %d" % i)
    plane2 = _dog(gold["c%d/image" % i])
    deg2, var2 = _gabor(plane2)
    assert np.array_equal(plane.cpu().numpy().view(np.uint32), plane2.cpu().numpy().view(np.uint32))
    assert np.array_equal(deg, deg2) and np.array_equal(var.view(np.uint32), var2.view(np.uint32))


@pytest.mark.parametrize("i", range(N_CASES))
def test_bank_kernel_alone_on_the_golden_plane(gold, i):
    deg, var = _gabor(_dev(gold["c%d/dog32" % i]))
    check_maps(deg, var, case_ref(gold, i), "gpu case %d, bank alone" % i)


def test_kernels_match_the_float64_restatement_at_130_by_200(big):
    plane = _dog(big["image"])
    check_plane(plane.cpu().numpy(), big["dog32"], "gpu 130x200")
    deg, var = _gabor(plane)
    check_maps(deg, var, big, "gpu 130x200")
    deg2, var2 = _gabor(plane)
    assert np.array_equal(deg, deg2) and np.array_equal(var.view(np.uint32), var2.view(np.uint32))


def test_a_second_bank_of_45_filters_and_11_taps(gold, bank45):
    ref = _restated(gold["c2/image"], bank45)
    deg, var = _gabor(_dev(ref["dog32"]), bank45)
    assert deg.max() < 45
    check_maps(deg, var, ref, "gpu 45 filters, ksize 11")


def test_grey_and_float_images(gold):
    img = gold["c2/image"]
    g8 = np.ascontiguousarray(img[:, :, 1])
    ref = mk.difference_of_gaussians(g8.astype(np.float64), 0.4, 10).astype(np.float32)
    check_plane(_dog(g8).cpu().numpy(), ref, "gpu grey uint8")
    check_plane(_dog(g8.astype(np.float32)).cpu().numpy(), ref, "gpu grey float32")
    check_plane(_dog(img.astype(np.float32)).cpu().numpy(), gold["c2/dog32"], "gpu rgb float32")


def test_zero_plane_gives_the_first_filter_and_zero_variance():
    deg, var, angle, conf = _gabor(torch.zeros((19, 35), dtype=torch.float32, device=DEV), ground_truth=True)
    assert deg.shape == var.shape == (19, 35) and not deg.any() and not var.any()
    assert not angle.any() and np.array_equal(conf, np.full((1, 19, 35), conf_numpy(np.zeros(1, np.float32))[0]))


def test_ground_truth_tensors_come_out_of_the_same_launch(gold):
    from gaussianhaircut_amd import orientation as ori
    plane = _dev(gold["c3/dog32"])
    deg, var, angle, conf = _gabor(plane, ground_truth=True)
    deg0, var0 = _gabor(plane)
    assert np.array_equal(deg, deg0) and np.array_equal(var.view(np.uint32), var0.view(np.uint32))
    assert angle.shape == conf.shape == (1,) + deg.shape and angle.dtype == conf.dtype == np.float32
    assert np.array_equal(angle[0], deg.astype(np.float32) / np.float32(180.0))
    exp = conf_numpy(var.astype(np.float16))
    assert (np.abs(conf[0] - exp) <= 2 * np.spacing(exp)).all()
    full = _gabor(plane, ground_truth=True, via_float16=False)[3]
    exp = conf_numpy(var)
    assert (np.abs(full[0] - exp) <= 2 * np.spacing(exp)).all() and not np.array_equal(full, conf)
    a, c = ori.ground_truth_from_maps(deg, var)   # the loader's form of the same two tensors
    assert np.array_equal(a, angle) and (np.abs(c - conf) <= 2 * np.spacing(conf)).all()


def test_attach_fills_ring_cameras_and_the_loss_accepts_them(gold):
    from gaussianhaircut_amd import orientation as ori
    from gaussianhaircut_amd.fused_loss import stage1_loss
    from gaussianhaircut_amd.scene.cameras import ring_cameras
    imgs = [gold["c3/image"], np.ascontiguousarray(gold["c3/image"][::-1])]
    H, W = imgs[0].shape[:2]
    cams = ring_cameras(2, W, H, device=DEV)
    assert ori.attach_orientation_ground_truth(cams, [_dev(im) for im in imgs]) == cams
    for cam in cams:
        for t in (cam.original_orient_angle, cam.original_orient_conf):
            assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (1, H, W) and torch.isfinite(t).all()
    a, c = ori.ground_truth_from_maps(*ori.orientation_maps(_dev(imgs[0]))[:2])
    # the loader's form on the device: the same angle; each confidence is within 2 float32 spacings of the loader's float32 chain
    # (the bar of the tests above), so the two are within 4 spacings = 4.8e-7 of each other
    assert torch.equal(cams[0].original_orient_angle, a)
    assert torch.allclose(cams[0].original_orient_conf, c, rtol=4.8e-7, atol=0)
    exp = conf_numpy(ori.orientation_maps(_dev(imgs[0])).var.cpu().numpy().astype(np.float16))
    assert (np.abs(c[0].cpu().numpy() - exp) <= 2 * np.spacing(exp)).all()
    assert (np.abs(cams[0].original_orient_conf[0].cpu().numpy() - exp) <= 2 * np.spacing(exp)).all()
    assert not torch.equal(cams[0].original_orient_angle, cams[1].original_orient_angle)
    assert ori.attach_orientation_ground_truth(cams, imgs) == []   # nothing is missing any more
    g = torch.Generator().manual_seed(11)
    packed = torch.rand((10, H, W), generator=g).to(DEV)
    packed[5:7] -= 0.5
    gt_image, gt_mask = torch.rand((3, H, W), generator=g).to(DEV), torch.rand((2, H, W), generator=g).to(DEV)
    base = stage1_loss(packed, gt_image, gt_mask, cams[0].original_orient_angle, cams[0].original_orient_conf, 0.8, 0.2, 0.1, 0.0)
    full = stage1_loss(packed, gt_image, gt_mask, cams[0].original_orient_angle, cams[0].original_orient_conf, 0.8, 0.2, 0.1, 0.1)
    assert torch.isfinite(base) and torch.isfinite(full) and float(full) > float(base)


def test_fused_and_comparator_on_the_device_at_70_by_90(gold):
    from gaussianhaircut_amd import orientation as ori
    img = _dev(gold["c3/image"])
    for fused in (None, False):
        m = ori.orientation_maps(img, fused=fused)
        assert m.deg.is_cuda and m.deg.dtype == torch.uint8 and m.var.dtype == torch.float32
        what = "device, fused=%s" % fused
        check_plane(m.filtered.cpu().numpy(), gold["c3/dog32"], what)
        check_maps(m.deg.cpu().numpy(), m.var.cpu().numpy(), case_ref(gold, 3), what)
