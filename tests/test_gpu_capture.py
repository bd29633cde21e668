"""Synthetic captures on the device (csrc/ghr_capture.h), through the C ABI and the Python API.

Every result is a byte or a float32 compared by its bits, no pixel left out.
 1. ghr_strandview_capture against the numpy model of the definition (tests/capture_cases.py) on every case, into one poisoned
    buffer that holds the four planes with guards around and between them -- once with every plane aligned (row loads, dword and
    16-B stores) and once with the index planes off their 16 B and the output planes at odd addresses (single loads and stores).
    The index planes are the numpy model's where the finer grid is small and the device's own raster otherwise (the raster is
    held to its model in tests/test_gpu_strand_view.py); entries outside their tables are planted through the C ABI only.
 2. capture_view(fused=True) against the PyTorch-composed form on the device; two thousand strands over the sphere at 96 x 128.
 3. capture_ground_truth on four ring cameras against the composed form's tensors on the CPU.
 4. The convention: what the rasterizer, the Gabor bank and the capture mean by an orientation byte (see the test)."""
import ctypes

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd import strand_view as sv
from gaussianhaircut_amd import synthetic_capture as cap
from gaussianhaircut_amd.scene.cameras import ring_cameras
from tests import capture_cases as cc
from tests import capture_convention as conv
from tests import strand_view_cases as sc

pytestmark = pytest.mark.gpu
GUARD = 64
POISON = 0xA5
SMALL = set(cc.SMALL) | set(cc.PLANTED)    # the cases whose index planes come from the numpy model (every planted case is cheap)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _planes(name, s, dev):
    """(case, seg, face) with the index planes [s H, s W] as int32 numpy: the model's, or the device's own raster on a large grid"""
    if (name, s) in SMALL:
        c = cc.case(name, s)
        return c, c["seg"], c["face"]
    b = sc.case(name)
    Ms, rs = sc.supersampled(b["M"], b["r"], s)
    seg, _, face, _ = sv.rasterize_strands(b["points"], Ms, s * b["H"], s * b["W"], mesh=None if b["v"] is None else (b["v"], b["f"]),
                                           half_width=float(rs), head_bias=b["bias"], near=float(sc.NEAR), device=dev)
    c = dict(points=b["points"], Ms=Ms, H=b["H"], W=b["W"], s=s, F=0 if b["f"] is None else len(b["f"]), var_floor=0.0)
    return c, seg.cpu().numpy(), face.cpu().numpy()


def _capture_capi(dev, c, seg, face, aligned, var_floor=None):
    """the four planes through the C entry, in one poisoned buffer: guard | hair | guard | body | guard | angle | guard | var | guard"""
    H, W, s = c["H"], c["W"], c["s"]
    N = H * W
    S, Lp = c["points"].shape[:2]
    pts = torch.from_numpy(np.array(c["points"])).to(dev)
    shift = 0 if aligned else 1
    big = [torch.full((seg.size + 4,), -7, dtype=torch.int32, device=dev) for _ in range(2)]   # 16-B aligned; [1:] is off by 4 B
    for t, plane in zip(big, (seg, face)):
        assert t.data_ptr() % 16 == 0
        t[shift:shift + seg.size] = torch.from_numpy(np.array(plane.reshape(-1))).to(dev)
    pad = lambda n: (n + 15) // 16 * 16    # noqa: E731
    o_hair = GUARD + shift
    o_body = o_hair + pad(N) + GUARD
    o_angle = o_body + pad(N) + GUARD
    o_var = o_angle + pad(N) + GUARD + (3 * shift)                               # 4-B aligned always; 16-B aligned only when `aligned`
    total = o_var + 4 * N + GUARD
    buf = torch.full((total + 16,), POISON, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0 and (buf.data_ptr() + o_var) % 4 == 0 and ((buf.data_ptr() + o_var) % 16 == 0) == aligned
    T = torch.from_numpy(cc.table()).to(dev)
    Mc = (ctypes.c_float * 12)(*[float(x) for x in c["Ms"]])
    at = lambda o: ctypes.c_void_p(buf.data_ptr() + o)   # noqa: E731
    vf = c["var_floor"] if var_floor is None else var_floor
    _lib.check(_lib.lib().ghr_strandview_capture(_stream(), S, Lp, _ptr(pts) if S else None, ctypes.byref(Mc), float(sc.NEAR), H, W, s,
                                                 c["F"], ctypes.c_void_p(big[0].data_ptr() + 4 * shift),
                                                 ctypes.c_void_p(big[1].data_ptr() + 4 * shift), _ptr(T), float(np.float32(vf)),
                                                 at(o_hair), at(o_body), at(o_angle), at(o_var)))
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    keep = np.ones(len(a), bool)
    for o, n in ((o_hair, N), (o_body, N), (o_angle, N), (o_var, 4 * N)):
        keep[o:o + n] = False
    assert (a[keep] == POISON).all(), "a byte outside the four planes was written"
    return (a[o_hair:o_hair + N].reshape(H, W), a[o_body:o_body + N].reshape(H, W), a[o_angle:o_angle + N].reshape(H, W),
            a[o_var:o_var + 4 * N].copy().view(np.float32).reshape(H, W))


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,s", cc.CASES, ids=cc.IDS)
def test_c_abi_equals_the_model_bit_for_bit(dev, name, s):
    c, seg, face = _planes(name, s, dev)
    if (name, s) in SMALL:
        want = cc.model(name, s)[:4]
    else:
        want = cc.model_capture(c["points"], c["Ms"], c["H"], c["W"], s, c["F"], seg, face, c["var_floor"])[:4]
    for aligned in (True, False):
        got = _capture_capi(dev, c, seg, face, aligned)
        for k, (g, w) in enumerate(zip(got, want)):
            assert _same_bits(g, w), (name, s, aligned, k)


@pytest.mark.parametrize("name,s", [("hair-front-15x17", 1), ("ss2-17x33", 2), ("ss4-17x33", 4), ("comb-5x7", 4)])
def test_entries_outside_their_tables_count_as_nothing(dev, name, s):
    c = cc.case(name, s)
    rng = np.random.default_rng(s)
    seg, face = c["seg"].copy(), c["face"].copy()
    K = c["points"].shape[0] * (c["points"].shape[1] - 1)
    bad_seg = np.array([K, K + 1, 2 ** 31 - 1, -2, -(2 ** 31)], np.int64)
    bad_face = np.array([c["F"], c["F"] + 7, 2 ** 31 - 1, -2, -(2 ** 31)], np.int64)
    hit = rng.random(seg.shape) < 0.2
    seg[hit] = rng.choice(bad_seg, int(hit.sum())).astype(np.int32)
    hit = rng.random(seg.shape) < 0.2
    face[hit] = rng.choice(bad_face, int(hit.sum())).astype(np.int32)
    want = cc.model_capture(c["points"], c["Ms"], c["H"], c["W"], s, c["F"], seg, face, 0.125)[:4]
    for aligned in (True, False):
        got = _capture_capi(dev, c, seg, face, aligned, var_floor=0.125)
        for k, (g, w) in enumerate(zip(got, want)):
            assert _same_bits(g, w), (name, s, aligned, k)
    assert (want[0] != cc.model(name, s)[0]).any()


def test_empty_sizes_are_valid_and_touch_nothing(dev):
    L = _lib.lib()
    T = torch.from_numpy(cc.table()).to(dev)
    Mc = (ctypes.c_float * 12)(*([1.0] * 12))
    for H, W in ((0, 5), (5, 0), (0, 0)):
        assert L.ghr_strandview_capture(_stream(), 0, 2, None, ctypes.byref(Mc), 1e-3, H, W, 4, 0, None, None, _ptr(T), 0.0,
                                        None, None, None, None) == _lib.GHR_OK
    got = cap.capture_view(np.zeros((0, 2, 3), np.float32), (sc.view_front(0, 7), 0, 7), device=dev)
    assert tuple(got.mask_hair.shape) == (0, 7) and tuple(got.image.shape) == (0, 7, 3)
    torch.cuda.synchronize()


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def _api(c, fused, dev, **kw):
    sh = sc.shading(c["M"])
    return cap.capture_view(c["points"], (c["M"], c["H"], c["W"]), mesh=None if c["v"] is None else (c["v"], c["f"]), supersample=c["s"],
                            half_width=c["r"], head_bias=c["bias"], near=float(cc.NEAR), var_floor=c["var_floor"], fused=fused,
                            device=dev, eye=sh["eye"], light=sh["light"], **kw)


@pytest.mark.parametrize("name,s", cc.PLANTED + cc.FROM_PREVIEW[::3], ids=["%s-s%d" % x for x in cc.PLANTED + cc.FROM_PREVIEW[::3]])
def test_python_api_fused_equals_composed(dev, name, s):
    if (name, s) in SMALL:
        c = cc.case(name, s)
    else:
        b = sc.case(name)
        c = dict(b, s=s, var_floor=0.0)
    a, b = _api(c, True, dev), _api(c, False, dev)
    assert all(x.device.type == "cuda" for x in a)
    for k, (x, y) in enumerate(zip(a[:4], b[:4])):
        assert x.dtype == torch.uint8 and torch.equal(x, y), (name, s, k)
    assert torch.equal(a.var.view(torch.int32), b.var.view(torch.int32)), (name, s)
    if (name, s) in SMALL:
        for x, w in zip(a[1:], cc.model(name, s)[:4]):
            assert _same_bits(x.cpu().numpy(), w), (name, s)


def test_two_thousand_strands_over_the_sphere(dev):
    pts = sc.hair(2000, 24, 21, through=False)
    v, f = sc.meshes()["sphere"]
    view = (sc.view_front(96, 128), 96, 128)
    for kw in (dict(), dict(shadows=True, shadow_size=256, var_floor=0.094, supersample=2)):
        a = cap.capture_view(pts, view, mesh=(v, f), device=dev, **kw)
        b = cap.capture_view(pts, view, mesh=(v, f), fused=False, device=dev, **kw)
        for k, (x, y) in enumerate(zip(a[:4], b[:4])):
            assert torch.equal(x, y), k
        assert torch.equal(a.var.view(torch.int32), b.var.view(torch.int32))
        pic = sv.render_strands(pts, view, mesh=(v, f), device=dev, **{k: x for k, x in dict(dict(supersample=4), **kw).items()
                                                                         if k != "var_floor"})
        assert torch.equal(a.image, pic)
        hair = a.mask_hair.cpu().numpy()
        assert (hair == 255).sum() > 500 and ((hair > 0) & (hair < 255)).sum() > 500 and (a.mask_body >= a.mask_hair).all()
        assert len(torch.unique(a.angle[a.mask_hair > 0])) > 90


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def test_capture_ground_truth_on_ring_cameras_equals_the_cpu_tensors(dev):
    pts, (v, f) = sc.hair(300, 16, 31, through=False), sc.meshes()["small_sphere"]
    on_dev, on_cpu = ring_cameras(4, 64, 48, radius=4.0, device=dev), ring_cameras(4, 64, 48, radius=4.0)
    cap.capture_ground_truth(pts, on_dev, mesh=(v, f), var_floor=0.05, device=dev)
    cap.capture_ground_truth(pts, on_cpu, mesh=(v, f), var_floor=0.05, fused=False)
    for a, b in zip(on_dev, on_cpu):
        assert a.original_image.is_cuda and tuple(a.original_image.shape) == (3, 48, 64)
        for n in ("original_image", "original_mask", "original_orient_angle", "original_orient_conf"):
            assert torch.equal(getattr(a, n).cpu(), getattr(b, n)), n
        assert float(a.original_mask[0].max()) == 1.0 and 0 < float(a.original_mask[0].mean()) < float(a.original_mask[1].mean())


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phi0", conv.PHI0)
def test_convention_of_the_orientation_byte(dev, phi0):
    """A flat comb of straight dark strands 4.5 pixels apart, as wide as the light gaps between them, turning by half a degree per
    strand from ``phi0``, no head, 128 x 128 (tests/capture_convention.py).  On the pixels where the capture's hair byte is 255 and the
    rendered hair mask is > 0.9, circular differences in degrees against the capture's byte:
      (a) render()'s orient_angle x 180 of free strand-aligned Gaussians of the same segments;
      (b) orientation_maps' byte on the capture's image.
    MEASURED with the CPU forms (the oracle backend; fused=False) on 2391 ... 2440 such pixels per comb, median / 99th percentile in
    degrees (tests/capture_convention.py: CPU_MEASURED, pinned by tests/test_capture_cpu.py):
      (a) 0.44 / 0.54 ... 0.55 -- the quantisation of the byte alone; the median of the signed difference is -0.006;
      (b) 0.0 / 5.0 ... 6.0; the median of the signed difference is 0: no offset, no mirrored angle in either.
    The device's figures are held to those plus 2 degrees (a: one bin of quantisation on each side) and plus 3 degrees (b: the
    bank's own most frequent bytes scatter by up to 3 degrees on ideal stripes)."""
    got = conv.measure(phi0, dev)
    print("convention phi0=%g: %d pixels, (a) median %.2f p99 %.2f, (b) median %.2f p99 %.2f" % ((phi0, got["pixels"]) + got["a"] + got["b"]))
    assert got["pixels"] >= conv.MIN_PIXELS
    ca, cb = conv.CPU_MEASURED[phi0]
    assert got["a"][0] <= ca[0] + 2.0 and got["a"][1] <= ca[1] + 2.0, got
    assert got["b"][0] <= cb[0] + 3.0 and got["b"][1] <= cb[1] + 3.0, got
