"""`-m gpu`: the comparison video's frame assembly on the device (csrc/ghr_compare.h, gaussianhaircut_amd/comparison.py, DESIGN.md
8n): ghr_cmp_over_white and ghr_cmp_strip through the C ABI against the comparator that tests/test_comparison_cpu.py pins to
Pillow, in every access form, into sentinel-filled buffers with guard bytes; whole frames against the golden file and the
comparator; the frame generator; one frame from interpolated cameras through the Gaussian render and the strand preview.
Everything is compared bit for bit.  Neither the reference nor Pillow is needed here."""
import math

import numpy as np
import pytest
import torch

from tests import comparison_cases as cc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD, SENTINEL = 64, 0xAB


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _guarded(n, offset=0):
    """a sentinel-filled buffer and its n-byte middle, which starts 64 + offset bytes into it (torch's blocks are 256-B aligned)"""
    buf = torch.full((GUARD + offset + n + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD + offset:GUARD + offset + n]


def _intact(buf, n, offset=0):
    return bool((buf[:GUARD + offset] == SENTINEL).all()) and bool((buf[GUARD + offset + n:] == SENTINEL).all())


# ---- ghr_cmp_over_white ----------------------------------------------------------------------------------------------------------

def _over_white_forms(rgba):
    """the four-pixel form (both buffers aligned), the one-pixel form through an input one pixel into its buffer, and through an
    output one byte into its buffer"""
    from gaussianhaircut_amd import comparison as cmp
    H, W = rgba.shape[:2]
    n = 3 * H * W
    t = _dev(rgba)
    assert t.data_ptr() % 16 == 0
    buf, mid = _guarded(n)
    vec = cmp.over_white_fused(t, out=mid).reshape(H, W, 3).clone()
    assert mid.data_ptr() % 4 == 0 and _intact(buf, n)
    shifted = torch.empty(4 * H * W + 4, dtype=torch.uint8, device=DEV)
    view = shifted[4:].view(H, W, 4)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    buf, mid = _guarded(n)
    scalar_in = cmp.over_white_fused(view, out=mid).reshape(H, W, 3).clone()
    assert _intact(buf, n)
    buf, mid = _guarded(n, offset=1)
    scalar_out = cmp.over_white_fused(t, out=mid).reshape(H, W, 3).clone()
    assert mid.data_ptr() % 4 == 1 and _intact(buf, n, offset=1)
    return vec, scalar_in, scalar_out


def test_over_white_all_pairs_in_every_form():
    from gaussianhaircut_amd import comparison as cmp
    rgba = cc.all_pairs()
    want = cmp.over_white(rgba, fused=False)
    assert np.array_equal(want, cc.gold()["over_white_rgb"])
    for got in _over_white_forms(rgba):
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(cmp.over_white(_dev(rgba)), _dev(want))                  # fused=None on a ROCm tensor: the kernel
    assert torch.equal(cmp.over_white(_dev(rgba), fused=False), _dev(want))     # the comparator on the device


@pytest.mark.parametrize("shape", [(1, 1), (1, 3), (3, 5), (7, 9), (41, 25)], ids=lambda s: "%dx%d" % s)
def test_over_white_at_pixel_counts_that_are_no_multiple_of_four(shape):
    """(41, 25): 1025 pixels, a last quad of one pixel alone in a second block (a block makes 1024 pixels)"""
    from gaussianhaircut_amd import comparison as cmp
    g = np.random.default_rng(shape[0] * 100 + shape[1])
    rgba = g.integers(0, 256, shape + (4,), dtype=np.uint8)
    rgba[0, 0, 3] = 0
    rgba[-1, -1, 3] = 255
    want = cmp.over_white(rgba, fused=False)
    assert np.array_equal(want, cc.over_white_formula(rgba))
    for got in _over_white_forms(rgba):
        assert np.array_equal(got.cpu().numpy(), want)


# ---- ghr_cmp_strip ---------------------------------------------------------------------------------------------------------------

def _strip_case(preview_size, render_size, seed):
    from gaussianhaircut_amd import comparison as cmp
    g = np.random.default_rng(seed)
    w, h = render_size
    lay = cmp.comparison_layout(None, preview_size, render_size)
    gt = g.integers(1, 256, (h, w, 3), dtype=np.uint8)
    render = g.integers(1, 256, (h, w, 3), dtype=np.uint8)
    small = g.integers(1, 256, (lay.preview_h, lay.preview_w, 3), dtype=np.uint8)   # no zero byte: zeros are padding
    return lay, gt, small, render


def _check_strip(lay, gt, small, render):
    from gaussianhaircut_amd import comparison as cmp
    w, h = lay.w, lay.h
    n = 9 * w * h
    want = cmp.strip_torch(torch.from_numpy(gt), torch.from_numpy(small), torch.from_numpy(render), lay).numpy()
    assert np.array_equal(want, cc.strip_by_hand(gt, small, render, lay.pad_left, lay.pad_top, lay.crop_left, lay.crop_top))
    outs = []
    for offset in (0, 1):   # an output 4-B aligned (dwords where w % 4 == 0) and one byte off (single bytes)
        buf, mid = _guarded(n, offset)
        got = cmp.strip_fused(_dev(gt), _dev(small), _dev(render), lay, out=mid).reshape(h, 3 * w, 3)
        assert mid.data_ptr() % 4 == offset and _intact(buf, n, offset)
        assert np.array_equal(got.cpu().numpy(), want), (lay, offset)
        outs.append(got.clone())
    assert torch.equal(outs[0], outs[1])
    mid_panel = outs[0][:, w:2 * w].cpu().numpy()
    zero = (mid_panel == 0).all(axis=2)
    assert int(zero.sum()) == h * (lay.pad_left + lay.pad_right) + w * (lay.pad_top + lay.pad_bottom) \
        - (lay.pad_left + lay.pad_right) * (lay.pad_top + lay.pad_bottom)
    assert zero[:, :lay.pad_left].all() and zero[:, w - lay.pad_right:].all()
    assert int((mid_panel == 0).sum()) == 3 * int(zero.sum())               # padded pixels are exactly zero, and nothing else is


@pytest.mark.parametrize("render_size", [(5, 7), (16, 9), (33, 18)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("case", cc.LAYOUTS, ids=[c[0] for c in cc.LAYOUTS])
def test_strip_equals_the_comparator(case, render_size):
    """every strand-render shape of the CPU list against each of the three panels: (5, 7) and (33, 18) have rows of 45 and 297
    bytes (single bytes), (16, 9) rows of 144 (dwords); (33, 18) is more than one block"""
    _check_strip(*_strip_case(case[1], render_size, seed=len(case[0]) + render_size[0]))


@pytest.mark.parametrize("name,preview,render,resized,pads,crop", cc.LAYOUTS, ids=[c[0] for c in cc.LAYOUTS])
def test_strip_at_the_layouts_own_sizes(name, preview, render, resized, pads, crop):
    lay, gt, small, rnd = _strip_case(preview, render, seed=3)
    assert (lay.preview_w, lay.preview_h) == resized and (lay.pad_left, lay.pad_top, lay.pad_right, lay.pad_bottom) == pads
    _check_strip(lay, gt, small, rnd)


def test_strip_pads_above_and_below_too():
    """Resize never leaves the strand render lower than the panel, so the layout never pads rows; the C function takes it"""
    from gaussianhaircut_amd import comparison as cmp
    g = np.random.default_rng(9)
    for w, h in ((12, 11), (7, 10)):
        lay = cmp.ComparisonLayout(w, h, w - 3, h - 5, 1, 2, 2, 3, 0, 0, 3 * w, h)
        _check_strip(lay, g.integers(1, 256, (h, w, 3), dtype=np.uint8), g.integers(1, 256, (h - 5, w - 3, 3), dtype=np.uint8),
                     g.integers(1, 256, (h, w, 3), dtype=np.uint8))


# ---- frames ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cc.golden_names())
def test_frame_equals_the_golden(name):
    from gaussianhaircut_amd import comparison as cmp
    gt, preview, render, short, want = cc.golden_case(name)
    got = cmp.comparison_frame(_dev(gt), _dev(preview), _dev(render), short, fused=True)
    assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(cmp.comparison_frame(_dev(gt), _dev(preview), _dev(render), short), got)             # fused=None
    assert torch.equal(cmp.comparison_frame(_dev(gt), _dev(preview), _dev(render), short, fused=False), got)
    host = cmp.comparison_frame(gt, _dev(preview), _dev(render), short)     # a host photograph is uploaded; numpy in, numpy out
    assert isinstance(host, np.ndarray) and np.array_equal(host, want)


def _large_case():
    g = np.random.default_rng(70126)
    y, x = np.meshgrid(np.arange(252), np.arange(140), indexing="ij")
    gt = np.stack([(x * 3 + y) % 256, (x + 2 * y) % 256, (5 * x + 7 * y) % 251], -1).astype(np.uint8)
    gt ^= g.integers(0, 32, gt.shape, dtype=np.uint8)
    preview = g.integers(0, 256, (150, 150, 4), dtype=np.uint8)
    preview[:, :, 3] = np.where(g.random((150, 150)) < 0.5, 255, preview[:, :, 3])
    render = g.integers(0, 256, (126, 70, 3), dtype=np.uint8)
    return gt, preview, render


def test_a_frame_of_more_than_one_block():
    """render 70 x 126, strand render 150 x 150 RGBA, photograph 140 x 252, out_short 64: every pass has several blocks"""
    from gaussianhaircut_amd import comparison as cmp
    gt, preview, render = _large_case()
    want = cmp.comparison_frame(gt, preview, render, 64, fused=False)
    lay = cmp.comparison_layout((140, 252), (150, 150), (70, 126), 64)
    assert want.shape == (lay.out_h, lay.out_w, 3) == (64, 106, 3)
    d = [_dev(a) for a in (gt, preview, render)]
    first = cmp.comparison_frame(*d, 64, fused=True)
    assert np.array_equal(first.cpu().numpy(), want)
    out = torch.empty((lay.out_h, lay.out_w, 3), dtype=torch.uint8, device=DEV)
    res = cmp.comparison_frame(*d, 64, fused=True, out=out)
    assert res.data_ptr() == out.data_ptr() and torch.equal(out, first)                 # the same call twice: the same bytes
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(DEV)
    res = cmp.comparison_frame(*d, 64, fused=True, out=out)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(DEV) == before and res.data_ptr() == out.data_ptr() and torch.equal(out, first)
    st_f, st_c = cmp.comparison_stages(*d, 64, fused=True), cmp.comparison_stages(*d, 64, fused=False)
    for k in ("preview", "gt", "strip", "frame"):
        assert torch.equal(st_f[k], st_c[k]), k
    with pytest.raises(ValueError):
        cmp.comparison_frame(*d, 64, fused=True, out=torch.empty((64, 105, 3), dtype=torch.uint8, device=DEV))


def test_frames_are_the_single_frames_and_stay_valid():
    from gaussianhaircut_amd import comparison as cmp
    names = ["square_rgba", "half_of_one", "square_rgba"]      # the first and the third share a pinned buffer
    cases = [cc.golden_case(n) for n in names]
    renders = [c[2].copy() for c in cases]
    renders[2] = 255 - renders[2]
    it = cmp.comparison_frames([c[0] for c in cases], [_dev(c[1]) for c in cases], [_dev(r) for r in renders], out_short=10)
    got, kept = [], []
    for f in it:
        assert isinstance(f, np.ndarray) and f.dtype == np.uint8 and f.flags["OWNDATA"]
        got.append(f)
        kept.append(f.copy())
    assert len(got) == 3
    for f, k, c, r in zip(got, kept, cases, renders):
        assert np.array_equal(f, k)                                                      # not overwritten by a later frame
        assert np.array_equal(f, cmp.comparison_frame(c[0], c[1], r, 10, fused=False))
    assert not np.array_equal(got[0], got[2])
    host_only = list(cmp.comparison_frames([c[0] for c in cases], [c[1] for c in cases], renders, out_short=10, device=DEV))
    assert all(np.array_equal(a, b) for a, b in zip(host_only, got))


# ---- one frame, end to end -------------------------------------------------------------------------------------------------------

def test_one_frame_from_interpolated_cameras_to_the_strip():
    from gaussianhaircut_amd import comparison as cmp
    from gaussianhaircut_amd import evaluation as ev
    from gaussianhaircut_amd import strand_view as sv
    from gaussianhaircut_amd import visibility as vis
    from gaussianhaircut_amd.scene import interpolated_cameras, ring_cameras
    from gaussianhaircut_amd.utils import synthetic as syn
    W, H = 36, 64
    spec = syn.WorkloadSpec("comparison_300_36x64", 300, W, H, 21, "random", math.log(0.12))
    model = syn.make_model(spec, DEV)
    bg = syn.background(DEV)
    keys = ring_cameras(16, W, H, device=DEV)[:2]
    keys[0].image_name, keys[1].image_name = "000002", "000006"
    cams = interpolated_cameras(keys, speed_up=2, device=DEV)
    assert [c.image_name for c in cams] == ["000002", "000004"]
    origins, dirs = syn.strand_polylines(12, 24, 4, step=0.04)
    points = (origins + torch.cat([torch.zeros_like(origins), torch.cumsum(dirs, dim=1)], dim=1)).contiguous().to(DEV)
    g = np.random.default_rng(2)
    lay = cmp.comparison_layout((2 * W, 2 * H), (W, H), (W, H), out_short=48)
    frames = []
    for cam, prod in zip(cams, ev.render_products(model, cams, bg)):
        assert prod["name"] == cam.image_name and prod["render"].shape == (H, W, 3)
        pic = sv.render_strands(points, vis.view_matrix_from_camera(cam), supersample=1, device=DEV)
        assert tuple(pic.shape) == (H, W, 3) and pic.dtype == torch.uint8
        photo = g.integers(0, 256, (2 * H, 2 * W, 3), dtype=np.uint8)
        st = cmp.comparison_stages(_dev(photo), pic, _dev(prod["render"]), out_short=48, fused=True)
        frame = st["frame"]
        assert tuple(frame.shape) == (lay.out_h, lay.out_w, 3) == (48, 81, 3) and frame.dtype == torch.uint8
        strip = st["strip"].cpu().numpy()
        assert np.array_equal(strip[:, 2 * W:], prod["render"])                          # the right third: the render's bytes
        assert tuple(st["preview"].shape) == (lay.preview_h, lay.preview_w, 3) == (113, 64, 3)   # the short edge becomes h
        assert np.array_equal(strip[:, W:2 * W], st["preview"].cpu().numpy()[lay.crop_top:lay.crop_top + H, lay.crop_left:lay.crop_left + W])
        assert np.array_equal(frame.cpu().numpy(), cmp.comparison_frame(photo, pic.cpu().numpy(), prod["render"], 48, fused=False))
        assert prod["render"].std() > 0 and pic.float().std() > 0
        frames.append(frame.cpu().numpy())
    assert not np.array_equal(frames[0], frames[1])
