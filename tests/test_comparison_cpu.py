"""The comparison video's frame assembly without a GPU (gaussianhaircut_amd/comparison.py): the comparator
(fused=False) against the formula, the golden file Pillow wrote (tests/golden/make_comparison_golden.py) and, where Pillow imports,
Pillow itself; the layout's numbers; what the two C functions refuse.  Everything is compared bit for bit: the arithmetic is in
integers."""
import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd import comparison as cmp
from tests import comparison_cases as cc

X = 0x10000   # stands for a buffer: a refused call follows no pointer


# ---- over white ------------------------------------------------------------------------------------------------------------------

def test_the_all_pairs_image_carries_every_pair_in_every_channel():
    rgba = cc.all_pairs()
    for c in range(3):
        assert len(set(zip(rgba[:, :, 3].ravel().tolist(), rgba[:, :, c].ravel().tolist()))) == 65536
    assert not np.array_equal(rgba[:, :, 0], rgba[:, :, 1]) and not np.array_equal(rgba[:, :, 1], rgba[:, :, 2])


def test_over_white_equals_the_formula_and_the_golden():
    rgba = cc.all_pairs()
    got = cmp.over_white(rgba, fused=False)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (256, 256, 3)
    assert np.array_equal(got, cc.over_white_formula(rgba))
    assert np.array_equal(got, cc.gold()["over_white_rgb"])
    t = cmp.over_white(torch.from_numpy(rgba), fused=False)
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), got)
    assert np.array_equal(got[255], rgba[255, :, :3]) and (got[0] == 255).all()   # opaque: the image; clear: white


def test_over_white_equals_pillow():
    pytest.importorskip("PIL")
    from tests.golden import make_comparison_golden as mk
    rgba = cc.all_pairs()
    assert np.array_equal(cmp.over_white(rgba, fused=False), np.asarray(mk.over_white(rgba)))


def test_over_white_refuses_what_it_is_not_built_for():
    with pytest.raises(ValueError):
        cmp.over_white(np.zeros((4, 4, 3), np.uint8), fused=False)
    with pytest.raises(ValueError):
        cmp.over_white(np.zeros((4, 4), np.uint8), fused=False)
    with pytest.raises(ValueError):
        cmp.over_white(np.zeros((4, 4, 4), np.float32), fused=False)
    with pytest.raises(ValueError):
        cmp.over_white(np.zeros((4, 4, 4), np.uint8), fused=True)   # CPU tensors have no kernels


# ---- layout ----------------------------------------------------------------------------------------------------------------------

def test_short_edge_truncates_as_python_does():
    assert cmp.short_edge(7, 9, 5) == (5, 6)          # 45 / 7 = 6.43
    assert cmp.short_edge(9, 7, 5) == (6, 5)
    assert cmp.short_edge(8, 8, 3) == (3, 3)
    assert cmp.short_edge(2160, 3840, 576) == (576, 1024)
    assert cmp.short_edge(3 * 576, 1024, 720) == (1215, 720)
    assert all(isinstance(v, int) for v in cmp.short_edge(7, 9, 5))


@pytest.mark.parametrize("name,preview,render,resized,pads,crop", cc.LAYOUTS, ids=[c[0] for c in cc.LAYOUTS])
def test_layout_of_the_middle_panel(name, preview, render, resized, pads, crop):
    w, h = render
    lay = cmp.comparison_layout(None, preview, render)
    assert (lay.w, lay.h) == (w, h) and (lay.preview_w, lay.preview_h) == resized
    assert (lay.pad_left, lay.pad_top, lay.pad_right, lay.pad_bottom) == pads
    assert (lay.crop_left, lay.crop_top) == crop
    assert all(type(v) is int for v in lay)
    # the window lies inside the padded image
    assert 0 <= lay.crop_left <= lay.preview_w + lay.pad_left + lay.pad_right - w
    assert 0 <= lay.crop_top <= lay.preview_h + lay.pad_top + lay.pad_bottom - h
    if w <= h:   # a photograph of the render's own size fits, and changes nothing of the middle panel
        assert cmp.comparison_layout((w, h), preview, render) == lay
        assert cmp.comparison_layout((2 * w, 2 * h), preview, render) == lay


def test_layout_of_the_frame():
    lay = cmp.comparison_layout((2160, 3840), (1920, 1920), (576, 1024))
    assert lay == cmp.ComparisonLayout(576, 1024, 1024, 1024, 0, 0, 0, 0, 224, 0, 1215, 720)
    assert cmp.comparison_layout((18, 32), (40, 40), (9, 16), out_short=12)[-2:] == (20, 12)   # 12 * 27 / 16 = 20.25


def test_a_photograph_of_another_aspect_is_refused():
    with pytest.raises(ValueError, match=r"9 x 15 .* 9 x 16"):
        cmp.comparison_layout((19, 32), (40, 40), (9, 16))      # int(9 * 32 / 19) = 15, not 16
    with pytest.raises(ValueError, match=r"28 x 16 .* 16 x 9"):
        cmp.comparison_layout((16, 9), (5, 21), (16, 9))        # a landscape render: Resize(16) makes 28 x 16 of its own size
    with pytest.raises(ValueError):
        cmp.comparison_layout((18, 32), (40, 40), (0, 16))


# ---- frames ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cc.golden_names())
def test_frame_equals_the_golden(name):
    gt, preview, render, short, want = cc.golden_case(name)
    got = cmp.comparison_frame(gt, preview, render, short, fused=False)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want)
    lay = cmp.comparison_layout(gt.shape[1::-1], preview.shape[1::-1], render.shape[1::-1], short)
    assert got.shape == (lay.out_h, lay.out_w, 3)
    t = cmp.comparison_frame(torch.from_numpy(gt), torch.from_numpy(preview), torch.from_numpy(render), short)   # fused=None on the CPU
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), want)


@pytest.mark.parametrize("name", cc.golden_names())
def test_frame_equals_pillow(name):
    pytest.importorskip("PIL")
    from tests.golden import make_comparison_golden as mk
    gt, preview, render, short, _ = cc.golden_case(name)
    assert np.array_equal(cmp.comparison_frame(gt, preview, render, short, fused=False), mk.frame(gt, preview, render, short))


def test_the_strip_of_a_frame_is_the_three_panels():
    gt, preview, render, short, _ = cc.golden_case("square_rgba")
    st = cmp.comparison_stages(gt, preview, render, short, fused=False)
    lay = cmp.comparison_layout(gt.shape[1::-1], preview.shape[1::-1], render.shape[1::-1], short)
    strip = st["strip"].numpy()
    assert strip.shape == (lay.h, 3 * lay.w, 3)
    assert np.array_equal(strip[:, 2 * lay.w:], render) and np.array_equal(strip[:, :lay.w], st["gt"].numpy())
    assert np.array_equal(strip, cc.strip_by_hand(st["gt"].numpy(), st["preview"].numpy(), render, lay.pad_left, lay.pad_top,
                                                  lay.crop_left, lay.crop_top))


@pytest.mark.parametrize("name,preview,render,resized,pads,crop", cc.LAYOUTS, ids=[c[0] for c in cc.LAYOUTS])
def test_the_comparators_strip_is_the_definition(name, preview, render, resized, pads, crop):
    """padding included: the zeros are where the C ABI's words put them"""
    g = np.random.default_rng(5)
    w, h = render
    lay = cmp.comparison_layout(None, preview, render)
    a, b = g.integers(1, 256, (h, w, 3), dtype=np.uint8), g.integers(1, 256, (h, w, 3), dtype=np.uint8)
    small = g.integers(1, 256, (lay.preview_h, lay.preview_w, 3), dtype=np.uint8)
    got = cmp.strip_torch(torch.from_numpy(a), torch.from_numpy(small), torch.from_numpy(b), lay).numpy()
    assert np.array_equal(got, cc.strip_by_hand(a, small, b, lay.pad_left, lay.pad_top, lay.crop_left, lay.crop_top))
    mid = got[:, w:2 * w]
    assert (mid[:, :lay.pad_left] == 0).all() and (mid[:, w - lay.pad_right:] == 0).all()
    assert int((mid == 0).all(axis=2).sum()) == h * (lay.pad_left + lay.pad_right)   # the inputs hold no zero


def test_frame_checks_its_inputs():
    gt, preview, render, short, _ = cc.golden_case("square_rgba")
    with pytest.raises(ValueError, match="uint8"):
        cmp.comparison_frame(gt.astype(np.float32), preview, render, short, fused=False)
    with pytest.raises(ValueError, match="uint8"):
        cmp.comparison_frame(gt, preview, render.astype(np.int16), short, fused=False)
    with pytest.raises(ValueError):
        cmp.comparison_frame(gt[:, :, 0], preview, render, short, fused=False)            # rank
    with pytest.raises(ValueError):
        cmp.comparison_frame(gt, preview[:, :, :2], render, short, fused=False)           # two channels
    with pytest.raises(ValueError):
        cmp.comparison_frame(gt, preview, np.concatenate([render, render[:, :, :1]], 2), short, fused=False)   # an RGBA render
    with pytest.raises(ValueError):
        cmp.comparison_frame(gt[:-1], preview, render, short, fused=False)                # another aspect
    with pytest.raises(ValueError):
        cmp.comparison_frame(gt, preview, render, short, fused=True)                      # CPU tensors have no kernels


def test_frames_on_the_cpu_are_the_single_frames():
    names = ["square_rgba", "portrait_rgb", "upscale"]
    cases = [cc.golden_case(n) for n in names]
    got = list(cmp.comparison_frames([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], out_short=8))
    assert len(got) == 3
    for f, c in zip(got, cases):
        assert isinstance(f, np.ndarray) and np.array_equal(f, cmp.comparison_frame(c[0], c[1], c[2], 8, fused=False))


# ---- the tool --------------------------------------------------------------------------------------------------------------------

def _tool():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "render_comparison_video.py")
    spec = importlib.util.spec_from_file_location("render_comparison_video", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_tool_assembles_frames_from_directories(tmp_path):
    pytest.importorskip("PIL")
    from PIL import Image
    tool = _tool()
    gt, preview, render, _, _ = cc.golden_case("square_rgba")
    gt2, preview2, render2 = gt[::-1].copy(), preview[:, ::-1].copy(), 255 - render
    for d in ("renders", "blender", "ours", "raw"):
        (tmp_path / d).mkdir()
    # renders 000005 and 000009 pair with photographs 000004 and 000008; Blender's results carry the renders' names, ours are
    # numbered by position
    for name, r, p, g, pos in (("000005", render, preview, gt, 0), ("000009", render2, preview2, gt2, 1)):
        Image.fromarray(r, "RGB").save(tmp_path / "renders" / (name + ".png"))
        Image.fromarray(p, "RGBA").save(tmp_path / "blender" / (name + ".png"))
        Image.fromarray(cmp.over_white(p, fused=False), "RGB").save(tmp_path / "ours" / ("%06d.png" % pos))
        Image.fromarray(g, "RGB").save(tmp_path / "raw" / ("%06d.png" % (int(name) - 1)))
    Image.fromarray(preview, "RGBA").save(tmp_path / "blender" / "000001.png")        # another name: not a render's, not read
    want = [cmp.comparison_frame(gt, preview, render, 12, fused=False), cmp.comparison_frame(gt2, preview2, render2, 12, fused=False)]
    for k, pv in enumerate(("blender", "ours")):
        out = tmp_path / ("out%d" % k)
        n = tool.main(["frames", "--renders", str(tmp_path / "renders"), "--preview", str(tmp_path / pv), "--gt", str(tmp_path / "raw"),
                       "--out", str(out), "--out_short", "12", "--composed"])
        assert n == 2 and sorted(f.name for f in (out / "frames").iterdir()) == ["000000.png", "000001.png"]
        for i in range(2):
            assert np.array_equal(np.asarray(Image.open(out / "frames" / ("%06d.png" % i))), want[i]), (pv, i)


def test_the_tool_reads_key_cameras(tmp_path):
    import json
    from gaussianhaircut_amd.scene.cameras import interpolated_cameras, ring_cameras
    tool = _tool()
    cams = ring_cameras(12, 36, 64)[:3]
    entries = []
    for k, (c, frame) in enumerate(zip(cams, (2, 6, 7))):
        w2c = c.world_view_transform.double().numpy().T
        c2w = np.linalg.inv(w2c)
        entries.append(dict(id=k, img_name="%06d" % frame, width=36, height=64, position=c2w[:3, 3].tolist(), rotation=c2w[:3, :3].tolist(),
                            fx=36 / (2 * np.tan(float(c.FoVx) / 2)), fy=64 / (2 * np.tan(float(c.FoVy) / 2))))
    entries.append(dict(entries[0], img_name="thumbnail"))
    path = tmp_path / "cameras.json"
    path.write_text(json.dumps(entries))
    keys = tool.load_key_cameras(str(path))
    assert [k.image_name for k in keys] == ["000002", "000006", "000007"]
    for k, c in zip(keys, cams):
        assert np.allclose(k.R, c.R, atol=1e-6) and np.allclose(k.T, c.T, atol=1e-6) and abs(float(k.FoVx) - float(c.FoVx)) < 1e-6
        assert torch.allclose(k.world_view_transform, c.world_view_transform, atol=1e-5)
    assert [c.image_name for c in interpolated_cameras(keys, speed_up=2)] == ["000002", "000004", "000006"]


# ---- the C functions' refusals ---------------------------------------------------------------------------------------------------

def _refused(rc, word):
    msg = _lib.lib().ghr_last_error().decode()
    return rc == _lib.GHR_E_INVALID and word in msg, (rc, msg)


def test_the_library_exports_the_two_functions():
    import os
    import re
    L = _lib.lib()
    with open(os.path.join(os.path.dirname(_lib.CSRC), "..", "include", "ghr.h")) as f:
        hdr = f.read()
    for n in ("ghr_cmp_over_white", "ghr_cmp_strip"):
        assert re.search(r"\bint %s\(" % n, hdr) and n in _lib.EXPORTS and hasattr(L, n) and getattr(L, n).argtypes, n
    assert "ghr_compare.h" in _lib.HEADERS and os.path.exists(os.path.join(_lib.CSRC, "ghr_compare.h"))
    assert int(L.ghr_abi_version()) == _lib.ABI_VERSION


@pytest.mark.parametrize("args,word", [
    ((None, 16, None, X + 4096), "NULL"),
    ((None, 16, X, None), "NULL"),
    ((None, 0, X, X + 4096), "n_pixels"),
    ((None, -3, X, X + 4096), "n_pixels"),
    ((None, 16, X, X), "overlap"),
    ((None, 16, X, X + 63), "overlap"),          # rgb begins at rgba's last byte
    ((None, 16, X + 47, X), "overlap"),          # rgba begins at rgb's last byte
    ((None, 1 << 41, X, X + (1 << 44)), "too large"),
], ids=["null-in", "null-out", "zero", "negative", "same", "out-in-in", "in-in-out", "grid"])
def test_over_white_refusals(args, word):
    ok, got = _refused(_lib.lib().ghr_cmp_over_white(*args), word)
    assert ok, got


def _strip_args(**over):
    """w 16, h 9, the resized preview 9 x 37 padded by 3 | 4 to 16 x 37, the window at (0, 14); the four buffers far apart"""
    a = dict(stream=None, w=16, h=9, gt=X, preview=X + 0x10000, pw=9, ph=37, pad_left=3, pad_top=0, crop_left=0, crop_top=14,
             render=X + 0x20000, out=X + 0x30000)
    a.update(over)
    return tuple(a.values())


@pytest.mark.parametrize("over,word", [
    (dict(gt=None), "NULL"), (dict(preview=None), "NULL"), (dict(render=None), "NULL"), (dict(out=None), "NULL"),
    (dict(w=0), "sizes"), (dict(h=-1), "sizes"), (dict(pw=0), "sizes"), (dict(ph=0), "sizes"),
    (dict(out=X), "overlap"), (dict(out=X + 0x20000 - 1), "overlap"), (dict(out=X + 0x10000 + 9 * 37 * 3 - 1), "overlap"),
    (dict(gt=X + 0x30000 + 16 * 9 * 9 - 1), "overlap"),
    (dict(crop_top=29), "window"),               # 29 + 9 > 37
    (dict(crop_left=1), "window"),               # the padded width is w: the window starts at 0
    (dict(crop_left=-1), "window"), (dict(crop_top=-1), "window"),
    (dict(pad_left=8), "padding"),               # 8 + 9 > 16
    (dict(pad_top=1), "padding"),                # 37 >= 9: that axis is not padded
    (dict(pad_left=-1), "padding"),
    (dict(w=1 << 20, h=1 << 20), "too large"),
], ids=["null-gt", "null-preview", "null-render", "null-out", "w0", "h-1", "pw0", "ph0", "out-is-gt", "out-ends-in-render",
        "out-in-preview", "gt-in-out", "window-below", "window-right", "window-left", "window-above", "pad-too-wide", "pad-unpadded-axis",
        "pad-negative", "grid"])
def test_strip_refusals(over, word):
    ok, got = _refused(_lib.lib().ghr_cmp_strip(*_strip_args(**over)), word)
    assert ok, got
