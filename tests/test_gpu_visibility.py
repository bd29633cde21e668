"""Head-mesh visibility on the device (csrc/ghr_visibility.h), through the C ABI and the Python API.

Every result is an integer or a byte and every comparison is exact, no pixel left out: ghr_vis_view and ghr_vis_head_mask
against the numpy float32 model of the definition (tests/visibility_cases.py, brute force over all faces) and against the
PyTorch-composed form evaluated on the device.  Outputs land in poisoned buffers between guards."""
import ctypes

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd import visibility as vis
from tests import visibility_cases as vc

pytestmark = pytest.mark.gpu
CASES = list(vc.CASES)
GUARD = 256
POISON = 0xA5
POISON32 = -1515870811  # 0xA5A5A5A5


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _guarded(n, dtype, dev):
    fill = POISON if dtype == torch.uint8 else POISON32
    return torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)


def _check_guards(t, n):
    a = t.cpu().numpy()
    fill = POISON if a.dtype == np.uint8 else POISON32
    assert (a[:GUARD] == fill).all() and (a[GUARD + n:] == fill).all()
    return a[GUARD:GUARD + n]


def _view_capi(dev, v, f, M, H, W, body, hair, ws=None, cnt=None, cnt_head=None):
    """ghr_vis_view into poisoned, guarded buffers (the workspace poisoned too, when it is made here)"""
    V, F = len(v), len(f)
    if ws is None:
        ws = torch.full((vis.vis_workspace_bytes(V, F, H, W),), POISON, dtype=torch.uint8, device=dev)
    vd = torch.from_numpy(np.array(v)).to(dev)
    fd = torch.from_numpy(np.array(f)).to(dev)
    pix, visp = _guarded(H * W, torch.int32, dev), _guarded(H * W, torch.uint8, dev)
    own = cnt is None
    if own:
        cnt, cnt_head = _guarded(V, torch.int32, dev), _guarded(V, torch.int32, dev)
        cnt[GUARD:GUARD + V] = 0
        cnt_head[GUARD:GUARD + V] = 0
    bd = None if body is None else torch.from_numpy(np.array(body)).to(dev)
    hd = None if hair is None else torch.from_numpy(np.array(hair)).to(dev)
    Mc = (ctypes.c_float * 12)(*[float(x) for x in M])
    _lib.check(_lib.lib().ghr_vis_view(_stream(), V, _ptr(vd) if V else None, F, _ptr(fd) if F else None, ctypes.byref(Mc),
                                       float(vc.NEAR), H, W, _ptr(bd), _ptr(hd), _ptr(ws), _ptr(pix[GUARD:]), _ptr(visp[GUARD:]),
                                       _ptr(cnt[GUARD:]), _ptr(cnt_head[GUARD:])))
    torch.cuda.synchronize()
    out = _check_guards(pix, H * W).reshape(H, W), _check_guards(visp, H * W).reshape(H, W)
    return out + ((_check_guards(cnt, V), _check_guards(cnt_head, V)) if own else (None, None))


@pytest.mark.parametrize("name", CASES)
def test_vis_view_equals_the_model_exactly(dev, name):
    v, f, M, H, W, body, hair = vc.case(name)
    want_pix, want_vis, seen, seen_head, head = vc.model_case(name)
    pix, visp, cnt, cnt_head = _view_capi(dev, v, f, M, H, W, body, hair)
    assert np.array_equal(pix, want_pix)
    assert np.array_equal(visp, want_vis)
    assert np.array_equal(cnt, seen.astype(np.int32)) and np.array_equal(cnt_head, seen_head.astype(np.int32))
    # no masks: head holds nowhere
    pix, visp, cnt, cnt_head = _view_capi(dev, v, f, M, H, W, None, None)
    assert np.array_equal(pix, want_pix) and not visp.any()
    assert np.array_equal(cnt, seen.astype(np.int32)) and not cnt_head.any()
    # the Python API: fused against the composed form on the device
    fused = vis.rasterize_mesh((v, f), M, H, W, fused=True, device=dev)
    composed = vis.rasterize_mesh((v, f), M, H, W, fused=False, device=dev)
    assert torch.equal(fused, composed) and np.array_equal(fused.cpu().numpy(), want_pix)


@pytest.mark.parametrize("kind", vc.MASK_KINDS)
def test_head_mask_on_every_kind_and_size(dev, kind):
    for H, W in vc.SIZES:
        body, hair = vc.masks(kind, H, W)
        bd, hd = torch.from_numpy(body).to(dev), torch.from_numpy(hair).to(dev)
        out = _guarded(H * W, torch.uint8, dev)
        _lib.check(_lib.lib().ghr_vis_head_mask(_stream(), H, W, _ptr(bd), _ptr(hd), _ptr(out[GUARD:])))
        torch.cuda.synchronize()
        want = vc.model_head(body, hair)
        assert np.array_equal(_check_guards(out, H * W).reshape(H, W), want.astype(np.uint8)), (kind, H, W)
        assert torch.equal(vis.head_mask(bd, hd), vis.head_mask(bd, hd, fused=False))


@pytest.fixture(scope="module")
def five_views():
    """five views of the torus at three image sizes, with masks of every kind but one; the model's counts"""
    v, f = vc.meshes()["torus"]
    views, masks = [], []
    for k, (vw, (H, W)) in enumerate((("oblique", (48, 64)), ("front", (17, 33)), ("inside", (15, 17)), ("front", (48, 64)),
                                      ("oblique", (16, 16)))):
        views.append((vc.VIEWS[vw](H, W), H, W))
        masks.append(vc.masks(vc.MASK_KINDS[1 + k % 4], H, W, seed=k))
    cnt, cnt_head, planes = np.zeros(len(v), np.int32), np.zeros(len(v), np.int32), []
    for (M, H, W), (body, hair) in zip(views, masks):
        _, visp, seen, seen_head, _ = vc.model_view(v, f, M, H, W, body, hair)
        cnt += seen
        cnt_head += seen_head
        planes.append(visp)
    return v, f, views, masks, cnt, cnt_head, planes


def test_vertex_visibility_over_five_views(dev, five_views):
    v, f, views, masks, want_cnt, want_head, want_planes = five_views
    assert want_cnt.max() >= 3 and 0 < want_head.sum() < want_cnt.sum()
    cnt, cnt_head, planes = vis.vertex_visibility((v, f), views, masks, device=dev)
    assert np.array_equal(cnt.cpu().numpy(), want_cnt) and np.array_equal(cnt_head.cpu().numpy(), want_head)
    for got, want in zip(planes, want_planes):
        assert np.array_equal(got.cpu().numpy(), want)
    # the same views in reverse order (the one workspace then goes through the image sizes the other way round)
    cnt_r, cnt_head_r, planes_r = vis.vertex_visibility((v, f), views[::-1], masks[::-1], device=dev)
    assert torch.equal(cnt_r, cnt) and torch.equal(cnt_head_r, cnt_head)
    assert all(torch.equal(a, b) for a, b in zip(planes_r[::-1], planes))
    # the composed form on the device
    cnt_t, cnt_head_t, planes_t = vis.vertex_visibility((v, f), views, masks, fused=False, device=dev)
    assert torch.equal(cnt_t, cnt) and torch.equal(cnt_head_t, cnt_head)
    assert all(torch.equal(a, b) for a, b in zip(planes_t, planes))
    mask = vis.visible_vertex_mask(cnt, cnt_head, len(views))
    assert np.array_equal(mask.cpu().numpy(), vc.model_vertex_mask(want_cnt, want_head, len(views))) and 0 < int(mask.sum()) < len(v)


def test_workspace_reused_across_image_sizes_and_meshes(dev):
    """one poisoned workspace, sized for the largest case, serves smaller images and other meshes in turn; the counts add up"""
    names = ("ico2-inside-130x250", "bad-camera-17x33", "stack129-screen_w-48x64", "box-front-1x1", "ico2-inside-130x250")
    need = max(vis.vis_workspace_bytes(len(vc.case(n)[0]), len(vc.case(n)[1]), vc.case(n)[3], vc.case(n)[4]) for n in names)
    ws = torch.full((need,), POISON, dtype=torch.uint8, device=dev)
    V = len(vc.case(names[0])[0])
    cnt, cnt_head = _guarded(V, torch.int32, dev), _guarded(V, torch.int32, dev)
    cnt[GUARD:GUARD + V] = 0
    cnt_head[GUARD:GUARD + V] = 0
    for n in names:
        v, f, M, H, W, body, hair = vc.case(n)
        own = n != names[0]
        pix, visp, c, ch = _view_capi(dev, v, f, M, H, W, body, hair, ws=ws, cnt=None if own else cnt, cnt_head=None if own else cnt_head)
        want = vc.model_case(n)
        assert np.array_equal(pix, want[0]) and np.array_equal(visp, want[1]), n
        if own:
            assert np.array_equal(c, want[2].astype(np.int32)) and np.array_equal(ch, want[3].astype(np.int32)), n
    want = vc.model_case(names[0])
    assert np.array_equal(_check_guards(cnt, V), 2 * want[2].astype(np.int32))
    assert np.array_equal(_check_guards(cnt_head, V), 2 * want[3].astype(np.int32))


def test_no_faces_and_no_vertices_leave_minus_one_and_zero(dev):
    v, f, M, H, W, body, hair = vc.case("box-front-48x64")
    full = np.full((H, W), 255, np.uint8)
    for vv, ff in ((v, f[:0]), (v[:0], f), (v[:0], f[:0])):
        pix, visp, cnt, cnt_head = _view_capi(dev, vv, ff, M, H, W, full, np.zeros_like(full))
        assert (pix == -1).all() and not visp.any() and not cnt.any() and not cnt_head.any()
    assert (vis.rasterize_mesh((v[:0], f[:0]), M, H, W, device=dev) == -1).all()
    # H * W == 0: nothing is written
    pix, visp, cnt, cnt_head = _view_capi(dev, v, f, M, 0, 64, None, None)
    assert pix.size == 0 and not cnt.any()
