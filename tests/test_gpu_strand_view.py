"""The strand preview on the device (csrc/ghr_strandview.h), through the C ABI and the Python API.

Every result is an integer, a byte or a float32 compared by its bits, no pixel left out: ghr_strandview_face_depth, _raster,
_shade and _resolve against the numpy float32 model of the definition (tests/strand_view_cases.py, brute force over all
segments) and against the PyTorch-composed form evaluated on the device.  Outputs land in poisoned buffers between guards."""
import ctypes

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd import strand_view as sv
from tests import strand_view_cases as sc

pytestmark = pytest.mark.gpu
CASES = sc.CASES
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
    """n elements of `dtype` between two guards, every byte 0xA5 (a float plane is handed out as a view of int32 words)"""
    if dtype == torch.uint8:
        return torch.full((n + 2 * GUARD,), POISON, dtype=torch.uint8, device=dev)
    return torch.full((n + 2 * GUARD,), POISON32, dtype=torch.int32, device=dev)


def _check_guards(t, n, as_float=False):
    a = t.cpu().numpy()
    fill = POISON if a.dtype == np.uint8 else POISON32
    assert (a[:GUARD] == fill).all() and (a[GUARD + n:] == fill).all()
    body = a[GUARD:GUARD + n]
    return body.view(np.float32) if as_float else body


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _up(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)


def _frame_capi(dev, c, m, ws=None):
    """one frame on the grid of model frame m through the four entries: (four planes, qf, rgb, the resolved picture)"""
    L = _lib.lib()
    H, W, s = m["H"], m["W"], c["s"]
    N = H * W
    pts = _up(c["points"], dev)
    S, Lp = c["points"].shape[:2]
    has_mesh = c["v"] is not None
    V, F = (len(c["v"]), len(c["f"])) if has_mesh else (0, 0)
    vd, fd, pix = (_up(c["v"], dev), _up(c["f"], dev), _up(m["pix"], dev)) if has_mesh else (None, None, None)
    base = _up(c["base"], dev)
    Mc = (ctypes.c_float * 12)(*[float(x) for x in m["M"]])
    if ws is None:
        ws = torch.full((sv.strandview_workspace_bytes(S, Lp, H, W),), POISON, dtype=torch.uint8, device=dev)
    qf = None
    if has_mesh:
        qf = _guarded(N, torch.float32, dev)
        _lib.check(L.ghr_strandview_face_depth(_stream(), V, _ptr(vd), F, _ptr(fd), ctypes.byref(Mc), float(sc.NEAR), H, W, _ptr(pix),
                                               _ptr(qf[GUARD:])))
    seg, t, face, inv = (_guarded(N, torch.int32, dev) for _ in range(4))
    _lib.check(L.ghr_strandview_raster(_stream(), S, Lp, _ptr(pts) if S else None, ctypes.byref(Mc), float(sc.NEAR), H, W, m["r"],
                                       float(np.float32(c["bias"])), _ptr(pix), _ptr(qf[GUARD:]) if has_mesh else None, _ptr(ws),
                                       _ptr(seg[GUARD:]), _ptr(t[GUARD:]), _ptr(face[GUARD:]), _ptr(inv[GUARD:])))
    rgb = _guarded(3 * N, torch.uint8, dev)
    st = sv._shading_struct(c["sh"])
    _lib.check(L.ghr_strandview_shade(_stream(), S, Lp, _ptr(pts) if S else None, V, _ptr(vd), F, _ptr(fd), H, W, _ptr(seg[GUARD:]),
                                      _ptr(face[GUARD:]), c["mode"], ctypes.byref(st), _ptr(base), _ptr(rgb[GUARD:])))
    small = _guarded(3 * c["H"] * c["W"], torch.uint8, dev)
    _lib.check(L.ghr_strandview_resolve(_stream(), c["H"], c["W"], s, _ptr(rgb[GUARD:]), _ptr(small[GUARD:])))
    torch.cuda.synchronize()
    planes = (_check_guards(seg, N).reshape(H, W), _check_guards(t, N, True).reshape(H, W), _check_guards(face, N).reshape(H, W),
              _check_guards(inv, N, True).reshape(H, W))
    return (planes, _check_guards(qf, N, True).reshape(H, W) if has_mesh else None, _check_guards(rgb, 3 * N).reshape(H, W, 3),
            _check_guards(small, 3 * c["H"] * c["W"]).reshape(c["H"], c["W"], 3))


def _assert_frame(got, m, picture, name):
    planes, qf, rgb, small = got
    for k, (g, want) in enumerate(zip(planes, m["planes"])):
        assert _same_bits(g, want), (name, k)
    if qf is not None:
        assert _same_bits(qf, m["qf"]), name
    assert _same_bits(rgb, m["rgb"]), name
    assert _same_bits(small, picture), name


def _api_kwargs(c):
    sh = c["sh"]
    colors = c["base"] if c["base"] is not None else (tuple(float(x) for x in sh["base_rgb"]) if c["colors"] == "one" else None)
    return dict(mesh=None if c["v"] is None else (c["v"], c["f"]), colors=colors, mode=("kajiya", "tangent")[c["mode"]],
                supersample=c["s"], half_width=c["r"], head_bias=c["bias"], near=float(sc.NEAR), eye=sh["eye"], light=sh["light"])


@pytest.mark.parametrize("name", CASES)
def test_c_abi_equals_the_model_exactly(dev, name):
    """every case (the supersampled ones on their finer grid) into poisoned buffers between guards, the workspace poisoned too"""
    c = sc.case(name)
    _assert_frame(_frame_capi(dev, c, sc.model_frame(name, c["s"])), sc.model_frame(name, c["s"]), sc.model_picture(name), name)


@pytest.mark.parametrize("name", CASES)
def test_python_api_fused_equals_composed_and_the_model(dev, name):
    c = sc.case(name)
    m = sc.model_frame(name)
    mesh = None if c["v"] is None else (c["v"], c["f"])
    kw = dict(mesh=mesh, half_width=c["r"], head_bias=c["bias"], near=float(sc.NEAR), device=dev)
    fused = sv.rasterize_strands(c["points"], c["M"], c["H"], c["W"], fused=True, **kw)
    composed = sv.rasterize_strands(c["points"], c["M"], c["H"], c["W"], fused=False, **kw)
    for k, (a, b, want) in enumerate(zip(fused, composed, m["planes"])):
        assert a.dtype == b.dtype and _same_bits(a.cpu().numpy(), b.cpu().numpy()), (name, k)
        assert _same_bits(a.cpu().numpy(), want), (name, k)
    view = (c["M"], c["H"], c["W"])
    pic = sv.render_strands(c["points"], view, fused=True, device=dev, **_api_kwargs(c))
    pic_t = sv.render_strands(c["points"], view, fused=False, device=dev, **_api_kwargs(c))
    assert pic.dtype == torch.uint8 and pic.is_cuda and torch.equal(pic, pic_t)
    assert _same_bits(pic.cpu().numpy(), sc.model_picture(name))       # the supersampled cases at their own s


def test_workspace_reused_across_views_of_different_content(dev):
    """one poisoned workspace, sized for the largest, serves frames of other strands, sizes and views in turn"""
    names = ("hair-front-130x250", "stack257", "long-130x250", "hair-front-1x1", "dups129", "hair-oblique-130x250", "hair-front-130x250")
    need = 0
    for n in names:
        c = sc.case(n)
        need = max(need, sv.strandview_workspace_bytes(c["points"].shape[0], c["points"].shape[1], c["H"], c["W"]))
    ws = torch.full((need,), POISON, dtype=torch.uint8, device=dev)
    for n in names:
        _assert_frame(_frame_capi(dev, sc.case(n), sc.model_frame(n), ws=ws), sc.model_frame(n), sc.model_picture(n), n)


def test_api_reuses_its_buffers_along_a_path(dev):
    """two views of one groom through the Python API: the device buffers are allocated once"""
    c = sc.case("hair-front-48x64")
    mesh = (c["v"], c["f"])
    a = sv.rasterize_strands(c["points"], sc.view_front(48, 64), 48, 64, mesh=mesh, device=dev)
    frames = sv._frames
    addr = frames.ws.data_ptr()
    b = sv.rasterize_strands(c["points"], sc.view_oblique(48, 64), 48, 64, mesh=mesh, device=dev)
    assert sv._frames is frames and frames.ws.data_ptr() == addr
    b2 = sv.rasterize_strands(c["points"], sc.view_oblique(48, 64), 48, 64, mesh=mesh, fused=False, device=dev)
    a2 = sv.rasterize_strands(c["points"], sc.view_front(48, 64), 48, 64, mesh=mesh, device=dev)
    assert not torch.equal(a[0], b[0])
    assert all(torch.equal(x, y) for x, y in zip(b, b2)) and all(_same_bits(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(a, a2))


def test_empty_inputs_leave_background(dev):
    c = sc.case("hair-front-48x64")
    white = np.full((48, 64, 3), 255, np.uint8)
    pic = sv.render_strands(c["points"][:0], (c["M"], 48, 64), device=dev)
    assert np.array_equal(pic.cpu().numpy(), white)
    planes = sv.rasterize_strands(c["points"][:0], c["M"], 48, 64, mesh=(c["v"], c["f"][:0]), device=dev)
    assert (planes[0] == -1).all() and (planes[2] == -1).all() and not planes[1].any() and not planes[3].any()
    planes = sv.rasterize_strands(c["points"], c["M"], 0, 64, device=dev)           # H * W == 0: nothing is written
    assert all(p.numel() == 0 for p in planes)
    assert sv.render_strands(c["points"], (c["M"], 0, 64), device=dev).numel() == 0


def test_two_thousand_strands_over_the_sphere_against_the_composed_form(dev):
    """2 000 x 100 points at 270 x 480 over the 9976-face sphere: every plane and every byte equal to the composed form's"""
    H, W = 270, 480
    pts = sc.hair(2000, 100, 21)
    mesh = sc.meshes()["sphere"]
    M = sc.view_front(H, W)
    kw = dict(mesh=mesh, half_width=0.75, head_bias=0.0, device=dev)
    fused = sv.rasterize_strands(pts, M, H, W, fused=True, **kw)
    composed = sv.rasterize_strands(pts, M, H, W, fused=False, **kw)
    for k, (a, b) in enumerate(zip(fused, composed)):
        assert _same_bits(a.cpu().numpy(), b.cpu().numpy()), k
    seg, face = fused[0].cpu().numpy(), fused[2].cpu().numpy()
    assert (seg >= 0).mean() > 0.1 and (face >= 0).any() and len(np.unique(seg)) > 5000
    pic = sv.render_strands(pts, (M, H, W), supersample=1, fused=True, **kw)
    pic_t = sv.render_strands(pts, (M, H, W), supersample=1, fused=False, **kw)
    assert torch.equal(pic, pic_t) and len(np.unique(pic.cpu().numpy().reshape(-1, 3), axis=0)) > 100
