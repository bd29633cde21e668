"""Self-shadowing of the strand preview on the device (csrc/ghr_strandview.h "Self-shadowing"), through the C ABI and
the Python API.

Every result is an integer, a byte or a float32 compared by its bits, no texel or pixel left out: ghr_strandview_opacity and
ghr_strandview_shade_shadowed against the numpy float32 model of the definition (tests/strand_shadow_cases.py, brute force over all
segments) and against the PyTorch-composed form evaluated on the device.  Outputs land in poisoned buffers between guards."""
import ctypes

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd import strand_view as sv
from tests import strand_shadow_cases as ss
from tests import strand_view_cases as sc
from tests.test_gpu_strand_view import GUARD, POISON, _check_guards, _guarded, _ptr, _same_bits, _stream, _up

pytestmark = pytest.mark.gpu
MAPS, FRAMES = ss.MAPS, ss.FRAMES


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _opacity_capi(dev, c, ws=None):
    """one light pass through the entry: (q0 float32 [Hl, Wl], layers uint32 [Hl, Wl, 4]) from poisoned buffers between guards"""
    Hl, Wl = c["Hl"], c["Wl"]
    N = Hl * Wl
    S, Lp = c["points"].shape[:2]
    pts = _up(c["points"], dev)
    if ws is None:
        ws = torch.full((sv.strandview_workspace_bytes(S, Lp, Hl, Wl),), POISON, dtype=torch.uint8, device=dev)
    Mc = (ctypes.c_float * 12)(*[float(x) for x in c["Ml"]])
    q0, layers = _guarded(N, torch.float32, dev), _guarded(4 * N, torch.int32, dev)
    assert layers[GUARD:].data_ptr() % 16 == 0
    _lib.check(_lib.lib().ghr_strandview_opacity(_stream(), S, Lp, _ptr(pts) if S else None, ctypes.byref(Mc), float(sc.NEAR), Hl, Wl,
                                                 float(c["rl"]), float(c["layer"]), _ptr(ws), ws.numel(), _ptr(q0[GUARD:]),
                                                 _ptr(layers[GUARD:])))
    torch.cuda.synchronize()
    return _check_guards(q0, N, True).reshape(Hl, Wl), _check_guards(layers, 4 * N).view(np.uint32).reshape(Hl, Wl, 4)


@pytest.mark.parametrize("name", MAPS)
def test_opacity_equals_the_model_exactly_and_twice(dev, name):
    """every map into poisoned buffers between guards, the workspace poisoned too; a second run gives the same bits"""
    c = ss.light_map(name)
    q0, layers = _opacity_capi(dev, c)
    assert _same_bits(q0, c["q0"]) and _same_bits(layers, c["layers"]), name
    q0b, layersb = _opacity_capi(dev, c)
    assert _same_bits(q0, q0b) and _same_bits(layers, layersb), name


def _shade_capi(dev, c):
    """ghr_strandview_shade_shadowed on the model's planes and the model's map: the bytes on the s-times finer grid"""
    H, W = c["rgb"].shape[:2]
    N = H * W
    S, Lp = c["points"].shape[:2]
    has_mesh = c["v"] is not None
    V, F = (len(c["v"]), len(c["f"])) if has_mesh else (0, 0)
    pts, vd, fd, base = _up(c["points"], dev), _up(c["v"], dev), _up(c["f"], dev), _up(c["base"], dev)
    seg, t, face = (_up(a, dev) for a in c["planes"])
    sm = c["sm"]
    shadow = sv.ShadowMap(sm["Ml"], sm["Hl"], sm["Wl"], float(sc.NEAR), _up(sm["q0"], dev), _up(sm["layers"].view(np.int32), dev),
                          _up(sm["qfl"], dev), float(sm["layer"]))
    sd, st = sv._shadow_struct(shadow, c["kappa"], c["bias"]), sv._shading_struct(c["sh"])
    rgb = _guarded(3 * N, torch.uint8, dev)
    _lib.check(_lib.lib().ghr_strandview_shade_shadowed(_stream(), S, Lp, _ptr(pts) if S else None, V, _ptr(vd), F, _ptr(fd), H, W,
                                                        _ptr(seg), _ptr(face), _ptr(t), c["mode"], ctypes.byref(st), _ptr(base),
                                                        ctypes.byref(sd), _ptr(rgb[GUARD:])))
    torch.cuda.synchronize()
    return _check_guards(rgb, 3 * N).reshape(H, W, 3), shadow


@pytest.mark.parametrize("name", FRAMES)
def test_shade_shadowed_equals_the_model_per_pixel(dev, name):
    """the frames meet every branch of the lookup on strand and on head pixels, with qfl and without (asserted on the model)"""
    c = ss.frame(name)
    rgb, shadow = _shade_capi(dev, c)
    assert _same_bits(rgb, c["rgb"]), name
    if name == "sphere-48x64-ss2":
        assert {0, 1, 2, 3, 4} <= c["branches"] and {10, 11, 14} <= c["branches"] and c["sm"]["qfl"] is not None
    if name == "sphere-48x64-noqfl":
        assert {0, 1, 2, 3} <= c["branches"] and {10, 11, 12, 13} <= c["branches"] and c["sm"]["qfl"] is None
    # and through the Python API, fused and composed, on the same map
    view = (c["M"], c["H"], c["W"])
    kw = dict(mesh=None if c["v"] is None else (c["v"], c["f"]), colors=c["base"], mode=("kajiya", "tangent")[c["mode"]],
              supersample=c["s"], half_width=c["r"], near=float(sc.NEAR), eye=c["sh"]["eye"], light=c["sh"]["light"],
              shadow_kappa=c["kappa"], shadow_bias=c["bias"], shadows=shadow, device=dev)
    pic = sv.render_strands(c["points"], view, fused=True, **kw)
    assert _same_bits(pic.cpu().numpy(), c["picture"]), name
    assert torch.equal(pic, sv.render_strands(c["points"], view, fused=False, **kw)), name


def test_render_strands_with_shadows_fused_equals_composed(dev):
    """a 48 x 64 camera, a 17 x 33 light map made by the call itself, supersample 2, the sphere mesh"""
    c = sc.case("hair-front-48x64")
    view = (c["M"], 48, 64)
    kw = dict(mesh=(c["v"], c["f"]), supersample=2, shadows=True, shadow_size=(17, 33), device=dev)
    fused = sv.render_strands(c["points"], view, fused=True, **kw)
    composed = sv.render_strands(c["points"], view, fused=False, **kw)
    assert fused.is_cuda and fused.dtype == torch.uint8 and torch.equal(fused, composed)
    plain = sv.render_strands(c["points"], view, mesh=(c["v"], c["f"]), supersample=2, device=dev)
    assert (fused <= plain).all() and (fused < plain).any(dim=2).float().mean() > 0.05
    # the map itself, fused against composed and the model
    Ml, Hl, Wl, rho = sv.light_view(c["points"], (c["v"], c["f"]), view=c["M"], size=(17, 33))
    a = sv.strand_shadow_map(c["points"], Ml, Hl, Wl, mesh=(c["v"], c["f"]), device=dev)
    b = sv.strand_shadow_map(c["points"], Ml, Hl, Wl, mesh=(c["v"], c["f"]), fused=False, device=dev)
    assert torch.equal(a.q0, b.q0) and torch.equal(a.layers, b.layers) and torch.equal(a.qfl, b.qfl) and a.layer == b.layer
    q0, layers = ss.model_opacity(c["points"], Ml.reshape(12), Hl, Wl, 1.0, rho / 32)
    assert _same_bits(a.q0.cpu().numpy(), q0) and _same_bits(a.layers.cpu().numpy().view(np.uint32), layers) and layers.any()


def test_a_map_that_sees_nothing_gives_the_unshadowed_bytes(dev):
    """Tr == 1 at every pixel: ghr_strandview_shade_shadowed's bytes are ghr_strandview_shade's"""
    from tests.visibility_cases import _M, _look_at, _pinhole
    c = sc.case("hair-front-48x64")
    view = (c["M"], 48, 64)
    kw = dict(mesh=(c["v"], c["f"]), supersample=2, device=dev)
    Ml = _M(_pinhole(24, 24), *_look_at((50.0, 0.0, 0.0), (100.0, 0.0, 0.0)))
    sm = sv.strand_shadow_map(c["points"], Ml, 24, 24, mesh=(c["v"], c["f"]), layer=0.05, device=dev)
    assert not sm.q0.any() and not sm.layers.any() and not sm.qfl.any()
    plain = sv.render_strands(c["points"], view, **kw)
    assert torch.equal(sv.render_strands(c["points"], view, shadows=sm, **kw), plain)
    assert torch.equal(sv.render_strands(c["points"], view, shadows=False, **kw), plain)
    empty = sv.strand_shadow_map(c["points"], Ml, 0, 24, device=dev)               # Hl * Wl == 0: nothing is written, nothing read
    assert empty.q0.numel() == 0 and torch.equal(sv.render_strands(c["points"], view, shadows=empty, **kw), plain)
    none = sv.strand_shadow_map(c["points"][:0], sc.view_oblique(17, 33), 17, 33, device=dev)     # S == 0
    assert not none.q0.any() and not none.layers.any() and none.qfl is None


def test_workspace_reused_across_light_views_of_different_content(dev):
    """one poisoned workspace, sized for the largest, serves maps of other strands, sizes and views in turn"""
    names = ("hair-L100-40x48", "stack257", "long-80x96", "ladder0", "dups129", "hair-sphere-17x33", "hair-L100-40x48")
    need = 0
    for n in names:
        c = ss.light_map(n)
        need = max(need, sv.strandview_workspace_bytes(c["points"].shape[0], c["points"].shape[1], c["Hl"], c["Wl"]))
    ws = torch.full((need,), POISON, dtype=torch.uint8, device=dev)
    for n in names:
        c = ss.light_map(n)
        q0, layers = _opacity_capi(dev, c, ws=ws)
        assert _same_bits(q0, c["q0"]) and _same_bits(layers, c["layers"]), n
    # the Python API keeps the light pass's buffers along a path
    c = ss.light_map("hair-sphere-17x33")
    a = sv.strand_shadow_map(c["points"], c["Ml"], 17, 33, mesh=(c["v"], c["f"]), half_width=c["rl"], layer=c["layer"], device=dev)
    frames, addr = sv._light_frames, sv._light_frames.ws.data_ptr()
    b = sv.strand_shadow_map(c["points"], sc.view_front(17, 33), 17, 33, mesh=(c["v"], c["f"]), half_width=c["rl"], layer=c["layer"],
                             device=dev)
    assert sv._light_frames is frames and frames.ws.data_ptr() == addr and not torch.equal(a.q0, b.q0)
    assert _same_bits(a.q0.cpu().numpy(), c["q0"]) and _same_bits(a.qfl.cpu().numpy(), c["qfl"])      # a's planes are its own


def test_two_thousand_strands_over_the_sphere_against_the_composed_form(dev):
    """2 000 x 100 points over the 9976-face sphere, a 256 x 256 light map and a 270 x 480 camera: the map and every byte of the
    picture equal to the composed form's"""
    H, W = 270, 480
    pts = sc.hair(2000, 100, 21)
    mesh = sc.meshes()["sphere"]
    M = sc.view_front(H, W)
    Ml, Hl, Wl, rho = sv.light_view(pts, mesh, view=M, size=256)
    a = sv.strand_shadow_map(pts, Ml, Hl, Wl, mesh=mesh, device=dev)
    b = sv.strand_shadow_map(pts, Ml, Hl, Wl, mesh=mesh, fused=False, device=dev)
    assert torch.equal(a.q0, b.q0) and torch.equal(a.layers, b.layers) and torch.equal(a.qfl, b.qfl)
    lay = a.layers.cpu().numpy()
    assert (a.q0 > 0).float().mean() > 0.3 and (lay.sum((0, 1)) > 1000).all() and lay.sum(2).max() > 20
    kw = dict(mesh=mesh, supersample=1, shadows=a, device=dev)
    pic = sv.render_strands(pts, (M, H, W), fused=True, **kw)
    assert torch.equal(pic, sv.render_strands(pts, (M, H, W), fused=False, **kw))
    plain = sv.render_strands(pts, (M, H, W), mesh=mesh, supersample=1, device=dev)
    assert (pic <= plain).all() and (pic < plain).any(dim=2).float().mean() > 0.1
