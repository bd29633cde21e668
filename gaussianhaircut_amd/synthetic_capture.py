"""Synthetic captures: a known groom seen through cameras, as the five arrays a photographed view comes in (csrc/ghr_capture.h;
DESIGN.md 8r) -- the reference's third dataset type, "Synthetic" (``src/scene/dataset_readers.py:306-396``), without Blender.

``capture_view`` gives one view: ``image`` uint8 [H, W, 3] (``render_strands``' picture, byte for byte), ``mask_hair`` and
``mask_body`` uint8 [H, W] (anti-aliased: the covered share of the s x s subsamples; the body is the silhouette and includes the
hair), ``angle`` uint8 [H, W] (degrees 0 ... 179; byte k is the screen direction (sin k deg, cos k deg), x right, y down: the
rasterizer's ``orient_angle`` and the Gabor bank's degree byte) and ``var`` float32 [H, W] (rad^2).  They are exactly the arguments
of ``ground_truth.view_ground_truth``.  One mesh raster, one face depth and one strand raster serve the picture and the maps.
``fused=True`` launches the HIP kernels (ROCm tensors only: there is no CPU path); ``fused=False`` evaluates the PyTorch-composed
comparator on any device: the same float32 expressions in the same operand order.  ``capture_ground_truth`` fills the training
tensors of a list of cameras from a groom.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from . import strand_view as sv
from . import visibility as vis
from .visibility import NEAR

BINS = 180
_SHADOW_KEYS = ("shadow_size", "shadow_half_width", "shadow_layer", "shadow_kappa", "shadow_bias")
_chunk_pixels = 1 << 16   # output pixels per block of the composed form's [pixels, 180] score table


class CaptureView(NamedTuple):
    image: torch.Tensor
    mask_hair: torch.Tensor
    mask_body: torch.Tensor
    angle: torch.Tensor
    var: torch.Tensor


def angle_table() -> np.ndarray:
    """T [180, 2] float32: (cos 2 th_k, sin 2 th_k), th_k = k pi / 180, formed in float64 and rounded once"""
    th = np.arange(BINS, dtype=np.float64) * (np.pi / 180.0)
    return np.ascontiguousarray(np.stack([np.cos(2.0 * th), np.sin(2.0 * th)], axis=1).astype(np.float32))


def _table(dev):
    from .orientation import _on_dev
    return _on_dev(("capture-angle-table",), dev, lambda: torch.from_numpy(angle_table()))


def _check_var_floor(var_floor):
    if not (np.isfinite(var_floor) and var_floor >= 0):
        raise ValueError("synthetic_capture: var_floor must be finite and >= 0")


# ---------------------------------------------------------------------------------------------------------------- composed
def _maps_torch(pts, Ms, H, W, s, Fc, seg, face, near, var_floor):
    """(mask_hair, mask_body, angle, var) of the definition from the index planes [s H, s W] on their device"""
    dev = seg.device
    S, L = pts.shape[0], pts.shape[1]
    K, n = S * (L - 1), s * s
    seg, face = seg.long(), face.long()
    hair = (seg >= 0) & (seg < K)
    head = ~hair & (face >= 0) & (face < Fc)
    zero = torch.zeros((s * H, s * W), dtype=torch.float32, device=dev)
    c2, s2 = zero, zero
    if K and H * W:
        k = torch.where(hair, seg, torch.zeros_like(seg))
        si, ii = k // (L - 1), k % (L - 1)
        m = [float(x) for x in sv._m12(Ms)]
        nr = float(np.float32(near))
        ax, ay, _, va = sv._project_torch(pts[si, ii], m, nr)
        bx, by, _, vb = sv._project_torch(pts[si, ii + 1], m, nr)
        dx, dy = bx - ax, by - ay
        len2 = dx * dx + dy * dy
        c = (dy * dy - dx * dx) / len2
        sn = (2.0 * (dx * dy)) / len2
        ok = hair & va & vb & (len2 > 0) & torch.isfinite(c) & torch.isfinite(sn)
        c2, s2 = torch.where(ok, c, zero), torch.where(ok, sn, zero)   # (+ 0 changes no bit of a sum that starts at + 0)
    C, Sm = torch.zeros((H, W), dtype=torch.float32, device=dev), torch.zeros((H, W), dtype=torch.float32, device=dev)
    for a in range(s):          # the definition's order: a-major, then b; a loop, not a sum
        for b in range(s):
            C = C + c2[a::s, b::s]
            Sm = Sm + s2[a::s, b::s]
    n_hair = hair.reshape(H, s, W, s).sum(dim=(1, 3))
    n_body = n_hair + head.reshape(H, s, W, s).sum(dim=(1, 3))
    mask_hair = ((255 * n_hair + n // 2) // n).to(torch.uint8)
    mask_body = ((255 * n_body + n // 2) // n).to(torch.uint8)
    T = _table(dev) if dev.type == "cuda" else torch.from_numpy(angle_table())
    Cf, Sf = C.reshape(-1), Sm.reshape(-1)
    angle = torch.zeros(H * W, dtype=torch.uint8, device=dev)
    bins = torch.arange(BINS, device=dev)
    for p0 in range(0, H * W, _chunk_pixels):
        sl = slice(p0, min(p0 + _chunk_pixels, H * W))
        score = Cf[sl, None] * T[None, :, 0] + Sf[sl, None] * T[None, :, 1]
        score = torch.where(torch.isnan(score), torch.full_like(score, -np.inf), score)
        top = score.max(dim=1).values
        first = torch.where((score == top[:, None]) & (score > -np.inf), bins[None], BINS).min(dim=1).values   # the lowest among equals
        angle[sl] = torch.where(first == BINS, torch.zeros_like(first), first).to(torch.uint8)
    R = sv._sqrt(C * C + Sm * Sm)
    var = float(np.float32(var_floor)) + 0.5 * torch.fmax(torch.zeros_like(R), 1.0 - sv._div(R, float(n)))
    return mask_hair, mask_body, angle.reshape(H, W), var


# ---------------------------------------------------------------------------------------------------------------- fused
def _maps_fused(pts, Ms, H, W, s, Fc, seg, face, near, var_floor):
    from .diff_gaussian_rasterization import _on_device, _ptr, _stream
    dev = pts.device
    S, L = pts.shape[0], pts.shape[1]
    mask_hair = torch.empty((H, W), dtype=torch.uint8, device=dev)
    mask_body = torch.empty((H, W), dtype=torch.uint8, device=dev)
    angle = torch.empty((H, W), dtype=torch.uint8, device=dev)
    var = torch.empty((H, W), dtype=torch.float32, device=dev)
    T = _table(dev)
    Mc = sv._mc(Ms)
    n = H * W
    with _on_device(dev):
        _lib.check(_lib.lib().ghr_strandview_capture(
            _stream(), S, L, _ptr(pts) if S else None, ctypes.byref(Mc), float(near), H, W, int(s), int(Fc),
            _ptr(seg) if n else None, _ptr(face) if n else None, _ptr(T), float(var_floor),
            _ptr(mask_hair) if n else None, _ptr(mask_body) if n else None, _ptr(angle) if n else None, _ptr(var) if n else None))
    return mask_hair, mask_body, angle, var


# ---------------------------------------------------------------------------------------------------------------- public
@torch.no_grad()
def capture_view(points, view, mesh=None, colors=None, supersample: int = 4, half_width: float = 0.75, head_bias: float = 0.0,
                 near: float = NEAR, var_floor: float = 0.0, shadows=False, fused: bool = True, device=None, **shading) -> CaptureView:
    """One synthetic view of ``points`` [S, L, 3] under ``view`` = (M, H, W) over ``mesh`` (a HeadMesh, (vertices, faces) or None),
    on the device.  ``image`` is ``render_strands(points, view, mesh, colors, supersample=..., shadows=..., **shading)`` in kajiya
    mode, byte for byte (``shading`` also takes that function's ``shadow_*`` keywords).  ``var`` is ``var_floor`` + half of one minus
    the mean resultant length of the doubled angles over the pixel's subsamples: 0 for a pixel filled with parallel strands, 0.5 where
    no strand is seen.  The Gabor bank itself gives about 0.094 rad^2 on ideal stripes: ``var_floor=0.094`` for weights of the range
    that photographs give."""
    dev = vis._device(device, fused)
    if fused and dev.type != "cuda":
        raise RuntimeError("capture_view(fused=True) needs a ROCm device: the kernels have no CPU path (fused=False is the "
                           "PyTorch form)")
    sv._check_scalars(half_width, head_bias)
    _check_var_floor(var_floor)
    shadow_kw = {k: shading.pop(k) for k in _SHADOW_KEYS if k in shading}
    M, H, W = view
    H, W, s = int(H), int(W), int(supersample)
    Ms, rs = sv.supersampled(M, half_width, s)
    pts = sv._points(points, dev)
    base = None
    if colors is not None:
        c = colors.detach().cpu().numpy() if isinstance(colors, torch.Tensor) else np.asarray(colors)
        c = np.array(c, np.float32)
        if c.size == 3:
            shading = dict(shading, hair_rgb=c.reshape(3))
        else:
            assert c.shape == (pts.shape[0], 3), (c.shape, tuple(pts.shape))
            base = torch.from_numpy(c).to(dev).contiguous()
    sh = sv.shading_for_view(M, **shading)
    v, f32 = sv._mesh_tensors(mesh, dev)
    Fc = int(f32.shape[0]) if f32 is not None else 0
    shadow, kappa, bias = None, shadow_kw.get("shadow_kappa", sv.SHADOW_KAPPA), shadow_kw.get("shadow_bias", sv.SHADOW_BIAS)
    if shadows is not False and shadows is not None:
        if isinstance(shadows, sv.ShadowMap):
            shadow = shadows
            sv._check_shadow_scalars(1.0, shadow.layer, kappa, bias)
            if shadow.q0.device != dev:
                raise ValueError("capture_view: the ShadowMap is on %s, the picture on %s" % (shadow.q0.device, dev))
        else:
            Ml, Hl, Wl, rho = sv.light_view(pts, None if v is None else (v, f32), light=sh["light"],
                                            size=shadow_kw.get("shadow_size", sv.SHADOW_SIZE))
            layer = shadow_kw.get("shadow_layer")
            layer = rho / sv.SHADOW_LAYERS_PER_RADIUS if layer is None else layer
            shw = shadow_kw.get("shadow_half_width", sv.SHADOW_HALF_WIDTH)
            sv._check_shadow_scalars(shw, layer, kappa, bias)
            shadow = sv._shadow_map(pts, v, f32, Ml, Hl, Wl, shw, layer, near, fused)
    seg, t, face, _ = sv._rasterize(pts, v, f32, Ms, s * H, s * W, rs, head_bias, near, fused)
    mode = _lib.STRANDVIEW_KAJIYA
    if fused:
        if shadow is not None:
            big = sv._shade_shadowed_fused(pts, v, f32, s * H, s * W, seg, face, t, mode, sh, base, shadow, kappa, bias)
        else:
            big = sv._shade_fused(pts, v, f32, s * H, s * W, seg, face, mode, sh, base)
        image = sv._resolve_fused(big, H, W, s)
        maps = _maps_fused(pts, Ms, H, W, s, Fc, seg, face, near, var_floor)
    else:
        big = sv._shade_torch(pts, v, None if f32 is None else f32.long(), s * H, s * W, seg, face, mode, sh, base, t=t, shadow=shadow,
                              kappa=kappa, bias=bias)
        image = sv._resolve_torch(big, H, W, s)
        maps = _maps_torch(pts, Ms, H, W, s, Fc, seg, face, near, var_floor)
    return CaptureView(image, *maps)


@torch.no_grad()
def capture_ground_truth(points, cams, mesh=None, colors=None, supersample: int = 4, half_width: float = 0.75, head_bias: float = 0.0,
                         near: float = NEAR, var_floor: float = 0.0, shadows=False, fused: bool = True, device=None,
                         white_background: bool = False, binarize_masks: bool = False, **shading):
    """Fills ``original_image`` / ``original_mask`` / ``original_orient_angle`` / ``original_orient_conf`` of every camera with the
    capture of ``points`` through it: each camera's view is ``visibility.view_matrix_from_camera``'s, at the camera's own size, and
    the five arrays go through ``ground_truth.attach_ground_truth`` on the device they were made on -- nothing through the host.
    Returns the cameras."""
    from . import ground_truth as gt
    dev = vis._device(device, fused)
    pts = sv._points(points, dev)
    mesh_dev = None if mesh is None else sv._mesh_tensors(mesh, dev)   # uploaded once for all views
    for cam in cams:
        cv = capture_view(pts, vis.view_matrix_from_camera(cam), mesh=mesh_dev, colors=colors, supersample=supersample,
                          half_width=half_width, head_bias=head_bias, near=near, var_floor=var_floor, shadows=shadows, fused=fused,
                          device=dev, **shading)
        gt.attach_ground_truth([cam], [tuple(cv)], white_background=white_background, binarize_masks=binarize_masks)
    return list(cams)
