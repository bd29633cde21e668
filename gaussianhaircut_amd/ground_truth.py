"""The ground-truth loader: a view's four training tensors from its image, masks and orientation maps, at the training resolution.

What the reference does in two places, both by resampling 8-bit images with Pillow's bicubic filter:

* ``src/preprocessing/resize_images.py:101-106`` -- every image and both masks to ``// 2`` and ``// 4`` (``resize_pyramid``,
  ``frame_is_skipped`` for its face / hair test);
* ``src/utils/camera_utils.py:29-84`` (``loadCam``) and ``src/scene/cameras.py:51-64`` -- the ``-r 1 | 2 | 4 | 8 | <width>`` rule
  (``training_resolution``), ``PILtoTorch``'s ``Image.resize`` with its default filter, ``/ 255`` and ``/ 180``, the variance map
  through ``F.interpolate(mode='bilinear')``, ``conf = 1 / ((v / pi^2)^2 + 1e-7)``, ``binarize_masks``, the clamps,
  ``original_mask = cat[hair, body]`` and ``original_image = image * body + white_background * (1 - body)``
  (``view_ground_truth``, ``attach_ground_truth``).

Pillow's 8-bit resampling is fixed-point integer arithmetic: ``resample_coefficients`` computes the per-axis windows and weights
in float64 exactly as Pillow does, and the rest is integer work -- the kernels of ``csrc/ghr_gt.h`` on a ROCm tensor
(``fused=None`` / ``True``), or the same arithmetic composed from torch integer operations (``fused=False``, the comparator,
CPU and device).  Both give Pillow's bytes.  numpy in, numpy out; tensor in, tensor out on the tensor's device.

Synthetic ground truth (``--load_synthetic_rgba --load_synthetic_geom``, ``camera_utils.py:51-64``): the strand stages train on
what ``render_gaussians.py`` wrote from the stage-1 model, read back with everything ``/ 255`` and the confidence plane as it is.
``synthetic_view_ground_truth`` is that reader on arrays; ``ground_truth_from_render`` is the whole chain -- render, quantise,
write, read, divide, composite -- from the packed rasterizer output, one launch of ``k_gt_from_render`` at the render's size;
``attach_synthetic_ground_truth`` fills cameras with it.

Not built: RGBA (Pillow premultiplies alpha), other dtypes, other filters, file formats, COLMAP, ``Scene`` and depth.  The module
needs no Pillow.
"""
from __future__ import annotations

import math
from collections import namedtuple
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from . import orientation as ori
from .orientation import _as_tensor, _launch_env, _on_dev, _out, _use_kernels

ViewGroundTruth = namedtuple("ViewGroundTruth", ("original_image", "original_mask", "original_orient_angle", "original_orient_conf",
                                                 "original_mask_hair", "original_mask_body"))
PRECISION_BITS = 22   # GHR_RESAMPLE_BITS
_WARNED = False


# ---- sizes -------------------------------------------------------------------------------------------------------------------------

def training_resolution(orig_w: int, orig_h: int, resolution, resolution_scale: float = 1.0) -> Tuple[int, int]:
    """``loadCam``'s rule, ``(w, h)``: ``round(orig / (resolution_scale * r))`` for r in 1, 2, 4, 8 (Python's rounding: halves go
    to the even neighbour); otherwise ``resolution`` is a width (``-1``: the image's own, capped at 1600 with a notice the first
    time) and both sides are ``int(orig / (orig_w / width * resolution_scale))``."""
    if resolution in (1, 2, 4, 8):
        return round(orig_w / (resolution_scale * resolution)), round(orig_h / (resolution_scale * resolution))
    if resolution == -1:
        if orig_w > 1600:
            global _WARNED
            if not _WARNED:
                print("[ INFO ] Encountered quite large input images (>1.6K pixels width), rescaling to 1.6K.\n "
                      "If this is not desired, please explicitly specify '--resolution/-r' as 1")
                _WARNED = True
            global_down = orig_w / 1600
        else:
            global_down = 1
    else:
        global_down = orig_w / resolution
    scale = float(global_down) * float(resolution_scale)
    return int(orig_w / scale), int(orig_h / scale)


# ---- coefficients -----------------------------------------------------------------------------------------------------------------

def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def resample_coefficients(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for the bicubic filter (support 2, a = -0.5) along one axis:
    ``(bounds int32 [out, 2] = (first source index, taps), coef int32 [out, ksize])``, weights with 22 fractional bits, zero
    past a row's taps.  Float64 throughout, each operation in Pillow's order."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("resample_coefficients: sizes must be >= 1, got %d -> %d" % (in_size, out_size))
    scale = float(in_size) / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)           # (int): towards zero; below zero is clamped anyway
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    n = xmax - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    live = x < n[:, None]
    w = np.where(live, _bicubic((x + xmin[:, None] - center[:, None] + 0.5) * ss), 0.0)
    ww = np.zeros(out_size, np.float64)
    for i in range(ksize):                                                     # Pillow's running sum, taps ascending
        ww = ww + w[:, i]
    w = np.where((ww != 0.0)[:, None], w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    k = np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)   # (int): towards zero
    k = np.where(live, k, 0)
    return np.stack([xmin, n], 1).astype(np.int32), np.ascontiguousarray(k.astype(np.int32))


def _check_bounds(bounds, coef, in_size, what):
    """what the C ABI refuses, on the host's copy"""
    lo, n = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
    if (lo < 0).any() or (n < 0).any() or (n > coef.shape[1]).any() or (lo + n > in_size).any():
        raise ValueError("resize_u8: %s windows leave the input of %d or exceed %d taps" % (what, in_size, coef.shape[1]))


_coef_cache = {}


def _coefficients(in_size, out_size):
    key = (int(in_size), int(out_size))
    if key not in _coef_cache:
        if len(_coef_cache) > 64:
            _coef_cache.clear()
        _coef_cache[key] = resample_coefficients(*key)
    return _coef_cache[key]


# ---- resize ------------------------------------------------------------------------------------------------------------------------

def _check_u8(t, what="resize_u8"):
    if t.dtype != torch.uint8:
        raise ValueError("%s: %s images are not built (uint8 only)" % (what, str(t.dtype).replace("torch.", "")))
    if t.dim() == 3 and t.shape[2] == 4:
        raise ValueError("%s: four channels (RGBA) are not built: Pillow premultiplies alpha there" % what)
    if not (t.dim() == 2 or (t.dim() == 3 and t.shape[2] in (1, 3))):
        raise ValueError("%s: image must be [H,W] or [H,W,3], got %s" % (what, tuple(t.shape)))
    if t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError("%s: empty image %s" % (what, tuple(t.shape)))
    return t.contiguous()


def resample_axis_torch(t: torch.Tensor, axis: int, bounds: np.ndarray, coef: np.ndarray, accumulators: bool = False):
    """One pass of the comparator over ``axis`` (0: vertical, 1: horizontal) of a uint8 [H,W] / [H,W,C] tensor: per tap a gather
    and an int32 multiply-add.  ``accumulators``: the int32 sums before shift and clip (the tests look for saturation there)."""
    _check_bounds(bounds, coef, t.shape[axis], "axis %d" % axis)
    dev = t.device
    lo = torch.from_numpy(bounds[:, 0].astype(np.int64)).to(dev)
    n = torch.from_numpy(bounds[:, 1].astype(np.int64)).to(dev)
    k = torch.from_numpy(coef).to(dev)
    shape = [1] * t.dim()
    shape[axis] = -1
    acc = None
    last = t.shape[axis] - 1
    for i in range(coef.shape[1]):
        live = i < n
        if not bool(live.any()):
            break
        idx = torch.clamp(lo + i, max=last)
        term = t.index_select(axis, idx).to(torch.int32) * torch.where(live, k[:, i], torch.zeros_like(k[:, i])).view(shape)
        acc = term if acc is None else acc + term
    if acc is None:
        out_shape = list(t.shape)
        out_shape[axis] = bounds.shape[0]
        acc = torch.zeros(out_shape, dtype=torch.int32, device=dev)
    acc = acc + (1 << (PRECISION_BITS - 1))
    if accumulators:
        return acc
    return torch.clamp(acc >> PRECISION_BITS, 0, 255).to(torch.uint8)


def _resize_torch(t, w, h):
    H, W = int(t.shape[0]), int(t.shape[1])
    if (W, H) == (w, h):
        return t.clone()
    if W != w:
        t = resample_axis_torch(t, 1, *_coefficients(W, w))
    if H != h:
        t = resample_axis_torch(t, 0, *_coefficients(H, h))
    return t


def resize_u8_fused(t: torch.Tensor, w: int, h: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``ghr_resample_u8`` on the current stream: at most two launches (none at equal sizes: a copy).  ``out``: a contiguous
    uint8 tensor of the result's size to write into (tests)."""
    assert t.is_cuda, "the resize kernels have no CPU path (fused=False is the torch form)"
    H, W = int(t.shape[0]), int(t.shape[1])
    C = 1 if t.dim() == 2 else int(t.shape[2])
    dev = t.device
    guard, _ptr, _stream = _launch_env(t)
    with guard:
        L = _lib.lib()
        if out is None:
            out = torch.empty((h, w) + tuple(t.shape[2:]), dtype=torch.uint8, device=dev)
        assert out.dtype == torch.uint8 and out.numel() == h * w * C and out.is_contiguous() and out.device == dev
        ax = {}
        for name, (a, b) in (("x", (W, w)), ("y", (H, h))):
            if a == b:
                ax[name] = (None, None, 0)
                continue
            bounds, coef = _coefficients(a, b)
            _check_bounds(bounds, coef, a, name)
            # the tensors themselves are kept until the call is made: the cache drops its entries when it is full, and a pointer
            # into a freed block would be handed to the next allocation
            ax[name] = (_on_dev(("resample-bounds", a, b), dev, lambda: torch.from_numpy(bounds)),
                        _on_dev(("resample-coef", a, b), dev, lambda: torch.from_numpy(coef)), int(coef.shape[1]))
        nbytes = int(L.ghr_resample_scratch_bytes(W, H, w, h, C))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        _lib.check(L.ghr_resample_u8(_stream(), W, H, C, _ptr(t), w, h, _ptr(out), _ptr(ax["x"][0]), _ptr(ax["x"][1]), ax["x"][2],
                                     _ptr(ax["y"][0]), _ptr(ax["y"][1]), ax["y"][2], _ptr(scratch) if nbytes else None))
    return out


def _size(size):
    w, h = int(size[0]), int(size[1])
    if w < 1 or h < 1:
        raise ValueError("resize_u8: size must be (w, h) with both >= 1, got %s" % (tuple(size),))
    return w, h


def resize_u8(image, size, fused: Optional[bool] = None, filter: str = "bicubic"):
    """``Image.fromarray(image).resize(size, Image.BICUBIC)`` bit for bit: ``image`` uint8 [H,W] or [H,W,3], numpy or tensor,
    ``size = (w, h)`` as Pillow takes it; the result is of the input's kind.  Horizontal pass first, then vertical, uint8 between
    them, each only where the size differs."""
    if str(filter).lower() != "bicubic":
        raise ValueError("resize_u8: the %s filter is not built (bicubic only)" % filter)
    t, was_numpy = _as_tensor(image)
    t = _check_u8(t)
    w, h = _size(size)
    res = resize_u8_fused(t, w, h) if _use_kernels(t, fused) else _resize_torch(t, w, h)
    return _out(res, was_numpy)


def resize_pyramid(image, mask_hair, mask_body, factors: Sequence[int] = (2, 4), fused: Optional[bool] = None, device=None) -> dict:
    """The six products of resize_images.py: ``{factor: (image, mask_hair, mask_body)}``, each at ``(w // factor, h // factor)`` and
    each resized from the original, not from the previous level.  ``device``: where to compute (every input is uploaded once); the
    results are of the inputs' kind."""
    ins = []
    for a in (image, mask_hair, mask_body):
        t, was_numpy = _as_tensor(a)
        t = _check_u8(t, "resize_pyramid")
        ins.append((t.to(device) if device is not None else t, was_numpy))
    H, W = int(ins[0][0].shape[0]), int(ins[0][0].shape[1])
    for t, _ in ins[1:]:
        if (int(t.shape[0]), int(t.shape[1])) != (H, W):
            raise ValueError("resize_pyramid: a mask of %s for an image of %d x %d" % (tuple(t.shape), H, W))
    out = {}
    for f in factors:
        w, h = _size((W // int(f), H // int(f)))
        out[int(f)] = tuple(_out(resize_u8_fused(t, w, h) if _use_kernels(t, fused) else _resize_torch(t, w, h), was_numpy)
                            for t, was_numpy in ins)
    return out


def frame_is_skipped(mask_hair, mask_body, mask_face) -> bool:
    """resize_images.py:37-42: the frame is dropped when hair and face overlap on more than 0.1 of the body's pixels."""
    hair, body, face = (np.asarray(m.cpu() if isinstance(m, torch.Tensor) else m) for m in (mask_hair, mask_body, mask_face))
    return bool(((hair > 127) * (face > 127)).sum() > (body > 127).sum() * 0.1)


# ---- the variance map ------------------------------------------------------------------------------------------------------------------

def resize_variance(var, size, via_float16: bool = True, fused: Optional[bool] = None):
    """camera_utils.py:67: the variance map (rounded through the float16 of the reference's file unless ``via_float16`` is off) at
    ``size = (w, h)`` through ``F.interpolate(mode='bilinear')``; float32 [h, w].  On a ROCm tensor: the kernels' own sample."""
    t, was_numpy = _as_tensor(var)
    if t.dim() != 2:
        raise ValueError("resize_variance: var must be [H,W], got %s" % (tuple(t.shape),))
    w, h = _size(size)
    t = t.float().contiguous()
    if _use_kernels(t, fused):
        guard, _ptr, _stream = _launch_env(t)
        with guard:
            out = torch.empty((h, w), dtype=torch.float32, device=t.device)
            _lib.check(_lib.lib().ghr_gt_resize_variance(_stream(), w, h, _ptr(t), int(t.shape[1]), int(t.shape[0]), int(bool(via_float16)),
                                                         _ptr(out)))
    else:
        v = t.to(torch.float16).float() if via_float16 else t
        out = F.interpolate(v[None, None], size=(h, w), mode="bilinear")[0, 0]
    return _out(out, was_numpy)


def _conf_torch(v):
    """camera_utils.py:67-68 after the resize, as the host computes it (see orientation.ground_truth_from_maps)"""
    q = v / torch.full_like(v, math.pi ** 2)
    return torch.ones_like(q) / (q * q + 1e-7)


# ---- assembly --------------------------------------------------------------------------------------------------------------------------

def _tables(dev):
    """i / 255 and i / 180 as PILtoTorch divides: a uint8 tensor by a Python float on the host (a device would multiply by the
    reciprocal, one rounding more)"""
    i = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    return (_on_dev(("gt-div255",), dev, lambda: i / 255.0), _on_dev(("gt-div180",), dev, lambda: i / 180.0))


def assemble_fused(image, mask_hair, mask_body, angle=None, var=None, white_background=False, binarize_masks=False, via_float16=True,
                   fill=None):
    """ONE launch of ``k_gt_assemble`` on the current stream from uint8 tensors at the training size (``var`` float32 at its
    own): ``(image [3,H,W], mask [2,H,W], angle [1,H,W] | None, conf [1,H,W] | None)``.  ``fill``: a byte the outputs are
    pre-filled with (tests)."""
    return _assemble_launch(image, mask_hair, mask_body, angle, var, white_background, binarize_masks, via_float16, fill, 180)


def _new_planes(c, H, W, dev, fill):
    t = torch.empty((c, H, W), dtype=torch.float32, device=dev)
    if fill is not None:
        t.view(torch.uint8).fill_(fill)
    return t


def _assemble_launch(image, mask_hair, mask_body, angle, var, white_background, binarize_masks, via_float16, fill, angle_max):
    """``assemble_fused`` with the angle's divisor chosen: 180 for the orientation files, 255 for a rendered ``orients`` image"""
    assert image.is_cuda, "the assembly kernel has no CPU path (fused=False is the torch form)"
    H, W = int(image.shape[0]), int(image.shape[1])
    dev = image.device
    t255, t180 = _tables(dev)
    t_angle = t255 if angle_max == 255 else t180
    guard, _ptr, _stream = _launch_env(image)
    with guard:
        o_img, o_mask = _new_planes(3, H, W, dev, fill), _new_planes(2, H, W, dev, fill)
        o_ang = _new_planes(1, H, W, dev, fill) if angle is not None else None
        o_conf = _new_planes(1, H, W, dev, fill) if var is not None else None
        vw, vh = (int(var.shape[1]), int(var.shape[0])) if var is not None else (0, 0)
        _lib.check(_lib.lib().ghr_gt_assemble(_stream(), W, H, _ptr(image), _ptr(mask_hair), _ptr(mask_body),
                                              _ptr(angle) if angle is not None else None, _ptr(var) if var is not None else None, vw, vh,
                                              _ptr(t255), _ptr(t_angle), int(bool(white_background)), int(bool(binarize_masks)),
                                              int(bool(via_float16)), _ptr(o_img), _ptr(o_mask),
                                              _ptr(o_ang) if angle is not None else None, _ptr(o_conf) if var is not None else None))
    return o_img, o_mask, o_ang, o_conf


def _assemble_torch(image, mask_hair, mask_body, angle, var, white_background, binarize_masks, via_float16, angle_max=180):
    """loadCam's tail and Camera.__init__ in the reference's order of operations"""
    dev = image.device
    t255, t180 = _tables(dev)
    H, W = int(image.shape[0]), int(image.shape[1])
    img = t255[image.long()].permute(2, 0, 1)

    def mask(m):
        v = t255[m.long()][None]
        return (v >= 0.5).float() if binarize_masks else v
    hair, body = mask(mask_hair), mask(mask_body)
    white = 1.0 if white_background else 0.0
    o_img = img.clamp(0.0, 1.0) * body.clamp(0.0, 1.0) + white * (1 - body.clamp(0.0, 1.0))
    o_ang = (t255 if angle_max == 255 else t180)[angle.long()][None].clamp(0.0, 1.0) if angle is not None else None
    o_conf = None
    if var is not None:
        v = var.to(torch.float16).float() if via_float16 else var.float()
        if (int(v.shape[0]), int(v.shape[1])) != (H, W):
            v = F.interpolate(v[None, None], size=(H, W), mode="bilinear")[0, 0]
        o_conf = _conf_torch(v)[None]
    return o_img.contiguous(), torch.cat([hair, body], 0), o_ang, o_conf


def _plane(t, what):
    if t.dim() == 3 and t.shape[2] == 1:
        t = t[:, :, 0]
    if t.dim() == 3 and t.shape[2] == 3:   # PILtoTorch keeps channel 0 of an RGB mask ([:1])
        t = t[:, :, 0]
    if t.dim() != 2:
        raise ValueError("view_ground_truth: %s must be [H,W], got %s" % (what, tuple(t.shape)))
    return t.contiguous()


def _conf_plane(c, dev, what):
    """``orient_confs/*.pth``: float [H,W] or [1,H,W] -> float32 [H,W] on ``dev``"""
    c = _as_tensor(c)[0].to(dev)
    if c.dim() == 3 and c.shape[0] == 1:
        c = c[0]
    if c.dim() != 2 or not c.is_floating_point():
        raise ValueError("%s: orient_conf must be a float [H,W] or [1,H,W], got %s %s" % (what, str(c.dtype).replace("torch.", ""), tuple(c.shape)))
    return c.float().contiguous()


def _fit_conf(conf, w, h, k):
    """camera_utils.py:64: ``F.interpolate(conf, mode='bilinear')`` alone -- at equal size the plane's own values"""
    if (int(conf.shape[1]), int(conf.shape[0])) == (w, h):
        return conf.clone()[None]
    return resize_variance(conf, (w, h), via_float16=False, fused=k)[None]


def view_ground_truth(image, mask_hair, mask_body, angle=None, var=None, resolution=None, white_background: bool = False,
                      binarize_masks: bool = False, via_float16: bool = True, fused: Optional[bool] = None,
                      resolution_scale: float = 1.0, *, orient=None, orient_conf=None) -> ViewGroundTruth:
    """One view's tensors as ``loadCam`` + ``Camera`` build them.  ``image`` uint8 [H,W,3]; ``mask_hair`` / ``mask_body`` uint8
    [H,W]; ``angle`` uint8 [H,W] (degrees 0 ... 179) and ``var`` [vh,vw] the two orientation files -- when either is absent both are
    computed from ``image`` at its own size (orientation.dog_fused / gabor_fused), then resized like files would be.
    ``resolution``: None (the image's size), ``(w, h)``, or loadCam's ``-r`` (1 | 2 | 4 | 8 | a width | -1).  Everything that
    differs from the training size is resized (Pillow's bicubic for the bytes, bilinear for the variance), then assembled: on a
    ROCm tensor at most two launches per resized input and one for the assembly.  numpy in, numpy out.
    ``orient`` uint8 [H,W] and ``orient_conf`` float [H,W] instead of ``angle`` / ``var``: ``load_synthetic_geom`` on a
    photograph -- the rendered ``orients`` image ``/ 255`` and the rendered confidence through the bilinear resize alone."""
    t, was_numpy = _as_tensor(image)
    t = _check_u8(t, "view_ground_truth")
    if t.dim() != 3 or t.shape[2] != 3:
        raise ValueError("view_ground_truth: image must be [H,W,3], got %s" % (tuple(t.shape),))
    synth = orient is not None or orient_conf is not None
    if synth and (orient is None or orient_conf is None):
        raise ValueError("view_ground_truth: orient and orient_conf come together")
    if synth and (angle is not None or var is not None):
        raise ValueError("view_ground_truth: give angle / var (the orientation files) or orient / orient_conf (rendered), not both")
    dev = t.device
    H0, W0 = int(t.shape[0]), int(t.shape[1])
    if resolution is None:
        w, h = W0, H0
    elif isinstance(resolution, (tuple, list)):
        w, h = _size(resolution)
    else:
        w, h = _size(training_resolution(W0, H0, resolution, resolution_scale))
    k = _use_kernels(t, fused)
    planes = []
    for m, what in ((mask_hair, "mask_hair"), (mask_body, "mask_body")):
        planes.append(_plane(_check_u8(_as_tensor(m)[0].to(dev), "view_ground_truth"), what))
    conf_t = None
    if synth:
        ang_t = _plane(_check_u8(_as_tensor(orient)[0].to(dev), "view_ground_truth"), "orient")
        conf_t, var_t = _conf_plane(orient_conf, dev, "view_ground_truth"), None
    elif angle is None or var is None:
        if k:
            deg, v = ori.gabor_fused(ori.dog_fused(t))
        else:
            bw, bth = ori._bank(None)
            deg, v = ori._gabor_torch(ori._dog_torch(t, ori.DOG_LOW, ori.DOG_HIGH), bw, bth)
        ang_t, var_t = deg, v
    else:
        ang_t = _plane(_check_u8(_as_tensor(angle)[0].to(dev), "view_ground_truth"), "angle")
        var_t = _as_tensor(var)[0].to(dev)
        if var_t.dim() != 2:
            raise ValueError("view_ground_truth: var must be [H,W], got %s" % (tuple(var_t.shape),))
        var_t = var_t.float().contiguous()

    def fit(x):
        if (int(x.shape[1]), int(x.shape[0])) == (w, h):
            return x
        return resize_u8_fused(x, w, h) if k else _resize_torch(x, w, h)
    img, hair, body, ang = fit(t), fit(planes[0]), fit(planes[1]), fit(ang_t)
    if k:
        o_img, o_mask, o_ang, o_conf = _assemble_launch(img, hair, body, ang, var_t, white_background, binarize_masks, via_float16, None,
                                                        255 if synth else 180)
    else:
        o_img, o_mask, o_ang, o_conf = _assemble_torch(img, hair, body, ang, var_t, white_background, binarize_masks, via_float16,
                                                       255 if synth else 180)
    if synth:
        o_conf = _fit_conf(conf_t, w, h, k)
    res = (o_img, o_mask, o_ang, o_conf, o_mask[0:1], o_mask[1:2])
    return ViewGroundTruth(*(_out(x, was_numpy) for x in res))


def attach_ground_truth(cams: Sequence, views: Sequence, resolution=None, white_background: bool = False, binarize_masks: bool = False,
                        via_float16: bool = True, fused: Optional[bool] = None, resolution_scale: float = 1.0) -> List:
    """Fills ``original_image`` / ``original_mask`` / ``original_orient_angle`` / ``original_orient_conf`` of every camera
    (``Camera``, ``BankCamera``) from its view: a dict (or tuple, in this order) of ``image``, ``mask_hair``, ``mask_body`` and
    optionally ``angle``, ``var``.  The result's size must be the camera's ``(image_height, image_width)``."""
    if len(cams) != len(views):
        raise ValueError("attach_ground_truth: %d cameras, %d views" % (len(cams), len(views)))
    for cam, view in zip(cams, views):
        if not isinstance(view, dict):
            view = dict(zip(("image", "mask_hair", "mask_body", "angle", "var"), view))
        gt = view_ground_truth(view["image"], view["mask_hair"], view["mask_body"], view.get("angle"), view.get("var"),
                               resolution=resolution, white_background=white_background, binarize_masks=binarize_masks,
                               via_float16=via_float16, fused=fused, resolution_scale=resolution_scale)
        got = tuple(gt.original_image.shape[1:])
        if got != (cam.image_height, cam.image_width):
            raise ValueError("attach_ground_truth: ground truth of %d x %d (h x w) for a %d x %d camera" % (got + (cam.image_height, cam.image_width)))
        as_t = lambda x: torch.from_numpy(x) if isinstance(x, np.ndarray) else x   # noqa: E731
        cam.original_image, cam.original_mask = as_t(gt.original_image), as_t(gt.original_mask)
        cam.original_orient_angle, cam.original_orient_conf = as_t(gt.original_orient_angle), as_t(gt.original_orient_conf)
    return list(cams)


# ---- synthetic ground truth ------------------------------------------------------------------------------------------------------------

def synthetic_view_ground_truth(render, head_mask, hair_mask, orient=None, orient_conf=None, angle=None, var=None, size=None,
                                white_background: bool = False, binarize_masks: bool = False, fused: Optional[bool] = None) -> ViewGroundTruth:
    """``loadCam`` with ``load_synthetic_rgba`` on the arrays of ``<model>/train_cropped/ours_<it>/``: ``render`` uint8 [H,W,3]
    (``renders``), ``head_mask`` / ``hair_mask`` uint8 [H,W] or [H,W,3] (``head_masks``, ``hair_masks``; channel 0 is used).
    With ``orient`` uint8 (``orients``) and ``orient_conf`` float [H,W] or [1,H,W] (``orient_confs``) it is ``load_synthetic_geom``
    too: the angle is ``orient / 255`` and the confidence the plane itself, through ``F.interpolate(mode='bilinear')`` alone.  With
    ``angle`` and ``var`` instead (the orientation files of the photograph) it is ``load_synthetic_rgba`` alone: ``/ 180``,
    float16, ``1 / ((v / pi^2)^2 + 1e-7)``.  ``size``: None (the render's) or the ``(w, h)`` the caller got from
    ``training_resolution`` on the ORIGINAL photograph's size, as loadCam does; everything else is resized.  numpy in, numpy out."""
    geom, files = (orient is not None, orient_conf is not None), (angle is not None, var is not None)
    if geom[0] != geom[1] or files[0] != files[1]:
        raise ValueError("synthetic_view_ground_truth: orient comes with orient_conf, angle with var")
    if geom[0] == files[0]:
        raise ValueError("synthetic_view_ground_truth: give orient / orient_conf (load_synthetic_geom) or angle / var (the "
                         "orientation files), one pair")
    resolution = None if size is None else _size(size)
    if geom[0]:
        return view_ground_truth(render, hair_mask, head_mask, resolution=resolution, white_background=white_background,
                                 binarize_masks=binarize_masks, fused=fused, orient=orient, orient_conf=orient_conf)
    return view_ground_truth(render, hair_mask, head_mask, angle, var, resolution=resolution, white_background=white_background,
                             binarize_masks=binarize_masks, via_float16=True, fused=fused)


def _core_products_torch(packed):
    """The five products the synthetic branch reads, as ``evaluation.products_torch`` forms and quantises them, kept on ``packed``'s
    device: uint8 render [H,W,3], hair, head, orient [H,W] and float32 conf [H,W]"""
    from .evaluation import quantise8
    from .gaussian_renderer import orient_angle_from
    image, hair, head, conf = packed[0:3], packed[3:4], packed[4:5], packed[8:9]
    angle = orient_angle_from(packed[5:8])
    return (quantise8(image).contiguous(), quantise8(hair)[:, :, 0].contiguous(), quantise8(head)[:, :, 0].contiguous(),
            quantise8(angle * hair)[:, :, 0].contiguous(), (conf * hair)[0].float().contiguous())


def core_products_fused(packed):
    """``evaluation.products_fused`` and the five planes of its block the synthetic branch reads (views into the block)"""
    from .evaluation import products_fused
    _, H, W = packed.shape
    n = H * W
    block = products_fused(packed)
    return (block[:3 * n].view(H, W, 3), block[3 * n:4 * n].view(H, W), block[4 * n:5 * n].view(H, W), block[5 * n:6 * n].view(H, W),
            block[12 * n:16 * n].view(torch.float32).view(H, W))


def from_render_fused(packed, white_background=False, binarize_masks=False, fill=None):
    """ONE launch of ``k_gt_from_render`` on the current stream: ``(image [3,H,W], mask [2,H,W], angle [1,H,W], conf [1,H,W])`` from
    the packed [10,H,W] render.  ``fill``: a byte the outputs are pre-filled with (tests)."""
    assert packed.is_cuda, "the synthetic ground-truth kernel has no CPU path (fused=False is the torch form)"
    C, H, W = (int(x) for x in packed.shape)
    assert C == _lib.NUM_CHANNELS
    r = packed.detach().float().contiguous()
    dev = r.device
    t255, _ = _tables(dev)
    guard, _ptr, _stream = _launch_env(r)
    with guard:
        outs = tuple(_new_planes(c, H, W, dev, fill) for c in (3, 2, 1, 1))
        _lib.check(_lib.lib().ghr_gt_from_render(_stream(), W, H, _ptr(r), _ptr(t255), int(bool(white_background)),
                                                 int(bool(binarize_masks)), *(_ptr(o) for o in outs)))
    return outs


def ground_truth_from_render(packed, size=None, white_background: bool = False, binarize_masks: bool = False,
                             fused: Optional[bool] = None) -> ViewGroundTruth:
    """What ``loadCam`` builds with ``load_synthetic_rgba`` and ``load_synthetic_geom`` from the files ``render_gaussians.py`` would
    write for this render, without the files: ``packed`` is the [10,H,W] rasterizer output (``render(...).renders_packed``), finite.
    ``size`` None or ``(W, H)``: on a ROCm tensor ONE launch.  Another ``(w, h)`` (the caller's ``training_resolution`` of the
    original photograph's size): the products on the device, the four byte planes through ``resize_u8``, the assembly with the
    angle ``/ 255``, the confidence through the bilinear resize.  ``fused=False``: ``evaluation.products_torch``'s values and the
    torch assembly, on CPU tensors too."""
    t, was_numpy = _as_tensor(packed)
    if t.dim() != 3 or t.shape[0] != _lib.NUM_CHANNELS or t.shape[1] < 1 or t.shape[2] < 1:
        raise ValueError("ground_truth_from_render: packed must be [%d,H,W], got %s" % (_lib.NUM_CHANNELS, tuple(t.shape)))
    H, W = int(t.shape[1]), int(t.shape[2])
    w, h = (W, H) if size is None else _size(size)
    k = _use_kernels(t, fused)
    if k and (w, h) == (W, H):
        o_img, o_mask, o_ang, o_conf = from_render_fused(t, white_background, binarize_masks)
    else:
        img, hair, head, orient, conf = core_products_fused(t) if k else _core_products_torch(t.float())
        if (w, h) != (W, H):
            img, hair, head, orient = ((resize_u8_fused(x, w, h) if k else _resize_torch(x, w, h)) for x in (img, hair, head, orient))
        if k:
            o_img, o_mask, o_ang, _ = _assemble_launch(img, hair, head, orient, None, white_background, binarize_masks, False, None, 255)
        else:
            o_img, o_mask, o_ang, _ = _assemble_torch(img, hair, head, orient, None, white_background, binarize_masks, False, 255)
        o_conf = _fit_conf(conf, w, h, k)
    res = (o_img, o_mask, o_ang, o_conf, o_mask[0:1], o_mask[1:2])
    return ViewGroundTruth(*(_out(x, was_numpy) for x in res))


@torch.no_grad()
def attach_synthetic_ground_truth(cams: Sequence, gaussians, background, pipe=None, gaussians_hair=None, white_background: bool = False,
                                  binarize_masks: bool = False, fused: Optional[bool] = None) -> List:
    """The strand stages' ``--load_synthetic_rgba --load_synthetic_geom`` at ``-r 1``: renders every camera (``Camera``,
    ``BankCamera``) with ``render``, or ``render_hair`` when ``gaussians_hair`` is given, and fills its ``original_image`` /
    ``original_mask`` / ``original_orient_angle`` / ``original_orient_conf`` with ``ground_truth_from_render`` of that render:
    28 B per pixel per view stay on the device, nothing goes through the host.  The tensors are new ones (the cameras' previous
    ones are not written), so what is cached per ground-truth tensor (trainer._gt_stats) is recomputed."""
    from .evaluation import _default_pipe, _render_view
    pipe = _default_pipe() if pipe is None else pipe
    for cam in cams:
        pkg = _render_view(cam, gaussians, gaussians_hair, pipe, background)
        gt = ground_truth_from_render(pkg.renders_packed, None, white_background, binarize_masks, fused)
        got = tuple(gt.original_image.shape[1:])
        if got != (cam.image_height, cam.image_width):
            raise ValueError("attach_synthetic_ground_truth: a render of %d x %d (h x w) for a %d x %d camera"
                             % (got + (cam.image_height, cam.image_width)))
        cam.original_image, cam.original_mask = gt.original_image, gt.original_mask
        cam.original_orient_angle, cam.original_orient_conf = gt.original_orient_angle, gt.original_orient_conf
    return list(cams)
