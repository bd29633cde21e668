"""The comparison video's frames: photograph | strand render | Gaussian render, one strip per camera of the path.

What ``src/postprocessing/concat_video.py:26-40`` computes from its three decoded images per frame: the strand render composited
over white (Pillow's ``paste`` through the image's own alpha), the strand render and the photograph brought to the Gaussian
render's size (torchvision's ``Resize(int)`` and ``CenterCrop`` on PIL images, Pillow's 8-bit bicubic resize), the three panels
side by side, and the strip resized to a short edge of 720.  File formats, decoding and the encoder stay outside
(``tools/render_comparison_video.py`` reads and writes PNGs; nothing here needs Pillow).

The definition of a frame, in integers on interleaved uint8 images:

1. over white: per colour byte ``c`` of a pixel with alpha ``a``, ``t = c a + 255 (255 - a) + 128``, ``out = ((t >> 8) + t) >> 8``;
2. ``short_edge(w, h, size)``: ``(size, int(size * h / w))`` if ``w <= h`` else ``(int(size * w / h), size)``; a resize to the
   image's own size is the identity;
3. the render is ``[h, w, 3]``;
4. the strand render is resized (``ground_truth.resize_u8``, bicubic) to ``short_edge(wb, hb, h)``; an axis shorter than the
   panel is padded with black, ``(d) // 2`` before and ``(d + 1) // 2`` after for a deficit ``d``; the ``h x w`` window is cut at
   ``int(round((size - panel) / 2.0))`` per axis of the padded image, Python's rounding (halves go to the even neighbour);
5. the photograph is resized to ``short_edge(wg, hg, w)``, which must be ``(w, h)``;
6. the strip is ``[h, 3 w, 3]``: photograph | strand render | render;
7. the frame is the strip resized to ``short_edge(3 w, h, out_short)``.

``fused=None`` / ``True`` on a ROCm tensor: ``ghr_cmp_over_white`` (a four-channel strand render only), the two resizes,
``ghr_cmp_strip`` and the last resize -- at most eight launches -- on the current stream (``csrc/ghr_compare.h``,
``csrc/ghr_gt.h``).  ``fused=False``: the same arithmetic composed from torch integer operations and ``resize_u8(fused=False)``,
the comparator, the only form for CPU tensors.  Both give the same bytes.  numpy in, numpy out; tensor in, tensor out.
"""
from __future__ import annotations

from typing import Iterable, Iterator, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .ground_truth import _resize_torch, resize_u8_fused
from .orientation import _as_tensor, _launch_env, _out


def _use_kernels(t, fused):
    if fused is None:
        return bool(t.is_cuda)
    if fused and not t.is_cuda:
        raise ValueError("comparison: the kernels have no CPU path (fused=False is the torch form)")
    return bool(fused)


class ComparisonLayout(NamedTuple):
    """Every number of a frame, plain ints.  Sizes are in pixels; ``pad_*`` and ``crop_*`` are CenterCrop's on the resized strand
    render (``preview_w x preview_h``), whose padded size is ``max(preview_w, w) x max(preview_h, h)``."""
    w: int
    h: int
    preview_w: int
    preview_h: int
    pad_left: int
    pad_top: int
    pad_right: int
    pad_bottom: int
    crop_left: int
    crop_top: int
    out_w: int
    out_h: int


def short_edge(w: int, h: int, size: int) -> Tuple[int, int]:
    """torchvision's ``Resize(size)`` with an int: the shorter edge becomes ``size``, the longer ``int(size * long / short)`` --
    an integer product, a true division and a truncation, as Python evaluates it.  ``(w, h)``."""
    w, h, size = int(w), int(h), int(size)
    if w < 1 or h < 1 or size < 1:
        raise ValueError("short_edge: sizes must be >= 1, got %d x %d to %d" % (w, h, size))
    if w <= h:
        return size, int(size * h / w)
    return int(size * w / h), size


def _wh(size, what):
    w, h = int(size[0]), int(size[1])
    if w < 1 or h < 1:
        raise ValueError("comparison_layout: %s must be (w, h) with both >= 1, got %s" % (what, tuple(size)))
    return w, h


def comparison_layout(gt_size, preview_size, render_size, out_short: int = 720) -> ComparisonLayout:
    """The numbers of one frame from the three images' ``(w, h)``: host arithmetic only.  Raises ``ValueError`` when the
    photograph, resized to the render's width, is not exactly the render's size (the script's ``np.concatenate`` fails there).
    That rule holds only for ``w <= h``, where both edges of the resized strand render are ``>= h >= w``: a whole frame never
    pads.  ``gt_size=None`` leaves the photograph out -- the middle panel's numbers alone, for any render (the strip's tests)."""
    wb, hb = _wh(preview_size, "preview_size")
    w, h = _wh(render_size, "render_size")
    if gt_size is not None:
        wg, hg = _wh(gt_size, "gt_size")
        got = short_edge(wg, hg, w)
        if got != (w, h):
            raise ValueError("comparison_layout: the photograph of %d x %d becomes %d x %d (w x h) at the render's width, the render "
                             "is %d x %d" % (wg, hg, got[0], got[1], w, h))
    rw, rh = short_edge(wb, hb, h)
    if rw < 1 or rh < 1:
        raise ValueError("comparison_layout: the strand render of %d x %d vanishes at a short edge of %d" % (wb, hb, h))
    dw, dh = max(w - rw, 0), max(h - rh, 0)
    pad_left, pad_right, pad_top, pad_bottom = dw // 2, (dw + 1) // 2, dh // 2, (dh + 1) // 2
    crop_left = int(round((rw + dw - w) / 2.0))
    crop_top = int(round((rh + dh - h) / 2.0))
    out_w, out_h = short_edge(3 * w, h, out_short)
    if out_w < 1 or out_h < 1:
        raise ValueError("comparison_layout: a strip of %d x %d vanishes at a short edge of %d" % (3 * w, h, int(out_short)))
    return ComparisonLayout(w, h, rw, rh, pad_left, pad_top, pad_right, pad_bottom, crop_left, crop_top, out_w, out_h)


# ---- checks --------------------------------------------------------------------------------------------------------------------------

def _image(a, what, channels):
    t, was_numpy = _as_tensor(a)
    if t.dtype != torch.uint8:
        raise ValueError("%s: %s images are not built (uint8 only)" % (what, str(t.dtype).replace("torch.", "")))
    if t.dim() != 3 or int(t.shape[2]) not in channels:
        raise ValueError("%s: image must be [H,W,%s], got %s" % (what, " or ".join(str(c) for c in channels), tuple(t.shape)))
    if t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError("%s: empty image %s" % (what, tuple(t.shape)))
    return t.contiguous(), was_numpy


# ---- the comparator ------------------------------------------------------------------------------------------------------------------

def over_white_torch(rgba: torch.Tensor) -> torch.Tensor:
    """cmp_over_white of csrc/ghr_compare.h in torch integers"""
    c, a = rgba[:, :, :3].to(torch.int32), rgba[:, :, 3:4].to(torch.int32)
    t = c * a + 255 * (255 - a) + 128
    return (((t >> 8) + t) >> 8).to(torch.uint8)


def strip_torch(gt, preview, render, lay: ComparisonLayout) -> torch.Tensor:
    """cmp_strip_byte of csrc/ghr_compare.h as torchvision composes it: pad with zeros, cut the window, concatenate"""
    H, W = lay.preview_h + lay.pad_top + lay.pad_bottom, lay.preview_w + lay.pad_left + lay.pad_right
    padded = torch.zeros((H, W, 3), dtype=torch.uint8, device=preview.device)
    padded[lay.pad_top:lay.pad_top + lay.preview_h, lay.pad_left:lay.pad_left + lay.preview_w] = preview
    window = padded[lay.crop_top:lay.crop_top + lay.h, lay.crop_left:lay.crop_left + lay.w]
    return torch.cat([gt, window, render], dim=1).contiguous()


def _frame_torch(gt, preview, render, lay, stages=None):
    if preview.shape[2] == 4:
        preview = over_white_torch(preview)
    small = _resize_torch(preview, lay.preview_w, lay.preview_h)
    photo = _resize_torch(gt, lay.w, lay.h)
    strip = strip_torch(photo, small, render, lay)
    if stages is not None:
        stages.update(preview=small, gt=photo, strip=strip)
    return _resize_torch(strip, lay.out_w, lay.out_h)


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------

def over_white_fused(rgba: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ONE launch of ``k_cmp_over_white`` on the current stream: contiguous uint8 [H,W,4] (any byte offset into its buffer: the
    one-pixel form runs where the four-pixel form's alignment is missing) -> [H,W,3]."""
    assert rgba.is_cuda, "the comparison kernels have no CPU path (fused=False is the torch form)"
    H, W = int(rgba.shape[0]), int(rgba.shape[1])
    guard, _ptr, _stream = _launch_env(rgba)
    with guard:
        if out is None:
            out = torch.empty((H, W, 3), dtype=torch.uint8, device=rgba.device)
        assert out.dtype == torch.uint8 and out.numel() == 3 * H * W and out.is_contiguous() and out.device == rgba.device
        _lib.check(_lib.lib().ghr_cmp_over_white(_stream(), H * W, _ptr(rgba), _ptr(out)))
    return out


def strip_fused(gt, preview, render, lay: ComparisonLayout, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ONE launch of ``k_cmp_strip`` on the current stream: ``gt`` and ``render`` [h,w,3], ``preview`` [preview_h,preview_w,3] ->
    [h,3w,3]"""
    assert gt.is_cuda, "the comparison kernels have no CPU path (fused=False is the torch form)"
    assert tuple(gt.shape) == (lay.h, lay.w, 3) and tuple(render.shape) == (lay.h, lay.w, 3), (gt.shape, render.shape, lay)
    assert tuple(preview.shape) == (lay.preview_h, lay.preview_w, 3), (preview.shape, lay)
    assert gt.is_contiguous() and preview.is_contiguous() and render.is_contiguous()
    guard, _ptr, _stream = _launch_env(gt)
    with guard:
        if out is None:
            out = torch.empty((lay.h, 3 * lay.w, 3), dtype=torch.uint8, device=gt.device)
        assert out.dtype == torch.uint8 and out.numel() == 9 * lay.h * lay.w and out.is_contiguous() and out.device == gt.device
        _lib.check(_lib.lib().ghr_cmp_strip(_stream(), lay.w, lay.h, _ptr(gt), _ptr(preview), lay.preview_w, lay.preview_h, lay.pad_left,
                                            lay.pad_top, lay.crop_left, lay.crop_top, _ptr(render), _ptr(out)))
    return out


_workspaces = {}


def _workspace(dev, lay, preview_shape):
    """a frame's intermediates, kept per device and sizes: a sequence of equal frames allocates them once"""
    key = (str(dev), lay, tuple(preview_shape))
    ws = _workspaces.get(key)
    if ws is None:
        if len(_workspaces) >= 4:
            _workspaces.clear()
        new = lambda *s: torch.empty(s, dtype=torch.uint8, device=dev)   # noqa: E731
        ws = _workspaces[key] = dict(rgb=new(int(preview_shape[0]), int(preview_shape[1]), 3) if preview_shape[2] == 4 else None,
                                     preview=new(lay.preview_h, lay.preview_w, 3), gt=new(lay.h, lay.w, 3),
                                     strip=new(lay.h, 3 * lay.w, 3))
    return ws


def _frame_fused(gt, preview, render, lay, out=None, stages=None):
    ws = _workspace(gt.device, lay, preview.shape)
    if preview.shape[2] == 4:
        preview = over_white_fused(preview, ws["rgb"])
    # at equal sizes Pillow returns a copy; the strip copies the bytes anyway, so the image itself is read
    small = preview if (int(preview.shape[1]), int(preview.shape[0])) == (lay.preview_w, lay.preview_h) else \
        resize_u8_fused(preview, lay.preview_w, lay.preview_h, out=ws["preview"])
    photo = gt if (int(gt.shape[1]), int(gt.shape[0])) == (lay.w, lay.h) else resize_u8_fused(gt, lay.w, lay.h, out=ws["gt"])
    strip = strip_fused(photo, small, render, lay, ws["strip"])
    if stages is not None:
        stages.update(preview=small.clone(), gt=photo.clone(), strip=strip.clone())
    if out is None:
        out = torch.empty((lay.out_h, lay.out_w, 3), dtype=torch.uint8, device=gt.device)
    if tuple(out.shape) != (lay.out_h, lay.out_w, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != gt.device:
        raise ValueError("comparison_frame: out must be a contiguous uint8 [%d,%d,3] on %s" % (lay.out_h, lay.out_w, gt.device))
    return resize_u8_fused(strip, lay.out_w, lay.out_h, out=out)


# ---- the public interface --------------------------------------------------------------------------------------------------------------

def over_white(rgba, fused: Optional[bool] = None):
    """``Image.new("RGBA", size, "WHITE")`` with ``rgba`` pasted through its own alpha, ``.convert("RGB")``, bit for bit: uint8
    [H,W,4] -> [H,W,3], of the input's kind."""
    t, was_numpy = _image(rgba, "over_white", (4,))
    return _out(over_white_fused(t) if _use_kernels(t, fused) else over_white_torch(t), was_numpy)


def _frame(gt, preview, render, out_short, fused, out, stages):
    g, was_numpy = _image(gt, "comparison_frame: gt", (3,))
    r, _ = _image(render, "comparison_frame: render", (3,))
    p, _ = _image(preview, "comparison_frame: preview", (3, 4))
    dev = r.device
    g, p = g.to(dev), p.to(dev)
    lay = comparison_layout((g.shape[1], g.shape[0]), (p.shape[1], p.shape[0]), (r.shape[1], r.shape[0]), out_short)
    if _use_kernels(r, fused):
        res = _frame_fused(g, p, r, lay, out, stages)
    else:
        res = _frame_torch(g, p, r, lay, stages)
        if out is not None:
            out.copy_(res)
            res = out
    return _out(res, was_numpy)


def comparison_frame(gt, preview, render, out_short: int = 720, fused: Optional[bool] = None, out: Optional[torch.Tensor] = None):
    """One frame of the comparison video, uint8 ``[Ho, Wo, 3]`` with ``(Wo, Ho) = short_edge(3 w, h, out_short)``: ``gt`` (the
    photograph) and ``render`` (the Gaussian render, ``[h, w, 3]``) uint8 ``[*, *, 3]``, ``preview`` (the strand render) uint8
    ``[*, *, 3]`` or ``[*, *, 4]`` -- four channels go over white first.  The images are brought to ``render``'s device; the result
    is of ``gt``'s kind (numpy in, numpy out).  ``out``: a contiguous uint8 tensor of the frame's size to write into; with it and
    sizes that repeat, a fused frame after the first makes no new tensor of its own (the intermediates are kept per size; the
    resize's scratch comes back from torch's caching allocator)."""
    return _frame(gt, preview, render, out_short, fused, out, None)


def comparison_stages(gt, preview, render, out_short: int = 720, fused: Optional[bool] = None) -> dict:
    """``comparison_frame`` with its intermediates (tests): ``{"preview", "gt", "strip", "frame"}``, tensors on ``render``'s
    device: the two resized panels, the strip before the last resize and the frame."""
    stages = {}
    frame = _frame(*(_as_tensor(x)[0] for x in (gt, preview, render)), out_short, fused, None, stages)
    stages["frame"] = frame
    return stages


def comparison_frames(gts: Iterable, previews: Iterable, renders: Iterable, out_short: int = 720, fused: Optional[bool] = None,
                      device=None) -> Iterator[np.ndarray]:
    """Yields the frames of a path as host ``numpy`` arrays, one per triple of the three iterables (arrays or tensors; host arrays
    are uploaded to ``device``, by default that of the first render that is a tensor, else the CPU).  On a ROCm device the frame
    lands in one of two device buffers and is copied into one of two pinned host buffers on a copy stream: frame k copies down
    while frame k + 1 is assembled, as ``evaluation.render_products`` does.  Every yielded array is the caller's own: it is copied
    out of the pinned buffer and stays valid however far the generator advances."""
    dev = torch.device(device) if device is not None else None
    slots = [None, None]
    pending = None
    side = main = None
    for k, (gt, preview, render) in enumerate(zip(gts, previews, renders)):
        r = _as_tensor(render)[0]
        if dev is None:
            dev = r.device if isinstance(render, torch.Tensor) else torch.device("cpu")
        r, g, p = r.to(dev), _as_tensor(gt)[0].to(dev), _as_tensor(preview)[0].to(dev)
        if not _use_kernels(r, fused):
            yield comparison_frame(g, p, r, out_short, False).cpu().numpy()
            continue
        if side is None:
            main, side = torch.cuda.current_stream(dev), torch.cuda.Stream(dev)
        lay = comparison_layout((g.shape[1], g.shape[0]), (p.shape[1], p.shape[0]), (r.shape[1], r.shape[0]), out_short)
        shape = (lay.out_h, lay.out_w, 3)
        s = slots[k & 1]
        if s is None or tuple(s["dev"].shape) != shape:
            s = slots[k & 1] = dict(dev=torch.empty(shape, dtype=torch.uint8, device=dev),
                                    host=torch.empty(shape, dtype=torch.uint8).pin_memory(),
                                    ready=torch.cuda.Event(), done=torch.cuda.Event())
        else:
            main.wait_event(s["done"])   # the slot's previous frame has left the device buffer
        comparison_frame(g, p, r, out_short, True, out=s["dev"])
        s["ready"].record(main)
        side.wait_event(s["ready"])
        with torch.cuda.stream(side):
            s["host"].copy_(s["dev"], non_blocking=True)
            s["done"].record(side)
        if pending is not None:
            pending["done"].synchronize()
            yield pending["host"].numpy().copy()
        pending = s
    if pending is not None:
        pending["done"].synchronize()
        yield pending["host"].numpy().copy()
