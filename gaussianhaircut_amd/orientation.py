"""Ground-truth orientation maps from images: what the reference's ``src/preprocessing/calc_orientation_maps.py`` computes with
its argparse defaults, and what ``src/utils/camera_utils.py:66-68`` makes of its two files.

* ``difference_of_gaussians`` -- ``rgb2gray`` and skimage's ``difference_of_gaussians(gray, 0.4, 10)``: two
  ``scipy.ndimage.gaussian_filter`` calls in float64 (``mode='nearest'``, ``truncate=4``), subtracted, narrowed to float32.
* ``gabor_bank`` -- ``generate_gabor_filters``: the real part of skimage's ``gabor_kernel`` at 180 angles, each zero-padded,
  centred, to the bank's common odd size (17 at the defaults).
* ``gabor_orientation`` -- ``calc_orients``: cross-correlation of the zero-padded plane with the bank, ``F_k = |response_k|``,
  ``deg`` = the first arg-max, ``var = sum_k d_k^2 F_k / max(sum_k F_k, 1e-12)``.
* ``ground_truth_from_maps`` / ``attach_orientation_ground_truth`` -- the loader: ``angle = deg / 180`` and
  ``conf = 1 / ((var / pi^2)^2 + 1e-7)`` on the float16 the reference stores, into ``original_orient_angle`` / ``_conf``.

``fused=True`` (the default on a ROCm tensor) runs the HIP kernels of ``csrc/ghr_orient.h``: two launches for the difference of
Gaussians and ONE for the whole bank with its arg-max, variance and ground-truth tensors -- the 180 responses of a pixel never
reach memory.  ``fused=False`` is the same computation composed from PyTorch operations as the reference composes it (its patch
loop included); it takes CPU tensors too and is what the kernels are tested and timed against.  numpy in, numpy out (through
the comparator on the host); tensor in, tensors out on the tensor's device.  Images are on the 0 ... 255 scale whatever their
dtype.  Multi-scale banks (more than one sigma, offset or frequency) and resizing are not built.
"""
from __future__ import annotations

import ctypes
import math
from collections import namedtuple
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib

OrientationMaps = namedtuple("OrientationMaps", ("deg", "var", "filtered"))
DOG_LOW, DOG_HIGH = 0.4, 10.0
MAX_FILTERS, MAX_KSIZE = 256, 25   # GHR_ORIENT_MAX_*
PATCH = 64                         # --patch_size of the reference


# ---- host side: taps and the bank -----------------------------------------------------------------------------------------------

def dog_taps(sigma: float, truncate: float = 4.0) -> np.ndarray:
    """scipy.ndimage's Gaussian taps in double: ``exp(-x^2 / (2 sigma^2))`` over ``|x| <= int(truncate sigma + 0.5)``, sum 1."""
    r = int(truncate * float(sigma) + 0.5)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    return phi / phi.sum()


def _gabor_kernel_real(frequency, theta, sigma_x, sigma_y, offset, n_stds=3):
    """real part of skimage.filters.gabor_kernel, in float64"""
    ct, st = math.cos(theta), math.sin(theta)
    x0 = math.ceil(max(abs(n_stds * sigma_x * ct), abs(n_stds * sigma_y * st), 1))
    y0 = math.ceil(max(abs(n_stds * sigma_y * ct), abs(n_stds * sigma_x * st), 1))
    y, x = np.meshgrid(np.arange(-y0, y0 + 1), np.arange(-x0, x0 + 1), indexing="ij", sparse=True)
    rotx = x * ct + y * st
    roty = -x * st + y * ct
    g = np.exp(-0.5 * (rotx ** 2 / sigma_x ** 2 + roty ** 2 / sigma_y ** 2))
    g /= 2 * math.pi * sigma_x * sigma_y
    return g * np.cos(2 * math.pi * frequency * rotx + offset)


def _one(v, what):
    if np.ndim(v) == 0:
        return float(v)
    if len(v) != 1:
        raise ValueError("orientation: a bank over several %s is not built (the reference's defaults use one)" % what)
    return float(v[0])


def gabor_bank(num_filters: int = 180, sigma_x=1.8, sigma_y=2.4, frequency=0.23, offset=0.0) -> Tuple[np.ndarray, np.ndarray]:
    """``(weights float32 [F,K,K], thetas float64 [F])`` of generate_gabor_filters: filter k is the real part of
    ``gabor_kernel(frequency, theta = pi - theta_k, sigma_x, sigma_y, offset)``, ``theta_k = pi k / F``, padded to the largest
    support of the bank made odd.  A sequence of more than one sigma, offset or frequency raises ValueError."""
    sigma_x, sigma_y = _one(sigma_x, "sigma_x"), _one(sigma_y, "sigma_y")
    frequency, offset = _one(frequency, "frequencies"), _one(offset, "offsets")
    num_filters = int(num_filters)
    if not 1 <= num_filters <= MAX_FILTERS:
        raise ValueError("orientation: num_filters must be 1 ... %d" % MAX_FILTERS)
    thetas = np.linspace(0, math.pi * (num_filters - 1) / num_filters, num_filters)
    kernels = [_gabor_kernel_real(frequency, math.pi - t, sigma_x, sigma_y, offset) for t in thetas]
    K = max(max(k.shape) for k in kernels)
    K += 1 - (K % 2)
    if K > MAX_KSIZE:
        raise ValueError("orientation: the bank's support %d exceeds %d taps" % (K, MAX_KSIZE))
    w = np.zeros((num_filters, K, K))
    for i, k in enumerate(kernels):
        py, px = (K - k.shape[0]) // 2, (K - k.shape[1]) // 2
        w[i, py:py + k.shape[0], px:px + k.shape[1]] = k
    return w.astype(np.float32), thetas


def pack_bank(weights: np.ndarray) -> np.ndarray:
    """[F,K,K] float32 -> the order ghr_orient_gabor reads (include/ghr.h): [tile][chunk][lane] with lane l holding filter
    16 tile + (l & 15), tap 4 chunk + (l >> 4); zero where the filter or the tap does not exist."""
    Fn, K, K2 = weights.shape
    assert K == K2 and K % 2 == 1 and K <= MAX_KSIZE and 1 <= Fn <= MAX_FILTERS, weights.shape
    tiles = 4 * ((((Fn + 15) // 16) + 3) // 4)
    chunks = (K * K + 3) // 4
    w = np.zeros((tiles * 16, chunks * 4), np.float32)
    w[:Fn, :K * K] = np.asarray(weights, np.float32).reshape(Fn, K * K)
    return np.ascontiguousarray(w.reshape(tiles, 16, chunks, 4).transpose(0, 2, 3, 1)).reshape(-1)


_DEFAULT_BANK = None


def _bank(bank):
    global _DEFAULT_BANK
    if bank is None:
        if _DEFAULT_BANK is None:
            _DEFAULT_BANK = gabor_bank()
        return _DEFAULT_BANK
    w, th = bank
    return np.asarray(w, np.float32), np.asarray(th, np.float64)


_dev_cache = {}


def _on_dev(key, dev, make):
    """small constants (taps, the packed bank) are uploaded once per device"""
    k = (key, str(dev))
    if k not in _dev_cache:
        if len(_dev_cache) > 32:
            _dev_cache.clear()
        _dev_cache[k] = make().to(dev)
    return _dev_cache[k]


def _bank_key(w, th):
    return ("bank", w.shape, hash(w.tobytes()), hash(np.asarray(th).tobytes()))


# ---- input handling ----------------------------------------------------------------------------------------------------------------

def _as_tensor(a):
    """-> (tensor, was_numpy)"""
    if isinstance(a, torch.Tensor):
        return a.detach(), False
    return torch.from_numpy(np.ascontiguousarray(a)), True


def _check_image(t):
    if t.dim() == 3 and t.shape[2] == 1:
        t = t[:, :, 0]
    if not (t.dim() == 2 or (t.dim() == 3 and t.shape[2] == 3)):
        raise ValueError("orientation: image must be [H,W] or [H,W,3], got %s" % (tuple(t.shape),))
    return t


def _use_kernels(t, fused):
    if fused is None:
        return bool(t.is_cuda)
    if fused and not t.is_cuda:
        raise ValueError("orientation: the kernels have no CPU path (fused=False is the PyTorch form)")
    return bool(fused)


def _out(t, was_numpy):
    return t.cpu().numpy() if was_numpy else t


def _launch_env(t):
    from .diff_gaussian_rasterization import _on_device, _ptr, _stream
    return _on_device(t.device), _ptr, _stream


# ---- difference of Gaussians ---------------------------------------------------------------------------------------------------

def _grey64(t):
    x = t.double()
    if x.dim() == 2:
        return x
    return 0.2989 * x[:, :, 0] + 0.5870 * x[:, :, 1] + 0.1140 * x[:, :, 2]


def _gauss64(g, sigma):
    """scipy.ndimage.gaussian_filter(g, sigma, mode='nearest'): axis 0, then axis 1, each as correlate1d sums a symmetric
    filter (the centre tap, then the mirrored pairs from the outermost inwards)"""
    w = dog_taps(sigma)
    r = (len(w) - 1) // 2
    for axis in (0, 1):
        n = g.shape[axis]
        idx = torch.arange(-r, n + r, device=g.device).clamp_(0, n - 1)
        gp = g.index_select(axis, idx)
        t = gp.narrow(axis, r, n) * float(w[r])
        for j in range(-r, 0):
            t = t + (gp.narrow(axis, r + j, n) + gp.narrow(axis, r - j, n)) * float(w[j + r])
        g = t
    return g


def _dog_torch(t, low, high):
    grey = _grey64(t)
    return (_gauss64(grey, low) - _gauss64(grey, high)).float()


def dog_fused(image: torch.Tensor, low: float = DOG_LOW, high: float = DOG_HIGH, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Two launches of k_orient_dog on the current stream: [H,W] or [H,W,3], uint8 or float -> the float32 plane [H,W]."""
    assert image.is_cuda, "the orientation kernels have no CPU path (fused=False is the PyTorch form)"
    t = _check_image(image)
    if t.dtype != torch.uint8:
        t = t.float()
    t = t.contiguous()
    H, W = int(t.shape[0]), int(t.shape[1])
    ch = 1 if t.dim() == 2 else 3
    dev = t.device
    wl = _on_dev(("taps", float(low)), dev, lambda: torch.from_numpy(dog_taps(low)))
    wh = _on_dev(("taps", float(high)), dev, lambda: torch.from_numpy(dog_taps(high)))
    guard, _ptr, _stream = _launch_env(t)
    with guard:
        L = _lib.lib()
        scratch = torch.empty(int(L.ghr_orient_dog_scratch_bytes(W, H)) // 8, dtype=torch.float64, device=dev)
        if out is None:
            out = torch.empty((H, W), dtype=torch.float32, device=dev)
        assert out.dtype == torch.float32 and out.numel() == H * W and out.is_contiguous()
        _lib.check(L.ghr_orient_dog(_stream(), W, H, ch, int(t.dtype == torch.uint8), _ptr(t), (wl.numel() - 1) // 2, _ptr(wl),
                                    (wh.numel() - 1) // 2, _ptr(wh), _ptr(scratch), _ptr(out)))
    return out


def difference_of_gaussians(image, low: float = DOG_LOW, high: float = DOG_HIGH, fused: Optional[bool] = None):
    """The float32 plane [H,W] the Gabor bank runs over."""
    t, was_numpy = _as_tensor(image)
    t = _check_image(t)
    res = dog_fused(t, low, high) if _use_kernels(t, fused) else _dog_torch(t, low, high)
    return _out(res, was_numpy)


# ---- the bank ----------------------------------------------------------------------------------------------------------------------

def _gabor_torch(plane, weights, thetas, patch_size=PATCH):
    """calc_orients:59-92 on one plane, its patch loop included (the patches change no value)"""
    Fn, K = int(weights.shape[0]), int(weights.shape[-1])
    pad = K // 2
    H, W = plane.shape
    w = torch.from_numpy(np.asarray(weights, np.float32)).to(plane.device)[:, None]
    th = torch.from_numpy(np.asarray(thetas)).float().to(plane.device)[:, None, None]
    pp = F.pad(plane.float(), (pad, pad, pad, pad))
    deg = torch.zeros((H, W), dtype=torch.long, device=plane.device)
    var = torch.zeros((H, W), dtype=torch.float32, device=plane.device)
    for i in range(0, H, patch_size):
        for j in range(0, W, patch_size):
            patch = pp[i:i + patch_size + 2 * pad, j:j + patch_size + 2 * pad]
            Fp = F.conv2d(patch[None, None], w)[0].abs()
            Fnorm = F.normalize(Fp, p=1.0, dim=0)
            d = Fp.argmax(0)
            rad = d / Fn * math.pi
            dist = torch.minimum((rad[None] - th).abs(), torch.minimum((rad[None] - th - math.pi).abs(), (rad[None] - th + math.pi).abs()))
            deg[i:i + patch_size, j:j + patch_size] = d
            var[i:i + patch_size, j:j + patch_size] = (dist ** 2 * Fnorm).sum(0)
    return deg.to(torch.uint8), var


def gabor_fused(filtered: torch.Tensor, bank=None, ground_truth: bool = False, via_float16: bool = True, fill=None):
    """ONE launch of k_orient_gabor on the current stream: ``(deg uint8, var float32)`` [H,W], and with ``ground_truth`` also
    ``(angle, conf)`` [1,H,W] from the same launch.  ``fill``: a byte the outputs are pre-filled with (tests)."""
    assert filtered.is_cuda, "the orientation kernels have no CPU path (fused=False is the PyTorch form)"
    p = filtered.detach().float().contiguous()
    assert p.dim() == 2, p.shape
    H, W = int(p.shape[0]), int(p.shape[1])
    w, th = _bank(bank)
    Fn, K = int(w.shape[0]), int(w.shape[-1])
    dev = p.device
    key = _bank_key(w, th)
    wd = _on_dev(key + ("w",), dev, lambda: torch.from_numpy(pack_bank(w)))
    td = _on_dev(key + ("t",), dev, lambda: torch.from_numpy(np.asarray(th, np.float64).astype(np.float32)))
    guard, _ptr, _stream = _launch_env(p)
    with guard:
        L = _lib.lib()
        assert wd.numel() == int(L.ghr_orient_bank_floats(Fn, K)), (wd.numel(), Fn, K)

        def new(shape, dtype):
            t = torch.empty(shape, dtype=dtype, device=dev)
            if fill is not None:
                t.view(torch.uint8).fill_(fill)
            return t
        deg, var = new((H, W), torch.uint8), new((H, W), torch.float32)
        angle = new((1, H, W), torch.float32) if ground_truth else None
        conf = new((1, H, W), torch.float32) if ground_truth else None
        _lib.check(L.ghr_orient_gabor(_stream(), W, H, _ptr(p), Fn, K, _ptr(wd), _ptr(td), _ptr(deg), _ptr(var),
                                      _ptr(angle) if ground_truth else None, _ptr(conf) if ground_truth else None,
                                      int(bool(via_float16))))
    return (deg, var, angle, conf) if ground_truth else (deg, var)


def gabor_orientation(filtered, bank=None, fused: Optional[bool] = None, patch_size: int = PATCH):
    """``(deg uint8 [H,W], var float32 [H,W])`` of a float32 plane; ``bank``: ``gabor_bank(...)`` (None: the defaults)."""
    t, was_numpy = _as_tensor(filtered)
    if _use_kernels(t, fused):
        deg, var = gabor_fused(t, bank)
    else:
        w, th = _bank(bank)
        deg, var = _gabor_torch(t, w, th, patch_size)
    return _out(deg, was_numpy), _out(var, was_numpy)


def orientation_maps(image, dog_low: float = DOG_LOW, dog_high: float = DOG_HIGH, num_filters: int = 180, sigma_x=1.8, sigma_y=2.4,
                     frequency=0.23, offset=0.0, bank=None, fused: Optional[bool] = None, patch_size: int = PATCH) -> OrientationMaps:
    """``calc_orients``: ``(deg, var, filtered)`` of an [H,W,3] or [H,W] image, uint8 or float, numpy or tensor."""
    if bank is None and (num_filters, sigma_x, sigma_y, frequency, offset) != (180, 1.8, 2.4, 0.23, 0.0):
        bank = gabor_bank(num_filters, sigma_x, sigma_y, frequency, offset)
    t, was_numpy = _as_tensor(image)
    t = _check_image(t)
    k = _use_kernels(t, fused)
    filtered = dog_fused(t, dog_low, dog_high) if k else _dog_torch(t, dog_low, dog_high)
    if k:
        deg, var = gabor_fused(filtered, bank)
    else:
        w, th = _bank(bank)
        deg, var = _gabor_torch(filtered, w, th, patch_size)
    return OrientationMaps(_out(deg, was_numpy), _out(var, was_numpy), _out(filtered, was_numpy))


# ---- the loader ----------------------------------------------------------------------------------------------------------------------

def ground_truth_from_maps(deg, var, via_float16: bool = True):
    """camera_utils.py:66-68 at an unchanged size: ``angle = deg / 180`` in [0, 1] and ``conf = 1 / ((var / pi^2)^2 + 1e-7)``,
    ``var`` rounded through float16 (the reference's ``vars/*.npy``) unless ``via_float16`` is off; both float32 [1,H,W]."""
    d, was_numpy = _as_tensor(deg)
    v, _ = _as_tensor(var)
    # The loader divides on the CPU.  On a device PyTorch turns `tensor / python_scalar` into a multiplication by the reciprocal,
    # one rounding more: the angle comes from a table divided on the host, the variance is divided by a tensor.
    table = (torch.arange(256, dtype=torch.float32) / 180.0).clamp_(0.0, 1.0).to(d.device)
    angle = table[d.long()][None]
    v = v.to(torch.float16).float() if via_float16 else v.float()
    q = v / torch.full_like(v, math.pi ** 2)
    conf = (1 / (q * q + 1e-7))[None]
    return _out(angle, was_numpy), _out(conf, was_numpy)


def attach_orientation_ground_truth(cams: Sequence, images: Sequence, overwrite: bool = False, fused: Optional[bool] = None,
                                    bank=None) -> List:
    """Fills ``original_orient_angle`` / ``original_orient_conf`` ([1,H,W], on the image's device) of every camera (``Camera``,
    ``BankCamera``) that lacks one of them -- or of all, with ``overwrite`` -- from its image ([H,W,3] or [H,W], 0 ... 255).
    On a ROCm tensor: three launches per image, the two tensors straight out of the bank's kernel.  Returns the cameras filled."""
    if len(cams) != len(images):
        raise ValueError("attach_orientation_ground_truth: %d cameras, %d images" % (len(cams), len(images)))
    done = []
    for cam, image in zip(cams, images):
        if not overwrite and getattr(cam, "original_orient_angle", None) is not None and getattr(cam, "original_orient_conf", None) is not None:
            continue
        t, _ = _as_tensor(image)
        t = _check_image(t)
        if (int(t.shape[0]), int(t.shape[1])) != (cam.image_height, cam.image_width):
            raise ValueError("attach_orientation_ground_truth: image %s for a %d x %d camera (resizing is not built)"
                             % (tuple(t.shape), cam.image_height, cam.image_width))
        if _use_kernels(t, fused):
            _, _, angle, conf = gabor_fused(dog_fused(t), bank, ground_truth=True)
        else:
            w, th = _bank(bank)
            angle, conf = ground_truth_from_maps(*_gabor_torch(_dog_torch(t, DOG_LOW, DOG_HIGH), w, th))
        cam.original_orient_angle, cam.original_orient_conf = angle, conf
        done.append(cam)
    return done


def vis_orientation(deg, hair_mask) -> np.ndarray:
    """calc_orientation_maps.py:134-150: the four-colour wheel over ``deg`` times the hair mask ([H,W] in [0, 1]) as uint8 [H,W,3],
    channels in the order the reference hands to cv2.imwrite -- which writes them as B, G, R."""
    rad = np.asarray(deg.cpu() if isinstance(deg, torch.Tensor) else deg).astype(np.uint8)
    mask = np.asarray(hair_mask.cpu() if isinstance(hair_mask, torch.Tensor) else hair_mask, np.float64)
    red = np.clip(1 - np.abs(rad - 0.) / 45., 0, 1) + np.clip(1 - np.abs(rad - 180.) / 45., 0, 1)
    green = np.clip(1 - np.abs(rad - 90.) / 45., 0, 1)
    magenta = np.clip(1 - np.abs(rad - 45.) / 45., 0, 1)
    teal = np.clip(1 - np.abs(rad - 135.) / 45., 0, 1)
    rgb = (np.array([0, 0, 1])[None, None] * red[..., None] + np.array([0, 1, 0])[None, None] * green[..., None] +
           np.array([1, 0, 1])[None, None] * magenta[..., None] + np.array([1, 1, 0])[None, None] * teal[..., None])
    return (np.clip(rgb, 0, 1) * mask[..., None] * 255.).astype(np.uint8)


def filtered_to_u8(filtered) -> np.ndarray:
    """:115, :154: ``(f - min) / (max - min) * 255``, truncated"""
    f = np.asarray(filtered.cpu() if isinstance(filtered, torch.Tensor) else filtered)
    return ((f - f.min()) / (f.max() - f.min()) * 255).astype(np.uint8)
