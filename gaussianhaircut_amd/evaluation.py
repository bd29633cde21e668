"""The evaluation pass: what the reference's scripts do with ``render()`` besides training.

* ``evaluate_views`` / ``validation_report`` -- ``training_report`` (``src/train_gaussians.py:232-293``,
  ``src/train_strands.py:204-266``: L1, mask L1 -- logged as ``ce`` --, orientation error and PSNR on clamped images) plus the
  per-view SSIM of ``src/metrics.py:71-78``.  (LPIPS is not computed: it needs pretrained VGG weights.)
* ``render_products`` -- the seven products of ``render_set`` (``src/render_gaussians.py:31-68``) per view: six 8-bit images,
  quantised as torchvision's ``save_image`` does, and the masked orientation confidence as a float plane.

``fused=True`` (the default on a ROCm tensor) runs the HIP kernels of ``csrc/ghr_eval.h`` on the packed [10,H,W] rasterizer
output: three launches per view for the metrics, written into one device table that is read back once after the last view, and
one launch per view for the products, 16 bytes per pixel over PCIe instead of 52.  ``fused=False`` is the same pass composed
from PyTorch operations with the reference's formulas (``utils.loss_utils``, ``utils.image_utils``) -- the comparator the
kernels are tested and timed against; its metric and product functions also take CPU tensors.  Rendering itself is ROCm-only.
One process: views are not sharded over ranks.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Iterator, List, Optional

import numpy as np
import torch

from . import _lib
from .gaussian_renderer import orient_angle_from
from .utils.image_utils import psnr, vis_orient
from .utils.loss_utils import l1_loss, or_loss, ssim

METRICS = ("l1", "ce", "or", "psnr", "ssim")
PRODUCTS = ("render", "hair_mask", "head_mask", "orient", "orient_vis", "orient_conf_vis")   # 8-bit, in block order
_CHANNELS = (3, 1, 1, 1, 3, 3)


def _default_pipe():
    from .trainer import PIPE
    return PIPE


# ---- PyTorch-composed comparator ---------------------------------------------------------------------------------------------

def metrics_torch(packed, gt_image, gt_mask, gt_orient_angle=None, gt_orient_conf=None, with_ssim=True) -> torch.Tensor:
    """``[l1, ce, or, psnr, ssim]`` of one view as a float64 tensor on ``packed``'s device, formed as training_report forms them
    (in ``packed``'s dtype).  Without the orientation ground truth ``or`` is NaN; without ``with_ssim`` ``ssim`` is 0."""
    image = torch.clamp(packed[0:3], 0.0, 1.0)
    mask = torch.clamp(packed[3:5], 0.0, 1.0)
    gt_image = torch.clamp(gt_image.to(packed), 0.0, 1.0)
    gt_mask = torch.clamp(gt_mask.to(packed), 0.0, 1.0)
    out = [l1_loss(image, gt_image).double(), l1_loss(mask, gt_mask).double()]
    if gt_orient_angle is not None and gt_orient_conf is not None:
        angle = torch.clamp(orient_angle_from(packed[5:8]), 0.0, 1.0)
        gt_angle = torch.clamp(gt_orient_angle.to(packed), 0.0, 1.0)
        out.append(or_loss(angle, gt_angle, mask=gt_mask[:1], weight=gt_orient_conf.to(packed)).double())
    else:
        out.append(torch.full((), float("nan"), dtype=torch.float64, device=packed.device))
    out.append(psnr(image, gt_image).mean().double())
    out.append(ssim(image, gt_image).double() if with_ssim else torch.zeros((), dtype=torch.float64, device=packed.device))
    return torch.stack(out)


def quantise8(v: torch.Tensor) -> torch.Tensor:
    """torchvision.utils.save_image: ``mul(255).add_(0.5).clamp_(0, 255).to(uint8)``; CHW -> HWC."""
    return (v * 255 + 0.5).clamp(0, 255).to(torch.uint8).permute(1, 2, 0)


def product_values_torch(packed) -> Dict[str, torch.Tensor]:
    """The seven products of render_set as CHW tensors of ``packed``'s dtype, before quantisation."""
    image, hair, head, conf = packed[0:3], packed[3:4], packed[4:5], packed[8:9]
    angle = orient_angle_from(packed[5:8])
    orient_conf = conf * hair
    return dict(render=image, hair_mask=hair, head_mask=head, orient=angle * hair, orient_vis=vis_orient(angle, hair),
                orient_conf_vis=vis_orient(angle, 1 - 1 / (orient_conf + 1)), orient_conf=orient_conf)


def products_torch(packed) -> Dict[str, np.ndarray]:
    """Host arrays of one view: uint8 [H,W,3] / [H,W] images and the float32 [H,W] ``orient_conf`` plane."""
    vals = product_values_torch(packed)
    out = {}
    for k, c in zip(PRODUCTS, _CHANNELS):
        q = quantise8(vals[k]).cpu().numpy()
        out[k] = q if c == 3 else q[:, :, 0]
    out["orient_conf"] = vals["orient_conf"][0].float().cpu().numpy()
    return out


# ---- HIP kernels ---------------------------------------------------------------------------------------------------------------

def _f32c(t):
    return t.detach().float().contiguous()


def _launch_env(t):
    from .diff_gaussian_rasterization import _on_device, _ptr, _stream
    return _on_device(t.device), _ptr, _stream


def metrics_fused(packed, gt_image, gt_mask, gt_orient_angle=None, gt_orient_conf=None, with_ssim=True, row=None, scratch=None):
    """Launches the metric kernels of one view on the current stream; ``row`` (8 float64 of a device table, made here when
    None) receives ``{l1, ce, or_num, or_den, mse[3], ssim}``.  Nothing is read back."""
    assert packed.is_cuda, "the evaluation kernels have no CPU path (fused=False is the PyTorch form)"
    C, H, W = packed.shape
    assert C == _lib.NUM_CHANNELS
    r, gi, gm = _f32c(packed), _f32c(gt_image).to(packed.device), _f32c(gt_mask).to(packed.device)
    assert tuple(gi.shape) == (3, H, W) and tuple(gm.shape) == (2, H, W), (gi.shape, gm.shape)
    orient = gt_orient_angle is not None and gt_orient_conf is not None
    ga = _f32c(gt_orient_angle).to(packed.device) if orient else None
    gw = _f32c(gt_orient_conf).to(packed.device) if orient else None
    if orient:
        assert ga.numel() == H * W and gw.numel() == H * W, (ga.shape, gw.shape)
    guard, _ptr, _stream = _launch_env(r)
    with guard:
        if row is None:
            row = torch.empty(_lib.EVAL_TERMS, dtype=torch.float64, device=r.device)
        assert row.dtype == torch.float64 and row.numel() == _lib.EVAL_TERMS and row.is_contiguous()
        if scratch is None:
            scratch = torch.empty(eval_scratch_floats(W, H), dtype=torch.float32, device=r.device)
        a = _lib.EvalArgs()
        a.W, a.H = int(W), int(H)
        a.renders, a.gt_image, a.gt_mask = _ptr(r), _ptr(gi), _ptr(gm)
        a.gt_orient_angle, a.gt_orient_conf = (_ptr(ga), _ptr(gw)) if orient else (None, None)
        a.with_ssim = int(bool(with_ssim))
        _lib.check(_lib.lib().ghr_eval_metrics(_stream(), ctypes.byref(a), _ptr(scratch), _ptr(row)))
    return row


def eval_scratch_floats(W: int, H: int) -> int:
    return int(_lib.lib().ghr_eval_scratch_floats(int(W), int(H)))


def metrics_from_table(table: np.ndarray, with_ssim=True) -> np.ndarray:
    """[V,8] float64 rows of the kernels -> [V,5] ``METRICS`` in double on the host: ``or = or_num / or_den`` (0 / 0 = NaN, the
    reference's value for a view without orientation weight), ``psnr`` = mean over channels of ``20 log10(1 / sqrt(mse_c))``
    (``inf`` for an exact match)."""
    table = np.asarray(table, np.float64).reshape(-1, _lib.EVAL_TERMS)
    with np.errstate(divide="ignore", invalid="ignore"):
        orr = table[:, 2] / table[:, 3]
        ps = (20.0 * np.log10(1.0 / np.sqrt(table[:, 4:7]))).mean(axis=1)
    return np.stack([table[:, 0], table[:, 1], orr, ps, table[:, 7]], axis=1)


def product_block_bytes(W: int, H: int) -> int:
    """bytes of one view's block: 12 H W of 8-bit products followed by the H W float32 plane"""
    return 16 * int(W) * int(H)


def products_fused(packed, block=None):
    """One launch: the 8-bit products and the float plane of one view into ``block`` (uint8 [16 H W] on the device, made here
    when None)."""
    assert packed.is_cuda, "the evaluation kernels have no CPU path (fused=False is the PyTorch form)"
    C, H, W = packed.shape
    assert C == _lib.NUM_CHANNELS
    r = _f32c(packed)
    guard, _ptr, _stream = _launch_env(r)
    with guard:
        if block is None:
            block = torch.empty(product_block_bytes(W, H), dtype=torch.uint8, device=r.device)
        assert block.dtype == torch.uint8 and block.numel() == product_block_bytes(W, H) and block.is_contiguous()
        _lib.check(_lib.lib().ghr_eval_products(_stream(), int(W), int(H), _ptr(r), _ptr(block),
                                                ctypes.c_void_p(block.data_ptr() + 12 * H * W)))
    return block


def split_product_block(block: np.ndarray, W: int, H: int, copy=True) -> Dict[str, np.ndarray]:
    """Host block of ``products_fused`` -> the arrays of ``products_torch`` (views into ``block`` unless ``copy``)."""
    n = H * W
    out, off = {}, 0
    for k, c in zip(PRODUCTS, _CHANNELS):
        a = block[off:off + c * n].reshape((H, W, 3) if c == 3 else (H, W))
        out[k] = a.copy() if copy else a
        off += c * n
    a = block[12 * n:16 * n].view(np.float32).reshape(H, W)
    out["orient_conf"] = a.copy() if copy else a
    return out


# ---- the passes -------------------------------------------------------------------------------------------------------------------

def _render_view(cam, gaussians, gaussians_hair, pipe, background):
    from .gaussian_renderer import render, render_hair
    if gaussians_hair is not None:
        return render_hair(cam, gaussians, gaussians_hair, pipe, background)
    return render(cam, gaussians, pipe, background)


def _gt(cam, dev):
    def get(name):
        t = getattr(cam, name, None)
        return None if t is None else t.to(dev)
    return get("original_image"), get("original_mask"), get("original_orient_angle"), get("original_orient_conf")


def _result(per_view: np.ndarray, cams) -> dict:
    views = [dict(zip(METRICS, (float(x) for x in row))) for row in per_view]
    for v, cam in zip(views, cams):
        v["name"] = getattr(cam, "image_name", None)
    with np.errstate(invalid="ignore"):   # inf - inf never happens (PSNR is never -inf); NaN and inf propagate
        mean = per_view.mean(axis=0) if len(per_view) else np.full(len(METRICS), np.nan)
    return dict(views=views, mean=dict(zip(METRICS, (float(x) for x in mean))))


@torch.no_grad()
def evaluate_views(gaussians, cams: List, background, pipe=None, gaussians_hair=None, fused: Optional[bool] = None,
                   with_ssim: bool = True) -> dict:
    """Renders every camera of ``cams`` (``render``, or ``render_hair`` when ``gaussians_hair`` is given) and returns
    ``{"views": [{l1, ce, or, psnr, ssim, name}, ...], "mean": {...}}`` in double against the cameras' ``original_*`` maps.
    The per-view sums go into one device table that is read back ONCE, after the last view (``evaluate_views.table_reads``
    counts those transfers); the loop itself reads nothing from the device.  A view whose orientation weights sum to 0 reports
    NaN ``or``, an exact match ``inf`` PSNR, and the means propagate both, as the reference's running sums do."""
    pipe = _default_pipe() if pipe is None else pipe
    dev = background.device
    fused = bool(dev.type == "cuda") if fused is None else bool(fused)
    V = len(cams)
    if V == 0:
        return _result(np.zeros((0, len(METRICS))), cams)
    table = torch.empty((V, _lib.EVAL_TERMS if fused else len(METRICS)), dtype=torch.float64, device=dev)
    scratch = {}
    for v, cam in enumerate(cams):
        pkg = _render_view(cam, gaussians, gaussians_hair, pipe, background)
        packed = pkg.renders_packed
        gi, gm, ga, gw = _gt(cam, dev)
        if fused:
            _, H, W = packed.shape
            if (W, H) not in scratch:
                scratch[(W, H)] = torch.empty(eval_scratch_floats(W, H), dtype=torch.float32, device=dev)
            metrics_fused(packed, gi, gm, ga, gw, with_ssim, row=table[v], scratch=scratch[(W, H)])
        else:
            table[v] = metrics_torch(packed, gi, gm, ga, gw, with_ssim)
    host = table.cpu().numpy()
    evaluate_views.table_reads += 1
    return _result(metrics_from_table(host, with_ssim) if fused else host, cams)


evaluate_views.table_reads = 0


def validation_cameras(train_cams: List, test_cams: List) -> Dict[str, List]:
    """The two configurations of training_report (train_gaussians.py:243-244): every test camera, and the train cameras
    ``idx % len`` for ``idx in range(5, 30, 5)``."""
    train = [train_cams[idx % len(train_cams)] for idx in range(5, 30, 5)] if train_cams else []
    return {"test": list(test_cams or []), "train": train}


def validation_report(gaussians, train_cams: List, test_cams: List, background, pipe=None, gaussians_hair=None,
                      fused: Optional[bool] = None, with_ssim: bool = True, iteration: Optional[int] = None, log=None) -> dict:
    """``{"test": ..., "train": ...}``: ``evaluate_views`` over the reference's two validation configurations (an empty one is
    skipped, as the reference skips it).  ``log``: optional callable for the reference's one line per configuration."""
    out = {}
    for name, cams in validation_cameras(train_cams, test_cams).items():
        if not cams:
            continue
        res = evaluate_views(gaussians, cams, background, pipe, gaussians_hair, fused, with_ssim)
        out[name] = res
        if log is not None:
            m = res["mean"]
            log("\n[ITER {}] Evaluating {}: L1 {} CE {} OR {} PSNR {} SSIM {}".format(iteration, name, m["l1"], m["ce"], m["or"],
                                                                                     m["psnr"], m["ssim"]))
    return out


@torch.no_grad()
def render_products(gaussians, cams: List, background, pipe=None, gaussians_hair=None, fused: Optional[bool] = None,
                    copy: bool = True) -> Iterator[dict]:
    """Yields, per view, ``{name, render [H,W,3], hair_mask [H,W], head_mask [H,W], orient [H,W], orient_vis [H,W,3],
    orient_conf_vis [H,W,3]}`` as host uint8 arrays plus ``orient_conf`` [H,W] float32.  Fused: one launch and ONE device-to-host
    copy of the view's 16 H W byte block into pinned memory on a copy stream, double-buffered -- view v + 1 renders while view v
    copies.  ``copy=False`` yields views into the pinned buffer, valid until the generator is advanced twice."""
    pipe = _default_pipe() if pipe is None else pipe
    dev = background.device
    fused = bool(dev.type == "cuda") if fused is None else bool(fused)
    if not fused:
        for cam in cams:
            pkg = _render_view(cam, gaussians, gaussians_hair, pipe, background)
            out = products_torch(pkg.renders_packed)
            out["name"] = getattr(cam, "image_name", None)
            yield out
        return
    main = torch.cuda.current_stream(dev)
    side = torch.cuda.Stream(dev)
    slots: List[Optional[dict]] = [None, None]
    pending = None   # (slot, cam, W, H) of the view whose copy is in flight

    def finish(p):
        s, cam, W, H = p
        s["done"].synchronize()
        out = split_product_block(s["host"].numpy()[:product_block_bytes(W, H)], W, H, copy)
        out["name"] = getattr(cam, "image_name", None)
        return out

    for v, cam in enumerate(cams):
        pkg = _render_view(cam, gaussians, gaussians_hair, pipe, background)
        _, H, W = pkg.renders_packed.shape
        nbytes = product_block_bytes(W, H)
        s = slots[v & 1]
        if s is None or s["dev"].numel() < nbytes:
            s = slots[v & 1] = dict(dev=torch.empty(nbytes, dtype=torch.uint8, device=dev),
                                    host=torch.empty(nbytes, dtype=torch.uint8).pin_memory(),
                                    ready=torch.cuda.Event(), done=torch.cuda.Event())
        products_fused(pkg.renders_packed, s["dev"][:nbytes])
        s["ready"].record(main)
        side.wait_event(s["ready"])
        with torch.cuda.stream(side):
            s["host"][:nbytes].copy_(s["dev"][:nbytes], non_blocking=True)
            s["done"].record(side)
        if pending is not None:
            yield finish(pending)
        pending = (s, cam, W, H)
    if pending is not None:
        yield finish(pending)


# ---- strand geometry -----------------------------------------------------------------------------------------------------------

def _segments(points: torch.Tensor):
    """``[S, L, 3]`` strand points -> midpoints and directions of their ``S (L - 1)`` segments, ``[1, S (L - 1), 3]`` each."""
    if points.dim() != 3 or points.shape[1] < 2 or points.shape[2] != 3:
        raise ValueError("strand_geometry: strands must be [S, L >= 2, 3], got %s" % (tuple(points.shape),))
    a, b = points[:, :-1], points[:, 1:]
    return ((a + b) * 0.5).reshape(1, -1, 3).contiguous(), (b - a).reshape(1, -1, 3).contiguous()


@torch.no_grad()
def strand_geometry(pred_points: torch.Tensor, gt_points: torch.Tensor, dist_thresholds, angle_thresholds_deg,
                    fused: Optional[bool] = None) -> dict:
    """How far two grooms are from each other, on segment midpoints with the segment directions as normals (this package's own
    definition; not the paper's evaluation script).  ``pred_points [S, L, 3]``, ``gt_points [S', L', 3]``.

    Returns ``chamfer_pred_to_gt`` / ``chamfer_gt_to_pred`` (mean SQUARED distance of a midpoint to the nearest midpoint of the
    other groom), ``direction_pred_to_gt`` / ``direction_gt_to_pred`` (mean ``1 - |cos|`` to that neighbour's direction) and, for
    every pair of ``thresholds`` = ``dist_thresholds x angle_thresholds_deg``, ``precision`` (the share of predicted midpoints
    whose neighbour lies within the distance -- a distance, not squared: ``d2 <= t_d^2`` -- AND at an unsigned angle below the
    angle threshold: ``1 - |cos| < 1 - cos(t_a)``), ``recall`` (the same from the ground truth's side) and ``fscore``
    (``2 P R / (P + R)``, 0 when both are 0).  Lists are in ``thresholds``' order.  One read-back at the end."""
    from . import nearest
    px, pn = _segments(pred_points)
    gx, gn = _segments(gt_points)
    sides = []
    for (x, xn), (y, yn) in (((px, pn), (gx, gn)), ((gx, gn), (px, pn))):
        nn = nearest.knn_points(x, y, norm=2, K=1, fused=fused)
        term, _ = nearest.point_terms(nn.idx, xn, yn, abs_cosine=True, fused=fused)
        sides.append((nn.dists[0, :, 0], term[0]))
    thresholds = [(float(td), float(ta)) for td in dist_thresholds for ta in angle_thresholds_deg]
    dev, dt = px.device, px.dtype
    td2 = torch.tensor([td * td for td, _ in thresholds], dtype=dt, device=dev)
    ta1 = torch.tensor([1.0 - float(np.cos(np.deg2rad(ta))) for _, ta in thresholds], dtype=dt, device=dev)
    row = []
    for d2, term in sides:
        row += [d2.double().mean(), term.double().mean()]
        hit = (d2[None, :] <= td2[:, None]) & (term[None, :] < ta1[:, None])
        row.append(hit.sum(dim=1).double() / max(d2.shape[0], 1))
    flat = torch.cat([t.reshape(-1) for t in row]).tolist()   # the one read-back
    T = len(thresholds)
    precision, recall = flat[2:2 + T], flat[4 + T:4 + 2 * T]
    fscore = [2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(precision, recall)]
    return dict(chamfer_pred_to_gt=flat[0], direction_pred_to_gt=flat[1], chamfer_gt_to_pred=flat[2 + T],
                direction_gt_to_pred=flat[3 + T], thresholds=thresholds, precision=precision, recall=recall, fscore=fscore)
