"""The native view step: render + stage-1 loss + backward of one training view as ONE library call (``ghr_view_step``,
include/ghr.h) on buffers that are allocated once.  A view whose camera is a row of a training ``scene.cameras.CameraBank`` is
``ghr_view_step_camera``: the same call with the camera's compose in front and the fold of its gradients and the compose's
backward behind, as ``_BankCompose`` and ``fused._camera_grads`` chain them on the Python path.

``trainer.training_step(native=True)`` (or ``GHR_NATIVE_STEP=1``) routes the views of an eligible step through here instead of
through the two ``autograd.Function`` round trips of ``render()`` / ``view_loss()`` / ``backward()``: the same kernels with the
same arguments in the same order -- the library call is a composition of the six calls the Python path makes -- without a
dozen ``torch.empty``, the autograd graph and five of the six ctypes crossings per view.  What a view needs lives in a *slot*
per HIP stream the step's views run on (workspaces at the capacity guess, render and gradient planes, loss scratch) with one
filled ``ghr_view_step_args`` of which only the per-step and per-view fields are rewritten.

Everything about the step that is not the views -- plan, opening the optimizer, the update, the overflow recovery -- stays in
``trainer``; the optimizer's host-side bookkeeping (``FusedAdam``: known-zero gradients, view slots, the fused update, the event
chain around the shared gradient buffer) is driven through the same two calls as ``gaussian_renderer.fused`` drives it:
``FusedAdam.open_view`` / ``close_view``.
"""
from __future__ import annotations

import ctypes
import os
from typing import List, Optional

import torch

from . import _lib
from . import diff_gaussian_rasterization as _dgr
from .diff_gaussian_rasterization import PendingCount
from .gaussian_renderer import _tan_half
from .gaussian_renderer import fused as _fused

LOSS_RING = 256  # steps a returned loss scalar stays valid for (it is a row of a ring, not a fresh allocation)
# Slots a stream keeps: one per image size among the views, the least recently made dropped beyond this many.  A slot holds what
# the Python path allocates and frees per view -- geom / img / binning workspaces, the gradient lines (64 B per instance of
# capacity: ~0.5 GB at 2 M Gaussians), four image-sized planes -- for as long as the model lives.
MAX_SLOTS_PER_STREAM = 2
_MAX_VIEWS_INIT = 8


def _plain_f32(t) -> bool:
    return (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and
            not t.requires_grad)


class _CamFields:
    """Pointers of a constant camera and of its ground truth, remade when one of the tensors is replaced.  ``bank``: the camera is a
    row of this TRAINING bank -- it has no tensors of its own (the first three are None), the view composes them."""
    __slots__ = ("tensors", "ptrs", "W", "H", "bank", "fov")

    def __init__(self, tensors, W, H, bank, fov):
        self.tensors, self.W, self.H, self.bank, self.fov = tensors, W, H, bank, fov
        self.ptrs = tuple(None if t is None else t.data_ptr() for t in tensors)


def _cam_fields(cam, dev=None) -> Optional[_CamFields]:
    """None: this camera's view cannot take the native path (its tensors are trained leaves or composed per access by PyTorch, it
    belongs to a bank that is not fused or not on ``dev``, or its ground truth is not plain contiguous fp32 device data).  A camera
    of a fused bank is a constant camera while the bank does not train (``BankCamera.tensors()`` caches them then)."""
    bank = getattr(cam, "bank", None)
    live = None
    if bank is not None:
        if not bank.fused or (dev is not None and bank.params.device != dev):
            return None
        live = bank if (bank.live and bank.train_mask) else None
    elif hasattr(cam, "tensors"):
        return None
    try:
        gt = (cam.original_image, cam.original_mask, cam.original_orient_angle, cam.original_orient_conf)
        if live is not None:
            ts, fov = (None, None, None) + gt, None
        elif bank is not None:
            t = cam.tensors()
            ts, fov = (t[0], t[1], t[2]) + gt, (t[3], t[4])
        else:
            ts, fov = (cam.world_view_transform, cam.full_proj_transform, cam.camera_center) + gt, (cam.FoVx, cam.FoVy)
    except AttributeError:
        return None
    c = cam.__dict__.get("_ghr_native_fields")
    if c is not None and c.bank is live and all(a is b for a, b in zip(c.tensors, ts)):
        if live is not None:
            return c
        c.fov = fov
        # (the same tensors: still constants?  requires_grad_() does not replace the object)
        trained = ts[0].requires_grad or ts[1].requires_grad or ts[2].requires_grad or \
            any(isinstance(f, torch.Tensor) and f.requires_grad for f in fov)
        return None if trained else c
    W, H = int(cam.image_width), int(cam.image_height)
    if not all(_plain_f32(t) for t in ts if live is None or t is not None):
        return None
    if live is None:
        if any(isinstance(f, torch.Tensor) and f.requires_grad for f in fov):
            return None
        if ts[0].numel() != 16 or ts[1].numel() != 16 or ts[2].numel() != 3:
            return None
    if tuple(ts[3].shape) != (3, H, W) or tuple(ts[4].shape) != (2, H, W) or ts[5].numel() != H * W or ts[6].numel() != H * W:
        return None
    c = _CamFields(ts, W, H, live, fov)
    cam.__dict__["_ghr_native_fields"] = c
    return c


def _leaves(g):
    return (g._xyz, g._scaling, g._rotation, g._opacity, g._label, g._orient_conf, g._features_dc, g._features_rest)


def ineligible(plan, gaussians, cams, background, pipe, bucket, banks) -> Optional[str]:
    """Why this step cannot take the native path (None: it can).  Decided from the plan and the configuration only."""
    from .optim import collectives_on
    if not (plan.fused_sink and plan.all_direct and plan.defer):
        return "the step is not all on the fused renderer's direct backward with deferred counts"
    if gaussians._xyz.device != background.device:
        return "the model and the background are on different devices"
    if collectives_on() or bucket is not None:
        return "data-parallel steps take the Python path"
    if getattr(pipe, "debug", False):
        return "pipe.debug"
    if plan.factored == "gathered":
        return "gathered view tables"
    if not cams or gaussians._xyz.shape[0] == 0:
        return "no views / an empty model"
    if not torch.is_grad_enabled():
        return "grad mode is off"
    if not _fused._grads_in_place(_leaves(gaussians)):
        return "a parameter's .grad does not alias the optimizer's gradient buffer"
    dev = gaussians._xyz.device
    for c in cams:
        if _cam_fields(c, dev) is None:
            return ("a camera that is neither constant nor a camera of a fused bank on the model's device (a bank with "
                    "fused=False or on another device, a TrainableCamera, leaf tensors that require grad), or ground truth "
                    "that is not plain fp32 device data")
    return None


def has_capacity_guess(gaussians, background) -> bool:
    """A view needs a capacity for its binning workspace before its count is known: the guess the blocking path learns
    (``diff_gaussian_rasterization._R_HINT``).  Without one -- the first step, or the first after the model changed size -- the
    step runs the Python way, which waits for the count."""
    idx = background.device.index
    P = int(gaussians._xyz.shape[0])
    return bool(_dgr._R_HINT.get(idx)) and _dgr._R_P.get(idx, P) == P


class _Slot:
    """The buffers of the views that run on one stream, and their argument struct."""

    def __init__(self, dev, P, W, H, K):
        self.P, self.W, self.H, self.K = P, W, H, K
        f32 = dict(dtype=torch.float32, device=dev)
        gbytes, ibytes = _lib.forward_sizes(P, W, H, False)
        self.geom = torch.empty((gbytes,), dtype=torch.uint8, device=dev)
        self.img = torch.empty((ibytes,), dtype=torch.uint8, device=dev)
        self.img_complete = False  # through stage 1 AND stage 2 once: its counters are back at zero (ghr_model_args.img_ws_recycled)
        self.radii = torch.empty((P,), dtype=torch.int32, device=dev)
        self.means2D = torch.empty((P, 3), **f32)
        self.d_means2D = torch.empty((P, 3), **f32)
        self.render = torch.empty((_lib.NUM_CHANNELS, H, W), **f32)
        self.d_pix = torch.empty((_lib.NUM_CHANNELS, H, W), **f32)
        self.maps = torch.empty((9, H, W), **f32)
        self.sums = torch.empty(_lib.loss_sums_floats(W, H), **f32)
        self.cap, self.bin, self.scratch = None, None, None
        # a view through a training bank camera (ghr_view_step_camera): its composed row, its folded gradients, its partial table
        self.cam_slots = int(_lib.lib().ghr_camera_slots(P))
        self.out_row = torch.empty((_lib.CAMERA_OUT,), **f32)
        self.d_cam = torch.empty((_lib.CAM_GRADS,), **f32)
        self.cam_partial = torch.empty((_lib.CAM_PARTIALS, self.cam_slots), **f32)
        self.campos = self.out_row[48:51]
        c = self.cam_args = _lib.ViewCameraArgs()
        c.out_row, c.d_cam = self.out_row.data_ptr(), self.d_cam.data_ptr()
        c.const_stride = _lib.CAMERA_CONST
        a = self.args = _lib.ViewStepArgs()
        m = a.model
        m.P, m.W, m.H, m.sh_coeffs = P, W, H, K
        a.loss.W, a.loss.H = W, H
        a.geom_ws, a.img_ws = self.geom.data_ptr(), self.img.data_ptr()
        a.radii, a.means2D_out, a.d_means2D = self.radii.data_ptr(), self.means2D.data_ptr(), self.d_means2D.data_ptr()
        a.render, a.d_pix = self.render.data_ptr(), self.d_pix.data_ptr()
        a.maps, a.sums = self.maps.data_ptr(), self.sums.data_ptr()
        self.step_id = -1

    def set_camera(self, ptrs, bank, index):
        """Where the view's model reads its camera: the three constant tensors, or -- a training bank's row -- this slot's
        ``out_row``, with the partial table its backward fills."""
        m = self.args.model
        if bank is None:
            m.viewmatrix, m.projmatrix, m.campos = ptrs
            m.fovx_dev = m.fovy_dev = m.cam_partial = None
            m.cam_slots = 0
            return
        row = self.out_row.data_ptr()
        m.viewmatrix, m.projmatrix, m.campos = row, row + 4 * 16, row + 4 * 48
        m.fovx_dev, m.fovy_dev = row + 4 * 51, row + 4 * 52
        m.cam_partial, m.cam_slot0, m.cam_slots = self.cam_partial.data_ptr(), 0, self.cam_slots
        m.tan_fovx = m.tan_fovy = 1.0  # (ignored: the kernels take tan(FoV / 2) of the device scalars)
        c = self.cam_args
        c.parametrisation, c.rows, c.index = bank.parametrisation, len(bank), index
        c.consts, c.params, c.param_stride = bank.consts.data_ptr(), bank.params.data_ptr(), bank.width
        c.grads, c.grad_stride, c.touched, c.train_mask = bank.grads.data_ptr(), bank.width, bank.touched.data_ptr(), bank.train_mask

    def set_capacity(self, cap, dev):
        """Binning workspace and gradient lines on the capacity grid: re-made only when the guess moves to another grid point."""
        if cap != self.cap:
            self.bin = torch.empty((_lib.binning_size(cap, self.W, self.H),), dtype=torch.uint8, device=dev)
            self.scratch = torch.empty((max(int(cap), 1), _lib.GRAD_STRIDE), dtype=torch.float32, device=dev)
            self.cap = cap
            a = self.args
            a.R, a.bin_ws, a.grad_scratch = cap, self.bin.data_ptr(), self.scratch.data_ptr()


class NativeViews:
    """What the native views of one model need, allocated once (kept on the model: ``for_model``)."""

    def __init__(self, dev):
        self.dev = dev
        self.slots = {}
        self.one = torch.ones((), dtype=torch.float32, device=dev)
        self.pinned = None
        self.count_events: List[torch.cuda.Event] = []
        self.acc_events: List[torch.cuda.Event] = []
        self.ring = None
        self.ring_pos = 0
        self.step_id = 0
        self._ensure_views(_MAX_VIEWS_INIT)

    def __deepcopy__(self, memo):
        return None  # (a copied model makes its own: events and workspaces are not state)

    @staticmethod
    def for_model(gaussians, dev) -> "NativeViews":
        nv = gaussians.__dict__.get("_ghr_native_views")
        if nv is None or nv.dev != dev:
            nv = gaussians.__dict__["_ghr_native_views"] = NativeViews(dev)
        return nv

    @staticmethod
    def _event(stream):
        ev = torch.cuda.Event()
        ev.record(stream)  # (the handle exists from the first record on; the library records it again for every view)
        return ev

    def _ensure_views(self, n):
        """Per view position of a step: the pinned word its count lands in, the event behind its stage 1, the event behind its
        accumulating kernels; and the ring of loss rows."""
        if self.pinned is not None and len(self.count_events) >= n:
            return
        n = max(n, 2 * len(self.count_events))
        with torch.cuda.device(self.dev):
            stream = torch.cuda.current_stream(self.dev)
            stream.synchronize()  # (growing: nobody is still writing the words that are replaced)
            self.pinned = torch.zeros(n, dtype=torch.int32).pin_memory()
            self.count_events = [self._event(stream) for _ in range(n)]
            self.acc_events = [self._event(stream) for _ in range(n)]
            # a row: the views' losses from column 0 (16-B aligned, like a fresh tensor), their sum in the last column
            self.ring_width = (n + 1 + 3) // 4 * 4
            self.ring = torch.zeros((LOSS_RING, self.ring_width), dtype=torch.float32, device=self.dev)

    def _slot(self, stream_key, P, W, H, K):
        key = (stream_key, P, W, H, K)
        s = self.slots.get(key)
        if s is None:
            # (a model that changed size leaves its old slots behind: drop them, they hold workspaces of the old size; and a
            # stream keeps slots for MAX_SLOTS_PER_STREAM image sizes, the oldest going first -- dicts keep insertion order)
            mine = [k for k in self.slots if k[0] == stream_key]
            stale = [k for k in mine if k[1] != P or k[4] != K]
            keep = [k for k in mine if k not in stale]
            for k in stale + keep[:max(0, len(keep) - (MAX_SLOTS_PER_STREAM - 1))]:
                del self.slots[k]
            s = self.slots[key] = _Slot(self.dev, P, W, H, K)
        return s

    def views_forward_backward(self, gaussians, cams, background, opt, plan, fuse, densify_stats):
        """The native form of ``trainer._views_forward_backward``: returns (per-view loss scalars, PendingCounts, total loss)."""
        # every stream, event and launch below is the MODEL's device's (as gaussian_renderer.fused and optim guard their calls)
        with _dgr._on_device(self.dev):
            return self._views_forward_backward(gaussians, cams, background, opt, plan, fuse, densify_stats)

    def _views_forward_backward(self, gaussians, cams, background, opt, plan, fuse, densify_stats):
        from .trainer import _gt_stats, _view_streams
        sink, V, dev = plan.sink, plan.V, self.dev
        n = len(cams)
        self._ensure_views(n)
        self.step_id += 1
        leaves = _leaves(gaussians)
        P, K = int(leaves[0].shape[0]), 1 + int(leaves[7].shape[1])
        p_ptrs = [t.data_ptr() for t in leaves]
        g_ptrs = [t.grad.data_ptr() for t in leaves]
        bg = background if _plain_f32(background) else background.detach().float().contiguous()
        bg_ptr = bg.data_ptr()
        sh_degree = int(gaussians.active_sh_degree)
        eps = float(getattr(gaussians, "conic_eps", 1e-12))
        dens_ptrs = [t.data_ptr() for t in _fused.densify_stats_tensors(gaussians, P)] if densify_stats else None
        scale = 1.0 / V
        w = (opt.lambda_dl1 * scale, opt.lambda_dssim * scale, opt.lambda_dmask * scale, opt.lambda_dorient * scale)
        orient = float(w[3]) != 0.0
        cap = int(_dgr._R_HINT[dev.index])
        prezero = int(not os.environ.get("GHR_NO_PREZERO"))
        recycle = _fused.RECYCLE_IMG_WS
        row = self.ring[self.ring_pos]
        self.ring_pos = (self.ring_pos + 1) % LOSS_RING
        row_ptr = row.data_ptr()
        pinned_ptr = self.pinned.data_ptr()
        lib = _lib.lib()
        losses, counts = [], []
        with _view_streams(dev, plan.n_streams, sink, n) as (_, on_stream):
            for i, (cam, ctx) in enumerate(zip(cams, on_stream)):
                with ctx:
                    stream = _dgr._stream()
                    cf = _cam_fields(cam, dev)
                    slot = self._slot(stream.value or 0, P, cf.W, cf.H, K)
                    slot.set_capacity(cap, dev)
                    a = slot.args
                    m, l = a.model, a.loss
                    if slot.step_id != self.step_id:  # ---- what holds for every view of the step
                        slot.step_id = self.step_id
                        (m.xyz, m.log_scales, m.rotations, m.opacity_logit, m.label_logit, m.orient_conf_log, m.features_dc,
                         m.features_rest) = p_ptrs
                        (a.d_xyz, a.d_log_scales, a.d_rotations, a.d_opacity_logit, a.d_label_logit,
                         a.d_orient_conf_log) = g_ptrs[:6]
                        m.background, m.sh_degree, m.conic_eps, m.scale_modifier = bg_ptr, sh_degree, eps, 1.0
                        l.w_l1, l.w_ssim, l.w_mask, l.w_orient = w[0], w[1], w[2], (w[3] if orient else 0.0)
                        if dens_ptrs is not None:
                            m.dens_grad_accum, m.dens_denom, m.dens_max_radii2D = dens_ptrs
                        else:
                            m.dens_grad_accum = m.dens_denom = m.dens_max_radii2D = None
                        a.grad_loss, a.prezero = self.one.data_ptr(), prezero
                    # ---- this view: camera, ground truth (+ its cached SSIM moments), where its outputs go
                    pv, pp, pc, gi, gm, ga, gc = cf.ptrs
                    bank = cf.bank
                    slot.set_camera((pv, pp, pc), bank, getattr(cam, "index", None))
                    if bank is None:
                        m.tan_fovx, m.tan_fovy = _tan_half(cf.fov[0]), _tan_half(cf.fov[1])
                    l.gt_image, l.gt_mask = gi, gm
                    l.gt_orient_angle, l.gt_orient_conf = (ga, gc) if orient else (None, None)
                    stats = _gt_stats(cam, cf.tensors[3], cf.tensors[4], True)
                    l.gt_stats = stats.data_ptr() if stats is not None else None
                    m.img_ws_recycled = int(recycle and slot.img_complete)
                    a.R_host = pinned_ptr + 4 * i
                    a.loss_out = row_ptr + 4 * i
                    a.count_event = int(self.count_events[i].cuda_event)
                    # ---- the optimizer's side of a direct backward (the last view's applies the update of a fused step)
                    # (a bank camera's centre does not exist yet: the call composes it)
                    h = sink.open_view(bool(fuse) and i == n - 1, cf.tensors[2])
                    # a step whose LAST backward carries the update: every view checks its instance count on the device
                    m.dens_img_ws = a.img_ws if h.check_overflow or dens_ptrs is not None else None
                    m.overflow_raises_flag, m.adam_fuse = int(h.check_overflow), h.adam_fuse
                    a.accumulate, a.nan_flag, m.d_rgb = h.accumulate, h.nan_flag, h.d_rgb
                    a.d_features_dc, a.d_features_rest = (g_ptrs[6], g_ptrs[7]) if h.d_rgb is None else (None, None)
                    # the earlier views' tables are folded into the flat gradient first, inside the call
                    a.sh_fold = sink.fold_own_views_args() if h.fold else None
                    # concurrent views: only the kernels that add into the shared gradient buffer are ordered after the
                    # previous view's
                    acc_event = self.acc_events[i] if sink.concurrent else None
                    a.acc_wait_event = None if h.wait_event is None else int(h.wait_event.cuda_event)
                    a.acc_record_event = None if acc_event is None else int(acc_event.cuda_event)
                    if bank is None:
                        _lib.check(lib.ghr_view_step(stream, ctypes.byref(a)))
                    else:
                        _lib.check(lib.ghr_view_step_camera(stream, ctypes.byref(a), ctypes.byref(slot.cam_args)))
                        if h.d_rgb is not None:
                            # the centre behind the view's dL/d(rgb) table, now that it is composed; whoever folds the table
                            # waits for the event behind it
                            sink.write_view_campos(slot.campos)
                            if acc_event is not None:
                                acc_event.record()
                    slot.img_complete = True
                    sink.close_view(h, acc_event)
                    losses.append(row[i])
                    counts.append(PendingCount(self.pinned[i:i + 1], self.count_events[i], cap, dev.index, P))
        if n == 1:
            total = losses[0]
        else:
            total = row[self.ring_width - 1]
            torch.sum(row[:n], dim=0, out=total)
        return losses, counts, total
