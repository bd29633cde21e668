"""The measured gradient step: shape of the reference's stage-1 loop body (``src/train_gaussians.py:96-181``) without
densification / logging / GUI -- lr schedule, render, losses, backward, [grad all-reduce], NaN guard, Adam."""
from __future__ import annotations

import contextlib
import os
from types import SimpleNamespace
from typing import List, NamedTuple, Optional

import torch

from . import optim as _optim
from .gaussian_renderer import _use_fused, _use_fused_hair, render, render_hair
from .optim import FusedAdam, collectives_on
from .parallel import FlatGradBucket
from .utils.loss_utils import l1_loss, or_loss, ssim

PIPE = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)


_ONES = {}


def _one_like(loss):
    """A cached scalar 1 to seed backward() with (saves autograd's ones_like fill kernel on every view)."""
    key = (loss.device, loss.dtype)
    one = _ONES.get(key)
    if one is None:
        one = _ONES[key] = torch.ones((), device=loss.device, dtype=loss.dtype)
    return one


OVERLAP_ALL_REDUCE_WITH_ADAM = os.environ.get("GHR_OVERLAP_AR_ADAM", "1") != "0"
# One rank, fused path: the step's LAST projection backward applies the optimizer update itself (optim.FusedAdam.begin_fused_step)
FUSE_STRAND_ADAM = os.environ.get("GHR_FUSE_STRAND_ADAM", "1") != "0"  # strand stage: the SH features' update in the backward
FUSE_ADAM_INTO_BACKWARD = os.environ.get("GHR_FUSE_ADAM", "1") != "0"
DEFER_GRAD_ZEROING = os.environ.get("GHR_DEFER_GRAD_ZEROING", "1") != "0"
# The views of an eligible step as one library call each on buffers allocated once (native_step; include/ghr.h, ghr_view_step)
# instead of render() + view_loss() + backward() through autograd: training_step(native=None) reads this, default off
NATIVE_STEP_ENV = "GHR_NATIVE_STEP"
_LAST_STEP_PATH = "python"
CACHE_GT_SSIM_STATS = True  # keep the SSIM window moments of every camera's ground truth (2*3*H*W floats per camera)


def _gt_stats(cam, gt_image, gt_mask, mask_colours):
    """Ground truth and mask are constants of a training view: their SSIM window moments are computed once per camera
    (fused_loss.gt_ssim_stats) and re-used until either tensor is replaced or written."""
    if not CACHE_GT_SSIM_STATS:
        return None
    key = (gt_image._version, gt_mask._version, bool(mask_colours))
    cached = getattr(cam, "_ghr_gt_stats", None)
    # the entry holds the two tensors themselves: identity (not an address that the allocator may hand out again)
    if cached is None or cached[0] is not gt_image or cached[1] is not gt_mask or cached[2] != key:
        from .fused_loss import gt_ssim_stats
        cached = (gt_image, gt_mask, key, gt_ssim_stats(gt_image, gt_mask, mask_colours))
        try:
            cam._ghr_gt_stats = cached
        except AttributeError:
            pass
    return cached[3]


def view_loss(render_pkg, cam, opt, fused=None, scale: float = 1.0):
    """train_gaussians.py:113-140.  On a ROCm device all four terms run as one fused HIP op."""
    image, mask = render_pkg["render"], render_pkg["mask"]
    gt_image, gt_mask = cam.original_image, cam.original_mask
    if fused is None:
        fused = image.is_cuda
    if fused and getattr(render_pkg, "renders_packed", None) is not None:
        # one HIP op on the rasterizer's packed [10,H,W] output, orientation term included (orient_weight =
        # ones_like(gt_mask[:1]) * gt_orient_conf, train_gaussians.py:130)
        from .fused_loss import stage1_loss
        # `scale` (1/V of a V-view batch) is folded into the weights: no separate elementwise kernels around the loss
        return stage1_loss(render_pkg.renders_packed, gt_image, gt_mask, cam.original_orient_angle,
                           cam.original_orient_conf, opt.lambda_dl1 * scale, opt.lambda_dssim * scale,
                           opt.lambda_dmask * scale, opt.lambda_dorient * scale,
                           gt_stats=_gt_stats(cam, gt_image, gt_mask, True))
    if fused and opt.lambda_dorient == 0.0:
        from .fused_loss import photometric_loss
        return photometric_loss(image, mask, gt_image, gt_mask, opt.lambda_dl1 * scale, opt.lambda_dssim * scale,
                                opt.lambda_dmask * scale)
    Ll1 = l1_loss(image, gt_image, mask=gt_mask[1:].detach())
    Lssim = 1.0 - ssim(image * gt_mask[1:], gt_image * gt_mask[1:])
    Lmask = l1_loss(mask, gt_mask)
    loss = Ll1 * opt.lambda_dl1 + Lssim * opt.lambda_dssim + Lmask * opt.lambda_dmask
    if opt.lambda_dorient != 0.0:
        w = torch.ones_like(gt_mask[:1]) * cam.original_orient_conf
        Lorient = or_loss(render_pkg["orient_angle"], cam.original_orient_angle, render_pkg["orient_conf"], weight=w,
                          mask=gt_mask[:1])
        # train_gaussians.py:133: `if torch.isnan(Lorient).any(): Lorient = torch.zeros_like(Ll1)` -- a host decision that
        # drops the term from the graph.  Masking the VALUE (torch.where) would still back-propagate 0/0 through a view
        # whose orientation weights are all zero and poison the other three terms' step.
        if bool(torch.isnan(Lorient).any()):
            Lorient = torch.zeros_like(Ll1)
        loss = loss + Lorient * opt.lambda_dorient
    return loss * scale if scale != 1.0 else loss


_SIDE_STREAMS = {}
_NO_STREAM = contextlib.nullcontext()  # (a view on the current stream)


@contextlib.contextmanager
def _view_streams(device, n_streams, sink, n_views):
    """The streams the views of a step run on: yields (the current stream or None, one stream context per view).  With
    ``n_streams`` > 1 the views alternate on that many side streams, forked off the current one and joined to it at the end, and
    the optimizer chains their accumulating kernels meanwhile (FusedAdam.set_concurrent); otherwise every view stays put."""
    if n_streams <= 1:
        yield None, [_NO_STREAM] * n_views
        return
    key = (device.index, n_streams)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = [torch.cuda.Stream(device=device) for _ in range(n_streams)]
    main, side = torch.cuda.current_stream(device), _SIDE_STREAMS[key]
    for s in side:
        s.wait_stream(main)  # parameters as the previous optimizer step left them
    sink.set_concurrent(True)
    try:
        yield main, [torch.cuda.stream(side[i % n_streams]) for i in range(n_views)]
    finally:
        sink.set_concurrent(False)
        for s in side:
            main.wait_stream(s)


def _views_forward_backward(gaussians, cams, background, opt, V, pipe, n_streams, sink, last_pipe=None):
    """render + loss + backward of every view; returns (detached losses, instance counts [int | PendingCount]).
    ``last_pipe``: the pipe of the step's LAST view (it may carry the fused optimizer update)."""
    losses, counts = [], []
    pipes = [pipe] * len(cams)
    if last_pipe is not None and cams:
        pipes[-1] = last_pipe
    with _view_streams(background.device, n_streams, sink, len(cams)) as (main, on_stream):
        for cam, pipe, ctx in zip(cams, pipes, on_stream):
            with ctx:
                pkg = render(cam, gaussians, pipe, background)
                loss = view_loss(pkg, cam, opt, scale=1.0 / V)
                loss.backward(gradient=_one_like(loss))
                _generic_densify_stats(gaussians, pkg, pipe)
                ld = loss.detach()
                if main is not None:
                    ld.record_stream(main)
                losses.append(ld)
                counts.append(getattr(pkg, "count", None))
    return losses, counts


@torch.no_grad()
def _generic_densify_stats(gaussians, pkg, pipe):
    """pipe.densify_stats on a view whose backward pass did not keep the statistics itself (generic path): the reference's
    PyTorch form (train_gaussians.py:161-165)."""
    if getattr(pipe, "densify_stats", False) and not getattr(pkg, "densify_stats_done", False):
        vis = pkg["visibility_filter"]
        gaussians.update_max_radii(pkg["radii"], vis)
        gaussians.add_densification_stats(pkg["viewspace_points"], vis)


class _StepPlan(NamedTuple):
    """What one training_step is going to do (_plan_step): decided once, before anything is opened on the optimizer."""
    V: int                       # every view's loss is scaled 1 / V
    sink: Optional[FusedAdam]    # the optimizer, where the fused backward may store its gradients itself
    fused_sink: bool             # ... and this step's configuration lets it
    all_direct: bool             # every view of this rank goes through that direct backward
    n_streams: int               # HIP streams the views alternate on (0: the current one)
    defer: bool                  # no view waits for its instance count
    fuse: bool                   # the last backward is to carry the update -- if the optimizer agrees (_open_step)
    factored: Optional[str]      # SH gradients as per-view tables: None, "gathered" over the ranks, or this rank's "own" fold
    slots: int                   # view slots per rank of the gathered form
    run_pipe: SimpleNamespace    # the pipe of the views; last_pipe: of the view that carries the update
    last_pipe: Optional[SimpleNamespace]


def _fused_adam(gaussians) -> Optional[FusedAdam]:
    o = getattr(gaussians, "optimizer", None)
    return o if isinstance(o, FusedAdam) else None


def _plan_step(gaussians, cams, background, bucket, global_views, pipe, streams, defer_counts, densify_stats, fuse_adam,
               views_per_rank) -> _StepPlan:
    """The decisions of a step and nothing else: no call that changes the optimizer."""
    # the loss of a view is scaled 1 / V: with more than one rank V defaults to the GLOBAL number of views (the
    # all-reduce sums the ranks' gradients), assuming every rank holds len(cams) of them
    V = global_views or len(cams) * _world_size()
    sink = _fused_adam(gaussians)
    if sink is not None and sink.direct_grads:
        # the direct backward needs every leaf of the fused renderer inside the optimizer (e.g. train_orient_conf = False
        # leaves _orient_conf out): otherwise autograd accumulates and the scanning guard applies -- a property of the
        # configuration, identical on every rank
        leaves = (gaussians._xyz, gaussians._scaling, gaussians._rotation, gaussians._opacity, gaussians._label,
                  gaussians._orient_conf, gaussians._features_dc, gaussians._features_rest)
        if not all(isinstance(p, torch.nn.Parameter) and p.grad is not None for p in leaves):
            sink = None
    fused_sink = (sink is not None and sink.direct_grads and background.is_cuda and not getattr(pipe, "debug", False))
    n_streams = (2 if streams is None else int(streams)) if fused_sink and len(cams) > 1 else 0
    # every view of this step goes through the fused renderer's direct backward (render() decides per camera: a camera
    # whose tensors require grad takes the generic path, whose gradients arrive through autograd)
    all_direct = bool(fused_sink and cams and all(_use_fused(gaussians, pipe, c) for c in cams))
    defer = fused_sink and (True if defer_counts is None else bool(defer_counts))
    run_pipe = pipe
    if defer or densify_stats:
        run_pipe = SimpleNamespace(**{**vars(pipe), "defer_count": bool(defer), "densify_stats": bool(densify_stats)})
    # (the fused update leaves the gradient buffer undefined, like zero_grad="defer": not for callers who switched that off)
    fuse = (FUSE_ADAM_INTO_BACKWARD and DEFER_GRAD_ZEROING if fuse_adam is None else bool(fuse_adam)) and all_direct and \
        bool(cams) and not collectives_on() and bucket is None
    # Data-parallel steps of few views send the SH gradients -- 48 of the 61 floats per Gaussian -- in factored form: every view's
    # backward leaves its dL/d(rgb) table (12 B per Gaussian) in a slot of the optimizer, the ranks all-gather the slots and each
    # rebuilds the f_dc / f_rest gradients (optim.FusedAdam.begin_factored_views).  The choice decides the sequence of
    # collectives: it depends on the configuration and on the GLOBAL number of views only, never on this rank's cameras.
    slots = int(views_per_rank) if views_per_rank else -(-V // max(_world_size(), 1))
    factored = None
    if (collectives_on() and fused_sink and OVERLAP_ALL_REDUCE_WITH_ADAM and bucket is None and _optim.FACTORED_SH_REDUCE and
            0 < slots * _world_size() <= _optim.FACTORED_SH_MAX_VIEWS and sink.can_factor_views()):
        factored = "gathered"
    elif (all_direct and bucket is None and _optim.FACTORED_SH_REDUCE and sink.can_factor_views() and
          len(cams) >= (3 if fuse else 2) and (not collectives_on() or OVERLAP_ALL_REDUCE_WITH_ADAM)):
        # one rank, or too many views in all for the gathered form: the rank folds ITS views' tables into the flat gradient
        # once (before the sums / the update; before the last view's backward when that one carries the update) and every other
        # view's backward skips the read-modify-write of 192 B of SH gradients per Gaussian (4 views per rank through the
        # collective branch: 2.74 -> 2.45 ms, profiles/r06k).  A rank's own choice: the sequence of collectives is the plain one.
        factored = "own"
    last_pipe = SimpleNamespace(**{**vars(run_pipe), "fuse_adam": True}) if fuse else None
    return _StepPlan(V, sink, fused_sink, all_direct, n_streams, defer, fuse, factored, slots, run_pipe, last_pipe)


def _open_step(plan: _StepPlan, gaussians, cams) -> bool:
    """Opens the planned step on the optimizer, in this order.  Returns whether the last backward carries the update."""
    sink, o = plan.sink, _fused_adam(gaussians)
    if o is not None and not plan.all_direct:
        # the previous step may have left the gradient buffer undefined (zero_grad="defer" below): only a fused backward
        # redefines it -- a rank without views, or the generic / autograd path, needs the zeros the eager step leaves
        o.resolve_deferred()
    if sink is not None:
        sink.end_factored_views()  # (a step that died between its backwards and its update)
    if plan.factored == "gathered":
        if len(cams) > plan.slots:
            raise RuntimeError("training_step: %d views on this rank, %d view slots per rank (%d global views on %d ranks): "
                               "pass views_per_rank = the largest number of views any rank holds, on every rank" %
                               (len(cams), plan.slots, plan.V, _world_size()))
        sink.begin_factored_views(plan.slots, sh_degree=int(gaussians.active_sh_degree))
    elif plan.factored == "own":
        sink.begin_factored_views(len(cams), gather=False, sh_degree=int(gaussians.active_sh_degree))
    fuse = plan.fuse
    if fuse:
        sink.cancel_skip()  # (as in _update: every backward of this step runs after any earlier surgery)
        fuse = sink.can_fuse_step()
    if fuse:
        sink.begin_fused_step()
    return fuse


def _redo_overflowed_step(plan: _StepPlan, gaussians, cams, background, opt, pipe, densify_stats, overflow, fused_done):
    """A guessed capacity was too small: that view's image, loss and gradients are garbage (memory-safe garbage).
    Drops everything this step accumulated and redoes it with blocking, exactly sized forwards."""
    plan.sink.abort_step(fused_update_undone=fused_done)  # (the overflowed views raised the step's flag)
    # (densify_stats: an overflowed view's backward pass left the statistics alone -- k_project_bwd checks the count on the
    # device -- but the step's OTHER views have been counted, and ALL views are recomputed below: theirs would be counted twice)
    if densify_stats and len(cams) > 1 and not all(overflow):
        raise RuntimeError("training_step(densify_stats=True): a capacity guess overflowed in a multi-view step; the "
                           "statistics of its other views cannot be rolled back -- use defer_counts=False for the first "
                           "step after the scene has grown")
    redo_pipe = SimpleNamespace(**{**vars(pipe), "densify_stats": True}) if densify_stats else pipe
    return _views_forward_backward(gaussians, cams, background, opt, plan.V, redo_pipe, 0, plan.sink)[0]


def _update(plan: _StepPlan, gaussians, cams, bucket):
    """The step's end when no backward carried the update: [gradient collectives], NaN guard, Adam."""
    o = _fused_adam(gaussians)
    if o is not None:
        # Every backward of this step ran AFTER any earlier optimizer surgery (densification / opacity reset between two
        # calls), so all groups hold fresh gradients: the "parameters replaced since the last backward" marks never apply
        # here, whichever path produced the gradients (generic pipe, autograd accumulation, a rank without views).  They
        # only matter for a hand-written loop that runs backward -> surgery -> step (the reference's order), which calls
        # optimizer.step() itself.  Unconditional, hence identical on every rank.
        o.cancel_skip()
        # SH bands above the active degree carry exactly-zero gradients on every rank: not part of the all-reduce
        o.active_rest_coeffs = (int(gaussians.active_sh_degree) + 1) ** 2 - 1
        # grads already live in the optimizer's flat buffer; NaN guard + Adam + grad zeroing are one HIP pass
        # every view's gradients went through the fused renderer's direct backward (which keeps the NaN flag) and no
        # other rank contributes: the guard needs no scan over the gradients
        direct_local = o.direct_backwards == len(cams)
        # On the fused path the next training_step's first backward ASSIGNS the whole gradient buffer, so the Adam pass
        # need not zero it (an eighth of its traffic): FusedAdam.step(zero_grad="defer").  Anything else that touches the
        # buffer first either gets the zeros (resolve_deferred) or fails loudly (optim.py).
        zg = "defer" if (plan.all_direct and direct_local and DEFER_GRAD_ZEROING) else True
        # The choice below must be the same on every rank (it decides the sequence of collectives): it only depends on
        # the configuration (`fused_sink`), and a rank whose gradients did not all come through the direct backward
        # fails loudly instead of silently taking the other branch.
        if collectives_on() and plan.fused_sink and OVERLAP_ALL_REDUCE_WITH_ADAM:
            if not direct_local:
                raise RuntimeError("training_step: %d of %d views went through the fused backward on this rank" %
                                   (o.direct_backwards, len(cams)))
            # all-reduce in chunks, each chunk's Adam update as soon as its sum is there (FusedAdam.step_chunked)
            o.step_chunked(chunks=4, zero_grad=zg, reduce=True)
        else:
            o.all_reduce()
            o.step(zero_grad=zg, nan_scan=not (direct_local and not collectives_on()))
        return
    if bucket is not None:
        bucket.all_reduce()
        bad = bucket.has_nan()
    else:
        bad = torch.stack([p.grad.isnan().any() for p in gaussians.leaf_parameters() if p.grad is not None]).any()
    # train_gaussians.py:174-181: a NaN anywhere skips the update -- the reference drops the gradients
    # (zero_grad(set_to_none=True)), so optimizer.step() touches nothing: no moment decay, no step count.
    # One host decision per step, like the reference's `if torch.isnan(...)` (the torch.optim.Adam path is not the measured
    # one; round 2's clone-everything-and-restore variant tripled the optimizer traffic and still synchronised on Adam's
    # CPU-resident step counters).
    if bool(bad):
        print('NaN during backprop was found, skipping iteration...')
        if bucket is not None:
            # the gradients alias the bucket and cannot be dropped to None: a step over zeroed gradients would still decay
            # the moments and move the parameters by lr m / sqrt(v) -- skip the whole step, as the reference's does in effect
            bucket.zero()
            return
        gaussians.optimizer.zero_grad(set_to_none=True)
    gaussians.optimizer.step()
    if bucket is not None:
        bucket.zero()
    else:
        gaussians.optimizer.zero_grad(set_to_none=True)


def training_step(gaussians, cams: List, background, opt, iteration: int, bucket: Optional[FlatGradBucket] = None,
                  global_views: Optional[int] = None, pipe=PIPE, streams: Optional[int] = None,
                  defer_counts: Optional[bool] = None, densify_stats: bool = False, fuse_adam: Optional[bool] = None,
                  views_per_rank: Optional[int] = None, camera_bank=None, native: Optional[bool] = None):
    """One global gradient step over this rank's views.  Returns the (detached) summed local loss.

    ``streams`` (default 2 with the fused path and more than one view): the views of the step are independent given
    the parameters, so consecutive views run on alternating HIP streams -- the next view's projection / binning /
    compositing / loss fills the CUs the current view's VALU-bound backward leaves idle and vice versa (measured
    3.38 -> 3.08 ms for the 4-view step).  Only the kernels that add into the shared flat gradient buffer are
    chained (FusedAdam.open_view / close_view); the optimizer step waits for every stream.

    ``defer_counts`` (default on with the fused path): no view waits for its ``num_rendered`` -- the forward runs with
    the capacity guessed from the previous frame and the counts are checked once, after everything is queued (the host
    never blocks inside the step: 3.10 -> 2.92 ms).  If a count exceeded its capacity the accumulated gradients are
    dropped and the step is recomputed view by view with exact capacities, so the result never depends on the guess.

    ``densify_stats``: every view's backward pass also keeps the per-iteration densification statistics of the stage-1 loop
    (``max_radii2D``, ``xyz_gradient_accum``, ``denom``: src/train_gaussians.py:161-165, half of the iterations of a run) --
    inside ``k_project_bwd`` on the fused path (no extra launch); ``densification_step(..., stats_done=True)`` then only
    densifies / prunes at its interval.  Views that take the generic path get the PyTorch form.

    ``fuse_adam`` (default on: one rank, every view on the fused path): the step's last ``k_project_bwd`` applies the Adam
    update from the gradients it holds in registers (``ghr_adam_fuse``): no 244 B of gradient per Gaussian written and read
    back, no separate optimizer pass.  Same parameters, bit for bit, as the separate pass; the NaN rule stays exact (the
    update is undone on the device when the step's flag is up).  After such a step ``p.grad`` still holds what the previous
    separate pass left there (``zero_grad="defer"`` semantics: undefined) -- pass ``fuse_adam=False`` to log gradient norms.

    ``views_per_rank`` (more than one rank): the LARGEST number of views any rank holds in this step, the same value on every
    rank; default ceil(global views / ranks), which is what ``parallel.shard_views`` deals.  Steps of up to
    ``optim.FACTORED_SH_MAX_VIEWS`` view slots in all send the SH gradients as per-view dL/d(rgb) tables (12 B per Gaussian and
    view, all-gathered; ``FusedAdam.begin_factored_views``) instead of summing 192 B per Gaussian: every rank opens that many
    slots, and a rank with more views than slots fails loudly before any collective.

    ``camera_bank`` (a ``scene.cameras.CameraBank`` after ``training_setup``; on more than one rank a bank that every rank
    ``replicate()``-d: its ``step`` merges the ranks' gradient rows first, on every rank, also one without views -- a bank that was
    not replicated raises ``NotImplementedError`` there): the step's views are cameras of the bank
    and the cameras are trained with the Gaussians, in the reference's order (src/train_gaussians.py:183-196): every view's
    backward leaves dL/d(residuals) in its camera's gradient row, and after the Gaussians' update -- every stream of the step
    joined -- ``camera_bank.step(iteration)`` steps the viewed cameras in one launch.  The views must be DISTINCT cameras (their
    rows are then disjoint across the view streams): that is checked for the cameras of ANY bank among the views, with or without
    this argument.  From ``opt.iterations_cam`` on the bank composes constants for the duration of the step and the views take the
    constant-camera path.  A step that raises drops what its views left in their banks' gradient rows.

    ``native`` (default: ``GHR_NATIVE_STEP``, off): every view of the step is ONE library call (``ghr_view_step``: the six calls
    of render + loss + backward composed in C, the same kernels with the same arguments) on workspaces, planes and an argument
    struct that are allocated once (``native_step``), instead of two ``autograd.Function`` round trips, six calls and a dozen
    ``torch.empty`` per view.  Same parameters, moments, flags, statistics and loss, bit for bit.  Eligible is a step on one rank
    whose views all take the fused renderer's direct backward with deferred counts (the default of this function on a ROCm
    device), through constant cameras or cameras of a fused ``CameraBank`` on the model's device (while the bank trains such a view
    is ``ghr_view_step_camera``: compose, the view, the camera gradients' fold and the compose's backward in one call; no trained
    camera tensor, no ``TrainableCamera``, no bank with ``fused=False``), without ``pipe.debug``; streams, the per-view SH
    tables, ``densify_stats`` and the update inside the last backward work as they do here.  Anything else takes the path above
    untouched -- with ``native=True`` it raises instead.  A step without a capacity guess yet (the first one, or the first after
    the model changed size) has to wait for its instance count and runs the Python way, whatever ``native`` says;
    ``last_step_path()`` tells.  The returned scalar is a row of a ring of ``native_step.LOSS_RING`` steps, not a fresh tensor:
    clone it to keep it longer."""
    banks = _check_bank_views(camera_bank, cams)
    try:
        with contextlib.ExitStack() as scopes:
            for b in banks:  # (a bank that is only viewed, not stepped here, keeps its own notion of whether it trains)
                scopes.enter_context(b.step_scope(iteration if b is camera_bank else None))
            return _training_step(gaussians, cams, background, opt, iteration, bucket, global_views, pipe, streams, defer_counts,
                                  densify_stats, fuse_adam, views_per_rank, camera_bank, banks, native)
    finally:  # (the optimizer's view slots never outlive the step)
        o = getattr(gaussians, "optimizer", None)
        if hasattr(o, "end_factored_views"):
            o.end_factored_views()


def last_step_path() -> str:
    """``"native"`` when the views of the last ``training_step`` ran as ``ghr_view_step`` / ``ghr_view_step_camera`` calls,
    ``"python"`` otherwise."""
    return _LAST_STEP_PATH


def _native_views(native, plan, gaussians, cams, background, pipe, bucket, banks):
    """The model's ``native_step.NativeViews`` when this step's views are to run natively, else None."""
    forced = native is not None and bool(native)  # (the caller asked for it: an ineligible step is an error, not a fallback)
    if native is None:
        native = os.environ.get(NATIVE_STEP_ENV, "0") not in ("", "0")
    if not native:
        return None
    from . import native_step
    why = native_step.ineligible(plan, gaussians, cams, background, pipe, bucket, banks)
    if why is not None:
        if forced:
            raise RuntimeError("training_step(native=True): this step cannot take the native path: " + why)
        return None
    if not native_step.has_capacity_guess(gaussians, background):
        return None
    return native_step.NativeViews.for_model(gaussians, background.device)


def _training_step(gaussians, cams, background, opt, iteration, bucket, global_views, pipe, streams, defer_counts, densify_stats,
                   fuse_adam, views_per_rank, camera_bank, banks, native=None):
    global _LAST_STEP_PATH
    gaussians.update_learning_rate(iteration)
    plan = _plan_step(gaussians, cams, background, bucket, global_views, pipe, streams, defer_counts, densify_stats,
                      fuse_adam, views_per_rank)
    nv = _native_views(native, plan, gaussians, cams, background, pipe, bucket, banks)
    _LAST_STEP_PATH = "python" if nv is None else "native"
    fuse = _open_step(plan, gaussians, cams)
    native_total = None
    try:
        if nv is not None:
            losses, counts, native_total = nv.views_forward_backward(gaussians, cams, background, opt, plan, fuse, densify_stats)
        else:
            losses, counts = _views_forward_backward(gaussians, cams, background, opt, plan.V, plan.run_pipe, plan.n_streams,
                                                     plan.sink, plan.last_pipe if fuse else None)
    finally:
        fused_done = plan.sink.end_fused_step() if fuse else False
    overflow = [c.resolve()[1] for c in counts if hasattr(c, "resolve")]  # resolve every one: they feed the next guess
    if any(overflow):
        for b in banks:  # (the views run again: their camera gradients must not be added a second time)
            b.discard_gradients()
        losses = _redo_overflowed_step(plan, gaussians, cams, background, opt, pipe, densify_stats, overflow, fused_done)
        fused_done = False
        native_total = None
    if native_total is not None:  # (summed in place: a native step allocates nothing)
        total = native_total
    elif not losses:  # a rank without views in this step still takes part in the collectives and the update
        total = torch.zeros((), device=background.device)
    else:
        total = losses[0] if len(losses) == 1 else torch.stack(losses).sum()
    if not fused_done:  # (otherwise the last view's backward carried the update: k_adam_v4 does not run)
        _update(plan, gaussians, cams, bucket)
    if camera_bank is not None:
        camera_bank.step(iteration)
    return total


def _check_bank_views(bank, cams):
    """The banks among a step's views (``bank``, the one to be stepped, first).  Views that are cameras of a bank must be DISTINCT
    cameras of it, whether the step also steps that bank or not: two views of one camera would read-modify-write the same gradient
    row and touched mark from two streams.  With ``bank``: every view is a camera of it; on more than one rank it must be a
    replicated bank (``CameraBank.replicate``: its ``step`` merges the ranks' gradient rows first)."""
    if bank is not None and _world_size() > 1 and not getattr(bank, "replicated", False):
        raise NotImplementedError("training_step(camera_bank=...) on more than one rank: replicating the camera updates across "
                                  "ranks is not implemented for a bank that was not replicated (CameraBank.replicate)")
    banks, seen = ([] if bank is None else [bank]), set()
    for c in cams:
        b = getattr(c, "bank", None)
        if bank is not None and b is not bank:
            raise ValueError("training_step(camera_bank=...): every view must be a camera of that bank (bank[i])")
        if b is None:
            continue
        if (id(b), c.index) in seen:
            raise ValueError("training_step: the views of one step must be distinct cameras of their bank (row %d twice): two "
                             "views of one camera would write the same gradient row from two streams" % c.index)
        seen.add((id(b), c.index))
        if not any(b is x for x in banks):
            banks.append(b)
    return banks


@torch.no_grad()
def densification_step(gaussians, render_pkg, opt, iteration: int, cameras_extent: float,
                       white_background: bool = False, generator=None, stats_done: Optional[bool] = None):
    """The densification block of the stage-1 loop (src/train_gaussians.py:158-171), to be called between
    ``loss.backward()`` and the optimizer step of an iteration: image-space radius tracking, gradient statistics,
    densify_and_prune every ``densification_interval`` and the periodic opacity reset.  Under data parallelism every
    rank must call it with identical statistics (``parallel.all_reduce_densification_stats``) and the same
    ``generator`` seed so the replicas stay bit-identical."""
    if iteration >= opt.densify_until_iter:
        return False
    # ``stats_done`` (default: what the package says): this iteration's statistics were kept by the fused backward pass
    # (pipe.densify_stats / training_step(densify_stats=True)); ``render_pkg`` may then be None
    if stats_done is None:
        stats_done = bool(getattr(render_pkg, "densify_stats_done", False))
    if not stats_done:
        vis, radii = render_pkg["visibility_filter"], render_pkg["radii"]
        gaussians.update_max_radii(radii, vis)
        gaussians.add_densification_stats(render_pkg["viewspace_points"], vis)
    changed = False
    if iteration > opt.densify_from_iter and iteration % opt.densification_interval == 0:
        size_threshold = 20 if iteration > opt.opacity_reset_interval else None
        gaussians.densify_and_prune(opt.densify_grad_threshold, 0.005, cameras_extent, size_threshold,
                                    generator=generator)
        changed = True
    if iteration % opt.opacity_reset_interval == 0 or (white_background and iteration == opt.densify_from_iter):
        gaussians.reset_opacity()
    return changed


def strand_view_loss(render_pkg, cam, opt, fused=None, scale: float = 1.0):
    """The image terms of the strand-stage loss (src/train_strands.py:121-138): L1 and SSIM on the WHOLE image, mask L1, the
    orientation loss weighted by the ground-truth confidence.  The prior term ``Lsds * lambda_dsds`` (:139-147) does not depend
    on the view: ``strand_training_step`` adds it once per step when the strand model has a prior attached
    (``GaussianModelStrands.attach_prior``, strand_prior.py) -- its two networks are the prior's callables."""
    image, mask = render_pkg["render"], render_pkg["mask"]
    gt_image, gt_mask = cam.original_image, cam.original_mask
    if fused is None:
        fused = image.is_cuda
    if fused and getattr(render_pkg, "renders_packed", None) is not None and opt.train_orient_conf:
        from .fused_loss import stage1_loss
        w_conf = cam.original_orient_conf if opt.use_gt_orient_conf else torch.ones_like(gt_mask[:1])
        return stage1_loss(render_pkg.renders_packed, gt_image, gt_mask, cam.original_orient_angle, w_conf,
                           opt.lambda_dl1 * scale, opt.lambda_dssim * scale, opt.lambda_dmask * scale,
                           opt.lambda_dorient * scale, mask_colours=False,
                           gt_stats=_gt_stats(cam, gt_image, gt_mask, False))
    loss = l1_loss(image, gt_image) * opt.lambda_dl1 + (1.0 - ssim(image, gt_image)) * opt.lambda_dssim + \
        l1_loss(mask, gt_mask) * opt.lambda_dmask
    if opt.lambda_dorient != 0.0:
        w = torch.ones_like(gt_mask[:1])
        if opt.use_gt_orient_conf:
            w = w * cam.original_orient_conf
        conf = render_pkg["orient_conf"] if opt.train_orient_conf else None
        Lorient = or_loss(render_pkg["orient_angle"], cam.original_orient_angle, conf, weight=w, mask=gt_mask[:1])
        if bool(torch.isnan(Lorient).any()):  # train_strands.py:141: the term is dropped from the graph
            Lorient = torch.zeros_like(loss)
        loss = loss + Lorient * opt.lambda_dorient
    return loss * scale if scale != 1.0 else loss


def strand_training_step(gaussians, gaussians_hair, cams: List, background, opt, iteration: int, pipe=PIPE):
    """One iteration of the strand stage (src/train_strands.py:98-160): rebuild the strand Gaussians from the strand
    parameters, render head + hair, loss, backward, NaN guard on the strand parameters, Adam.  With a prior attached to the
    strand model the step's first rebuild computes ``Lsds`` and ``Lsds * opt.lambda_dsds`` joins the first view's loss, whole
    (not divided by the number of views); the term has no NaN drop (the reference has none): a NaN reaches ``_dirs.grad`` and
    the step is skipped by the guard below.  A collision term attached to the strand model (``attach_collision``) joins the same
    way as ``Lpen * opt.lambda_dpen`` -- only when ``opt.lambda_dpen`` is there and not 0: otherwise it is not evaluated.  A shape
    term (``attach_shape``, strand_shape.py) likewise, as ``Lshape * opt.lambda_dshape``."""
    use_sds = bool(getattr(gaussians_hair, "use_sds", False))
    attached = getattr(gaussians_hair, "collision", None) is not None
    use_pen = attached and getattr(opt, "lambda_dpen", 0.0) != 0
    shaped = getattr(gaussians_hair, "shape", None) is not None
    use_shape = shaped and getattr(opt, "lambda_dshape", 0.0) != 0
    first = {}
    if attached:
        first["collision"] = use_pen
    if shaped:
        first["shape"] = use_shape
    gaussians_hair.initialize_gaussians_hair(**first)
    gaussians_hair.update_learning_rate(iteration)
    V = len(cams)
    losses = []
    # One view, FusedAdam, the fused render_hair path: the optimizer update of the SH features (48 of the 52 floats per strand
    # Gaussian) rides in the projection backward (ghr_adam_fuse, strand segment): no 192 B of gradient per Gaussian written
    # for an Adam pass to read back.  The strand directions' and the confidence's gradients arrive through autograd after
    # that kernel; they are stepped -- and their NaN mark is added to the step's flag -- before the step is finished on the
    # device (FusedAdam.finish_fused_step_with_late_groups), which undoes everything when the flag is up.
    o = _fused_adam(gaussians_hair)
    fuse = bool(FUSE_STRAND_ADAM and o is not None and V == 1 and o.direct_grads and o.can_fuse_step() and
                not getattr(pipe, "debug", False) and _use_fused_hair(gaussians, gaussians_hair, pipe, cams[0]) and
                all(g["name"] in ("xyz", "f_dc", "f_rest", "orient_conf") for g in o.param_groups))
    run_pipe = pipe
    if fuse:
        o.resolve_deferred()
        o.begin_fused_step()
        run_pipe = SimpleNamespace(**{**vars(pipe), "fuse_adam": True})
    fused_done = False
    try:
        for view, cam in enumerate(cams):
            pkg = render_hair(cam, gaussians, gaussians_hair, run_pipe, background)
            loss = strand_view_loss(pkg, cam, opt, scale=1.0 / V)
            if use_sds and view == 0:
                loss = loss + gaussians_hair.Lsds.to(loss.dtype) * opt.lambda_dsds
            if use_pen and view == 0:
                loss = loss + gaussians_hair.Lpen.to(loss.dtype) * opt.lambda_dpen
            if use_shape and view == 0:
                loss = loss + gaussians_hair.Lshape.to(loss.dtype) * opt.lambda_dshape
            loss.backward(gradient=_one_like(loss))
            losses.append(loss.detach())
            if cam is not cams[-1]:  # a fresh graph for the next view (the prior's term is in the first view's already)
                if use_sds or attached or shaped:
                    gaussians_hair.initialize_gaussians_hair(prior=False)
                else:
                    gaussians_hair.initialize_gaussians_hair()
        if fuse and o.fused_update_launched:
            o.finish_fused_step_with_late_groups([g["name"] for g in o.param_groups if g["name"] not in ("f_dc", "f_rest")])
    finally:
        if fuse:
            fused_done = o.end_fused_step(grads_zero=True)
    if fused_done:
        return losses[0]
    if o is not None:
        if o.direct_backwards == V and V > 0:
            # every view's SH-feature gradients (48 of the 52 floats per Gaussian) were assigned by the fused backward, which
            # raised the optimizer's flag for any non-finite value it stored; what reached the remaining parameters through
            # autograd (strand directions, confidence: 4 of the 52 floats per Gaussian) is scanned here -- not everything
            o.scan_groups_for_nan([g["name"] for g in o.param_groups if g["name"] not in ("f_dc", "f_rest")])
            o.step(zero_grad=True, nan_scan=False)
        else:
            o.step(zero_grad=True)  # device-side NaN guard: a scan over every strand parameter's gradient
    else:
        ps = [gaussians_hair._dirs, gaussians_hair._features_dc, gaussians_hair._features_rest]
        if any(p.grad is not None and bool(p.grad.isnan().any()) for p in ps):  # train_strands.py:151-155
            gaussians_hair.optimizer.zero_grad(set_to_none=True)
            print('NaN during backprop was found, skipping iteration...')
        gaussians_hair.optimizer.step()
        gaussians_hair.optimizer.zero_grad()
    return losses[0] if len(losses) == 1 else torch.stack(losses).sum()


def latent_view_loss(render_pkg, cam, opt, l_diff=None, fused=None):
    """The latent-strand stage's loss (src/train_latent_strands.py:130-152): L1 on the whole image, L1 on mask channel 0, the
    orientation loss and the generator's scalar ``l_diff`` (``gaussians_hair.LDiff``), each dropped when it is NaN; no SSIM.
    On a ROCm device the three image terms are one HIP op (csrc/ghr_latent.h); the generator's term and its NaN rule are added
    on a device scalar.  Nothing is read back.  (A dropped ``l_diff`` receives a ZERO cotangent here, not a cut graph: a generator
    whose backward turns 0 into NaN needs the form of ``latent_strand_training_step``.)"""
    image, mask = render_pkg["render"], render_pkg["mask"]
    gt_image, gt_mask = cam.original_image, cam.original_mask
    if fused is None:
        fused = image.is_cuda
    if fused and getattr(render_pkg, "renders_packed", None) is not None:
        from .fused_loss import latent_loss
        loss = latent_loss(render_pkg.renders_packed, cam, opt)
    else:
        LCE = l1_loss(mask[:1], gt_mask[:1])
        Ll1 = l1_loss(image, gt_image)
        w = torch.ones_like(gt_mask[:1])
        if opt.use_gt_orient_conf:
            w = w * cam.original_orient_conf
        conf = render_pkg["orient_conf"] if opt.train_orient_conf else None
        LOR = or_loss(render_pkg["orient_angle"], cam.original_orient_angle, conf, weight=w, mask=gt_mask[:1])
        # :143-145 decide on the host; here the flag stays on the device: value 0 and a zero cotangent for a NaN term
        zero = torch.zeros_like(Ll1)
        loss = _drop_nan(Ll1, zero) * opt.lambda_dl1 + _drop_nan(LCE, zero) * opt.lambda_dmask + \
            _drop_nan(LOR, zero) * opt.lambda_dorient
    if l_diff is not None:
        loss = loss + _drop_nan(l_diff.to(loss.dtype), torch.zeros_like(loss)) * getattr(opt, "lambda_dsds", 0.0)
    return loss


class _DropNan(torch.autograd.Function):
    """``x if not isnan(x) else zero`` of a scalar, with a zero gradient for a dropped x (train_latent_strands.py:143-146), decided
    on the device."""

    @staticmethod
    def forward(ctx, x, zero):
        bad = torch.isnan(x)
        ctx.save_for_backward(bad)
        return torch.where(bad, zero, x)

    @staticmethod
    def backward(ctx, g):
        (bad,) = ctx.saved_tensors
        return torch.where(bad, torch.zeros_like(g), g), None


def _drop_nan(x, zero):
    return _DropNan.apply(x, zero)


def latent_strand_training_step(gaussians, gaussians_hair, cams: List, background, opt, iteration: int, pipe=PIPE):
    """One iteration of the latent-strand stage (src/train_latent_strands.py:103-164): the generator's strands -> segment
    Gaussians, render head + hair, loss, backward, the NaN rule over the first parameter group, the caller's optimizer.
    ``cams`` holds the iteration's view (the reference draws one).  Returns the detached device loss; nothing is read back
    except by the reference's own NaN test on the gradients."""
    gaussians_hair.initialize_gaussians_hair(iteration)
    gaussians_hair.update_learning_rate(iteration)
    cam = cams[0]
    pkg = render_hair(cam, gaussians, gaussians_hair, pipe, background)
    loss = latent_view_loss(pkg, cam, opt)
    l_diff, o = gaussians_hair.LDiff, gaussians_hair.optimizer
    if l_diff is None:
        loss.backward(gradient=_one_like(loss))
    else:
        # :142, 146: the generator's term is dropped when it is NaN.  The reference decides on the host and cuts the graph; a
        # zero cotangent sent into a graph that made a NaN comes out as 0 * NaN.  So the term is differentiated on its own and
        # the select is made on its parameter gradients, on the device.
        w = float(getattr(opt, "lambda_dsds", 0.0))
        params = [q for g in o.param_groups for q in g['params'] if q.requires_grad]
        loss.backward(gradient=_one_like(loss), retain_graph=True)
        bad = torch.isnan(l_diff.detach())
        for q, g in zip(params, torch.autograd.grad(l_diff, params, allow_unused=True)):
            if g is not None:
                g = torch.where(bad, torch.zeros_like(g), g * w)
                q.grad = g if q.grad is None else q.grad.add_(g)
        loss = loss.detach() + torch.where(bad, torch.zeros_like(loss), l_diff.detach().to(loss.dtype)) * w
    if iteration < opt.iterations:
        for param in o.param_groups[0]['params']:  # :157-162, call for call
            if param.grad is not None and param.grad.isnan().any():
                o.zero_grad()
                print('NaN during backprop was found, skipping iteration...')
        o.step()
        o.zero_grad(set_to_none=True)
    return loss.detach()


def _world_size() -> int:
    import torch.distributed as dist
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


@torch.no_grad()
def make_ground_truth(gaussians_gt, cams: List, background, pipe=PIPE):
    """Synthetic supervision: render a (perturbed) model and attach the maps the loss reads (cameras.py fields)."""
    for cam in cams:
        pkg = render(cam, gaussians_gt, pipe, background)
        cam.original_image = pkg["render"].clamp(0, 1).detach()
        cam.original_mask = pkg["mask"].clamp(0, 1).detach()
        cam.original_orient_angle = pkg["orient_angle"].detach()
        cam.original_orient_conf = torch.ones_like(pkg["orient_conf"]).detach()
