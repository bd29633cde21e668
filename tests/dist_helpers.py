"""Shared pieces of the data-parallel GPU tests (tests/test_gpu_dist_shared.py, tests/test_gpu_dist_wide.py): G ranks
started with ``spawn`` that share cuda:0 over gloo, the synthetic scene they train on, and the capture of the reduced
gradient of a step."""
import queue
import socket
import time

import torch


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def scene_cameras(dev, views):
    """``views`` ring cameras of ``tiny_strands`` with the ground truth of a perturbed model attached, and the background."""
    from gaussianhaircut_amd.scene.cameras import ring_cameras
    from gaussianhaircut_amd.trainer import make_ground_truth
    from gaussianhaircut_amd.utils import synthetic as syn
    spec = syn.CONFIGS["tiny_strands"]
    gt = syn.make_model(spec, dev)
    with torch.no_grad():
        gt._features_dc.add_(0.25)
        gt._xyz.add_(0.003 * torch.randn(gt._xyz.shape, generator=torch.Generator().manual_seed(5)).to(dev))
    cams = ring_cameras(views, spec.W, spec.H, device=dev)
    bg = syn.background(dev)
    make_ground_truth(gt, cams, bg)
    return cams, bg


def fresh_model(dev, sh_degree):
    """The model every rank (and every reference run) starts from, with its FusedAdam; the options of the step."""
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    from gaussianhaircut_amd.utils import synthetic as syn
    opt = OptimizationParams()
    opt.lambda_dorient = 0.1
    model = syn.make_model(syn.CONFIGS["tiny_strands"], dev)
    model.active_sh_degree = sh_degree
    model.training_setup(opt)
    return model, opt


def scene(dev, sh_degree, views):
    """(model, cameras, background, options)"""
    cams, bg = scene_cameras(dev, views)
    model, opt = fresh_model(dev, sh_degree)
    return model, cams, bg, opt


def capture_reduced_gradient(model, store):
    """step / step_chunked with the gradient zeroing taken out, so the (reduced) flat gradient can be copied first"""
    o = model.optimizer
    orig_c, orig_s = o.step_chunked, o.step

    def chunked(chunks=4, zero_grad=True, reduce=False, shard=None):
        # (replicated update: with the sharded one a rank only ever holds ITS slices of the reduced gradient)
        orig_c(chunks=chunks, zero_grad=False, reduce=reduce, shard=False)
        store.append(o.flat_grad.detach().clone())
        o.flat_grad.zero_()

    def step(zero_grad=True, nan_scan=True):
        o.fold_own_views()  # (a multi-view step on one rank keeps its SH gradients as per-view tables until the update)
        store.append(o.flat_grad.detach().clone())
        orig_s(zero_grad=zero_grad, nan_scan=nan_scan)

    o.step_chunked, o.step = chunked, step


def collect(q, procs, n, timeout=900):
    """The workers' results; fails as soon as one of them has died (its peers would wait in a collective until the timeout)."""
    out, t0 = [], time.time()
    while len(out) < n:
        try:
            out.append(q.get(timeout=2))
        except queue.Empty:
            dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
            if dead or time.time() - t0 > timeout:
                for p in procs:
                    if p.is_alive():
                        p.terminate()
                raise AssertionError("worker exit codes %s after %.0f s" % ([p.exitcode for p in procs], time.time() - t0))
    return sorted(out, key=lambda d: d["rank"])
