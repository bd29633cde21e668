"""`-m gpu`: the fused model path (k_project / k_project_bwd behind render()) against the generic path it replaces
(PyTorch projection graph + autograd around the same HIP rasterizer)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gaussianhaircut_amd.gaussian_renderer import render
from gaussianhaircut_amd.utils import synthetic as syn
from tests.projection_shared import FUSED, GENERIC, _pixel_mask, _trainable_camera

pytestmark = pytest.mark.gpu



def _model(spec, dev, deg, max_deg=3):
    model = syn.make_model(spec, dev, sh_degree=max_deg)
    model.active_sh_degree = deg
    return model


def _run(spec, pipe, dev, weights, deg, max_deg=3):
    model = _model(spec, dev, deg, max_deg)
    cam = syn.make_view(spec, dev)
    pkg = render(cam, model, pipe, syn.background(dev))
    full = torch.cat([pkg["render"], pkg["mask"], pkg["orient_conf"]], dim=0)
    loss = (full * weights[:6]).sum() + (pkg["orient_angle"] * weights[6:7]).sum() * 0.1
    loss.backward()
    grads = {}
    for n in ("_xyz", "_scaling", "_rotation", "_opacity", "_label", "_orient_conf", "_features_dc", "_features_rest"):
        t = getattr(model, n)
        if t.numel() == 0:  # a degree-0 model stores no higher SH coefficients
            continue
        grads[n] = t.grad.detach().cpu().numpy()
    grads["viewspace"] = pkg["viewspace_points"].grad.detach().cpu().numpy()
    return pkg, grads


def _assert_rows_close(name, a, b, tol=1e-4, floor=1e-5):
    """|a - b| <= tol * (|b| + largest |b| of the ROW) + floor * largest |b| of the tensor -- every element.  The floor
    covers rows whose own gradient is the small difference of large terms (quaternion / scale chains) with fp32 atomics
    of a different order on BOTH sides of these HIP-vs-HIP comparisons; 1e-5 of the tensor's largest element."""
    a, b = a.reshape(len(a), -1), b.reshape(len(b), -1)
    assert np.isfinite(a).all(), name
    rows = np.abs(b).max(axis=1, keepdims=True)
    ok = np.abs(a - b) <= tol * (np.abs(b) + rows) + floor * np.abs(b).max()
    assert ok.all(), "%s: %d / %d elements off, worst |d| %g (tensor max %g)" % (
        name, (~ok).sum(), ok.size, np.abs(a - b)[~ok].max(), np.abs(b).max())


@pytest.mark.parametrize("cfg,deg,max_deg", [("tiny", 3, 3), ("tiny_strands", 3, 3), ("ragged", 1, 3), ("cfg1", 2, 3),
                                             ("ragged", 0, 0), ("tiny_strands", 1, 1)])
def test_fused_render_matches_generic_path(cfg, deg, max_deg):
    """Fused projection (k_project / k_project_bwd) vs the generic PyTorch projection around the same HIP rasterizer.
    No quantiles: the pixels that may legitimately differ are named (`_pixel_mask`, from the oracle chain's state of the
    same scene) and get zero weight on both sides; everything else must agree -- image 1e-4, every gradient row 1e-4.
    ``max_deg`` 0 / 1: models that store 1 / 4 SH coefficients per channel (k_project<false>: no coefficient slab at all;
    9-float slab rows)."""
    from tests import oracle_backend as ob
    dev = torch.device("cuda:0")
    spec = syn.CONFIGS[cfg]
    g = torch.Generator().manual_seed(5)
    weights = torch.randn(7, spec.H, spec.W, generator=g)
    # the oracle chain of the same scene names the fragile pixels
    mc = syn.make_model(spec, "cpu", sh_degree=max_deg)
    mc.active_sh_degree = deg
    with ob.oracle_rasterizer():
        pc = render(syn.make_view(spec, "cpu"), mc, GENERIC, syn.background("cpu"))
    st = ob.LAST["state"]
    with torch.no_grad():
        pf0 = render(syn.make_view(spec, dev), _model(spec, dev, deg, max_deg), FUSED, syn.background(dev))
        pg0 = render(syn.make_view(spec, dev), _model(spec, dev, deg, max_deg), GENERIC, syn.background(dev))
    rf, rg, rc = pf0["radii"].cpu().numpy(), pg0["radii"].cpu().numpy(), pc["radii"].numpy()
    m2d = pc["viewspace_points"].detach().numpy()
    mask, n1 = _pixel_mask(st, spec.H, spec.W, rf, rg, m2d)
    mask2, n2 = _pixel_mask(st, spec.H, spec.W, rf, rc, m2d)
    mask |= mask2
    assert n1 + n2 <= max(2, int(1e-3 * spec.P)) and mask.mean() < 0.05, (n1, n2, mask.mean())
    weights = weights * torch.from_numpy(~mask).float()
    # the orientation angle (normalize / mirror / clamp / acos of the rendered 2D direction, gaussian_renderer:53-57) has
    # its own non-smooth places: null direction, mirror line, clamp ends -- no weight there either
    d = pc._cov2d[:2].detach()
    nrm = d.norm(dim=0)
    c = d[1] / nrm.clamp_min(1e-12)
    weights[6] *= ((nrm > 1e-2) & (d[0].abs() > 1e-3 * nrm) & (c.abs() < 0.998)).float()
    weights = weights.to(dev)
    pf, gf = _run(spec, FUSED, dev, weights, deg, max_deg)
    pg, gg = _run(spec, GENERIC, dev, weights, deg, max_deg)
    assert torch.equal(pf["visibility_filter"], pf["radii"] > 0)
    ok = torch.from_numpy(~mask).to(dev)
    for k in ("render", "mask", "orient_conf"):
        a, b = pf[k].detach()[:, ok].cpu().numpy(), pg[k].detach()[:, ok].cpu().numpy()
        assert (np.abs(a - b) <= 1e-4 * np.maximum(1.0, np.abs(b))).all(), (k, np.abs(a - b).max())
    vf, vg = pf["viewspace_points"].detach().cpu().numpy(), pg["viewspace_points"].detach().cpu().numpy()
    assert np.abs(vf[:, :2] - vg[:, :2]).max() < 1e-5
    for k in gg:
        _assert_rows_close(k, gf[k], gg[k])


def test_fused_training_step_runs_and_learns():
    from gaussianhaircut_amd.parallel import FlatGradBucket
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    from gaussianhaircut_amd.trainer import make_ground_truth, training_step
    dev = torch.device("cuda:0")
    spec = syn.CONFIGS["tiny"]
    model, cam, bg = syn.make_model(spec, dev), syn.make_view(spec, dev), syn.background(dev)
    gt = syn.make_model(spec, dev)
    with torch.no_grad():
        gt._features_dc.add_(0.3)
    make_ground_truth(gt, [cam], bg)
    opt = OptimizationParams()
    model.training_setup(opt)  # FusedAdam owns the flat gradient buffer: no separate FlatGradBucket
    losses = [float(training_step(model, [cam], bg, opt, i + 1)) for i in range(8)]
    assert losses[-1] < losses[0] and np.isfinite(losses).all()


def test_multi_stream_views_equal_sequential_views():
    """training_step(streams=2/3): consecutive views of a step run on alternating HIP streams with only the accumulating
    kernels chained, so the per-view gradients are summed in the same order as on one stream.  The accumulated
    gradient of the first step (identical parameters) must agree with the sequential schedule to fp32 rounding of the
    render backward's atomics -- a race on the shared gradient buffer would lose a whole view's contribution -- and the
    run must keep learning."""
    from gaussianhaircut_amd.scene.cameras import ring_cameras
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    from gaussianhaircut_amd.trainer import make_ground_truth, training_step
    dev = torch.device("cuda:0")
    spec = syn.CONFIGS["tiny"]
    bg = syn.background(dev)
    cams = ring_cameras(5, spec.W, spec.H, device=dev)
    gt = syn.make_model(spec, dev)
    with torch.no_grad():
        gt._features_dc.add_(0.3)
    make_ground_truth(gt, cams, bg)
    opt = OptimizationParams()
    opt.lambda_dorient = 0.1
    runs = []
    for n_streams in (1, 2, 3):
        model = syn.make_model(spec, dev)
        model.training_setup(opt)
        o = model.optimizer
        grads, orig_step = [], o.step

        def capture(**kw):
            grads.append(o.flat_grad.detach().clone())
            return orig_step(**kw)
        o.step = capture
        # (fuse_adam=False: the wrapper around optimizer.step() above is how this test sees the gradients)
        losses = [float(training_step(model, cams, bg, opt, i + 1, streams=n_streams, fuse_adam=False)) for i in range(6)]
        torch.cuda.synchronize()
        assert not o.concurrent and o._acc_event is None
        assert np.isfinite(losses).all() and losses[-1] < losses[0]
        runs.append((losses, grads[0]))
    ref_loss, ref_grad = runs[0]
    scale = float(ref_grad.abs().max())
    assert scale > 0
    for losses, grad in runs[1:]:
        assert abs(losses[0] - ref_loss[0]) <= 5e-6 * abs(ref_loss[0])  # partial sums meet in float atomics
        assert float((grad - ref_grad).abs().max()) <= 1e-5 * scale


def test_deferred_counts_recover_from_a_too_small_capacity_guess():
    """training_step never waits for num_rendered (defer_counts): every view runs with the capacity guessed from the
    previous frame and the counts are checked after the step is queued.  With the guess forced far too small the
    forward drops instances and the backward clamps its gradient lines into the buffer; the step must notice, discard
    and recompute -- same gradient as a run that always waited."""
    import gaussianhaircut_amd.diff_gaussian_rasterization as dgr
    import gaussianhaircut_amd.trainer as tr
    from gaussianhaircut_amd.scene.cameras import ring_cameras
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    dev = torch.device("cuda:0")
    spec = syn.CONFIGS["tiny"]
    bg = syn.background(dev)
    cams = ring_cameras(3, spec.W, spec.H, device=dev)
    gt = syn.make_model(spec, dev)
    with torch.no_grad():
        gt._features_dc.add_(0.3)
    tr.make_ground_truth(gt, cams, bg)
    opt = OptimizationParams()
    opt.lambda_dorient = 0.1
    grads, passes = {}, {}
    orig = tr._views_forward_backward
    for mode in ("wait", "defer_ok", "defer_overflow"):
        model = syn.make_model(spec, dev)
        model.training_setup(opt)
        o = model.optimizer
        render(cams[0], model, tr.PIPE, bg)  # a blocking forward establishes a sane guess (parameters untouched)
        R_true = dgr.LAST_STATS["num_rendered"]
        assert R_true > 1000
        if mode == "defer_overflow":
            dgr._R_HINT[dev.index] = 64
        n_pass = [0]

        def counted(*a, **k):
            n_pass[0] += 1
            return orig(*a, **k)
        tr._views_forward_backward = counted
        captured, orig_step = [], o.step

        def capture(**kw):
            captured.append(o.flat_grad.detach().clone())
            assert int(o.state_dev[1]) == 0
            return orig_step(**kw)
        o.step = capture
        try:
            loss = float(tr.training_step(model, cams, bg, opt, 1, defer_counts=(mode != "wait"), fuse_adam=False))
        finally:
            tr._views_forward_backward = orig
        torch.cuda.synchronize()
        grads[mode], passes[mode] = (loss, captured[0]), n_pass[0]
        assert dgr._R_HINT[dev.index] > R_true // 2  # the guess recovered
    assert passes == {"wait": 1, "defer_ok": 1, "defer_overflow": 2}
    ref_loss, ref = grads["wait"]
    scale = float(ref.abs().max())
    for mode in ("defer_ok", "defer_overflow"):
        loss, g = grads[mode]
        assert abs(loss - ref_loss) <= 5e-6 * abs(ref_loss)  # partial sums meet in float atomics
        assert float((g - ref).abs().max()) <= 1e-5 * scale


def test_direct_gradient_sink_equals_autograd_accumulation_and_raises_nan_flag():
    """FusedAdam(direct_grads=True): the renderer's backward adds into the flat gradient buffer itself (two views ->
    accumulation) and maintains the NaN flag; must equal the autograd-accumulated gradients of direct_grads=False."""
    from gaussianhaircut_amd.scene.cameras import ring_cameras
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    dev = torch.device("cuda:0")
    spec = syn.CONFIGS["tiny"]
    cams = ring_cameras(2, spec.W, spec.H, device=dev)
    bg = syn.background(dev)
    g = torch.Generator().manual_seed(11)
    weights = torch.randn(6, spec.H, spec.W, generator=g).to(dev)
    flats = []
    for direct in (True, False):
        model = syn.make_model(spec, dev)
        model.training_setup(OptimizationParams())
        model.optimizer.direct_grads = direct
        for cam in cams:
            pkg = render(cam, model, FUSED, bg)
            full = torch.cat([pkg["render"], pkg["mask"], pkg["orient_conf"]], dim=0)
            (full * weights).sum().backward()
        assert model.optimizer._direct_backwards == (2 if direct else 0)
        assert int(model.optimizer.state_dev[1]) == 0
        flats.append(model.optimizer.flat_grad.detach().cpu().numpy().copy())
    scale = np.abs(flats[1]).max()
    assert scale > 0 and np.abs(flats[0] - flats[1]).max() <= 1e-5 * scale
    # a NaN parameter poisons its gradients: the producer-side flag must go up and the step must be skipped
    model = syn.make_model(spec, dev)
    model.training_setup(OptimizationParams())
    with torch.no_grad():
        model._opacity[3] = float("nan")
    before = model.optimizer.flat_param.detach().clone()
    pkg = render(cams[0], model, FUSED, bg)
    torch.cat([pkg["render"], pkg["mask"], pkg["orient_conf"]], dim=0).sum().backward()
    assert int(model.optimizer.state_dev[1]) == 1
    model.optimizer.step(zero_grad=True, nan_scan=False)
    after = model.optimizer.flat_param
    same = (after == before) | (torch.isnan(after) & torch.isnan(before))
    assert bool(same.all()) and int(model.optimizer.state_dev[0]) == 0 and int(model.optimizer.state_dev[1]) == 0


def _hair_weights(spec, pkg_cpu, state, radii_list, seed=3):
    """Loss weights of the hair comparisons: random, zero on the pixels named by `_pixel_mask` (against every radii set
    in radii_list) and, for the angle channel, on the non-smooth places of the orientation angle."""
    w = torch.randn(7, spec.H, spec.W, generator=torch.Generator().manual_seed(seed))
    rc = pkg_cpu["radii"].numpy()
    m2d = pkg_cpu["viewspace_points"].detach().numpy()
    mask, flips = np.zeros((spec.H, spec.W), bool), 0
    for r in radii_list:
        mk, n = _pixel_mask(state, spec.H, spec.W, rc, r, m2d)
        mask |= mk
        flips += n
    assert flips <= max(2, int(1e-3 * rc.size)) and mask.mean() < 0.05, (flips, mask.mean())
    w = w * torch.from_numpy(~mask).float()
    d = pkg_cpu._cov2d[:2].detach()
    nrm = d.norm(dim=0)
    c = d[1] / nrm.clamp_min(1e-12)
    w[6] *= ((nrm > 1e-2) & (d[0].abs() > 1e-3 * nrm) & (c.abs() < 0.998)).float()
    return w, mask


def _hair_pass(where, pipe, w, init_gaussians=False):
    from gaussianhaircut_amd.gaussian_renderer import render_hair
    from tests.oracle_backend import oracle_rasterizer
    from tests.test_api_cpu import _hair_scene
    import contextlib
    spec, head, hair, cam = _hair_scene(where)
    if init_gaussians:  # strand parameters are the leaves: rebuild the per-Gaussian tensors inside the graph
        hair.initialize_gaussians_hair()
    with (oracle_rasterizer() if str(where) == "cpu" else contextlib.nullcontext()):
        pkg = render_hair(cam, head, hair, pipe, syn.background(where))
        full = torch.cat([pkg["render"], pkg["mask"], pkg["orient_conf"], pkg["orient_angle"]], dim=0)
        if w is not None:
            (full * w.to(where)).sum().backward()
    grads = None
    if w is not None:
        grads = {n: getattr(hair, n).grad.detach().cpu().numpy() for n in ("_dirs", "_features_dc", "_features_rest", "_orient_conf")}
    return spec, pkg, full.detach().cpu().numpy(), grads


def test_render_hair_gpu_matches_cpu_oracle_path():
    """render_hair() on the HIP rasterizer (mode A_sr) vs the same host code driving the CPU oracle: image, radii and
    the gradients that reach the strand parameters.  Explicit pixel mask (`_pixel_mask`), then every element: image 1e-4,
    gradient rows 1e-4."""
    from tests import oracle_backend as ob
    dev = torch.device("cuda:0")
    spec, pc0, _, _ = _hair_pass("cpu", GENERIC, None)
    st = ob.LAST["state"]
    with torch.no_grad():
        _, pg0, _, _ = _hair_pass(dev, GENERIC, None)
    w, mask = _hair_weights(spec, pc0, st, [pg0["radii"].cpu().numpy()])
    _, pc, img_c, g_c = _hair_pass("cpu", GENERIC, w)
    _, pg, img_g, g_g = _hair_pass(dev, GENERIC, w)
    ok = ~mask
    assert (np.abs(img_g[:6] - img_c[:6])[:, ok] <= 1e-4 * np.maximum(1.0, np.abs(img_c[:6][:, ok]))).all()
    for k in g_c:
        _assert_rows_close(k, g_g[k], g_c[k])


def test_densification_with_fused_adam_matches_torch_adam_surgery():
    """SURVEY N3 on the GPU: densify_and_prune + reset_opacity re-lay FusedAdam's flat buffers exactly like the
    reference's per-parameter torch.optim.Adam surgery (same seeds), and the fused step keeps training afterwards."""
    from gaussianhaircut_amd.optim import FusedAdam
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    from gaussianhaircut_amd.trainer import make_ground_truth, training_step
    from tests.test_reference_golden import _densify_sequence
    dev = torch.device("cuda:0")
    spec = syn.CONFIGS["tiny"]
    opt = OptimizationParams()
    res = []
    for fused in (True, False):
        m = syn.make_model(spec, dev)
        m.training_setup(opt, fused=fused)
        assert isinstance(m.optimizer, FusedAdam) == fused
        _densify_sequence(m, opt, dev)
        torch.manual_seed(991)
        m.densify_and_prune(opt.densify_grad_threshold, 0.005, 2.5, 20)
        m.reset_opacity()
        state = {}
        if fused:
            for g, p, mm, vv in m.optimizer._group_views():
                state[g["name"]] = (p.detach().clone(), mm.clone(), vv.clone())
                assert p.grad is not None and p.grad.data_ptr() >= m.optimizer.flat_grad.data_ptr()
        else:
            for g in m.optimizer.param_groups:
                st = m.optimizer.state[g["params"][0]]
                state[g["name"]] = (g["params"][0].detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone())
        res.append((m, state))
    (mf, sf), (mt, stt) = res
    assert mf.get_xyz.shape[0] == mt.get_xyz.shape[0] != spec.P
    for k in stt:
        for a, b, what in zip(sf[k], stt[k], ("param", "exp_avg", "exp_avg_sq")):
            assert a.shape == b.shape and torch.allclose(a, b, rtol=1e-4, atol=1e-9), (k, what, (a - b).abs().max())
    # the resized model keeps training through the fused render / loss / Adam path
    cam, bg = syn.make_view(spec, dev), syn.background(dev)
    gt = syn.make_model(spec, dev)
    with torch.no_grad():
        gt._features_dc.add_(0.3)
    make_ground_truth(gt, [cam], bg)
    losses = [float(training_step(mf, [cam], bg, opt, i + 3)) for i in range(6)]
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    assert mf._xyz.data_ptr() == mf.optimizer.flat_param.data_ptr()


def test_densification_step_loop_on_gpu():
    """trainer.densification_step inside a short stage-1 loop (train_gaussians.py:158-171): statistics accumulate from
    viewspace_points.grad, the model is resized at the interval, training goes on."""
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    from gaussianhaircut_amd.trainer import PIPE, densification_step, make_ground_truth, view_loss
    dev = torch.device("cuda:0")
    spec = syn.CONFIGS["tiny"]
    opt = OptimizationParams()
    opt.densify_from_iter, opt.densification_interval, opt.lambda_dorient = 2, 4, 0.1
    opt.densify_grad_threshold = 1e-7
    m, cam, bg = syn.make_model(spec, dev), syn.make_view(spec, dev), syn.background(dev)
    gt = syn.make_model(spec, dev)
    with torch.no_grad():
        gt._features_dc.add_(0.3)
    make_ground_truth(gt, [cam], bg)
    m.training_setup(opt)
    sizes = []
    for it in range(1, 10):
        m.update_learning_rate(it)
        pkg = render(cam, m, PIPE, bg)
        view_loss(pkg, cam, opt).backward()
        assert pkg["viewspace_points"].grad is not None
        densification_step(m, pkg, opt, it, cameras_extent=2.5)
        m.optimizer.step(zero_grad=True)
        sizes.append(m.get_xyz.shape[0])
    assert sizes[2] == spec.P and sizes[3] != spec.P and sizes[7] != sizes[3]
    assert torch.isfinite(m.optimizer.flat_param).all()


@pytest.mark.parametrize("pipe", [FUSED, GENERIC])
def test_speculative_stage2_capacity_guess_never_changes_the_result(pipe):
    """run_stage2: stage 2 is launched with a capacity guessed from the previous frame before num_rendered is read;
    too small a guess drops instances inside the workspace bounds and triggers a relaunch.  Image, radii and gradients
    must be identical for no guess / a far too small guess / a generous guess."""
    import gaussianhaircut_amd.diff_gaussian_rasterization as dgr
    dev = torch.device("cuda:0")
    spec = syn.CONFIGS["cfg1"]
    cam, bg = syn.make_view(spec, dev), syn.background(dev)
    w = torch.randn(6, spec.H, spec.W, generator=torch.Generator().manual_seed(2)).to(dev)
    outs = []
    for hint in (None, 64, 10_000_000):
        dgr._R_HINT.pop(dev.index, None)
        dgr._R_RECENT.pop(dev.index, None)
        if hint:
            dgr._R_HINT[dev.index] = hint
        model = syn.make_model(spec, dev)
        pkg = render(cam, model, pipe, bg)
        full = torch.cat([pkg["render"], pkg["mask"], pkg["orient_conf"]], dim=0)
        (full * w).sum().backward()
        R = dgr.LAST_STATS["num_rendered"]
        g_ = R + R // 4 + 4096   # (on a grid of 1/32 .. 1/16 of itself, at least 64k instances: round 6)
        assert 64 < R < 10_000_000 and g_ <= dgr._R_HINT[dev.index] < g_ + max(65536, g_ // 16)
        outs.append((full.detach().clone(), pkg["radii"].clone(), model._xyz.grad.clone(), model._features_dc.grad.clone()))
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])
        for a, b in zip(o[2:], outs[0][2:]):   # float atomics inside a tile: order-dependent rounding only
            assert torch.allclose(a, b, rtol=1e-4, atol=1e-7 * float(b.abs().max()))


def test_fused_render_hair_matches_generic_path():
    """Strand stage: the segmented fused projection behind render_hair() (explicit mode of k_project / k_project_bwd,
    head + strands as two segments of one rasterizer state) vs the generic PyTorch projection path: image, radii,
    viewspace points and the gradients that reach the strand parameters through initialize_gaussians_hair().  Explicit
    pixel mask from the oracle chain of the same scene, then every element."""
    from tests import oracle_backend as ob
    dev = torch.device("cuda:0")
    spec, pc0, _, _ = _hair_pass("cpu", GENERIC, None, init_gaussians=True)
    st = ob.LAST["state"]
    with torch.no_grad():
        _, pf0, _, _ = _hair_pass(dev, FUSED, None, init_gaussians=True)
        _, pg0, _, _ = _hair_pass(dev, GENERIC, None, init_gaussians=True)
    w, mask = _hair_weights(spec, pc0, st, [pf0["radii"].cpu().numpy(), pg0["radii"].cpu().numpy()])
    res = {}
    for name, pipe in (("fused", FUSED), ("generic", GENERIC)):
        _, pkg, img, g = _hair_pass(dev, pipe, w, init_gaussians=True)
        res[name] = (img, pkg["radii"].cpu().numpy(), pkg["viewspace_points"].detach().cpu().numpy(), g,
                     pkg["viewspace_points"].grad.detach().cpu().numpy())
    (img_f, rad_f, vs_f, g_f, vg_f), (img_g, rad_g, vs_g, g_g, vg_g) = res["fused"], res["generic"]
    assert rad_f.shape == rad_g.shape
    ok = ~mask
    assert (np.abs(img_f[:6] - img_g[:6])[:, ok] <= 1e-4 * np.maximum(1.0, np.abs(img_g[:6][:, ok]))).all()
    assert np.abs(vs_f[:, :2] - vs_g[:, :2]).max() < 1e-5
    n_head = int((rad_f.shape[0] - g_f["_features_dc"].shape[0]))
    # densification signal of the strand rows (the head is frozen: its rows stay 0 on the fused path)
    assert np.abs(vg_f[:n_head]).max() == 0
    _assert_rows_close("viewspace", vg_f[n_head:, :2], vg_g[n_head:, :2])
    for k in g_g:
        _assert_rows_close(k, g_f[k], g_g[k])


def test_strand_training_step_learns_on_gpu():
    """trainer.strand_training_step (src/train_strands.py:98-160): fused render_hair + fused strand-stage loss + Adam on
    the strand parameters; the loss towards a perturbed copy of the strands goes down, for both optimizers."""
    from gaussianhaircut_amd.gaussian_renderer import render_hair
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    from gaussianhaircut_amd.trainer import strand_training_step
    from tests.test_api_cpu import _hair_scene
    dev = torch.device("cuda:0")
    opt = OptimizationParams()
    opt.lambda_dorient, opt.lambda_dmask = 0.1, 0.1          # run.sh:177
    bg = syn.background(dev)
    for fused_adam in (True, False):
        spec, head, hair, cam = _hair_scene(dev)
        _, _, gt_hair, _ = _hair_scene(dev)
        with torch.no_grad():
            gt_hair._features_dc.add_(0.4)
            gt_hair._dirs.mul_(1.1)
            gt_hair.initialize_gaussians_hair()
            pkg = render_hair(cam, head, gt_hair, FUSED, bg)
            cam.original_image = pkg["render"].clamp(0, 1).detach()
            cam.original_mask = pkg["mask"].clamp(0, 1).detach()
            cam.original_orient_angle = pkg["orient_angle"].detach()
            cam.original_orient_conf = torch.ones_like(pkg["orient_conf"]).detach()
        hair.training_setup(opt, fused=fused_adam)
        assert [g["name"] for g in hair.optimizer.param_groups] == ["xyz", "f_dc", "f_rest", "orient_conf"]
        d0 = hair._dirs.detach().clone()
        losses = [float(strand_training_step(head, hair, [cam], bg, opt, i + 1, pipe=FUSED)) for i in range(10)]
        assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
        assert (hair._dirs.detach() - d0).abs().max() > 0


def test_strand_stage_direct_sh_gradients_match_autograd_accumulation():
    """Round 6, three forms of the strand-stage iteration (src/train_strands.py:98-160) with FusedAdam, the same parameters bit
    for bit after every one of five iterations:
      fused    -- the SH features' update rides in the render_hair backward (ghr_adam_fuse, strand segment); directions and
                  confidence are stepped when autograd has delivered their gradients; the step is finished on the device;
      direct   -- the backward ASSIGNS the SH-feature gradients into the optimizer's (known-zero) buffer and raises its flag;
                  the step scans only the autograd-fed groups;
      autograd -- the gradients are returned and accumulated by autograd; the step scans everything.
    A two-view step takes the classic road in all three; a NaN that only autograd carries (into the strand directions) skips
    the update in all three and the next iteration goes through again."""
    import copy
    from gaussianhaircut_amd import _lib as ghr_lib
    from gaussianhaircut_amd import trainer
    from gaussianhaircut_amd.gaussian_renderer import render_hair
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    from gaussianhaircut_amd.trainer import strand_training_step
    from tests.test_api_cpu import _hair_scene
    dev = torch.device("cuda:0")
    opt = OptimizationParams()
    opt.lambda_dorient, opt.lambda_dmask = 0.1, 0.1
    bg = syn.background(dev)
    lib = ghr_lib.lib()
    lib.ghr_set_deterministic(1)
    saved = trainer.FUSE_STRAND_ADAM
    try:
        res = {}
        for mode in ("fused", "direct", "autograd"):
            trainer.FUSE_STRAND_ADAM = mode == "fused"
            spec, head, hair, cam = _hair_scene(dev)
            _, _, gt_hair, _ = _hair_scene(dev)
            with torch.no_grad():
                gt_hair._features_dc.add_(0.4)
                gt_hair._dirs.mul_(1.1)
                gt_hair.initialize_gaussians_hair()
                pkg = render_hair(cam, head, gt_hair, FUSED, bg)
                cam.original_image = pkg["render"].clamp(0, 1).detach()
                cam.original_mask = pkg["mask"].clamp(0, 1).detach()
                cam.original_orient_angle = pkg["orient_angle"].detach()
                cam.original_orient_conf = torch.ones_like(pkg["orient_conf"]).detach()
            hair.training_setup(opt, fused=True)
            o = hair.optimizer
            o.direct_grads = mode != "autograd"
            seen = []
            step0 = o.step
            o.step = lambda *a, **k: (seen.append(k.get("nan_scan", True)), step0(*a, **k))[1]
            params = lambda: [p.detach().clone() for p in (hair._dirs, hair._features_dc, hair._features_rest, hair._orient_conf)]
            trace = []
            for i in range(3):
                strand_training_step(head, hair, [cam], bg, opt, i + 1, pipe=FUSED)
                trace.append(params())
            strand_training_step(head, hair, [cam, copy.copy(cam)], bg, opt, 4, pipe=FUSED)  # the second view accumulates
            trace.append(params())
            # a NaN that only autograd carries (into the strand directions): the update is skipped, nothing moves
            h = hair._dirs.register_hook(lambda g: torch.full_like(g, float("nan")))
            strand_training_step(head, hair, [cam], bg, opt, 5, pipe=FUSED)
            h.remove()
            torch.cuda.synchronize()
            for x, y in zip(trace[-1], params()):
                assert torch.equal(x, y), mode
            assert int(o.state_dev[0]) == 4 and int(o.state_dev[1]) == 0 and float(o.flat_grad.abs().max()) == 0.0, mode
            strand_training_step(head, hair, [cam], bg, opt, 6, pipe=FUSED)  # and the next one goes through again
            trace.append(params())
            assert not torch.equal(trace[-2][1], trace[-1][1]) and int(o.state_dev[0]) == 5, mode
            if mode == "fused":
                assert seen == [True] and o.fused_steps == 5, (seen, o.fused_steps)   # only the two-view step called step()
                assert hair._dirs.data_ptr() == o.flat_param.data_ptr()                # the parameters alias the CURRENT set
            elif mode == "direct":
                assert seen == [False, False, False, True, False, False] and o.fused_steps == 0, seen
            else:
                assert seen == [True] * 6, seen
            res[mode] = trace
        for mode in ("direct", "autograd"):
            for it, (ta, tb) in enumerate(zip(res["fused"], res[mode])):
                for x, y in zip(ta, tb):
                    assert torch.equal(x, y), (mode, it, float((x - y).abs().max()))
    finally:
        trainer.FUSE_STRAND_ADAM = saved
        lib.ghr_set_deterministic(0)


def test_first_direct_backward_assigns_only_into_a_buffer_known_to_be_zero():
    """FusedAdam.take_known_zero: the step's first direct backward may assign instead of accumulate (k_project_bwd then
    skips reading the zeros) -- but only while the gradient buffer is KNOWN to be zero; anything PyTorch wrote into a
    .grad view in the meantime (another loss, here an in-place add) must survive."""
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    dev = torch.device("cuda:0")
    spec = syn.CONFIGS["tiny"]
    cam, bg = syn.make_view(spec, dev), syn.background(dev)
    w = torch.randn(6, spec.H, spec.W, generator=torch.Generator().manual_seed(2)).to(dev)
    model = syn.make_model(spec, dev)
    model.training_setup(OptimizationParams())
    opt = model.optimizer

    def backward():
        pkg = render(cam, model, FUSED, bg)
        (torch.cat([pkg["render"], pkg["mask"], pkg["orient_conf"]], dim=0) * w).sum().backward()
        torch.cuda.synchronize()
        return opt.flat_grad.detach().clone()

    assert opt._zero_version is not None          # fresh optimizer: zeros
    g0 = backward()                               # assigned
    assert opt._zero_version is None and opt._direct_backwards == 1
    g1 = backward()                               # accumulated on top
    assert torch.allclose(g1, 2 * g0, rtol=1e-5, atol=1e-6 * float(g0.abs().max()))
    opt._direct_backwards = 0
    opt.zero()
    model._xyz.grad.add_(1.0)                     # somebody else's gradient, through PyTorch
    g2 = backward()
    expect = g0.clone()
    n_xyz = model._xyz.numel()
    expect[:n_xyz] += 1.0                         # xyz is the first group of the flat buffer
    assert torch.allclose(g2, expect, rtol=1e-5, atol=1e-6 * float(g0.abs().max()))
    # and a step leaves the buffer known-zero again; the next backward reproduces g0 (parameters moved: only its shape)
    opt._direct_backwards = 1
    opt.step(zero_grad=True, nan_scan=True)
    assert opt._zero_version is not None and float(opt.flat_grad.abs().sum()) == 0.0


@pytest.mark.parametrize("cfg,deg", [("tiny_strands", 3), ("tiny", 1)])
def test_sh_gradients_rebuilt_from_per_view_factors_equal_the_accumulated_ones(cfg, deg):
    """ABI 19 (the data-parallel gradient message): with view slots open (FusedAdam.begin_factored_views) the fused backward of
    every view leaves dL/d(rgb) [P,3] + its camera centre instead of adding 192 B per Gaussian of SH gradients, and the update
    rebuilds them (ghr_sh_grad_from_views).  One process, three views (one slot stays empty): the whole flat gradient and the
    parameters after the update are the BITS of the plain accumulation."""
    from gaussianhaircut_amd import _lib
    from gaussianhaircut_amd.scene.cameras import ring_cameras
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    dev = torch.device("cuda:0")
    spec = syn.CONFIGS[cfg]
    bg = syn.background(dev)
    cams = ring_cameras(3, spec.W, spec.H, device=dev)
    w = torch.randn(6, spec.H, spec.W, generator=torch.Generator().manual_seed(2)).to(dev)
    _lib.lib().ghr_set_deterministic(1)
    try:
        res = {}
        for factored in (False, True):
            model = syn.make_model(spec, dev)
            model.active_sh_degree = deg
            model.training_setup(OptimizationParams())
            o = model.optimizer
            assert o.can_factor_views()
            if factored:
                o.begin_factored_views(4)
            for cam in cams:
                pkg = render(cam, model, FUSED, bg)
                (torch.cat([pkg["render"], pkg["mask"], pkg["orient_conf"]], dim=0) * w).sum().backward()
            assert o._direct_backwards == 3
            o.active_rest_coeffs = (deg + 1) ** 2 - 1
            P = model.get_xyz.shape[0]
            if factored:
                assert o._views["next"] == 3
                before = o.flat_grad[3 * P: 51 * P].detach().clone()   # the SH ranges: untouched by the three backwards
                assert float(before.abs().max()) == 0.0
            o.step_chunked(chunks=4, zero_grad=False)
            o.end_factored_views()
            torch.cuda.synchronize()
            res[factored] = (o.flat_grad.detach().clone(), o.flat_param.detach().clone(), int(o.state_dev[0]))
        (g0, p0, s0), (g1, p1, s1) = res[False], res[True]
        assert s0 == s1 == 1 and float(g0[3 * P: 51 * P].abs().max()) > 0
        assert torch.equal(g0, g1) and torch.equal(p0, p1)
        # a non-finite cotangent of the red channel: the view's dL/d(rgb) table is non-finite and the optimizer's flag goes up
        model = syn.make_model(spec, dev)
        model.training_setup(OptimizationParams())
        o = model.optimizer
        o.begin_factored_views(1)
        w_bad = w[:3].clone()
        w_bad[0] = float("inf")
        pkg = render(cams[0], model, FUSED, bg)
        (pkg["render"] * w_bad).sum().backward()
        torch.cuda.synchronize()
        assert not bool(torch.isfinite(o._views["buf"][0, : 3 * P]).all())
        o.end_factored_views()
        assert int(o.state_dev[1]) == 1
    finally:
        _lib.lib().ghr_set_deterministic(0)


def test_trainable_camera_takes_the_fused_path_and_keeps_its_gradients(monkeypatch):
    """ABI 17 (VERDICT r5 missing #1; rounds 2-5 sent such a camera down the generic path): render() with the DEFAULT pipe on
    a GaussianModel + a camera whose tensors are FUNCTIONS of trainable leaves (full_proj = view @ P, centre = inverse(view),
    as src/scene/cameras.py:113-151 builds them) takes the fused entry point, and d loss / d (view matrix, FoV) -- the camera
    cotangents of k_project_bwd<CAM> + k_cam_fold carried on by autograd through the camera's own graph -- agree with the same
    PyTorch projection graph around the CPU oracle (the chain every other parity test is anchored to)."""
    from tests import oracle_backend as ob
    import gaussianhaircut_amd.gaussian_renderer.fused as fused_mod
    dev = torch.device("cuda:0")
    spec, deg = syn.CONFIGS["tiny"], 2
    g = torch.Generator().manual_seed(11)
    weights = torch.randn(6, spec.H, spec.W, generator=g)
    called = []
    orig = fused_mod.render_model_fused
    monkeypatch.setattr(fused_mod, "render_model_fused", lambda *a, **k: (called.append(1), orig(*a, **k))[1])

    def run(device, pipe):
        model = _model(spec, device, deg)
        cam = _trainable_camera(spec, device)
        pkg = render(cam, model, pipe, syn.background(device))
        full = torch.cat([pkg["render"], pkg["mask"], pkg["orient_conf"]], dim=0)
        (full * weights.to(device)).sum().backward()
        return (pkg, cam.world_view_transform.grad.cpu().numpy(), cam.FoVx.grad.item(), cam.FoVy.grad.item(),
                model._xyz.grad.cpu().numpy())

    with ob.oracle_rasterizer():
        pc, vc, fxc, fyc, xc = run("cpu", GENERIC)
    st = ob.LAST["state"]
    assert not called
    mask = np.asarray(st.fragile).reshape(spec.H, spec.W).astype(bool)
    assert mask.mean() < 0.02
    weights = weights * torch.from_numpy(~mask).float()
    with ob.oracle_rasterizer():
        pc, vc, fxc, fyc, xc = run("cpu", GENERIC)
    ph, vh, fxh, fyh, xh = run(dev, FUSED)   # FUSED = the default pipe: fused_projection=True
    assert called, "the fused path must serve a trainable camera"
    assert np.abs(vc).max() > 0 and np.isfinite(vh).all()
    # rows 0..2 x cols 0..2 and the translation row carry gradient; column 3 of W2C^T does not enter the projection.
    # The camera's gradients are sums over all Gaussians: relative to the tensor's largest entry
    tol = 2e-4 * np.abs(vc).max()
    assert (np.abs(vh - vc) <= tol).all(), (vh, vc)
    assert abs(fxh - fxc) <= 2e-4 * (abs(fxc) + abs(fyc)) and abs(fyh - fyc) <= 2e-4 * (abs(fxc) + abs(fyc))
    _assert_rows_close("xyz", xh, xc)


@pytest.mark.parametrize("pipe", [FUSED, GENERIC])
def test_training_step_after_surgery_is_not_a_skipped_step(pipe):
    """ADVICE r2 (optim.py:146): densification / opacity reset mark every group "replaced since the last backward" so
    that a hand-written backward -> surgery -> step loop passes the new parameters by like the reference does.  Inside
    training_step the backward always follows the surgery, so the very next step must update -- also when the gradients
    do not come through the fused direct backward (generic pipe)."""
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    from gaussianhaircut_amd.trainer import make_ground_truth, training_step
    from tests.test_reference_golden import _densify_sequence
    dev = torch.device("cuda:0")
    spec = syn.CONFIGS["tiny"]
    opt = OptimizationParams()
    m, cam, bg = syn.make_model(spec, dev), syn.make_view(spec, dev), syn.background(dev)
    gt = syn.make_model(spec, dev)
    with torch.no_grad():
        gt._features_dc.add_(0.3)
    make_ground_truth(gt, [cam], bg)
    m.training_setup(opt)
    _densify_sequence(m, opt, dev)
    torch.manual_seed(3)
    m.densify_and_prune(opt.densify_grad_threshold, 0.005, 2.5, 20)
    m.reset_opacity()
    assert m.optimizer._skip_next != 0
    before = m.optimizer.flat_param.clone()
    step0 = int(m.optimizer.state_dev[0])
    training_step(m, [cam], bg, opt, 5, pipe=pipe)
    assert int(m.optimizer.state_dev[0]) == step0 + 1
    assert int(m.optimizer.state_dev[2:2 + len(m.optimizer.param_groups)].abs().sum()) == 0  # no group sat the step out
    assert (m.optimizer.flat_param != before).float().mean() > 0.2


def test_deferred_gradient_zeroing_is_invisible_or_loud():
    """trainer.training_step on the fused path steps with FusedAdam.step(zero_grad="defer"): the Adam pass leaves the
    gradient buffer undefined because the next step's first backward ASSIGNS all of it.  (a) Three steps are bit-identical
    to the eager run (GHR_DEFER_GRAD_ZEROING=0 semantics: trainer.DEFER_GRAD_ZEROING = False); (b) a step() without a
    backward in between sees zeros; (c) optimizer surgery in between (reset_opacity) works; (d) accumulating gradients by
    other means while the buffer is undefined fails loudly at the next step instead of stepping on garbage; (e) a step
    that does not take the fused path (pipe.fused_projection = False) gets the zeros first."""
    import gaussianhaircut_amd.trainer as tr
    from gaussianhaircut_amd import _lib
    from gaussianhaircut_amd.scene.cameras import ring_cameras
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    from gaussianhaircut_amd.trainer import make_ground_truth, training_step
    dev = torch.device("cuda:0")
    spec = syn.CONFIGS["tiny_strands"]
    opt = OptimizationParams()
    opt.lambda_dorient = 0.1
    cams = ring_cameras(4, spec.W, spec.H, device=dev)
    bg = syn.background(dev)
    gt = syn.make_model(spec, dev)
    with torch.no_grad():
        gt._features_dc.add_(0.3)
    make_ground_truth(gt, cams, bg)
    _lib.lib().ghr_set_deterministic(1)  # two RUNS are compared bit for bit
    try:
        runs = []
        for defer in (True, False):
            tr.DEFER_GRAD_ZEROING = defer
            model = syn.make_model(spec, dev)
            model.training_setup(opt)
            o = model.optimizer
            for it in range(3):
                training_step(model, cams[:2], bg, opt, it + 1)
                assert (o._deferred is not None) == defer
            o.step()                                        # (b) no backward since: zeros, whichever way
            assert o._deferred is None and float(o.flat_grad.abs().sum()) == 0.0
            training_step(model, cams[:2], bg, opt, 4)
            model.reset_opacity()                           # (c) surgery between two steps
            training_step(model, cams[:2], bg, opt, 5)
            torch.cuda.synchronize()
            runs.append((o.flat_param.clone(), o.exp_avg.clone(), o.exp_avg_sq.clone(), o.state_dev.clone()))
        for a, b in zip(*runs):
            assert torch.equal(a, b)
        # (d)
        tr.DEFER_GRAD_ZEROING = True
        model = syn.make_model(spec, dev)
        model.training_setup(opt)
        training_step(model, cams[:2], bg, opt, 1)
        assert model.optimizer._deferred is not None
        (model._xyz.sum() * 1.0).backward()                 # autograd accumulates into the undefined buffer
        with pytest.raises(RuntimeError, match="undefined"):
            model.optimizer.step()
        model.optimizer.zero_grad()                         # the documented way out
        model.optimizer.step()
        # (d') READERS: between two fused steps p.grad still holds the gradients of the step just taken (the
        # reference's are None at that point) -- finite, usable for gradient-norm logging -- while the bucket accessor
        # `optimizer.flat`, whose contract is "what the next accumulation starts from", zero-fills first
        model = syn.make_model(spec, dev)
        model.training_setup(opt)
        training_step(model, cams[:2], bg, opt, 1, fuse_adam=False)  # (a fused update stores no gradients at all)
        o = model.optimizer
        assert o._deferred is not None
        g = model._xyz.grad
        assert g is not None and torch.isfinite(g).all() and float(g.abs().sum()) > 0
        assert float(o.flat.abs().sum()) == 0.0 and o._deferred is None and float(model._xyz.grad.abs().sum()) == 0.0
        with pytest.raises(ValueError):
            o.step(zero_grad="true")                        # a typo must not silently mean "defer"
        training_step(model, cams[:2], bg, opt, 2)          # ... and the next step runs on as if nothing had happened
        # (e)
        model = syn.make_model(spec, dev)
        model.training_setup(opt)
        ref = syn.make_model(spec, dev)
        ref.training_setup(opt)
        training_step(model, cams[:1], bg, opt, 1)
        tr.DEFER_GRAD_ZEROING = False
        training_step(ref, cams[:1], bg, opt, 1)
        tr.DEFER_GRAD_ZEROING = True
        generic = SimpleNamespace(**{**vars(tr.PIPE), "fused_projection": False})
        for m in (model, ref):
            cam = _trainable_camera(spec, dev)              # a fresh graph per model: full_proj = f(view matrix)
            with torch.no_grad():
                make_ground_truth(gt, [cam], bg)
            training_step(m, [cam], bg, opt, 2, pipe=generic)   # generic path: gradients through autograd
        torch.cuda.synchronize()
        assert model.optimizer._deferred is None
        assert torch.equal(model.optimizer.flat_param, ref.optimizer.flat_param)
    finally:
        tr.DEFER_GRAD_ZEROING = True
        _lib.lib().ghr_set_deterministic(0)


def test_recycled_image_workspace_skips_the_zero_fill_and_changes_nothing():
    """Round 5: a fused forward pass that gets the image workspace of an earlier, completed pass back from the pool
    (gaussian_renderer/fused.py _ImgLease) tells stage 1 so (ghr_model_args.img_ws_recycled) and the per-tile counters'
    zero-fill launch is dropped -- k_tile_scan / the tile sort left them at zero.  Images, radii and instance counts of
    three passes in a row (different cameras, so different counts per tile) must equal the fresh-buffer path's bit for
    bit, and the second and third pass must really have run on a recycled buffer."""
    from gaussianhaircut_amd.gaussian_renderer import fused
    from gaussianhaircut_amd.scene.cameras import ring_cameras
    dev = torch.device("cuda:0")
    spec = syn.CONFIGS["cfg1"]
    cams = ring_cameras(3, spec.W, spec.H, device=dev)
    outs = {}
    for recycle in (False, True):
        fused.RECYCLE_IMG_WS = recycle
        fused._ImgLease._pools.clear()
        model = _model(spec, dev, 2)
        got = []
        seen = []
        orig = fused._ImgLease.__init__

        def spy(self, d, n, w, h, _orig=orig, _seen=seen):
            _orig(self, d, n, w, h)
            _seen.append(self.recycled)
        fused._ImgLease.__init__ = spy
        try:
            for cam in cams:
                pkg = render(cam, model, FUSED, syn.background(dev))
                (pkg["render"].sum() + pkg["mask"].sum()).backward()
                got.append((pkg["render"].detach().clone(), pkg["radii"].clone(), model._xyz.grad.detach().clone()))
                del pkg  # the graph is gone: the lease returns its buffer
        finally:
            fused._ImgLease.__init__ = orig
        outs[recycle] = got
        if recycle:
            assert seen == [False, True, True], seen
        torch.cuda.synchronize()
    fused.RECYCLE_IMG_WS = True
    for a, b in zip(outs[False], outs[True]):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        # (the gradient walk's atomics are unordered: same sums, last-bit differences between any two runs)
        assert torch.allclose(a[2], b[2], rtol=1e-5, atol=1e-7 * float(a[2].abs().max()))


def test_empty_model_pass_never_pools_its_image_workspace():
    """with P == 0 the library returns from stage 1 and stage 2 without touching the image workspace, so
    that pass's (uninitialised) buffer must not enter the recycling pool -- the next P > 0 pass at the same size would skip the
    counters' zero-fill over garbage.  Render an empty model, then a real one, same W x H, same stream, in debug mode (the
    library then verifies a recycled workspace's counters itself); result == a fresh-pool render, bit for bit."""
    from gaussianhaircut_amd.gaussian_renderer import fused
    from gaussianhaircut_amd.scene.gaussian_model import GaussianModel
    dev = torch.device("cuda:0")
    spec = syn.CONFIGS["cfg1"]
    cam = syn.make_view(spec, dev)
    model = _model(spec, dev, 2)
    dbg = SimpleNamespace(debug=True, fused_projection=True)
    fused._ImgLease._pools.clear()
    with torch.no_grad():
        ref = render(cam, model, dbg, syn.background(dev))
        ref_img, ref_radii = ref["render"].clone(), ref["radii"].clone()
    del ref
    fused._ImgLease._pools.clear()
    empty = GaussianModel(3)
    for n in ("_xyz", "_scaling", "_rotation", "_opacity", "_label", "_orient_conf", "_features_dc", "_features_rest"):
        setattr(empty, n, torch.nn.Parameter(getattr(model, n).detach()[:0].clone()))
    empty.active_sh_degree = 2
    # poison whatever buffer the allocator hands the empty pass (and, if it were pooled, the next pass)
    junk = torch.full((64 << 20,), 0x7F, dtype=torch.uint8, device=dev)
    del junk
    pkg0 = render(cam, empty, dbg, syn.background(dev))
    assert float(pkg0["render"].abs().max()) == 0.0 and pkg0["radii"].numel() == 0
    del pkg0
    assert not any(fused._ImgLease._pools.values()), "the empty pass's workspace was pooled"
    with torch.no_grad():
        pkg = render(cam, model, dbg, syn.background(dev))
    assert torch.equal(pkg["render"], ref_img) and torch.equal(pkg["radii"], ref_radii)


def test_densification_statistics_inside_the_projection_backward_are_bit_identical_to_the_torch_form():
    """the stage-1 loop's per-iteration bookkeeping (src/train_gaussians.py:161-165,
    src/scene/gaussian_model.py:739-741: max_radii2D, xyz_gradient_accum += |viewspace grad.xy|, denom += 1 over the visible
    Gaussians) folded into k_project_bwd (pipe.densify_stats).  Three views in a row (accumulation), against
    densification_step's PyTorch form on the same gradients: bit for bit.  A view whose capacity guess overflowed leaves the
    statistics alone."""
    from gaussianhaircut_amd import _lib
    from gaussianhaircut_amd.scene.cameras import ring_cameras
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    from gaussianhaircut_amd.trainer import make_ground_truth, view_loss
    import gaussianhaircut_amd.diff_gaussian_rasterization as dgr
    dev = torch.device("cuda:0")
    spec = syn.CONFIGS["cfg1"]
    opt = OptimizationParams()
    opt.lambda_dorient = 0.1
    cams = ring_cameras(3, spec.W, spec.H, device=dev)
    bg = syn.background(dev)
    gt = syn.make_model(spec, dev)
    with torch.no_grad():
        gt._features_dc.add_(0.3)
    make_ground_truth(gt, cams, bg)
    a, b = syn.make_model(spec, dev), syn.make_model(spec, dev)
    for m in (a, b):
        m.training_setup(opt)
    stats_pipe = SimpleNamespace(debug=False, fused_projection=True, densify_stats=True)
    _lib.lib().ghr_set_deterministic(1)  # the two models' viewspace gradients must be the same bits
    try:
        for cam in cams:
            pa = render(cam, a, stats_pipe, bg)
            assert pa.densify_stats_done
            view_loss(pa, cam, opt).backward()
            pb = render(cam, b, FUSED, bg)
            assert not pb.densify_stats_done
            view_loss(pb, cam, opt).backward()
            assert torch.equal(pa["viewspace_points"].grad, pb["viewspace_points"].grad)
            with torch.no_grad():
                vis = pb["visibility_filter"]
                b.update_max_radii(pb["radii"], vis)
                b.add_densification_stats(pb["viewspace_points"], vis)
            a.optimizer.zero_grad()
            b.optimizer.zero_grad()
        torch.cuda.synchronize()
        assert float(b.denom.max()) == 3.0 and float(b.xyz_gradient_accum.abs().max()) > 0
        assert torch.equal(a.denom, b.denom) and torch.equal(a.max_radii2D, b.max_radii2D)
        assert torch.equal(a.xyz_gradient_accum, b.xyz_gradient_accum), \
            float((a.xyz_gradient_accum - b.xyz_gradient_accum).abs().max())
        # an overflowed view: a capacity far below the instance count -> the kernel skips the update
        before = [t.clone() for t in (a.xyz_gradient_accum, a.denom, a.max_radii2D)]
        saved = dict(dgr._R_HINT), {k: list(v) for k, v in dgr._R_RECENT.items()}
        dgr._R_RECENT.clear()
        dgr._R_HINT[dev.index] = 4096
        pipe = SimpleNamespace(debug=False, fused_projection=True, densify_stats=True, defer_count=True)
        pa = render(cams[0], a, pipe, bg)
        view_loss(pa, cams[0], opt).backward()
        assert pa.count.resolve()[1], "the guess was meant to overflow"
        torch.cuda.synchronize()
        for t0, t1 in zip(before, (a.xyz_gradient_accum, a.denom, a.max_radii2D)):
            assert torch.equal(t0, t1)
    finally:
        _lib.lib().ghr_set_deterministic(0)
        dgr._R_HINT.pop(dev.index, None)
        dgr._R_RECENT.clear()


def _same_bits(a, b):
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def test_adam_fused_into_the_last_projection_backward_is_bit_identical():
    """on one rank the step's LAST k_project_bwd applies the Adam update itself (ghr_adam_fuse: p, m, v read
    from one buffer set, written to the other, roles swapped after the step; the gradients of the step never reach HBM).  Same
    parameters, moments and step count as the separate k_adam_v4 pass, bit for bit, over a sequence with a single-view step, a
    step whose gradients are NaN (skipped: train_gaussians.py:174-181 -- the update is undone on the device), a two-view step on
    two streams, and a step whose capacity guess overflows (the overflowed view raises the step's flag; the trainer recomputes)."""
    import copy
    import gaussianhaircut_amd.diff_gaussian_rasterization as dgr
    from gaussianhaircut_amd import _lib
    from gaussianhaircut_amd.scene.cameras import ring_cameras
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    from gaussianhaircut_amd.trainer import make_ground_truth, training_step
    dev = torch.device("cuda:0")
    spec = syn.CONFIGS["tiny_strands"]
    opt = OptimizationParams()
    opt.lambda_dorient = 0.1
    cams = ring_cameras(4, spec.W, spec.H, device=dev)
    bg = syn.background(dev)
    gt = syn.make_model(spec, dev)
    with torch.no_grad():
        gt._features_dc.add_(0.3)
    make_ground_truth(gt, cams, bg)
    # step 2 (0-based) runs with a NaN opacity logit: its gradients are NaN, the producer-side flag goes up, the step is skipped
    plan = [([cams[0]], False), ([cams[1]], False), ([cams[1]], False), ([cams[2], cams[3]], False), ([cams[0]], True),
            ([cams[3]], False)]
    _lib.lib().ghr_set_deterministic(1)
    try:
        runs = {}
        for fused in (True, False):
            model = syn.make_model(spec, dev)
            model.training_setup(opt)
            o = model.optimizer
            trace = []
            for it, (views, overflow) in enumerate(plan):
                if overflow:  # a capacity guess far below the instance count
                    dgr._R_RECENT.clear()
                    dgr._R_HINT[dev.index] = 4096
                if it == 2:
                    with torch.no_grad():
                        keep = model._opacity[3].clone()
                        model._opacity[3] = float("nan")
                training_step(model, views, bg, opt, it + 1, fuse_adam=fused)
                torch.cuda.synchronize()
                if it == 2:
                    with torch.no_grad():
                        assert bool(torch.isnan(model._opacity[3]).all())  # (the skipped step left it alone)
                        model._opacity[3] = keep
                assert model._xyz.data_ptr() == o.flat_param.data_ptr(), "the parameters must alias the CURRENT flat buffer"
                trace.append((o.flat_param.clone(), o.exp_avg.clone(), o.exp_avg_sq.clone(), int(o.state_dev[0])))
            runs[fused] = trace
            # every step but the overflowed one (recomputed the blocking way, with the separate pass) was carried by the backward
            assert o.fused_steps == (len(plan) - 1 if fused else 0), o.fused_steps
        for it, (a, b) in enumerate(zip(runs[True], runs[False])):
            assert a[3] == b[3], (it, a[3], b[3])
            for x, y in zip(a[:3], b[:3]):
                assert _same_bits(x, y), (it, float((x - y).abs().max()))
        steps = [t[3] for t in runs[True]]
        assert steps == [1, 2, 2, 3, 4, 5], steps   # the NaN step did not count
        assert _same_bits(runs[True][2][0], runs[True][1][0])  # ... and left the parameters alone
        assert not _same_bits(runs[True][3][0], runs[True][2][0])
    finally:
        _lib.lib().ghr_set_deterministic(0)
        dgr._R_HINT.pop(dev.index, None)
        dgr._R_RECENT.clear()


def test_multi_view_steps_fold_their_sh_gradients_from_per_view_tables_bit_for_bit():
    """Round 6: in a step of several views on one rank every view but the one that carries the update leaves its dL/d(rgb) table
    (12 B per Gaussian) instead of read-modify-writing 192 B of SH gradients, and the tables are folded into the flat gradient
    once (optim.FusedAdam.begin_factored_views(gather=False)).  Same parameters, moments and step count as with the in-place
    accumulation, bit for bit: four-view and three-view steps with the update in the last backward, the same with the separate
    pass, a two-view step (separate pass only), a step whose capacity guess overflows, a NaN step; and a gradient somebody else
    left in ``.grad`` before the step survives the fold."""
    import gaussianhaircut_amd.diff_gaussian_rasterization as dgr
    from gaussianhaircut_amd import _lib, optim
    from gaussianhaircut_amd.scene.cameras import ring_cameras
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    from gaussianhaircut_amd.trainer import make_ground_truth, training_step
    dev = torch.device("cuda:0")
    spec = syn.CONFIGS["tiny_strands"]
    opt = OptimizationParams()
    opt.lambda_dorient = 0.1
    cams = ring_cameras(6, spec.W, spec.H, device=dev)
    bg = syn.background(dev)
    gt = syn.make_model(spec, dev)
    with torch.no_grad():
        gt._features_dc.add_(0.3)
    make_ground_truth(gt, cams, bg)
    plan = [(cams[:4], False, False), (cams[1:4], False, False), (cams[2:4], False, False), (cams[:4], True, False),
            (cams[2:6], False, True), (cams[:5], False, False)]
    degrees = [1, 1, 2, 2, 3, 3]  # the active SH degree of each step (the fold must use the step's, bands above it get zeros)
    _lib.lib().ghr_set_deterministic(1)
    saved = optim.FACTORED_SH_REDUCE
    try:
        for fused in (True, False):
            runs = {}
            for factored in (True, False):
                optim.FACTORED_SH_REDUCE = factored
                model = syn.make_model(spec, dev)
                model.training_setup(opt)
                o = model.optimizer
                folds = []
                orig = o._rebuild_sh_from_views
                o._rebuild_sh_from_views = lambda g, folds=folds, orig=orig, **k: (folds.append(int(g.shape[0])), orig(g, **k))[1]
                trace = []
                for it, (views, overflow, nan) in enumerate(plan):
                    model.active_sh_degree = degrees[it]
                    if overflow:
                        dgr._R_RECENT.clear()
                        dgr._R_HINT[dev.index] = 4096
                    if nan:
                        with torch.no_grad():
                            keep = model._opacity[3].clone()
                            model._opacity[3] = float("nan")
                    training_step(model, list(views), bg, opt, it + 1, fuse_adam=fused)
                    torch.cuda.synchronize()
                    if nan:
                        with torch.no_grad():
                            model._opacity[3] = keep
                    assert o._views is None
                    trace.append((o.flat_param.clone(), o.exp_avg.clone(), o.exp_avg_sq.clone(), int(o.state_dev[0])))
                runs[factored] = (trace, folds)
            (ta, fa), (tb, fb) = runs[True], runs[False]
            assert fb == [] and len(fa) >= 5, (fa, fb)
            # tables folded: all but the updating view's (fused) / all (separate pass); two views fold only with the separate pass
            assert fa[0] == (3 if fused else 4) and fa[1] == (2 if fused else 3), fa
            for it, (a, b) in enumerate(zip(ta, tb)):
                assert a[3] == b[3], (fused, it, a[3], b[3])
                for x, y in zip(a[:3], b[:3]):
                    assert _same_bits(x, y), (fused, it, float((x - y).abs().max()))
            assert [t[3] for t in ta] == [1, 2, 3, 4, 4, 5]
        # somebody else's gradient in .grad before the step: the fold adds to it
        res = []
        for factored in (True, False):
            optim.FACTORED_SH_REDUCE = factored
            model = syn.make_model(spec, dev)
            model.training_setup(opt)
            o = model.optimizer
            model._features_rest.grad.add_(0.5)
            model._features_dc.grad.add_(0.25)
            grads = []
            orig_step = o.step
            o.step = lambda *a, **k: (grads.append(o.flat_grad.detach().clone()) if o._views is None else
                                      (o.fold_own_views(), grads.append(o.flat_grad.detach().clone())), orig_step(*a, **k))[-1]
            training_step(model, list(cams[:3]), bg, opt, 1, fuse_adam=False)
            torch.cuda.synchronize()
            res.append(grads[0])
        P = model.get_xyz.shape[0]
        assert torch.allclose(res[0], res[1], rtol=1e-5, atol=1e-7)
        assert float((res[0][3 * P: 51 * P] - 0.25).abs().min()) >= 0.0 and float(res[0][6 * P: 51 * P].mean()) > 0.4
    finally:
        optim.FACTORED_SH_REDUCE = saved
        _lib.lib().ghr_set_deterministic(0)
        dgr._R_HINT.pop(dev.index, None)
        dgr._R_RECENT.clear()


def test_onepass_densify_and_prune_equals_the_stepwise_sequence_bit_for_bit():
    """scene/densification.py: with FusedAdam one densification event is ONE re-lay of the flat buffers (decisions on per-row
    scalars, every group gathered once by index) instead of the reference's clone / split / prune sequence with its ~60
    boolean-mask gathers (src/scene/gaussian_model.py:680-741, which the stepwise path mirrors and tests/test_reference_golden.py
    pins to the reference).  Same rows in the same order, parameters, moments, statistics and random samples, bit for bit --
    with and without a size threshold, and with an empty selection."""
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    from gaussianhaircut_amd.trainer import make_ground_truth, training_step
    dev = torch.device("cuda:0")
    spec = syn.CONFIGS["cfg1"]
    opt = OptimizationParams()
    opt.lambda_dorient = 0.1
    cam, bg = syn.make_view(spec, dev), syn.background(dev)
    gt = syn.make_model(spec, dev)
    with torch.no_grad():
        gt._features_dc.add_(0.3)
    make_ground_truth(gt, [cam], bg)
    from gaussianhaircut_amd import _lib
    _lib.lib().ghr_set_deterministic(1)  # (the two models must reach the event with the same bits)
    try:
        _onepass_cases(spec, opt, cam, bg, dev)
    finally:
        _lib.lib().ghr_set_deterministic(0)


def _onepass_cases(spec, opt, cam, bg, dev):
    from gaussianhaircut_amd.trainer import training_step
    for thr_q, size in ((0.5, None), (0.7, 20), (2.0, 20)):   # (quantile 2.0 -> a threshold nothing reaches)
        states = []
        for onepass in (True, False):
            m = syn.make_model(spec, dev)
            m.training_setup(opt)
            m.ONEPASS_DENSIFY = onepass
            for it in range(4):
                training_step(m, [cam], bg, opt, it + 1, densify_stats=True, fuse_adam=False)
            with torch.no_grad():  # some Gaussians nearly transparent: the opacity prune has work to do
                m._opacity[::7] = -7.0
            g = (m.xyz_gradient_accum / m.denom.clamp_min(1)).reshape(-1)
            thr = float(g[m.denom.reshape(-1) > 0].quantile(min(thr_q, 1.0))) * (10.0 if thr_q > 1 else 1.0)
            gen = torch.Generator(device=dev).manual_seed(5)
            P0 = m.get_xyz.shape[0]
            m.densify_and_prune(thr, 0.005, 2.5, size, generator=gen)
            torch.cuda.synchronize()
            o = m.optimizer
            states.append(dict(P=m.get_xyz.shape[0], p=o.flat_param.clone(), m=o.exp_avg.clone(), v=o.exp_avg_sq.clone(),
                               skip=o._skip_next, acc=m.xyz_gradient_accum.clone(), den=m.denom.clone(),
                               rad=m.max_radii2D.clone(), conf=m._orient_conf.detach().clone(), P0=P0))
            training_step(m, [cam], bg, opt, 10)   # the re-laid model trains on
        a, b = states
        assert a["P"] == b["P"] and a["skip"] == b["skip"], (a["P"], b["P"])
        if thr_q <= 1:
            assert a["P"] != a["P0"]
        for k in ("p", "m", "v", "acc", "den", "rad", "conf"):
            assert torch.equal(a[k], b[k]), (thr_q, size, k)
