"""`-m gpu`: the native view step (``training_step(native=True)``: one ``ghr_view_step`` call per view on buffers allocated once)
against the Python path it stands in for (render + view_loss + backward through autograd): two models from one seed stepped
side by side, every piece of state compared bit for bit after every step."""
import collections
import math

import pytest
import torch

import gaussianhaircut_amd.diff_gaussian_rasterization as dgr
import gaussianhaircut_amd.trainer as tr
from gaussianhaircut_amd import _lib
from gaussianhaircut_amd.scene.cameras import ring_cameras
from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
from gaussianhaircut_amd.utils import synthetic as syn

pytestmark = pytest.mark.gpu

# The smallest scenes at which the bookkeeping can go wrong.  A: one full 256-row block of the projection kernels plus one row;
# rows of 33 floats are not 16-B aligned, so the loss runs in its tile form; partial 16 x 16 tiles in both directions.
# B: rows of 64 floats, so the loss runs in its marching form.
SCENES = {"A": syn.WorkloadSpec("native_a_257_33x17", 257, 33, 17, 21, "random", math.log(0.1)),
          "B": syn.WorkloadSpec("native_b_1000_64x48", 1000, 64, 48, 22, "random", math.log(0.08))}
STEPS, NAN_STEP, DEGREE_STEP, OVERFLOW_STEP = 20, 7, 10, 13
TOO_SMALL = 64  # a capacity guess below any view's instance count


def _same_bits(a, b):
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _scene(name, dev, n_cams):
    spec = SCENES[name]
    opt = OptimizationParams()
    opt.lambda_dorient = 0.1
    cams = ring_cameras(n_cams, spec.W, spec.H, device=dev)
    bg = syn.background(dev)
    gt = syn.make_model(spec, dev)
    with torch.no_grad():
        gt._features_dc.add_(0.3)
    tr.make_ground_truth(gt, cams, bg)
    return spec, opt, cams, bg


def _fresh_model(spec, opt, dev, degree=1):
    model = syn.make_model(spec, dev)
    model.active_sh_degree = degree
    model.training_setup(opt)
    return model


def _state(model, loss):
    o = model.optimizer
    flags = o._fuse["flags"].clone() if o._fuse is not None else None
    return dict(p=o.flat_param.clone(), m=o.exp_avg.clone(), v=o.exp_avg_sq.clone(), state=o.state_dev.clone(), flags=flags,
                parity=None if o._fuse is None else o._fuse["parity"], accum=model.xyz_gradient_accum.clone(),
                denom=model.denom.clone(), radii=model.max_radii2D.clone(), loss=loss.detach().clone(),
                fused_steps=o.fused_steps)


def _assert_same_state(a, b, where):
    for k in ("p", "m", "v", "accum", "denom", "radii", "loss"):
        assert _same_bits(a[k], b[k]), (where, k, float((a[k].float() - b[k].float()).abs().max()))
    assert torch.equal(a["state"], b["state"]), (where, a["state"].tolist(), b["state"].tolist())
    assert (a["flags"] is None) == (b["flags"] is None) and a["parity"] == b["parity"], where
    if a["flags"] is not None:
        assert torch.equal(a["flags"], b["flags"]), (where, a["flags"].tolist(), b["flags"].tolist())
    assert a["fused_steps"] == b["fused_steps"], (where, a["fused_steps"], b["fused_steps"])


@pytest.fixture
def clean_guess():
    """The capacity guess is process-wide state: every test starts without one and leaves none; the gradient walk is ordered."""
    dev = torch.device("cuda:0")
    saved = dict(dgr._R_HINT), {k: list(v) for k, v in dgr._R_RECENT.items()}, dict(dgr._R_P)
    dgr._R_HINT.pop(dev.index, None)
    dgr._R_RECENT.clear()
    was_ordered = _lib.lib().ghr_set_deterministic(1)
    try:
        yield dev
    finally:
        _lib.lib().ghr_set_deterministic(was_ordered)
        dgr._R_HINT.clear()
        dgr._R_HINT.update(saved[0])
        dgr._R_RECENT.clear()
        for k, counts in saved[1].items():
            dgr._R_RECENT[k] = collections.deque(counts, maxlen=64)
        dgr._R_P.clear()
        dgr._R_P.update(saved[2])


@pytest.mark.parametrize("densify_stats", [False, True])
@pytest.mark.parametrize("fuse_adam", [True, False])
@pytest.mark.parametrize("V", [1, 2, 3])
@pytest.mark.parametrize("scene", ["A", "B"])
def test_native_steps_equal_python_steps_bit_for_bit(clean_guess, scene, V, fuse_adam, densify_stats):
    """20 steps each of ``native=False`` and ``native=True``: V = 1 (the current stream), 2 (two streams, the event chain around
    the shared gradient buffer) and 3 (two streams and the views' own SH tables, folded inside the call of the view that carries
    the update); the update inside the last backward or as the separate pass; the densification statistics inside the backward;
    an SH-degree step; a step with a NaN gradient (the skip rule) and one whose capacity guess is too small (the memory-safe
    clamped overflow: both are provoked the way tests/test_gpu_fused.py provokes them)."""
    dev = clean_guess
    spec, opt, cams, bg = _scene(scene, dev, 4)
    models = {False: _fresh_model(spec, opt, dev), True: _fresh_model(spec, opt, dev)}
    paths = []
    # the fold of the views' SH tables INSIDE the call of the view that carries the update (ghr_view_step_args.sh_fold)
    o, folds = models[True].optimizer, []
    fold_args = o.fold_own_views_args
    o.fold_own_views_args = lambda: (lambda f: (folds.append(f is not None), f)[1])(fold_args())
    for it in range(1, STEPS + 1):
        views = [cams[(it + k) % len(cams)] for k in range(V)]
        states = {}
        for native in (False, True):
            model = models[native]
            if it == DEGREE_STEP:
                model.oneupSHdegree()
            if it == OVERFLOW_STEP:
                dgr._R_RECENT.clear()
                dgr._R_HINT[dev.index] = TOO_SMALL
            if it == NAN_STEP:
                with torch.no_grad():
                    keep = model._opacity[3].clone()
                    model._opacity[3] = float("nan")
            loss = tr.training_step(model, views, bg, opt, it, fuse_adam=fuse_adam, densify_stats=densify_stats, native=native)
            path = tr.last_step_path()
            torch.cuda.synchronize()
            if it == NAN_STEP:
                with torch.no_grad():
                    assert bool(torch.isnan(model._opacity[3]).all())  # (the skipped step left it alone)
                    model._opacity[3] = keep
            if it == OVERFLOW_STEP:
                assert dgr.LAST_STATS["num_rendered"] > TOO_SMALL  # (the guess WAS too small: the step was recomputed)
            states[native] = _state(model, loss)
            if native:
                paths.append(path)
            else:
                assert path == "python"
        _assert_same_state(states[False], states[True], (scene, V, fuse_adam, densify_stats, it))
        if it == NAN_STEP:
            assert int(states[True]["state"][0]) == NAN_STEP - 1  # the step did not count
    # (rendering the ground truth has left a capacity guess for this model size: the very first step runs natively already,
    # and so does the one after the overflowed step, whose blocking recomputation learns the count again)
    assert paths == ["native"] * STEPS, paths
    # three views with the update in the last backward: every step's last call carried a fold of the two earlier views' tables
    # (the separate pass folds in front of ghr_adam_step instead; fewer views keep no tables)
    assert folds == ([True] * STEPS if V == 3 and fuse_adam else []), folds
    assert int(models[True].optimizer.state_dev[0]) == STEPS - 1
    assert models[True].active_sh_degree == 2
    if densify_stats:
        assert float(models[True].denom.sum()) > 0


class _CountingLib:
    """``_lib.lib()`` with every call of a ``ghr_*`` function counted."""

    def __init__(self, real):
        self._real, self.calls = real, {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("ghr_"):
            return fn

        def counted(*a, **k):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a, **k)
        return counted


@pytest.mark.parametrize("fuse_adam", [True, False])
@pytest.mark.parametrize("V", [1, 2, 3])
def test_a_steady_native_step_is_one_call_per_view_and_allocates_nothing(clean_guess, monkeypatch, V, fuse_adam):
    """After the warm-up a native step crosses into the library V times for its views -- with the update inside the last
    backward that is every call of the step; the separate pass adds its ``ghr_adam_step`` and, with several views, the one fold
    of their SH tables in front of it -- and asks the caching allocator
    for nothing.  The path is chosen through ``GHR_NATIVE_STEP`` here, as ``bench.py`` would."""
    dev = clean_guess
    monkeypatch.setenv(tr.NATIVE_STEP_ENV, "1")
    spec, opt, cams, bg = _scene("B", dev, 3)
    model = _fresh_model(spec, opt, dev, degree=3)
    views = cams[:V]
    for it in range(1, 4):  # three warm-up steps
        tr.training_step(model, views, bg, opt, it, fuse_adam=fuse_adam)
    assert tr.last_step_path() == "native"
    torch.cuda.synchronize()
    real = _lib.lib()
    counting = _CountingLib(real)
    monkeypatch.setattr(_lib, "_lib", counting)
    before = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    loss = tr.training_step(model, views, bg, opt, 4, fuse_adam=fuse_adam)
    after = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    monkeypatch.setattr(_lib, "_lib", real)
    torch.cuda.synchronize()
    assert tr.last_step_path() == "native"
    expect = {"ghr_view_step": V}
    if not fuse_adam:  # the update is not the views': the separate pass, and in front of it the fold of the views' own SH tables
        expect["ghr_adam_step"] = 1
        if V >= 2:
            expect["ghr_sh_grad_from_views"] = 1
    assert counting.calls == expect, counting.calls
    assert after == before, (before, after)
    assert math.isfinite(float(loss))


def test_a_trained_camera_tensor_takes_the_python_path(clean_guess, monkeypatch):
    """A camera tensor that requires grad gets its gradient through autograd: such a step falls back to the Python path (same
    results as without the knob), and asking for the native path outright raises."""
    dev = clean_guess
    spec, opt, cams, bg = _scene("A", dev, 2)
    for c in cams:
        c.camera_center.requires_grad_(True)
    runs = {}
    for knob in ("0", "1"):
        monkeypatch.setenv(tr.NATIVE_STEP_ENV, knob)
        model = _fresh_model(spec, opt, dev)
        trace = []
        for it in range(1, 5):
            loss = tr.training_step(model, [cams[it % 2]], bg, opt, it)
            assert tr.last_step_path() == "python"
            torch.cuda.synchronize()
            trace.append(_state(model, loss))
        runs[knob] = trace
    for it, (a, b) in enumerate(zip(runs["0"], runs["1"])):
        _assert_same_state(a, b, it)
    assert all(c.camera_center.grad is not None for c in cams)
    before = _state(model, loss)
    with pytest.raises(RuntimeError, match="native=True"):
        tr.training_step(model, [cams[0]], bg, opt, 5, native=True)
    _assert_same_state(before, _state(model, loss), "a refused step changes nothing")
    for c in cams:  # ... and the same cameras, constant again, run natively
        c.camera_center.requires_grad_(False)
    tr.training_step(model, [cams[0]], bg, opt, 5, native=True)
    assert tr.last_step_path() == "native"
    cams[0].FoVx.requires_grad_(True)  # a FoV that starts to be trained AFTER the camera ran natively is noticed, too
    with pytest.raises(RuntimeError, match="native=True"):
        tr.training_step(model, [cams[0]], bg, opt, 6, native=True)
    cams[0].FoVx.requires_grad_(False)
    # without a capacity guess (the first step of a process, or the first after the model changed size) a view has to wait for its
    # instance count: that step runs the Python way whatever was asked for, and learns the guess the next one uses
    dgr._R_HINT.pop(dev.index, None)
    dgr._R_RECENT.clear()
    tr.training_step(model, [cams[1]], bg, opt, 6, native=True)
    assert tr.last_step_path() == "python"
    tr.training_step(model, [cams[0]], bg, opt, 7, native=True)
    assert tr.last_step_path() == "native"
    torch.cuda.synchronize()


@pytest.mark.parametrize("V", [1, 3])
def test_native_step_with_the_default_gradient_walk(V):
    """The same call with the gradient walk in its default form (float atomics into the gradient lines in scheduling order: not
    reproducible to the bit, so not comparable bit for bit).  The forward pass and the loss have a fixed order: the first step's
    loss is the Python path's, bit for bit.  The first Adam step from zero moments moves every parameter by
    lr g / (|g| + eps), at most its group's lr in magnitude, whatever g is: two runs differ by at most 2 lr per element."""
    dev = torch.device("cuda:0")
    assert _lib.lib().ghr_set_deterministic(0) == 0  # (the default form; the call returns the previous setting)
    spec, opt, cams, bg = _scene("B", dev, 3)
    runs = {}
    for native in (False, True):
        model = _fresh_model(spec, opt, dev, degree=3)
        p0 = model.optimizer.flat_param.clone()
        loss = tr.training_step(model, cams[:V], bg, opt, 1, native=native)
        assert tr.last_step_path() == ("native" if native else "python")
        torch.cuda.synchronize()
        runs[native] = (loss.detach().clone(), model.optimizer.flat_param.clone(), int(model.optimizer.state_dev[0]))
        lr_max = max(float(g["lr"]) for g in model.optimizer.param_groups)
        assert not torch.equal(runs[native][1], p0) and bool(torch.isfinite(runs[native][1]).all())
    assert _same_bits(runs[False][0], runs[True][0])
    assert runs[False][2] == runs[True][2] == 1
    assert float((runs[False][1] - runs[True][1]).abs().max()) <= 2.0 * lr_max
