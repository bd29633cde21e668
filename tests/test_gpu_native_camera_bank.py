"""`-m gpu`: the native view step with a camera bank (``ghr_view_step_camera``: compose, the view, the fold of the camera gradients
and the compose's backward as one call) against the Python path over the same bank (``_BankCompose`` + ``_RenderModelFused`` through
autograd): two models and two banks from one seed stepped side by side, model and bank compared bit for bit after every step.
Scenes and the state comparison are those of tests/test_gpu_native_step.py."""
import gc
import math

import pytest
import torch

import gaussianhaircut_amd.diff_gaussian_rasterization as dgr
import gaussianhaircut_amd.trainer as tr
from gaussianhaircut_amd import _lib
from gaussianhaircut_amd.scene.cameras import CameraBank
from tests.test_gpu_native_step import (TOO_SMALL, _assert_same_state, _CountingLib, _fresh_model, _same_bits, _scene, _state,  # noqa: F401
                                        clean_guess)

pytestmark = pytest.mark.gpu

STEPS, ITERATIONS_CAM, OVERFLOW_STEP = 7, 5, 3


def _bank(cams, opt, dev, use_barf=True, trainable_intrinsics=True, fused=None):
    bank = CameraBank(cams, use_barf=use_barf, trainable_intrinsics=trainable_intrinsics, device=dev, fused=fused)
    return bank.training_setup(opt)


def _bank_state(bank):
    return dict(params=bank.params.clone(), exp_avg=bank.exp_avg.clone(), exp_avg_sq=bank.exp_avg_sq.clone(),
                steps=bank.steps.clone(), touched=bank.touched.clone())


def _assert_same_bank(a, b, where):
    for k in ("params", "exp_avg", "exp_avg_sq"):
        assert _same_bits(a[k], b[k]), (where, k, float((a[k] - b[k]).abs().max()))
    assert torch.equal(a["steps"], b["steps"]), (where, a["steps"].tolist(), b["steps"].tolist())
    assert not a["touched"].any() and not b["touched"].any(), where


@pytest.mark.parametrize("trainable_intrinsics", [True, False])
@pytest.mark.parametrize("fuse_adam", [True, False])
@pytest.mark.parametrize("use_barf", [True, False])
@pytest.mark.parametrize("V", [1, 2, 3])
def test_native_banked_steps_equal_python_banked_steps_bit_for_bit(clean_guess, V, use_barf, fuse_adam, trainable_intrinsics):
    """7 steps with ``opt.iterations_cam = 5``: steps 1 .. 4 train the bank (one ``ghr_view_step_camera`` per view), steps 5 .. 7
    run its frozen cameras through the plain ``ghr_view_step``.  Step 3 has its capacity guess forced too small and is recomputed
    (the camera gradients of the discarded pass must not be counted).  V = 1, 2 (two streams) and 3 (the views' own SH tables: a
    bank view writes its camera centre behind its table after the call has composed it)."""
    dev = clean_guess
    spec, opt, cams, bg = _scene("A", dev, 4)
    opt.iterations_cam = ITERATIONS_CAM
    models = {n: _fresh_model(spec, opt, dev) for n in (False, True)}
    banks = {n: _bank(cams, opt, dev, use_barf, trainable_intrinsics) for n in (False, True)}
    init = banks[True].params.clone()
    paths = []
    for it in range(1, STEPS + 1):
        states, bstates = {}, {}
        for native in (False, True):
            model, bank = models[native], banks[native]
            views = [bank[(it + k) % len(bank)] for k in range(V)]
            if it == OVERFLOW_STEP:
                dgr._R_RECENT.clear()
                dgr._R_HINT[dev.index] = TOO_SMALL
            loss = tr.training_step(model, views, bg, opt, it, fuse_adam=fuse_adam, camera_bank=bank, native=native)
            path = tr.last_step_path()
            torch.cuda.synchronize()
            if it == OVERFLOW_STEP:
                assert dgr.LAST_STATS["num_rendered"] > TOO_SMALL  # (the guess WAS too small: the step was recomputed)
            states[native], bstates[native] = _state(model, loss), _bank_state(bank)
            if native:
                paths.append(path)
            else:
                assert path == "python"
        where = (V, use_barf, fuse_adam, trainable_intrinsics, it)
        _assert_same_state(states[False], states[True], where)
        _assert_same_bank(bstates[False], bstates[True], where)
    assert paths == ["native"] * STEPS, paths
    bank = banks[True]
    # every camera was viewed in steps 1 .. 4 and none stepped from iterations_cam on
    expect = [sum(1 for it in range(1, ITERATIONS_CAM) for k in range(V) if (it + k) % 4 == i) for i in range(4)]
    assert bank.steps.tolist() == expect, (bank.steps.tolist(), expect)
    moved = (bank.params != init)
    assert bool(moved[:, :bank.rot_dim + 3].any()) and bool(moved[:, bank.rot_dim + 3:].any()) == trainable_intrinsics
    assert bool(torch.isfinite(bank.params).all())


@pytest.mark.parametrize("fuse_adam", [True, False])
@pytest.mark.parametrize("V", [1, 2, 3])
def test_a_steady_native_banked_step_is_one_call_per_view_and_allocates_nothing(clean_guess, monkeypatch, V, fuse_adam):
    """A steady native banked step crosses into the library V times for its views (``ghr_view_step_camera``) and once for the
    cameras' Adam; the separate Gaussian pass adds what it adds to a step of constant cameras.  Nothing is allocated."""
    dev = clean_guess
    monkeypatch.setenv(tr.NATIVE_STEP_ENV, "1")
    spec, opt, cams, bg = _scene("B", dev, 3)
    model = _fresh_model(spec, opt, dev, degree=3)
    bank = _bank(cams, opt, dev)
    views = [bank[i] for i in range(V)]
    for it in range(1, 4):
        tr.training_step(model, views, bg, opt, it, fuse_adam=fuse_adam, camera_bank=bank)
    assert tr.last_step_path() == "native"
    torch.cuda.synchronize()
    gc.collect()  # (cyclic garbage of the set-up must not be freed in the middle of the measured step)
    real = _lib.lib()
    counting = _CountingLib(real)
    monkeypatch.setattr(_lib, "_lib", counting)
    before = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    held = torch.cuda.memory_allocated(dev)
    loss = tr.training_step(model, views, bg, opt, 4, fuse_adam=fuse_adam, camera_bank=bank)
    after = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    monkeypatch.setattr(_lib, "_lib", real)
    torch.cuda.synchronize()
    assert tr.last_step_path() == "native"
    expect = {"ghr_view_step_camera": V, "ghr_camera_adam_step": 1}
    if not fuse_adam:
        expect["ghr_adam_step"] = 1
        if V >= 2:
            expect["ghr_sh_grad_from_views"] = 1
    assert counting.calls == expect, counting.calls
    assert torch.cuda.memory_allocated(dev) == held and after == before, (before, after)
    assert math.isfinite(float(loss)) and bank.steps.tolist()[:V] == [4] * V


def test_an_unfused_bank_takes_the_python_path_and_native_true_raises(clean_guess, monkeypatch):
    dev = clean_guess
    spec, opt, cams, bg = _scene("A", dev, 2)
    model = _fresh_model(spec, opt, dev)
    bank = _bank(cams, opt, dev, fused=False)
    tr.training_step(model, [bank[0]], bg, opt, 1, camera_bank=bank)
    torch.cuda.synchronize()
    before, bank_before = _state(model, torch.zeros((), device=dev)), _bank_state(bank)
    with pytest.raises(RuntimeError, match="native=True"):
        tr.training_step(model, [bank[1]], bg, opt, 2, camera_bank=bank, native=True)
    torch.cuda.synchronize()
    _assert_same_state(before, _state(model, torch.zeros((), device=dev)), "a refused step changes nothing")
    _assert_same_bank(bank_before, _bank_state(bank), "a refused step changes nothing")
    monkeypatch.setenv(tr.NATIVE_STEP_ENV, "1")  # the knob alone: the step falls back
    tr.training_step(model, [bank[1]], bg, opt, 2, camera_bank=bank)
    assert tr.last_step_path() == "python" and bank.steps.tolist() == [1, 1]
    torch.cuda.synchronize()
