"""scene.cameras.CameraBank on the CPU: its PyTorch form against the reference's own Camera (tests/golden/
reference_camera_bank_golden.npz, made by tests/golden/make_reference_camera_bank_golden.py from src/scene/cameras.py and
src/utils/camera_opt_utils.py), persistence, and training_step's camera_bank argument.

The criterion (``check``) has the form of tests/test_camera_grads.py::_check_cam, elementwise:
    |got - f64| <= tol * max|f64| + 3 |ref32 - f64|,   tol = 1e-5 for outputs and gradients
-- the reference's own fp32 chain stays within 1.9e-7 of max on these cases, so 1e-5 leaves room for another summation order in
the 4x4 products and the series, and for nothing else."""
import copy
import os
import pickle

import numpy as np
import pytest
import torch

from gaussianhaircut_amd.scene.cameras import BankCamera, CameraBank, ring_cameras
from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
from gaussianhaircut_amd.utils import synthetic as syn
from tests.golden import make_reference_camera_bank_golden as mk

TOL = 1e-5
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_camera_bank_golden.npz")
OUT_NAMES = ("view", "full", "center", "fovx", "fovy", "proj")   # order of tensors()
PARAMS = [True, False]   # use_barf


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def sub(gold, use_barf):
    tag = mk.TAGS[use_barf]
    return {k[len(tag):]: v for k, v in gold.items() if k.startswith(tag)}


def check(got, r64, r32, what, tol=TOL):
    """Returns the worst err / bar (must be <= 1) of one array against the double arbiter; asserts it."""
    got, r64, r32 = (np.asarray(a, dtype=np.float64) for a in (got, r64, r32))
    assert got.shape == r64.shape, (what, got.shape, r64.shape)
    assert np.isfinite(got).all(), what
    bar = tol * np.abs(r64).max() + 3.0 * np.abs(r32 - r64)
    err = np.abs(got - r64)
    ratio = float((err / (bar + 1e-300)).max()) if err.size else 0.0
    assert (err <= bar + 1e-30).all(), (what, ratio, got, r64)
    return ratio


def groups(use_barf):
    rd = 3 if use_barf else 6
    return (("rotation", slice(0, rd)), ("translation", slice(rd, rd + 3)), ("fov", slice(rd + 3, rd + 5)))


def check_grad_row(got, r64, r32, use_barf, what):
    """a gradient row, group by group (the reference's three parameters per camera)"""
    return max(check(got[s], r64[s], r32[s], "%s %s" % (what, n)) for n, s in groups(use_barf))


def bank_from(ref, use_barf, device="cpu", n_pad=0, **kw):
    """A bank of the golden's six cameras (+ n_pad copies of the first behind them) holding the golden's parameter rows."""
    recs = [(ref["R"][i], ref["T"][i], float(ref["fov0"][i, 0]), float(ref["fov0"][i, 1]), mk.W, mk.H, "ring%03d" % (mk.FIRST + i))
            for i in range(len(ref["R"]))]
    recs += [recs[0][:6] + ("pad%03d" % k,) for k in range(n_pad)]
    bank = CameraBank(recs, use_barf=use_barf, device=device, **kw)
    with torch.no_grad():
        bank.params[:len(ref["params"])] = torch.from_numpy(ref["params"]).to(device)
    return bank


def cotangent_loss(t, ref, i, names, device="cpu"):
    return sum((t[OUT_NAMES.index(n)] * torch.as_tensor(np.asarray(ref["cot_" + n][i])).to(device)).sum() for n in names)


@pytest.mark.parametrize("use_barf", PARAMS)
def test_bank_constants_are_the_reference_cameras(gold, use_barf):
    ref = sub(gold, use_barf)
    bank = bank_from(ref, use_barf)
    c = bank.consts.numpy()
    assert np.array_equal(c[:, :16].reshape(-1, 4, 4), ref["w2c"])
    assert np.array_equal(c[:, 16:18], ref["fov0"])
    assert isinstance(bank[2], BankCamera) and bank[2].image_name == "ring007" and len(bank) == 6
    assert (bank[2].image_width, bank[2].image_height, bank[2].znear, bank[2].zfar) == (mk.W, mk.H, 0.01, 100.0)
    rd = bank.rot_dim
    assert bank[2]._rotation_res.shape == (rd,) and bank[2]._translation_res.shape == (3,) and bank[2]._fov_res.shape == (2,)
    assert bank[2]._fov_res.data_ptr() == bank.params[2, rd + 3:].data_ptr()   # views of the bank's row


@pytest.mark.parametrize("use_barf", PARAMS)
def test_torch_form_reproduces_the_reference_camera(gold, use_barf):
    ref = sub(gold, use_barf)
    bank = bank_from(ref, use_barf)
    worst_o = worst_g = 0.0
    for i in range(len(bank)):
        t = bank[i].tensors()
        for n, x in zip(OUT_NAMES, t):
            worst_o = max(worst_o, check(x.detach().numpy(), ref[n + "64"][i], ref[n + "32"][i], "%s[%d]" % (n, i)))
        cotangent_loss(t, ref, i, ("view", "full", "center", "fovx", "fovy")).backward()
        worst_g = max(worst_g, check_grad_row(bank.grads[i].numpy(), ref["grad64"][i], ref["grad32"][i], use_barf, "grad[%d]" % i))
    assert bank.touched.tolist() == [1] * 6
    # world_view_transform's cotangent alone, into a fresh bank
    bank = bank_from(ref, use_barf)
    for i in range(len(bank)):
        cotangent_loss(bank[i].tensors(), ref, i, ("view",)).backward()
        worst_g = max(worst_g, check_grad_row(bank.grads[i].numpy(), ref["gradview64"][i], ref["gradview32"][i], use_barf, "gradview[%d]" % i))
    bank = bank_from(ref, use_barf)   # projection_matrix's cotangent alone: only the FoV residual gets a gradient
    for i in range(len(bank)):
        cotangent_loss(bank[i].tensors(), ref, i, ("proj",)).backward()
        worst_g = max(worst_g, check_grad_row(bank.grads[i].numpy(), ref["gradproj64"][i], ref["gradproj32"][i], use_barf, "gradproj[%d]" % i))
        assert not bank.grads[i, :bank.rot_dim + 3].any() and bank.grads[i, bank.rot_dim + 3:].all()
    print("camera bank, PyTorch form, use_barf=%s: worst err / bar outputs %.3g gradients %.3g" % (use_barf, worst_o, worst_g))


@pytest.mark.parametrize("use_barf", PARAMS)
def test_value_and_gradient_are_finite_at_zero_residual(use_barf):
    bank = CameraBank(ring_cameras(3, 64, 48, roll_deg=20.0), use_barf=use_barf)
    t = bank[1].tensors()
    assert all(torch.isfinite(x).all() for x in t)
    sum(x.sum() for x in t[:5]).backward()
    g = bank.grads[1].clone()
    assert torch.isfinite(g).all() and (g != 0).any()
    if use_barf:  # the generators' gradients: every component of w gets one
        assert (g[:3] != 0).all()
    assert torch.equal(bank.grads[0], torch.zeros_like(g)) and bank.touched.tolist() == [0, 1, 0]
    # a second backward into a touched row adds
    sum(x.sum() for x in bank[1].tensors()[:5]).backward()
    assert torch.allclose(bank.grads[1], 2 * g)


@pytest.mark.parametrize("use_barf", PARAMS)
def test_frozen_groups_get_no_gradient_and_no_update(use_barf):
    cams = ring_cameras(3, 64, 48, roll_deg=20.0)
    opt = OptimizationParams()
    bank = CameraBank(cams, use_barf=use_barf, trainable_cameras=False).training_setup(opt)
    rd = bank.rot_dim
    sum(x.sum() for x in bank[0].tensors()[:5]).backward()
    assert torch.equal(bank.grads[0, :rd + 3], torch.zeros(rd + 3)) and (bank.grads[0, rd + 3:] != 0).all()
    before = bank.params.clone()
    bank.step(1)
    assert torch.equal(bank.params[:, :rd + 3], before[:, :rd + 3]) and (bank.params[0, rd + 3:] != before[0, rd + 3:]).all()
    assert torch.equal(bank.exp_avg[:, :rd + 3], torch.zeros(3, rd + 3))
    bank = CameraBank(cams, use_barf=use_barf, trainable_intrinsics=False)
    sum(x.sum() for x in bank[0].tensors()[:5]).backward()
    assert torch.equal(bank.grads[0, rd + 3:], torch.zeros(2)) and (bank.grads[0, :rd + 3] != 0).any()
    bank = CameraBank(cams, use_barf=use_barf, trainable_cameras=False, trainable_intrinsics=False)
    assert not any(x.requires_grad for x in bank[0].tensors())


def _stepped_bank(use_barf, steps=3):
    opt = OptimizationParams()
    bank = CameraBank(ring_cameras(4, 64, 48, roll_deg=20.0), use_barf=use_barf).training_setup(opt, spatial_lr_scale=2.0)
    for it in range(steps):
        sum((x * x).sum() for x in bank[it % 2].tensors()[:5]).backward()
        bank.step(it + 1)
    return bank, opt


@pytest.mark.parametrize("use_barf", PARAMS)
def test_step_counts_are_per_camera_and_state_dict_round_trips(use_barf):
    bank, opt = _stepped_bank(use_barf)
    assert bank.steps.tolist() == [2, 1, 0, 0] and bank.touched.tolist() == [0] * 4
    assert torch.equal(bank.grads, torch.zeros_like(bank.grads))
    init = CameraBank(ring_cameras(4, 64, 48, roll_deg=20.0), use_barf=use_barf).params
    assert (bank.params[:2] != init[:2]).any(dim=1).all() and torch.equal(bank.params[2:], init[2:])
    sd = pickle.loads(pickle.dumps(bank.state_dict()))
    other = CameraBank(ring_cameras(4, 64, 48, roll_deg=20.0), use_barf=use_barf).training_setup(opt, spatial_lr_scale=2.0)
    other.load_state_dict(sd)
    for k in ("params", "exp_avg", "exp_avg_sq", "steps"):
        assert torch.equal(getattr(other, k), getattr(bank, k)), k
    # ... and the two continue identically
    for b in (bank, other):
        sum((x * x).sum() for x in b[0].tensors()[:5]).backward()
        b.step(4)
    assert torch.equal(other.params, bank.params) and other.steps.tolist() == [3, 1, 0, 0]
    with pytest.raises(ValueError):
        CameraBank(ring_cameras(4, 64, 48), use_barf=not use_barf).load_state_dict(sd)
    # the translation's learning rate follows its schedule, the other two are constants
    r0, t0, f0 = bank.learning_rates(0)
    r1, t1, f1 = bank.learning_rates(opt.cam_lr_max_steps)
    assert (r0, f0, r1, f1) == (opt.cam_rotation_lr, opt.cam_fov_lr, opt.cam_rotation_lr, opt.cam_fov_lr)
    assert t0 == pytest.approx(2.0 * opt.cam_translation_lr_init) and t1 == pytest.approx(2.0 * opt.cam_translation_lr_final)
    # from iterations_cam on the step is a no-op
    sum((x * x).sum() for x in bank[0].tensors()[:5]).backward()
    before = bank.params.clone()
    bank.step(opt.iterations_cam)
    assert torch.equal(bank.params, before) and bank.steps.tolist() == [3, 1, 0, 0]


def test_nan_in_a_viewed_camera_skips_the_whole_step_on_the_torch_form():
    bank, opt = _stepped_bank(True, steps=2)
    sum((x * x).sum() for x in bank[0].tensors()[:5]).backward()
    sum((x * x).sum() for x in bank[1].tensors()[:5]).backward()
    with torch.no_grad():
        bank.grads[1, 2] = float("nan")
        bank.grads[3, 0] = float("nan")   # stale, in a row nobody viewed: ignored
    keep = {k: getattr(bank, k).clone() for k in ("params", "exp_avg", "exp_avg_sq", "steps")}
    bank.step(3)
    for k, v in keep.items():
        assert torch.equal(getattr(bank, k), v), k
    assert bank.touched.tolist() == [0] * 4 and torch.equal(bank.grads[:3], torch.zeros(3, bank.width))
    sum((x * x).sum() for x in bank[0].tensors()[:5]).backward()
    bank.step(4)   # the stale NaN of row 3 does not stop a later step
    assert bank.steps.tolist() == [2, 1, 0, 0] and (bank.params[0] != keep["params"][0]).any()
    sum((x * x).sum() for x in bank[3].tensors()[:5]).backward()   # ... and is overwritten when its row is next viewed
    assert torch.isfinite(bank.grads[3]).all()


@pytest.mark.parametrize("use_barf", PARAMS)
def test_reference_pickles_round_trip(use_barf):
    bank, opt = _stepped_bank(use_barf)
    dicts, matrices = pickle.loads(pickle.dumps(bank.reference_pickles()))
    names = [c.image_name for c in bank]
    assert names == ["ring%03d" % k for k in range(4)]
    assert all(list(d) == names for d in dicts) and list(matrices) == names
    rd = bank.rot_dim
    assert dicts[0][names[1]].shape == (rd,) and dicts[1][names[1]].shape == (3,) and dicts[2][names[1]].shape == (2,)
    full = bank.compose_all()[1]
    assert all(torch.equal(matrices[n], full[i]) for i, n in enumerate(names))
    assert torch.allclose(full[1], bank[1].full_proj_transform.detach(), rtol=0, atol=0)
    other = CameraBank(ring_cameras(4, 64, 48, roll_deg=20.0), use_barf=use_barf)
    other.load_reference_pickles(dicts)
    assert torch.equal(other.params, bank.params)
    frozen = CameraBank(ring_cameras(4, 64, 48), use_barf=use_barf, trainable_cameras=False)
    (rot, tra, fov), _ = frozen.reference_pickles()
    assert rot == {} and tra == {} and list(fov) == names


def test_optimization_params_carry_the_reference_camera_defaults():
    opt = OptimizationParams()
    assert (opt.iterations_cam, opt.cam_lr_max_steps, opt.cam_rotation_lr, opt.cam_translation_lr_init,
            opt.cam_translation_lr_final, opt.cam_fov_lr) == (15000, 15000, 0.001, 0.0016, 0.000016, 0.001)


def test_training_step_checks_its_camera_bank_arguments(monkeypatch):
    from gaussianhaircut_amd import trainer
    opt = OptimizationParams()
    bank = CameraBank(ring_cameras(3, 64, 48), use_barf=True).training_setup(opt)
    other = CameraBank(ring_cameras(3, 64, 48), use_barf=True).training_setup(opt)
    with pytest.raises(ValueError, match="distinct"):
        trainer.training_step(None, [bank[0], bank[1], bank[0]], None, opt, 1, camera_bank=bank)
    with pytest.raises(ValueError, match="camera of that bank"):
        trainer.training_step(None, [bank[0], other[1]], None, opt, 1, camera_bank=bank)
    monkeypatch.setattr(trainer, "_world_size", lambda: 2)
    with pytest.raises(NotImplementedError):
        trainer.training_step(None, [bank[0]], None, opt, 1, camera_bank=bank)


def test_training_step_on_the_cpu_oracle_path_with_and_without_a_bank():
    """camera_bank=None changes nothing (same parameters, bit for bit, as leaving the argument out); with a bank the viewed
    cameras are stepped after the Gaussians, the others stay."""
    from gaussianhaircut_amd.trainer import make_ground_truth, training_step
    from tests.oracle_backend import oracle_rasterizer
    spec = syn.CONFIGS["tiny"]
    opt = OptimizationParams()
    cams = ring_cameras(32, spec.W, spec.H, roll_deg=20.0)[5:8]
    with oracle_rasterizer():
        gt = syn.make_model(spec)
        with torch.no_grad():
            gt._features_dc.add_(0.3)
        make_ground_truth(gt, cams, syn.background())
        a, b, c = syn.make_model(spec), syn.make_model(spec), syn.make_model(spec)
        for m in (a, b, c):
            m.training_setup(opt)
        for it in range(2):
            la = training_step(a, [cams[it]], syn.background(), opt, it + 1)
            lb = training_step(b, [cams[it]], syn.background(), opt, it + 1, camera_bank=None)
            assert torch.equal(la, lb)
        assert all(torch.equal(p, q) for p, q in zip(a.leaf_parameters(), b.leaf_parameters()))
        bank = CameraBank(cams, use_barf=True).training_setup(opt)
        assert bank[1].original_image is cams[1].original_image
        init = bank.params.clone()
        for it, i in enumerate((0, 1, 0)):
            training_step(c, [bank[i]], syn.background(), opt, it + 1, camera_bank=bank)
        assert bank.steps.tolist() == [2, 1, 0] and bank.touched.tolist() == [0, 0, 0]
        assert (bank.params[:2] != init[:2]).any(dim=1).all() and torch.equal(bank.params[2], init[2])
        # from iterations_cam on: constants, nothing moves
        before = bank.params.clone()
        training_step(c, [bank[2]], syn.background(), opt, opt.iterations_cam, camera_bank=bank)
        assert torch.equal(bank.params, before) and bank.touched.tolist() == [0, 0, 0]
        assert bank.live and bank[2].FoVx.requires_grad   # constants for the duration of that step only
        with bank.step_scope(opt.iterations_cam):
            assert not bank[2].FoVx.requires_grad
        # a step that raises drops what its views left in the bank's rows (here: the loss of the second view fails)
        broken = copy.copy(bank[1])
        broken.original_image = None
        with pytest.raises(Exception):
            training_step(c, [bank[0], broken], syn.background(), opt, 5, camera_bank=bank)
        assert bank.touched.tolist() == [0, 0, 0] and torch.equal(bank.params, before)
        # distinct cameras also when the bank is only viewed, not stepped
        with pytest.raises(ValueError, match="distinct"):
            training_step(c, [bank[0], bank[0]], syn.background(), opt, 5)
