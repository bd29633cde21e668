"""The camera bank on the device: ghr_camera_compose / ghr_camera_compose_backward / ghr_camera_adam_step through the C ABI
against the reference's golden and torch.optim.Adam (the cases of tests/test_hostsim_camera.py), BankCamera.tensors() through
autograd, and bank cameras inside trainer.training_step and render_hair.  The bar is the one of tests/test_camera_bank.py."""
import copy
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gaussianhaircut_amd.scene.cameras import Camera, CameraBank, compose_camera_torch, ring_cameras
from gaussianhaircut_amd.utils import synthetic as syn
from tests.golden import make_reference_camera_bank_golden as mk
from tests.test_camera_bank import OUT_NAMES, PARAMS, bank_from, check, check_grad_row, cotangent_loss, gold, sub  # noqa: F401
from tests.test_hostsim_camera import COT, adam_scenario, compose_case

pytestmark = pytest.mark.gpu
LEAVES = ("world_view_transform", "full_proj_transform", "camera_center", "FoVx", "FoVy")
LEAF_COT = ("view", "full", "center", "fovx", "fovy")


class GpuApi:
    """the array interface of tests/test_hostsim_camera.py over the C ABI: numpy in, device call, numpy out"""

    def __init__(self):
        from gaussianhaircut_amd import _lib
        self.lib, self.L, self.dev = _lib, _lib.lib(), torch.device("cuda:0")

    def _d(self, a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    @staticmethod
    def _p(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    def _s(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def compose(self, param, first, n, consts, params):
        c, p = self._d(consts), self._d(params)
        out = torch.full((n, 53), float("nan"), device=self.dev)
        self.lib.check(self.L.ghr_camera_compose(self._s(), param, c.shape[0], first, n, self._p(c), c.shape[1], self._p(p), p.shape[1],
                                                 self._p(out), 53))
        return out.cpu().numpy()

    def backward(self, param, first, n, consts, params, cot, grads, touched, mask=3):
        c, p, g, t = self._d(consts), self._d(params), self._d(grads), self._d(touched)
        cots = [self._d(None if cot.get(k) is None else np.asarray(cot[k], dtype=np.float32)) for k in COT]
        self.lib.check(self.L.ghr_camera_compose_backward(self._s(), param, c.shape[0], first, n, self._p(c), c.shape[1], self._p(p), p.shape[1],
                                                          *[self._p(x) for x in cots], self._p(g), g.shape[1], self._p(t), mask))
        return g.cpu().numpy(), t.cpu().numpy()

    def adam(self, param, st, lrs, mask=3):
        d = {k: self._d(v) for k, v in st.items()}
        self.lib.check(self.L.ghr_camera_adam_step(self._s(), param, len(st["steps"]), self._p(d["p"]), self._p(d["g"]),
                                                   self._p(d["m"]), self._p(d["v"]), st["p"].shape[1], self._p(d["steps"]),
                                                   self._p(d["touched"]), lrs[0], lrs[1], lrs[2], 0.9, 0.999, 1e-15, mask))
        for k, v in d.items():
            st[k][...] = v.cpu().numpy()


@pytest.fixture(scope="module")
def api():
    return GpuApi()


# N = 1, 3 and 65 cameras (65: past one wavefront of a lane per camera), ranges from row 0 and row 2, one row and all of them
RANGES = [(1, 0, 1), (3, 0, 1), (3, 0, 3), (3, 2, 1), (65, 0, 65), (65, 2, 1), (65, 2, 63)]


@pytest.mark.parametrize("use_barf", PARAMS)
def test_compose_and_backward_through_the_c_abi_reproduce_the_reference_camera(api, gold, use_barf):
    ref = sub(gold, use_barf)
    worst = [0.0, 0.0]
    for N, first, n in RANGES:
        for which in ("all", "view", "proj"):
            o, g = compose_case(api, ref, use_barf, N, first, n, which)
            worst = [max(worst[0], o), max(worst[1], g)]
    print("camera bank, C ABI on the device, use_barf=%s: worst err / bar outputs %.3g gradients %.3g" % (use_barf, worst[0], worst[1]))


def test_the_c_abi_rejects_bad_camera_arguments(api):
    L, E = api.L, api.lib.GHR_E_INVALID
    t = torch.zeros(4, 64, device=api.dev)
    i = torch.zeros(4, dtype=torch.int32, device=api.dev)
    p, s = api._p, api._s()
    assert L.ghr_camera_compose(s, 2, 4, 0, 1, p(t), 21, p(t), 11, p(t), 53) == E          # unknown parametrisation
    assert L.ghr_camera_compose(s, 0, 4, 0, -1, p(t), 21, p(t), 11, p(t), 53) == E         # n < 0
    assert L.ghr_camera_compose(s, 0, 4, 0, 1, None, 21, p(t), 11, p(t), 53) == E          # null base
    assert L.ghr_camera_compose(s, 0, 4, 0, 1, p(t), 20, p(t), 11, p(t), 53) == E          # strides smaller than the row
    assert L.ghr_camera_compose(s, 0, 4, 0, 1, p(t), 21, p(t), 10, p(t), 53) == E
    assert L.ghr_camera_compose(s, 1, 4, 0, 1, p(t), 21, p(t), 8, p(t), 52) == E
    assert b"stride" in L.ghr_last_error()
    assert L.ghr_camera_compose(s, 0, 4, 3, 2, p(t), 21, p(t), 11, p(t), 53) == E         # the range reaches past the bank's rows
    assert L.ghr_camera_compose_backward(s, 1, 4, 4, 1, p(t), 21, p(t), 8, None, None, None, None, None, None, p(t), 8, p(i), 3) == E
    assert L.ghr_camera_compose_backward(s, 1, 4, 0, 1, p(t), 21, p(t), 8, None, None, None, None, None, None, None, 8, p(i), 3) == E
    assert L.ghr_camera_compose_backward(s, 1, 4, 0, 1, p(t), 21, p(t), 8, None, None, None, None, None, None, p(t), 7, p(i), 3) == E
    assert L.ghr_camera_adam_step(s, 1, 4, p(t), p(t), p(t), None, 8, p(i), p(i), 0.0, 0.0, 0.0, 0.9, 0.999, 1e-15, 3) == E
    assert L.ghr_camera_adam_step(s, 3, 4, p(t), p(t), p(t), p(t), 8, p(i), p(i), 0.0, 0.0, 0.0, 0.9, 0.999, 1e-15, 3) == E
    assert L.ghr_camera_compose(s, 0, 4, 0, 0, p(t), 21, p(t), 11, p(t), 53) == 0          # n = 0: nothing to do


@pytest.mark.parametrize("use_barf", PARAMS)
def test_bank_camera_tensors_through_autograd_reproduce_the_reference_camera(gold, use_barf):
    dev = torch.device("cuda:0")
    ref = sub(gold, use_barf)
    worst_o = worst_g = 0.0
    for names, g64, g32 in ((LEAF_COT, "grad64", "grad32"), (("view",), "gradview64", "gradview32"), (("proj",), "gradproj64", "gradproj32")):
        bank = bank_from(ref, use_barf, device=dev, n_pad=1)
        assert bank.fused
        for i in range(6):
            t = bank[i].tensors()
            assert all(x.requires_grad for x in t)
            for n, x in zip(OUT_NAMES, t):
                worst_o = max(worst_o, check(x.detach().cpu().numpy(), ref[n + "64"][i], ref[n + "32"][i], "%s[%d]" % (n, i)))
            cotangent_loss(t, ref, i, names, dev).backward()
        grads = bank.grads.cpu().numpy()
        for i in range(6):
            worst_g = max(worst_g, check_grad_row(grads[i], ref[g64][i], ref[g32][i], use_barf, "grad[%d]" % i))
        assert bank.touched.tolist() == [1] * 6 + [0] and not grads[6].any() and bank._anchor.grad is None
        # compose_all: the same rows from one launch; the properties read the same evaluation
        allv = bank.compose_all()
        for k in range(6):
            assert torch.equal(allv[k][2], bank[2].tensors()[k].detach())
        with torch.no_grad():
            assert torch.equal(bank[2].full_proj_transform, allv[1][2]) and bank[2].tensors()[0] is bank[2].tensors()[0]
    print("camera bank, BankCamera.tensors() + autograd, use_barf=%s: worst err / bar outputs %.3g gradients %.3g" %
          (use_barf, worst_o, worst_g))


@pytest.mark.parametrize("use_barf", PARAMS)
def test_camera_adam_matches_torch_adam_with_per_camera_step_counts(api, use_barf):
    adam_scenario(api, use_barf)


# ---- inside a step -----------------------------------------------------------------------------------------------------------
def _scene(dev, n_cams=4, use_barf=True):
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    from gaussianhaircut_amd.trainer import make_ground_truth
    spec = syn.CONFIGS["tiny_strands"]
    opt = OptimizationParams()
    opt.lambda_dorient = 0.1
    bg = syn.background(dev)
    gt = syn.make_model(spec, dev)
    with torch.no_grad():
        gt._features_dc.add_(0.3)
    plain = ring_cameras(32, spec.W, spec.H, device=dev, roll_deg=20.0)[5:5 + n_cams]
    make_ground_truth(gt, plain, bg)

    def new_bank():
        bank = CameraBank(plain, use_barf=use_barf, device=dev).training_setup(opt)
        g = torch.Generator().manual_seed(11)
        with torch.no_grad():
            bank.params.add_((1e-2 * torch.randn(bank.params.shape, generator=g)).to(dev))
        return bank
    return spec, opt, bg, plain, new_bank


def _leaf_twin(plain_cam, bank_cam):
    """a plain camera whose five tensors are leaves holding copies of the bank camera's composed values"""
    c = copy.copy(plain_cam)
    with torch.no_grad():
        t = bank_cam.tensors()
    for n, x in zip(LEAVES, t[:5]):
        setattr(c, n, x.detach().clone().requires_grad_(True))
    c.projection_matrix = t[5].detach().clone()
    return c


def _check_row_against_leaf_grads(bank, i, leaf_cam, what):
    """the bank's gradient row vs the leaf gradients pushed through the double restatement's VJP (fp32 side of the bar: the same
    through the bank's PyTorch form on the CPU)"""
    cot = {k: (getattr(leaf_cam, n).grad.detach().cpu().numpy() if getattr(leaf_cam, n).grad is not None else None)
           for k, n in zip(LEAF_COT, LEAVES)}
    assert cot["view"] is not None and np.abs(cot["view"]).max() > 0
    crow, prow = bank.consts[i].cpu(), bank.params[i].detach().cpu()
    _, g64 = mk.vjp64(bank.use_barf, crow.numpy(), prow.numpy(), cot)
    p32 = prow.clone().requires_grad_(True)
    rd = bank.rot_dim
    t32 = compose_camera_torch(bank.use_barf, crow, p32[:rd], p32[rd:rd + 3], p32[rd + 3:])
    sum((t32[OUT_NAMES.index(k)] * torch.from_numpy(np.asarray(v))).sum() for k, v in cot.items() if v is not None).backward()
    ratio = check_grad_row(bank.grads[i].cpu().numpy(), g64, p32.grad.numpy(), bank.use_barf, what)
    print("%s: worst err / bar %.3g" % (what, ratio))
    return ratio


@pytest.mark.parametrize("fuse_adam", [True, False])
def test_bank_camera_in_a_training_step_equals_the_leaf_camera_step(fuse_adam):
    from gaussianhaircut_amd import _lib
    from gaussianhaircut_amd.gaussian_renderer import _use_fused, render
    from gaussianhaircut_amd.trainer import PIPE, training_step
    dev = torch.device("cuda:0")
    spec, opt, bg, plain, new_bank = _scene(dev)
    bank, i = new_bank(), 1
    prev = _lib.lib().ghr_set_deterministic(1)
    try:
        model = syn.make_model(spec, dev)
        model.training_setup(opt)
        assert _use_fused(model, PIPE, bank[i])
        # (_fused_was_taken's criterion, on a model of its own: no backward, the bank's row stays untouched)
        assert getattr(render(bank[i], syn.make_model(spec, dev), PIPE, bg), "count", None) is not None
        training_step(model, [bank[i]], bg, opt, 1, fuse_adam=fuse_adam)
        assert model.optimizer.fused_steps == (1 if fuse_adam else 0)
        assert bank.touched.tolist() == [0, 1, 0, 0] and not bank.grads[[0, 2, 3]].any()
        twin_model, twin = syn.make_model(spec, dev), _leaf_twin(plain[i], bank[i])
        twin_model.training_setup(opt)
        training_step(twin_model, [twin], bg, opt, 1, fuse_adam=fuse_adam)
        torch.cuda.synchronize()
        assert torch.equal(model.optimizer.flat_param, twin_model.optimizer.flat_param)
        assert torch.equal(model.optimizer.exp_avg, twin_model.optimizer.exp_avg)
        _check_row_against_leaf_grads(bank, i, twin, "bank row inside training_step (fuse_adam=%s)" % fuse_adam)
    finally:
        _lib.lib().ghr_set_deterministic(prev)


def test_training_step_steps_the_viewed_cameras_of_its_bank():
    from gaussianhaircut_amd import _lib
    from gaussianhaircut_amd.trainer import training_step
    dev = torch.device("cuda:0")
    spec, opt, bg, plain, new_bank = _scene(dev)
    prev = _lib.lib().ghr_set_deterministic(1)
    try:
        bank = new_bank()
        init = bank.params.clone()
        model = syn.make_model(spec, dev)
        model.training_setup(opt)
        for it, i in enumerate((0, 1, 0)):
            training_step(model, [bank[i]], bg, opt, it + 1, camera_bank=bank)
        assert bank.steps.tolist() == [2, 1, 0, 0] and bank.touched.tolist() == [0] * 4 and not bank.grads.any()
        assert (bank.params[:2] != init[:2]).any(dim=1).all() and torch.equal(bank.params[2:], init[2:])
        assert torch.isfinite(bank.params).all()
        # two views on two streams (cameras 2 and 3) leave both rows as one stream does, bit for bit
        rows = {}
        for streams in (2, 0):
            b2, m2 = new_bank(), syn.make_model(spec, dev)
            m2.training_setup(opt)
            training_step(m2, [b2[2], b2[3]], bg, opt, 1, camera_bank=b2, streams=streams)
            torch.cuda.synchronize()
            assert b2.steps.tolist() == [0, 0, 1, 1]
            rows[streams] = (b2.params.clone(), b2.exp_avg.clone(), b2.exp_avg_sq.clone())
        for a, b in zip(rows[2], rows[0]):
            assert torch.equal(a, b)
        assert (rows[2][0][2:] != init[2:]).any(dim=1).all()
        # from iterations_cam on nothing moves and the view takes the constant-camera path
        before = bank.params.clone()
        training_step(model, [bank[2]], bg, opt, opt.iterations_cam, camera_bank=bank)
        assert torch.equal(bank.params, before) and bank.steps.tolist() == [2, 1, 0, 0] and bank.touched.tolist() == [0] * 4
        assert bank.live and all(x.requires_grad for x in bank[2].tensors())   # (constants for that step only)
        with bank.step_scope(opt.iterations_cam):
            assert not bank.live and not any(x.requires_grad for x in bank[2].tensors())
        with pytest.raises(ValueError):   # also without camera_bank=: the rows would race on two streams
            training_step(model, [bank[0], bank[0]], bg, opt, 5)
        with pytest.raises(ValueError):
            training_step(model, [bank[0], bank[0]], bg, opt, 5, camera_bank=bank)
    finally:
        _lib.lib().ghr_set_deterministic(prev)


def test_render_hair_with_a_bank_camera():
    from gaussianhaircut_amd import _lib
    from gaussianhaircut_amd.gaussian_renderer import _use_fused_hair, render_hair
    from tests.golden.make_reference_render_golden import functional, weights
    from tests.test_api_cpu import _hair_scene
    dev = torch.device("cuda:0")
    spec, head, hair, cam = _hair_scene(dev, "ring13roll")
    bank = CameraBank([cam], use_barf=True, device=dev)
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        bank.params.add_((1e-2 * torch.randn(bank.params.shape, generator=g)).to(dev))
    pipe = SimpleNamespace(debug=False)
    w = weights(spec, 3).to(dev)
    prev = _lib.lib().ghr_set_deterministic(1)
    try:
        hair.initialize_gaussians_hair()
        assert _use_fused_hair(head, hair, pipe, bank[0])
        functional(render_hair(bank[0], head, hair, pipe, syn.background(dev)), w).backward()
        twin = _leaf_twin(cam, bank[0])
        hair.initialize_gaussians_hair()
        functional(render_hair(twin, head, hair, pipe, syn.background(dev)), w).backward()
        assert bank.touched.tolist() == [1]
        _check_row_against_leaf_grads(bank, 0, twin, "bank row behind render_hair")
    finally:
        _lib.lib().ghr_set_deterministic(prev)
