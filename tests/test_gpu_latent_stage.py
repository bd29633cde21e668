"""The latent-strand stage on the device: the kernels of csrc/ghr_latent.h through the C ABI into NaN-filled buffers between NaN
guards, under the checks of tests/test_latent_stage.py (same cases, same bars), and the stage end to end.

Launch shapes.  Build: 256 segment rows (forward) / 256 points (backward) per workgroup -- (1, 257) and (5, 100) put a workgroup
boundary inside a strand on the point and on the segment grid, (257, 2) has more strands than a workgroup has rows (its LDS
stage holds the most points a workgroup can need: two per row), (1, 4099) is longer than GHR_STRAND_MAX_SEG.  Expand / reduce:
one thread per element or float4, no cap.  Loss: 1024 pixels per workgroup, no cap on the grid -- (1, 1020), (1, 1024), (1, 1028)
straddle one workgroup, (5, 205) = 1025 pixels is the scalar form with a second workgroup of one pixel, (36, 68) has three."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd.utils import synthetic as syn
from tests import loss_cases as lc
from tests import test_latent_stage as tl
from tests.golden import make_reference_latent_golden as mk

pytestmark = pytest.mark.gpu
GUARD = 64  # floats on either side of every output (256 B: the payload keeps the allocation's 16-B alignment)
LOSS_SHAPES = ((1, 1), (1, 3), (1, 4), (1, 5), (5, 205), (1, 1020), (1, 1024), (1, 1028), (36, 68))
FUSED = SimpleNamespace(debug=False, fused_projection=True)


@pytest.fixture(scope="module")
def gold():
    return np.load(tl.GOLD_PATH)


class Out:
    """a NaN-filled device buffer between two NaN guards"""

    def __init__(self, shape, dev):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + 4 * GUARD)

    def get(self, written=None):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        assert np.isnan(b[:GUARD]).all() and np.isnan(b[GUARD + self.n:]).all(), "a guard was written"
        body = b[GUARD:GUARD + self.n]
        if written is not None:
            assert np.isnan(body[written:]).all(), "written past the expected slots"
        return body.reshape(self.shape).copy()


class DevApi:
    """tests/test_latent_stage.SimApi's interface over libghr_hip.so on the GPU"""

    def __init__(self):
        self.L = _lib.lib()
        self.dev = torch.device("cuda:0")

    def _in(self, a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.dev)

    @staticmethod
    def _ptr(t, off=0):
        return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * off)

    def build(self, p, scale):
        S, L = p.shape[:2]
        P = S * (L - 1)
        pt = self._in(p)
        o = [Out((P, n), self.dev) for n in (3, 4, 3, 3)]
        _lib.check(self.L.ghr_strand_points_build(None, S, L, self._ptr(pt), scale, *[x.ptr for x in o]))
        return dict(zip(mk.COTS, [x.get() for x in o]))

    def build_backward(self, p, cots):
        S, L = p.shape[:2]
        pt = self._in(p)
        c = [self._in(cots.get(k)) for k in mk.COTS]
        d_p = Out(p.shape, self.dev)
        _lib.check(self.L.ghr_strand_points_build_backward(None, S, L, self._ptr(pt), *[self._ptr(x) for x in c], d_p.ptr))
        return d_p.get()

    def expand(self, src, n_seg):
        S, C = src.shape
        s, dst = self._in(src), Out((S * n_seg, C), self.dev)
        _lib.check(self.L.ghr_strand_rows_expand(None, S, n_seg, C, self._ptr(s), dst.ptr))
        return dst.get()

    def reduce(self, g, S, n_seg):
        C = g.shape[1]
        gt, out = self._in(g), Out((S, C), self.dev)
        _lib.check(self.L.ghr_strand_rows_reduce(None, S, n_seg, C, self._ptr(gt), out.ptr))
        return out.get()

    def loss(self, c, w, conf=True, weight=True, grad_loss=None):
        r = self._in(c["renders"])
        _, H, W = r.shape
        n = H * W
        gi, gm, ga, gc = self._in(c["gt_image"]), self._in(c["gt_mask"][0]), self._in(c["gt_angle"]), self._in(c["gt_oconf"])
        ptrs = dict(image=r.data_ptr(), mask0=r.data_ptr() + 12 * n, dir2d=r.data_ptr() + 20 * n,
                    orient_conf=r.data_ptr() + 32 * n if conf else None, gt_image=gi.data_ptr(), gt_mask0=gm.data_ptr(),
                    gt_orient_angle=ga.data_ptr(), gt_orient_conf=gc.data_ptr() if weight else None)
        a = tl.loss_struct(W, H, ptrs, w)
        floats = _lib.latent_loss_sums_floats(W, H)
        assert floats == 8 + 4 * ((n + 1023) // 1024)
        sums, loss, d = Out((floats + 16,), self.dev), Out((1,), self.dev), Out((10, H, W), self.dev)
        _lib.check(self.L.ghr_latent_loss_forward(None, ctypes.byref(a), sums.ptr, loss.ptr))
        s = sums.get(written=floats)[:floats]
        assert not np.isnan(s).all()
        gl = None if grad_loss is None else torch.tensor([grad_loss], dtype=torch.float32, device=self.dev)
        _lib.check(self.L.ghr_latent_loss_backward(None, ctypes.byref(a), sums.ptr, self._ptr(gl), d.ptr))
        return s, float(loss.get()[0]), d.get()


@pytest.fixture(scope="module")
def api():
    return DevApi()


@pytest.mark.parametrize("S,L", mk.BUILD_SHAPES)
def test_gpu_points_build_matches_the_reference(api, gold, S, L):
    tl.check_build(api, gold, S, L)


@pytest.mark.parametrize("C", [1, 3, 45, 48, 49])
@pytest.mark.parametrize("S,n_seg", [(1, 1), (3, 99), (300, 7), (2, 1025)])
def test_gpu_rows_expand_is_exact_and_reduce_is_a_sequential_sum(api, S, n_seg, C):
    tl.check_rows(api, S, n_seg, C)


@pytest.mark.parametrize("H,W", mk.LOSS_SHAPES)
def test_gpu_latent_loss_matches_the_reference(api, gold, H, W):
    tl.check_loss_golden(api, gold, H, W)


def test_gpu_latent_loss_drops_exactly_the_nan_terms(api, gold):
    tl.check_loss_nan_rules(api, tl.golden_case(gold, 12, 20)[0])


@pytest.mark.parametrize("H,W", LOSS_SHAPES)
def test_gpu_latent_loss_at_boundary_shapes(api, monkeypatch, H, W):
    """every term and the blend against the composed form in float64; where the float4 form applies (H W % 4 == 0) the scalar
    form forced on the same buffers gives the same bits"""
    c = {k: v.numpy() if isinstance(v, torch.Tensor) else v for k, v in lc.make_case(H, W).items()}
    for w, conf, weight in [(tl.BLEND, True, True)] + list(tl.VARIANTS.values()):
        f64, g64 = tl.comparator_loss(c, w, torch.float64, conf, weight)
        f32, _ = tl.comparator_loss(c, w, torch.float32, conf, weight)
        sums, loss, d = api.loss(c, w, conf, weight)
        if np.isnan(f64):       # a mask without a set pixel and zero weights cannot happen with make_case's gt_oconf >= 0.05
            raise AssertionError("the case has a NaN term")
        tl.check_loss_value(loss, f64, f32, (w, conf, weight))
        lc.check_grad(d, g64, c["special"], str((w, conf, weight)))
        if w is tl.BLEND:
            monkeypatch.setenv("GHR_LATENT_SCALAR", "1")
            sums_s, loss_s, d_s = api.loss(c, w, conf, weight)
            monkeypatch.delenv("GHR_LATENT_SCALAR")
            assert sums_s.tobytes() == sums.tobytes() and loss_s == loss and d_s.tobytes() == d.tobytes()


# --------------------------------------------------------------------------------------------------------------- end to end
def _graph_has(t, name):
    """a node whose class name starts with `name` in the autograd graph of t"""
    seen, todo = set(), [t.grad_fn]
    while todo:
        n = todo.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        if type(n).__name__.startswith(name):
            return True
        todo += [f for f, _ in n.next_functions]
    return False


class ToyGenerator(torch.nn.Module):
    """a parameter tensor of points plus one linear layer for the per-strand appearance"""

    def __init__(self, points, K, l_diff=None):
        super().__init__()
        g = torch.Generator().manual_seed(4)
        self.points = torch.nn.Parameter(points.clone())
        self.code = torch.nn.Parameter(torch.randn(points.shape[0], 8, generator=g).to(points.device))
        self.lin = torch.nn.Linear(8, 3 * K + 1).to(points.device)
        with torch.no_grad():
            self.lin.weight.copy_((torch.randn(3 * K + 1, 8, generator=g) * 0.1).to(points.device))
            self.lin.bias.zero_()
        self.l_diff = l_diff

    def forward(self, iteration):
        z = self.lin(self.code)
        out = {"points": self.points * 1.0, "features": z[:, :-1], "orient_conf": z[:, -1:]}
        if self.l_diff == "nan":
            out["L_diff"] = self.points.sum() * float("nan")
        elif self.l_diff == "real":
            out["L_diff"] = (self.points ** 2).mean()
        return out


def _scene(dev, fused=True, l_diff=None):
    from gaussianhaircut_amd.gaussian_renderer import render_hair
    from gaussianhaircut_amd.scene.gaussian_model_latent_strands import GaussianModelLatentStrands
    from tests.test_api_cpu import _hair_scene
    spec, head, strands, cam = _hair_scene(dev)
    pts = strands._pts.detach()                                   # [40, 11, 3] polylines of the explicit-strand scene
    hair = GaussianModelLatentStrands(3, ToyGenerator(pts, 16, l_diff), None, fused=fused)
    bg = syn.background(dev)
    with torch.no_grad():                                         # ground truth: the same strands, displaced and recoloured
        gt = GaussianModelLatentStrands(3, ToyGenerator(pts * 1.03, 16), None)
        gt.strands_generator.lin.bias.add_(0.3)
        gt.initialize_gaussians_hair(0)
        pkg = render_hair(cam, head, gt, FUSED, bg)
        cam.original_image = pkg["render"].clamp(0, 1).detach()
        cam.original_mask = pkg["mask"].clamp(0, 1).detach()
        cam.original_orient_angle = pkg["orient_angle"].detach()
        cam.original_orient_conf = torch.ones_like(pkg["orient_conf"]).detach()
    return head, hair, cam, bg


def _opt():
    return SimpleNamespace(lambda_dl1=1.0, lambda_dmask=0.1, lambda_dorient=0.1, lambda_dsds=0.5, use_gt_orient_conf=True,
                           train_orient_conf=True, iterations=100, latent_lr=1e-3)


def test_gpu_latent_stage_end_to_end_matches_the_composed_form():
    from gaussianhaircut_amd.gaussian_renderer import render_hair
    from gaussianhaircut_amd.trainer import latent_view_loss
    from tests import helpers as hp
    dev = torch.device("cuda:0")
    L = _lib.lib()
    L.ghr_set_deterministic(1)
    try:
        res = {}
        for fused in (True, False):
            head, hair, cam, bg = _scene(dev, fused, "real")
            hair.initialize_gaussians_hair(1)
            pkg = render_hair(cam, head, hair, FUSED, bg)
            assert getattr(pkg, "renders_packed", None) is not None                       # the fused renderer took it
            assert type(pkg.renders_packed.grad_fn).__name__.startswith("_RenderHairFused")
            if fused:
                assert type(hair._xyz.grad_fn).__name__.startswith("_PointsBuild")
                assert _graph_has(hair._features_dc, "_RowsExpand") and _graph_has(hair._orient_conf, "_RowsExpand")
            loss = latent_view_loss(pkg, cam, _opt(), l_diff=hair.LDiff, fused=fused)
            assert _graph_has(loss, "_LatentLossPacked") == fused and _graph_has(hair._xyz, "_PointsBuild") == fused
            loss.backward()
            res[fused] = (float(loss.detach()), {n: q.grad.detach().cpu().numpy() for n, q in hair.strands_generator.named_parameters()})
    finally:
        L.ghr_set_deterministic(0)
    (lf, gf), (lt, gt) = res[True], res[False]
    assert hp.image_close(np.float64(lf), np.float64(lt)).all()
    hp.assert_grads_close(gf, gt)


def test_gpu_latent_training_steps_move_the_parameters_and_follow_the_nan_rules():
    dev = torch.device("cuda:0")
    L = _lib.lib()
    L.ghr_set_deterministic(1)   # the renderer's backward adds in a fixed order: two runs of the same step give the same bits
    try:
        _training_steps_and_nan_rules(dev)
    finally:
        L.ghr_set_deterministic(0)


def _training_steps_and_nan_rules(dev):
    from gaussianhaircut_amd.trainer import latent_strand_training_step
    opt = _opt()
    finals = {}
    for l_diff in (None, "nan"):
        head, hair, cam, bg = _scene(dev, True, l_diff)
        hair.training_setup(opt)
        p0 = {n: q.detach().clone() for n, q in hair.strands_generator.named_parameters()}
        losses = [latent_strand_training_step(head, hair, [cam], bg, opt, i + 1, pipe=FUSED) for i in range(3)]
        assert all(not t.requires_grad and t.is_cuda for t in losses) and np.isfinite([float(t) for t in losses]).all()
        finals[l_diff] = {n: q.detach().clone() for n, q in hair.strands_generator.named_parameters()}
        for n, q in finals[l_diff].items():
            assert torch.isfinite(q).all() and (q - p0[n]).abs().max() > 0, n
    for n in finals[None]:                 # a NaN L_diff is dropped: the same parameters as without the term
        assert torch.equal(finals[None][n], finals["nan"][n]), n
    # a NaN planted in one parameter's gradient takes the reference's branch: zero_grad() before the step
    head, hair, cam, bg = _scene(dev, True, None)
    hair.training_setup(opt)
    first = hair.optimizer.param_groups[0]["params"][0]
    calls = []
    real_zero, real_step = hair.optimizer.zero_grad, hair.optimizer.step
    hair.optimizer.zero_grad = lambda *a, **k: (calls.append(("zero_grad", k)), real_zero(*a, **k))[1]
    hair.optimizer.step = lambda *a, **k: (calls.append(("step", k)), real_step(*a, **k))[1]
    h = first.register_hook(lambda g: torch.where(torch.arange(g.numel(), device=g.device).reshape(g.shape) == 0,
                                                  torch.full_like(g, float("nan")), g))
    before = {n: q.detach().clone() for n, q in hair.strands_generator.named_parameters()}
    latent_strand_training_step(head, hair, [cam], bg, opt, 1, pipe=FUSED)
    h.remove()
    assert [c[0] for c in calls] == ["zero_grad", "step", "zero_grad"] and calls[0][1] == {} and calls[2][1] == {"set_to_none": True}
    import inspect
    if inspect.signature(torch.optim.Optimizer.zero_grad).parameters["set_to_none"].default:
        for n, q in hair.strands_generator.named_parameters():   # this torch's zero_grad() drops the gradients: nothing moves
            assert torch.equal(q.detach(), before[n]), n
    calls.clear()
    latent_strand_training_step(head, hair, [cam], bg, opt, opt.iterations, pipe=FUSED)   # the last iteration takes no step (:156)
    assert calls == []
