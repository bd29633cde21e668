"""The latent-strand stage (csrc/ghr_latent.h; src/train_latent_strands.py:103-164, src/scene/gaussian_model_latent_strands.py:451-499)
on the CPU: the product's `__host__ __device__` row and pixel functions through tests/hostsim/ghr_hostsim_latent.cpp, and the
``fused=False`` comparator, against tests/golden/reference_latent_golden.npz (the reference's own functions, float32 and float64).

The cases are written against a small array interface (``SimApi`` here) so that tests/test_gpu_latent_stage.py runs the same
checks through the C ABI on the device.

Bars.  xyz / dir: bit-equal to float32 torch.  rotation / scaling / d_p: the bars of tests/test_strand_build.py for the same row
functions (atol 3e-7, rtol 3e-7, 2e-5 of max|ref| -- here per group: the end points of zero-length segments, whose gradient is
~1e12, apart from the ordinary ones).  Reduce: (n_seg - 1) 2^-24 sum_k |g_k| per element, the bound of a sequential fp32 sum.
Loss values: 1e-5 max(1, |f64|) + 3 |ref32 - f64|; loss gradients: tests/loss_cases.check_grad."""
import ctypes
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from tests import helpers as hp
from tests import loss_cases as lc
from tests.golden import make_reference_latent_golden as mk

GOLD_PATH = os.path.join(hp.ROOT, "tests", "golden", "reference_latent_golden.npz")
SCALE = mk.SCALE
TERM_W = dict(l1=(1.0, 0.0, 0.0), ce=(0.0, 1.0, 0.0), orient=(0.0, 0.0, 1.0))
BLEND = (0.8, 0.2, 0.1)
# golden term -> (weights, confidence given, weight given)
VARIANTS = {"l1": (TERM_W["l1"], True, True), "ce": (TERM_W["ce"], True, True), "or": (TERM_W["orient"], True, True),
            "or_noconf": (TERM_W["orient"], False, True), "or_noweight": (TERM_W["orient"], True, False)}


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD_PATH)


def _build():
    """as tests/test_hostsim_camera.py builds its library"""
    src = os.path.join(hp.ROOT, "tests", "hostsim", "ghr_hostsim_latent.cpp")
    out_dir = os.path.join(hp.ROOT, "tests", "hostsim", "_build")
    so = os.path.join(out_dir, "libghr_hostsim_latent.so")
    csrc = os.path.join(hp.ROOT, "gaussianhaircut_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(out_dir, exist_ok=True)
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-x", "hip", "-O2", "-std=c++17", "-ffp-contract=off",
                        "-fPIC", "-shared", "-o", so, src], check=True)
    return so


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def loss_struct(W, H, ptrs, w):
    """ghr_latent_loss_args from a dict of addresses (None: NULL)"""
    a = _lib.LatentLossArgs()
    a.W, a.H = W, H
    for k in ("image", "mask0", "dir2d", "orient_conf", "gt_image", "gt_mask0", "gt_orient_angle", "gt_orient_conf"):
        setattr(a, k, ptrs.get(k))
    a.w_l1, a.w_mask, a.w_orient = [float(x) for x in w]
    return a


class SimApi:
    """numpy in, numpy out; the calls of include/ghr.h's latent-strand stage on the CPU"""

    def __init__(self):
        import torch  # noqa: F401  (one HIP runtime for every HIP-linked library of the process)
        self.L = ctypes.CDLL(_build())
        self.L.ghrsim_latent_loss_sums_floats.restype = ctypes.c_size_t

    def build(self, p, scale):
        S, L = p.shape[:2]
        P = S * (L - 1)
        o = [np.full((P, n), np.nan, np.float32) for n in (3, 4, 3, 3)]
        self.L.ghrsim_points_build(S, L, _p(p), ctypes.c_float(scale), *[_p(x) for x in o])
        return dict(xyz=o[0], rot=o[1], scaling=o[2], dir=o[3])

    def build_backward(self, p, cots):
        S, L = p.shape[:2]
        d_p = np.full(p.shape, np.nan, np.float32)
        c = [None if cots.get(k) is None else _f32(cots[k]) for k in mk.COTS]
        self.L.ghrsim_points_build_backward(S, L, _p(p), *[_p(x) for x in c], _p(d_p))
        return d_p

    def expand(self, src, n_seg):
        S, C = src.shape
        dst = np.full((S * n_seg, C), np.nan, np.float32)
        self.L.ghrsim_rows_expand(S, n_seg, C, _p(src), _p(dst))
        return dst

    def reduce(self, g, S, n_seg):
        C = g.shape[1]
        out = np.full((S, C), np.nan, np.float32)
        self.L.ghrsim_rows_reduce(S, n_seg, C, _p(g), _p(out))
        return out

    def loss(self, c, w, conf=True, weight=True, grad_loss=None):
        """c: dict of float32 arrays renders [10,H,W], gt_image, gt_mask, gt_angle, gt_oconf -> (sums, loss, d_packed)"""
        r = _f32(c["renders"])
        _, H, W = r.shape
        keep = dict(gi=_f32(c["gt_image"]), gm=_f32(c["gt_mask"][0]), ga=_f32(c["gt_angle"]), gc=_f32(c["gt_oconf"]))
        n = 4 * H * W
        ptrs = dict(image=r.ctypes.data, mask0=r.ctypes.data + 3 * n, dir2d=r.ctypes.data + 5 * n,
                    orient_conf=r.ctypes.data + 8 * n if conf else None, gt_image=keep["gi"].ctypes.data,
                    gt_mask0=keep["gm"].ctypes.data, gt_orient_angle=keep["ga"].ctypes.data,
                    gt_orient_conf=keep["gc"].ctypes.data if weight else None)
        a = loss_struct(W, H, ptrs, w)
        sums = np.full(int(self.L.ghrsim_latent_loss_sums_floats(W, H)), np.nan, np.float32)
        loss = np.full(1, np.nan, np.float32)
        self.L.ghrsim_latent_loss_forward(ctypes.byref(a), _p(sums), _p(loss))
        d = np.full((10, H, W), np.nan, np.float32)
        gl = None if grad_loss is None else np.array([grad_loss], np.float32)
        self.L.ghrsim_latent_loss_backward(ctypes.byref(a), _p(sums), _p(gl), _p(d))
        return sums, float(loss[0]), d


@pytest.fixture(scope="module")
def sim():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    return SimApi()


# ------------------------------------------------------------------------------------------------------------ comparator
def comparator_build(p, cots, dtype, use=mk.COTS, fused=False):
    """the product's ``fused=False`` form (scene/gaussian_model_latent_strands.build_from_points): outputs and d p"""
    from gaussianhaircut_amd.scene.gaussian_model_latent_strands import build_from_points
    pt = torch.from_numpy(np.asarray(p)).to(dtype).requires_grad_(True)
    outs = dict(zip(mk.COTS, build_from_points(pt, SCALE, fused)))
    total = sum((outs[k] * torch.from_numpy(np.asarray(cots[k])).to(dtype)).sum() for k in use)
    (g,) = torch.autograd.grad(total, pt)
    return {k: v.detach().numpy() for k, v in outs.items()}, g.numpy()


def comparator_loss(c, w, dtype, conf=True, weight=True):
    """trainer.latent_view_loss's composed PyTorch form on a packed render: loss and its gradient (float64 numpy)"""
    from gaussianhaircut_amd.gaussian_renderer import orient_angle_from
    from gaussianhaircut_amd.trainer import latent_view_loss
    r = torch.from_numpy(np.asarray(c["renders"])).to(dtype).requires_grad_(True)
    t = {k: torch.from_numpy(np.asarray(c[k])).to(dtype) for k in ("gt_image", "gt_mask", "gt_angle", "gt_oconf")}
    pkg = {"render": r[0:3], "mask": r[3:5], "orient_angle": orient_angle_from(r[5:8]), "orient_conf": r[8:9]}
    cam = SimpleNamespace(original_image=t["gt_image"], original_mask=t["gt_mask"], original_orient_angle=t["gt_angle"],
                          original_orient_conf=t["gt_oconf"])
    opt = SimpleNamespace(lambda_dl1=w[0], lambda_dmask=w[1], lambda_dorient=w[2], lambda_dsds=0.0, use_gt_orient_conf=weight,
                          train_orient_conf=conf)
    loss = latent_view_loss(pkg, cam, opt, fused=False)
    (g,) = torch.autograd.grad(loss, r)
    return float(loss.detach().double()), g.detach().double().numpy()


# ------------------------------------------------------------------------------------------------------------ the checks
def degenerate_points(dir32, S, L):
    """[S, L] bool: end points of a zero-length segment"""
    z = (np.asarray(dir32).reshape(S, L - 1, 3) == 0).all(axis=-1)
    m = np.zeros((S, L), bool)
    m[:, :-1] |= z
    m[:, 1:] |= z
    return m


def check_d_p(got, ref, degenerate, what=""):
    assert np.isfinite(got).all(), what
    for name, sel in (("ordinary", ~degenerate), ("degenerate", degenerate)):
        if not sel.any():
            continue
        scale = np.abs(ref[sel]).max()
        err = np.abs(got[sel].astype(np.float64) - ref[sel]).max()
        assert err <= 2e-5 * scale, (what, name, err, scale)


def check_build(api, gold, S, L):
    key = "b%dx%d/" % (S, L)
    p, cots = gold[key + "p"], {k: v.numpy() for k, v in mk.make_cots(S, L).items()}
    o = api.build(p, SCALE)
    P = S * (L - 1)
    assert o["xyz"].tobytes() == gold[key + "xyz32"].tobytes() and o["dir"].tobytes() == gold[key + "dir32"].tobytes()
    assert np.allclose(o["rot"], gold[key + "rot32"], rtol=0, atol=3e-7) and np.array_equal(o["rot"][:, 1], np.zeros(P, np.float32))
    assert np.allclose(o["scaling"], gold[key + "scaling32"], rtol=3e-7, atol=0)
    deg = degenerate_points(gold[key + "dir32"], S, L)
    if S >= 3 and L >= 3:
        assert deg[0, 0] and deg[0, 1]          # the coincident points are in the case
    d_all = api.build_backward(p, cots)
    check_d_p(d_all, gold[key + "d_p64"], deg, "all")
    assert api.build_backward(p, cots).tobytes() == d_all.tobytes()      # the same bits run after run
    for k in mk.COTS:                                                    # each cotangent absent; alone where the golden has it
        ref = comparator_build(p, cots, torch.float64, [j for j in mk.COTS if j != k])[1]
        check_d_p(api.build_backward(p, {j: (None if j == k else cots[j]) for j in mk.COTS}), ref, deg, "without " + k)
        if key + "d_p64_" + k in gold.files:
            check_d_p(api.build_backward(p, {k: cots[k]}), gold[key + "d_p64_" + k], deg, "only " + k)
    none = api.build_backward(p, {})
    assert not none.any()


def check_rows(api, S, n_seg, C):
    g = np.random.default_rng(S + 10 * n_seg + 1000 * C)
    src = g.standard_normal((S, C)).astype(np.float32)
    dst = api.expand(src, n_seg)
    assert dst.tobytes() == np.repeat(src, n_seg, axis=0).tobytes()
    rows = (g.standard_normal((S * n_seg, C)) * np.exp(g.standard_normal((S * n_seg, C)))).astype(np.float32)
    got = api.reduce(rows, S, n_seg)
    r3 = rows.reshape(S, n_seg, C).astype(np.float64)
    bound = (n_seg - 1) * 2.0 ** -24 * np.abs(r3).sum(axis=1)
    assert np.isfinite(got).all() and (np.abs(got - r3.sum(axis=1)) <= bound).all()
    if n_seg == 1:
        assert got.tobytes() == rows.tobytes()


def check_loss_value(got, f64, ref32, what=""):
    bar = 1e-5 * max(1.0, abs(f64)) + 3.0 * abs(ref32 - f64)
    assert np.isfinite(got) and abs(got - f64) <= bar, (what, got, f64, ref32, bar)


def golden_case(gold, H, W):
    key = "l%dx%d/" % (H, W)
    return {k: gold[key + k] for k in ("renders", "gt_image", "gt_mask", "gt_angle", "gt_oconf", "special")}, key


def check_loss_golden(api, gold, H, W):
    c, key = golden_case(gold, H, W)
    v32, v64 = dict(zip(mk.TERMS, gold[key + "val32"])), dict(zip(mk.TERMS, gold[key + "val64"]))
    for term, (w, conf, weight) in VARIANTS.items():          # each term alone
        sums, loss, d = api.loss(c, w, conf, weight)
        check_loss_value(loss, v64[term], v32[term], term)
        lc.check_grad(d, gold[key + "grad64_" + term], c["special"], term)
        assert not sums[3:6].any() and sums[7] == 0
    sums, loss, d = api.loss(c, BLEND)
    f64 = sum(wi * v64[t] for wi, t in zip(BLEND, ("l1", "ce", "or")))
    f32 = sum(wi * v32[t] for wi, t in zip(BLEND, ("l1", "ce", "or")))
    check_loss_value(loss, f64, f32, "blend")
    for i, t in enumerate(("l1", "ce", "or")):
        check_loss_value(float(sums[i]), v64[t], v32[t], "aux " + t)
    lc.check_grad(d, sum(wi * gold[key + "grad64_" + t] for wi, t in zip(BLEND, ("l1", "ce", "or"))), c["special"], "blend")
    d2 = api.loss(c, BLEND, grad_loss=-2.5)[2]                 # the upstream gradient scales every plane
    lc.check_grad(d2, -2.5 * sum(wi * gold[key + "grad64_" + t] for wi, t in zip(BLEND, ("l1", "ce", "or"))), c["special"], "up")


PLANES = dict(l1=(0, 1, 2), ce=(3,), orient=(5, 6, 8))
NAN_AT = dict(l1=0, ce=3, orient=5)        # a render plane only that term reads


def check_loss_nan_rules(api, c):
    """each term NaN alone: value 0, flag 1, an all-zero gradient for that term, the others unchanged bit for bit"""
    sums0, loss0, d0 = api.loss(c, BLEND)
    assert np.isfinite(d0).all() and not sums0[3:6].any()
    for i, term in enumerate(("l1", "ce", "orient")):
        bad = dict(c)
        bad["renders"] = np.array(c["renders"], np.float32, copy=True)
        bad["renders"][NAN_AT[term]].flat[-1] = np.nan
        sums, loss, d = api.loss(bad, BLEND)
        assert sums[i] == 0 and sums[3 + i] == 1 and np.isfinite(loss)
        for j, other in enumerate(("l1", "ce", "orient")):
            same = d[list(PLANES[other])].tobytes() == d0[list(PLANES[other])].tobytes()
            if other == term:
                assert not d[list(PLANES[other])].any()
            else:
                assert same and sums[j].tobytes() == sums0[j].tobytes() and sums[3 + j] == 0
        assert not d[[4, 7, 9]].any()
        rest = [sums0[j] * BLEND[j] for j in range(3) if j != i]
        assert abs(loss - float(np.float32(rest[0]) + np.float32(rest[1]))) <= 1e-6 * max(1.0, abs(loss0))
    zero_w = dict(c)
    zero_w["gt_oconf"] = np.zeros_like(c["gt_oconf"])          # 0 / 0: the orientation term is NaN without a NaN input
    sums, loss, d = api.loss(zero_w, BLEND)
    assert sums[2] == 0 and sums[5] == 1 and not d[[5, 6, 8]].any() and d[:4].tobytes() == d0[:4].tobytes()
    inf = dict(c)
    inf["renders"] = np.array(c["renders"], np.float32, copy=True)
    inf["renders"][0].flat[0] = np.inf                          # isnan, not isinf: an infinite term stays
    sums, loss, d = api.loss(inf, BLEND)
    assert np.isinf(sums[0]) and sums[3] == 0 and np.isinf(loss)


# ------------------------------------------------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("S,L", mk.BUILD_SHAPES)
def test_hostsim_points_build_matches_the_reference(sim, gold, S, L):
    check_build(sim, gold, S, L)


@pytest.mark.parametrize("C", [1, 3, 45, 48, 49])
@pytest.mark.parametrize("S,n_seg", [(1, 1), (3, 99), (300, 7), (2, 1025)])
def test_hostsim_rows_expand_is_exact_and_reduce_is_a_sequential_sum(sim, S, n_seg, C):
    check_rows(sim, S, n_seg, C)


@pytest.mark.parametrize("H,W", mk.LOSS_SHAPES)
def test_hostsim_latent_loss_matches_the_reference(sim, gold, H, W):
    check_loss_golden(sim, gold, H, W)


def test_hostsim_latent_loss_drops_exactly_the_nan_terms(sim, gold):
    check_loss_nan_rules(sim, golden_case(gold, 12, 20)[0])


def test_hostsim_latent_loss_fold_over_several_workgroups(sim):
    """(36, 68): three workgroups' slots, the last one partly filled; against the comparator in float64"""
    c = {k: v.numpy() if isinstance(v, torch.Tensor) else v for k, v in lc.make_case(36, 68).items()}
    f64, g64 = comparator_loss(c, BLEND, torch.float64)
    f32, _ = comparator_loss(c, BLEND, torch.float32)
    sums, loss, d = sim.loss(c, BLEND)
    assert sums.size == 8 + 4 * 3
    check_loss_value(loss, f64, f32)
    lc.check_grad(d, g64, c["special"])


@pytest.mark.parametrize("S,L", [(3, 3), (7, 100), (1, 257)])
def test_comparator_build_equals_the_golden(gold, S, L):
    key = "b%dx%d/" % (S, L)
    p, cots = gold[key + "p"], {k: v.numpy() for k, v in mk.make_cots(S, L).items()}
    o32, _ = comparator_build(p, cots, torch.float32)
    assert o32["xyz"].tobytes() == gold[key + "xyz32"].tobytes() and o32["dir"].tobytes() == gold[key + "dir32"].tobytes()
    assert np.allclose(o32["rot"], gold[key + "rot32"], rtol=0, atol=3e-7)
    assert np.allclose(o32["scaling"], gold[key + "scaling32"], rtol=3e-7, atol=0)
    deg = degenerate_points(gold[key + "dir32"], S, L)
    check_d_p(comparator_build(p, cots, torch.float64)[1], gold[key + "d_p64"], deg)
    for k in mk.COTS:
        if key + "d_p64_" + k in gold.files:
            check_d_p(comparator_build(p, cots, torch.float64, (k,))[1], gold[key + "d_p64_" + k], deg, k)


@pytest.mark.parametrize("H,W", mk.LOSS_SHAPES)
def test_comparator_loss_equals_the_golden(gold, H, W):
    c, key = golden_case(gold, H, W)
    v32, v64 = dict(zip(mk.TERMS, gold[key + "val32"])), dict(zip(mk.TERMS, gold[key + "val64"]))
    for term, (w, conf, weight) in VARIANTS.items():
        f64, g64 = comparator_loss(c, w, torch.float64, conf, weight)
        f32, g32 = comparator_loss(c, w, torch.float32, conf, weight)
        check_loss_value(f64, v64[term], v64[term], term)
        check_loss_value(f32, v64[term], v32[term], term)
        lc.check_grad(g64, gold[key + "grad64_" + term], c["special"], term)
        lc.check_grad(g32, gold[key + "grad64_" + term], c["special"], term)


def test_comparator_loss_drops_nan_terms_and_the_generators_term():
    from gaussianhaircut_amd.trainer import latent_view_loss
    c = {k: v.numpy() if isinstance(v, torch.Tensor) else v for k, v in lc.make_case(6, 7).items()}
    f0, g0 = comparator_loss(c, BLEND, torch.float32)
    bad = dict(c)
    bad["renders"] = c["renders"].copy()
    bad["renders"][0, 0, 0] = np.nan
    f1, g1 = comparator_loss(bad, BLEND, torch.float32)
    assert np.isfinite(f1) and not g1[0:3].any() and g1[3:].tobytes() == g0[3:].tobytes()
    pkg = {"render": torch.zeros(3, 2, 2), "mask": torch.zeros(2, 2, 2), "orient_angle": torch.zeros(1, 2, 2),
           "orient_conf": torch.ones(1, 2, 2)}
    cam = SimpleNamespace(original_image=torch.ones(3, 2, 2), original_mask=torch.ones(2, 2, 2),
                          original_orient_angle=torch.full((1, 2, 2), 0.2), original_orient_conf=torch.ones(1, 2, 2))
    opt = SimpleNamespace(lambda_dl1=1.0, lambda_dmask=1.0, lambda_dorient=1.0, lambda_dsds=0.5, use_gt_orient_conf=True,
                          train_orient_conf=True)
    z = torch.tensor(2.0, requires_grad=True)
    base = float(latent_view_loss(pkg, cam, opt, fused=False))
    with_term = latent_view_loss(pkg, cam, opt, l_diff=z * 3.0, fused=False)
    assert abs(float(with_term.detach()) - (base + 3.0)) < 1e-6
    with_term.backward()
    assert float(z.grad) == 1.5
    z.grad = None
    nan_term = latent_view_loss(pkg, cam, opt, l_diff=z * float("nan"), fused=False)
    assert float(nan_term.detach()) == base


def test_model_on_the_cpu_takes_the_torch_form_and_keeps_the_reference_layout():
    from gaussianhaircut_amd.scene.gaussian_model_latent_strands import GaussianModelHair, GaussianModelLatentStrands
    from gaussianhaircut_amd.scene.gaussian_model_strands import GaussianModelStrands
    assert GaussianModelHair is GaussianModelLatentStrands and issubclass(GaussianModelHair, GaussianModelStrands)
    assert GaussianModelLatentStrands is not GaussianModelStrands
    S, L, K = 4, 6, 16
    g = torch.Generator().manual_seed(2)
    pts = torch.nn.Parameter(torch.randn(S, L, 3, generator=g))
    lin = torch.nn.Linear(8, 3 * K)
    code = torch.nn.Parameter(torch.randn(S, 8, generator=g))
    calls = []

    def generator(iteration):
        calls.append(iteration)
        return {"points": pts * 1.0, "features": lin(code), "orient_conf": code[:, :1] * 0.1, "L_diff": (pts ** 2).mean()}

    m = GaussianModelLatentStrands(3, generator, lin)
    assert m.active_sh_degree == m.max_sh_degree == 3
    m.initialize_gaussians_hair(7)
    P = S * (L - 1)
    assert calls == [7] and m.num_strands == S and m.strand_length == L
    assert m._xyz.shape == (P, 3) and m._rotation.shape == (P, 4) and m.get_scaling.shape == (P, 3) and m._dir.shape == (P, 3)
    assert m._features_dc.shape == (P, 1, 3) and m._features_rest.shape == (P, K - 1, 3) and m._orient_conf.shape == (P, 1)
    assert torch.equal(m.get_opacity, torch.ones(P, 1)) and torch.equal(m.get_label, torch.ones(P, 1))
    z = lin(code)
    dc, rest = z.view(S, 1, 3 * K).split([3, 3 * (K - 1)], dim=-1)       # :464-467
    assert torch.equal(m._features_dc, dc.repeat(1, L - 1, 1).reshape(P, 1, 3))
    assert torch.equal(m._features_rest, rest.repeat(1, L - 1, 1).reshape(P, K - 1, 3))
    assert torch.equal(m._xyz, (pts[:, 1:] + pts[:, :-1]).view(-1, 3) * 0.5) and m.LDiff is not None
    (m._xyz.sum() + m._features_rest.sum() + m.LDiff).backward()
    assert pts.grad is not None and lin.weight.grad is not None
    # per-segment features are taken as they are; no L_diff: LDiff is None
    m2 = GaussianModelLatentStrands(3, lambda it: {"points": pts.detach(), "features": torch.ones(P, 3 * K)})
    m2.initialize_gaussians_hair(1)
    assert m2._features_dc.shape == (P, 1, 3) and m2.LDiff is None and not m2._orient_conf.any()
    # the six-slot checkpoint (:84-107)
    m.training_setup(SimpleNamespace(iterations=10))
    cap = m.capture()
    assert len(cap) == 6 and cap[1] == 3 and set(cap[3]) == {"weight", "bias"} and "param_groups" in cap[4]
    m3 = GaussianModelLatentStrands(3, generator, torch.nn.Linear(8, 3 * K))
    m3.restore(cap, SimpleNamespace(iterations=10))
    assert torch.equal(m3.color_decoder.weight, lin.weight) and m3.scheduler is not None


def test_c_abi_symbols_and_refusals():
    """the seven symbols are exported and declared; every refusal names its field (and launches nothing: the pointers below are
    not device memory)"""
    L = _lib.lib()
    names = ["ghr_strand_points_build", "ghr_strand_points_build_backward", "ghr_strand_rows_expand", "ghr_strand_rows_reduce",
             "ghr_latent_loss_sums_floats", "ghr_latent_loss_forward", "ghr_latent_loss_backward"]
    hdr = open(os.path.join(hp.ROOT, "include", "ghr.h")).read()
    for n in names:
        assert n in _lib.EXPORTS and hasattr(L, n) and n + "(" in hdr
    assert "ghr_latent.h" in _lib.HEADERS and int(L.ghr_abi_version()) == _lib.ABI_VERSION
    buf = np.zeros(64, np.float32)
    q = _p(buf)

    def refused(rc, field):
        msg = L.ghr_last_error().decode()
        assert rc == _lib.GHR_E_INVALID and field in msg, (rc, msg, field)

    refused(L.ghr_strand_points_build(None, 1, 1, q, 1e-3, q, q, q, q), "L < 2")
    refused(L.ghr_strand_points_build(None, -1, 2, q, 1e-3, q, q, q, q), "S < 0")
    for i, field in enumerate(("p", "xyz", "rotation", "scaling", "dir_rows")):
        a = [q] * 5
        a[i] = None
        refused(L.ghr_strand_points_build(None, 1, 2, a[0], 1e-3, a[1], a[2], a[3], a[4]), field + " is NULL")
    refused(L.ghr_strand_points_build_backward(None, 1, 1, q, q, q, q, q, q), "L < 2")
    refused(L.ghr_strand_points_build_backward(None, 1, 2, None, q, q, q, q, q), "p is NULL")
    refused(L.ghr_strand_points_build_backward(None, 1, 2, q, q, q, q, q, None), "d_p is NULL")
    for fn, fields in ((L.ghr_strand_rows_expand, ("src", "dst")), (L.ghr_strand_rows_reduce, ("g", "out"))):
        refused(fn(None, 1, 1, 0, q, q), "C < 1")
        refused(fn(None, 1, 0, 3, q, q), "n_seg < 1")
        refused(fn(None, 1, 1, 3, None, q), fields[0] + " is NULL")
        refused(fn(None, 1, 1, 3, q, None), fields[1] + " is NULL")
    assert L.ghr_strand_points_build(None, 0, 2, None, 1e-3, None, None, None, None) == 0     # nothing to do
    assert L.ghr_latent_loss_sums_floats(0, 5) == 0 and L.ghr_latent_loss_sums_floats(1024, 1) == 8 + 4
    assert L.ghr_latent_loss_sums_floats(1025, 1) == 8 + 8 and L.ghr_latent_loss_sums_floats(1920, 1080) == 8 + 4 * 2025
    full = dict(image=buf.ctypes.data, mask0=buf.ctypes.data, dir2d=buf.ctypes.data, orient_conf=None, gt_image=buf.ctypes.data,
                gt_mask0=buf.ctypes.data, gt_orient_angle=buf.ctypes.data, gt_orient_conf=None)
    for W, H in ((0, 4), (4, 0)):
        a = loss_struct(W, H, full, BLEND)
        refused(L.ghr_latent_loss_forward(None, ctypes.byref(a), q, q), "W * H == 0")
        refused(L.ghr_latent_loss_backward(None, ctypes.byref(a), q, None, q), "W * H == 0")
    for field in ("image", "mask0", "dir2d", "gt_image", "gt_mask0", "gt_orient_angle"):
        a = loss_struct(2, 2, dict(full, **{field: None}), BLEND)
        refused(L.ghr_latent_loss_forward(None, ctypes.byref(a), q, q), field + " is NULL")
        refused(L.ghr_latent_loss_backward(None, ctypes.byref(a), q, None, q), field + " is NULL")
    a = loss_struct(2, 2, full, BLEND)
    refused(L.ghr_latent_loss_forward(None, None, q, q), "args is NULL")
    refused(L.ghr_latent_loss_forward(None, ctypes.byref(a), None, q), "sums is NULL")
    refused(L.ghr_latent_loss_forward(None, ctypes.byref(a), q, None), "loss_out is NULL")
    refused(L.ghr_latent_loss_backward(None, ctypes.byref(a), None, None, q), "sums is NULL")
    refused(L.ghr_latent_loss_backward(None, ctypes.byref(a), q, None, None), "d_packed is NULL")
