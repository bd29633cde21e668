"""Point-in-mesh containment and the between-stage filters on the device (csrc/ghr_mesh.h), through the C ABI and the Python API.

Every result is a byte or an integer and every comparison is exact: k_mesh_contains and k_gaussian_probe_outside against the
numpy float32 model of the definition (tests/mesh_cases.py, brute force over all faces) and against the PyTorch-composed forms
evaluated on the device.  Outputs land in poisoned buffers between guards.  The non-finite queries run on the CPU only
(tests/test_mesh_cpu.py)."""
import ctypes

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd import between_stages as bs
from gaussianhaircut_amd.mesh import HeadMesh
from gaussianhaircut_amd.utils import synthetic as syn
from tests import mesh_cases as mc

pytestmark = pytest.mark.gpu
CASES = list(mc.meshes())
GUARD = 64
POISON = 0xA5


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model():
    """name -> (inside, crossings) of the numpy model on the first 1000 finite queries of the case; computed once"""
    out = {}
    for n in CASES:
        v, f, _, _ = mc.meshes()[n]
        out[n] = mc.model_contains(v, f, mc.queries(n)[:1000])
    return out


@pytest.fixture(scope="module")
def head_meshes():
    return {n: HeadMesh(*mc.meshes()[n][:3]) for n in CASES}


def _contains_capi(mesh, q_dev, with_counts=True):
    """ghr_mesh_contains into poisoned, guarded buffers"""
    Q = q_dev.shape[0]
    inside = torch.full((Q + 2 * GUARD,), POISON, dtype=torch.uint8, device=q_dev.device)
    cross = torch.full((Q + 2 * GUARD, 3), -1, dtype=torch.int32, device=q_dev.device)
    tab = mesh._tables(q_dev.device)
    _lib.check(_lib.lib().ghr_mesh_contains(_stream(), ctypes.byref(mesh.header), _ptr(tab), Q, _ptr(q_dev) if Q else None,
                                            _ptr(inside[GUARD:]), _ptr(cross[GUARD:]) if with_counts else None))
    torch.cuda.synchronize()
    i, c = inside.cpu().numpy(), cross.cpu().numpy()
    assert (i[:GUARD] == POISON).all() and (i[GUARD + Q:] == POISON).all()
    assert (c[:GUARD] == -1).all() and (c[GUARD + Q:] == -1).all()
    return i[GUARD:GUARD + Q], c[GUARD:GUARD + Q].astype(np.uint32)


@pytest.mark.parametrize("name", CASES)
def test_mesh_contains_equals_the_model_at_the_block_boundaries(dev, model, head_meshes, name):
    mesh = head_meshes[name]
    q = mc.queries(name)[:1000]
    want_in, want_c = model[name]
    for Q in (0, 1, 63, 64, 65, 1000):
        qd = torch.from_numpy(q[:Q].copy()).to(dev)
        inside, c = _contains_capi(mesh, qd)
        assert np.array_equal(c, want_c[:Q]), (name, Q)
        assert np.array_equal(inside, want_in[:Q].astype(np.uint8)), (name, Q)
    inside, c = _contains_capi(mesh, qd, with_counts=False)           # crossings are optional
    assert np.array_equal(inside, want_in.astype(np.uint8)) and (c == 0xFFFFFFFF).all()
    # the Python API: fused against the composed form on the device
    fi, fc = mesh.contains(qd, fused=True, return_crossings=True)
    ti, tc = mesh.contains(qd, fused=False, return_crossings=True)
    assert torch.equal(fi, ti) and torch.equal(fc, tc)
    assert np.array_equal(fi.cpu().numpy(), want_in) and np.array_equal(fc.cpu().numpy().astype(np.uint32), want_c)


def test_cube_tie_lattice_follows_the_half_open_rule_on_the_device(dev, head_meshes):
    lat = mc.cube_tie_lattice()
    for a in range(3):
        _, c = _contains_capi(head_meshes["cube"], torch.from_numpy(lat[a].copy()).to(dev))
        assert np.array_equal((c[:, a] & 1).astype(bool), mc.half_open_rule(lat[a], a)), a


PROBE_P = (0, 1, 3, 4, 5, 63, 64, 65, 1001)


@pytest.fixture(scope="module")
def probe_model():
    out = {}
    for name in ("icosphere2", "stack65"):
        v, f, _, _ = mc.meshes()[name]
        g = mc.gaussians(name, max(PROBE_P))
        out[name] = (g, [mc.model_probes_outside(v, f, *g, mode) for mode in (0, 1)])
    return out


@pytest.mark.parametrize("probe,mode", [("reference", 0), ("axis_scaled", 1)])
@pytest.mark.parametrize("name", ["icosphere2", "stack65"])
def test_gaussian_probe_outside_at_the_row_and_wave_boundaries(dev, head_meshes, probe_model, name, probe, mode):
    mesh = head_meshes[name]
    (xyz, s, r), want = probe_model[name]
    assert not np.allclose(np.linalg.norm(r, axis=1), 1.0, atol=0.1)   # un-normalised quaternions
    tab = mesh._tables(dev)
    for P in PROBE_P:
        t = [torch.from_numpy(a[:P].copy()).to(dev) for a in (xyz, s, r)]
        out = torch.full((P + 2 * GUARD,), POISON, dtype=torch.uint8, device=dev)
        _lib.check(_lib.lib().ghr_gaussian_probe_outside(_stream(), ctypes.byref(mesh.header), _ptr(tab), P,
                                                         *[_ptr(x) if P else None for x in t], mode, _ptr(out[GUARD:])))
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert (o[:GUARD] == POISON).all() and (o[GUARD + P:] == POISON).all(), P
        assert np.array_equal(o[GUARD:GUARD + P], want[mode][:P].astype(np.uint8)), (name, probe, P)
        if P:
            composed = mesh.probes_outside(*t, probe=probe, fused=False)                 # torch probes + k_mesh_contains + all
            brute = mesh.probes_outside(*t, probe=probe, fused=False, fused_contains=False)  # torch all the way
            fused = mesh.probes_outside(*t, probe=probe, fused=True)
            assert torch.equal(fused, composed) and torch.equal(fused, brute), (name, probe, P)
            assert np.array_equal(fused.cpu().numpy(), want[mode][:P])
    if name == "icosphere2":
        assert 0 < want[mode].sum() < max(PROBE_P)


def test_filter_head_intersections_keeps_an_optimizer_consistent(dev):
    from gaussianhaircut_amd.optim import FusedAdam
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    from gaussianhaircut_amd.trainer import make_ground_truth, training_step
    spec = syn.CONFIGS["tiny"]  # 2000 Gaussians in [-1.3, 1.3]^3
    assert spec.P == 2000
    opt = OptimizationParams()
    mesh = HeadMesh(*mc.icosphere(2, 0.8))
    cam, bg = syn.make_view(spec, dev), syn.background(dev)
    gt = syn.make_model(spec, dev)
    with torch.no_grad():
        gt._features_dc.add_(0.3)
    make_ground_truth(gt, [cam], bg)
    res = []
    for fused in (True, False):
        m = syn.make_model(spec, dev)
        m.training_setup(opt)
        assert isinstance(m.optimizer, FusedAdam)
        gen = torch.Generator().manual_seed(77)               # non-trivial Adam moments, the same for both models (training
        for _, p, mm, vv in m.optimizer._group_views():       # steps would not do: their atomics make two runs differ)
            mm.copy_(torch.randn(p.shape, generator=gen).to(dev) * 1e-3)
            vv.copy_(torch.rand(p.shape, generator=gen).to(dev) * 1e-6)
        before = {g["name"]: (p.detach().clone(), mm.clone(), vv.clone()) for g, p, mm, vv in m.optimizer._group_views()}
        keep = bs.filter_head_intersections(m, mesh, fused=fused)
        after = {g["name"]: (p.detach().clone(), mm.clone(), vv.clone()) for g, p, mm, vv in m.optimizer._group_views()}
        res.append((m, keep, before, after))
    (mf, kf, bf, af), (mt, kt, bt, at) = res
    assert torch.equal(kf, kt) and 0 < int(kf.sum()) < spec.P
    label_low = (bf["label"][0].sigmoid().reshape(-1) <= 0.5)
    assert bool((kf | ~label_low).all()) and not bool(kf[~label_low].all())      # only hair-labelled Gaussians go
    assert mf.get_xyz.shape[0] == int(kf.sum())
    for k in af:
        for x, y, b in zip(af[k], at[k], bf[k]):
            assert torch.equal(x, y), k                       # the composed form's rows and moments
            assert torch.equal(x, b[kf]), k                   # = the surviving rows, untouched
    assert mf._xyz.data_ptr() == mf.optimizer.flat_param.data_ptr()
    losses = [float(training_step(mf, [cam], bg, opt, i + 3)) for i in range(3)]
    assert np.isfinite(losses).all()


@pytest.mark.parametrize("L", [2, 99, 100])
@pytest.mark.parametrize("S", [1, 70])
def test_prune_strands_equals_the_model(dev, head_meshes, S, L):
    v, f, _, _ = mc.meshes()["icosphere2"]
    rng = np.random.default_rng(S * 1000 + L)
    # strands that wander across the surface: a start inside 1.2 x the box and steps of 2 % of it
    p = (rng.uniform(-1.2, 1.2, (S, 1, 3)) + np.cumsum(rng.normal(0, 0.02, (S, L, 3)), axis=1)).astype(np.float32)
    outside = ~mc.model_contains(v, f, p.reshape(-1, 3))[0].reshape(S, L)
    want = 2 * outside.sum(1) >= L
    pd = torch.from_numpy(p).to(dev)
    kept, keep = bs.prune_strands(pd, head_meshes["icosphere2"])
    assert np.array_equal(keep.cpu().numpy(), want)
    assert torch.equal(kept, pd[torch.from_numpy(want).to(dev)])
    assert torch.equal(bs.prune_strands(pd, head_meshes["icosphere2"], fused=False)[1], keep)
