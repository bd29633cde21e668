"""Closest point on / signed distance to a triangle mesh on the GPU (csrc/ghr_meshdist.h through gaussianhaircut_amd/mesh.py;
DESIGN.md 8o).  Every comparison is bit for bit: the HIP search against the numpy float32 model of the definition
(tests/mesh_distance_cases.py) and against the PyTorch-composed comparator on the device, on every case -- the partial last
block (63 / 65 faces), the two-superblock meshes (4097 / 5120 faces), the non-finite queries -- and at Q = 1, 63, 64, 65, 257;
under a permutation of the queries and of the faces; signed_distance forward and backward; one strand training step with the
collision term attached (HIP against the composed term) and unattached (against a process that never imported the module)."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd import mesh as gm
from gaussianhaircut_amd.mesh import HeadMesh
from tests import mesh_cases as mc
from tests import mesh_distance_cases as dc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FUSED = SimpleNamespace(debug=False, fused_projection=True)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want):
    return all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want))


@pytest.fixture(scope="module")
def head_meshes():
    return {n: HeadMesh(*dc.meshes()[n][:2]) for n in dc.CASES}


@pytest.mark.parametrize("name", dc.CASES)
def test_fused_equals_the_model_and_the_comparator_bit_for_bit(head_meshes, name):
    q, d, face, p = dc.expected(name)
    mesh = head_meshes[name]
    t = torch.from_numpy(q).to(DEV)
    got = mesh.closest_point(t, fused=True)
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32 and got[2].shape == (len(q), 3)
    assert _same(got, (d, face, p)), name
    assert _same(mesh.closest_point(t, fused=False), (d, face, p)), name
    bad = ~np.isfinite(q).all(1)
    assert bool(torch.isinf(got[0][torch.from_numpy(bad).to(DEV)]).all()) and bool((got[1].cpu()[bad] == -1).all())


@pytest.mark.parametrize("Q", dc.Q_SIZES)
@pytest.mark.parametrize("name", ["icosphere2", "ico4_65", "ico4_4097"])
def test_partial_waves_and_workgroups(head_meshes, name, Q):
    q, d, face, p = dc.expected(name)
    got = head_meshes[name].closest_point(torch.from_numpy(q[:Q]).to(DEV), fused=True)
    assert _same(got, (d[:Q], face[:Q], p[:Q])), (name, Q)


def test_shapes_are_kept_and_an_empty_query_launches_nothing(head_meshes):
    q, d, face, p = dc.expected("torus")
    mesh = head_meshes["torus"]
    d2, f2, p2 = mesh.closest_point(torch.from_numpy(q[:90]).to(DEV).reshape(9, 10, 3))
    assert d2.shape == (9, 10) and f2.shape == (9, 10) and p2.shape == (9, 10, 3)
    assert _same((d2.reshape(-1), f2.reshape(-1), p2.reshape(-1, 3)), (d[:90], face[:90], p[:90]))
    e = mesh.closest_point(torch.zeros(0, 3, device=DEV))
    assert e[0].shape == (0,) and e[1].shape == (0,) and e[2].shape == (0, 3)


@pytest.mark.parametrize("name", ["torus", "ico4_5120"])
def test_results_do_not_depend_on_the_order_of_queries_or_faces(head_meshes, name):
    v, f, _ = dc.meshes()[name]
    q, d, face, p = dc.expected(name)
    rng = np.random.default_rng(5)
    pq, pf = rng.permutation(len(q)), rng.permutation(len(f))
    qp, fp = np.ascontiguousarray(q[pq]), np.ascontiguousarray(f[pf])
    # the queries permuted: the same bits at the permuted places
    got = head_meshes[name].closest_point(torch.from_numpy(qp).to(DEV))
    assert _same(got, (d[pq], face[pq], p[pq]))
    # the faces permuted (renamed): the same d; among the faces at that d the lowest NEW index wins, as the comparator says;
    # mapped back it is the same face and the same point wherever one face alone reaches the smallest d
    renamed = HeadMesh(v, fp)
    got = renamed.closest_point(torch.from_numpy(qp).to(DEV))
    assert np.array_equal(_bits(got[0]), _bits(d[pq]))
    assert _same(got, renamed.closest_point(torch.from_numpy(qp).to(DEV), fused=False))
    fin = np.isfinite(qp).all(1)
    sub = np.nonzero(fin)[0][:400]
    pairs, _ = dc.model_pairs(v, f, qp[sub])
    alone = (pairs == pairs.min(1, keepdims=True)).sum(1) == 1
    assert alone.sum() > 100
    back = pf[got[1].cpu().numpy()[sub][alone]]
    assert np.array_equal(back, face[pq][sub][alone]) and np.array_equal(_bits(got[2])[sub][alone], _bits(p[pq])[sub][alone])


@pytest.mark.parametrize("name", ["icosphere2", "cube", "ico4_4097"])
def test_signed_distance_forward_and_backward_equal_the_comparator(head_meshes, name):
    q, d, _, _ = dc.expected(name)
    mesh = head_meshes[name]
    g = torch.from_numpy(np.random.default_rng(3).normal(0, 1, len(q)).astype(np.float32)).to(DEV)
    out = {}
    for fused in (True, False):
        x = torch.from_numpy(q).to(DEV).requires_grad_(True)
        sd = gm.signed_distance(x, mesh, fused=fused)
        sd.backward(g)
        out[fused] = (sd.detach(), x.grad)
    assert _same(out[True], out[False]), name
    sd, grad = out[True]
    inside = mesh.contains(torch.from_numpy(q).to(DEV))
    root = np.sqrt(d)
    assert np.array_equal(_bits(sd), _bits(np.where(inside.cpu().numpy(), -root, root)))
    dead = (d == 0) | ~np.isfinite(d) | ~np.isfinite(q).all(1)
    assert dead.sum() > 20 and bool((grad.cpu()[dead] == 0).all()) and bool(torch.isfinite(grad).all())
    assert float(grad.cpu()[~dead].abs().max()) > 0
    if name == "icosphere2":
        assert torch.equal(mesh.signed_distance(torch.from_numpy(q).to(DEV).reshape(-1, 1, 3)).reshape(-1), sd)


def test_split_strands_on_the_device_equals_the_composed_form():
    from gaussianhaircut_amd import between_stages as bs
    head = HeadMesh(*mc.meshes()["icosphere2"][:2])
    scalp = HeadMesh(*mc.icosphere(2, 1.02))
    rng = np.random.default_rng(8)
    roots = rng.normal(0, 1, (40, 1, 3))
    roots = 1.02 * roots / np.linalg.norm(roots, axis=-1, keepdims=True)
    steps = np.cumsum(rng.normal(0, 0.08, (40, 12, 3)), axis=1)
    pts = torch.from_numpy(np.concatenate([roots, roots + steps], axis=1).astype(np.float32))
    a, sa = bs.split_strands(pts.to(DEV), head, scalp, max_root_dist=0.05)
    b, sb = bs.split_strands(pts, head, scalp, max_root_dist=0.05, fused=False)
    assert a.is_cuda and torch.equal(a.cpu(), b) and torch.equal(sa.cpu(), sb)
    assert 0 < a.shape[0] and len(set(sb.tolist())) < len(sb)              # some strand was cut and re-rooted


# ---- the trainer --------------------------------------------------------------------------------------------------------------------
def _scene():
    from tests.test_gpu_strand_prior import _scene as strand_scene
    return strand_scene()


def _collision_mesh(hair):
    """a box over the lower half of the strands' own points: some points are inside, some are not"""
    p = hair._pts.detach().reshape(-1, 3).cpu().numpy()
    lo, hi = p.min(0), p.max(0)
    v, f = mc.box(lo - 0.01, [hi[0] + 0.01, (lo[1] + hi[1]) / 2, hi[2] + 0.01])
    return HeadMesh(v, f)


def _steps(attach, n=2):
    """n strand training steps; attach: None, or fused True / False of the collision term.  Returns the parameters after each."""
    from gaussianhaircut_amd.trainer import strand_training_step
    lib = _lib.lib()
    lib.ghr_set_deterministic(1)
    try:
        opt, bg, head, hair, cam = _scene()
        if attach is not None:
            from gaussianhaircut_amd.strand_collision import HeadCollision
            opt.lambda_dpen = 0.5
            hair.attach_collision(HeadCollision(_collision_mesh(hair), margin=0.01, stride=1, fused=attach))
        trace, pens = [], []
        for i in range(n):
            loss = strand_training_step(head, hair, [cam], bg, opt, i + 1, pipe=FUSED)
            assert bool(torch.isfinite(loss))
            trace.append([p.detach().cpu().clone() for p in (hair._dirs, hair._features_dc, hair._features_rest, hair._orient_conf)])
            pens.append(None if attach is None else hair.Lpen.detach().cpu())
        return trace, pens
    finally:
        lib.ghr_set_deterministic(0)


def test_training_step_with_the_collision_term_equals_the_composed_term():
    hip, pen_hip = _steps(True)
    cmp_, pen_cmp = _steps(False)
    plain, _ = _steps(None)
    assert float(pen_hip[0]) > 0
    for it in range(len(hip)):
        assert torch.equal(pen_hip[it], pen_cmp[it]), it
        for x, y in zip(hip[it], cmp_[it]):
            assert torch.equal(x, y), (it, float((x - y).abs().max()))
    assert not torch.equal(hip[0][0], plain[0][0])     # the term reaches the strand directions
    assert torch.equal(hip[0][1], plain[0][1])         # and, in the first step, nothing else


def test_unattached_step_equals_a_run_that_never_imported_the_module(tmp_path):
    """The child process runs the same two steps with nothing attached and checks that gaussianhaircut_amd.strand_collision was
    never imported; a process of its own is the only way to have that (this module's other tests import it)."""
    out = str(tmp_path / "plain.pt")
    code = ("import sys, torch\n"
            "from tests import test_gpu_mesh_distance as t\n"
            "trace, _ = t._steps(None)\n"
            "assert 'gaussianhaircut_amd.strand_collision' not in sys.modules\n"
            "torch.save(trace, sys.argv[1])\n")
    res = subprocess.run([sys.executable, "-c", code, out], cwd=ROOT, capture_output=True, text=True, timeout=300,
                         env={**os.environ, "PYTHONPATH": ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")})
    assert res.returncode == 0, res.stdout + res.stderr
    want = torch.load(out)
    from gaussianhaircut_amd.strand_collision import HeadCollision  # noqa: F401  (imported here: it changes nothing)
    got, _ = _steps(None)
    for it in range(len(got)):
        for x, y in zip(got[it], want[it]):
            assert torch.equal(x, y), it
