"""Closest point on / signed distance to a triangle mesh (csrc/ghr_meshdist.h, gaussianhaircut_amd/mesh.py), the strand collision
term and the strand split, without a GPU.

 1. the numpy float32 MODEL of the definition (tests/mesh_distance_cases.py) against a float64 truth (Ericson's region algorithm)
    on the closed case meshes, 20 000 random queries each: |sqrt(d) - truth| <= 16 * 2^-24 * E, no query left out;
 2. vertex queries: d == 0 and the lowest incident face;
 3. the product's own builder, per-element functions and a restatement of the wave walk compiled for the host
    (tests/hostsim/ghr_hostsim_meshdist.cpp, every index checked) against the model, bit for bit, on every case; the tables
    against their specification and the library's own build; boxdist <= d for every (query, face) pair of the small meshes;
 4. the same cases through a stand-alone program built with -fsanitize=address,undefined (nothing sanitized is loaded here);
 5. the PyTorch comparator (fused=False) on CPU tensors against the model, the sign, the backward against float64 autograd;
 6. split_strands on hand-made strands;
 7. HeadCollision and the strand training step on CPU tensors;
 8. the refusals of the C ABI."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd import between_stages as bs
from gaussianhaircut_amd import mesh as gm
from gaussianhaircut_amd.mesh import HeadMesh
from gaussianhaircut_amd.strand_collision import HeadCollision
from tests import helpers as hp
from tests import mesh_cases as mc
from tests import mesh_distance_cases as dc

DEPS = ["ghr_hostsim_meshdist.cpp", "ghr_meshdist.h", "ghr_mesh.h", "ghr_nn.h", "ghr_knn.h"]
EPS = 2.0 ** -24


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def sim():
    L = ctypes.CDLL(hp.compile_hostsim("libghr_hostsim_meshdist.so", "ghr_hostsim_meshdist.cpp", ["-O2", "-fPIC", "-shared"], DEPS))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    L.ghrsim_md_sizes.argtypes = [i32, vp, i32, vp, vp, vp]
    L.ghrsim_md_build.argtypes = [i32, vp, i32, vp, vp, ctypes.c_ulonglong, vp]
    L.ghrsim_md_verify.argtypes = [vp, vp, vp]
    L.ghrsim_md_keys.argtypes = [vp, i64, vp, vp]
    L.ghrsim_md_closest.argtypes = [vp, i64] + [vp] * 7
    L.ghrsim_md_check_bounds.argtypes = [vp, i64, vp]
    L.ghrsim_md_check_bounds.restype = ctypes.c_longlong
    L.ghrsim_md_backward.argtypes = [i64] + [vp] * 6
    L.ghrsim_md_faces_taken.restype = ctypes.c_ulonglong
    assert L.ghrsim_md_header_bytes() == ctypes.sizeof(_lib.MeshTris)
    return L


def _sim_build(sim, v, f):
    h, why = _lib.MeshTris(), ctypes.create_string_buffer(128)
    assert sim.ghrsim_md_sizes(len(v), _p(v), len(f), _p(f), ctypes.byref(h), why) == 0, why.value
    blob = np.zeros(int(h.bytes) // 16, dtype=[("a", "<u8"), ("b", "<u8")]).view(np.uint8)  # 16-B aligned
    assert blob.ctypes.data % 16 == 0
    assert sim.ghrsim_md_build(len(v), _p(v), len(f), _p(f), _p(blob), int(h.bytes), why) == 0, why.value
    return blob


@pytest.fixture(scope="module")
def blobs(sim):
    return {n: _sim_build(sim, *dc.meshes()[n][:2]) for n in dc.CASES}


def _sim_closest(sim, blob, q, order=None, keys=None):
    q = np.ascontiguousarray(q, np.float32)
    Q = len(q)
    d, f, p = np.full(Q, 7, np.float32), np.full(Q, 7, np.int32), np.full((Q, 3), 7, np.float32)
    scanned = np.zeros((Q + 63) // 64, np.uint32)
    sim.ghrsim_md_closest(_p(blob), Q, _p(q), None if order is None else _p(order), None if keys is None else _p(keys), _p(d), _p(f),
                          _p(p), _p(scanned))
    return d, f, p, scanned


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.CLOSED)
def test_model_agrees_with_the_float64_truth(name):
    v, f, _ = dc.meshes()[name]
    lo, hi = mc.mesh_box(v, f)
    rng = np.random.default_rng(1)
    q = ((lo + hi) / 2 + rng.uniform(-1.5, 1.5, (20000, 3)) * (hi - lo).max() / 2).astype(np.float32)
    d, face, _ = dc.model_closest(v, f, q)
    truth = dc.truth_distance(v, f, q)
    E = dc.max_coord_diff(v, f, q)
    err = np.abs(np.sqrt(d.astype(np.float64)) - truth)
    print("%s: max |sqrt(d) - truth| = %.3f * 2^-24 * E (E = %.3f)" % (name, err.max() / (EPS * E), E))
    assert (face >= 0).all() and np.isfinite(truth).all()
    assert float(err.max()) <= 16 * EPS * E, (name, err.max() / (EPS * E))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.CASES)
def test_vertex_queries_are_at_distance_zero_on_their_lowest_face(name):
    v, f, _ = dc.meshes()[name]
    used = np.unique(f)
    if name not in dc.BASE:
        used = used[:400]
    d, face, p = dc.model_closest(v, f, v[used])
    lowest = np.array([np.nonzero((f == i).any(1))[0][0] for i in used], np.int32)
    assert (d == 0).all() and np.array_equal(face, lowest)
    assert np.array_equal(p, v[used])


def test_model_ties_on_the_integer_cube_go_to_the_lowest_face():
    v, f, _ = dc.meshes()["cube"]
    d, face, p = dc.model_closest(v, f, np.array([[2, 2, 2], [2, 2, 1], [5, 5, 5], [2, -1, 2]], np.float32))
    assert d.tolist() == [4.0, 1.0, 3.0, 1.0]
    pairs, _ = dc.model_pairs(v, f, np.array([[2, 2, 2]], np.float32))
    assert (pairs[0] == 4.0).sum() >= 6 and face[0] == int(np.nonzero(pairs[0] == 4.0)[0][0])   # every side ties at the centre
    assert p[2].tolist() == [4.0, 4.0, 4.0]


def test_model_refuses_non_finite_queries_and_takes_degenerate_faces():
    v, f, _ = dc.meshes()["flat"]
    q = dc.nonfinite_queries()
    d, face, p = dc.model_closest(v, f, q)
    bad = ~np.isfinite(q).all(1)
    assert bad.sum() == 11 and np.isinf(d[bad]).all() and (face[bad] == -1).all()
    assert np.array_equal(_bits(p[bad]), _bits(q[bad]))
    assert (face[~bad] >= 0).all()                      # 1e30 is a finite float: it is answered (d overflows to +inf)
    # the collinear triangle (face 12) answers through its edges
    dd, ff, pp = dc.model_closest(v, f[12:13], np.array([[0.0, 0.0, 0.0], [0.125, 0.0625, 0.5]], np.float32))
    assert dd.tolist() == [0.0, 0.25] and ff.tolist() == [0, 0] and pp[1].tolist() == [0.125, 0.0625, 0.0]


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.CASES)
def test_tables_meet_their_specification_and_are_the_librarys(sim, blobs, name):
    v, f, _ = dc.meshes()[name]
    blob = blobs[name]
    assert sim.ghrsim_md_verify(_p(v), _p(f), _p(blob)) == 0
    assert np.array_equal(blob, _sim_build(sim, v, f))               # deterministic
    mesh = HeadMesh(v, f)
    assert np.array_equal(mesh.tris_blob(), blob)                    # the library's host builder: the same bytes
    h = _lib.MeshTris.from_buffer_copy(blob[:ctypes.sizeof(_lib.MeshTris)].tobytes())
    assert h.n_faces == len(f) and h.n_blocks == (len(f) + 63) // 64 and h.n_super == (h.n_blocks + 63) // 64
    lo, hi = mc.mesh_box(v, f)
    assert list(h.lo) == lo.tolist() and list(h.hi) == hi.tolist()


def test_case_meshes_cover_the_block_and_superblock_edges(blobs):
    n = {name: _lib.MeshTris.from_buffer_copy(blobs[name][:ctypes.sizeof(_lib.MeshTris)].tobytes()) for name in dc.CASES}
    assert [n["ico4_%d" % k].n_blocks for k in dc.ICO4_SLICES] == [1, 1, 2, 64, 65, 80]
    assert [n["ico4_%d" % k].n_super for k in dc.ICO4_SLICES] == [1, 1, 1, 1, 2, 2]
    assert n["icosphere2"].n_blocks == 5 and n["torus"].n_blocks == 9


@pytest.mark.parametrize("name", dc.CASES)
def test_host_sim_equals_the_model_bit_for_bit(sim, blobs, name):
    q, d, face, p = dc.expected(name)
    got_d, got_f, got_p, scanned = _sim_closest(sim, blobs[name], q)
    assert np.array_equal(_bits(got_d), _bits(d))
    assert np.array_equal(got_f, face)
    assert np.array_equal(_bits(got_p), _bits(p))
    nb = (len(dc.meshes()[name][1]) + 63) // 64
    assert scanned.min() >= 1 and scanned.max() <= nb


@pytest.mark.parametrize("Q", dc.Q_SIZES)
@pytest.mark.parametrize("name", ["icosphere2", "ico4_4097"])
def test_host_sim_at_partial_waves(sim, blobs, name, Q):
    q, d, face, p = dc.expected(name)
    got_d, got_f, got_p, _ = _sim_closest(sim, blobs[name], q[:Q])
    assert np.array_equal(_bits(got_d), _bits(d[:Q])) and np.array_equal(got_f, face[:Q]) and np.array_equal(_bits(got_p), _bits(p[:Q]))


def test_host_sim_does_not_depend_on_the_order_of_queries_or_faces(sim, blobs):
    v, f, _ = dc.meshes()["torus"]
    q, d, face, p = dc.expected("torus")
    rng = np.random.default_rng(5)
    pq, pf = rng.permutation(len(q)), rng.permutation(len(f))
    fp, qp = np.ascontiguousarray(f[pf]), np.ascontiguousarray(q[pq])
    got_d, got_f, got_p, _ = _sim_closest(sim, _sim_build(sim, v, fp), qp)
    # the faces were renamed: among the faces at the smallest d the lowest NEW index wins (and with it that face's point)
    want_d, want_f, want_p = dc.model_closest(v, fp, qp)
    assert np.array_equal(_bits(got_d), _bits(want_d)) and np.array_equal(got_f, want_f) and np.array_equal(_bits(got_p), _bits(want_p))
    # mapped back: the same d for every query; the same face and point wherever one face alone reaches it
    assert np.array_equal(_bits(got_d), _bits(d[pq]))
    fin = np.isfinite(qp).all(1)
    pairs, _ = dc.model_pairs(v, f, qp[fin])
    alone = (pairs == pairs.min(1, keepdims=True)).sum(1) == 1
    assert alone.sum() > 300
    assert np.array_equal(pf[got_f[fin][alone]], face[pq][fin][alone]) and np.array_equal(_bits(got_p[fin][alone]), _bits(p[pq][fin][alone]))
    # a caller's bad permutation is clamped, a reversed (unsorted) one only costs speed
    order = np.arange(len(q), dtype=np.int64)[::-1].copy()
    keys = np.zeros(len(q), np.uint64)
    sim.ghrsim_md_keys(_p(blobs["torus"]), len(q), _p(q), _p(keys))
    got_d, got_f, _, _ = _sim_closest(sim, blobs["torus"], q, order, np.ascontiguousarray(keys[order]))
    assert np.array_equal(_bits(got_d), _bits(d)) and np.array_equal(got_f, face)
    order[3], order[7] = -5, len(q) + 9
    _sim_closest(sim, blobs["torus"], q, order, np.ascontiguousarray(keys[np.clip(order, 0, len(q) - 1)]))


@pytest.mark.parametrize("name", dc.SMALL)
def test_block_bounds_hold_for_every_pair_on_the_small_meshes(sim, blobs, name):
    q = dc.expected(name)[0]
    assert sim.ghrsim_md_check_bounds(_p(blobs[name]), len(q), _p(q)) == 0


def test_the_walk_prunes(sim, blobs):
    """near queries in key order skip most blocks of the two-superblock mesh (the far and the scattered ones cannot)"""
    v, f, _ = dc.meshes()["ico4_5120"]
    q = np.ascontiguousarray((v[np.unique(f)][:1024] * np.float32(1.01)).astype(np.float32))
    d, face, p = dc.model_closest(v, f, q)
    sim.ghrsim_md_faces_taken()  # zero
    got_d, got_f, got_p, scanned = _sim_closest(sim, blobs["ico4_5120"], q)
    taken = sim.ghrsim_md_faces_taken()
    assert np.array_equal(_bits(got_d), _bits(d)) and np.array_equal(got_f, face) and np.array_equal(_bits(got_p), _bits(p))
    print("blocks scanned per wave: mean %.1f of 80; faces evaluated: %d of the %d in them" % (scanned.mean(), taken, 64 * scanned.sum()))
    assert scanned.mean() < 40
    assert taken < 0.5 * 64 * scanned.sum()     # the ballot on a face's own box skips most faces of the scanned blocks


def test_host_sim_backward_is_the_unit_vector_from_the_closest_point(sim):
    v, f, _ = dc.meshes()["icosphere2"]
    q, d, face, p = dc.expected("icosphere2")
    inside = mc.model_contains(v, f, q)[0].astype(np.uint8)
    g = np.random.default_rng(2).normal(0, 1, len(q)).astype(np.float32)
    out = np.full((len(q), 3), 7, np.float32)
    sim.ghrsim_md_backward(len(q), _p(q), _p(p), _p(d), _p(inside), _p(g), _p(out))
    with np.errstate(all="ignore"):
        live = (d > 0) & np.isfinite(d) & np.isfinite(q).all(1)
        t = g * np.where(inside.astype(bool), np.float32(-1), np.float32(1))
        want = np.where(live[:, None], t[:, None] * ((q - p) / np.sqrt(d)[:, None]), np.float32(0)).astype(np.float32)
    assert (~live).sum() > 100 and np.array_equal(_bits(out), _bits(want))


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_sanitized_stand_alone_program_runs_the_cases_clean(tmp_path):
    """ghr_meshdist_selfcheck: the builder, the table check, the wave walk and the backward under AddressSanitizer and
    UndefinedBehaviorSanitizer, as a program of its own (exact-size buffers); the non-finite queries ride along."""
    san = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    if os.path.basename(hp.host_cxx()) == "g++":
        san += ["-static-libasan", "-static-libubsan"]
    exe = hp.compile_hostsim("ghr_meshdist_selfcheck_san", "ghr_meshdist_selfcheck.cpp", san, DEPS)
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as fh:
        for name in dc.CASES:
            v, f, _ = dc.meshes()[name]
            q, d, face, p = dc.expected(name)
            fh.write(np.array([len(v), len(f), len(q)], np.int32).tobytes())
            for arr in (v, f, q, d, face, p):
                fh.write(np.ascontiguousarray(arr).tobytes())
    res = subprocess.run([exe, path], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "%d cases ok" % len(dc.CASES) in res.stdout and "runtime error" not in res.stderr, res.stdout + res.stderr


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.CASES)
def test_torch_comparator_equals_the_model_on_cpu_tensors(name):
    v, f, _ = dc.meshes()[name]
    q, d, face, p = dc.expected(name)
    mesh = HeadMesh(v, f)
    got_d, got_f, got_p = mesh.closest_point(torch.from_numpy(q), fused=False)
    assert got_d.dtype == torch.float32 and got_f.dtype == torch.int32
    assert np.array_equal(_bits(got_d.numpy()), _bits(d)) and np.array_equal(got_f.numpy(), face)
    assert np.array_equal(_bits(got_p.numpy()), _bits(p))
    if name == "icosphere2":  # chunking does not enter, shapes are kept
        d2, f2, p2 = mesh.closest_point(torch.from_numpy(q[:90]).reshape(9, 10, 3), fused=False)
        assert d2.shape == (9, 10) and f2.shape == (9, 10) and p2.shape == (9, 10, 3)
        assert torch.equal(d2.reshape(-1), got_d[:90]) and torch.equal(p2.reshape(-1, 3), got_p[:90])
        d3, f3, _ = mesh._closest_torch(torch.from_numpy(q[:90]), chunk_elems=7)
        assert torch.equal(d3, got_d[:90]) and torch.equal(f3, got_f[:90])


@pytest.mark.parametrize("name", ["icosphere2", "cube", "torus"])
def test_signed_distance_has_the_sign_of_contains(name):
    v, f, _ = dc.meshes()[name]
    q, d, _, _ = dc.expected(name)
    mesh = HeadMesh(v, f)
    t = torch.from_numpy(q)
    sd = mesh.signed_distance(t, fused=False)
    inside = mesh.contains(t, fused=False)
    root = np.sqrt(d)
    assert 0 < int(inside.sum()) < len(q)
    assert np.array_equal(_bits(sd.numpy()), _bits(np.where(inside.numpy(), -root, root)))
    assert bool((sd[inside] <= 0).all()) and bool((sd[~inside] >= 0).all())       # negative INSIDE (pysdf: the opposite)
    assert torch.equal(gm.signed_distance(t.reshape(-1, 1, 3), mesh, fused=False).reshape(-1), sd)


def _sd64(v, f, q, face, inside, cand=None):
    """float64 autograd of the same formula on the winning face.  ``cand`` [Q]: the candidate of that face the float32 run
    selected (autograd never differentiates a selection: it is a constant of the graph); None: the smallest of the four float64
    candidates, selected anew."""
    fs = np.sort(f, axis=1)
    A, B, C = (torch.from_numpy(v[fs[face, k]].astype(np.float64)) for k in range(3))
    x = torch.from_numpy(q.astype(np.float64)).requires_grad_(True)

    def seg(P0, P1):
        e = P1 - P0
        t = (((x - P0) * e).sum(1) / (e * e).sum(1)).clamp(0, 1)
        c = P0 + t[:, None] * e
        return ((c - x) ** 2).sum(1)
    n = torch.linalg.cross(B - A, C - A)
    k = ((x - A) * n).sum(1) / (n * n).sum(1)
    c = x - k[:, None] * n
    ok = ((torch.linalg.cross(C - B, c - B) * n).sum(1) >= 0) & ((torch.linalg.cross(A - C, c - C) * n).sum(1) >= 0) & \
         ((torch.linalg.cross(B - A, c - A) * n).sum(1) >= 0)
    ds = torch.stack([seg(A, B), seg(A, C), seg(B, C), ((c - x) ** 2).sum(1)])
    if cand is None:
        ds = torch.cat([ds[:3], torch.where(ok, ds[3], torch.full_like(k, float("inf")))[None]])
        d = ds.min(0).values
    else:
        d = ds.gather(0, torch.from_numpy(cand.astype(np.int64))[None])[0]
    sd = torch.sqrt(d) * torch.from_numpy(np.where(inside, -1.0, 1.0))
    return x, sd


@pytest.mark.parametrize("name", ["icosphere2", "torus", "cube"])
def test_backward_against_float64_autograd(name):
    """Per component within 32 * 2^-24 * E / sqrt(d) * |g| of float64 autograd of the same formula, at every query with
    sqrt(d) >= 0.05 E, none left out.  The formula's two selections -- the winning face and which of its four candidates answered
    -- are taken from the float32 run: a selection is a constant of an autograd graph, and where two candidates' d agree to
    float32 rounding (a query whose projection falls within about sqrt(2^-24) |e| of an edge) float64 may select the other one,
    whose closest point lies up to 2 sqrt(d1 - d2) away.  Measured when float64 selects anew: icosphere2 2 of 1325 queries at 17.1
    and 7.3 times the bound, every other query at most 0.02 times it; those deviations are checked against the conditioning
    of the closest point instead: |c1 - c2| <= 2 sqrt(|d1 - d2|) on a convex face, with |d1 - d2| <= 8 * 2^-24 * d."""
    v, f, _ = dc.meshes()[name]
    lo, hi = mc.mesh_box(v, f)
    q = ((lo + hi) / 2 + np.random.default_rng(6).uniform(-0.75, 0.75, (1500, 3)) * (hi - lo)).astype(np.float32)
    d, face, _ = dc.model_closest(v, f, q)
    E = dc.max_coord_diff(v, f, q)
    far = np.sqrt(d.astype(np.float64)) >= 0.05 * E
    assert far.sum() > 300
    q, d, face = q[far], d[far], face[far]
    cand = np.array([dc.model_pairs(v, f[face[i]:face[i] + 1], q[i:i + 1], with_candidate=True)[2][0, 0] for i in range(len(q))])
    assert len(set(cand.tolist())) >= 2
    mesh = HeadMesh(v, f)
    x = torch.from_numpy(q).requires_grad_(True)
    sd = gm.signed_distance(x, mesh, fused=False)
    g = torch.from_numpy(np.random.default_rng(3).normal(0, 1, len(q)).astype(np.float32))
    sd.backward(g)
    inside = mesh.contains(x.detach(), fused=False).numpy()
    x64, sd64 = _sd64(v, f, q, face, inside, cand)
    sd64.backward(g.double())
    assert float((sd.detach().double() - sd64.detach()).abs().max()) <= 16 * EPS * E
    absg = np.abs(g.numpy().astype(np.float64))
    bound = 32 * EPS * E / np.sqrt(d.astype(np.float64)) * absg
    err = (x.grad.double() - x64.grad).abs().numpy()
    print("%s: max backward error / bound = %.3f over %d queries" % (name, (err / bound[:, None]).max(), len(q)))
    assert (err <= bound[:, None]).all()
    # float64 selecting the candidate anew: the same, but for near-ties of two candidates, bounded by their conditioning
    y64, sdy = _sd64(v, f, q, face, inside)
    sdy.backward(g.double())
    err2 = (x.grad.double() - y64.grad).abs().numpy()
    over = (err2 > bound[:, None]).any(1)
    print("%s: float64 selects anew: %d of %d queries over the bound, max %.1f times" % (name, over.sum(), len(q), (err2 / bound[:, None]).max()))
    assert over.sum() <= 0.01 * len(q)
    assert (err2 <= np.maximum(bound, 2 * np.sqrt(8 * EPS) * absg + bound)[:, None]).all()


def test_backward_is_zero_on_the_surface_and_for_non_finite_points():
    v, f, _ = dc.meshes()["icosphere2"]
    mesh = HeadMesh(v, f)
    q = np.concatenate([v[:5], dc.nonfinite_queries()[:4], np.array([[2, 0, 0], [0.1, 0.1, 0.1]], np.float32)])
    x = torch.from_numpy(q).requires_grad_(True)
    sd = gm.signed_distance(x, mesh, fused=False)
    sd.backward(torch.ones(len(q)))
    assert bool((x.grad[:9] == 0).all()) and bool(torch.isfinite(x.grad).all())
    sd = sd.detach()
    assert float(sd[9]) > 0 > float(sd[10]) and bool(torch.isinf(sd[5:9]).all())
    assert abs(float(x.grad[9, 0]) - 1.0) < 1e-5                             # outside: away from the mesh grows sd
    g10 = x.grad[10].double()
    assert abs(float(g10.norm()) - 1.0) < 1e-5 and float((g10 * torch.tensor([0.1, 0.1, 0.1]).double()).sum()) > 0  # inside too: outwards grows sd
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.closest_point(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        gm.signed_distance(torch.zeros(4, 3), mesh)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def _strand(xs, y=0.2, z=0.75):
    return [[x, y, z] for x in xs]


def test_split_strands_on_hand_made_strands():
    head = HeadMesh(*mc.meshes()["box"][:2])                                # x 0.1 .. 0.9, y -0.3 .. 0.7, z 0.2 .. 1.3
    L = 8
    # a "scalp": one big triangle in the plane z = 1.4, just above the box
    scalp = HeadMesh(np.array([[-5, -5, 1.4], [5, -5, 1.4], [0, 8, 1.4]], np.float32), np.array([[0, 1, 2]], np.int32))
    strands = np.array([
        _strand([-0.4, -0.3, -0.2, -0.1, 0.0, 0.05, 0.08, 0.09]),            # 0: wholly outside: kept as it is
        _strand([0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.85]),                  # 1: wholly inside: dropped
        [[-0.2, 0.2, 1.35], [-0.1, 0.2, 1.35], [0.0, 0.2, 1.35], [0.5, 0.2, 1.0], [0.5, 0.2, 0.9],   # 2: dips in and out:
         [0.5, 0.2, 1.35], [0.6, 0.2, 1.35], [0.7, 0.2, 1.36]],                                      #    the tail is 0.05 from the scalp
        [[-0.2, 0.2, 0.0], [-0.1, 0.2, 0.0], [0.0, 0.2, 0.0], [0.5, 0.2, 1.0], [0.5, 0.2, 0.9],      # 3: the same, far below the scalp:
         [0.5, 0.2, 0.1], [0.6, 0.2, 0.1], [0.7, 0.2, 0.1]],                                         #    the re-root is refused
        [[0.5, 0.2, 0.5], [-0.2, 0.2, 0.0], [-0.1, 0.2, 0.0], [0.5, 0.2, 0.6], [0.5, 0.2, 1.35],     # 4: root inside (a 0-point first run),
         [0.5, 0.2, 0.7], [-0.3, 0.2, 0.0], [-0.4, 0.2, 0.0]],                                       #    a piece of 1 point + root, tails far
        _strand([0.2, 0.3, 0.4, 0.5, 0.6, -0.1, -0.2, -0.3]),                # 5: fewer than half outside: dropped
    ], np.float32)
    pts = torch.from_numpy(strands)
    pieces, source = bs.split_strands(pts, head, scalp, max_root_dist=0.1, fused=False)
    assert pieces.dtype == torch.float32 and pieces.shape[1:] == (L, 3) and source.dtype == torch.int64
    assert source.tolist() == [0, 2, 2, 3, 4]
    assert not bool(head.contains(pieces, fused=False).any())                # nothing of any piece is inside
    P = pieces.numpy()
    f64 = lambda a: a.astype(np.float64)  # noqa: E731
    assert np.array_equal(P[0], strands[0])
    # strand 2, rooted piece: 3 points -> first segment resampled to L - 3 + 2 = 7 points, then the third point
    want = np.concatenate([np.linspace(f64(strands[2, 0]), f64(strands[2, 1]), 7).astype(np.float32), strands[2, 2:3]])
    assert np.array_equal(P[1], want) and np.array_equal(P[1][0], strands[2, 0]) and np.array_equal(P[1][6], strands[2, 1])
    # strand 2, re-rooted piece: root = the scalp's closest point to (0.5, 0.2, 1.35), then the 3 points of the run
    d2, _, root = scalp.closest_point(torch.from_numpy(strands[2, 5:6]), fused=False)
    root = root.numpy()[0]
    assert abs(float(d2) - 0.0025) < 1e-6 and np.abs(root - np.array([0.5, 0.2, 1.4])).max() < 1e-6
    want = np.concatenate([np.linspace(f64(root), f64(strands[2, 5]), 6).astype(np.float32), strands[2, 6:]])
    assert np.array_equal(P[2], want)
    # strand 3: its tail is 1.3 below the scalp: the re-root is refused, the rooted piece stays
    want = np.concatenate([np.linspace(f64(strands[3, 0]), f64(strands[3, 1]), 7).astype(np.float32), strands[3, 2:3]])
    assert np.array_equal(P[3], want)
    # strand 4: the root is inside; its first run (points 1, 2) does not hold point 0 and is far from the scalp -> dropped; the
    # single point 4 is 0.05 from the scalp: root + 1 point = a piece of 2, resampled to L; the tail (6, 7) is far -> dropped
    want = np.linspace(f64(root), f64(strands[4, 4]), L).astype(np.float32)
    assert np.array_equal(P[4], want)
    # without a scalp only the rooted pieces survive; a larger max_root_dist accepts the far runs too
    p2, s2 = bs.split_strands(pts, head, None, fused=False)
    assert s2.tolist() == [0, 2, 3] and torch.equal(p2, pieces[[0, 1, 3]])
    p3, s3 = bs.split_strands(pts, head, scalp, max_root_dist=2.0, fused=False)
    assert s3.tolist() == [0, 2, 2, 3, 3, 4, 4, 4] and not bool(torch.isnan(p3).any())
    # all roots in ONE query
    calls = []
    real = scalp.closest_point
    scalp.closest_point = lambda *a, **k: (calls.append(tuple(a[0].shape)), real(*a, **k))[1]
    bs.split_strands(pts, head, scalp, fused=False)
    assert calls == [(5, 3)]
    e, se = bs.split_strands(pts[1:2], head, scalp, fused=False)
    assert e.shape == (0, L, 3) and se.shape == (0,)
    # a run of one point that holds point 0 is a piece of 1 point: dropped
    lone = np.array([[[0.0, 0.2, 0.75]] + _strand([0.2, 0.3, 0.4]) + [[-0.1, 0.2, 0.0]] * 4], np.float32)
    e, se = bs.split_strands(torch.from_numpy(lone), head, None, fused=False)
    assert e.shape == (0, L, 3)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def test_head_collision_is_the_mean_squared_penetration():
    v, f, _ = dc.meshes()["icosphere2"]
    mesh = HeadMesh(v, f)
    rng = np.random.default_rng(4)
    pts = torch.from_numpy(rng.uniform(-1.2, 1.2, (6, 9, 3)).astype(np.float32)).requires_grad_(True)
    for margin, stride in ((0.0, 1), (0.25, 1), (0.1, 3)):
        c = HeadCollision(mesh, margin=margin, stride=stride, fused=False)
        taken = pts[:, 1:][:, ::stride]
        assert taken.shape[1] == len(range(1, 9, stride))
        sd = mesh.signed_distance(taken.detach(), fused=False)
        want = torch.clamp(margin - sd, min=0).square().mean()
        got = c(pts)
        assert got.dim() == 0 and torch.equal(got.detach(), want) and float(want) > 0
        (grad,) = torch.autograd.grad(got, pts)
        assert bool((grad[:, 0] == 0).all())                              # the root is left out
        mask = torch.zeros(9, dtype=torch.bool)
        mask[1::stride] = True
        assert bool((grad[:, ~mask] == 0).all()) and float(grad[:, mask].abs().max()) > 0
        assert bool((grad[:, 1:][:, ::stride][sd >= margin] == 0).all())     # points beyond the margin do not pull
    assert float(HeadCollision(mesh, fused=False)(pts[:, :1]).detach()) == 0.0      # no point is taken
    with pytest.raises(ValueError, match="stride"):
        HeadCollision(mesh, stride=0)


def _collision_for(hair, margin=0.0, stride=1):
    """a box over the lower half of the strands' own points: some points are inside, some are not"""
    p = hair._pts.detach().reshape(-1, 3).numpy()
    lo, hi = p.min(0), p.max(0)
    mid = (lo + hi) / 2
    v, f = mc.box(lo - 0.01, [hi[0] + 0.01, mid[1], hi[2] + 0.01])
    return HeadCollision(HeadMesh(v, f), margin=margin, stride=stride, fused=False)


def test_the_training_step_gains_exactly_the_collision_term():
    from tests.test_strand_prior_cpu import _one_step, _scene_with_ground_truth
    opt, head, hair, cam = _scene_with_ground_truth()
    base_loss, base_grad, calls = _one_step(hair, head, cam, opt)
    assert calls == [((), {})] and hair.collision is None and hair.Lpen is None
    # attached with weight 0, or with no weight at all: not evaluated, the parent's loss and gradients bit for bit
    for lam in (None, 0.0):
        opt, head, hair, cam = _scene_with_ground_truth()
        pen = _collision_for(hair)
        seen = []
        hair.attach_collision(lambda pts: (seen.append(1), pen(pts))[1])
        if lam is not None:
            opt.lambda_dpen = lam
        loss, grad, calls = _one_step(hair, head, cam, opt)
        assert calls == [((), {"collision": False})] and not seen and hair.Lpen is None
        assert torch.equal(loss, base_loss) and torch.equal(grad, base_grad)
    # attached: the loss is the base plus lambda_dpen * Lpen, the gradient the sum of the two backward passes
    for margin, stride in ((0.0, 1), (0.02, 2)):
        opt, head, hair, cam = _scene_with_ground_truth()
        opt.lambda_dpen = 0.5
        hair.attach_collision(_collision_for(hair, margin, stride))
        dirs0 = hair._dirs.detach().clone()
        loss, grad, calls = _one_step(hair, head, cam, opt)
        assert calls == [((), {"collision": True})]
        d = dirs0.clone().requires_grad_(True)
        pts = hair.pts_origins + torch.cat([torch.zeros_like(hair.pts_origins), torch.cumsum(d, dim=1)], dim=1)
        Lpen = hair.collision(pts)
        (Lpen * opt.lambda_dpen).backward()
        assert float(Lpen.detach()) > 0 and torch.equal(hair.Lpen.detach(), Lpen.detach())
        assert torch.equal(loss, base_loss + Lpen.detach() * opt.lambda_dpen)
        assert float(d.grad.abs().max()) > 0
        # (float32 addition of the two paths' gradients: the order autograd adds them in is its own)
        tol = 4 * EPS * (base_grad.abs() + d.grad.abs())
        assert bool(((grad - (base_grad + d.grad)).abs() <= tol).all())
    hair.attach_collision(None)
    assert hair.collision is None and hair.Lpen is None


def test_two_views_evaluate_the_collision_term_once():
    import copy
    from tests.test_strand_prior_cpu import _one_step, _scene_with_ground_truth
    opt, head, hair, cam = _scene_with_ground_truth()
    two_base, _, _ = _one_step(hair, head, cam, opt, cams=[cam, copy.copy(cam)])
    opt, head, hair, cam = _scene_with_ground_truth()
    opt.lambda_dpen = 0.5
    hair.attach_collision(_collision_for(hair))
    two, _, calls = _one_step(hair, head, cam, opt, cams=[cam, copy.copy(cam)])
    assert calls == [((), {"collision": True}), ((), {"prior": False})]
    assert abs(float(two) - float(two_base) - 0.5 * float(hair.Lpen)) <= 1e-6 * abs(float(two))


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_launch_nothing():
    L = _lib.lib()
    assert L.ghr_abi_version() == 20 and _lib.ABI_VERSION == 20               # the entries were added without a bump
    v, f, _ = dc.meshes()["cube"]
    h = _lib.MeshTris()
    INV = _lib.GHR_E_INVALID
    bad_f = f.copy(); bad_f[3, 1] = 8
    assert L.ghr_mesh_tris_sizes(8, _p(v), 12, _p(bad_f), ctypes.byref(h)) == INV and b"face index" in L.ghr_last_error()
    bad_v = v.copy(); bad_v[2, 1] = np.inf
    assert L.ghr_mesh_tris_sizes(8, _p(bad_v), 12, _p(f), ctypes.byref(h)) == INV and b"not finite" in L.ghr_last_error()
    assert L.ghr_mesh_tris_sizes(8, _p(v), 0, _p(f), ctypes.byref(h)) == INV and b"F == 0" in L.ghr_last_error()
    assert L.ghr_mesh_tris_sizes(8, _p(v), -1, _p(f), ctypes.byref(h)) == INV
    assert L.ghr_mesh_tris_sizes(-1, _p(v), 12, _p(f), ctypes.byref(h)) == INV
    assert L.ghr_mesh_tris_sizes(8, None, 12, _p(f), ctypes.byref(h)) == INV
    assert L.ghr_mesh_tris_sizes(8, _p(v), 12, None, ctypes.byref(h)) == INV
    assert L.ghr_mesh_tris_sizes(8, _p(v), 12, _p(f), None) == INV
    assert L.ghr_mesh_tris_sizes(8, _p(v), 12, _p(f), ctypes.byref(h)) == _lib.GHR_OK and h.n_blocks == 1 and h.bytes > 0
    blob = np.zeros(int(h.bytes) // 8, np.uint64)
    assert L.ghr_mesh_tris_build(8, _p(v), 12, _p(f), _p(blob), int(h.bytes) - 16) == INV and b"bytes" in L.ghr_last_error()
    assert L.ghr_mesh_tris_build(8, _p(v), 12, _p(f), None, int(h.bytes)) == INV
    assert L.ghr_mesh_tris_build(8, _p(v), 0, _p(f), _p(blob), int(h.bytes)) == INV
    fake = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before a launch
    hb = ctypes.byref(h)
    assert L.ghr_mesh_closest(None, None, fake, 4, fake, fake, fake, fake, fake, fake) == INV
    assert L.ghr_mesh_closest(None, hb, None, 4, fake, fake, fake, fake, fake, fake) == INV
    assert L.ghr_mesh_closest(None, hb, ctypes.c_void_p(4100), 4, fake, fake, fake, fake, fake, fake) == INV
    assert L.ghr_mesh_closest(None, hb, fake, -1, fake, fake, fake, fake, fake, fake) == INV
    assert L.ghr_mesh_closest(None, hb, fake, 2 ** 31, fake, fake, fake, fake, fake, fake) == INV
    for k in range(6):
        args = [fake] * 6
        args[k] = None
        assert L.ghr_mesh_closest(None, hb, fake, 4, *args) == INV, k
    for field, value in (("magic", 0), ("n_faces", 0), ("n_blocks", 2), ("off_keys", h.bytes), ("off_rec", 24), ("bytes", 64)):
        broken = _lib.MeshTris.from_buffer_copy(bytes(h))
        setattr(broken, field, value)
        assert L.ghr_mesh_closest(None, ctypes.byref(broken), fake, 4, fake, fake, fake, fake, fake, fake) == INV, field
    assert L.ghr_mesh_closest(None, hb, fake, 0, None, None, None, None, None, None) == _lib.GHR_OK
    assert L.ghr_mesh_distance_backward(None, -1, fake, fake, fake, fake, fake, fake) == INV
    for k in range(6):
        args = [fake] * 6
        args[k] = None
        assert L.ghr_mesh_distance_backward(None, 4, *args) == INV, k
    assert L.ghr_mesh_distance_backward(None, 0, None, None, None, None, None, None) == _lib.GHR_OK


def test_header_declares_the_entries_and_the_binding_knows_them():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "ghr.h")) as fh:
        text = fh.read()
    assert re.search(r"#define GHR_ABI_VERSION 20\b", text)
    for name in ("ghr_mesh_tris_sizes", "ghr_mesh_tris_build", "ghr_mesh_closest", "ghr_mesh_distance_backward"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert "ghr_meshdist.h" in _lib.HEADERS
    assert "typedef struct ghr_mesh_tris" in text
