"""The strand shape term (csrc/ghr_shape.h, gaussianhaircut_amd/strand_shape.py) without a GPU.

 1. the host walk of the kernels (tests/hostsim/ghr_hostsim_shape.cpp, every index checked) against the float64 arbiter of
    tests/shape_cases.py: E per term, d_dirs per element and cotangent, under C * 2^-24 * mag;
 2. the composed float32 form (fused=False on CPU tensors) against the arbiter under the same bar (C is four times ITS largest
    ratio, recorded in shape_cases.py), finite gradients on every planted case;
 3. the neighbour search (host walk and the composed torch form) and the list builder against the numpy model, bit for bit;
 4. the planted dead segments; the default rest length;
 5. the wiring of the training step on CPU tensors;
 6. behaviour in float64: 50 Adam steps on the term alone, each mean falls;
 7. a stand-alone program, plain and with -fsanitize=address,undefined (nothing sanitized is loaded here);
 8. the C ABI: names, header, HEADERS, ABI 20, the refusal table of tests/golden/shape_refusals.json."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd import strand_shape as ss
from tests import helpers as hp
from tests import shape_cases as sc
from tests import shape_sim

CASES = sc.cases()
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def sim():
    return shape_sim.load()


def _shape_of(case, **kw):
    """a StrandShape on CPU tensors over the case's roots, with the case's rest lengths and (where hand-made) its table"""
    shape = ss.StrandShape(torch.from_numpy(case["roots"]), torch.from_numpy(case["dirs"]), radius=case["radius"],
                           rest=torch.from_numpy(case["rest"]), fused=False, **kw)
    if case["nbr"] is not None:
        shape.nbr = torch.from_numpy(case["nbr"])
        shape.start, shape.list = ss.inverted_lists(shape.nbr)
        shape.M = int((shape.nbr >= 0).sum())
    return shape


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_host_walk_against_the_float64_arbiter(sim, index):
    c = CASES[index]
    nbr = sc.case_nbr(c)
    start, lists = sc.model_lists(nbr)
    partial, E = shape_sim.forward(sim, c["dirs"], c["rest"], nbr)
    assert np.isfinite(partial).all() and np.isfinite(E).all()
    rE, rg = sc.ratios(E, lambda cot: shape_sim.backward(sim, c["dirs"], c["rest"], nbr, start, lists, cot), index)
    print(c["name"], "host walk: ratio E %.2f, d_dirs %.2f (bar %.1f)" % (rE, rg, sc.C))
    assert rE <= sc.C and rg <= sc.C


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def _composed_grad(shape, dirs, cot):
    d = torch.from_numpy(dirs).clone().requires_grad_(True)
    (shape.terms(d) * torch.tensor(cot, dtype=torch.float32)).sum().backward()
    return d.grad.numpy()


@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_composed_form_against_the_float64_arbiter(index):
    c = CASES[index]
    shape = _shape_of(c)
    E = shape.terms(torch.from_numpy(c["dirs"])).numpy()
    rE, rg = sc.ratios(E, lambda cot: _composed_grad(shape, c["dirs"], cot), index)
    print(c["name"], "composed: ratio E %.2f, d_dirs %.2f" % (rE, rg))
    assert rE <= sc.C and rg <= sc.C and sc.C == 4 * sc.COMPOSED_RATIO


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def _root_sets():
    sets = [(c["name"], c["roots"], c["radius"]) for c in CASES]
    sets.append(("lattice130_cut", sc.lattice_roots(130), 1.0))
    sets.append(("lattice65", sc.lattice_roots(65), None))
    sets.append(("radius_tiny", sc.radius_roots(), 0.5))
    return sets


@pytest.mark.parametrize("name,roots,radius", _root_sets(), ids=[s[0] for s in _root_sets()])
def test_neighbour_search_and_lists_equal_the_numpy_model(sim, name, roots, radius):
    want = sc.model_neighbours(roots, radius)
    r2 = np.inf if radius is None else np.float32(radius) * np.float32(radius)
    assert np.array_equal(shape_sim.neighbours(sim, roots, r2), want)
    got = ss.nearest_roots(torch.from_numpy(roots), radius, fused=False)
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want)
    start, lists = ss.inverted_lists(got)
    ws, wl = sc.model_lists(want)
    assert start.dtype == torch.int32 and lists.dtype == torch.int32
    assert np.array_equal(start.numpy(), ws) and np.array_equal(lists.numpy(), wl)
    S = roots.shape[0]
    assert ((want == -1) | ((want >= 0) & (want < S) & (want != np.arange(S)[:, None]))).all()
    if S - 1 < 4:
        assert ((want >= 0).sum(1) == S - 1).all()


def test_the_planted_root_sets_are_what_they_claim():
    co = sc.model_neighbours(np.zeros((70, 3), np.float32))
    assert np.array_equal(co[4:], np.tile(np.arange(4), (66, 1))) and co[0].tolist() == [1, 2, 3, 4]
    start, lists = sc.model_lists(co)
    assert start[1] - start[0] == 69 and (np.diff(start) == 0).sum() == 65                  # longer than a wave; most are empty
    counts = (sc.model_neighbours(sc.radius_roots(), 1.5) >= 0).sum(1)
    assert set(counts.tolist()) >= {0, 1, 2, 3}
    lat = sc.model_neighbours(sc.lattice_roots(65))
    assert lat[0].tolist() == [1, 5, 25, 6]                                    # three ties at 1, then the lowest of the ties at 2
    hub = [c for c in CASES if c["name"] == "hub130"][0]["nbr"]
    start, lists = sc.model_lists(hub)
    assert start[1] == 4 * 129 and np.array_equal(lists, np.arange(4, 520, dtype=np.int32))


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_planted_segments_are_dead_at_the_threshold_and_alive_an_ulp_above(sim):
    seen = set()
    for c in CASES:
        alive = sc.alive_mask(c["dirs"], c["rest"])
        ln = sc.f32_len(c["dirs"])
        p = c["planted"]
        seen |= set(p)
        if "zero" in p:
            assert ln[p["zero"]] == 0 and not alive[p["zero"]]
        if "at" in p:
            s, i = p["at"]
            assert ln[s, i] == sc.DEAD * c["rest"][s] and not alive[s, i]
        if "above" in p:
            s, i = p["above"]
            assert ln[s, i] == np.nextafter(sc.DEAD * c["rest"][s], np.float32(np.inf)) and alive[s, i]
    assert seen == {"zero", "at", "above"}
    assert np.float32(sim.ghrsim_shape_dead()) == sc.DEAD == np.float32(ss.DEAD)
    # a pair with a dead member contributes exactly 1 and passes no gradient: two strands, one segment each
    dirs = np.array([[[0.0, 0.0, 0.0]], [[0.0, 0.003, 0.0]]], np.float32)
    rest = np.array([0.003, 0.003], np.float32)
    nbr = np.array([[1, -1, -1, -1], [0, -1, -1, -1]], np.int32)
    partial, E = shape_sim.forward(sim, dirs, rest, nbr)
    assert partial[:, 2].tolist() == [1.0, 1.0] and E[2] == 1.0
    start, lists = sc.model_lists(nbr)
    g = shape_sim.backward(sim, dirs, rest, nbr, start, lists, (0.0, 0.0, 1.0))
    assert not g.any()


def test_a_start_table_that_leaves_the_list_is_read_as_empty(sim):
    """ranges of start inside 4 S but beyond the list's M entries: nothing of them is read (the walk checks every index against M)"""
    c = [c for c in CASES if c["name"] == "radius"][0]
    nbr = sc.case_nbr(c)
    start, lists = sc.model_lists(nbr)
    M, S = int((nbr >= 0).sum()), nbr.shape[0]
    bad = start.copy()
    bad[-1] = M + 3
    assert M < bad[-1] <= 4 * S and start[-1] - start[-2] > 0
    want = shape_sim.backward(sim, c["dirs"], c["rest"], nbr, bad, lists, (0.0, 0.0, 1.0))
    good = shape_sim.backward(sim, c["dirs"], c["rest"], nbr, start, lists, (0.0, 0.0, 1.0))
    assert np.isfinite(want).all() and np.array_equal(want[:-1], good[:-1]) and not np.array_equal(want[-1], good[-1])


def test_dirs_on_another_device_than_the_tables_raise():
    roots, dirs = sc.smooth_groom(5, 7, seed=3)
    shape = ss.StrandShape(torch.from_numpy(roots), torch.from_numpy(dirs))           # fused=True by default, CPU tables
    with pytest.raises(ValueError, match="device"):
        shape.terms(torch.empty(5, 7, 3, device="meta"))
    assert shape.terms(torch.from_numpy(dirs)).shape == (3,)                          # CPU dirs: the composed form


def test_default_rest_is_the_float64_mean_segment_length_rounded_once():
    roots, dirs = sc.smooth_groom(5, 7, seed=3)
    shape = ss.StrandShape(torch.from_numpy(roots), torch.from_numpy(dirs), fused=False)
    assert shape.rest.dtype == torch.float32 and np.array_equal(shape.rest.numpy(), sc.default_rest(dirs))
    assert shape.nbr.shape == (5, 4) and shape.M == 20 and shape.S == 5 and shape.n == 7
    with pytest.raises(ValueError, match="neighbours"):
        ss.StrandShape(torch.from_numpy(roots), torch.from_numpy(dirs), neighbours=3)
    with pytest.raises(ValueError, match="rest"):
        ss.StrandShape(torch.from_numpy(roots), torch.from_numpy(dirs), rest=torch.zeros(5))
    with pytest.raises(ValueError, match="radius"):
        ss.StrandShape(torch.from_numpy(roots), torch.from_numpy(dirs), radius=0.0)
    w = ss.StrandShape(torch.from_numpy(roots), torch.from_numpy(dirs), weights=(2.0, 0.5, 0.25), fused=False)
    d = torch.from_numpy(dirs)
    t = w.terms(d)
    assert t.shape == (3,) and torch.equal(w(d), (torch.tensor([2.0, 0.5, 0.25]) * t).sum())
    hair = type("H", (), {"pts_origins": torch.from_numpy(roots)[:, None], "_dirs": d})()
    assert torch.equal(ss.StrandShape.from_model(hair, fused=False).nbr, shape.nbr)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
class _OnePath(torch.autograd.Function):
    """the composed term behind ONE autograd node, as the fused term is: its gradient reaches ``_dirs`` as one summand, so the
    step's gradient is the base's plus this one and the comparison below needs no bound on the term's own partial sums"""

    @staticmethod
    def forward(ctx, dirs, term):
        with torch.enable_grad():
            d = dirs.detach().clone().requires_grad_(True)
            L = term(d)
            (ctx.g,) = torch.autograd.grad(L, d)
        return L.detach()

    @staticmethod
    def backward(ctx, cot):
        return ctx.g * cot, None


def test_the_training_step_gains_exactly_the_shape_term():
    from tests.test_strand_prior_cpu import _one_step, _scene_with_ground_truth
    opt, head, hair, cam = _scene_with_ground_truth()
    base_loss, base_grad, calls = _one_step(hair, head, cam, opt)
    assert calls == [((), {})] and hair.shape is None and hair.Lshape is None
    # attached with weight 0, or with no weight at all: not evaluated, the parent's loss and gradients bit for bit
    for lam in (None, 0.0):
        opt, head, hair, cam = _scene_with_ground_truth()
        term = ss.StrandShape.from_model(hair, fused=False)
        seen = []
        hair.attach_shape(lambda dirs: (seen.append(1), term(dirs))[1])
        if lam is not None:
            opt.lambda_dshape = lam
        loss, grad, calls = _one_step(hair, head, cam, opt)
        assert calls == [((), {"shape": False})] and not seen and hair.Lshape is None
        assert torch.equal(loss, base_loss) and torch.equal(grad, base_grad)
    # attached: the loss is the base plus lambda_dshape * Lshape, the gradient the sum of the two backward passes
    opt, head, hair, cam = _scene_with_ground_truth()
    opt.lambda_dshape = 0.5
    rest = torch.linalg.vector_norm(hair._dirs.detach().double(), dim=-1).mean(1) * 0.9    # (a term that is not 0 at the start)
    term = ss.StrandShape.from_model(hair, rest=rest, weights=(1.0, 2.0, 0.5), fused=False)
    hair.attach_shape(lambda dirs: _OnePath.apply(dirs, term))
    dirs0 = hair._dirs.detach().clone()
    loss, grad, calls = _one_step(hair, head, cam, opt)
    assert calls == [((), {"shape": True})]
    d = dirs0.clone().requires_grad_(True)
    L = hair.shape(d)
    (L * opt.lambda_dshape).backward()
    assert float(L.detach()) > 0 and torch.equal(hair.Lshape.detach(), L.detach())
    assert torch.equal(loss, base_loss + L.detach() * opt.lambda_dshape)
    assert float(d.grad.abs().max()) > 0
    tol = 4 * sc.EPS * (base_grad.abs() + d.grad.abs())   # (float32 addition of the two paths' gradients, in autograd's order)
    assert bool(((grad - (base_grad + d.grad)).abs() <= tol).all())
    hair.attach_shape(None)
    assert hair.shape is None and hair.Lshape is None
    opt, head, hair2, cam = _scene_with_ground_truth()
    hair2.attach_shape(ss.StrandShape.from_model(hair2, fused=False))
    hair2.attach_shape(None)
    opt.lambda_dshape = 0.5
    loss, grad, calls = _one_step(hair2, head, cam, opt)
    assert calls == [((), {})] and torch.equal(loss, base_loss) and torch.equal(grad, base_grad)


def test_two_views_evaluate_the_shape_term_once():
    import copy
    from tests.test_strand_prior_cpu import _one_step, _scene_with_ground_truth
    opt, head, hair, cam = _scene_with_ground_truth()
    opt.lambda_dshape = 0.5
    term = ss.StrandShape.from_model(hair, fused=False)
    seen = []
    hair.attach_shape(lambda dirs: (seen.append(1), term(dirs))[1])
    _, _, calls = _one_step(hair, head, cam, opt, cams=[cam, copy.copy(cam)])
    assert calls == [((), {"shape": True}), ((), {"prior": False})] and seen == [1]


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_fifty_adam_steps_on_the_term_alone_lower_each_mean():
    roots, dirs = sc.smooth_groom(20, 32, seed=21)
    clean = torch.from_numpy(dirs).double()
    rng = np.random.default_rng(22)
    noisy = (clean + torch.from_numpy(rng.normal(0, 0.0008, dirs.shape))).requires_grad_(True)
    shape = ss.StrandShape(torch.from_numpy(roots), clean, fused=False)                    # the clean groom's rest lengths
    before = shape.terms(noisy).detach()
    o = torch.optim.Adam([noisy], lr=2e-5)
    for _ in range(50):
        o.zero_grad()
        shape(noisy).backward()
        o.step()
    after = shape.terms(noisy).detach()
    assert noisy.dtype == torch.float64 and bool((after < before).all()), (before, after)


def test_smooth_polylines_keeps_the_roots_and_lowers_the_term():
    roots, dirs = sc.smooth_groom(12, 16, seed=31)
    rng = np.random.default_rng(32)
    noisy = torch.from_numpy(dirs + rng.normal(0, 0.0008, dirs.shape).astype(np.float32))
    origins = torch.from_numpy(roots)[:, None]
    pts = torch.cat([origins, origins + torch.cumsum(noisy, 1)], 1)
    out = ss.smooth_polylines(pts, 40, fused=False)
    assert out.shape == pts.shape and torch.equal(out[:, 0], pts[:, 0])
    shape = ss.StrandShape(origins, noisy, fused=False)
    before, after = shape(noisy), shape(out[:, 1:] - out[:, :-1])
    assert float(after) < float(before)
    assert torch.equal(ss.smooth_polylines(pts, 0, fused=False), pts)
    with pytest.raises(ValueError, match="points"):
        ss.smooth_polylines(pts[:, :1], 3)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,out", [(["-O1"], "ghr_shape_selfcheck"),
                                       (["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"],
                                        "ghr_shape_selfcheck_san")], ids=["plain", "sanitized"])
def test_stand_alone_program_walks_the_loops_clean(flags, out):
    if len(flags) > 1 and os.path.basename(hp.host_cxx()) == "g++":
        flags = flags + ["-static-libasan", "-static-libubsan"]
    exe = hp.compile_hostsim(out, "ghr_shape_selfcheck.cpp", flags, ["ghr_hostsim_shape.cpp"] + shape_sim.DEPS)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "2 cases ok" in res.stdout and "runtime error" not in res.stderr, res.stdout + res.stderr


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
NAMES = ("ghr_shape_neighbours", "ghr_shape_forward", "ghr_shape_backward")
ARGS = {
    "ghr_shape_neighbours": ("stream", "S", "roots", "r2", "nbr"),
    "ghr_shape_forward": ("stream", "S", "n", "dirs", "rest", "nbr", "M", "partial", "E"),
    "ghr_shape_backward": ("stream", "S", "n", "dirs", "rest", "nbr", "start", "list", "M", "dE", "d_dirs"),
}
SCALARS = dict(S=10, n=8, M=40, r2=0.01)
X = 0x1000  # stands for a buffer: none of these calls follows a pointer
TABLE = os.path.join(hp.ROOT, "tests", "golden", "shape_refusals.json")


def _table():
    """tests/golden/shape_refusals.json: calls of the three entry points -- the well-formed argument set above with the fields a case
    changes (null: a NULL pointer; "nan", "inf", "-inf": those floats) -- and the (return code, ghr_last_error text) each gave when
    the table was recorded"""
    with open(TABLE) as fh:
        return json.load(fh)["cases"]


def call_refused(L, case):
    names = ARGS[case["fn"]]
    a = {k: SCALARS.get(k, None if k == "stream" else X) for k in names}
    assert set(case["set"]) <= set(a), case["id"]
    a.update({k: float(v) if isinstance(v, str) else v for k, v in case["set"].items()})
    rc = getattr(L, case["fn"])(*[a[k] for k in names])
    return [int(rc), L.ghr_last_error().decode()]


def test_c_abi_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    with open(os.path.join(hp.ROOT, "include", "ghr.h")) as fh:
        hdr = fh.read()
    for n in NAMES:
        assert re.search(r"\bint %s\(" % n, hdr) and n in _lib.EXPORTS and hasattr(L, n) and getattr(L, n).argtypes, n
        assert len(getattr(L, n).argtypes) == len(ARGS[n]), n
    assert L.ghr_abi_version() == 20 == _lib.ABI_VERSION and "#define GHR_ABI_VERSION 20" in hdr
    assert "ghr_shape.h" in _lib.HEADERS and os.path.exists(os.path.join(_lib.CSRC, "ghr_shape.h"))
    with open(os.path.join(_lib.CSRC, "ghr_capi.hip")) as fh:
        assert '#include "ghr_shape.h"' in fh.read()
    with open(os.path.join(_lib.CSRC, "ghr_shape.h")) as fh:
        txt = fh.read()
    assert "atomic" not in txt.replace("no floating-point atomics", "") and "asm" not in txt


@pytest.mark.parametrize("case", _table(), ids=lambda c: c["id"])
def test_c_abi_refusals_launch_nothing(case):
    """every call of the table is refused before the runtime is touched (the pointers are never dereferenced), in the recorded words"""
    got = call_refused(_lib.lib(), case)
    assert got == case["expect"], (case["id"], got)
    assert got[0] == _lib.GHR_E_INVALID and case["fn"] + ":" in got[1]


def test_the_refusal_table_covers_every_rule_and_every_pointer():
    cases = _table()
    assert len({c["id"] for c in cases}) == len(cases)
    for fn, names in ARGS.items():
        mine = [c for c in cases if c["fn"] == fn]
        nulls = {k for c in mine for k, v in c["set"].items() if v is None}
        assert nulls == {k for k in names if k not in SCALARS} - {"stream"}, (fn, nulls)
        text = " | ".join(c["expect"][1] for c in mine)
        rules = {"S": "S < 0", "n": "n < 1", "M": "M < 0", "r2": "r2 must be"}
        for k in names:
            if k in rules:
                assert rules[k] in text, (fn, k)
        assert "32-bit" in text, fn
    L = _lib.lib()
    for fn in NAMES:
        assert call_refused(L, dict(fn=fn, set=dict(S=0, M=0) if "M" in ARGS[fn] else dict(S=0), id=""))[0] == _lib.GHR_OK
    # +inf is no refusal of the radius: with S == 0 the call then does nothing
    assert call_refused(L, dict(fn="ghr_shape_neighbours", set=dict(S=0, r2="inf"), id=""))[0] == _lib.GHR_OK
