"""The strand shape term on the GPU (csrc/ghr_shape.h through the C ABI and gaussianhaircut_amd/strand_shape.py).

 1. Through the C ABI on every case of tests/shape_cases.py: nbr, partial, E and d_dirs equal the host walk
    (tests/hostsim/ghr_hostsim_shape.cpp) bit for bit; a second pass gives the same bits; the outputs lie NaN-filled between guard
    words: every element written, nothing beyond.
 2. Through strand_shape.py: fused=True against fused=False under the bar of shape_cases.py (both against the float64 arbiter); a
    CPU-built StrandShape equals a device-built one in nbr, start and list.
 3. The trainer: two steps under ghr_set_deterministic(1); the gradient the term adds to _dirs and Lshape of every step are held to
    the arbiter on the scene, for the fused and the composed run; in step 1 nothing but _dirs moves; the unattached run equals a
    process that never imported the module, byte for byte.
 4. A term whose tables are on another device raises in Python; a start table that leaves the list is read as empty."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from tests import shape_cases as sc
from tests import shape_sim

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FUSED = SimpleNamespace(debug=False, fused_projection=True)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sc.cases()
IDS = [c["name"] for c in CASES]
GUARD = 64  # words in front of and behind every output
COTANGENTS = sc.COTANGENTS
LAMBDA = 0.5  # opt.lambda_dshape of the trainer runs


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def sim():
    return shape_sim.load()


def _guarded(words, dtype):
    """[GUARD | words | GUARD] on the device: the guards a pattern, the body NaN (float) / 0x7fc00000 (int32)"""
    buf = torch.full((words + 2 * GUARD,), 0x7fc00000, dtype=torch.int32, device=DEV)
    buf[:GUARD] = 0x5a5a5a5a
    buf[GUARD + words:] = 0x5a5a5a5a
    return buf, buf[GUARD:GUARD + words].view(dtype)


def _intact(buf, words):
    g = buf.cpu().numpy()
    body = g[GUARD:GUARD + words]
    return bool((g[:GUARD] == 0x5a5a5a5a).all() and (g[GUARD + words:] == 0x5a5a5a5a).all() and (body != 0x7fc00000).all())


def _ptr(t):
    return t.data_ptr()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_c_abi_equals_the_host_walk_bit_for_bit(sim, index):
    c = CASES[index]
    L = _lib.lib()
    S, n = c["dirs"].shape[:2]
    stream = torch.cuda.current_stream().cuda_stream
    roots, dirs, rest = _dev(c["roots"]), _dev(c["dirs"]), _dev(c["rest"])
    r2 = np.inf if c["radius"] is None else float(np.float32(c["radius"]) * np.float32(c["radius"]))
    want_nbr = shape_sim.neighbours(sim, c["roots"], r2)
    for _ in range(2):
        gbuf, nbr = _guarded(4 * S, torch.int32)
        _lib.check(L.ghr_shape_neighbours(stream, S, _ptr(roots), r2, _ptr(nbr)))
        torch.cuda.synchronize()
        assert _intact(gbuf, 4 * S) and np.array_equal(nbr.cpu().numpy().reshape(S, 4), want_nbr), c["name"]
    table = sc.case_nbr(c)                                                    # the hand-made table where the case has one
    assert c["nbr"] is not None or np.array_equal(table, want_nbr)
    start, lists = sc.model_lists(table)
    M = int((table >= 0).sum())
    nbr_d, start_d = _dev(table), _dev(start)
    list_d = _dev(lists if lists.size else np.zeros(1, np.int32))
    want_partial, want_E = shape_sim.forward(sim, c["dirs"], c["rest"], table)
    for _ in range(2):
        pbuf, partial = _guarded(3 * S, torch.float32)
        ebuf, E = _guarded(3, torch.float32)
        _lib.check(L.ghr_shape_forward(stream, S, n, _ptr(dirs), _ptr(rest), _ptr(nbr_d), M, _ptr(partial), _ptr(E)))
        torch.cuda.synchronize()
        assert _intact(pbuf, 3 * S) and _intact(ebuf, 3)
        assert np.array_equal(_bits(partial).reshape(S, 3), _bits(want_partial)), c["name"]
        assert np.array_equal(_bits(E), _bits(want_E)), (c["name"], E.cpu(), want_E)
    for cot in COTANGENTS:
        want = shape_sim.backward(sim, c["dirs"], c["rest"], table, start, lists, cot)
        dE = _dev(np.array(cot, np.float32))
        for _ in range(2):
            dbuf, d_dirs = _guarded(3 * S * n, torch.float32)
            _lib.check(L.ghr_shape_backward(stream, S, n, _ptr(dirs), _ptr(rest), _ptr(nbr_d), _ptr(start_d), _ptr(list_d), M, _ptr(dE),
                                            _ptr(d_dirs)))
            torch.cuda.synchronize()
            assert _intact(dbuf, 3 * S * n)
            assert np.array_equal(_bits(d_dirs), _bits(want).reshape(-1)), (c["name"], cot)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def _shape_on(case, device, fused):
    from gaussianhaircut_amd import strand_shape as ss
    shape = ss.StrandShape(torch.from_numpy(case["roots"]).to(device), torch.from_numpy(case["dirs"]).to(device), radius=case["radius"],
                           rest=torch.from_numpy(case["rest"]).to(device), fused=fused)
    if case["nbr"] is not None:
        shape.nbr = torch.from_numpy(case["nbr"]).to(device)
        shape.start, shape.list = ss.inverted_lists(shape.nbr)
        shape.M = int((shape.nbr >= 0).sum())
    return shape


def _grad(shape, dirs, cot):
    d = dirs.clone().requires_grad_(True)
    (shape.terms(d) * torch.tensor(cot, dtype=torch.float32, device=d.device)).sum().backward()
    return d.grad.cpu().numpy()


@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_fused_and_composed_agree_under_the_bar_and_the_tables_are_the_cpu_ones(index):
    c = CASES[index]
    fused, composed, cpu = _shape_on(c, DEV, True), _shape_on(c, DEV, False), _shape_on(c, "cpu", False)
    for name in ("nbr", "start", "list"):
        a, b, d = (getattr(s, name) for s in (fused, composed, cpu))
        assert a.dtype == torch.int32 and torch.equal(a.cpu(), d) and torch.equal(b.cpu(), d), (c["name"], name)
    assert fused.M == cpu.M and torch.equal(fused.rest.cpu(), cpu.rest)
    dirs = torch.from_numpy(c["dirs"]).to(DEV)
    for shape, who in ((fused, "fused"), (composed, "composed")):
        E = shape.terms(dirs).cpu().numpy()
        rE, rg = sc.ratios(E, lambda cot: _grad(shape, dirs, cot), index)
        print(c["name"], who, "ratio E %.2f, d_dirs %.2f (bar %.1f)" % (rE, rg, sc.C))
        assert rE <= sc.C and rg <= sc.C, (c["name"], who)
    assert torch.equal(fused(dirs), (fused.weights * fused.terms(dirs)).sum())


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def _scene():
    from tests.test_gpu_strand_prior import _scene as strand_scene
    return strand_scene()


def _steps(attach, n=2, capture=False):
    """n strand training steps; attach: None, or fused True / False of the shape term (the composed term behind ONE autograd node,
    as the fused term is, so that its gradient reaches ``_dirs`` as one summand).  Returns the parameters after each step, the
    term's value in each, and -- with capture -- what the arbiter needs: the gradient that reached ``_dirs`` in each step (a tensor
    hook on the leaf: the sum of that backward's parts, as the optimizer sees it), the directions at the start, rest and nbr."""
    from gaussianhaircut_amd.trainer import strand_training_step
    lib = _lib.lib()
    lib.ghr_set_deterministic(1)
    try:
        opt, bg, head, hair, cam = _scene()
        info = dict(grads=[], dirs0=hair._dirs.detach().cpu().clone())
        if attach is not None:
            from gaussianhaircut_amd.strand_shape import StrandShape
            opt.lambda_dshape = LAMBDA
            rest = torch.linalg.vector_norm(hair._dirs.detach().double(), dim=-1).mean(1) * 0.9   # a term that is not 0 at the start
            shape = StrandShape.from_model(hair, rest=rest, fused=attach)
            info.update(rest=shape.rest.cpu().numpy(), nbr=shape.nbr.cpu().numpy())
            if attach:
                hair.attach_shape(shape)
            else:
                from tests.test_strand_shape_cpu import _OnePath
                hair.attach_shape(lambda dirs: _OnePath.apply(dirs, shape))
        if capture:
            hair._dirs.register_hook(lambda g: info["grads"].append(g.detach().cpu().clone()))
        trace, terms = [], []
        for i in range(n):
            loss = strand_training_step(head, hair, [cam], bg, opt, i + 1, pipe=FUSED)
            assert bool(torch.isfinite(loss))
            trace.append([p.detach().cpu().clone() for p in (hair._dirs, hair._features_dc, hair._features_rest, hair._orient_conf)])
            terms.append(None if attach is None else hair.Lshape.detach().cpu())
        return trace, terms, info
    finally:
        lib.ghr_set_deterministic(0)


def test_training_step_with_the_shape_term_agrees_with_the_arbiter_and_the_composed_term():
    """The gradient that reaches ``_dirs`` in step 1, less the plain run's, is lambda_dshape times the term's gradient: held per
    element to the float64 arbiter on the scene's own directions, rest lengths and neighbours under lambda C 2^-24 mag -- plus
    4 x 2^-24 (|g_plain| + |g_run|) for the float32 additions of the paths into ``_dirs``, in autograd's order, as the CPU wiring
    test allows -- for the fused and for the composed run, and the two against each other under twice that.  A wrong sign or scale,
    a dropped lambda_dshape or weight moves an element by the order of the term's gradient itself.  ``Lshape`` of every step is
    held to the arbiter on the directions that step started from under C 2^-24 sum(mag_E), plus 2 x 2^-24 sum(E) for the float32
    sum of the three weighted means."""
    hip, term_hip, ih = _steps(True, capture=True)
    cmp_, term_cmp, ic = _steps(False, capture=True)
    plain, _, ip = _steps(None, capture=True)
    assert len(ih["grads"]) == len(ic["grads"]) == len(ip["grads"]) == 2          # one summed gradient per step
    assert np.array_equal(ih["nbr"], ic["nbr"]) and np.array_equal(ih["rest"], ic["rest"]) and torch.equal(ih["dirs0"], ip["dirs0"])
    E64, g64, mE, mg = sc.arbiter(ih["dirs0"].numpy(), ih["rest"], ih["nbr"])
    want = LAMBDA * sum(g64)                                                      # weights (1, 1, 1)
    mag = LAMBDA * sum(mg)
    g_plain = ip["grads"][0].double().numpy()
    assert float(np.abs(want).max()) > 100 * float((sc.C * sc.EPS * mag).max())   # the bar is far below the term's gradient
    runs = {}
    for who, info in (("fused", ih), ("composed", ic)):
        g_run = info["grads"][0].double().numpy()
        bar = sc.C * sc.EPS * mag + 4 * sc.EPS * (np.abs(g_plain) + np.abs(g_run))
        err = np.abs((g_run - g_plain) - want)
        print(who, "largest error / bar %.3f" % float((err / bar).max()))
        assert (err <= bar).all(), (who, float((err / bar).max()))
        runs[who] = (g_run, bar)
    assert (np.abs(runs["fused"][0] - runs["composed"][0]) <= runs["fused"][1] + runs["composed"][1]).all()
    for who, trace, terms, info in (("fused", hip, term_hip, ih), ("composed", cmp_, term_cmp, ic)):
        for it in range(2):
            start = info["dirs0"] if it == 0 else trace[it - 1][0]
            E, _, magE, _ = sc.arbiter(start.numpy(), info["rest"], info["nbr"])
            assert float(E.sum()) > 0
            assert abs(float(terms[it]) - float(E.sum())) <= sc.C * sc.EPS * float(magE.sum()) + 2 * sc.EPS * float(E.sum()), (who, it)
    assert not torch.equal(hip[0][0], plain[0][0])     # the term reaches the strand directions
    for k in (1, 2, 3):
        assert torch.equal(hip[0][k], plain[0][k])     # and, in the first step, nothing else
    again, term_again, _ = _steps(True)
    for it in range(2):
        assert torch.equal(term_hip[it], term_again[it])
        for x, y in zip(hip[it], again[it]):
            assert torch.equal(x, y), it               # the same bits every run, with the hook or without


def test_a_term_built_on_another_device_is_refused_in_python():
    from gaussianhaircut_amd import strand_shape as ss
    c = CASES[IDS.index("S5_n63")]
    shape = ss.StrandShape(torch.from_numpy(c["roots"]), torch.from_numpy(c["dirs"]))        # CPU tables, fused=True by default
    with pytest.raises(ValueError, match="device"):
        shape.terms(torch.from_numpy(c["dirs"]).to(DEV))


def test_a_start_table_that_leaves_the_list_is_read_as_empty(sim):
    """start ranges inside 4 S but beyond the list's M entries: the kernel reads nothing of them, as the host walk"""
    c = CASES[IDS.index("radius")]                                                           # M = 12 of 4 S = 24
    L = _lib.lib()
    S, n = c["dirs"].shape[:2]
    nbr = sc.case_nbr(c)
    start, lists = sc.model_lists(nbr)
    M = int((nbr >= 0).sum())
    bad = start.copy()
    bad[-1] = M + 3                                                                          # the last strand's range runs past the list
    assert bad[-1] <= 4 * S
    want = shape_sim.backward(sim, c["dirs"], c["rest"], nbr, bad, lists, (0.0, 0.0, 1.0))
    good = shape_sim.backward(sim, c["dirs"], c["rest"], nbr, start, lists, (0.0, 0.0, 1.0))
    assert not np.array_equal(want[-1], good[-1]) and np.array_equal(want[:-1], good[:-1])
    dbuf, d_dirs = _guarded(3 * S * n, torch.float32)
    args = [_dev(x) for x in (c["dirs"], c["rest"], nbr, bad, lists, np.array([0, 0, 1], np.float32))]
    _lib.check(L.ghr_shape_backward(torch.cuda.current_stream().cuda_stream, S, n, *[_ptr(a) for a in args[:5]], M, _ptr(args[5]),
                                    _ptr(d_dirs)))
    torch.cuda.synchronize()
    assert _intact(dbuf, 3 * S * n) and np.array_equal(_bits(d_dirs), _bits(want).reshape(-1))


def test_unattached_step_equals_a_run_that_never_imported_the_module(tmp_path):
    """The child process runs the same two steps with nothing attached and checks that gaussianhaircut_amd.strand_shape was never
    imported; a process of its own is the only way to have that (this module's other tests import it)."""
    out = str(tmp_path / "plain.pt")
    code = ("import sys, torch\n"
            "from tests import test_gpu_strand_shape as t\n"
            "trace, _, _ = t._steps(None)\n"
            "assert 'gaussianhaircut_amd.strand_shape' not in sys.modules\n"
            "torch.save(trace, sys.argv[1])\n")
    res = subprocess.run([sys.executable, "-c", code, out], cwd=ROOT, capture_output=True, text=True, timeout=300,
                         env={**os.environ, "PYTHONPATH": ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")})
    assert res.returncode == 0, res.stdout + res.stderr
    want = torch.load(out)
    from gaussianhaircut_amd.strand_shape import StrandShape  # noqa: F401  (imported here: it changes nothing)
    got, _, _ = _steps(None)
    for it in range(len(got)):
        for x, y in zip(got[it], want[it]):
            assert torch.equal(x, y), it
