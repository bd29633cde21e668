"""The hair field, the strand trace and the resampling of csrc/ghr_field.h (strand_growing.py) without a GPU.

 1. The host walk of the kernels' loops (tests/hostsim/ghr_hostsim_field.cpp) and the composed form (fused=False, fp32 CPU tensors)
    against the float64 arbiter of tests/field_cases.py under its bar; n exactly.
 2. Trajectories teacher-forced: the arbiter takes the host walk's fp32 (x_j, t_j) of every step, must make the same decision and
    the next point under the bar; from its decisions alone it replays coast, rows and steps, which must equal the walk's exactly.
 3. The resampling's (q, rem) exactly, read back from a path whose points are their own row numbers.
 4. The same query in waves of different company and in permuted order gives the same bits; so does a strand.
 5. The host walk as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer.
 6. The C ABI: symbols, header, HEADERS, ABI 20, the refusal table of tests/golden/field_refusals.json.
 7. HairField.from_model against hand-built rows.   8. create_from_polylines against create_from_strands.
 9. A bundle of helices sampled as a cloud: every kept point of every grown strand within r of a true curve, >= 30 steps each."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd import strand_growing as sg
from tests import field_cases as fc
from tests import field_sim as fs
from tests import helpers as hp


@pytest.fixture(scope="module")
def sim():
    return fs.load()


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def field_of(cloud):
    return sg.HairField(T(cloud["points"]), T(cloud["directions"]), T(cloud["weights"]), T(cloud["colors"]))


def composed_query(cloud, x, t, r2):
    out = sg.field_composed(T(cloud["points"]), T(cloud["directions"]), T(cloud["weights"]), T(cloud["colors"]), T(x), T(t), float(r2))
    return [o.numpy() for o in out]


def field_errors(got, want, cloud):
    """(rho, v, c) errors of an fp32 form in units of rho (c: rho max|f|); asserts n and the exact zeros"""
    rho, v, c, n = want
    g_rho, g_v, g_c, g_n = [np.asarray(a) for a in got[:4]]
    assert g_rho.dtype == np.float32 and g_n.dtype == np.int32
    assert np.array_equal(g_n, n)
    empty = rho == 0
    assert np.all(n[empty] == 0) and not g_rho[empty].any() and not g_v[empty].any() and not g_c[empty].any()
    if empty.all():
        return 0.0, 0.0, 0.0
    s = rho[~empty]
    fmax = float(np.abs(cloud["colors"]).max())
    return (float((np.abs(g_rho[~empty] - s) / s).max()), float((np.abs(g_v[~empty] - v[~empty]) / s[:, None]).max()),
            float((np.abs(g_c[~empty] - c[~empty]) / (s[:, None] * fmax)).max()))


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.ALL_QUERY_CASES)
def test_host_walk_and_composed_form_meet_the_arbiter(sim, name):
    c = fc.query_case(name)
    want = fc.field64(c["cloud"], c["x"], c["t"], c["r2"])
    for who, got in (("host walk", fs.query(sim, c["cloud"], c["x"], c["t"], c["r2"])),
                     ("composed", composed_query(c["cloud"], c["x"], c["t"], c["r2"]))):
        e = field_errors(got, want, c["cloud"])
        print(name, who, "errors / bar:", [x / fc.BAR_FIELD for x in e], "largest n", int(want[3].max()))
        assert max(e) <= fc.BAR_FIELD, (who, e)


def test_the_tie_case_decides_as_stated(sim):
    """a point at exactly r is outside; d . t = 0 counts as +; the sums are exact in fp32 here"""
    c = fc.tie_case()
    rho, v, cc, n, _ = fs.query(sim, c["cloud"], c["x"], c["t"], c["r2"])
    assert n.tolist() == [2, 1, 2]
    k = np.float32(0.5625)   # (1 - 0.25)^2
    assert rho.tolist() == [float(k * 1 + k * np.float32(0.5)), float(k * 2), float(k * 1 + k * np.float32(0.5))]
    assert v[0].tolist() == [float(k * np.float32(0.5)), float(k), 0.0]     # point 3: +(0,1,0); point 4: -(-1,0,0)
    assert v[1].tolist() == [0.0, 0.0, float(k * 2)]                       # -(0,0,-1)
    assert v[2].tolist() == [float(-k * np.float32(0.5)), float(k), 0.0]    # both perpendicular: both +


def test_the_bar_is_four_times_the_composed_forms_measured_error(sim):
    """prints what tests/field_cases.py's docstring records; the constants there are these measurements times 4, rounded up"""
    worst = np.zeros(3)
    for name in fc.ALL_QUERY_CASES:
        c = fc.query_case(name)
        want = fc.field64(c["cloud"], c["x"], c["t"], c["r2"])
        worst = np.maximum(worst, field_errors(composed_query(c["cloud"], c["x"], c["t"], c["r2"]), want, c["cloud"]))
    point = 0.0
    for S, M, coast in ((65, 40, 2), (64, 7, 0)):
        sc, st = _states(sim, S, M, coast)
        point = max(point, _composed_one_step(sc, st)[0])
    print("composed fp32 form, largest errors: rho %.3g v %.3g c %.3g next point %.3g" % (*worst, point))
    assert 4 * worst.max() <= fc.BAR_FIELD and 4 * point <= fc.BAR_POINT
    assert 4 * worst.max() >= 0.5 * fc.BAR_FIELD and 4 * point >= 0.5 * fc.BAR_POINT   # the constants are not stale


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def _trace(sim, scene, M, coast, args=fc.TRACE_ARGS, rorder=None):
    return fs.trace(sim, scene["cloud"], scene["roots"], scene["normals"], M, fc.r2_of(args["r"]), args["h"], args["beta"],
                    args["rho_min"], coast, rorder)


def _states(sim, S, M, coast):
    scene = fc.small_scene(S)
    return scene, _trace(sim, scene, M, coast)


def teacher_forced(scene, got, M, coast, args):
    """item 2 for one trace: -> the largest errors (field in units of the bar's scales, next point in units of h)"""
    path, steps, rgb, log = got
    cloud, S = scene["cloud"], path.shape[0]
    h, beta, rho_min = [float(np.float32(args[k])) for k in ("h", "beta", "rho_min")]
    r2 = fc.r2_of(args["r"])
    fmax = float(np.abs(cloud["colors"]).max())
    live, coast_n, rows, st = np.ones(S, bool), np.zeros(S, int), np.ones(S, int), np.zeros(S, int)
    C, R = np.zeros((S, 3)), np.zeros(S)
    e_field = e_point = 0.0
    assert np.array_equal(path[:, 0], scene["roots"])
    for j in range(M):
        made = ~np.isnan(log[:, j, 13])
        assert np.array_equal(made, live), j                                # the walk asked the field exactly where the replay is live
        if not live.any():
            break
        i = np.nonzero(live)[0]
        x, t = log[i, j, 0:3].astype(np.float64), log[i, j, 3:6].astype(np.float64)
        assert np.array_equal(log[i, j, 0:3], path[i, rows[i] - 1])         # the state is the path's last point
        rho, v, c, _n = fc.field64(cloud, x, t, r2)                         # (asserts the d2 and the d . t margins)
        assert np.all(np.abs(rho - rho_min) >= fc.M_RHO * rho_min), "a state within 1e-4 of rho_min"
        g_rho, g_v, g_c = log[i, j, 6].astype(np.float64), log[i, j, 7:10].astype(np.float64), log[i, j, 10:13].astype(np.float64)
        some = rho > 0
        assert not g_rho[~some].any()
        if some.any():
            e_field = max(e_field, float((np.abs(g_rho - rho)[some] / rho[some]).max()),
                          float((np.abs(g_v - v)[some] / rho[some, None]).max()),
                          float((np.abs(g_c - c)[some] / (rho[some, None] * fmax)).max()))
        sup, tn, xn = fc.step64(x, t, rho, v, h, beta, rho_min)
        assert np.array_equal(sup, log[i, j, 13] == 1), j                   # the same decision
        coast_n[i] = np.where(sup, 0, coast_n[i] + 1)
        stop = coast_n[i] > coast
        assert np.array_equal(stop, log[i, j, 13] == -1), j
        go = i[~stop]
        rows[go] += 1
        e_point = max(e_point, float(np.abs(path[go, rows[go] - 1] - xn[~stop]).max() / h) if go.size else 0.0)
        st[i[sup]] = rows[i[sup]] - 1
        C[i[sup]] += g_c[sup]
        R[i[sup]] += g_rho[sup]
        live[i[stop]] = False
    assert np.array_equal(steps, st)                                        # item 3: steps exactly
    for s in range(S):                                                      # every row written; the tail repeats the last point
        assert not np.isnan(path[s]).any() and np.all(path[s, rows[s]:] == path[s, rows[s] - 1])
    want_rgb = np.where((R == 0)[:, None], 0.0, C / np.where(R == 0, 1.0, R)[:, None])
    assert not rgb[R == 0].any()
    # C and R are fp32 sums of at most M logged terms each: (M - 1) 2^-24 relative apiece, and one division
    assert np.all(np.abs(rgb - want_rgb) <= 2 * M * 2.0 ** -24 * fmax), float(np.abs(rgb - want_rgb).max())
    return e_field, e_point


@pytest.mark.parametrize("coast", fc.TRACE_COAST)
@pytest.mark.parametrize("S", fc.TRACE_S)
def test_trajectories_teacher_forced(sim, S, coast):
    scene = fc.small_scene(S)
    for M in fc.TRACE_M:
        got = _trace(sim, scene, M, coast)
        e_field, e_point = teacher_forced(scene, got, M, coast, fc.TRACE_ARGS)
        print("S %d M %d max_coast %d: steps %d..%d, field %.3g point %.3g of the bar" %
              (S, M, coast, got[1].min(), got[1].max(), e_field / fc.BAR_FIELD, e_point / fc.BAR_POINT))
        assert e_field <= fc.BAR_FIELD and e_point <= fc.BAR_POINT
        if M == 40 and S > 1:
            assert got[1].max() == M                                         # one that stops at M


def _composed_one_step(scene, got, args=fc.TRACE_ARGS):
    """the composed form's step from every state the walk visited (a trace of M = 1) against the arbiter's"""
    log = got[3]
    made = ~np.isnan(log[..., 13])
    x, t = log[made][:, 0:3], log[made][:, 3:6]
    cloud, r2 = scene["cloud"], fc.r2_of(args["r"])
    h, beta, rho_min = [float(np.float32(args[k])) for k in ("h", "beta", "rho_min")]
    fld = field_of(cloud)
    path, steps, _ = sg.trace_composed(lambda a, b: sg.field_composed(fld.points, fld.directions, fld.weights, fld.colors, a, b, float(r2)),
                                       T(x), T(t), 1, h, beta, rho_min, 1)
    rho, v, _c, _n = fc.field64(cloud, x, t, r2)
    t64 = t.astype(np.float64)
    sup, _tn, xn = fc.step64(x.astype(np.float64), t64 / fc.len64(t64)[:, None], rho, v, h, beta, rho_min)
    return float(np.abs(path[:, 1].numpy() - xn).max() / h), np.array_equal(steps.numpy() == 1, sup)


def test_composed_trace_steps_as_the_arbiter_from_the_walks_states(sim):
    scene, got = _states(sim, 65, 40, 2)
    e, same = _composed_one_step(scene, got)
    assert same and e <= fc.BAR_POINT, e


def test_composed_trace_follows_the_host_walk_on_the_gap_cases(sim):
    for name, (coast, k, _gap, _crosses) in fc.GAP_CASES.items():
        scene, a = fc.line_scene(k), fc.LINE_ARGS
        path, steps, rgb, _ = _trace(sim, scene, a["M"], coast, a)
        fld = field_of(scene["cloud"])
        out = sg.grow_strands(fld, T(scene["roots"]), T(scene["normals"]), L=5, radius=a["r"], step=a["h"], max_steps=a["M"],
                              rho_min=a["rho_min"], beta=a["beta"], max_coast=coast, min_steps=0, fused=False)
        assert np.array_equal(out["steps"].numpy(), steps), name
        assert np.abs(out["path"].numpy() - path).max() <= 1e-5 and np.abs(out["rgb"].numpy() - rgb).max() <= 1e-5


@pytest.mark.parametrize("name", sorted(fc.GAP_CASES))
def test_a_strand_coasts_over_max_coast_steps_and_stops_after_one_more(sim, name):
    coast, k, gap, crosses = fc.GAP_CASES[name]
    scene, a = fc.line_scene(k), fc.LINE_ARGS
    got = _trace(sim, scene, a["M"], coast, a)
    teacher_forced(scene, got, a["M"], coast, a)
    flags = got[3][0, :, 13]
    if gap == 0:                                                            # no gap: supported to the last step
        assert np.all(flags == 1) and got[1][0] == a["M"]
        return
    first = int(np.argmax(flags != 1))                                      # the first unsupported step: x = 0.34
    assert first == 17 and np.all(flags[:first] == 1)
    if crosses:
        assert np.all(flags[first:first + gap] == 0) and flags[first + gap] == 1 and got[1][0] > first + gap
        p64, s64, _ = fc.trace64(scene["cloud"], scene["roots"], scene["normals"], a["M"], fc.r2_of(a["r"]), a["h"], a["beta"],
                                 a["rho_min"], coast)
        assert s64[0] == got[1][0] and np.abs(p64 - got[0]).max() < 1e-5
    else:
        assert np.all(flags[first:first + gap - 1] == 0) and flags[first + gap - 1] == -1 and np.isnan(flags[first + gap:]).all()
        assert got[1][0] == first                                           # the coasted points are cut


def test_a_strand_that_never_finds_support_keeps_no_step(sim):
    scene = fc.small_scene(3)
    scene["roots"][1] = (30.0, 30.0, 30.0)
    for coast in fc.TRACE_COAST:
        path, steps, rgb, log = _trace(sim, scene, 7, coast)
        assert steps[1] == 0 and not rgb[1].any() and steps[0] > 0 and steps[2] > 0
        assert (~np.isnan(log[1, :, 13])).sum() == coast + 1                  # coast steps made, stopped at the next
        out = fs.resample(sim, path, steps, 5)
        assert np.all(out[1] == scene["roots"][1])


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", fc.RESAMPLE_L)
def test_resampling_spans_are_the_integers_of_the_definition(sim, L):
    steps = np.array(fc.resample_steps(L), np.int32)
    M = int(steps.max()) + 2
    rows = np.zeros((len(steps), M + 1, 3), np.float32)
    rows[:, :, 0] = np.arange(M + 1)                                        # a point is its own row number
    out = fs.resample(sim, rows, steps, L)
    q, q1, rem = fc.spans(steps, L)
    got_q = np.floor(out[:, :, 0]).astype(np.int64)
    got_rem = np.rint((out[:, :, 0] - got_q) * (L - 1)).astype(np.int64)
    assert np.array_equal(got_q, q) and np.array_equal(got_rem, np.where(q1 > q, rem, 0))
    assert np.all(rem[q1 == q] == 0)                                        # b = a only at the last point (or n = 0)
    g = np.random.default_rng(L)
    path = g.normal(size=(len(steps), M + 1, 3)).astype(np.float32)
    out = fs.resample(sim, path, steps, L)
    want = fc.resample64(path, steps, L)
    assert np.all(np.abs(out - want) <= 8 * 2.0 ** -24 * np.abs(path).max())  # w, b - a (<= 2 max), the product, the sum
    assert np.all(out[0] == path[0, 0]) and np.all(out[:, 0] == path[:, 0])  # steps = 0: L copies of the root
    assert np.array_equal(out[np.arange(len(steps)), -1], path[np.arange(len(steps)), steps])
    comp = sg.resample_strands(T(path), T(steps), L, fused=False).numpy()
    assert np.array_equal(comp.view(np.int32), out.view(np.int32))         # the same expressions elementwise: the same bits


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def _bits(*arrays):
    return [np.ascontiguousarray(a).view(np.int32).copy() for a in arrays]


@pytest.mark.parametrize("name", ["P4097", "Q257", "duplicates"])
def test_a_querys_bits_do_not_depend_on_its_company_or_the_order(sim, name):
    c = fc.query_case(name)
    Q = c["x"].shape[0]
    base = _bits(*fs.query(sim, c["cloud"], c["x"], c["t"], c["r2"])[:4])
    perm = np.random.default_rng(5).permutation(Q)
    for a, b in zip(base, _bits(*fs.query(sim, c["cloud"], c["x"], c["t"], c["r2"], qorder=perm)[:4])):
        assert np.array_equal(a, b)
    for i in (0, Q // 2, Q - 1):                                            # alone in its wave; with far-away company
        alone = _bits(*fs.query(sim, c["cloud"], c["x"][i:i + 1], c["t"][i:i + 1], c["r2"])[:4])
        x2 = np.concatenate([c["x"][i:i + 1], c["x"][i:i + 1] + 40, c["x"][:7]]).astype(np.float32)
        t2 = np.concatenate([c["t"][i:i + 1], c["t"][i:i + 1], c["t"][:7]])
        mixed = _bits(*fs.query(sim, c["cloud"], x2, t2, c["r2"])[:4])
        for a, b, m in zip(base, alone, mixed):
            assert np.array_equal(a[i], b[0]) and np.array_equal(a[i], m[0])


def test_a_strands_bits_do_not_depend_on_the_root_order(sim):
    scene = fc.small_scene(65)
    a = _trace(sim, scene, 40, 2)
    order, _ = fs.key_order(sim, scene["roots"])
    for rorder in (order, np.arange(65)[::-1].copy()):
        b = _trace(sim, scene, 40, 2, rorder=rorder)
        for u, w in zip(a[:3], b[:3]):
            assert np.array_equal(_bits(u)[0], _bits(w)[0])
    sub = dict(scene, roots=scene["roots"][10:11], normals=scene["normals"][10:11])
    c = _trace(sim, sub, 40, 2)
    assert np.array_equal(_bits(c[0])[0][0], _bits(a[0])[0][10]) and c[1][0] == a[1][10]


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_sanitized_stand_alone_program_runs_the_walks_clean():
    san = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    if os.path.basename(hp.host_cxx()) == "g++":
        san += ["-static-libasan", "-static-libubsan"]
    exe = hp.compile_hostsim("ghr_field_selfcheck_san", "ghr_field_selfcheck.cpp", san, ["ghr_hostsim_field.cpp"] + fs.DEPS)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "10 cases ok" in res.stdout and "runtime error" not in res.stderr, res.stdout + res.stderr


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
NAMES = ("ghr_field_workspace_size", "ghr_field_build", "ghr_field_query", "ghr_field_trace", "ghr_strands_resample")
ARGS = {
    "ghr_field_workspace_size": ("P", "bytes"),
    "ghr_field_build": ("stream", "P", "points", "order", "directions", "weights", "colors", "ws"),
    "ghr_field_query": ("stream", "P", "ws", "Q", "x", "t", "query_order", "r2", "rho", "v", "c", "n"),
    "ghr_field_trace": ("stream", "P", "ws", "S", "roots", "normals", "root_order", "M", "r2", "h", "beta", "rho_min", "max_coast", "path",
                        "steps", "rgb"),
    "ghr_strands_resample": ("stream", "S", "M", "L", "path", "steps", "out"),
}
MAY_BE_NULL = {"stream", "query_order", "root_order"}
SCALARS = dict(P=100, Q=10, S=10, M=8, L=5, r2=0.01, h=0.02, beta=0.5, rho_min=0.1, max_coast=2)
X = 0x1000  # stands for a buffer: none of these calls follows a pointer
TABLE = os.path.join(hp.ROOT, "tests", "golden", "field_refusals.json")


def _table():
    """tests/golden/field_refusals.json: calls of the five entry points -- the well-formed argument set above with the fields a
    case changes (null: a NULL pointer; "nan", "inf": those floats) -- and the (return code, ghr_last_error text) each gave when the
    table was recorded"""
    with open(TABLE) as fh:
        return json.load(fh)["cases"]


def call_refused(L, case):
    names = ARGS[case["fn"]]
    a = {k: SCALARS.get(k, None if k == "stream" else X) for k in names}
    assert set(case["set"]) <= set(a), case["id"]
    a.update({k: float(v) if isinstance(v, str) else v for k, v in case["set"].items()})
    if case["fn"] == "ghr_field_workspace_size" and a["bytes"] is not None:
        a["bytes"] = ctypes.byref(ctypes.c_size_t(0))
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
    assert "ghr_field.h" in _lib.HEADERS and os.path.exists(os.path.join(_lib.CSRC, "ghr_field.h"))
    with open(os.path.join(_lib.CSRC, "ghr_capi.hip")) as fh:
        assert '#include "ghr_field.h"' in fh.read()
    with open(os.path.join(_lib.CSRC, "ghr_field.h")) as fh:
        txt = fh.read()
    assert "atomic" not in txt.replace("No floating-point atomics", "") and "asm" not in txt


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
        assert nulls == {k for k in names if k not in SCALARS} - MAY_BE_NULL, (fn, nulls)
        text = " | ".join(c["expect"][1] for c in mine)
        rules = {"P": "P < 1", "Q": "Q < 0", "S": "S < 0", "M": "M < 1", "L": "L < 2", "r2": "r2 must be", "h": "h must be",
                 "beta": "beta must be", "rho_min": "rho_min must be", "max_coast": "max_coast < 0"}
        for k in names:
            if k in rules:
                assert rules[k] in text, (fn, k)
        assert "32-bit" in text, fn
    L = _lib.lib()
    a = dict(fn="ghr_field_query", set=dict(Q=0), id="Q = 0 is no refusal")
    assert call_refused(L, a)[0] == _lib.GHR_OK
    assert call_refused(L, dict(fn="ghr_field_trace", set=dict(S=0), id=""))[0] == _lib.GHR_OK
    assert call_refused(L, dict(fn="ghr_strands_resample", set=dict(S=0), id=""))[0] == _lib.GHR_OK
    b = ctypes.c_size_t(0)
    assert L.ghr_field_workspace_size(1000, ctypes.byref(b)) == _lib.GHR_OK
    lay = 1000 * 16 + 256 - (1000 * 16) % 256
    assert b.value >= 3 * lay and b.value % 256 == 0


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def _stage1_model(P=6):
    from gaussianhaircut_amd.scene.gaussian_model import GaussianModel
    g = torch.Generator().manual_seed(2)
    m = GaussianModel(0)
    m._xyz = torch.rand(P, 3, generator=g)
    m._scaling = torch.log(torch.tensor([[3.0, 1, 2], [1, 4, 2], [1, 2, 5], [2, 1, 1], [1, 1, 3], [1, 2, 1]]))[:P]
    q = torch.randn(P, 4, generator=g)
    m._rotation = q
    m._opacity = torch.randn(P, 1, generator=g)
    m._label = torch.tensor([[2.0], [-2.0], [0.0], [3.0], [-0.1], [1.0]])[:P]    # sigmoid: rows 0, 2 (exactly 0.5), 3, 5 are hair
    m._features_dc = torch.rand(P, 1, 3, generator=g)
    return m


def test_from_model_takes_the_hair_rows_their_longest_axis_opacity_and_colour():
    from gaussianhaircut_amd.utils.general_utils import build_rotation
    m = _stage1_model()
    assert float(m.get_label[2, 0]) == 0.5                                  # sigmoid(0): exactly the threshold, a hair row
    f = sg.HairField.from_model(m)
    rows = [0, 2, 3, 5]
    assert f.P == 4 and torch.equal(f.points, m._xyz[rows])
    R = build_rotation(m._rotation)
    for k, (i, axis) in enumerate(zip(rows, (0, 2, 0, 1))):
        want = R[i, axis] / R[i, axis].norm()
        assert torch.allclose(f.directions[k], want, atol=1e-6) and abs(float(f.directions[k].norm()) - 1) < 1e-6
    assert torch.equal(f.weights, m.get_opacity[rows, 0]) and torch.equal(f.colors, m._features_dc[rows, 0])
    assert sg.HairField.from_model(m, label_threshold=0.9).P == 1              # sigmoid(3) alone
    with pytest.raises(ValueError, match="no Gaussian"):
        sg.HairField.from_model(m, label_threshold=1.5)
    for name in ("_xyz", "_opacity", "_features_dc", "_rotation"):
        bad = _stage1_model()
        getattr(bad, name).view(-1)[0] = float("nan")
        with pytest.raises(ValueError, match="non-finite"):
            sg.HairField.from_model(bad)
    bad = _stage1_model()
    bad._xyz[1, 0] = float("inf")                                           # not a hair row: taken out before the check
    assert sg.HairField.from_model(bad).P == 4


def test_hair_field_checks_its_arguments():
    c = fc.make_cloud(5, "uniform", 1)
    with pytest.raises(ValueError, match="one row per point"):
        sg.HairField(T(c["points"]), T(c["directions"][:4]), T(c["weights"]), T(c["colors"]))
    with pytest.raises(ValueError, match=">= 0"):
        sg.HairField(T(c["points"]), T(c["directions"]), -T(c["weights"]), T(c["colors"]))
    f = field_of(c)
    with pytest.raises(ValueError, match="fused=True"):
        f.query(T(c["points"]), T(c["directions"]), radius=0.5, fused=True)
    with pytest.raises(ValueError, match="radius"):
        f.query(T(c["points"]), T(c["directions"]), radius=0.0)
    scaled = sg.HairField(T(c["points"]), T(c["directions"]) * 3, T(c["weights"]), T(c["colors"]))
    assert torch.allclose(scaled.directions, f.directions, atol=1e-6)


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
def test_create_from_polylines_is_create_from_strands_on_the_differences():
    from gaussianhaircut_amd.scene.gaussian_model_strands import GaussianModelStrands
    g = torch.Generator().manual_seed(4)
    S, L = 5, 7
    pts = torch.cumsum(torch.rand(S, L, 3, generator=g) * 0.01, dim=1)
    rgb = torch.rand(S, 3, generator=g)
    a = GaussianModelStrands(1).create_from_polylines(pts, rgb, spatial_lr_scale=2.0)
    K = 4
    feats = torch.zeros(S * (L - 1), K, 3)
    feats[:, 0] = rgb[:, None, :].expand(S, L - 1, 3).reshape(-1, 3)
    b = GaussianModelStrands(1).create_from_strands(pts[:, :1], pts[:, 1:] - pts[:, :-1], feats, None, 2.0)
    for name in ("pts_origins", "_dirs", "_features_dc", "_features_rest", "_orient_conf", "_xyz", "_rotation", "_scaling"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.spatial_lr_scale == 2.0 and (a.num_strands, a.strand_length) == (S, L)
    assert torch.allclose(a._pts, pts, atol=1e-6) and not a._features_rest.any()
    assert torch.equal(a._features_dc.view(S, L - 1, 3)[:, 3], rgb)
    z = GaussianModelStrands(1).create_from_polylines(pts)
    assert not z._features_dc.any() and z._features_dc.shape == (S * (L - 1), 1, 3)
    with pytest.raises(ValueError):
        GaussianModelStrands(1).create_from_polylines(pts[:, :1])
    with pytest.raises(ValueError):
        GaussianModelStrands(1).create_from_polylines(pts, rgb[:2])


# ---- 9 ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def helix():
    """the scene, the default rho_min and the arbiter's free-running trace"""
    scene = fc.helix_scene()
    rho_min = field_of(scene["cloud"]).default_rho_min(fc.HELIX_R, fused=False)
    return scene, rho_min, fc.trace64(scene["cloud"], scene["roots"], scene["normals"], 400, fc.r2_of(fc.HELIX_R), fc.HELIX_H, 0.5,
                                      rho_min, 4)


def test_the_definition_grows_hair_arbiter(helix):
    scene, _, (path, steps, rgb) = helix
    fc.assert_grown_hair(path, steps, scene["curves"])
    assert rgb.min() >= 0 and rgb.max() <= 1                                # a weighted mean of colours in [0, 1]


def test_the_definition_grows_hair_host_walk(sim, helix):
    scene, rho_min, (p64, s64, _) = helix
    path, steps, rgb, _ = fs.trace(sim, scene["cloud"], scene["roots"], scene["normals"], 400, fc.r2_of(fc.HELIX_R), fc.HELIX_H, 0.5,
                                   rho_min, 4)
    fc.assert_grown_hair(path, steps, scene["curves"])
    ar, end = np.arange(len(steps)), np.minimum(steps, s64)
    print("fp32 and float64 points at the shorter strand's end within %.3g" % np.abs(path[ar, end] - p64[ar, end]).max())
    out = fs.resample(sim, path, steps, 100)
    assert np.all(out[:, 0] == scene["roots"]) and np.array_equal(out[:, -1], path[ar, steps])


def test_grow_strands_composed_on_a_small_scene_keeps_what_the_walk_keeps(sim):
    scene = fc.small_scene(9)
    scene["roots"][4] = (9.0, 9.0, 9.0)
    fld = field_of(scene["cloud"])
    a = fc.TRACE_ARGS
    out = sg.grow_strands(fld, T(scene["roots"]), T(scene["normals"]), L=12, radius=a["r"], step=a["h"], max_steps=40,
                          rho_min=a["rho_min"], max_coast=2, min_steps=8)
    path, steps, rgb, _ = _trace(sim, scene, 40, 2)
    assert np.array_equal(out["steps"].numpy(), steps) and not bool(out["keep"][4]) and int(out["keep"].sum()) == 8
    assert out["points"].shape == (8, 12, 3) and out["rgb"].shape == (8, 3) and out["path"].shape == (9, 41, 3)
    keep = out["keep"].numpy()
    assert np.abs(out["points"].numpy() - fs.resample(sim, path, steps, 12)[keep]).max() <= 1e-5
    d = sg.grow_strands(fld, T(scene["roots"]), T(scene["normals"]), L=12, max_steps=5, min_steps=1)   # the look defaults
    assert d["radius"] > 0 and abs(d["step"] - d["radius"] / 2.5) < 1e-6 and d["rho_min"] > 0
