"""The guarded trace of csrc/ghr_grow.h (strand_growing.py) without a GPU.

 1. The host walk of the kernel's loop (tests/hostsim/ghr_hostsim_grow.cpp, over the headers' own GHR_HD functions) against the
    float64 arbiter of tests/grow_cases.py, teacher-forced: every decision, steps, contacts and stop exactly, a next point and a
    heading under the bar.  The composed form (fused=False, fp32 CPU tensors) one step from every state the walk visited, alike.
 2. The bar re-measured: the constants of tests/grow_cases.py are the composed form's largest errors times 4.
 3. Company, root order and the mesh search's seed block change no bit; a strand that never touches the mesh equals the unguarded
    trace bit for bit; avoid=False is the call without the new arguments, bit for bit and key for key.
 4. The C ABI: symbol, header, HEADERS, ABI 20, the refusal table of tests/golden/grow_refusals.json.
 5. The host walk as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer.
 6. The scene that fails without the feature: hair that lies on a head, grown with and without avoid."""
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
from tests import grow_cases as gc
from tests import grow_sim as gs
from tests import helpers as hp


@pytest.fixture(scope="module")
def sim():
    return gs.load()


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def field_of(cloud):
    return sg.HairField(T(cloud["points"]), T(cloud["directions"]), T(cloud["weights"]), T(cloud["colors"]))


def walk(sim, c, **kw):
    return gs.trace(sim, c["cloud"], gc.head_mesh(c["mesh_name"]), kw.pop("roots", c["roots"]), kw.pop("normals", c["normals"]),
                    kw.pop("M", c["M"]), fc.r2_of(c["r"]), c["h"], c["beta"], c["rho_min"], c["max_coast"], c["margin"], **kw)


_walks = {}


def walked(sim, name):
    """the host walk of a case, once per process, read-only"""
    if name not in _walks:
        _walks[name] = walk(sim, gc.case(name))
        for a in _walks[name]:
            a.setflags(write=False)
    return _walks[name]


def _bits(*arrays):
    return [np.ascontiguousarray(a).view(np.int32 if a.dtype.itemsize == 4 else np.uint8).copy() for a in arrays]


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.ALL_CASES)
def test_host_walk_meets_the_arbiter_teacher_forced(sim, name):
    c, got = gc.case(name), walked(sim, name)
    e_point, e_head = gc.check_trace(c, got)
    out = got[5][..., 25]
    print(name, "steps %d..%d, contacts %d..%d, stops %s, outcomes %s; point %.3g heading %.3g of the bar" %
          (got[1].min(), got[1].max(), got[3].min(), got[3].max(), np.bincount(got[4], minlength=3).tolist(),
           np.bincount(out[~np.isnan(out)].astype(int), minlength=4).tolist(), e_point / gc.BAR_PUSH, e_head / gc.BAR_HEADING))
    assert e_point <= gc.BAR_PUSH and e_head <= gc.BAR_HEADING


def test_the_planted_strands_do_what_they_were_planted_for(sim):
    path, steps, rgb, contacts, stop, log = walked(sim, "planted_cube")
    out = log[..., 25]
    assert out[0, :2].tolist() == [gc.ON_SURFACE, gc.HEAD_ON] and stop[0] == gc.STOP_HEADON and contacts[0] == 1
    assert path[0, 1].tolist() == [0.375, 0.625, 1.0] and np.all(path[0, 2:] == path[0, 1])      # d2 == 0: x = y, then no point
    assert out[1, 0] == gc.HEAD_ON and stop[1] == gc.STOP_HEADON and contacts[1] == 0 and np.all(path[1] == path[1, 0])
    assert out[2, :2].tolist() == [gc.PUSHED, gc.FREE] and path[2, 1].tolist() == [0.4375, 0.625, 1.125]      # tn == 0: t unchanged
    assert log[2, 0, 26:29].tolist() == [1.0, 0.0, 0.0] and path[2, 2].tolist() == [0.5, 0.625, 1.125]        # sd == m: free
    assert out[3, :2].tolist() == [gc.FREE, gc.FREE] and out[6, :2].tolist() == [gc.FREE, gc.FREE]
    assert out[4, :2].tolist() == [gc.PUSHED, gc.FREE] and log[4, 0, 26:29].tolist() == [1.0, 0.0, 0.0] and path[4, 1, 2] == 1.125
    assert out[5, 0] == gc.PUSHED and log[5, 0, 24] == 1 and path[5, 1, 2] == 1.125                            # it was inside
    assert stop[[2, 3, 4, 5, 6]].tolist() == [gc.STOP_COAST] * 5 and not steps.any()                           # nothing supported
    assert contacts.tolist() == [1, 0, 1, 0, 1, 1, 0]


def test_the_mixed_wave_holds_every_kind_of_strand(sim):
    path, steps, rgb, contacts, stop, log = walked(sim, "mixed")
    out, sup = log[..., 25], log[..., 13]
    assert set(np.unique(stop)) == {gc.STOP_STEPS, gc.STOP_COAST, gc.STOP_HEADON}
    assert stop[5] == gc.STOP_COAST and steps[5] == 0 and np.all(sup[5, :2] == 0) and sup[5, 2] == -1      # coasts, then stops
    assert stop[11] == gc.STOP_HEADON and out[9, 0] == gc.FREE and contacts.max() == gc.case("mixed")["M"]
    j = 1                                                                   # one step of the wave with all four at once
    assert {gc.FREE, gc.PUSHED} <= set(out[:, j][~np.isnan(out[:, j])]) and sup[5, j] == 0 and np.isnan(sup[11, j])


def _states(sim, name):
    """every state of a case's walk from which a guarded step was made: x, t, and the walk's log rows"""
    log = walked(sim, name)[5]
    made = ~np.isnan(log[..., 25])
    return log[made]


_composed = {}


def _composed_one_step(sim, name):
    """the composed form's step from every state the walk visited (a trace of M = 1) against the arbiter's -> point error (of h),
    heading error (of 1); computed once per case and process"""
    if name not in _composed:
        _composed[name] = _composed_errors(sim, name)
    return _composed[name]


def _composed_errors(sim, name):
    c, rows = gc.case(name), _states(sim, name)
    x, t = rows[:, 0:3], rows[:, 3:6]
    cloud, r2 = c["cloud"], fc.r2_of(c["r"])
    h, beta, rho_min, m = [float(np.float32(c[k])) for k in ("h", "beta", "rho_min", "margin")]
    fld = field_of(cloud)
    path, steps, _rgb, contacts, stop, t2 = sg.trace_guarded_composed(
        lambda a, b: sg.field_composed(fld.points, fld.directions, fld.weights, fld.colors, a, b, float(r2)), gc.head_mesh(c["mesh_name"]),
        T(x), T(t), 1, h, beta, rho_min, 1, m, headings=True)
    rho, v, _c, _n = fc.field64(cloud, x, t, r2)
    t64 = t.astype(np.float64)
    sup, tn, y = fc.step64(x.astype(np.float64), t64 / fc.len64(t64)[:, None], rho, v, h, beta, rho_min)
    outcome, want_t, want_x, _inn = gc.guard64(*c["mesh"], tn, y, rows[:, 21:24], m, ties=c.get("ties", False))
    assert np.array_equal(outcome, rows[:, 25].astype(int))
    ho = outcome == gc.HEAD_ON
    assert np.array_equal(stop.numpy() == gc.STOP_HEADON, ho) and np.array_equal(steps.numpy() == 1, sup & ~ho)
    assert np.array_equal(contacts.numpy() == 1, (outcome == gc.PUSHED) | (outcome == gc.ON_SURFACE))
    go = ~ho
    return (float(np.abs(path[:, 1].numpy()[go] - want_x[go]).max() / h), float(np.abs(t2.numpy()[go] - want_t[go]).max()))


@pytest.mark.parametrize("name", gc.ALL_CASES)
def test_composed_form_steps_as_the_arbiter_from_the_walks_states(sim, name):
    e_point, e_head = _composed_one_step(sim, name)
    print(name, "composed: point %.3g heading %.3g of the bar" % (e_point / gc.BAR_PUSH, e_head / gc.BAR_HEADING))
    assert e_point <= gc.BAR_PUSH and e_head <= gc.BAR_HEADING


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def test_the_bar_is_four_times_the_composed_forms_measured_error(sim):
    """prints what tests/grow_cases.py's docstring records; its constants are these measurements times 4: not below the
    measurement, not more than 8 times above it"""
    e = np.array([_composed_one_step(sim, name) for name in gc.ALL_CASES])
    point, head = e.max(0)
    print("composed fp32 form, largest errors: next point %.3g of h, heading %.3g" % (point, head))
    assert point <= gc.BAR_PUSH <= 8 * point and head <= gc.BAR_HEADING <= 8 * head


def test_composed_trace_follows_the_host_walk(sim):
    """free-running through grow_strands: the same steps, contacts and stops, the paths within 1e-4 (twenty steps of a bar each)"""
    for name in ("planted_cube", "mixed"):
        c = gc.case(name)
        path, steps, rgb, contacts, stop, _ = walked(sim, name)
        out = sg.grow_strands(field_of(c["cloud"]), T(c["roots"]), T(c["normals"]), L=5, radius=c["r"], step=c["h"], max_steps=c["M"],
                              rho_min=c["rho_min"], beta=c["beta"], max_coast=c["max_coast"], min_steps=0, fused=False,
                              mesh=gc.head_mesh(c["mesh_name"]), avoid=True, margin=c["margin"])
        assert np.array_equal(out["steps"].numpy(), steps) and np.array_equal(out["contacts"].numpy(), contacts), name
        assert np.array_equal(out["stop"].numpy(), stop) and out["stop"].dtype == torch.uint8 and out["contacts"].dtype == torch.int32
        assert np.abs(out["path"].numpy() - path).max() <= 1e-4 and out["margin"] == float(np.float32(c["margin"]))


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def test_a_strands_bits_do_not_depend_on_company_root_order_or_seed_block(sim):
    c = gc.case("mixed")
    S = c["roots"].shape[0]
    a = walked(sim, "mixed")
    order, _ = fs.key_order(sim, c["roots"])
    for kw in (dict(rorder=order), dict(rorder=np.arange(S)[::-1].copy()), dict(seed=0), dict(seed=7), dict(seed=19, rorder=order)):
        b = walk(sim, c, **kw)
        for u, w in zip(_bits(*a[:5]), _bits(*b[:5])):
            assert np.array_equal(u, w), kw
    for i in (0, 5, 11, 40):                                                # alone in its wave
        b = walk(sim, c, roots=c["roots"][i:i + 1], normals=c["normals"][i:i + 1])
        for u, w in zip(_bits(*a[:5]), _bits(*b[:5])):
            assert np.array_equal(u[i], w[0]), i
    c4 = gc.case("ico4")                                                    # two superblocks of faces: the rotation starts in either
    a4 = walked(sim, "ico4")
    for seed in (0, 63, 64, 79):
        for u, w in zip(_bits(*a4[:5]), _bits(*walk(sim, c4, seed=seed)[:5])):
            assert np.array_equal(u, w), seed


def test_a_strand_that_never_touches_the_mesh_is_the_unguarded_strand(sim):
    """field_strand_step keeps its own copy of the heading update (csrc/ghr_field.h): the two must agree in every bit"""
    c = gc.case("free")
    path, steps, rgb, contacts, stop, log = walked(sim, "free")
    p0, s0, rgb0, _ = fs.trace(sim, c["cloud"], c["roots"], c["normals"], c["M"], fc.r2_of(c["r"]), c["h"], c["beta"], c["rho_min"],
                               c["max_coast"])
    for u, w in zip(_bits(path, steps, rgb), _bits(p0, s0, rgb0)):
        assert np.array_equal(u, w)
    assert not contacts.any() and set(np.unique(stop)) <= {gc.STOP_STEPS, gc.STOP_COAST} and (stop == gc.STOP_STEPS).any()
    assert np.array_equal(stop == gc.STOP_STEPS, ~np.isnan(log[:, -1, 25]))   # ran out of M: made the last step


def test_avoid_false_is_the_call_without_the_new_arguments():
    c = gc.case("mixed")
    fld, mesh = field_of(c["cloud"]), gc.head_mesh(c["mesh_name"])
    kw = dict(L=7, radius=c["r"], step=c["h"], max_steps=c["M"], rho_min=c["rho_min"], max_coast=c["max_coast"], min_steps=2)
    for m in (None, mesh):
        a = sg.grow_strands(fld, T(c["roots"]), T(c["normals"]), mesh=m, **kw)
        b = sg.grow_strands(fld, T(c["roots"]), T(c["normals"]), mesh=m, avoid=False, margin=None, **kw)
        assert sorted(a) == sorted(b) == sorted(["points", "keep", "steps", "rgb", "path", "radius", "step", "rho_min"])
        for k in a:
            assert torch.equal(a[k], b[k]) if isinstance(a[k], torch.Tensor) else a[k] == b[k], k
    with pytest.raises(ValueError, match="needs mesh"):
        sg.grow_strands(fld, T(c["roots"]), T(c["normals"]), avoid=True, **kw)
    with pytest.raises(ValueError, match="avoid=True"):
        sg.grow_strands(fld, T(c["roots"]), T(c["normals"]), mesh=mesh, margin=0.1, **kw)
    with pytest.raises(ValueError, match="margin"):
        sg.grow_strands(fld, T(c["roots"]), T(c["normals"]), mesh=mesh, avoid=True, margin=0.0, **kw)
    g = sg.grow_strands(fld, T(c["roots"]), T(c["normals"]), mesh=mesh, avoid=True, **kw)
    assert g["margin"] == g["step"] and sorted(set(g) - set(a)) == ["contacts", "margin", "stop"]       # margin=None: the step


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
FN = "ghr_field_trace_guarded"
ARGS = ("stream", "P", "ws", "tris_header", "tris_dev", "grid_header", "grid_dev", "S", "roots", "normals", "root_order", "M", "r2", "h",
        "beta", "rho_min", "max_coast", "margin", "path", "steps", "rgb", "contacts", "stop")
MAY_BE_NULL = {"stream", "root_order"}
SCALARS = dict(P=100, S=10, M=8, r2=0.01, h=0.02, beta=0.5, rho_min=0.1, max_coast=2, margin=0.02)
X = 0x1000  # stands for a buffer: none of these calls follows a pointer
TABLE = os.path.join(hp.ROOT, "tests", "golden", "grow_refusals.json")


def _table():
    """tests/golden/grow_refusals.json: calls of the entry point -- the well-formed argument set with the fields a case changes (null:
    a NULL pointer; "nan", "inf": those floats; "bad_magic": a header of the other kind) -- and the (return code, ghr_last_error
    text) each gave when the table was recorded"""
    with open(TABLE) as fh:
        return json.load(fh)["cases"]


def _headers():
    mesh = gc.head_mesh("cube")
    mesh.tris_blob()
    return mesh._tris_header, mesh.header


def call_refused(L, case):
    tris, grid = _headers()
    a = {k: SCALARS.get(k, None if k == "stream" else X) for k in ARGS}
    a["tris_header"], a["grid_header"] = ctypes.byref(tris), ctypes.byref(grid)
    assert set(case["set"]) <= set(a), case["id"]
    keep = []
    for k, v in case["set"].items():
        if v == "bad_magic":                                               # the other blob's header: a header, of the wrong kind
            wrong = (_lib.MeshTris if k == "tris_header" else _lib.MeshGrid)()
            ctypes.memmove(ctypes.byref(wrong), ctypes.byref(tris if k == "tris_header" else grid), ctypes.sizeof(wrong))
            wrong.magic = grid.magic if k == "tris_header" else tris.magic
            keep.append(wrong)
            a[k] = ctypes.byref(wrong)
        else:
            a[k] = float(v) if isinstance(v, str) else v
    rc = getattr(L, FN)(*[a[k] for k in ARGS])
    return [int(rc), L.ghr_last_error().decode()]


def test_c_abi_symbol_is_declared_exported_and_bound():
    L = _lib.lib()
    with open(os.path.join(hp.ROOT, "include", "ghr.h")) as fh:
        hdr = fh.read()
    assert re.search(r"\bint %s\(" % FN, hdr) and FN in _lib.EXPORTS and len(getattr(L, FN).argtypes) == len(ARGS)
    decl = hdr[hdr.index("int %s(" % FN):]
    decl = decl[:decl.index(";")]
    assert [w for w in re.findall(r"(\w+)\s*[,)]", decl)] == [k for k in ARGS]                       # the issue's parameter list
    assert L.ghr_abi_version() == 20 == _lib.ABI_VERSION and "#define GHR_ABI_VERSION 20" in hdr
    assert "ghr_grow.h" in _lib.HEADERS and os.path.exists(os.path.join(_lib.CSRC, "ghr_grow.h"))
    with open(os.path.join(_lib.CSRC, "ghr_capi.hip")) as fh:
        assert '#include "ghr_grow.h"' in fh.read()
    with open(os.path.join(_lib.CSRC, "ghr_grow.h")) as fh:
        txt = fh.read()
    assert "atomic" not in txt.replace("floating-point atomics", "") and "asm" not in txt
    assert "k_grow_guarded" in txt and "GrowArgs" in txt and "grow_guard_step" in txt


@pytest.mark.parametrize("case", _table(), ids=lambda c: c["id"])
def test_c_abi_refusals_launch_nothing(case):
    """every call of the table is refused before the runtime is touched (the pointers are never dereferenced), in the recorded words"""
    got = call_refused(_lib.lib(), case)
    assert got == case["expect"], (case["id"], got)
    assert got[0] == _lib.GHR_E_INVALID and FN + ":" in got[1]


def test_the_refusal_table_covers_every_rule_and_every_pointer():
    cases = _table()
    assert len({c["id"] for c in cases}) == len(cases)
    nulls = {k for c in cases for k, v in c["set"].items() if v is None}
    assert nulls == {k for k in ARGS if k not in SCALARS} - MAY_BE_NULL, nulls
    text = " | ".join(c["expect"][1] for c in cases)
    for rule in ("P < 1", "S < 0", "M < 1", "r2 must be", "h must be", "beta must be", "rho_min must be", "max_coast < 0", "32-bit",
                 "margin must be", "triangle-blob header (magic)", "grid header (magic)"):
        assert rule in text, rule
    margins = {c["set"]["margin"] for c in cases if "margin" in c["set"]}
    assert {0, "nan", "inf"} <= margins and any(isinstance(m, float) and m < 0 for m in margins)
    # everything ghr_field_trace refuses, in its words: the shared rules of tests/golden/field_refusals.json
    with open(os.path.join(hp.ROOT, "tests", "golden", "field_refusals.json")) as fh:
        theirs = [c for c in json.load(fh)["cases"] if c["fn"] == "ghr_field_trace"]
    L = _lib.lib()
    for c in theirs:
        got = call_refused(L, dict(c, fn=FN))
        assert got == [c["expect"][0], c["expect"][1].replace("ghr_field_trace:", FN + ":")], c["id"]
    assert call_refused(L, dict(set=dict(S=0), id="S = 0 is no refusal"))[0] == _lib.GHR_OK


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_sanitized_stand_alone_program_runs_the_walk_clean():
    san = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    if os.path.basename(hp.host_cxx()) == "g++":
        san += ["-static-libasan", "-static-libubsan"]
    exe = hp.compile_hostsim("ghr_grow_selfcheck_san", "ghr_grow_selfcheck.cpp", san, ["ghr_hostsim_grow.cpp"] + gs.DEPS)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "4 cases ok" in res.stdout and "runtime error" not in res.stderr, res.stdout + res.stderr


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def assert_the_head_is_avoided(scene, plain, guarded):
    """the assertions of the scene that fails without the feature, for a grown pair (also tests/test_gpu_grow_guarded.py's).
    Measured on the CPU (composed, S = 65, the F = 1280 icosphere): unguarded 1 of 65 kept, median 10 steps; guarded 65 of 65
    kept, median 133 steps (13.3 x), smallest float64 sd of a kept point m (1 - 3.4e-6) -- m = 0.024 added to a point at 1 is
    rounded by 6e-8 = 2.5e-6 m --, 100 .. 134 contact steps per strand, 58 strands coasted out at the cloud's lower end, 7 ran
    out of M, no head-on stop.  (The issue's numpy model on the analytic sphere: 0 % and 100 % kept, 12 x.)"""
    S = scene["roots"].shape[0]
    kept0, kept1 = int(plain["keep"].sum()), int(guarded["keep"].sum())
    med0, med1 = float(np.median(plain["steps"].cpu().numpy())), float(np.median(guarded["steps"].cpu().numpy()))
    m = guarded["margin"]
    v, f = scene["mesh"]
    steps, keep, path = guarded["steps"].cpu().numpy(), guarded["keep"].cpu().numpy(), guarded["path"].cpu().numpy().astype(np.float64)
    pts = np.concatenate([path[s, 1:steps[s] + 1] for s in range(S) if keep[s]])     # (the root is the scalp's: on the surface)
    d, _ = gc.closest64(v, f, pts)
    sd = np.where(gc.inside64(v, f, pts), -d, d)
    print("unguarded: %d of %d kept, median steps %g; guarded: %d kept, median steps %g, smallest sd / m %.9f, contacts %d..%d, stops %s" %
          (kept0, S, med0, kept1, med1, sd.min() / m, guarded["contacts"].min(), guarded["contacts"].max(),
           np.bincount(guarded["stop"].cpu().numpy(), minlength=3).tolist()))
    assert 2 * kept0 < S                                                    # without the guard the head eats the strands
    assert 10 * kept1 >= 9 * S
    assert sd.min() >= m * (1 - 1e-5)
    assert med1 >= 5 * med0


def grow_pair(scene, field, mesh, T_, **kw):
    kw = dict(dict(L=50, radius=scene["r"], step=scene["h"], max_steps=scene["M"], rho_min=0.2, min_steps=8, mesh=mesh), **kw)
    plain = sg.grow_strands(field, T_(scene["roots"]), T_(scene["normals"]), **kw)
    guarded = sg.grow_strands(field, T_(scene["roots"]), T_(scene["normals"]), avoid=True, **kw)
    return plain, guarded


def test_hair_that_lies_on_the_head_grows_around_it_only_with_avoid():
    scene = gc.head_scene()
    plain, guarded = grow_pair(scene, field_of(scene["cloud"]), gc.head_mesh(scene["mesh_name"]), T, fused=False)
    assert guarded["margin"] == guarded["step"]
    assert_the_head_is_avoided(scene, plain, guarded)
