"""Groom upsampling (csrc/ghr_upsample.h, gaussianhaircut_amd/strand_upsampling.py) without a GPU.

 1. the neighbour search: host walk (tests/hostsim/ghr_hostsim_upsample.cpp, every index checked), the composed torch form and the
    numpy float32 model of tests/upsample_cases.py give the same nbr and the same nd2 bits; the planted lattice sets are what they
    claim;
 2. the blend: host walk and composed form (fused=False on CPU tensors) against the float64 arbiter under the derived per-element
    bound of upsample_cases.py; valid equal exactly; out[:, 0] == co bit for bit;
 3. the bound is not vacuous: each planted error exceeds it on every case it applies to;
 4. entries of nbr outside [0, G) end a child's list (host walk only); a child on a guide's root with that guide alone in reach
    reproduces the guide turned into the child's frame; permuting the children permutes the outputs bit for bit;
 5. the Python front: defaults, refusals, frames_at, frames_from_normals, create_from_polylines, the tool's `upsample` step;
 6. a stand-alone program, plain and with -fsanitize=address,undefined (nothing sanitized is loaded here);
 7. the C ABI: names, header, HEADERS, ABI 20, the refusals -- through the real library, before the runtime is touched."""
import importlib.util
import os
import pickle
import re
import subprocess

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd import strand_upsampling as su
from tests import helpers as hp
from tests import mesh_cases as mc
from tests import upsample_cases as uc
from tests import upsample_sim

CASES = uc.cases()
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def sim():
    return upsample_sim.load()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _composed(c, **kw):
    out = su.upsample_strands(_t(c["gp"]), _t(c["gM"]), _t(c["co"]), _t(c["cM"]), features=_t(c["gf"]), radius=c["radius"],
                              eps2=c["eps2"], tau=c["tau"], fused=False, **kw)
    return {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _walk(sim, c, nbr, nd2):
    return upsample_sim.blend(sim, c["gp"], c["gM"], c["gf"], c["co"], c["cM"], nbr, nd2, c["eps2"], c["tau"])


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_neighbours_of_walk_composed_form_and_numpy_model_are_equal(sim, index):
    c = CASES[index]
    want, want_d = uc.neighbours_of(index)
    roots = np.ascontiguousarray(c["gp"][:, 0])
    got, got_d = upsample_sim.near(sim, roots, c["co"], uc.r2_of(c["radius"]))
    assert np.array_equal(got, want) and np.array_equal(_bits(got_d), _bits(want_d))
    tn, td = su.guide_neighbours(_t(roots), _t(c["co"]), c["radius"], fused=False)
    assert tn.dtype == torch.int32 and td.dtype == torch.float32
    assert np.array_equal(tn.numpy(), want) and np.array_equal(_bits(td.numpy()), _bits(want_d))
    G = roots.shape[0]
    assert ((want == -1) | ((want >= 0) & (want < G))).all() and np.isinf(want_d[want < 0]).all()
    if c["radius"] is None:
        assert ((want >= 0).sum(1) == min(G, 4)).all()


def test_the_planted_root_sets_are_what_they_claim():
    nbr, nd2 = uc.neighbours_of(IDS.index("lattice"))
    assert nbr[0].tolist() == [0, 1, 2, 3] and nd2[0].tolist() == [1.0] * 4           # five ties: the four lowest indices
    assert nbr[1, 0] == 0 and nd2[1, 0] == 0.0                                          # a child on a guide's root
    assert nbr[2].tolist() == [5, -1, -1, -1] and nd2[2, 0] == uc.r2_of(2.0) == 4.0     # d2 == r2 counts as inside
    assert nbr[3].tolist() == [-1] * 4 and np.isinf(nd2[3]).all()
    counts = (uc.neighbours_of(IDS.index("counts"))[0] >= 0).sum(1)
    assert sorted(set(counts.tolist())) == [0, 1, 2, 3, 4]
    nd2 = uc.neighbours_of(IDS.index("counts"))[1]
    assert (nd2 == np.float32(2.25)).any()
    got = {k: set() for k in "GLNF"}
    for G, L, N, F in uc.SHAPES:
        for k, v in zip("GLNF", (G, L, N, F)):
            got[k].add(v)
    assert got["L"] >= {2, 3, 64, 65, 66, 100, 129} and got["G"] >= {1, 2, 3, 4, 5, 255, 256, 257, 513}
    assert got["N"] >= {1, 3, 63, 64, 65, 255, 256, 257} and got["F"] >= {0, 1, 3, 5} and (257, 66, 257, 3) in uc.SHAPES
    for c in CASES:                                                                     # frames differ per guide and per child
        assert not np.array_equal(c["gM"][0], np.eye(3, dtype=np.float32)) and not np.array_equal(c["cM"][0], c["gM"][0])
        assert np.abs(np.einsum("gij,gik->gjk", c["gM"].astype(np.float64), c["gM"].astype(np.float64)) - np.eye(3)).max() < 1e-6


def test_the_shaped_guides_have_the_similarities_they_claim():
    i = IDS.index("shapes_gated")
    c = CASES[i]
    nbr, nd2 = uc.neighbours_of(i)
    assert nbr[:7, 0].tolist() == list(range(7))                                       # every kind is the nearest guide once
    ref = uc.arbiter_of(i)
    w = ref["weights"]
    row = lambda child, guide: w[child, nbr[child].tolist().index(guide)]               # noqa: E731
    assert nbr[0].tolist() == [0, 1, 2, 3]
    assert row(0, 1) > 0 and row(0, 2) == 0 and row(0, 3) == 0                          # s = 0.707 > tau; s = 0.259 < tau; s = -1
    q1 = row(0, 1) / row(0, 0) * (nd2[0, 1] + c["eps2"]) / (nd2[0, 0] + c["eps2"])      # a_1 / a_0 with the distances taken out
    assert abs(q1 - (np.cos(np.radians(45)) - 0.5) / 0.5) < 1e-6
    assert row(3, 3) == 1 and w[3, 1:].tolist() == [0, 0, 0]                            # the mirrored guide is nearest: all others gated out
    assert nbr[6].tolist() == [6, 5, 4, 3] and row(6, 4) > 0 and row(6, 5) == 0 and row(6, 3) == 0   # s = 1; zero length later: s = 0
    assert abs(row(6, 4) / row(6, 6) * (nd2[6, 2] + c["eps2"]) / (nd2[6, 0] + c["eps2"]) - 1) < 1e-6
    assert nbr[5, 0] == 5 and w[5].tolist() == [1, 0, 0, 0]                             # zero length as the nearest: A_0 = 0
    assert np.array_equal(ref["points"][5], np.repeat(c["co"][5:6].astype(np.float64), c["gp"].shape[1], 0))
    assert nbr[7, :2].tolist() == [0, 1] and nd2[7, 0] == nd2[7, 1]                     # a tie in distance, the weights apart by q alone
    free = uc.arbiter_of(IDS.index("shapes_no_gate"))["weights"]
    assert (free > 0).all()


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_host_walk_and_composed_form_against_the_float64_arbiter(sim, index):
    c = CASES[index]
    nbr, nd2 = uc.neighbours_of(index)
    ref = uc.arbiter_of(index)
    walk, comp = _walk(sim, c, nbr, nd2), _composed(c)
    for who, got in (("host walk", walk), ("composed", comp)):
        ratio = uc.excess(got, ref)
        print(c["name"], who, "largest error / bound %.4f" % ratio)
        assert ratio <= 1.0, (c["name"], who, ratio)
        assert np.array_equal(np.asarray(got["valid"]).astype(bool), ref["valid"])
        assert np.array_equal(_bits(got["points"][:, 0]), _bits(c["co"]))               # out[:, 0] == co exactly
    assert np.array_equal(comp["nbr"], nbr) and np.array_equal(comp["keep"], ref["valid"]) and comp["eps2"] == c["eps2"]
    # the table handed over: the same bits as the table searched
    again = _composed(c, neighbours=(_t(nbr), _t(nd2)))
    for k in ("points", "weights", "features"):
        assert np.array_equal(_bits(again[k]), _bits(comp[k])), k


def test_point_zero_is_the_origin_whatever_the_sign_of_its_zeros(sim):
    c = dict(CASES[IDS.index("G5_L66_N65_F0")])
    co = c["co"].copy()
    co[0] = (-0.0, 0.0, -0.0)
    c["co"] = co
    nbr, nd2 = uc.model_neighbours(c["gp"][:, 0], co)
    for got in (_walk(sim, c, nbr, nd2), _composed(c)):
        assert np.array_equal(_bits(got["points"][:, 0]), _bits(co))


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plant", uc.PLANTS)
def test_each_planted_error_exceeds_the_bound_on_every_case_it_applies_to(plant):
    applies = [i for i, c in enumerate(CASES) if plant in c["plants"]]
    assert len(applies) >= 3, plant
    for i in applies:
        c = CASES[i]
        nbr, nd2 = uc.neighbours_of(i)
        wrong = uc.arbiter(c, *uc.fifth_for_fourth(i)) if plant == "fifth" else uc.arbiter(c, nbr, nd2, plant=plant)
        ratio = uc.excess(wrong, uc.arbiter_of(i))
        print(plant, c["name"], "error / bound %.1f" % ratio)
        assert ratio > 1.0, (plant, c["name"], ratio)


def test_the_planted_errors_apply_where_the_shapes_say():
    for c in CASES:
        G, L = c["gp"].shape[:2]
        assert "cM_T" in c["plants"]
        assert ("lane" in c["plants"]) == (L >= 64), c["name"]
        assert "fifth" not in c["plants"] or (G >= 5 and c["radius"] is None)
        assert "swap" not in c["plants"] or G >= 3
        assert "gate" not in c["plants"] or (c["tau"] is not None and G >= 2)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_entries_outside_the_guides_end_a_childs_list(sim):
    i = IDS.index("G5_L100_N3_F3")
    c = CASES[i]
    nbr, nd2 = (a.copy() for a in uc.neighbours_of(i))
    G = c["gp"].shape[0]
    nbr[0, 1] = G            # the list of child 0 ends after one entry, though entries 2 and 3 are guides
    nbr[1, 0] = -3           # child 1 has no list at all
    nbr[2, 3] = 1 << 30
    got = _walk(sim, c, nbr, nd2)                              # (the walk checks every index it forms)
    cut = nbr.copy()
    cut[0, 1:] = -1
    cut[1] = -1
    cut[2, 3] = -1
    want = _walk(sim, c, cut, nd2)
    for k in ("points", "weights", "features", "valid"):
        assert np.array_equal(got[k], want[k]), k
    assert got["valid"].tolist() == [1, 0, 1] and got["weights"][0].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert np.array_equal(got["points"][1], np.repeat(c["co"][1:2], c["gp"].shape[1], 0)) and not got["features"][1].any()
    comp = _composed(c, neighbours=(_t(nbr), _t(nd2)))         # the composed form reads the same rule
    ref = uc.arbiter(c, nbr, nd2)
    assert uc.excess(comp, ref) <= 1.0 and comp["valid"].tolist() == [True, False, True]


def test_a_child_on_a_guides_root_alone_in_reach_is_the_guide_turned_into_its_frame(sim):
    i = IDS.index("lattice")
    c = dict(CASES[i])
    c["co"] = np.ascontiguousarray(c["gp"][:, 0])              # a child on every guide's root
    c["cM"] = uc.rotations(np.random.default_rng(5), c["co"].shape[0])
    c["radius"] = 0.5
    nbr, nd2 = uc.model_neighbours(c["co"], c["co"], 0.5)
    G = c["co"].shape[0]
    assert np.array_equal(nbr[:, 0], np.arange(G)) and (nbr[:, 1:] == -1).all() and not nd2[:, 0].any()
    gp, gM, cM = (c[k].astype(np.float64) for k in ("gp", "gM", "cM"))
    local = np.einsum("gic,gli->glc", gM, gp - gp[:, :1])
    want = gp[:, :1] + np.einsum("grc,glc->glr", cM, local)
    for got in (_walk(sim, c, nbr, nd2), _composed(c)):
        assert (got["weights"] == np.array([1, 0, 0, 0], np.float32)).all()
        bound = 16 * uc.EPS * (2 * np.abs(local).sum(-1) + np.abs(gp[:, :1]).max(-1))[..., None]
        assert (np.abs(got["points"] - want) <= bound).all()
        assert np.array_equal(_bits(got["features"]), _bits(c["gf"]))           # w = 1 exactly: the guide's own features
    same = dict(c, cM=c["gM"])                                                   # the child's frame the guide's: the guide itself
    got = _walk(sim, same, nbr, nd2)
    assert (np.abs(got["points"] - gp) <= 16 * uc.EPS * (2 * np.abs(local).sum(-1) + np.abs(gp[:, :1]).max(-1))[..., None]).all()


@pytest.mark.parametrize("name", ["G257_L66_N257_F3", "counts"])
def test_permuting_the_children_permutes_the_outputs_bit_for_bit(sim, name):
    i = IDS.index(name)
    c = CASES[i]
    perm = np.random.default_rng(17).permutation(c["co"].shape[0])
    p = dict(c, co=np.ascontiguousarray(c["co"][perm]), cM=np.ascontiguousarray(c["cM"][perm]))
    nbr, nd2 = uc.neighbours_of(i)
    pn, pd = upsample_sim.near(sim, p["gp"][:, 0].copy(), p["co"], uc.r2_of(c["radius"]))
    assert np.array_equal(pn, nbr[perm]) and np.array_equal(_bits(pd), _bits(nd2[perm]))
    for a, b in ((_walk(sim, c, nbr, nd2), _walk(sim, p, pn, pd)), (_composed(c), _composed(p))):
        for k in ("points", "weights", "features"):
            assert np.array_equal(_bits(a[k][perm]), _bits(b[k])), k
        assert np.array_equal(np.asarray(a["valid"])[perm], b["valid"])


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_defaults_and_refusals_of_the_python_front():
    c = CASES[IDS.index("G5_L66_N65_F0")]
    gp, gM, co, cM = (_t(c[k]) for k in ("gp", "gM", "co", "cM"))
    out = su.upsample_strands(gp, gM, co, cM)                                   # CPU tensors: the composed form by default
    roots = c["gp"][:, 0].astype(np.float32)
    d = roots[:, None] - roots[None]
    d2 = ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])
    np.fill_diagonal(d2, np.inf)
    want = float(np.float32(1e-6) * np.float32(torch.median(torch.from_numpy(d2.min(1)))))
    assert out["eps2"] == want == su.default_eps2(gp[:, 0]) and su.TAU == 0.5 and su.EPS2_FACTOR == 1e-6
    assert su.default_eps2(gp[:1, 0]) == su.EPS2_FLOOR == su.default_eps2(torch.zeros(3, 3))
    assert out["points"].shape == (65, 66, 3) and out["features"].shape == (65, 0) and out["weights"].shape == (65, 4)
    assert out["valid"].dtype == torch.bool and out["keep"].dtype == torch.bool and out["nbr"].dtype == torch.int32
    off = su.upsample_strands(gp, gM, co, cM, tau=None)
    assert not torch.equal(off["weights"], out["weights"])
    empty = su.upsample_strands(gp, gM, co[:0], cM[:0])
    assert empty["points"].shape == (0, 66, 3) and empty["keep"].shape == (0,)
    with pytest.raises(RuntimeError, match="no CPU path"):
        su.upsample_strands(gp, gM, co, cM, fused=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        su.guide_neighbours(gp[:, 0], co, fused=True)
    for kw, match in ((dict(tau=1.0), "tau"), (dict(tau=-1.5), "tau"), (dict(eps2=0.0), "eps2"), (dict(eps2=float("inf")), "eps2"),
                      (dict(radius=0.0), "radius"), (dict(neighbours=(out["nbr"][:3], out["nbr"][:3].float())), "neighbours")):
        with pytest.raises(ValueError, match=match):
            su.upsample_strands(gp, gM, co, cM, **kw)
    with pytest.raises(ValueError, match="points"):
        su.upsample_strands(gp[:, :1], gM, co, cM)
    with pytest.raises(ValueError, match="frame"):
        su.upsample_strands(gp, gM[:3], co, cM)
    with pytest.raises(ValueError, match="guides on"):
        su.upsample_strands(gp, gM, co.to("meta"), cM)
    for name in ("upsample_strands", "default_eps2"):
        assert "chosen and not measured" in getattr(su, name).__doc__


def test_frames_from_normals_are_orthonormal_right_handed_and_deterministic():
    rng = np.random.default_rng(3)
    n = rng.normal(size=(50, 3))
    n[0] = (0, 2, 0)            # parallel to up
    n[1] = (0, -1, 0)
    n[2] = (0, 0, 0)            # no normal: the identity
    n[3] = (np.nan, 0, 1)
    M = su.frames_from_normals(torch.from_numpy(n))
    assert M.dtype == torch.float32 and M.shape == (50, 3, 3) and torch.equal(M, su.frames_from_normals(torch.from_numpy(n)))
    M64 = M.double().numpy()
    assert np.abs(np.einsum("nij,nik->njk", M64, M64) - np.eye(3)).max() < 1e-6 and (np.linalg.det(M64) > 0.999).all()
    good = np.ones(50, bool)
    good[[2, 3]] = False
    unit = n[good] / np.linalg.norm(n[good], axis=1, keepdims=True)
    assert np.abs(M64[good][:, :, 2] - unit).max() < 1e-6                       # the third column is the normal
    t = np.cross(np.array([0.0, 1.0, 0.0]), unit[4:])
    assert np.abs(M64[good][4:, :, 0] - t / np.linalg.norm(t, axis=1, keepdims=True)).max() < 1e-6
    assert np.array_equal(M64[0][:, 0], [0, 0, 1]) and np.array_equal(M64[1][:, 0], [0, 0, -1])   # the x axis stands in: x cross n
    assert np.array_equal(M64[2], np.eye(3)) and np.array_equal(M64[3], np.eye(3))
    with pytest.raises(ValueError, match="up"):
        su.frames_from_normals(torch.from_numpy(n), up=(0, 0, 0))


def _uv_scalp():
    from gaussianhaircut_amd import strand_generator as sgen
    from gaussianhaircut_amd.mesh import HeadMesh
    v, f = mc.uv_sphere(24, 10)
    uv = np.stack([np.arctan2(v[:, 2], v[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(v[:, 1], -1, 1)) / np.pi], 1).astype(np.float32)
    frames = sgen.scalp_frames(torch.from_numpy(v), torch.from_numpy(f.astype(np.int64)), torch.from_numpy(uv))
    return v, f, uv, frames, HeadMesh(v, f)


def test_frames_at_takes_the_frame_of_the_closest_scalp_face():
    v, f, uv, frames, mesh = _uv_scalp()
    rng = np.random.default_rng(4)
    pick = rng.choice(len(f), 40, replace=False)
    inner = v[f[pick]].astype(np.float64).mean(1)                                # a point inside face `pick`, lifted off it a little
    pts = torch.from_numpy((inner * 1.02).astype(np.float32))
    got = su.frames_at(mesh, frames, pts, fused=False)
    assert torch.equal(got, frames[torch.from_numpy(pick)]) and got.dtype == torch.float32
    assert torch.equal(su.frames_at(mesh, frames, pts.reshape(8, 5, 3)), got.reshape(8, 5, 3, 3))   # CPU tensors: composed by default
    bad = pts.clone()
    bad[0, 0] = float("nan")
    assert torch.equal(su.frames_at(mesh, frames, bad, fused=False)[0], torch.eye(3))
    with pytest.raises(ValueError, match="face_frames"):
        su.frames_at(mesh, frames[:-1], pts)


def _small_groom():
    """12 guides of 9 points on the small UV sphere, grown outwards with a lean"""
    rng = np.random.default_rng(8)
    d = rng.normal(size=(12, 3))
    d[:, 1] = np.abs(d[:, 1]) + 0.5                                              # the upper half
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    u = np.linspace(0, 0.4, 9)[None, :, None]
    lean = np.array([0.3, -0.2, 0.1])
    return (d[:, None] * (1.0 + u) + lean * u * u).astype(np.float32)


def test_create_from_polylines_accepts_the_result():
    from gaussianhaircut_amd.scene.gaussian_model_strands import GaussianModelStrands
    from gaussianhaircut_amd import strand_generator as sgen
    v, f, uv, frames, mesh = _uv_scalp()
    guides = torch.from_numpy(_small_groom())
    rgb = torch.rand(12, 3, generator=torch.Generator().manual_seed(1))
    roots = sgen.sample_roots(torch.from_numpy(v), torch.from_numpy(f.astype(np.int64)), torch.from_numpy(uv), 40,
                              generator=torch.Generator().manual_seed(2))
    out = su.upsample_strands(guides, su.frames_at(mesh, frames, guides[:, 0]), roots["origins"], roots["local2world"], features=rgb,
                              radius=1.0, mesh=mesh)
    keep = out["keep"]
    assert 0 < int(keep.sum()) <= int(out["valid"].sum()) <= 40 and not bool((keep & ~out["valid"]).any())
    hair = GaussianModelStrands(3).create_from_polylines(out["points"][keep], rgb=out["features"][keep])
    assert hair.num_strands == int(keep.sum()) and hair.strand_length == 9
    assert torch.equal(hair.pts_origins.reshape(-1, 3), roots["origins"][keep])
    assert float(out["features"][keep].min()) >= 0 and float(out["features"][keep].max()) <= 1   # a convex blend of the guides'
    # a blended strand leaves the scalp as its guides do: its first segment points outwards
    first = out["points"][keep][:, 1] - out["points"][keep][:, 0]
    assert bool(((first * roots["origins"][keep]).sum(1) > 0).all())


def test_the_tools_upsample_step_round_trips_a_small_scene(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("between_stages_tool", os.path.join(hp.ROOT, "tools", "between_stages.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    v, f, uv, frames, mesh = _uv_scalp()
    with open(tmp_path / "scalp.obj", "w") as fh:
        fh.write("".join("v %r %r %r\n" % tuple(map(float, p)) for p in v) + "".join("vt %r %r\n" % tuple(map(float, p)) for p in uv)
                 + "".join("f %d/%d %d/%d %d/%d\n" % (a + 1, a + 1, b + 1, b + 1, c + 1, c + 1) for a, b, c in f))
    hv, hf = mc.uv_sphere(24, 10, radius=0.98)
    with open(tmp_path / "head.obj", "w") as fh:
        fh.write("".join("v %r %r %r\n" % tuple(map(float, p)) for p in hv) + "".join("f %d %d %d\n" % tuple(t + 1) for t in hf))
    guides = _small_groom()
    np.save(tmp_path / "guides.npy", guides)
    rgb = np.random.default_rng(6).random((12, 3)).astype(np.float32)
    np.save(tmp_path / "rgb.npy", rgb)
    assert np.array_equal(tool._obj_uvs(str(tmp_path / "scalp.obj"), len(v)), uv)
    args = ["upsample", "--points", str(tmp_path / "guides.npy"), "--scalp", str(tmp_path / "scalp.obj"), "--mesh", str(tmp_path / "head.obj"),
            "--count", "50", "--seed", "3", "--radius", "1.0", "--tau", "0.25", "--features", str(tmp_path / "rgb.npy"), "--iter", "7", "--composed"]
    tool.main(args + ["--out_dir", str(tmp_path / "a")])
    text = capsys.readouterr().out
    got = pickle.load(open(tmp_path / "a" / "7_strands.pkl", "rb"))
    kept = int(re.search(r"kept (\d+)", text).group(1))
    assert got.shape == (kept, 9, 3) and 0 < kept <= 50 and "upsample: 12 guides of 9 points, 50 children" in text
    assert np.load(tmp_path / "a" / "7_strands_rgb.npy").shape == (kept, 3) and os.path.exists(tmp_path / "a" / "7_strands.ply")
    # the same call through the module
    from gaussianhaircut_amd import strand_generator as sgen
    roots = sgen.sample_roots(torch.from_numpy(v), torch.from_numpy(f.astype(np.int64)), torch.from_numpy(uv), 50,
                              generator=torch.Generator().manual_seed(3))
    from gaussianhaircut_amd.mesh import HeadMesh
    want = su.upsample_strands(torch.from_numpy(guides), su.frames_at(mesh, frames, torch.from_numpy(guides[:, 0])), roots["origins"],
                               roots["local2world"], features=torch.from_numpy(rgb), radius=1.0, tau=0.25, mesh=HeadMesh(hv, hf))
    assert np.array_equal(got, want["points"][want["keep"]].numpy())
    tool.main(args + ["--out_dir", str(tmp_path / "b"), "--with_guides", "--no_gate"])
    both = pickle.load(open(tmp_path / "b" / "7_strands.pkl", "rb"))
    assert np.array_equal(both[:12], guides) and both.shape[0] > 12 and np.load(tmp_path / "b" / "7_strands_rgb.npy").shape == (both.shape[0], 3)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,out", [(["-O1"], "ghr_upsample_selfcheck"),
                                       (["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"],
                                        "ghr_upsample_selfcheck_san")], ids=["plain", "sanitized"])
def test_stand_alone_program_walks_the_loops_clean(flags, out):
    if len(flags) > 1 and os.path.basename(hp.host_cxx()) == "g++":
        flags = flags + ["-static-libasan", "-static-libubsan"]
    exe = hp.compile_hostsim(out, "ghr_upsample_selfcheck.cpp", flags, ["ghr_hostsim_upsample.cpp"] + upsample_sim.DEPS)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "3 cases ok" in res.stdout and "runtime error" not in res.stderr, res.stdout + res.stderr


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
ARGS = {
    "ghr_upsample_neighbours": ("stream", "G", "guide_roots", "N", "child_origins", "r2", "nbr", "nd2"),
    "ghr_upsample_blend": ("stream", "G", "L", "gp", "gM", "gf", "F", "N", "co", "cM", "nbr", "nd2", "eps2", "tau", "gate", "out", "w", "of",
                           "valid"),
}
SCALARS = dict(G=10, L=8, F=3, N=20, r2=0.01, eps2=1e-6, tau=0.5, gate=1)
X = 0x1000  # stands for a buffer: none of these calls follows a pointer
NAN, INF = float("nan"), float("inf")
REFUSALS = [
    ("ghr_upsample_neighbours", dict(G=0), "G < 1"), ("ghr_upsample_neighbours", dict(G=-1), "G < 1"),
    ("ghr_upsample_neighbours", dict(N=-1), "N < 0"), ("ghr_upsample_neighbours", dict(r2=0.0), "r2 must be"),
    ("ghr_upsample_neighbours", dict(r2=-1.0), "r2 must be"), ("ghr_upsample_neighbours", dict(r2=NAN), "r2 must be"),
    ("ghr_upsample_neighbours", dict(G=(1 << 31) // 3 + 1), "32-bit"), ("ghr_upsample_neighbours", dict(N=1 << 29), "32-bit"),
    ("ghr_upsample_neighbours", dict(guide_roots=None), "NULL"), ("ghr_upsample_neighbours", dict(child_origins=None), "NULL"),
    ("ghr_upsample_neighbours", dict(nbr=None), "NULL"), ("ghr_upsample_neighbours", dict(nd2=None), "NULL"),
    ("ghr_upsample_blend", dict(G=0), "G < 1"), ("ghr_upsample_blend", dict(N=-1), "N < 0"), ("ghr_upsample_blend", dict(L=1), "L < 2"),
    ("ghr_upsample_blend", dict(F=-1), "F < 0"), ("ghr_upsample_blend", dict(eps2=0.0), "eps2 must be"),
    ("ghr_upsample_blend", dict(eps2=-1.0), "eps2 must be"), ("ghr_upsample_blend", dict(eps2=INF), "eps2 must be"),
    ("ghr_upsample_blend", dict(eps2=NAN), "eps2 must be"), ("ghr_upsample_blend", dict(tau=1.0), "tau must"),
    ("ghr_upsample_blend", dict(tau=-1.5), "tau must"), ("ghr_upsample_blend", dict(tau=NAN), "tau must"),
    ("ghr_upsample_blend", dict(G=1 << 20, L=1 << 10), "32-bit"), ("ghr_upsample_blend", dict(N=1 << 20, L=1 << 10), "32-bit"),
    ("ghr_upsample_blend", dict(N=1 << 29), "32-bit"), ("ghr_upsample_blend", dict(N=1 << 20, F=1 << 11), "32-bit"),
] + [("ghr_upsample_blend", {k: None}, "NULL") for k in ("gp", "gM", "gf", "co", "cM", "nbr", "nd2", "out", "w", "of", "valid")]


def _call(L, fn, changes):
    names = ARGS[fn]
    a = {k: SCALARS.get(k, None if k == "stream" else X) for k in names}
    assert set(changes) <= set(a), (fn, changes)
    a.update(changes)
    rc = getattr(L, fn)(*[a[k] for k in names])
    return int(rc), L.ghr_last_error().decode()


def test_c_abi_symbols_are_declared_exported_and_bound():
    L = _lib.lib()
    with open(os.path.join(hp.ROOT, "include", "ghr.h")) as fh:
        hdr = fh.read()
    for n in ARGS:
        assert re.search(r"\bint %s\(" % n, hdr) and n in _lib.EXPORTS and hasattr(L, n) and getattr(L, n).argtypes, n
        assert len(getattr(L, n).argtypes) == len(ARGS[n]), n
    assert L.ghr_abi_version() == 20 == _lib.ABI_VERSION and "#define GHR_ABI_VERSION 20" in hdr
    assert "ghr_upsample.h" in _lib.HEADERS and os.path.exists(os.path.join(_lib.CSRC, "ghr_upsample.h"))
    with open(os.path.join(_lib.CSRC, "ghr_capi.hip")) as fh:
        assert '#include "ghr_upsample.h"' in fh.read()
    with open(os.path.join(_lib.CSRC, "ghr_upsample.h")) as fh:
        txt = fh.read()
    assert "atomic" not in txt.replace("no floating-point atomics", "") and "asm" not in txt


@pytest.mark.parametrize("fn,changes,words", REFUSALS, ids=["%s-%s" % (r[0][13:], "-".join("%s=%s" % kv for kv in r[1].items())) for r in REFUSALS])
def test_c_abi_refusals_launch_nothing(fn, changes, words):
    """every call is refused before the runtime is touched (the pointers are never dereferenced; this machine needs no GPU)"""
    rc, text = _call(_lib.lib(), fn, changes)
    assert rc == _lib.GHR_E_INVALID and text.startswith(fn + ":") and words in text, (rc, text)


def test_c_abi_accepts_what_the_rules_leave_open():
    L = _lib.lib()
    for fn in ARGS:
        assert _call(L, fn, dict(N=0))[0] == _lib.GHR_OK                                   # N == 0 does nothing
    assert _call(L, "ghr_upsample_neighbours", dict(N=0, r2=INF))[0] == _lib.GHR_OK         # +inf: no cut
    assert _call(L, "ghr_upsample_blend", dict(N=0, F=0, gf=None, of=None))[0] == _lib.GHR_OK   # no features, no buffers for them
    assert _call(L, "ghr_upsample_blend", dict(N=0, gate=0, tau=7.0))[0] == _lib.GHR_OK     # tau is not read without the gate
    assert _call(L, "ghr_upsample_blend", dict(N=0, tau=-1.0))[0] == _lib.GHR_OK
    nulls = {k for fn, ch, _ in REFUSALS for k, v in ch.items() if v is None and fn == "ghr_upsample_blend"}
    assert nulls == {k for k in ARGS["ghr_upsample_blend"] if k not in SCALARS} - {"stream"}
