"""Guiding strands of the textured generator (gaussianhaircut_amd/strand_generator.py: blend_from_guides, csrc/ghr_guides.h;
DESIGN.md 8q) without a GPU.

 1. every case of tests/guides_cases.py satisfies the conditions on its inputs in float64 (the 4th / 5th distance gap >= 1e-5 or an
    exact tie, no csim within 1e-4 of 0.9), so float32 and float64 choose the same neighbours; the composed form (fused=False) on
    CPU tensors against the float64 restatement: nbr / start / list bit for bit, every float within
    1e-5 max|f64| + 3 |float32 restatement - f64|.
 2. host walks of the kernels' loops (tests/hostsim/ghr_hostsim_guides.cpp) against the same arbiter, with the choices arriving
    in the opposite order of the lists; the same walks in a stand-alone program built with -fsanitize=address,undefined (nothing
    sanitized is loaded here).
 3. rows s >= N of nbr / w for uvs = cat(uv_g, texel grid) equal strand_prior.neighbours_composed(uv_g, G).
 4. the C ABI: two symbols declared and exported, every refusal answered before the runtime is touched, ABI 20.
 5. TexturedStrands(num_guiding_strands=None | 0) is the generator it was; with guides the texture's gradient stays inside the
    guides' texels; the model's _gdn views."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd import strand_generator as sg
from gaussianhaircut_amd import strand_prior as sp
from tests import guides_cases as gc
from tests import helpers as hp
from tests import texstrands_cases as tc
from tests.sds_cases import assert_within

SMALL, case = gc.SMALL, gc.case
FLOATS = ("w", "csim", "alpha", "alpha_s")


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SMALL))
def test_conditions_on_the_inputs_hold_in_float64(name):
    c = case(name)
    gap, knee, above = gc.conditions(c["r64"])
    print("smallest 4th / 5th relative gap %.3e, nearest csim to 0.9 at %.3e, %.0f %% above 0.9" % (gap, knee, 100 * above))
    assert gap >= 1e-5 and knee >= 1e-4
    assert torch.equal(c["r32"]["nbr"], c["r64"]["nbr"])                  # float32 and float64 choose the same neighbours
    assert torch.equal((c["r32"]["csim"] <= 0.9), (c["r64"]["csim"] <= 0.9))


def test_the_cases_cover_both_branches_of_alpha_and_the_tie_rules():
    share = [gc.conditions(case(n)["r64"])[2] for n in sorted(SMALL)]
    assert min(share) < 0.5 < max(share)
    nbr = case("same-uv")["r64"]["nbr"]
    assert nbr[2, :2].tolist() == [2, 5] and nbr[5, :2].tolist() == [2, 5] and nbr[8, :2].tolist() == [2, 5]   # the lower index wins
    c = case("equidistant")
    sd = c["r64"]["sorted_d2"][6]
    assert float(sd[1]) == float(sd[2]) == 0.3125 and float(sd[3]) == float(sd[4]) == 0.8125
    assert c["r64"]["nbr"][6].tolist() == [2, 1, 3, 4]


def _composed(c, z_detached=False, v_detached=False):
    z_g, v_g = c["z_g"].clone().requires_grad_(not z_detached), c["v_g"].clone().requires_grad_(not v_detached)
    z, st = sg.blend_from_guides(c["uvs"], z_g, v_g, fused=False, return_state=True)
    (z * c["d_z"]).sum().backward()
    zero = torch.zeros_like
    return dict(z=z.detach(), d_zg=zero(z_g) if z_g.grad is None else z_g.grad, d_vg=zero(v_g) if v_g.grad is None else v_g.grad, **st)


def _check(got, r64, r32, what=("z", "d_zg", "d_vg") + FLOATS):
    assert torch.equal(got["nbr"].long().cpu(), r64["nbr"])
    assert torch.equal(got["start"].long().cpu(), r64["start"]) and torch.equal(got["list"].long().cpu(), r64["entries"])
    for k in what:
        assert_within(k, got[k], r64[k], r32[k])


@pytest.mark.parametrize("name", sorted(SMALL))
def test_composed_form_on_cpu_tensors(name):
    c = case(name)
    got = _composed(c)
    _check(got, c["r64"], c["r32"])
    N = c["N"]
    assert torch.equal(got["z"][:N], c["z_g"])                             # a guide's row is its fetched row
    assert got["nbr"].dtype == torch.int32 and got["start"].dtype == torch.int32 and got["list"].dtype == torch.int32


@pytest.mark.parametrize("which", ["z", "v"])
def test_composed_form_with_one_input_detached(which):
    c = case("rows64")
    r64, r32 = gc.detached("rows64", which)
    got = _composed(c, z_detached=which == "z", v_detached=which == "v")
    live = "d_vg" if which == "z" else "d_zg"
    assert float(r64[live].abs().max()) > 0
    _check(got, r64, r32, what=("z", "d_zg", "d_vg"))


def test_python_refusals():
    uv, z, v = torch.zeros(6, 2), torch.zeros(5, 3), torch.zeros(5, 2, 3)
    with pytest.raises(ValueError, match="needs 4"):
        sg.blend_from_guides(uv, z[:3], v[:3], fused=False)
    with pytest.raises(ValueError, match="S >= N"):
        sg.blend_from_guides(uv[:4], z, v, fused=False)
    with pytest.raises(ValueError, match="z_g must be"):
        sg.blend_from_guides(uv, z, v[:4], fused=False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sg.blend_from_guides(uv, z, v, fused=True)
    for bad in (1, 2, 3, -1):
        with pytest.raises(ValueError, match="num_guiding_strands"):
            sg.TexturedStrands(tc.scalp_grid(), tc.Linear3(6, 7), num_strands=8, max_num_strands=20, texture_size=8, geometry_channels=6,
                               appearance_channels=5, num_guiding_strands=bad)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
DEPS = ["ghr_hostsim_guides.cpp", "ghr_hostsim_haar.h", "ghr_guides.h", "ghr_haar.h"]


@pytest.fixture(scope="module")
def sim():
    L = ctypes.CDLL(hp.compile_hostsim("libghr_hostsim_guides.so", "ghr_hostsim_guides.cpp", ["-O2", "-fPIC", "-shared"], DEPS))
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    L.ghrsim_gd_blend.argtypes = [i32] * 4 + [vp] * 13
    L.ghrsim_gd_blend_backward.argtypes = [i32] * 4 + [vp] * 13
    assert L.ghrsim_gd_wave() == 64
    return L


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _np(t, dtype=np.float32):
    return np.ascontiguousarray(t.detach().cpu().numpy().astype(dtype))


def _sim_block(sim, c, want_dv=True):
    S, N, n, C = c["S"], c["N"], c["n"], c["C"]
    uvs, z_g, v_g, d_z = _np(c["uvs"]), _np(c["z_g"]), _np(c["v_g"]), _np(c["d_z"])
    st = dict(nbr=np.full((S, 4), -1, np.int32), w=np.full((S, 4), np.nan, np.float32), csim=np.full(N, np.nan, np.float32),
              alpha=np.full(N, np.nan, np.float32), alpha_s=np.full(S, np.nan, np.float32), count=np.full(N, -1, np.int32),
              start=np.full(N + 1, -1, np.int32), unsorted=np.full(4 * S, -1, np.int32), list=np.full(4 * S, -1, np.int32))
    z = np.full((S, C), np.nan, np.float32)
    sim.ghrsim_gd_blend(S, N, n, C, _p(uvs), _p(z_g), _p(v_g), *[_p(st[k]) for k in ("nbr", "w", "csim", "alpha", "alpha_s", "count", "start",
                                                                                    "unsorted", "list")], _p(z))
    sa, sc_ = np.full(S, np.nan, np.float32), np.full(N, np.nan, np.float32)
    d_zg = np.full((N, C), np.nan, np.float32)
    d_vg = np.full((N, n, 3), np.nan, np.float32) if want_dv else None
    sim.ghrsim_gd_blend_backward(S, N, n, C, _p(z_g), _p(v_g), *[_p(st[k]) for k in ("nbr", "w", "csim", "alpha_s", "start", "list")], _p(d_z),
                                 _p(sa), _p(sc_), _p(d_zg), _p(d_vg))
    T = torch.from_numpy
    return dict(z=T(z), d_zg=T(d_zg), d_vg=None if d_vg is None else T(d_vg), **{k: T(a) for k, a in st.items()})


@pytest.mark.parametrize("name", sorted(SMALL))
def test_host_walks(sim, name):
    c = case(name)
    got = _sim_block(sim, c)
    _check(got, c["r64"], c["r32"])
    assert not bool((got["unsorted"] == -1).any()) and int(got["count"].abs().max()) == 0
    assert torch.equal(torch.sort(got["unsorted"])[0], torch.arange(4 * c["S"], dtype=torch.int32))
    assert torch.equal(got["z"][:c["N"]], c["z_g"])
    if name == "rows3":                                                     # d_vg = NULL: d_zg is the same, nothing else is written
        assert torch.equal(_sim_block(sim, c, want_dv=False)["d_zg"], got["d_zg"])


def test_sanitized_stand_alone_program_runs_the_walks_clean(sim, tmp_path):
    """ghr_guides_selfcheck: the walks under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own
    (exact-size buffers)."""
    san = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    if os.path.basename(hp.host_cxx()) == "g++":
        san += ["-static-libasan", "-static-libubsan"]
    exe = hp.compile_hostsim("ghr_guides_selfcheck_san", "ghr_guides_selfcheck.cpp", san, DEPS)
    path = str(tmp_path / "cases.bin")
    names = sorted(SMALL)
    with open(path, "wb") as fh:
        for name in names:
            c = case(name)
            got = _sim_block(sim, c)
            tol = 1e-5 * max(float(c["r64"]["z"].abs().max()), float(c["r64"]["d_zg"].abs().max()))
            fh.write(np.array([c["S"], c["N"], c["n"], c["C"]], np.int32).tobytes())
            fh.write(np.array([tol], np.float32).tobytes())
            for arr, dt in ((c["uvs"], np.float32), (c["z_g"], np.float32), (c["v_g"], np.float32), (c["d_z"], np.float32),
                            (c["r64"]["nbr"], np.int32), (c["r64"]["start"], np.int32), (c["r64"]["entries"], np.int32),
                            (got["z"], np.float32), (got["d_zg"], np.float32)):
                fh.write(_np(arr, dt).tobytes())
    res = subprocess.run([exe, path], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "%d cases ok" % len(names) in res.stdout and "runtime error" not in res.stderr, res.stdout + res.stderr


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,G", [(9, 3), (65, 9), (130, 12)])
def test_rows_beside_the_guides_are_the_strand_priors_texel_neighbours(sim, N, G):
    """with the texel grid as the rows s >= N the blend's neighbours are the strand prior's (csrc/ghr_sds.h restated over strands)"""
    uv_g = torch.rand(N, 2, generator=torch.Generator().manual_seed(N)) * 2 - 1
    cc = sp.texel_centres(G, "cpu")
    grid = torch.stack(torch.meshgrid(cc, cc, indexing="xy"), dim=-1).view(-1, 2)
    uvs = torch.cat([uv_g, grid])
    want_nbr, want_w = sp.neighbours_composed(uv_g, G)
    nbr, w = sg.guide_neighbours_composed(uvs, N)
    assert torch.equal(nbr[N:], want_nbr) and torch.equal(w[N:], want_w)    # the same float32 expressions: the same bits
    c = dict(uvs=uvs, z_g=torch.zeros(N, 2), v_g=torch.ones(N, 1, 3), d_z=torch.zeros(N + G * G, 2), S=N + G * G, N=N, n=1, C=2)
    got = _sim_block(sim, c)
    assert torch.equal(got["nbr"][N:].long(), want_nbr)
    assert torch.allclose(got["w"][N:], want_w, rtol=1e-6, atol=0)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
NAMES = ("ghr_guides_blend", "ghr_guides_blend_backward")
FWD = ("uvs", "z_g", "v_g", "nbr", "w", "csim", "alpha", "alpha_s", "count", "start", "unsorted", "list", "z")
BWD = ("z_g", "v_g", "nbr", "w", "csim", "alpha_s", "start", "list", "d_z", "dalpha_s", "d_csim", "d_zg", "d_vg")
TABLE = os.path.join(hp.ROOT, "tests", "golden", "guides_refusals.json")
SIZES = dict(S=9, N=5, n=3, C=2)
X = 0x1000  # stands for a buffer: none of these calls follows a pointer


def _table():
    """tests/golden/guides_refusals.json: calls of the two entry points -- the well-formed argument set above with the fields a case
    changes (null: a NULL pointer) -- and the (return code, ghr_last_error text) each gave when the table was recorded"""
    import json
    with open(TABLE) as fh:
        return json.load(fh)["cases"]


def test_c_abi_symbols_are_declared_and_exported():
    L = _lib.lib()
    with open(os.path.join(hp.ROOT, "include", "ghr.h")) as fh:
        hdr = fh.read()
    for n in NAMES:
        assert re.search(r"\bint %s\(" % n, hdr) and n in _lib.EXPORTS and hasattr(L, n), n
    assert L.ghr_abi_version() == 20 == _lib.ABI_VERSION and "#define GHR_ABI_VERSION 20" in hdr
    assert "ghr_guides.h" in _lib.HEADERS and os.path.exists(os.path.join(hp.ROOT, "gaussianhaircut_amd", "csrc", "ghr_guides.h"))
    with open(os.path.join(hp.ROOT, "gaussianhaircut_amd", "csrc", "ghr_capi.hip")) as fh:
        assert '#include "ghr_guides.h"' in fh.read()


@pytest.mark.parametrize("case", _table(), ids=lambda c: c["id"])
def test_c_abi_refusals_launch_nothing(case):
    """every call of the table is refused before the runtime is touched (the pointers are never dereferenced), in the recorded words"""
    L = _lib.lib()
    names = dict(ghr_guides_blend=FWD, ghr_guides_blend_backward=BWD)[case["fn"]]
    a = dict(SIZES, **dict.fromkeys(names, X))
    assert set(case["set"]) <= set(a), case["id"]
    a.update(case["set"])
    rc = getattr(L, case["fn"])(None, *[a[k] for k in ("S", "N", "n", "C") + names])
    assert [int(rc), L.ghr_last_error().decode()] == case["expect"], (case["id"], rc, L.ghr_last_error())
    assert rc == _lib.GHR_E_INVALID and case["fn"] + ":" in case["expect"][1]


def test_the_refusal_table_covers_every_rule_and_every_pointer():
    cases = _table()
    assert len({c["id"] for c in cases}) == len(cases)
    for fn, names in (("ghr_guides_blend", FWD), ("ghr_guides_blend_backward", BWD)):
        mine = [c for c in cases if c["fn"] == fn]
        nulls = {k for c in mine for k, v in c["set"].items() if v is None}
        assert nulls == set(names) - {"d_vg"}, (fn, nulls)                    # d_vg may be NULL: no d_vg is asked for
        text = " | ".join(c["expect"][1] for c in mine)
        for rule in ("N < 4", "S < N", "n < 1", "C < 1", "32-bit"):
            assert rule in text, (fn, rule)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def _generator(num_guiding="absent", S=40, Smax=120, T=8, Cg=6, Ca=5, L=8, seed=3, fused=True):
    kw = {} if num_guiding == "absent" else dict(num_guiding_strands=num_guiding)
    target = torch.rand(1, Cg, T, T, generator=torch.Generator().manual_seed(seed + 1))
    gen = sg.TexturedStrands(tc.scalp_grid(), tc.Linear3(Cg, L - 1), tc.LinearColour(Ca - 1), lambda t: ((t - target) ** 2).mean(),
                             num_strands=S, max_num_strands=Smax, texture_size=T, geometry_channels=Cg, appearance_channels=Ca,
                             scale_decoder=2.0, generator=torch.Generator().manual_seed(seed), fused=fused, **kw)
    with torch.no_grad():
        gen.texture.copy_(torch.rand(gen.texture.shape, generator=torch.Generator().manual_seed(seed + 2)) * 2 - 1)
    return gen


@pytest.mark.parametrize("num_guiding", [None, 0, 40, 1000])
def test_without_guides_the_generator_is_the_one_it_was(num_guiding):
    """None, 0, and S <= N (every strand a guide): the tensors of the constructor without the argument, bit for bit"""
    a, b = _generator(), _generator(num_guiding)
    assert b.num_guiding_strands == (num_guiding or 0) and a.num_guiding_strands == 0
    for name in ("forward", "forward_reference"):
        oa, ob = getattr(a, name)(1), getattr(b, name)(1)
        oa, ob = (oa, ob) if isinstance(oa, dict) else (dict(enumerate(oa[:6])), dict(enumerate(ob[:6])))
        assert sorted(oa, key=str) == sorted(ob, key=str)
        for k in oa:
            assert torch.equal(oa[k], ob[k]), (name, k)
        assert torch.equal(a.last_idx, b.last_idx) and b.last_num_guiding == 0
    la, lb = a(2), b(2)
    (la["points"].sum() + la["features"].sum() + la["L_diff"]).backward()
    (lb["points"].sum() + lb["features"].sum() + lb["L_diff"]).backward()
    assert torch.equal(a.texture.grad, b.texture.grad)
    ia, ib = a.forward_inference(7), b.forward_inference(7)
    assert all(torch.equal(x, y) for x, y in zip(ia, ib))


def test_with_guides_the_rows_are_the_blend_and_the_gradient_stays_in_the_guides_texels():
    S, N, Cg = 40, 9, 6
    gen = _generator(N)
    p, uvs, l2w, pl, z_geom, z_app, diff = gen.forward_reference(1)
    idx = gen.last_idx
    assert gen.last_num_guiding == N and gen.num_guiding_strands == N and torch.equal(uvs, gen.uvs[idx])
    z_g = sg.sample_texture(gen.texture, gen.taps, idx[:N], fused=False)
    v_g = gen.strand_decoder(z_g[:, :Cg])
    z = sg.blend_from_guides(gen.uvs[idx], z_g, v_g, fused=False)
    assert torch.equal(z_geom, z[:, :Cg]) and torch.equal(z_app, z[:, Cg:])     # forward_reference's rows are the blended rows
    assert torch.equal(z[:N], z_g) and not torch.equal(z[N:], sg.sample_texture(gen.texture, gen.taps, idx[N:], fused=False))
    v = torch.cat([v_g, gen.strand_decoder(z[N:, :Cg])])
    assert torch.equal(p, sg.strands_to_world(v, gen.local2world, gen.origins, idx, gen.scale_decoder, fused=False))
    out = gen(2)
    assert out["points"].shape == (S, 8, 3) and out["features"].shape == (S, 48) and out["orient_conf"].shape == (S, 1)
    (out["points"] ** 2).sum().add(out["features"].sum()).backward()             # (no L_diff: it reaches every texel)
    tp, idx = gen.taps, gen.last_idx
    mask = torch.zeros(8, 8, dtype=torch.bool)
    for r in idx[:N].tolist():
        for k in range(4):
            x, y = int(tp.x0[r]) + (k & 1), int(tp.y0[r]) + (k >> 1)
            if 0 <= x < 8 and 0 <= y < 8:
                mask[y, x] = True
    g = gen.texture.grad[0]
    assert float(g[:, ~mask].abs().max()) == 0.0 and float(g[:, mask].abs().max()) > 0 and int((~mask).sum()) > 0
    q = gen.forward_inference(4)                                                  # S <= N: every strand a guide
    assert gen.last_num_guiding == 0 and q[0].shape == (4, 8, 3)
    q = gen.forward_inference(12)
    assert gen.last_num_guiding == N and q[4].shape == (12, Cg)


@pytest.mark.parametrize("shared", [False, True])
def test_the_models_guiding_views(shared):
    from gaussianhaircut_amd.scene.gaussian_model_latent_strands import GaussianModelLatentStrands
    S, N, n_seg = 40, 9, 7
    gen = _generator(N)
    hair = GaussianModelLatentStrands(3, gen, None, fused=False, shared_appearance=shared)
    assert hair.num_guiding_strands == N                                    # None reads the generator's attribute
    hair.initialize_gaussians_hair(1)
    P = N * n_seg
    assert hair._xyz_gdn.shape == (P, 3) and hair._dir_gdn.shape == (P, 3)
    assert torch.equal(hair._xyz_gdn, hair._xyz[:P]) and hair._xyz_gdn.data_ptr() == hair._xyz.data_ptr()     # a view
    assert torch.equal(hair._dir_gdn, hair._dir.view(S, n_seg, 3)[:N].reshape(-1, 3))
    rows = P if hair.feature_rows_per_strand <= 1 else N
    assert hair._features_dc_gdn.shape == (rows, 1, 3) and hair._features_rest_gdn.shape == (rows, 15, 3)
    assert hair.get_features_gdn.shape == (rows, 16, 3)
    assert torch.equal(hair.get_features_gdn, torch.cat((hair._features_dc, hair._features_rest), dim=1)[:rows])
    for given, want in ((0, 0), (5, 5)):
        other = GaussianModelLatentStrands(3, _generator(N), None, fused=False, num_guiding_strands=given)
        assert other.num_guiding_strands == want
    plain = GaussianModelLatentStrands(3, _generator(), None, fused=False)   # without guides: the full tensors (:459-461, :480-482)
    assert plain.num_guiding_strands == 0
    plain.initialize_gaussians_hair(1)
    assert plain._xyz_gdn is plain._xyz and plain._dir_gdn is plain._dir
    assert plain._features_dc_gdn is plain._features_dc and plain._features_rest_gdn is plain._features_rest
    assert torch.equal(plain.get_features_gdn, torch.cat((plain._features_dc, plain._features_rest), dim=1))
    assert GaussianModelLatentStrands(3, lambda it: {}, None).num_guiding_strands == 0
