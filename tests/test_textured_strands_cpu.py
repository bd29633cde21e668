"""The textured strand generator (gaussianhaircut_amd/strand_generator.py, csrc/ghr_texstrands.h) without a GPU.

 1. the host-side pieces: frames orthonormal and right-handed with the identity on degenerate faces; root draws reproducible
    under a seed with area-weighted face counts; float64 taps against F.grid_sample(double) within 4 * 2^-24 * max|texture| (the
    only difference is the rounding of fx, fy to float32) -- the distance of F.grid_sample(float32) is printed, not asserted;
    the inverted lists against a numpy model, bit for bit.
 2. the composed form (fused=False) on CPU tensors against the float64 arbiter of tests/texstrands_cases.py.
 3. host walks of the five kernels, lane by lane (tests/hostsim/ghr_hostsim_texstrands.cpp), against the arbiter under
    1e-5 max|f64| + 3 |composed - f64|; pos and the lists bit for bit; the same walks in a stand-alone program built with
    -fsanitize=address,undefined (nothing sanitized is loaded here).
 4. the C ABI: four symbols declared and exported, every refusal answered before the runtime is touched, ABI 20.
 5. the module: the reference's tuples in shape and order, a GaussianModelLatentStrands iteration and
    GaussianModelStrands.create_from_generator on CPU tensors."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd import strand_generator as sg
from tests import helpers as hp
from tests import texstrands_cases as tc


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
def test_frames_are_orthonormal_right_handed_and_follow_u():
    verts, faces, uv = tc.scalp_grid()
    fr = sg.scalp_frames(verts, faces, uv)
    assert fr.shape == (faces.shape[0], 3, 3) and fr.dtype == torch.float32
    assert torch.equal(fr[-1], torch.eye(3))                               # the zero-area face
    M = fr[:-1].double()
    assert float((M.transpose(1, 2) @ M - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-6
    assert float((torch.linalg.det(M) - 1).abs().max()) < 1e-6             # right-handed
    t, b, nrm = M[..., 0], M[..., 1], M[..., 2]
    assert float((torch.linalg.cross(nrm, t) - b).abs().max()) < 1e-6
    # t is d position / d u inside the face's plane, normalised: solve the face's 2 x 2 UV system in float64
    v, f = verts.double(), faces[:-1]
    e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    d1, d2 = uv.double()[f[:, 1]] - uv.double()[f[:, 0]], uv.double()[f[:, 2]] - uv.double()[f[:, 0]]
    det = d1[:, 0] * d2[:, 1] - d2[:, 0] * d1[:, 1]
    dPdu = (d2[:, 1:2] * e1 - d1[:, 1:2] * e2) / det[:, None]
    assert float((F.normalize(dPdu, dim=-1) - t).abs().max()) < 1e-6
    assert float((nrm - F.normalize(torch.linalg.cross(e1, e2), dim=-1)).abs().max()) < 1e-6
    # a zero UV determinant: identity as well; a mirrored UV chart flips the raw tangent back along +u
    uv2 = uv.clone()
    uv2[faces[0]] = uv2[faces[0, 0]].clone()
    assert torch.equal(sg.scalp_frames(verts, faces, uv2)[0], torch.eye(3))
    mirrored = sg.scalp_frames(verts, faces[:, [0, 2, 1]], uv)[:-1].double()
    assert float((mirrored[..., 0] - t).abs().max()) < 1e-6 and float((mirrored[..., 2] + nrm).abs().max()) < 1e-6


def test_root_draws_are_reproducible_and_area_weighted():
    verts, faces, uv = tc.scalp_grid()
    Smax = 20000
    a = sg.sample_roots(verts, faces, uv, Smax, torch.Generator().manual_seed(5))
    b = sg.sample_roots(verts, faces, uv, Smax, torch.Generator().manual_seed(5))
    c = sg.sample_roots(verts, faces, uv, Smax, torch.Generator().manual_seed(6))
    for k in ("origins", "uvs", "face_idx", "local2world"):
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["face_idx"], c["face_idx"])
    assert a["origins"].shape == (Smax, 3) and a["uvs"].shape == (Smax, 2) and a["local2world"].shape == (Smax, 3, 3)
    v = verts.double()
    area = 0.5 * torch.linalg.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]]).norm(dim=-1)
    prob = area / area.sum()
    count = torch.bincount(a["face_idx"], minlength=faces.shape[0]).double()
    assert count[-1] == 0                                                   # the degenerate face weighs nothing
    sigma = torch.sqrt(Smax * prob * (1 - prob))
    assert bool(((count - Smax * prob).abs() <= 5 * sigma + 1e-9).all()), (count - Smax * prob) / sigma.clamp_min(1e-9)
    assert torch.equal(a["local2world"], sg.scalp_frames(verts, faces, uv)[a["face_idx"]])
    # every root lies in its face: its UV inside the face's UV triangle's bounds, its origin in the face's plane
    fuv = uv[faces[a["face_idx"]]]
    assert bool((a["uvs"] >= fuv.min(1).values - 1e-6).all()) and bool((a["uvs"] <= fuv.max(1).values + 1e-6).all())
    off = ((a["origins"].double() - v[faces[a["face_idx"], 0]]) * a["local2world"][..., 2].double()).sum(-1)
    assert float(off.abs().max()) < 1e-6
    bad = uv.clone()
    bad[3, 0] = float("nan")
    with pytest.raises(ValueError, match="not finite"):
        sg.sample_roots(verts, faces, bad, 4000, torch.Generator().manual_seed(1))
    with pytest.raises(ValueError, match="degenerate"):
        sg.sample_roots(verts, faces[-1:], uv, 4, torch.Generator().manual_seed(1))


@pytest.mark.parametrize("T", [1, 2, 3, 5, 16, 64, 255, 256])
def test_float64_taps_against_grid_sample_in_double(T):
    g = torch.Generator().manual_seed(T)
    Smax, C = 600, 3
    uvs = torch.cat([torch.rand(Smax - 8, 2, generator=g) * 2.2 - 1.1, tc.uvs_for("corners", 4, T, g), tc.uvs_for("centres", 4, T, g)])
    tex = torch.rand(1, C, T, T, generator=g) * 2 - 1
    taps = sg.texture_taps(uvs, T)
    idx = torch.arange(Smax)
    got = sg.sample_texture(tex.double(), taps, idx, fused=False)
    want = F.grid_sample(tex.double(), uvs.double().view(1, 1, Smax, 2), mode="bilinear", padding_mode="zeros", align_corners=False)[0, :, 0].t()
    f32 = F.grid_sample(tex, uvs.view(1, 1, Smax, 2), mode="bilinear", padding_mode="zeros", align_corners=False)[0, :, 0].t()
    err, err32 = float((got - want).abs().max()), float((f32.double() - want).abs().max())
    rng = float(tex.abs().max())
    print("T = %d: float64 taps %.3e of the range, F.grid_sample(float32) %.3e of the range" % (T, err / rng, err32 / rng))
    assert err <= 4 * 2.0 ** -24 * rng


def test_taps_drop_what_lies_outside_and_refuse_non_finite_uvs():
    T = 4
    taps = sg.texture_taps(torch.tensor([[-1.0, -1.0], [1.0, 1.0], [1e30, 0.0], [-3.0, 0.2], [-0.75, -0.75]]), T)
    assert taps.x0.tolist() == [-1, 3, T, -2, 0] and taps.y0.tolist()[:2] == [-1, 3]
    assert taps.fx.tolist()[:2] == [0.5, 0.5] and taps.fx[4] == 0.0
    assert taps.list.tolist() == [4 * 0 + 3, 4 * 4 + 0, 4 * 4 + 1, 4 * 4 + 2, 4 * 4 + 3, 4 * 1 + 0]
    assert taps.start.dtype == torch.int32 and taps.list.dtype == torch.int32 and int(taps.start[-1]) == 6
    with pytest.raises(ValueError, match="not finite"):
        sg.texture_taps(torch.tensor([[0.0, float("inf")]]), T)
    tex = torch.ones(1, 2, T, T)
    z = sg.sample_texture(tex, taps, torch.arange(5), fused=False)
    assert z[:, 0].tolist() == [0.25, 0.25, 0.0, 0.0, 1.0]
    bad = tex.clone()
    bad[0, :, 1, 3] = float("nan")                                          # root 2's dropped taps clamp onto these texels
    bad[0, :, 2, 3] = float("inf")
    assert sg.sample_texture(bad, taps, torch.arange(3), fused=False)[:, 0].tolist() == [0.25, 0.25, 0.0]
    with pytest.raises(ValueError, match="twice"):
        sg.sample_texture(tex, taps, torch.tensor([1, 2, 1]), fused=False)
    with pytest.raises(ValueError, match="outside"):
        sg.sample_texture(tex, taps, torch.tensor([5]), fused=False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sg.sample_texture(tex, taps, torch.arange(5), fused=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sg.strands_to_world(torch.zeros(2, 3, 3), torch.eye(3).expand(5, 3, 3), torch.zeros(5, 3), torch.arange(2), fused=True)


@pytest.mark.parametrize("name", sorted(tc.SHAPES))
def test_inverted_lists_against_the_numpy_model(name):
    c = tc.case(name)
    start, lst = tc.lists_numpy(c["taps"].x0.numpy(), c["taps"].y0.numpy(), c["T"])
    assert c["taps"].start.numpy().tobytes() == start.tobytes() and c["taps"].list.numpy().tobytes() == lst.tobytes()
    if c["mode"] == "beyond":
        assert lst.size == 0 and float(c["r64"]["z"].abs().max()) == 0.0
    if c["mode"] == "one" and c["T"] > 1:
        lens = np.diff(start)
        assert sorted(lens[lens > 0].tolist()) == [c["Smax"]] * 4


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def _composed(c, dtype=torch.float32, d_p=True, d_pl=True):
    tex = c["texture"].to(dtype).requires_grad_(True)
    z = sg.sample_texture(tex, c["taps"], c["idx"], fused=False)
    (d_tex,) = torch.autograd.grad(z, tex, c["d_z"].to(dtype))
    v = c["v"].to(dtype).requires_grad_(True)
    p, pl = sg.strands_to_world(v, c["local2world"], c["origins"], c["idx"], c["scale"], fused=False, return_local=True)
    obj = (p * c["d_p"].to(dtype)).sum() * float(d_p) + (pl * c["d_pl"].to(dtype)).sum() * float(d_pl)
    (d_v,) = torch.autograd.grad(obj, v)
    return dict(z=z.detach(), d_texture=d_tex, p=p.detach(), p_local=pl.detach(), d_v=d_v)


_COMPOSED = {}


def composed(name):
    if name not in _COMPOSED:
        _COMPOSED[name] = _composed(tc.case(name))
    return _COMPOSED[name]


@pytest.mark.parametrize("name", sorted(tc.SHAPES))
def test_composed_form_against_the_arbiter(name):
    c = tc.case(name)
    got = composed(name)
    for k in ("z", "d_texture", "p", "p_local", "d_v"):
        tc.assert_within("composed " + k, got[k], c["r64"][k], c["r64"][k])   # 1e-5 of the largest value, nothing more
    in64 = _composed(c, torch.float64)
    for k in ("z", "d_texture", "p", "p_local", "d_v"):                      # and in float64 it IS the arbiter, to rounding
        assert float((in64[k] - c["r64"][k]).abs().max()) <= 1e-12 * max(float(c["r64"][k].abs().max()), 1.0), k


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
DEPS = ["ghr_hostsim_texstrands.cpp", "ghr_texstrands.h", "ghr_sds.h", "ghr_haar.h"]


@pytest.fixture(scope="module")
def sim():
    L = ctypes.CDLL(hp.compile_hostsim("libghr_hostsim_texstrands.so", "ghr_hostsim_texstrands.cpp", ["-O2", "-fPIC", "-shared"], DEPS))
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.ghrsim_ts_fetch.argtypes = [i32] * 4 + [vp] * 7
    L.ghrsim_ts_fetch_backward.argtypes = [i32] * 4 + [vp] * 4 + [i32] + [vp] * 4
    L.ghrsim_ts_world.argtypes = [i32] * 3 + [vp] * 4 + [f32, vp, vp]
    L.ghrsim_ts_world_backward.argtypes = [i32] * 3 + [vp, vp, f32, vp, vp, vp]
    L.ghrsim_ts_weight.argtypes, L.ghrsim_ts_weight.restype = [i32, f32, f32], f32
    L.ghrsim_ts_tap_in.argtypes = [i32] * 4
    assert L.ghrsim_ts_wave() == 64
    return L


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _np(t, dtype=np.float32):
    return np.ascontiguousarray(t.detach().cpu().numpy().astype(dtype))


def _sim_case(sim, c, d_p=True, d_pl=True):
    Smax, S, T, C, n = c["Smax"], c["S"], c["T"], c["C"], c["n"]
    tp = c["taps"]
    a = dict(tex=_np(c["texture"]), x0=_np(tp.x0, np.int32), y0=_np(tp.y0, np.int32), fx=_np(tp.fx), fy=_np(tp.fy),
             start=_np(tp.start, np.int32), list=_np(tp.list, np.int32), idx=_np(c["idx"], np.int64), v=_np(c["v"]),
             frames=_np(c["local2world"]), origins=_np(c["origins"]), d_z=_np(c["d_z"]), d_p=_np(c["d_p"]), d_pl=_np(c["d_pl"]))
    z = np.full((S, C), np.nan, np.float32)
    sim.ghrsim_ts_fetch(Smax, S, T, C, _p(a["tex"]), _p(a["x0"]), _p(a["y0"]), _p(a["fx"]), _p(a["fy"]), _p(a["idx"]), _p(z))
    pos, d_tex = np.full(Smax, -7, np.int32), np.full((1, C, T, T), np.nan, np.float32)
    sim.ghrsim_ts_fetch_backward(Smax, S, T, C, _p(a["fx"]), _p(a["fy"]), _p(a["start"]), _p(a["list"]), int(a["list"].size), _p(a["idx"]),
                                 _p(a["d_z"]), _p(pos), _p(d_tex))
    p, pl = np.full((S, n + 1, 3), np.nan, np.float32), np.full((S, n + 1, 3), np.nan, np.float32)
    sim.ghrsim_ts_world(Smax, S, n, _p(a["v"]), _p(a["frames"]), _p(a["origins"]), _p(a["idx"]), 1.0 / c["scale"], _p(p), _p(pl))
    d_v = np.full((S, n, 3), np.nan, np.float32)
    sim.ghrsim_ts_world_backward(Smax, S, n, _p(a["frames"]), _p(a["idx"]), 1.0 / c["scale"], _p(a["d_p"]) if d_p else None,
                                 _p(a["d_pl"]) if d_pl else None, _p(d_v))
    T_ = torch.from_numpy
    return dict(z=T_(z), d_texture=T_(d_tex), pos=T_(pos), p=T_(p), p_local=T_(pl), d_v=T_(d_v)), a


@pytest.mark.parametrize("name", sorted(tc.SHAPES))
def test_host_walks_of_the_five_kernels(sim, name):
    c = tc.case(name)
    got, _ = _sim_case(sim, c)
    comp = composed(name)
    assert torch.equal(got["pos"].long(), c["r64"]["pos"])
    for k in ("z", "d_texture", "p", "p_local", "d_v"):
        tc.assert_within("host walk " + k, got[k], c["r64"][k], comp[k])
    assert torch.equal(got["z"], comp["z"])                                 # the fetch: the same float32 expression, no contraction
    assert torch.equal(got["p"][:, 0], c["origins"][c["idx"]]) and float(got["p_local"][:, 0].abs().max()) == 0.0


@pytest.mark.parametrize("name", ["L2", "L66", "L130", "Smax65-S32"])
def test_host_walk_of_each_cotangent_alone(sim, name):
    c = tc.case(name)
    for kw in (dict(d_p=True, d_pl=False), dict(d_p=False, d_pl=True)):
        got, _ = _sim_case(sim, c, **kw)
        r64, comp = tc.restate(c, **kw), _composed(c, **kw)
        assert float(r64["d_v"].abs().max()) > 0
        tc.assert_within("host walk d_v %s" % kw, got["d_v"], r64["d_v"], comp["d_v"])


def test_host_walk_texture_gradient_does_not_depend_on_the_order_of_the_draw(sim):
    c = dict(tc.case("C65"))
    a, _ = _sim_case(sim, c)
    perm = torch.randperm(c["S"], generator=torch.Generator().manual_seed(2))
    c["idx"], c["d_z"] = c["idx"][perm], c["d_z"][perm]
    b, _ = _sim_case(sim, c)
    assert a["d_texture"].numpy().tobytes() == b["d_texture"].numpy().tobytes()


def test_per_element_functions(sim):
    for k in range(4):
        for fx, fy in ((0.0, 0.0), (1.0, 0.25), (0.3, 0.7)):
            x, y, one = np.float32(fx), np.float32(fy), np.float32(1)
            assert sim.ghrsim_ts_weight(k, fx, fy) == (x if k & 1 else one - x) * (y if k >> 1 else one - y)
            assert sim.ghrsim_ts_weight(k, fx, fy) == float(sg.tap_weight(k, torch.tensor(fx), torch.tensor(fy)))
    big = 2 ** 31 - 1
    for x0, y0, T, want in ((-1, -1, 4, [0, 0, 0, 1]), (3, 3, 4, [1, 0, 0, 0]), (0, 0, 1, [1, 0, 0, 0]), (-1, 0, 1, [0, 1, 0, 0]),
                            (big, 0, 4, [0, 0, 0, 0]), (-big - 1, -big - 1, 4, [0, 0, 0, 0]), (2, -2, 4, [0, 0, 0, 0])):
        assert [sim.ghrsim_ts_tap_in(x0, y0, k, T) for k in range(4)] == want
    assert sim.ghrsim_ts_tile_bytes() == 64 * 193 * 4


SELFCHECK = ["T1", "T2", "T65", "C1", "C129", "Smax1-S1", "Smax300-S150", "L2", "L130", "one", "corners", "beyond", "leftout"]


def test_sanitized_stand_alone_program_runs_the_walks_clean(sim, tmp_path):
    """ghr_texstrands_selfcheck: the walks under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own
    (exact-size buffers)."""
    san = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    if os.path.basename(hp.host_cxx()) == "g++":
        san += ["-static-libasan", "-static-libubsan"]
    exe = hp.compile_hostsim("ghr_texstrands_selfcheck_san", "ghr_texstrands_selfcheck.cpp", san, DEPS)
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as fh:
        for name in SELFCHECK:
            c = tc.case(name)
            got, a = _sim_case(sim, c)
            tol = 1e-5 * max(float(c["r64"][k].abs().max()) for k in ("z", "d_texture", "p", "d_v")) + 1e-30
            fh.write(np.array([c["Smax"], c["S"], c["T"], c["C"], c["n"], a["list"].size], np.int32).tobytes())
            fh.write(np.array([1.0 / c["scale"], tol], np.float32).tobytes())
            for k in ("tex", "x0", "y0", "fx", "fy", "start", "list", "idx", "v", "frames", "origins", "d_z", "d_p", "d_pl"):
                fh.write(a[k].tobytes())
            for k in ("z", "d_texture", "p", "d_v"):
                fh.write(_np(got[k]).tobytes())
            fh.write(_np(c["r64"]["pos"], np.int32).tobytes())
    res = subprocess.run([exe, path], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "%d cases ok" % len(SELFCHECK) in res.stdout and "runtime error" not in res.stderr, res.stdout + res.stderr


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
NAMES = ("ghr_ts_fetch", "ghr_ts_fetch_backward", "ghr_ts_world", "ghr_ts_world_backward")


def test_c_abi_symbols_are_declared_and_exported():
    L = _lib.lib()
    with open(os.path.join(hp.ROOT, "include", "ghr.h")) as fh:
        hdr = fh.read()
    for n in NAMES:
        assert re.search(r"\bint %s\(" % n, hdr) and n in _lib.EXPORTS and hasattr(L, n), n
    assert L.ghr_abi_version() == 20 == _lib.ABI_VERSION and "#define GHR_ABI_VERSION 20" in hdr
    assert "ghr_texstrands.h" in _lib.HEADERS


def test_c_abi_refusals_launch_nothing():
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before anything is enqueued
    INV = _lib.GHR_E_INVALID

    def fetch(Smax=9, S=5, T=4, C=3, **kw):
        names = ("texture", "x0", "y0", "fx", "fy", "idx", "z")
        a = dict(dict.fromkeys(names, fake), **kw)
        return L.ghr_ts_fetch(None, Smax, S, T, C, *[a[k] for k in names])

    def fetch_b(Smax=9, S=5, T=4, C=3, list_len=7, **kw):
        names = ("fx", "fy", "start", "list", "idx", "d_z", "pos", "d_texture")
        a = dict(dict.fromkeys(names, fake), **kw)
        return L.ghr_ts_fetch_backward(None, Smax, S, T, C, a["fx"], a["fy"], a["start"], a["list"], list_len, a["idx"], a["d_z"], a["pos"],
                                       a["d_texture"])

    def world(Smax=9, S=5, n=3, **kw):
        names = ("v", "local2world", "origins", "idx", "p", "p_local")
        a = dict(dict.fromkeys(names, fake), **kw)
        return L.ghr_ts_world(None, Smax, S, n, a["v"], a["local2world"], a["origins"], a["idx"], 1.0, a["p"], a["p_local"])

    def world_b(Smax=9, S=5, n=3, **kw):
        names = ("local2world", "idx", "d_p", "d_p_local", "d_v")
        a = dict(dict.fromkeys(names, fake), **kw)
        return L.ghr_ts_world_backward(None, Smax, S, n, a["local2world"], a["idx"], 1.0, a["d_p"], a["d_p_local"], a["d_v"])

    sizes = [(dict(S=0), b"S < 1"), (dict(S=-3), b"S < 1"), (dict(S=10), b"S > Smax")]
    tex_sizes = sizes + [(dict(T=0), b"T < 1"), (dict(C=0), b"C < 1"), (dict(T=16384, C=9), b"32-bit"), (dict(T=20000), b"32-bit")]
    for fn, cases in ((fetch, tex_sizes + [(dict(texture=None), b"texture is NULL"), (dict(x0=None), b"tap buffer"), (dict(y0=None), b"tap buffer"),
                                           (dict(fx=None), b"tap buffer"), (dict(fy=None), b"tap buffer"), (dict(idx=None), b"idx is NULL"),
                                           (dict(z=None), b"z is NULL")]),
                      (fetch_b, tex_sizes + [(dict(fx=None), b"tap buffer"), (dict(fy=None), b"tap buffer"), (dict(start=None), b"start or list"),
                                             (dict(list=None), b"start or list"), (dict(list_len=-1), b"list_len"), (dict(list_len=37), b"list_len"),
                                             (dict(idx=None), b"idx is NULL"), (dict(d_z=None), b"d_z is NULL"), (dict(pos=None), b"pos is NULL"),
                                             (dict(d_texture=None), b"d_texture is NULL")]),
                      (world, sizes + [(dict(n=0), b"n < 1"), (dict(v=None), b"v is NULL"), (dict(local2world=None), b"local2world or origins"),
                                       (dict(origins=None), b"local2world or origins"), (dict(idx=None), b"idx is NULL"), (dict(p=None), b"p is NULL"),
                                       (dict(Smax=2 ** 30, S=2 ** 29, n=3), b"32-bit")]),
                      (world_b, sizes + [(dict(n=0), b"n < 1"), (dict(local2world=None), b"local2world is NULL"), (dict(idx=None), b"idx is NULL"),
                                         (dict(d_p=None, d_p_local=None), b"both NULL"), (dict(d_v=None), b"d_v is NULL")])):
        for kw, why in cases:
            assert fn(**kw) == INV, (fn.__name__, kw)
            assert why in L.ghr_last_error(), (fn.__name__, kw, L.ghr_last_error())


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_the_reference_tuples_in_shape_and_order():
    gen = tc.tiny_generator(fused=False)
    S, Smax, L, T, Cg, Ca = 64, 200, 8, 16, 6, 5
    assert [n for n, _ in gen.named_parameters() if not n.startswith(("strand_decoder", "color_decoder"))] == ["texture"]
    assert gen.texture.shape == (1, Cg + Ca, T, T) and set(dict(gen.named_buffers())) == {
        "origins", "uvs", "face_idx", "local2world", "tap_x0", "tap_y0", "tap_fx", "tap_fy", "tap_start", "tap_list"}
    assert "strand_decoder.lin.weight" in gen.state_dict() and "color_decoder.lin.bias" in gen.state_dict()
    fresh = sg.TexturedStrands(tc.scalp_grid(), tc.Linear3(Cg, L - 1), num_strands=3, max_num_strands=5, texture_size=2, geometry_channels=Cg,
                               appearance_channels=Ca)
    assert float(fresh.texture.abs().max()) == 0.0 and set(fresh(0)) == {"points"}
    p, uvs, l2w, p_local, z_geom, z_app, dd = gen.forward_reference(1)
    idx = gen.last_idx
    assert idx.shape == (S,) and int(torch.unique(idx).numel()) == S and int(idx.max()) < Smax
    assert p.shape == (S, L, 3) and uvs.shape == (S, 2) and l2w.shape == (S, 3, 3) and p_local.shape == (S, L, 3)
    assert z_geom.shape == (S, Cg) and z_app.shape == (S, Ca) and set(dd) == {"L_diff"} and dd["L_diff"].dim() == 0
    assert torch.equal(uvs, gen.uvs[idx]) and torch.equal(l2w, gen.local2world[idx]) and torch.equal(p[:, 0], gen.origins[idx])
    assert p.requires_grad and dd["L_diff"].requires_grad
    want = gen.origins[idx][:, None] + torch.einsum("sab,sjb->sja", l2w, p_local)
    assert float((p - want).abs().max()) < 1e-6
    out = gen.forward_inference(17)
    assert len(out) == 6 and out[0].shape == (17, L, 3) and out[5].shape == (17, Ca) and not out[0].requires_grad
    with pytest.raises(ValueError, match="num_strands"):
        gen.forward_inference(Smax + 1)
    d = gen(3)
    assert set(d) == {"points", "features", "orient_conf", "L_diff"}
    assert d["points"].shape == (S, L, 3) and d["features"].shape == (S, 48) and d["orient_conf"].shape == (S, 1)
    # draws are reproducible under the module's generator and differ from call to call
    a, b = tc.tiny_generator(fused=False), tc.tiny_generator(fused=False)
    i1, i2 = a.draw(), a.draw()
    assert torch.equal(i1, b.draw()) and not torch.equal(i1, i2)
    # the whole chain in float64 is the arbiter's chain: texture.grad arrives whole
    d["points"].square().sum().backward()
    assert gen.texture.grad.shape == gen.texture.shape and float(gen.texture.grad[:, :Cg].abs().max()) > 0
    assert float(gen.texture.grad[:, Cg:].abs().max()) == 0.0


def test_a_latent_strands_iteration_and_create_from_generator_on_cpu_tensors():
    from types import SimpleNamespace
    from gaussianhaircut_amd.scene.gaussian_model_latent_strands import GaussianModelLatentStrands
    from gaussianhaircut_amd.scene.gaussian_model_strands import GaussianModelStrands
    from gaussianhaircut_amd.strand_prior import StrandPrior
    gen = tc.tiny_generator(fused=True)                                     # CPU tensors: the composed form is the only one
    S, L = 64, 8
    hair = GaussianModelLatentStrands(3, gen, None)                       # the colour decoder is the generator's submodule
    hair.initialize_gaussians_hair(1)
    P = S * (L - 1)
    assert hair._xyz.shape == (P, 3) and hair._features_dc.shape == (P, 1, 3) and hair._features_rest.shape == (P, 15, 3)
    assert hair._orient_conf.shape == (P, 1) and hair.LDiff is not None and hair.LDiff.requires_grad
    (hair._xyz.sum() + hair._features_dc.sum() + hair.LDiff).backward()
    assert float(gen.texture.grad.abs().max()) > 0
    hair.training_setup(SimpleNamespace(iterations=10, latent_lr=1e-3))
    got = {id(q) for g in hair.optimizer.param_groups for q in g["params"]}
    assert id(gen.texture) in got and all(id(q) in got for q in gen.strand_decoder.parameters())
    assert "texture" in hair.capture()[2] and "tap_list" in hair.capture()[2]
    # the strand stage's model out of the generator
    model = GaussianModelStrands(3).create_from_generator(gen, 20)
    n = L - 1
    assert model._dirs.shape == (20, n, 3) and model._dirs.requires_grad and model.pts_origins.shape == (20, 1, 3)
    assert model._features_dc.shape == (20 * n, 1, 3) and model._features_rest.shape == (20 * n, 15, 3) and model._orient_conf.shape == (20 * n, 1)
    assert model.uvs.shape == (20, 2) and model.local2world.shape == (20, 3, 3) and model.z_geom.shape == (20, 6) and model.p_local.shape == (20, L, 3)
    idx = gen.last_idx
    assert torch.equal(model.pts_origins[:, 0], gen.origins[idx]) and torch.equal(model.uvs, gen.uvs[idx])
    assert float((model._pts - gen.origins[idx][:, None] - torch.einsum("sab,sjb->sja", model.local2world, model.p_local)).abs().max()) < 1e-6
    assert torch.equal(model._features_dc[0], model._features_dc[n - 1]) and not torch.equal(model._features_dc[0], model._features_dc[n])
    assert model.num_strands == 20 and model.strand_length == L and model._xyz.shape == (20 * n, 3)
    prior = StrandPrior(lambda e: e.flatten(1)[:, :4], lambda t: (t ** 2).mean(dim=(1, 2, 3)), model.uvs, model.local2world, 3, 2.0,
                        num_guiding=8, channels=4, fused=False)
    assert bool(torch.isfinite(prior(model._dirs)))
    with pytest.raises(ValueError, match="colour decoder"):
        GaussianModelStrands(3).create_from_generator(sg.TexturedStrands(tc.scalp_grid(), tc.Linear3(6, 7), num_strands=3, max_num_strands=5,
                                                                         texture_size=2, geometry_channels=6, appearance_channels=5), 3)
