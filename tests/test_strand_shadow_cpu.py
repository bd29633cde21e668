"""Self-shadowing of the strand preview (csrc/ghr_strandview.h "Self-shadowing", gaussianhaircut_amd/strand_view.py)
without a GPU.

Every result is an integer, a byte or a float32 compared by its bits: every comparison is exact.
 1. the numpy float32 MODEL (tests/strand_shadow_cases.py) against hand-derived values: the ladder of exact depths, the lookups on
    it, the head as an occluder;
 2. the product's own per-element functions and a host walk of the light pass with k_sv_layers' two walks
    (tests/hostsim/ghr_hostsim_strandshadow.cpp, every index checked) against the model, bit for bit, on every map and frame; the
    same through a stand-alone program built with -fsanitize=address,undefined (nothing sanitized is loaded here);
 3. the PyTorch comparator (fused=False) on CPU tensors against the model; render_strands with a map that sees nothing;
 4. light_view against a float64 restatement; the refusals of the C ABI; the video tool with --shadows."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd import strand_view as sv
from tests import helpers as hp
from tests import strand_shadow_cases as ss
from tests import strand_view_cases as sc
from tests.test_strand_view_cpu import SV_HEADERS, _p, _same_bits, _shading_bytes

DEPS = ["ghr_hostsim_strandshadow.cpp"] + SV_HEADERS
MAPS, FRAMES = ss.MAPS, ss.FRAMES


@pytest.fixture(scope="module")
def sim():
    L = ctypes.CDLL(hp.compile_hostsim("libghr_hostsim_strandshadow.so", "ghr_hostsim_strandshadow.cpp", ["-O2", "-fPIC", "-shared"], DEPS))
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.ghrsim_ss_opacity.argtypes = [i32, i32, vp, vp, f32, i32, i32, f32, f32, vp, vp, vp, vp]
    L.ghrsim_ss_lookup.argtypes = [i32, vp, vp, f32, i32, i32, f32, f32, f32, vp, vp, vp, vp, vp]
    L.ghrsim_ss_shade.argtypes = [i32, i32, vp, i32, vp, i32, vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, f32, i32, i32, f32, f32, f32,
                                  vp, vp, vp, vp]
    assert L.ghrsim_ss_chunk() == ss.CHUNK
    assert L.ghrsim_ss_shadow_bytes() == ctypes.sizeof(_lib.StrandViewShadow) == 96
    return L


def _ladder_map(m):
    pts = ss.ladder(m)
    Ml = sc.view_screen_w(1, 1)
    q0, layers = ss.model_opacity(pts, Ml, 1, 1, 1.0, 1.0)
    return dict(Ml=Ml, Hl=1, Wl=1, layer=1.0, q0=q0, layers=layers, qfl=None)


def _torch_map(sm, dev="cpu"):
    up = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)  # noqa: E731
    return sv.ShadowMap(sm["Ml"], sm["Hl"], sm["Wl"], float(sc.NEAR), up(sm["q0"]), up(sm["layers"].view(np.int32)), up(sm["qfl"]),
                        float(sm["layer"]))


def _frame_kwargs(c):
    return dict(mesh=None if c["v"] is None else (c["v"], c["f"]), colors=c["base"], mode=("kajiya", "tangent")[c["mode"]],
                supersample=c["s"], half_width=c["r"], near=float(sc.NEAR), eye=c["sh"]["eye"], light=c["sh"]["light"],
                shadow_kappa=c["kappa"], shadow_bias=c["bias"])


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", ss.LADDER_M)
def test_model_meets_the_hand_derived_ladder(m):
    """segments at z = 1, 2, 4, 8, 16 over one texel, d = 1: u = 0, 1, 3, 7, 15 exactly, so the counts are (m_1, m_2, m_4, m_8 + m_16)"""
    sm = _ladder_map(m)
    assert sm["q0"].tolist() == [[1.0]] and sm["layers"].dtype == np.uint32
    assert sm["layers"].tolist() == [[[m[0], m[1], m[2], m[3] + m[4]]]]


def test_model_meets_the_hand_derived_lookups():
    sm = _ladder_map((4, 2, 0, 0, 0))
    P = np.stack([ss.ladder_point(1.5), ss.ladder_point(1.0), ss.ladder_point(2.0), ss.ladder_point(16.0), ss.ladder_point(32.0),
                  ss.ladder_point(0.75),                      # in front of the front plane: u < 0
                  ss.ladder_point(1.5, sx=1.0),               # lx == Wl: outside
                  ss.ladder_point(1.5, sy=-0.25),             # above the map
                  ss.ladder_point(0.0005),                    # behind near
                  np.array([np.nan, 0.75, 1.5], np.float32)])
    n, Tr, branch, behind = ss.model_lookup(P, sm, kappa=0.5)
    assert n.tolist() == [2.0, 0.0, 4.0, 6.0, 6.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert Tr.tolist() == [0.5, 1.0, float(np.float32(1) / np.float32(3)), 0.25, 0.25, 1.0, 1.0, 1.0, 1.0, 1.0]
    assert branch.tolist() == [0, -1, 1, 3, 3, -1, -1, -1, -1, -1] and not behind.any()
    # the four branches on a full ladder, each at its middle: c0 / 2, c0 + n1 / 2, c1 + n2 / 2, c2 + n3 / 2
    sm = _ladder_map((3, 5, 2, 4, 4))
    n, _, branch, _ = ss.model_lookup(np.stack([ss.ladder_point(z) for z in (1.5, 3.0, 6.0, 12.0)]), sm)
    assert branch.tolist() == [0, 1, 2, 3] and n.tolist() == [1.5, 5.5, 9.0, 14.0]


def test_model_puts_the_head_between_light_and_strands():
    """the sphere under the oblique light, 64 x 64 texels: a root on the far side has Tr == 0, a root on the lit side is kept by the
    bias (the roots sit ON the sphere, the mesh is inscribed; a texel holds the face's depth at its centre only, so towards the
    outline the slope of the sphere across a texel outgrows any bias: the lit roots and faces are taken within 45 degrees of the light, where
    the sphere's depth changes by less than a texel's width across a texel, 0.05 against the bias's 0.02 x 2.1 = 0.04 at half of it); a head
    face under hair on the lit side is shadowed by it"""
    pts = sc.hair(200, 4, 12, through=False)
    Ml = sc.view_oblique(64, 64)
    qfl = sc._mesh_planes("sphere", "oblique", 64, 64, 1)[1]
    q0, layers = ss.model_opacity(pts, Ml, 64, 64, 1.0, 0.05)
    sm = dict(Ml=Ml, Hl=64, Wl=64, layer=0.05, q0=q0, layers=layers, qfl=qfl)
    assert (qfl > 0).sum() > 500
    eye = np.array([1.9, 1.3, -1.6])
    to_light = eye / np.linalg.norm(eye)
    roots = pts[:, 0]
    side = roots.astype(np.float64) @ to_light
    _, Tr, _, behind = ss.model_lookup(roots, sm, ss.KAPPA, ss.BIAS)
    lit, far = side > 0.7, side < -0.3
    assert lit.sum() >= 20 and far.sum() >= 40
    assert behind[far].all() and (Tr[far] == 0).all()
    assert not behind[lit].any() and (Tr[lit] > 0).all()
    v, f = sc.meshes()["sphere"]
    f = np.asarray(f, np.int64)
    cen = ((v[f[:, 0]] + v[f[:, 1]]) + v[f[:, 2]]) / np.float32(3)
    n, Tr, _, behind = ss.model_lookup(cen, sm, ss.KAPPA, ss.BIAS)
    front, back = cen.astype(np.float64) @ to_light > 0.7, cen.astype(np.float64) @ to_light < -0.3
    assert not behind[front].any() and behind[back].all()         # a lit face is not in its own shadow (the bias)
    assert (n[front] > 0).sum() > 100 and (Tr[front] < 1).any()   # and hair shadows some of them
    # the frames of the other tests meet every branch of the lookup, on strand pixels (0 .. 4) and on head pixels (10 .. 14)
    c, c2 = ss.frame("sphere-48x64-ss2"), ss.frame("sphere-48x64-noqfl")
    assert {0, 1, 2, 3, 4} <= c["branches"] and {10, 11, 14} <= c["branches"] and {10, 11, 12, 13} <= c2["branches"]
    assert (c["rgb"] != c["plain"]).any(axis=2).mean() > 0.2


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MAPS)
def test_host_sim_equals_the_model_bit_for_bit(sim, name):
    c = ss.light_map(name)
    Hl, Wl = c["Hl"], c["Wl"]
    S, L = c["points"].shape[:2]
    q0, layers = np.full((Hl, Wl), 7, np.float32), np.full((Hl, Wl, 4), 7, np.uint32)
    tiles = np.zeros(((Hl + 15) // 16) * ((Wl + 15) // 16), np.uint32)
    n_big = np.zeros(1, np.uint32)
    assert sim.ghrsim_ss_opacity(S, L, _p(c["points"]), _p(c["Ml"]), float(sc.NEAR), Hl, Wl, c["rl"], c["layer"], _p(q0), _p(layers),
                                 _p(tiles), _p(n_big)) == 0
    assert _same_bits(q0, c["q0"]) and _same_bits(layers, c["layers"])
    if name.startswith(("stack", "dups")):
        K = int(name.lstrip("stackdup"))
        assert tiles[1 * 3 + 1] == K + (1 if name.startswith("dups") else 0) and tiles.sum() == tiles[4] and n_big[0] == 0
        assert int(layers[24, 24].sum()) == tiles[4]          # a texel every record of the tile covers: each one counted once
    if name == "long-80x96":
        assert n_big[0] == 2 and tiles.min() >= 2
    if name == "long-40x48":
        assert n_big[0] == 0
    if name.startswith("singles"):                            # all at w = 1: a tie for q0, everything in layer 0
        assert set(np.unique(q0).tolist()) <= {0.0, 1.0} and not layers[..., 1:].any() and layers[..., 0].max() >= (2 if Hl > 1 else 1)
    if name.startswith("empty"):
        assert not q0.any() and not layers.any() and not tiles.any()
    if name.startswith("dropped"):
        ref = sc.model_strand_winner(c["points"], c["Ml"], Hl, Wl, c["rl"], return_cover_count=True)
        assert np.array_equal(layers.sum(2), ref[3]) and _same_bits(q0, ref[2])   # the counts are the covering segments; q0 the winner's qs


def test_host_sim_lookup_equals_the_model(sim):
    for sm, kappa, P in ((_ladder_map((4, 2, 0, 0, 0)), 0.5, np.stack([ss.ladder_point(z) for z in (1.5, 1.0, 2.0, 16.0, 0.75, 0.0005)] +
                                                                        [ss.ladder_point(1.5, sx=1.0), np.full(3, np.nan, np.float32)])),
                         (ss.frame("sphere-48x64-ss2")["sm"], 0.2, ss.frame("sphere-48x64-ss2")["points"].reshape(-1, 3)),
                         (ss.frame("small-17x33")["sm"], 1.0, ss.frame("small-17x33")["points"].reshape(-1, 3))):
        P = np.ascontiguousarray(P, np.float32)
        n, tr = np.full(len(P), 7, np.float32), np.full(len(P), 7, np.float32)
        sim.ghrsim_ss_lookup(len(P), _p(P), _p(sm["Ml"]), float(sc.NEAR), sm["Hl"], sm["Wl"], sm["layer"], kappa, ss.BIAS, _p(sm["q0"]),
                             _p(sm["layers"]), _p(sm["qfl"]), _p(n), _p(tr))
        want = ss.model_lookup(P, sm, kappa, ss.BIAS)
        assert _same_bits(n, want[0]) and _same_bits(tr, want[1])


def _sim_shade(sim, c):
    H, W = c["rgb"].shape[:2]
    S, L = c["points"].shape[:2]
    V, F = (len(c["v"]), len(c["f"])) if c["v"] is not None else (0, 0)
    sm = c["sm"]
    seg, t, face = c["planes"]
    rgb = np.full((H, W, 3), 7, np.uint8)
    shb = np.frombuffer(_shading_bytes(c["sh"]), np.uint8).copy()
    sim.ghrsim_ss_shade(S, L, _p(c["points"]), V, _p(c["v"]), F, _p(c["f"]), H, W, _p(seg), _p(face), _p(t), c["mode"], _p(shb),
                        _p(c["base"]), _p(sm["Ml"]), float(sc.NEAR), sm["Hl"], sm["Wl"], sm["layer"], c["kappa"], c["bias"],
                        _p(sm["q0"]) if sm["q0"].size else None, _p(sm["layers"]) if sm["q0"].size else None, _p(sm["qfl"]), _p(rgb))
    return rgb


@pytest.mark.parametrize("name", FRAMES)
def test_host_sim_shade_equals_the_model(sim, name):
    c = ss.frame(name)
    assert _same_bits(_sim_shade(sim, c), c["rgb"])
    if name in ("tangent-17x33", "empty-map-15x17"):
        assert _same_bits(c["rgb"], c["plain"])                 # tangent mode is untouched; a map without texels shadows nothing


def test_sanitized_stand_alone_program_runs_the_cases_clean(tmp_path):
    """ghr_strandshadow_selfcheck: the per-element functions and the two-walk light pass under AddressSanitizer and
    UndefinedBehaviorSanitizer, as a program of its own (exact-size buffers)."""
    san = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    if os.path.basename(hp.host_cxx()) == "g++":
        san += ["-static-libasan", "-static-libubsan"]
    exe = hp.compile_hostsim("ghr_strandshadow_selfcheck_san", "ghr_strandshadow_selfcheck.cpp", san, DEPS)
    path = str(tmp_path / "cases.bin")
    raw = lambda a: np.ascontiguousarray(a).tobytes()  # noqa: E731
    with open(path, "wb") as fh:
        for name in MAPS:
            c = ss.light_map(name)
            S, L = c["points"].shape[:2]
            fh.write(raw(np.array([1, S, L, c["Hl"], c["Wl"]], np.int32)))
            fh.write(raw(np.concatenate([c["Ml"], [sc.NEAR, c["rl"], c["layer"]]]).astype(np.float32)))
            fh.write(raw(c["points"]) + raw(c["q0"]) + raw(c["layers"]))
        for name in FRAMES:
            c = ss.frame(name)
            sm = c["sm"]
            S, L = c["points"].shape[:2]
            H, W = c["rgb"].shape[:2]
            mesh = c["v"] is not None
            fh.write(raw(np.array([2, S, L, H, W, len(c["v"]) if mesh else 0, len(c["f"]) if mesh else 0, int(mesh), c["mode"],
                                   int(c["base"] is not None), sm["Hl"], sm["Wl"], int(sm["qfl"] is not None)], np.int32)))
            fh.write(raw(np.concatenate([sm["Ml"], [sc.NEAR, sm["layer"], c["kappa"], c["bias"]]]).astype(np.float32)))
            fh.write(_shading_bytes(c["sh"]))
            seg, t, face = c["planes"]
            arrs = [c["points"]] + ([c["v"], c["f"]] if mesh else []) + ([c["base"]] if c["base"] is not None else [])
            arrs += [seg, face, t, sm["q0"], sm["layers"]] + ([sm["qfl"]] if sm["qfl"] is not None else []) + [c["rgb"]]
            fh.write(b"".join(raw(a) for a in arrs))
    res = subprocess.run([exe, path], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "%d maps and %d frames ok" % (len(MAPS), len(FRAMES)) in res.stdout and "runtime error" not in res.stderr, res.stdout + res.stderr


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MAPS)
def test_torch_comparator_equals_the_model_on_cpu_tensors(name):
    c = ss.light_map(name)
    got = sv.strand_shadow_map(c["points"], c["Ml"], c["Hl"], c["Wl"], mesh=None if c["v"] is None else (c["v"], c["f"]),
                               half_width=c["rl"], layer=c["layer"], near=float(sc.NEAR), fused=False)
    assert got.q0.dtype == torch.float32 and got.layers.dtype == torch.int32 and tuple(got.layers.shape) == (c["Hl"], c["Wl"], 4)
    assert _same_bits(got.q0.numpy(), c["q0"]) and _same_bits(got.layers.numpy().view(np.uint32), c["layers"])
    if c["v"] is not None:
        assert _same_bits(got.qfl.numpy(), c["qfl"])
    else:
        assert got.qfl is None


def test_torch_comparator_does_not_depend_on_its_chunks():
    for name in ("hair-L2-17x33", "stack129"):
        c = ss.light_map(name)
        pts = torch.from_numpy(c["points"].copy())
        for chunk in (7, 1000, 1 << 16):
            q0, layers = sv._opacity_torch(pts, c["Ml"], c["Hl"], c["Wl"], c["rl"], c["layer"], sc.NEAR, chunk_elems=chunk)
            assert _same_bits(q0.numpy(), c["q0"]) and _same_bits(layers.numpy().view(np.uint32), c["layers"]), (name, chunk)


@pytest.mark.parametrize("name", FRAMES)
def test_render_strands_composed_equals_the_model_on_cpu_tensors(name):
    c = ss.frame(name)
    pic = sv.render_strands(c["points"], (c["M"], c["H"], c["W"]), fused=False, shadows=_torch_map(c["sm"]), **_frame_kwargs(c))
    assert pic.dtype == torch.uint8 and _same_bits(pic.numpy(), c["picture"])


def test_torch_lookup_equals_the_model_on_the_ladder():
    sm = _ladder_map((4, 2, 0, 0, 0))
    P = np.stack([ss.ladder_point(z) for z in (1.5, 1.0, 2.0, 16.0, 32.0, 0.75, 0.0005)] + [ss.ladder_point(1.5, sx=1.0),
                                                                                           np.full(3, np.nan, np.float32)])
    Pt = torch.from_numpy(P)
    n = sv._occluders_torch([Pt[:, k] for k in range(3)], _torch_map(sm))[0]
    Tr = sv._transmittance_torch([Pt[:, k] for k in range(3)], _torch_map(sm), 0.5, 0.02)
    want = ss.model_lookup(P, sm, 0.5)
    assert _same_bits(n.numpy(), want[0]) and _same_bits(Tr.numpy(), want[1])
    assert n.tolist() == [2.0, 0.0, 4.0, 6.0, 6.0, 0.0, 0.0, 0.0, 0.0] and Tr[0] == 0.5


def test_a_map_that_sees_nothing_returns_the_unshadowed_bytes():
    """render_strands(shadows=True, fused=False) with a light that looks away from the strands and the mesh: Tr == 1 everywhere,
    and 1.f x == x -- the bytes of shadows=False"""
    c = sc.case("hair-front-48x64")
    view = (c["M"], 48, 64)
    kw = dict(mesh=(c["v"], c["f"]), supersample=2, fused=False)
    plain = sv.render_strands(c["points"], view, **kw)
    # a light map (a view of its own) far to the side, looking away: no point and no vertex is valid in it
    from tests.visibility_cases import _M, _look_at, _pinhole
    Ml = _M(_pinhole(24, 24), *_look_at((50.0, 0.0, 0.0), (100.0, 0.0, 0.0)))
    sm = sv.strand_shadow_map(c["points"], Ml, 24, 24, mesh=(c["v"], c["f"]), layer=0.05, fused=False)
    assert not sm.q0.any() and not sm.layers.any() and not sm.qfl.any()
    assert torch.equal(sv.render_strands(c["points"], view, shadows=sm, **kw), plain)
    # shadows=True builds its own map, which does see the hair: the picture changes, and only gets darker
    dark = sv.render_strands(c["points"], view, shadows=True, shadow_size=64, **kw)
    assert (dark <= plain).all() and (dark < plain).any(dim=2).float().mean() > 0.05
    assert torch.equal(sv.render_strands(c["points"], view, shadows=False, **kw), plain)
    # tangent mode has no shadows
    assert torch.equal(sv.render_strands(c["points"], view, mode="tangent", shadows=True, shadow_size=64, **kw),
                       sv.render_strands(c["points"], view, mode="tangent", **kw))
    with pytest.raises(ValueError, match="shadow_kappa"):
        sv.render_strands(c["points"], view, shadows=True, shadow_kappa=-1.0, **kw)
    with pytest.raises(ValueError, match="layer"):
        sv.strand_shadow_map(c["points"], Ml, 24, 24, layer=0.0, fused=False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sv.strand_shadow_map(c["points"], Ml, 24, 24, device="cpu")


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,light", [(1024, None), (64, (0.0, 1.0, 0.0)), ((17, 33), (0.3, -0.2, 0.9)), (6, (1.0, 0.0, 0.0))])
def test_light_view_holds_every_point_and_vertex(size, light):
    """against a float64 restatement: the camera sits distance * rho from the centre of the bounds along the light, looks at it,
    and every finite point and vertex projects valid and at least a texel inside the map -- in float32 too"""
    pts = sc.hair(200, 20, 11).copy()
    pts[3, 4] = np.nan
    pts[7, 0, 2] = np.inf
    v, f = sc.meshes()["small_sphere"]
    view = sc.view_front(48, 64)
    Ml, Hl, Wl, rho = sv.light_view(pts, (v * 1.7, f), light=light, view=view, size=size)
    assert Ml.dtype == np.float32 and Ml.shape == (3, 4) and (Hl, Wl) == ((size, size) if np.ndim(size) == 0 else size)
    allp = np.concatenate([pts.reshape(-1, 3), v * 1.7]).astype(np.float64)
    allp = allp[np.isfinite(allp).all(1)]
    centre = (allp.min(0) + allp.max(0)) / 2
    assert np.isclose(rho, np.linalg.norm(allp - centre, axis=1).max(), rtol=1e-12)
    lw = np.asarray(sv.shading_for_view(view)["light"] if light is None else light, np.float64)
    lw /= np.linalg.norm(lw)
    _, R, t = sv.vis.decompose_projection(Ml.astype(np.float64))
    eye = -R.T @ t
    assert np.allclose(eye, centre + 8.0 * rho * lw, atol=1e-4 * rho) and np.allclose(R[2], -lw, atol=1e-6)
    h = Ml.astype(np.float64) @ np.concatenate([allp, np.ones((len(allp), 1))], 1).T
    assert (h[2] > 6.9 * rho).all()
    x, y = h[0] / h[2], h[1] / h[2]
    assert x.min() >= 1 and x.max() <= Wl - 1 and y.min() >= 1 and y.max() <= Hl - 1
    assert 2 <= min(x.min(), y.min(), Wl - x.max(), Hl - y.max()) < 2 + 0.2 * min(Hl, Wl)   # two texels of margin; the sphere fills the map
    sx, sy, _, valid = ss.vc.model_project(allp.astype(np.float32), Ml.reshape(12))
    assert valid.all() and sx.min() >= 0 and sx.max() < Wl and sy.min() >= 0 and sy.max() < Hl
    with pytest.raises(ValueError, match="6 texels"):
        sv.light_view(pts, light=(0, 0, 1), size=4)
    with pytest.raises(ValueError, match="light"):
        sv.light_view(pts)
    assert sv.light_view(np.zeros((0, 2, 3), np.float32), light=(0, 0, 1), size=8)[3] == 1.0


def test_defaults_are_the_headers():
    hdr = open(sc.HEADER).read()
    for text in ("light map 1024 x 1024", "rl 1.0 texel", "kappa 0.2", "shadow_bias 0.02", "d = rho / 32", "CHOSEN"):
        assert text in hdr, text
    assert (sv.SHADOW_SIZE, sv.SHADOW_HALF_WIDTH, sv.SHADOW_KAPPA, sv.SHADOW_BIAS, sv.SHADOW_LAYERS_PER_RADIUS) == (1024, 1.0, 0.2, 0.02, 32)
    assert (ss.KAPPA, ss.BIAS) == (sv.SHADOW_KAPPA, sv.SHADOW_BIAS)


def test_c_abi_refusals_launch_nothing():
    L = _lib.lib()
    fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)  # never dereferenced: every call below is refused before a launch
    M = (ctypes.c_float * 12)(*([1.0] * 12))
    need = sv.strandview_workspace_bytes(8, 12, 48, 64)
    ok = dict(S=8, L=12, points=fake, M=ctypes.byref(M), near=1e-3, H=48, W=64, r=1.0, layer=0.1, ws=fake, bytes=need, q0=fake, layers=fake)

    def opacity(**kw):
        a = dict(ok, **kw)
        return L.ghr_strandview_opacity(None, a["S"], a["L"], a["points"], a["M"], a["near"], a["H"], a["W"], a["r"], a["layer"], a["ws"],
                                        a["bytes"], a["q0"], a["layers"])
    nan, inf = float("nan"), float("inf")
    for kw, why in ((dict(S=-1), b"negative"), (dict(L=1), b"L < 2"), (dict(H=-1), b"negative"), (dict(points=None), b"points"),
                    (dict(M=None), b"Ml is NULL"), (dict(near=nan), b"near"), (dict(r=0.0), b"half_width"), (dict(r=-1.0), b"half_width"),
                    (dict(r=inf), b"half_width"), (dict(r=nan), b"half_width"), (dict(layer=0.0), b"layer"), (dict(layer=-0.1), b"layer"),
                    (dict(layer=inf), b"layer"), (dict(layer=nan), b"layer"), (dict(ws=None), b"workspace is NULL"),
                    (dict(ws=ctypes.c_void_p(4104)), b"16-B aligned"), (dict(bytes=need - 1), b"too small"), (dict(bytes=0), b"too small"),
                    (dict(q0=None), b"output plane"), (dict(layers=None), b"output plane"), (dict(q0=ctypes.c_void_p(4098)), b"4-B aligned"),
                    (dict(layers=odd), b"layers is not 16-B aligned"), (dict(points=ctypes.c_void_p(4098)), b"4-B aligned"),
                    (dict(H=65536, W=65536), b"H * W")):
        assert opacity(**kw) == _lib.GHR_E_INVALID, kw
        assert why in L.ghr_last_error(), (kw, L.ghr_last_error())
    assert opacity(H=0, q0=None, layers=None, bytes=sv.strandview_workspace_bytes(8, 12, 0, 64)) == _lib.GHR_OK      # Hl Wl == 0
    assert opacity(H=0, S=0, points=None, q0=None, layers=None) == _lib.GHR_OK

    sh = sv._shading_struct(sc.shading(sc.view_front(48, 64)))

    def shadow(**kw):
        a = dict(dict(near=1e-3, Hl=17, Wl=33, layer=0.1, kappa=0.2, bias=0.02, q0=4096, layers=4096, qfl=4096), **kw)
        s = _lib.StrandViewShadow()
        s.Ml = (ctypes.c_float * 12)(*([1.0] * 12))
        s.near_w, s.Hl, s.Wl, s.layer, s.kappa, s.bias = a["near"], a["Hl"], a["Wl"], a["layer"], a["kappa"], a["bias"]
        s.q0, s.layers, s.qfl = a["q0"], a["layers"], a["qfl"]
        return s

    def shade(fields=None, **kw):
        a = dict(dict(S=8, L=12, points=fake, V=8, v=fake, F=12, f=fake, H=48, W=64, seg=fake, face=fake, t=fake, mode=0,
                      sh=ctypes.byref(sh), base=fake, sd=ctypes.byref(shadow(**(fields or {}))), rgb=fake), **kw)
        return L.ghr_strandview_shade_shadowed(None, a["S"], a["L"], a["points"], a["V"], a["v"], a["F"], a["f"], a["H"], a["W"], a["seg"],
                                               a["face"], a["t"], a["mode"], a["sh"], a["base"], a["sd"], a["rgb"])
    for kw, why in ((dict(mode=2), b"mode"), (dict(L=1), b"L < 2"), (dict(sh=None), b"shading is NULL"), (dict(sd=None), b"shadow is NULL"),
                    (dict(points=None), b"points"), (dict(v=None), b"vertices"), (dict(f=None), b"faces"), (dict(seg=None), b"pix_to_segment"),
                    (dict(face=None), b"pix_to_segment"), (dict(t=None), b"t is NULL"), (dict(rgb=None), b"rgb is NULL"),
                    (dict(t=ctypes.c_void_p(4098)), b"4-B aligned"), (dict(F=-1), b"negative")):
        assert shade(**kw) == _lib.GHR_E_INVALID, kw
        assert why in L.ghr_last_error(), (kw, L.ghr_last_error())
    for sd, why in ((dict(layer=0.0), b"layer"), (dict(layer=nan), b"layer"), (dict(layer=inf), b"layer"), (dict(kappa=-0.1), b"kappa"),
                    (dict(kappa=nan), b"kappa"), (dict(kappa=inf), b"kappa"), (dict(bias=-0.01), b"bias"), (dict(bias=nan), b"bias"),
                    (dict(near=nan), b"near"), (dict(Hl=-1), b"negative"), (dict(Hl=65536, Wl=65536), b"Hl * Wl"), (dict(q0=None), b"q0 or layers"),
                    (dict(layers=None), b"q0 or layers"), (dict(layers=4100), b"16-B aligned"), (dict(qfl=4098), b"4-B aligned")):
        assert shade(fields=sd) == _lib.GHR_E_INVALID, sd
        assert why in L.ghr_last_error(), (sd, L.ghr_last_error())
    assert shade(H=0, seg=None, face=None, t=None, rgb=None) == _lib.GHR_OK
    for n in ("ghr_strandview_opacity", "ghr_strandview_shade_shadowed"):
        assert n in _lib.EXPORTS and hasattr(L, n) and getattr(L, n).argtypes, n
    assert L.ghr_abi_version() == 20   # added without a bump, as the preview itself was


def test_video_tool_writes_shadowed_frames_in_composed_mode(tmp_path):
    """tools/render_strand_video.py --shadows --composed on a small scene: its frames against the library calls, with the light
    following the camera and with --world-light (one map for the path)"""
    import importlib.util
    import pickle
    from PIL import Image
    from gaussianhaircut_amd import between_stages as bs
    from gaussianhaircut_amd import visibility as vis
    from tests.visibility_cases import _look_at
    spec = importlib.util.spec_from_file_location("render_strand_video_tool", os.path.join(hp.ROOT, "tools", "render_strand_video.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    pts = sc.hair(20, 10, 1, through=False)
    pkl, _ = bs.export_strands(pts, str(tmp_path), 10)
    v, f = sc.meshes()["small_sphere"]
    with open(tmp_path / "head.obj", "w") as fh:
        fh.write("".join("v %.9g %.9g %.9g\n" % tuple(p) for p in v) + "".join("f %d %d %d\n" % tuple(t + 1) for t in f))
    H, W, cams, keys = 24, 32, {}, {}
    for k, fr in enumerate((0, 4, 9)):
        R, t = _look_at((3 * np.sin(0.6 * k), 0.4, 3 * np.cos(0.6 * k)), (0.0, 0.0, 0.0))
        Kh = np.array([[2.4 * H / W, 0, 0.02], [0, 2.4, -0.01], [0, 0, 1.0]])
        P = np.eye(4)
        P[:3] = Kh @ np.concatenate([R, t[:, None]], 1)
        cams["%06d" % fr] = torch.from_numpy(P.T.copy())
        keys[fr] = vis.views_from_projections({"k": P[:3]}, {"k": (H, W)})["k"][0].astype(np.float64).reshape(3, 4)
    with open(tmp_path / "cams.pkl", "wb") as fh:
        pickle.dump(cams, fh)
    common = ["--strands", pkl, "--mesh", str(tmp_path / "head.obj"), "--cameras", str(tmp_path / "cams.pkl"), "--size", "24x32",
              "--composed", "--speed_up", "4", "--max_frames", "2", "--shadow_size", "48"]
    path = sv.camera_path(keys, speed_up=4)[:2]
    mesh = tool.read_obj(str(tmp_path / "head.obj"))
    assert tool.main(common + ["--out", str(tmp_path / "a"), "--shadows"]) == 2
    assert tool.main(common + ["--out", str(tmp_path / "b"), "--shadows", "--world-light", "0", "2", "0"]) == 2
    assert tool.main(common + ["--out", str(tmp_path / "c")]) == 2
    Ml, Hl, Wl, _ = sv.light_view(pts, mesh, light=(0.0, 1.0, 0.0), size=48)
    fixed = sv.strand_shadow_map(pts, Ml, Hl, Wl, mesh=mesh, fused=False)
    for k, P in enumerate(path):
        view = (P.astype(np.float32).reshape(12), H, W)
        read = lambda d: np.asarray(Image.open(tmp_path / d / "results" / ("%06d.png" % k)))  # noqa: E731
        assert np.array_equal(read("a"), sv.render_strands(pts, view, mesh=mesh, fused=False, shadows=True, shadow_size=48).numpy())
        assert np.array_equal(read("b"), sv.render_strands(pts, view, mesh=mesh, fused=False, shadows=fixed, light=(0.0, 1.0, 0.0)).numpy())
        assert np.array_equal(read("c"), sv.render_strands(pts, view, mesh=mesh, fused=False).numpy())
        assert (read("a") <= read("c")).all() and not np.array_equal(read("a"), read("c")) and not np.array_equal(read("a"), read("b"))
    with pytest.raises(SystemExit):
        tool.main(common + ["--out", str(tmp_path / "d"), "--world-light", "0", "1", "0"])
