"""The strand preview (csrc/ghr_strandview.h, gaussianhaircut_amd/strand_view.py) without a GPU.

Every result is an integer, a byte or a float32 compared by its bits: every comparison is exact.
 1. the numpy float32 MODEL of the definition (tests/strand_view_cases.py) against a float64 truth on the same screen points:
    the index planes are equal wherever the pixel is not FRAGILE, and fragile pixels are at most 2 % of the covered ones (asserted
    on the model alone before the mask is used); closed coverage and ties on the lattice cases;
 2. the product's own per-element functions and a host walk of the tile lists (tests/hostsim/ghr_hostsim_strandview.cpp, every
    index checked, no segment twice in a tile) against the model, bit for bit, on every case; the same cases through a stand-alone
    program built with -fsanitize=address,undefined (nothing sanitized is loaded here);
 3. the PyTorch comparator (fused=False) on CPU tensors against the model: all planes and the bytes;
 4. camera_path against a restatement with scipy; the refusals of the C ABI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd import strand_view as sv
from tests import helpers as hp
from tests import strand_view_cases as sc

CASES = sc.CASES
SV_HEADERS = ["ghr_hostsim_tilelists.h", "ghr_strandview.h", "ghr_visibility.h", "ghr_tilelists.h", "ghr_mesh.h"]
DEPS = ["ghr_hostsim_strandview.cpp"] + SV_HEADERS


@pytest.fixture(scope="module")
def sim():
    L = ctypes.CDLL(hp.compile_hostsim("libghr_hostsim_strandview.so", "ghr_hostsim_strandview.cpp", ["-O2", "-fPIC", "-shared"], DEPS))
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.ghrsim_sv_face_depth.argtypes = [i32, vp, i32, vp, vp, f32, i32, i32, vp, vp]
    L.ghrsim_sv_raster.argtypes = [i32, i32, vp, vp, f32, i32, i32, f32, f32] + [vp] * 8
    L.ghrsim_sv_shade.argtypes = [i32, i32, vp, i32, vp, i32, vp, i32, i32, vp, vp, i32, vp, vp, vp]
    L.ghrsim_sv_resolve.argtypes = [i32, i32, i32, vp, vp]
    assert L.ghrsim_sv_chunk() == sc.CHUNK and L.ghrsim_sv_big_rect() == sc.BIG_RECT
    assert L.ghrsim_sv_shading_bytes() == ctypes.sizeof(_lib.StrandViewShading) == 76
    return L


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _shading_bytes(sh):
    return bytes(sv._shading_struct(sh))


def _sim_frame(sim, c, m):
    """the host simulator on the grid of model frame m: (four planes, rgb, tile lengths, length of the big list)"""
    H, W = m["H"], m["W"]
    pts = c["points"]
    S, L = pts.shape[:2]
    has_mesh = c["v"] is not None
    V, F = (len(c["v"]), len(c["f"])) if has_mesh else (0, 0)
    qf = None
    if has_mesh:
        qf = np.full((H, W), 7, np.float32)
        sim.ghrsim_sv_face_depth(V, _p(c["v"]), F, _p(c["f"]), _p(m["M"]), float(sc.NEAR), H, W, _p(m["pix"]), _p(qf))
    seg, face = np.full((H, W), 7, np.int32), np.full((H, W), 7, np.int32)
    t, inv = np.full((H, W), 7, np.float32), np.full((H, W), 7, np.float32)
    tiles = np.zeros(((H + 15) // 16) * ((W + 15) // 16), np.uint32)
    n_big = np.zeros(1, np.uint32)
    assert sim.ghrsim_sv_raster(S, L, _p(pts), _p(m["M"]), float(sc.NEAR), H, W, m["r"], float(np.float32(c["bias"])),
                                _p(m["pix"]) if has_mesh else None, _p(qf), _p(seg), _p(t), _p(face), _p(inv), _p(tiles), _p(n_big)) == 0
    rgb = np.full((H, W, 3), 7, np.uint8)
    shb = np.frombuffer(_shading_bytes(c["sh"]), np.uint8).copy()
    sim.ghrsim_sv_shade(S, L, _p(pts), V, _p(c["v"]), F, _p(c["f"]), H, W, _p(seg), _p(face), c["mode"], _p(shb), _p(c["base"]), _p(rgb))
    return (seg, t, face, inv), qf, rgb, tiles, int(n_big[0])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == np.ascontiguousarray(b).tobytes()


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
def test_model_agrees_with_the_float64_truth_away_from_fragile_pixels():
    worst = (0.0, "")
    for name in CASES:
        if name.startswith(sc.EXACT_ONLY) or sc.case(name)["s"] != 1:
            continue
        seg, _, face, _ = sc.model_frame(name)["planes"]
        t_seg, t_face, fragile = sc.truth_frame(name)
        covered = int(((seg >= 0) | (sc.model_frame(name)["winner"][0] >= 0)).sum())
        assert covered > 0, name
        share = float(fragile.sum()) / covered
        worst = max(worst, (share, name))
        assert share <= 0.02, (name, share)                      # the cap, on the model alone, before the mask is used
        assert np.array_equal(seg[~fragile], t_seg[~fragile]), name
        assert np.array_equal(face[~fragile], t_face[~fragile]), name
    print("largest share of fragile pixels among the covered: %.4f (%s)" % worst)


@pytest.mark.parametrize("r", sc.RADII)
def test_coverage_is_closed_on_the_lattice(r):
    """the horizontal segment y = 3 from x = 2 to 63: centres at distance exactly r are covered (r = 0.5: rows 2 and 3; r = 2.5:
    rows 0 .. 5), nothing beyond; the round cap at x = 2 reaches the centre (1.5, 2.5) only from r = 0.75 on"""
    name = "singles-48x64-r%g" % r
    c = sc.case(name)
    k, t, qs, count = sc.model_strand_winner(c["points"][:1], c["M"], 48, 64, r, return_cover_count=True)
    rows = {0.5: (2, 3), 0.75: (2, 3), 2.5: (0, 5)}[r]
    assert (count[rows[0]:rows[1] + 1, 2:63] == 1).all() and not count[rows[1] + 1:, :].any()
    assert not count[:rows[0], :].any()
    assert count[2, 1] == (0 if r == 0.5 else 1)            # (1.5, 2.5): 0.5^2 + 0.5^2 = 0.5 against r^2
    assert count[2, 63] == (0 if r == 0.5 else 1)           # past the end at x = 63, as at the start
    assert t[2, 2] == np.float32(0.5 / 61) and t[3, 40] == np.float32(38.5 / 61)
    # the zero-length segment is a closed disc about (32.5, 24.5): the centre itself for every r, the four neighbours from 1 on
    k, _, _, count = sc.model_strand_winner(c["points"][3:], c["M"], 48, 64, r, return_cover_count=True)
    assert count[24, 32] == 1 and count.sum() == {0.5: 1, 0.75: 1, 2.5: 21}[r]
    # all four at w = 1: where several cover, the lowest k wins
    k = sc.model_frame(name)["planes"][0]
    assert k[3, 5] == 0 and set(np.unique(k).tolist()) == {-1, 0, 1, 2, 3}


@pytest.mark.parametrize("K", sc.STACK_K)
def test_stacks_give_the_nearest_and_duplicates_the_lowest_index(K):
    seg = sc.model_frame("dups%d" % K)["planes"][0]
    assert set(np.unique(seg).tolist()) == {-1, 1}            # strand 0 is farther; 1 .. K are the same segment
    m = sc.model_frame("stack%d" % K)
    order = np.random.default_rng(K).permutation(K)
    seg = m["planes"][0]
    assert (seg >= 0).sum() > 15 and seg[24, 24] == int(np.argmin(order))


def test_dropped_segments_leave_no_pixel():
    c = sc.case("dropped-48x64")
    seg = sc.model_frame("dropped-48x64")["planes"][0]
    # strand 0 keeps only its last segment (2), strand 1 only its first (3), strand 2 only its last (8), strand 3 all of (9 .. 11)
    assert set(np.unique(seg).tolist()) == {-1, 2, 3, 8, 9, 10, 11}, np.unique(seg)
    assert np.isnan(c["points"][2, 1, 1])


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_host_sim_equals_the_model_bit_for_bit(sim, name):
    c = sc.case(name)
    m = sc.model_frame(name, c["s"])
    planes, qf, rgb, tiles, n_big = _sim_frame(sim, c, m)
    for got, want in zip(planes, m["planes"]):
        assert _same_bits(got, want)
    if qf is not None:
        assert _same_bits(qf, m["qf"])
    assert _same_bits(rgb, m["rgb"])
    small = np.full((c["H"], c["W"], 3), 7, np.uint8)
    sim.ghrsim_sv_resolve(c["H"], c["W"], c["s"], _p(rgb), _p(small))
    assert _same_bits(small, sc.model_picture(name))
    if name.startswith(("stack", "dups")):
        K = int(name.lstrip("stackdup"))
        assert tiles[1 * 4 + 1] == K + (1 if name.startswith("dups") else 0) and tiles.sum() == tiles[5] and n_big == 0
    if name == "long-130x250":
        assert n_big == 2 and tiles.min() >= 2                 # the two long segments: every tile walks them, once (checked there)
        assert {12, 25} <= set(np.unique(planes[0]).tolist())
    if name == "long-48x64":
        assert n_big == 0                                      # 3 x 4 tiles: within the limit, listed tile by tile
    if name.startswith("empty"):
        assert (planes[0] == -1).all() and not tiles.any()


def test_sanitized_stand_alone_program_runs_the_cases_clean(tmp_path):
    """ghr_strandview_selfcheck: the per-element functions and the table walk under AddressSanitizer and
    UndefinedBehaviorSanitizer, as a program of its own (exact-size buffers)."""
    san = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    if os.path.basename(hp.host_cxx()) == "g++":
        san += ["-static-libasan", "-static-libubsan"]
    exe = hp.compile_hostsim("ghr_strandview_selfcheck_san", "ghr_strandview_selfcheck.cpp", san, DEPS)
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as fh:
        for name in CASES:
            c = sc.case(name)
            m = sc.model_frame(name, c["s"])
            has_mesh = c["v"] is not None
            S, L = c["points"].shape[:2]
            fh.write(np.array([S, L, m["H"], m["W"], len(c["v"]) if has_mesh else 0, len(c["f"]) if has_mesh else 0, int(has_mesh),
                               c["mode"], int(c["base"] is not None), c["s"]], np.int32).tobytes())
            fh.write(np.concatenate([m["M"], [sc.NEAR, m["r"], c["bias"]]]).astype(np.float32).tobytes())
            fh.write(_shading_bytes(c["sh"]))
            arrs = [c["points"]] + ([c["v"], c["f"], m["pix"]] if has_mesh else []) + ([c["base"]] if c["base"] is not None else [])
            for arr in arrs + list(m["planes"]) + [m["rgb"], sc.model_picture(name)]:
                fh.write(np.ascontiguousarray(arr).tobytes())
    res = subprocess.run([exe, path], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "%d cases ok" % len(CASES) in res.stdout and "runtime error" not in res.stderr, res.stdout + res.stderr


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def _api_kwargs(c):
    sh = c["sh"]
    colors = c["base"] if c["base"] is not None else (tuple(float(x) for x in sh["base_rgb"]) if c["colors"] == "one" else None)
    return dict(mesh=None if c["v"] is None else (c["v"], c["f"]), colors=colors, mode=("kajiya", "tangent")[c["mode"]],
                supersample=c["s"], half_width=c["r"], head_bias=c["bias"], near=float(sc.NEAR), eye=sh["eye"], light=sh["light"])


@pytest.mark.parametrize("name", CASES)
def test_torch_comparator_equals_the_model_on_cpu_tensors(name):
    c = sc.case(name)
    m = sc.model_frame(name)
    got = sv.rasterize_strands(c["points"], c["M"], c["H"], c["W"], mesh=None if c["v"] is None else (c["v"], c["f"]),
                               half_width=c["r"], head_bias=c["bias"], near=float(sc.NEAR), fused=False)
    assert [g.dtype for g in got] == [torch.int32, torch.float32, torch.int32, torch.float32]
    for g, want in zip(got, m["planes"]):
        assert _same_bits(g.numpy(), want)
    if c["v"] is not None:
        v, f = torch.from_numpy(c["v"].copy()), torch.from_numpy(c["f"].copy()).long()
        qf = sv._face_depth_torch(v, f, c["M"], c["H"], c["W"], sc.NEAR, torch.from_numpy(m["pix"].copy()))
        assert _same_bits(qf.numpy(), m["qf"])
    pic = sv.render_strands(c["points"], (c["M"], c["H"], c["W"]), fused=False, **_api_kwargs(c))
    assert pic.dtype == torch.uint8 and _same_bits(pic.numpy(), sc.model_picture(name))


def test_torch_comparator_does_not_depend_on_its_chunks():
    c = sc.case("hair-front-15x17")
    m = sc.model_frame("hair-front-15x17")
    pts = torch.from_numpy(c["points"].copy())
    got = sv._rasterize_torch(pts, c["M"], 15, 17, c["r"], c["bias"], sc.NEAR, torch.from_numpy(m["pix"].copy()),
                              torch.from_numpy(m["qf"].copy()), chunk_elems=7)
    for g, want in zip(got, m["planes"]):
        assert _same_bits(g.numpy(), want)


def test_default_shading_is_the_headers_and_the_eye_is_the_camera_centre():
    M = sc.view_front(48, 64)
    sh = sv.shading_for_view(M)
    want = sc.shading(M)
    for k in want:
        assert np.array_equal(np.asarray(sh[k]), np.asarray(want[k])), k
    assert np.allclose(sh["eye"], (0.3, 0.2, 3.1), atol=1e-5) and np.isclose(np.linalg.norm(sh["light"]), 1.0, atol=1e-6)
    hdr = open(sc.HEADER).read()
    for text in ("ambient 0.25, kd 0.65, ks 0.35, shininess_log2 5", "(0.45, 0.30, 0.18)", "(0.62, 0.62, 0.62)", "(0.45, -0.60, -0.66)"):
        assert text in hdr, text
    # above and to the right of the camera, on the camera's side: camera x right, y down, z forward
    _, R, _ = sv.vis.decompose_projection(np.asarray(M, np.float64).reshape(3, 4))
    lc = R @ sh["light"].astype(np.float64)
    assert lc[0] > 0 and lc[1] < 0 and lc[2] < 0


def test_fused_forms_refuse_cpu_and_bad_arguments():
    c = sc.case("hair-front-15x17")
    with pytest.raises(RuntimeError, match="no CPU path"):
        sv.rasterize_strands(c["points"], c["M"], 15, 17, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        sv.render_strands(c["points"], (c["M"], 15, 17), device="cpu")
    with pytest.raises(ValueError, match="supersample"):
        sv.render_strands(c["points"], (c["M"], 15, 17), supersample=3, fused=False)
    with pytest.raises(ValueError, match="mode"):
        sv.render_strands(c["points"], (c["M"], 15, 17), mode="marschner", fused=False)
    with pytest.raises(ValueError, match="half_width"):
        sv.rasterize_strands(c["points"], c["M"], 15, 17, half_width=0.0, fused=False)
    with pytest.raises(ValueError, match="head_bias"):
        sv.rasterize_strands(c["points"], c["M"], 15, 17, head_bias=-0.1, fused=False)
    with pytest.raises(ValueError, match="two points"):
        sv.rasterize_strands(c["points"][:, :1], c["M"], 15, 17, fused=False)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def _key_cameras():
    from tests.visibility_cases import _look_at
    keys = {}
    for n, fr in enumerate((3, 10, 14, 25, 31)):
        a = 0.5 * n
        K = np.array([[900.0 + 20 * n, 0.3, 540.0 + n], [0.0, 905.0 + 10 * n, 960.0 - 2 * n], [0.0, 0.0, 1.0]])
        R, t = _look_at((3 * np.sin(a), 0.3 * n, 3 * np.cos(a)), (0.0, 0.1, 0.0))
        keys[fr] = (K, R, t)
    return keys


def test_camera_path_equals_a_restatement_with_scipy():
    from scipy.spatial.transform import Rotation, RotationSpline
    keys = _key_cameras()
    P = {fr: (-2.5 if fr == 10 else 1.0) * K @ np.concatenate([R, t[:, None]], 1) for fr, (K, R, t) in keys.items()}
    frames = sorted(keys)
    full = sv.camera_path(P, speed_up=1, max_frames=10 ** 6)
    assert full.shape == (frames[-1] - frames[0], 3, 4) and full.dtype == np.float64
    # the restatement: the script's loop over range(frames[-1]) with its prev_j / next_j, then its slice
    spline = RotationSpline(frames, Rotation.from_matrix(np.stack([keys[fr][1] for fr in frames])))
    R_interp = spline(list(range(frames[-1]))).as_matrix()
    Ks, Ts = [keys[fr][0] for fr in frames], [keys[fr][2] for fr in frames]
    cams, prev_j, next_j = [], -1, 0
    for i in range(frames[-1]):
        if i in frames:
            prev_j += 1
            next_j += 1
        alpha = 1 - (i - frames[prev_j]) / (frames[next_j] - frames[prev_j])
        cams.append((Ks[prev_j] * alpha + Ks[next_j] * (1 - alpha)) @ np.concatenate(
            [R_interp[i], (Ts[prev_j] * alpha + Ts[next_j] * (1 - alpha))[:, None]], 1))
    cams = np.stack(cams)
    assert np.allclose(full, cams[frames[0]:frames[-1]], rtol=1e-9, atol=1e-9)
    # the key cameras at the key frames (but the last, which the script's range never reaches)
    for fr in frames[:-1]:
        K, R, t = keys[fr]
        assert np.allclose(full[fr - frames[0]], K @ np.concatenate([R, t[:, None]], 1), rtol=1e-9, atol=1e-8), fr
    # speed_up and max_frames: the script's slice
    for speed_up, max_frames in ((4, 200), (3, 5), (1, 7), (50, 2)):
        got = sv.camera_path(P, speed_up=speed_up, max_frames=max_frames)
        assert np.array_equal(got, full[::speed_up][:max_frames]) and len(got) == min(max_frames, -(-len(full) // speed_up))
    with pytest.raises(ValueError, match="two key frames"):
        sv.camera_path({3: P[3]})


def test_c_abi_refusals_launch_nothing():
    L = _lib.lib()
    b = ctypes.c_size_t(0)
    assert L.ghr_strandview_sizes(10, 20, 48, 64, ctypes.byref(b)) == _lib.GHR_OK and b.value > 0 and b.value % 16 == 0
    small = b.value
    assert L.ghr_strandview_sizes(0, 2, 0, 0, ctypes.byref(b)) == _lib.GHR_OK and 0 < b.value < small
    # sized from S, L, H, W alone: at most BIG_RECT list entries per segment, whatever the image
    assert L.ghr_strandview_sizes(10, 20, 4800, 6400, ctypes.byref(b)) == _lib.GHR_OK
    assert b.value <= 10 * 20 * 16 + 10 * 19 * (32 + 4 + 4 * sc.BIG_RECT) + 4 * (300 * 400 + 1) * 2 + 256
    assert L.ghr_strandview_sizes(10, 20, 48, 64, None) == _lib.GHR_E_INVALID
    for bad, why in (((-1, 2, 1, 1), b"negative"), ((1, 2, -1, 1), b"negative"), ((1, 1, 1, 1), b"L < 2"), ((1, 0, 1, 1), b"L < 2"),
                     ((1, 2, 65536, 65536), b"H * W"), ((2 ** 22, 100, 1024, 1024), b"tile lists")):
        assert L.ghr_strandview_sizes(*bad, ctypes.byref(b)) == _lib.GHR_E_INVALID, bad
        assert why in L.ghr_last_error(), (bad, L.ghr_last_error())
    fake = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before anything is enqueued
    M = (ctypes.c_float * 12)(*([1.0] * 12))
    sh = sv._shading_struct(sc.shading(sc.view_front(48, 64)))
    ok = dict(S=8, L=12, points=fake, M=ctypes.byref(M), near=1e-3, H=48, W=64, r=0.75, bias=0.0, pix=fake, qf=fake, ws=fake,
              seg=fake, t=fake, face=fake, inv=fake)

    def raster(**kw):
        a = dict(ok, **kw)
        return L.ghr_strandview_raster(None, a["S"], a["L"], a["points"], a["M"], a["near"], a["H"], a["W"], a["r"], a["bias"],
                                       a["pix"], a["qf"], a["ws"], a["seg"], a["t"], a["face"], a["inv"])
    odd = ctypes.c_void_p(4098)
    for kw, why in ((dict(S=-1), b"negative"), (dict(L=1), b"L < 2"), (dict(H=-1), b"negative"), (dict(points=None), b"points"),
                    (dict(M=None), b"M is NULL"), (dict(near=float("nan")), b"near"), (dict(r=0.0), b"half_width"),
                    (dict(r=-1.0), b"half_width"), (dict(r=float("inf")), b"half_width"), (dict(r=float("nan")), b"half_width"),
                    (dict(bias=-0.01), b"head_bias"), (dict(bias=float("nan")), b"head_bias"), (dict(pix=None), b"together"),
                    (dict(qf=None), b"together"), (dict(ws=None), b"workspace is NULL"), (dict(ws=ctypes.c_void_p(4104)), b"16-B aligned"),
                    (dict(seg=None), b"output plane"), (dict(t=None), b"output plane"), (dict(face=None), b"output plane"),
                    (dict(inv=None), b"output plane"), (dict(points=odd), b"4-B aligned"), (dict(inv=odd), b"4-B aligned"),
                    (dict(H=65536, W=65536), b"H * W")):
        assert raster(**kw) == _lib.GHR_E_INVALID, kw
        assert why in L.ghr_last_error(), (kw, L.ghr_last_error())
    assert raster(H=0, points=None, pix=None, qf=None, seg=None, t=None, face=None, inv=None, S=0) == _lib.GHR_OK   # H W == 0

    def depth(**kw):
        a = dict(dict(V=8, v=fake, F=12, f=fake, M=ctypes.byref(M), near=1e-3, H=48, W=64, pix=fake, qf=fake), **kw)
        return L.ghr_strandview_face_depth(None, a["V"], a["v"], a["F"], a["f"], a["M"], a["near"], a["H"], a["W"], a["pix"], a["qf"])
    for kw, why in ((dict(V=-1), b"negative"), (dict(v=None), b"vertices"), (dict(f=None), b"faces"), (dict(M=None), b"M is NULL"),
                    (dict(near=-1.0), b"near"), (dict(pix=None), b"pix_to_face"), (dict(qf=None), b"qf is NULL"), (dict(qf=odd), b"4-B aligned")):
        assert depth(**kw) == _lib.GHR_E_INVALID, kw
        assert why in L.ghr_last_error(), (kw, L.ghr_last_error())
    assert depth(H=0, pix=None, qf=None) == _lib.GHR_OK

    def shade(**kw):
        a = dict(dict(S=8, L=12, points=fake, V=8, v=fake, F=12, f=fake, H=48, W=64, seg=fake, face=fake, mode=0, sh=ctypes.byref(sh),
                      base=fake, rgb=fake), **kw)
        return L.ghr_strandview_shade(None, a["S"], a["L"], a["points"], a["V"], a["v"], a["F"], a["f"], a["H"], a["W"], a["seg"],
                                      a["face"], a["mode"], a["sh"], a["base"], a["rgb"])
    bad_sh = sv._shading_struct(sc.shading(sc.view_front(48, 64), shininess_log2=5))
    bad_sh.shininess_log2 = 17
    for kw, why in ((dict(mode=2), b"mode"), (dict(mode=-1), b"mode"), (dict(L=1), b"L < 2"), (dict(sh=None), b"shading is NULL"),
                    (dict(sh=ctypes.byref(bad_sh)), b"shininess_log2"), (dict(points=None), b"points"), (dict(v=None), b"vertices"),
                    (dict(f=None), b"faces"), (dict(seg=None), b"pix_to_segment"), (dict(face=None), b"pix_to_segment"),
                    (dict(rgb=None), b"rgb is NULL"), (dict(base=odd), b"4-B aligned"), (dict(F=-1), b"negative")):
        assert shade(**kw) == _lib.GHR_E_INVALID, kw
        assert why in L.ghr_last_error(), (kw, L.ghr_last_error())
    assert shade(H=0, seg=None, face=None, rgb=None) == _lib.GHR_OK
    for s in (0, 3, 8, -1):
        assert L.ghr_strandview_resolve(None, 48, 64, s, fake, fake) == _lib.GHR_E_INVALID and b"supersample" in L.ghr_last_error()
    assert L.ghr_strandview_resolve(None, 48, 64, 2, None, fake) == _lib.GHR_E_INVALID and b"src" in L.ghr_last_error()
    assert L.ghr_strandview_resolve(None, 48, 64, 2, fake, None) == _lib.GHR_E_INVALID and b"dst" in L.ghr_last_error()
    assert L.ghr_strandview_resolve(None, -1, 64, 2, fake, fake) == _lib.GHR_E_INVALID
    assert L.ghr_strandview_resolve(None, 0, 64, 4, None, None) == _lib.GHR_OK
    for n in ("ghr_strandview_sizes", "ghr_strandview_face_depth", "ghr_strandview_raster", "ghr_strandview_shade", "ghr_strandview_resolve"):
        assert n in _lib.EXPORTS and hasattr(L, n) and getattr(L, n).argtypes, n
    assert "ghr_strandview.h" in _lib.HEADERS


def test_video_tool_writes_the_frames_of_a_path_from_exported_strands(tmp_path):
    """tools/render_strand_video.py --composed on a small scene in the reference's layout: strands as export_strands writes them
    (pickle and PLY), an OBJ head, three key cameras in the reference's pickle format; its frames against the library calls"""
    import importlib.util
    import pickle
    from PIL import Image
    from gaussianhaircut_amd import between_stages as bs
    from gaussianhaircut_amd import visibility as vis
    from tests.visibility_cases import _look_at
    spec = importlib.util.spec_from_file_location("render_strand_video_tool", os.path.join(hp.ROOT, "tools", "render_strand_video.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    pts = sc.hair(20, 10, 1)
    pkl, ply = bs.export_strands(pts, str(tmp_path), 10)
    v, f = sc.meshes()["small_sphere"]
    with open(tmp_path / "head.obj", "w") as fh:
        fh.write("".join("v %.9g %.9g %.9g\n" % tuple(p) for p in v) + "".join("f %d %d %d\n" % tuple(t + 1) for t in f))
    H, W, cams, keys = 24, 32, {}, {}
    for k, fr in enumerate((0, 4, 9)):
        R, t = _look_at((3 * np.sin(0.6 * k), 0.4, 3 * np.cos(0.6 * k)), (0.0, 0.0, 0.0))
        Kh = np.array([[2.4 * H / W, 0, 0.02], [0, 2.4, -0.01], [0, 0, 1.0]])     # in units of half the image, as the reference's pickle
        P = np.eye(4)
        P[:3] = Kh @ np.concatenate([R, t[:, None]], 1)
        cams["%06d" % fr] = torch.from_numpy(P.T.copy())                          # stored transposed
        keys[fr] = vis.views_from_projections({"k": P[:3]}, {"k": (H, W)})["k"][0].astype(np.float64).reshape(3, 4)
    cams["not_a_frame"] = torch.eye(4)
    with open(tmp_path / "cams.pkl", "wb") as fh:
        pickle.dump(cams, fh)
    n = tool.main(["--strands", pkl, "--mesh", str(tmp_path / "head.obj"), "--cameras", str(tmp_path / "cams.pkl"), "--size", "24x32",
                   "--out", str(tmp_path / "a"), "--composed", "--speed_up", "4"])
    path = sv.camera_path(keys, speed_up=4)
    assert n == len(path) == 3 and sorted(os.listdir(tmp_path / "a" / "results")) == ["%06d.png" % k for k in range(3)]
    for k, P in enumerate(path):
        want = sv.render_strands(pts, (P.astype(np.float32).reshape(12), H, W), mesh=(v, f), fused=False)
        got = np.asarray(Image.open(tmp_path / "a" / "results" / ("%06d.png" % k)))
        assert np.array_equal(got, want.numpy()) and len(np.unique(got.reshape(-1, 3), axis=0)) > 20
    # the PLY of the points with --strand_length, no mesh, the tangent colours
    tool.main(["--strands", ply, "--strand_length", "10", "--cameras", str(tmp_path / "cams.pkl"), "--size", "24x32", "--out",
               str(tmp_path / "b"), "--composed", "--speed_up", "4", "--mode", "tangent", "--supersample", "1", "--max_frames", "2"])
    assert sorted(os.listdir(tmp_path / "b" / "results")) == ["000000.png", "000001.png"]
    want = sv.render_strands(pts, (path[1].astype(np.float32).reshape(12), H, W), mode="tangent", supersample=1, fused=False)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "b" / "results" / "000001.png")), want.numpy())
