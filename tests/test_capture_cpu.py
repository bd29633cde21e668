"""Synthetic captures (csrc/ghr_capture.h, gaussianhaircut_amd/synthetic_capture.py) without a GPU.

 1. the PyTorch comparator (capture_view(fused=False)) on CPU tensors against the numpy MODEL of tests/capture_cases.py: the three
    byte planes and the bits of var, on every case (every case of strand_view_cases.CASES at s = 1, 2, 4 and the planted ones);
 2. the model against a float64 atan2 TRUTH on the same float32 screen points: the angle is never more than one bin away
    (circularly) and equal wherever the truth lies more than 1e-3 rad from a bin boundary -- derived: adjacent bins' scores differ
    by about 0.07 d |Sigma| at d from the boundary, float32 error is about 1e-6 |Sigma| --, var within 1e-5, both masks exact; the
    planted answers (two strands crossing at 90 degrees: angle 0, var 0.5; directions on a bin; directions 1e-6 rad from a boundary);
 3. capture_view(...).image equals render_strands(...); view_ground_truth(*capture) equals capture_ground_truth's tensors;
 4. a host walk of the product's per-pixel functions (tests/hostsim/ghr_hostsim_capture.cpp), pixel by pixel and in the kernel's
    quads, bit for bit on every case; the same walks in a stand-alone program built with -fsanitize=address,undefined (nothing
    sanitized is loaded here);
 5. the C ABI: declared, exported, ABI 20, and the recorded refusal table tests/golden/capture_refusals.json: every refusal is
    answered before the runtime is touched;
 6. tools/synthetic_capture.py: write, then check, in a temporary directory;
 7. the convention check's figures with the CPU forms (tests/capture_convention.py), which the device's test is held to."""
import ctypes
import importlib.util
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd import ground_truth as gt
from gaussianhaircut_amd import strand_view as sv
from gaussianhaircut_amd import synthetic_capture as cap
from gaussianhaircut_amd import visibility as vis
from gaussianhaircut_amd.scene.cameras import ring_cameras
from tests import capture_cases as cc
from tests import capture_convention as conv
from tests import helpers as hp
from tests import strand_view_cases as sc

DEPS = ["ghr_hostsim_capture.cpp", "ghr_capture.h", "ghr_tilelists.h", "ghr_mesh.h"]
REFUSALS = os.path.join(hp.ROOT, "tests", "golden", "capture_refusals.json")


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == np.ascontiguousarray(b).tobytes()


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _light(c):
    """eye and light as the strand-preview tests form them: an affine view has no camera centre, one is given"""
    sh = sc.shading(c["M"])
    return dict(eye=sh["eye"], light=sh["light"])


def _api(c, **kw):
    kw = dict(_light(c), **kw)
    return cap.capture_view(c["points"], (c["M"], c["H"], c["W"]), mesh=None if c["v"] is None else (c["v"], c["f"]), supersample=c["s"],
                            half_width=c["r"], head_bias=c["bias"], near=float(cc.NEAR), var_floor=c["var_floor"], fused=False, **kw)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,s", cc.CASES, ids=cc.IDS)
def test_torch_comparator_equals_the_model_on_cpu_tensors(name, s):
    c = cc.case(name, s)
    hair, body, angle, var, _, _ = cc.model(name, s)
    got = _api(c)
    assert [g.dtype for g in got] == [torch.uint8] * 4 + [torch.float32] and tuple(got.image.shape) == (c["H"], c["W"], 3)
    assert _same_bits(got.mask_hair.numpy(), hair) and _same_bits(got.mask_body.numpy(), body)
    assert _same_bits(got.angle.numpy(), angle) and _same_bits(got.var.numpy(), var)


def test_table_is_the_float64_one_rounded_once():
    T = cap.angle_table()
    assert T.dtype == np.float32 and T.shape == (180, 2) and _same_bits(T, cc.table())
    assert T[0, 0] == 1 and T[0, 1] == 0 and T[90, 0] == -1 and T[45, 1] == 1


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,s", cc.CASES, ids=cc.IDS)
def test_model_agrees_with_the_float64_truth(name, s):
    c = cc.case(name, s)
    hair, body, angle, var, _, _ = cc.model(name, s)
    theta, var64, _ = cc.truth_capture(c["points"], c["Ms"], c["H"], c["W"], s, c["seg"], c["var_floor"])
    x = theta / (np.pi / 180.0)                       # the truth in bins
    nearest = np.mod(np.rint(x), 180).astype(np.int64)
    from_boundary = np.abs(np.abs(x - np.rint(x)) - 0.5) * (np.pi / 180.0)
    d = np.abs(angle.astype(np.int64) - nearest)
    d = np.minimum(d, 180 - d)
    assert int(d.max(initial=0)) <= 1, (name, s)
    safe = from_boundary > 1e-3
    assert np.array_equal(angle[safe], nearest[safe]), (name, s)
    assert float(np.abs(var.astype(np.float64) - var64).max(initial=0.0)) <= 1e-5
    n = s * s
    K = c["points"].shape[0] * (c["points"].shape[1] - 1)
    n_hair = ((c["seg"] >= 0) & (c["seg"] < K)).reshape(c["H"], s, c["W"], s).sum((1, 3))
    n_face = ((c["seg"] < 0) & (c["face"] >= 0) & (c["face"] < c["F"])).reshape(c["H"], s, c["W"], s).sum((1, 3))
    assert np.array_equal(hair, (255 * n_hair + n // 2) // n) and np.array_equal(body, (255 * (n_hair + n_face) + n // 2) // n)
    assert (body >= hair).all()


def _only(seg, k, s):
    """the pixels of a 20 x 50 case in which strand k (one segment) is the only hair"""
    mine = np.where(seg == k, 1, 0).reshape(20, s, 50, s).sum((1, 3))
    return (mine > 0) & (mine == np.where(seg >= 0, 1, 0).reshape(20, s, 50, s).sum((1, 3)))


def test_planted_answers():
    hair, body, angle, var, C, S = cc.model("crossing-3x3", 4)
    assert hair[1, 1] == (255 * 6 + 8) // 16 and C[1, 1] == 0 and S[1, 1] == 0 and angle[1, 1] == 0 and var[1, 1] == np.float32(0.5)
    assert not hair[0].any() and (var == np.float32(0.5)).all() and not angle.any()
    # no strand, no head: masks 0, angle 0, var 0.5 + var_floor
    for s in cc.SUPERSAMPLES:
        hair, body, angle, var, _, _ = cc.model("empty-3x5", s)
        assert not hair.any() and not body.any() and not angle.any() and (var == np.float32(0.5)).all()
        hair, body, angle, var, _, _ = cc.model("head-only-17x33", s)
        assert not hair.any() and body.max() == 255 and 0 < (body > 0).sum() < body.size and (var == np.float32(0.5)).all()
        hair, body, _, _, _, _ = cc.model("front-and-behind-17x33", s)
        c = cc.case("front-and-behind-17x33", s)
        assert {0, 1, 2, 3} <= set(np.unique(c["seg"]).tolist())                 # the strand in front is seen over the head
        on_head = c["face"] >= 0
        assert on_head.any() and not set(np.unique(c["seg"][:, 4 * s:-4 * s]).tolist()) & {5, 6}   # the one behind is hidden by it
        assert (hair > 0).any() and ((body == 255) & (hair == 0)).any()
    # a segment along the view ray covers its disc (hair) and adds no direction: var 0.5 there
    hair, _, angle, var, _, _ = cc.model("along-the-ray-5x6", 1)
    assert hair[2, 2] == 255 and angle[2, 2] == 0 and var[2, 2] == np.float32(0.5)
    # var_floor is added: the 3 x 5 comb has 0.094
    assert cc.model("comb-3x5", 2)[3].min() >= np.float32(0.094) and cc.model("comb-3x5", 2)[3].max() <= np.float32(0.594)
    # a strand thinner than a subsample is seen by the few centres it passes: never opaque at s = 4
    hair = cc.model("thin-17x33", 4)[0]
    assert 0 < hair.max() < 255
    # directions exactly on a bin give that bin wherever the strand fills the pixel
    for s in cc.SUPERSAMPLES:
        c = cc.case("on-bins-20x50", s)
        hair, _, angle, var, _, _ = cc.model("on-bins-20x50", s)
        K = c["points"].shape[0]
        for k, deg in enumerate(cc.THETAS_ON):
            own = _only(c["seg"], k, s)
            assert own.sum() >= 4, (s, deg)
            assert (angle[own] == deg).all(), (s, deg, np.unique(angle[own]))
            share = np.where(c["seg"] == k, 1, 0).reshape(20, s, 50, s).sum((1, 3))[own] / float(s * s)
            assert float(np.abs(var[own] - 0.5 * (1 - share)).max()) <= 1e-6      # one direction: the resultant is the covered share
        assert K == len(cc.THETAS_ON)
        # 1e-6 rad from a boundary k + 0.5: one of the two bins beside it
        c = cc.case("near-boundaries-20x50", s)
        angle = cc.model("near-boundaries-20x50", s)[2]
        for k, lo in enumerate(b for b in (0, 29, 44, 89, 134, 178) for _ in range(2)):
            own = _only(c["seg"], k, s)
            assert own.sum() >= 4 and set(np.unique(angle[own]).tolist()) <= {lo, (lo + 1) % 180}, (s, k, np.unique(angle[own]))


def test_docstring_states_the_banks_own_variance_and_the_header_the_definition():
    assert "0.094" in cap.capture_view.__doc__
    hdr = open(os.path.join(hp.CSRC, "ghr_capture.h")).read()
    for text in ("(255 n_hair + n / 2) / n", "c2 = (dy dy - dx dx) / len2", "s2 = (2.f (dx dy)) / len2", "a-major",
                 "var_floor + 0.5f fmaxf(0.f, 1.f - sqrtf(C C + S S) / (float)n)"):
        assert text in hdr, text


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,s,kw", [("ss2-17x33", 2, {}), ("ss4-17x33", 4, dict(shadows=True, shadow_size=64)),
                                       ("hair-front-15x17", 1, dict(colors=(0.7, 0.5, 0.2), ambient=0.3)),
                                       ("front-and-behind-17x33", 4, dict(shadows=True, shadow_size=48)), ("comb-4x9", 2, {})])
def test_image_is_render_strands_picture(name, s, kw):
    c = cc.case(name, s)
    got = _api(c, **kw)
    want = sv.render_strands(c["points"], (c["M"], c["H"], c["W"]), mesh=None if c["v"] is None else (c["v"], c["f"]), supersample=s,
                             half_width=c["r"], head_bias=c["bias"], near=float(cc.NEAR), fused=False, **dict(_light(c), **kw))
    assert torch.equal(got.image, want) and len(torch.unique(want)) > 2
    plain = _api(c)
    for a, b in zip(got[1:], plain[1:]):                      # the maps do not depend on the shading
        assert torch.equal(a, b)


def test_per_strand_colours_and_refusals():
    c = cc.case("ss2-17x33", 2)
    base = np.random.default_rng(0).uniform(0.1, 0.9, (c["points"].shape[0], 3)).astype(np.float32)
    got = _api(c, colors=base)
    want = sv.render_strands(c["points"], (c["M"], 17, 33), mesh=(c["v"], c["f"]), colors=base, supersample=2, half_width=c["r"],
                             near=float(cc.NEAR), fused=False, **_light(c))
    assert torch.equal(got.image, want)
    with pytest.raises(RuntimeError, match="no CPU path"):
        cap.capture_view(c["points"], (c["M"], 17, 33), device="cpu")
    with pytest.raises(ValueError, match="var_floor"):
        cap.capture_view(c["points"], (c["M"], 17, 33), var_floor=-0.1, fused=False)
    with pytest.raises(ValueError, match="var_floor"):
        cap.capture_view(c["points"], (c["M"], 17, 33), var_floor=float("nan"), fused=False)
    with pytest.raises(ValueError, match="supersample"):
        cap.capture_view(c["points"], (c["M"], 17, 33), supersample=3, fused=False)
    with pytest.raises(ValueError, match="two points"):
        cap.capture_view(c["points"][:, :1], (c["M"], 17, 33), fused=False)


def test_capture_ground_truth_is_view_ground_truth_of_the_capture():
    pts, (v, f) = sc.hair(40, 12, 11), sc.meshes()["small_sphere"]
    cams = ring_cameras(4, 32, 24, radius=4.0)
    for white, binarize in ((False, False), (True, True)):
        out = cap.capture_ground_truth(pts, cams, mesh=(v, f), supersample=2, var_floor=0.05, fused=False, white_background=white,
                                       binarize_masks=binarize)
        assert out == list(cams)
        for cam in cams:
            cv = cap.capture_view(pts, vis.view_matrix_from_camera(cam), mesh=(v, f), supersample=2, var_floor=0.05, fused=False)
            want = gt.view_ground_truth(*cv, white_background=white, binarize_masks=binarize)
            assert tuple(cam.original_image.shape) == (3, 24, 32) and float(cam.original_mask[0].max()) > 0
            assert torch.equal(cam.original_image, want.original_image) and torch.equal(cam.original_mask, want.original_mask)
            assert torch.equal(cam.original_orient_angle, want.original_orient_angle)
            assert torch.equal(cam.original_orient_conf, want.original_orient_conf)
            assert torch.equal(cam.original_orient_angle[0], (cv.angle.float() / 180.0).clamp(0, 1))


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim():
    L = ctypes.CDLL(hp.compile_hostsim("libghr_hostsim_capture.so", "ghr_hostsim_capture.cpp", ["-O2", "-fPIC", "-shared"], DEPS))
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.ghrsim_capture.argtypes = [i32, i32, vp, vp, f32, i32, i32, i32, i32, vp, vp, vp, f32, vp, vp, vp, vp, i32]
    assert L.ghrsim_cap_bins() == cc.BINS == cap.BINS
    return L


@pytest.mark.parametrize("name,s", cc.CASES, ids=cc.IDS)
def test_host_walks_equal_the_model_bit_for_bit(sim, name, s):
    c = cc.case(name, s)
    want = cc.model(name, s)
    H, W = c["H"], c["W"]
    S, L = c["points"].shape[:2]
    T = cc.table()
    for walk in (0, 1):
        outs = [np.full((H, W), 7, np.uint8) for _ in range(3)] + [np.full((H, W), 7, np.float32)]
        assert sim.ghrsim_capture(S, L, _p(c["points"]), _p(c["Ms"]), float(cc.NEAR), H, W, s, c["F"], _p(c["seg"]), _p(c["face"]), _p(T),
                                  float(np.float32(c["var_floor"])), *[_p(o) for o in outs], walk) == 0
        for got, w in zip(outs, want[:4]):
            assert _same_bits(got, w), (name, s, walk)


def test_sanitized_stand_alone_program_runs_the_cases_clean(tmp_path):
    """ghr_capture_selfcheck: both walks under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own (exact-size
    buffers)."""
    san = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    if os.path.basename(hp.host_cxx()) == "g++":
        san += ["-static-libasan", "-static-libubsan"]
    exe = hp.compile_hostsim("ghr_capture_selfcheck_san", "ghr_capture_selfcheck.cpp", san, DEPS)
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as fh:
        fh.write(cc.table().tobytes())
        for name, s in cc.SMALL:
            c = cc.case(name, s)
            S, L = c["points"].shape[:2]
            fh.write(np.array([S, L, c["H"], c["W"], s, c["F"]], np.int32).tobytes())
            fh.write(np.concatenate([c["Ms"], [cc.NEAR, c["var_floor"]]]).astype(np.float32).tobytes())
            for arr in (c["points"], c["seg"], c["face"]) + cc.model(name, s)[:4]:
                fh.write(np.ascontiguousarray(arr).tobytes())
    res = subprocess.run([exe, path], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "%d cases ok" % len(cc.SMALL) in res.stdout and "runtime error" not in res.stderr, res.stdout + res.stderr
    assert len(cc.SMALL) > 100


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
_POINTERS = {"null": None, "fake": 4096, "odd": 4098, "byte": 4097, "eight": 4104}


def _call(L, M, overrides):
    a = dict(S=8, L=12, points="fake", M="M", near=1e-3, H=48, W=64, s=4, F=12, seg="fake", face="fake", table="fake", var_floor=0.0,
             hair="fake", body="fake", angle="fake", var="fake")
    a.update(overrides)

    def ptr(x):
        return None if _POINTERS[x] is None else ctypes.c_void_p(_POINTERS[x])
    return L.ghr_strandview_capture(None, a["S"], a["L"], ptr(a["points"]), None if a["M"] == "null" else ctypes.byref(M), float(a["near"]),
                                    a["H"], a["W"], a["s"], a["F"], ptr(a["seg"]), ptr(a["face"]), ptr(a["table"]), float(a["var_floor"]),
                                    ptr(a["hair"]), ptr(a["body"]), ptr(a["angle"]), ptr(a["var"]))


def test_c_abi_refusals_are_the_recorded_table_and_launch_nothing():
    """every pointer is fake (never dereferenced): a call that is not refused before the runtime would fault here"""
    L = _lib.lib()
    assert _lib.ABI_VERSION == 20 == L.ghr_abi_version()
    assert "ghr_strandview_capture" in _lib.EXPORTS and L.ghr_strandview_capture.argtypes and "ghr_capture.h" in _lib.HEADERS
    assert "ghr_strandview_capture(" in open(os.path.join(hp.ROOT, "include", "ghr.h")).read()
    M = (ctypes.c_float * 12)(*([1.0] * 12))
    with open(REFUSALS) as fh:
        rows = json.load(fh)
    assert len(rows) >= 30
    seen = set()
    for row in rows:
        rc = _call(L, M, row["args"])
        assert rc == row["code"], (row, rc)
        if rc != _lib.GHR_OK:
            assert L.ghr_last_error().decode() == row["error"], (row, L.ghr_last_error())
            seen.add(row["error"])
    # what the entry must refuse, each with a text of its own
    for text in ("L < 2", "supersample", "var_floor", "points is NULL", "M is NULL", "table is NULL", "pix_to_segment or pix_to_face_out",
                 "output plane", "4-B aligned", "near", "negative size", "H * W"):
        assert any(text in e for e in seen), text
    valid = [row for row in rows if row["code"] == _lib.GHR_OK]
    assert len(valid) >= 2                                     # H * W == 0 with every plane NULL (and S == 0, F == 0 with it)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phi0", conv.PHI0)
def test_convention_figures_of_the_cpu_forms_are_the_recorded_ones(phi0):
    """the figures the device's test adds its 2 and 3 degrees to (tests/test_gpu_capture.py), measured here with the oracle backend
    and fused=False: no offset and no mirrored angle between the capture's byte, render()'s orient_angle and the Gabor bank's byte"""
    got = conv.measure(phi0, "cpu")
    assert got["pixels"] >= conv.MIN_PIXELS
    for key, want in zip(("a", "b"), conv.CPU_MEASURED[phi0]):
        assert want[0] - 0.02 <= got[key][0] <= want[0] + 0.005 and want[1] - 0.11 <= got[key][1] <= want[1] + 0.005, (key, got, want)
    assert abs(got["signed_a"]) <= 0.05 and abs(got["signed_b"]) <= 0.5, got


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_tool_writes_a_scene_and_checks_it(tmp_path):
    pytest.importorskip("PIL")
    from PIL import Image
    spec = importlib.util.spec_from_file_location("synthetic_capture_tool", os.path.join(hp.ROOT, "tools", "synthetic_capture.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = str(tmp_path / "scene")
    pts = sc.hair(30, 10, 2, through=False)
    np.save(tmp_path / "groom.npy", pts)
    v, f = sc.meshes()["small_sphere"]
    tool.write_obj(str(tmp_path / "head.obj"), v, f)
    n = tool.main(["write", "--out", out, "--strands", str(tmp_path / "groom.npy"), "--mesh", str(tmp_path / "head.obj"), "--views", "3",
                   "--size", "24x32", "--supersample", "2", "--composed"])
    assert n == 3
    for d, ext in (("images", "png"), ("masks/hair", "png"), ("masks/body", "png"), ("orientations/angles", "png"),
                   ("orientations/vars", "npy")):
        assert sorted(os.listdir(os.path.join(out, d))) == ["%04d.%s" % (k, ext) for k in range(3)], d
    assert os.path.exists(os.path.join(out, "flame_fitting/stage_3/mesh_final.obj"))
    assert _same_bits(np.load(os.path.join(out, "strands_gt.npy")), pts)
    P = np.load(os.path.join(out, "projection.npy"))
    assert P.shape == (3, 4, 4) and P.dtype == np.float64
    K, R, t = vis.decompose_projection(P[1, :3])
    assert np.isclose(K[0, 2], 32.0) and np.isclose(K[1, 2], 24.0)          # twice the written size: the reader halves it
    assert np.load(os.path.join(out, "orientations/vars/0001.npy")).dtype == np.float16
    assert np.asarray(Image.open(os.path.join(out, "masks/hair/0001.png"))).max() > 0
    assert np.asarray(Image.open(os.path.join(out, "orientations/angles/0001.png"))).max() < 180
    cams = tool.main(["check", "--scene", out, "--supersample", "2", "--composed"])
    assert len(cams) == 3 and tuple(cams[0].original_image.shape) == (3, 24, 32) and cams[0].original_orient_conf is not None
    # a changed byte is found
    img = np.array(Image.open(os.path.join(out, "masks/body/0002.png")))
    img[0, 0] ^= 1
    Image.fromarray(img).save(os.path.join(out, "masks/body/0002.png"))
    with pytest.raises(SystemExit, match="mask_body differs"):
        tool.main(["check", "--scene", out, "--supersample", "2", "--composed"])
