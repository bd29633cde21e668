"""The synthetic ground truth without a GPU (``--load_synthetic_rgba --load_synthetic_geom``): the torch-composed comparator of
gaussianhaircut_amd.ground_truth (``fused=False``) against the reference's golden (tests/golden/
make_reference_synthetic_golden.py: the reference's own loadCam / Camera on files), the `__host__ __device__` pixel function of
csrc/ghr_gt.h on the CPU through tests/hostsim/ghr_hostsim_synth.cpp against that comparator and a float64 model, the C ABI's
refusals, the kernel's resources and the reader of tools/synthstep.py.

Bars: tests/synth_cases.py.  Everything is bit-identical except (a) a bilinearly resized confidence or variance, held to
``|got - f64| <= 3 |torch32 - f64| + 9 * 2^-24 max|v|``, and (b) the angle plane of the pixel function, whose
sqrt / reciprocal / acos differ from torch's in the last places: the fragile rule of tests/test_eval_cpu.py against float64."""
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import helpers as hp
from tests import synth_cases as sc
from tests.golden import make_reference_synthetic_golden as mk
from tests.synth_cases import same_bits
from tests.test_ground_truth_cpu import conf_numpy

GOLDEN = os.path.join(hp.ROOT, "tests", "golden", "reference_synthetic_golden.npz")


@pytest.fixture(scope="module")
def gold():
    G = dict(np.load(GOLDEN))
    assert int(G["n_cases"]) == len(mk.CASES) and str(G["pillow"]) == "12.2.0"
    return G


def case_inputs(G, i):
    """(photograph's arrays, rendered arrays, (w, h), binarize, white, rgba, geom) of golden case i"""
    v, r, b, wb, rgba, geom = (int(x) for x in G["cases"][i])
    photo = {n: G["view/%s/%s" % (chr(v), n)] for n in ("image", "hair", "body", "angle", "var")}
    synth = {n: G["synth/%s/%s" % (chr(v), n)] for n in mk.SYNTH_NAMES}
    w, h = (int(x) for x in G["%d/size" % i])
    return photo, synth, (w, h), bool(b), bool(wb), bool(rgba), bool(geom)


def build(G, i, fused, to=lambda a: a):
    """golden case i through the public interface; ``to`` maps every array (numpy -> a tensor somewhere)"""
    from gaussianhaircut_amd import ground_truth as gt
    photo, synth, size, binarize, white, rgba, geom = case_inputs(G, i)
    kw = dict(white_background=white, binarize_masks=binarize, fused=fused)
    if rgba and geom:
        return gt.synthetic_view_ground_truth(to(synth["render"]), to(synth["head"]), to(synth["hair"]), to(synth["orient"]), to(synth["conf"]),
                                              size=size, **kw)
    if rgba:
        return gt.synthetic_view_ground_truth(to(synth["render"]), to(synth["head"]), to(synth["hair"]), angle=to(photo["angle"]),
                                              var=to(photo["var"]), size=size, **kw)
    return gt.view_ground_truth(to(photo["image"]), to(photo["hair"]), to(photo["body"]), resolution=size, orient=to(synth["orient"]),
                                orient_conf=to(synth["conf"]), **kw)


def check_case(G, i, v, what, resize_variance):
    """``v``: a ViewGroundTruth of numpy arrays.  ``resize_variance(var, (w, h))``: the variance resize of the path under test."""
    photo, synth, (w, h), _, _, _, geom = case_inputs(G, i)
    assert all(isinstance(x, np.ndarray) and x.dtype == np.float32 for x in v)
    assert same_bits(v.original_image, G["%d/image" % i]), (what, i, "image")
    assert same_bits(v.original_mask, G["%d/mask" % i]), (what, i, "mask")
    assert same_bits(v.original_orient_angle, G["%d/angle" % i]), (what, i, "angle")
    assert same_bits(v.original_mask_hair, G["%d/mask" % i][0:1]) and same_bits(v.original_mask_body, G["%d/mask" % i][1:2])
    if "%d/plane_dist" % i not in G:
        assert same_bits(v.original_orient_conf, G["%d/conf" % i]), (what, i, "conf")
    elif geom:
        sc.check_resized_plane(v.original_orient_conf, synth["conf"], G["%d/plane_dist" % i], "%s case %d" % (what, i))
    else:
        var = np.asarray(resize_variance(photo["var"], (w, h)))
        sc.check_resized_plane(var, photo["var"], G["%d/plane_dist" % i], "%s case %d" % (what, i))
        assert same_bits(v.original_orient_conf[0], conf_numpy(var)), (what, i, "conf of the resized variance")


# ---- 1. the golden and the comparator ------------------------------------------------------------------------------------------

def test_golden_has_the_cases_and_the_planted_bytes(gold):
    cases = [tuple(int(x) for x in row[1:]) for row in gold["cases"]]
    flags = {c[3:] for c in cases}
    assert flags == {(1, 1), (1, 0), (0, 1)}
    both = [(chr(int(row[0])),) + c for row, c in zip(gold["cases"], cases) if c[3:] == (1, 1)]
    assert {(v, r) for v, r, *_ in both} >= {("a", 1), ("a", 2), ("a", 4), ("b", 1), ("b", 2), ("b", 4), ("d", 33)}
    assert {(b, w) for _, _, b, w, _, _ in both} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert [tuple(gold["%d/size" % i]) for i in (0, 4, 6, 10)] == [(37, 53), (18, 26), (9, 13), (33, 41)]
    for k in mk.VIEWS:
        s = {n: gold["synth/%s/%s" % (k, n)] for n in mk.SYNTH_NAMES}
        for m in (s["hair"], s["head"]):
            assert (m == 127).any() and (m == 128).any()
        assert all((s["orient"] == b).any() for b in (0, 180, 200, 255))
        assert (s["conf"] >= 0).all() and (s["conf"] == 0).any() and (s["conf"] == 1e6).any() and s["conf"].dtype == np.float32
    # / 255, not / 180 and no clamp: byte 200 reads 200 / 255, byte 255 reads 1
    i = 0
    ang, orient = gold["%d/angle" % i][0], gold["synth/a/orient"]
    assert same_bits(ang, sc.t255()[orient]) and (ang[orient == 255] == 1).all() and (ang[orient == 200] < 0.79).all()


@pytest.mark.parametrize("i", range(len(mk.CASES)))
def test_comparator_equals_the_reference_camera(gold, i):
    from gaussianhaircut_amd import ground_truth as gt
    v = build(gold, i, fused=False)
    check_case(gold, i, v, "comparator", lambda var, size: gt.resize_variance(var, size, fused=False))
    t = build(gold, i, fused=False, to=torch.from_numpy)
    assert all(isinstance(x, torch.Tensor) for x in t) and all(same_bits(a.numpy(), b) for a, b in zip(t, v))


def test_pairs_of_geometry_inputs_are_checked(gold):
    from gaussianhaircut_amd import ground_truth as gt
    photo, s, _, _, _, _, _ = case_inputs(gold, 0)
    base = (s["render"], s["head"], s["hair"])
    for kw in (dict(), dict(orient=s["orient"]), dict(orient_conf=s["conf"]), dict(angle=photo["angle"]), dict(var=photo["var"]),
               dict(orient=s["orient"], orient_conf=s["conf"], angle=photo["angle"], var=photo["var"]),
               dict(orient=s["orient"], orient_conf=s["conf"], angle=photo["angle"]), dict(orient=s["orient"], var=photo["var"])):
        with pytest.raises(ValueError, match="orient|angle"):
            gt.synthetic_view_ground_truth(*base, fused=False, **kw)
    pbase = (photo["image"], photo["hair"], photo["body"])
    for kw in (dict(orient=s["orient"]), dict(orient_conf=s["conf"]), dict(orient=s["orient"], orient_conf=s["conf"], var=photo["var"])):
        with pytest.raises(ValueError, match="orient"):
            gt.view_ground_truth(*pbase, fused=False, **kw)
    with pytest.raises(ValueError, match="float"):
        gt.view_ground_truth(*pbase, fused=False, orient=s["orient"], orient_conf=s["orient"])
    with pytest.raises(ValueError):
        gt.ground_truth_from_render(np.zeros((9, 4, 4), np.float32), fused=False)
    with pytest.raises(ValueError):
        gt.ground_truth_from_render(torch.zeros(10, 4, 4), fused=True)   # the kernel has no CPU path
    # the confidence file's [1,H,W] and the masks' RGB forms are taken as loadCam takes them
    a = gt.synthetic_view_ground_truth(*base, s["orient"], s["conf"], fused=False)
    b = gt.synthetic_view_ground_truth(s["render"], mk.rgb3(s["head"]), mk.rgb3(s["hair"]), mk.rgb3(s["orient"]), s["conf"][None], fused=False)
    assert all(same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("shape", [(1, 1), (1, 5), (7, 257), (53, 37)])
def test_from_render_comparator_is_the_file_route(shape):
    """ground_truth_from_render(fused=False) = evaluation.products_torch's arrays through synthetic_view_ground_truth"""
    from gaussianhaircut_amd import evaluation as ev
    from gaussianhaircut_amd import ground_truth as gt
    packed, _ = sc.make_packed(*shape)
    p = ev.products_torch(torch.from_numpy(packed))
    for white, binarize in ((False, False), (True, True)):
        direct = gt.ground_truth_from_render(packed, white_background=white, binarize_masks=binarize, fused=False)
        files = gt.synthetic_view_ground_truth(p["render"], p["head_mask"], p["hair_mask"], p["orient"], p["orient_conf"],
                                               white_background=white, binarize_masks=binarize, fused=False)
        assert all(same_bits(x, y) for x, y in zip(direct, files)), (shape, white, binarize)
    core = gt._core_products_torch(torch.from_numpy(packed))
    for x, name in zip(core, ("render", "hair_mask", "head_mask", "orient", "orient_conf")):
        assert same_bits(x.numpy(), p[name]), name
    H, W = shape
    if H > 8:
        size = (18, 26)
        direct = gt.ground_truth_from_render(packed, size=size, fused=False)
        files = gt.synthetic_view_ground_truth(p["render"], p["head_mask"], p["hair_mask"], p["orient"], p["orient_conf"], size=size, fused=False)
        assert tuple(direct.original_image.shape) == (3, 26, 18) and all(same_bits(x, y) for x, y in zip(direct, files))
        assert same_bits(gt.ground_truth_from_render(packed, size=(W, H), fused=False).original_image,
                         gt.ground_truth_from_render(packed, fused=False).original_image)


def test_module_still_imports_without_pillow():
    import ast
    tree = ast.parse(open(os.path.join(hp.ROOT, "gaussianhaircut_amd", "ground_truth.py")).read())
    mods = [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names] + \
           [n.module or "" for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
    assert not any(m.split(".")[0] == "PIL" for m in mods), mods
    src = open(os.path.join(hp.ROOT, "gaussianhaircut_amd", "ground_truth.py")).read()
    assert "torch.load" not in src and "torch.save" not in src


# ---- 2. host simulator -----------------------------------------------------------------------------------------------------------

def _build():
    """as tests/test_eval_cpu.py builds its file"""
    src = os.path.join(hp.ROOT, "tests", "hostsim", "ghr_hostsim_synth.cpp")
    out_dir = os.path.join(hp.ROOT, "tests", "hostsim", "_build")
    so = os.path.join(out_dir, "libghr_hostsim_synth.so")
    csrc = os.path.join(hp.ROOT, "gaussianhaircut_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(out_dir, exist_ok=True)
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-x", "hip", "-O2", "-std=c++17", "-ffp-contract=off",
                        "-fPIC", "-shared", "-o", so, src], check=True)
    return so


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def sim():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    return ctypes.CDLL(_build())


def sim_from_render(sim, packed, white, binarize):
    _, H, W = packed.shape
    packed = np.ascontiguousarray(packed, np.float32)
    table = sc.t255()
    o = [np.full((c, H, W), np.nan, np.float32) for c in (3, 2, 1, 1)]
    sim.ghrsim_gt_from_render(W, H, _p(packed), _p(table), int(white), int(binarize), *(_p(x) for x in o))
    return o


@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_hostsim_pixel_function_equals_the_comparator(sim, shape):
    from gaussianhaircut_amd import ground_truth as gt
    packed, planted = sc.make_packed(*shape)
    for white, binarize in ((False, False), (True, False), (False, True), (True, True)):
        img, mask, angle, conf = sim_from_render(sim, packed, white, binarize)
        ref = gt.ground_truth_from_render(packed, white_background=white, binarize_masks=binarize, fused=False)
        what = "host-sim %dx%d white %d binarize %d" % (shape + (white, binarize))
        assert same_bits(img, ref.original_image), what
        assert same_bits(mask, ref.original_mask), what
        assert same_bits(conf, ref.original_orient_conf), what
        assert not np.isnan(angle).any()
        sc.check_angle(angle, packed, planted, what)
    if mask[1].size >= 64:   # (binarised here) an image that holds the planted block has both sides of level 128
        assert (mask[1] == 0).any() and (mask[1] == 1).any() and ((mask[1] == 0) | (mask[1] == 1)).all()


def test_comparator_angle_holds_the_fragile_rule_too():
    from gaussianhaircut_amd import ground_truth as gt
    for shape in ((7, 257), (64, 64)):
        packed, planted = sc.make_packed(*shape)
        ref = gt.ground_truth_from_render(packed, fused=False)
        sc.check_angle(ref.original_orient_angle, packed, planted, "comparator %dx%d" % shape)


# ---- 3. C ABI ----------------------------------------------------------------------------------------------------------------------

def test_c_abi_refuses_bad_arguments_before_any_launch():
    from gaussianhaircut_amd import _lib
    L = _lib.lib()
    assert "ghr_gt_from_render" in _lib.EXPORTS and hasattr(L, "ghr_gt_from_render") and L.ghr_gt_from_render.argtypes
    hdr = open(os.path.join(hp.ROOT, "include", "ghr.h")).read()
    assert re.search(r"\bint ghr_gt_from_render\(", hdr) and int(L.ghr_abi_version()) == _lib.ABI_VERSION
    assert "ghr_products.h" in _lib.HEADERS and os.path.exists(os.path.join(_lib.CSRC, "ghr_products.h"))
    X = 0x1000   # stands for a buffer: a refused call touches none

    def call(W=8, H=8, renders=X, table=X, white=0, binarize=0, o_img=X, o_mask=X, o_ang=X, o_conf=X):
        return L.ghr_gt_from_render(None, W, H, renders, table, white, binarize, o_img, o_mask, o_ang, o_conf)

    bad = [dict(W=0), dict(W=-3), dict(H=0), dict(H=-1), dict(renders=None), dict(table=None), dict(o_img=None), dict(o_mask=None),
           dict(o_ang=None), dict(o_conf=None), dict(white=2), dict(white=-1)]
    for kw in bad:
        assert call(**kw) == _lib.GHR_E_INVALID, kw
        assert b"ghr_gt_from_render" in L.ghr_last_error(), (kw, L.ghr_last_error())
    from gaussianhaircut_amd import ground_truth as gt
    with pytest.raises(AssertionError, match="no CPU path"):
        gt.from_render_fused(torch.zeros(10, 4, 4))


# ---- 4. kernel resources ------------------------------------------------------------------------------------------------------------

def test_from_render_kernels_compile_without_a_private_segment(tmp_path):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    src = tmp_path / "gt_synth.hip"
    src.write_text('#include "%s"\n' % os.path.join(hp.ROOT, "gaussianhaircut_amd", "csrc", "ghr_gt.h") +
                   "".join("template __global__ void ghr::k_gt_from_render<%s>(ghr::GtFromRenderArgs);\n" % n for n in ("true", "false")))
    res = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only",
                          "-c", "-o", str(tmp_path / "o.o"), "-Rpass-analysis=kernel-resource-usage", str(src)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    seen = {}
    for b in re.split(r"Function Name: ", res.stderr)[1:]:
        name = b.split()[0]
        if "k_gt_from_render" not in name:
            continue
        get = lambda key: int(re.search(re.escape(key) + r": (\d+)", b).group(1))   # noqa: E731
        assert get("ScratchSize [bytes/lane]") == 0 and get("VGPRs Spill") == 0 and get("SGPRs Spill") == 0, b
        assert get("LDS Size [bytes/block]") == 1024, b   # the / 255 table
        seen[name] = (get("VGPRs") + get("AGPRs"), get("Occupancy [waves/SIMD]"))
    assert len(seen) == 2 and all(occ >= 8 for _, occ in seen.values()), seen   # a streaming kernel: full occupancy


# ---- 5. the tool's reader --------------------------------------------------------------------------------------------------------

def test_tool_reads_what_render_views_writes(tmp_path):
    """tools/render_views.py's files, read back by tools/synthstep.py as loadCam opens them, give ground_truth_from_render's bits"""
    pytest.importorskip("PIL.Image")
    from gaussianhaircut_amd import evaluation as ev
    from gaussianhaircut_amd import ground_truth as gt
    tools = {}
    for name in ("render_views", "synthstep"):
        spec = importlib.util.spec_from_file_location("tool_" + name, os.path.join(hp.ROOT, "tools", name + ".py"))
        tools[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(tools[name])
    packed, _ = sc.make_packed(53, 37)
    p = ev.products_torch(torch.from_numpy(packed))
    p["name"] = "00000"
    assert tools["render_views"].write_products(str(tmp_path), "train", 30000, [p], scene_suffix="_cropped") == 1
    f = tools["synthstep"].read_view(str(tmp_path / "train_cropped" / "ours_30000"), "00000")
    assert f["render"].shape == (53, 37, 3) and f["hair_mask"].shape == (53, 37, 3) and f["orient_conf"].shape == (1, 53, 37)
    for white, binarize in ((False, True), (True, False)):
        files = gt.synthetic_view_ground_truth(f["render"], f["head_mask"], f["hair_mask"], f["orient"], f["orient_conf"],
                                               white_background=white, binarize_masks=binarize, fused=False)
        direct = gt.ground_truth_from_render(packed, white_background=white, binarize_masks=binarize, fused=False)
        assert all(same_bits(x, y) for x, y in zip(files, direct))
