"""Head-mesh visibility (csrc/ghr_visibility.h, gaussianhaircut_amd/visibility.py, the scalp cut of between_stages.py) without
a GPU.

Every result is an integer or a byte: every comparison is exact.
 1. the numpy float32 MODEL of the definition (tests/visibility_cases.py) against a float64 truth on the same screen vertices:
    pix_to_face is equal wherever the pixel is not FRAGILE, and fragile pixels are at most 1 % of the covered ones;
 2. the tie lattices: every pixel centre inside the grid is covered by exactly ONE face; on the duplicate stack the lowest
    index wins;
 3. the product's own per-element functions and a host walk of the tile lists (tests/hostsim/ghr_hostsim_visibility.cpp, every
    index checked) against the model, bit for bit, on every case; the same cases through a stand-alone program built with
    -fsanitize=address,undefined (nothing sanitized is loaded here);
 4. the PyTorch comparator (fused=False) on CPU tensors against the model; visible_vertex_mask, cut_scalp, scalp_uv_mask,
    write_scalp_data and views_from_projections on hand-checked inputs; the refusals of the C ABI."""
import ctypes
import os
import pickle
import subprocess

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd import between_stages as bs
from gaussianhaircut_amd import visibility as vis
from gaussianhaircut_amd.mesh import read_obj
from tests import helpers as hp
from tests import visibility_cases as vc

CASES = list(vc.CASES)
DEPS = ["ghr_hostsim_visibility.cpp", "ghr_hostsim_tilelists.h", "ghr_visibility.h", "ghr_tilelists.h", "ghr_mesh.h"]


@pytest.fixture(scope="module")
def sim():
    L = ctypes.CDLL(hp.compile_hostsim("libghr_hostsim_visibility.so", "ghr_hostsim_visibility.cpp", ["-O2", "-fPIC", "-shared"], DEPS))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    L.ghrsim_vis_sizes.argtypes = [i64, i64, i64, i64, ctypes.POINTER(ctypes.c_ulonglong), vp]
    L.ghrsim_vis_head_mask.argtypes = [i32, i32, vp, vp, vp]
    L.ghrsim_vis_view.argtypes = [i32, vp, i32, vp, vp, ctypes.c_float, i32, i32] + [vp] * 7
    assert L.ghrsim_vis_chunk() == vc.CHUNK and L.ghrsim_vis_big_rect() == vc.BIG_RECT
    return L


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _sim_view(sim, v, f, M, H, W, body, hair, cnt=None, cnt_head=None):
    pix, visp = np.full((H, W), 7, np.int32), np.full((H, W), 7, np.uint8)
    cnt = np.zeros(len(v), np.int32) if cnt is None else cnt
    cnt_head = np.zeros(len(v), np.int32) if cnt_head is None else cnt_head
    tiles = np.zeros(((H + 15) // 16) * ((W + 15) // 16), np.uint32)
    assert sim.ghrsim_vis_view(len(v), _p(v), len(f), _p(f), _p(M), float(vc.NEAR), H, W, _p(body), _p(hair), _p(pix), _p(visp),
                               _p(cnt), _p(cnt_head), _p(tiles)) == 0
    return pix, visp, cnt, cnt_head, tiles


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
def test_model_agrees_with_the_float64_truth_away_from_fragile_pixels():
    worst = (0.0, "")
    for name in CASES:
        if name.startswith(vc.EXACT_ONLY):
            continue
        v, f, M, H, W, _, _ = vc.case(name)
        pix = vc.model_case(name)[0]
        truth, fragile = vc.truth_rasterize(v, f, M, H, W)
        assert np.array_equal(pix[~fragile], truth[~fragile]), name
        covered = int((pix >= 0).sum())
        assert covered > 0, name
        share = float((fragile & (pix >= 0)).sum()) / covered
        worst = max(worst, (share, name))
        assert share <= 0.01, (name, share)
    print("largest share of fragile pixels among the covered: %.4f (%s)" % worst)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("lattice")])
def test_tie_lattice_gives_every_inner_pixel_to_exactly_one_face(name):
    v, f, M, H, W, _, _ = vc.case(name)
    pix, count = vc.model_rasterize(v, f, M, H, W, return_cover_count=True)
    lo, hi = vc.lattice_extent(10, 0.5 if "latticeB" in name else 0.0)
    ii, jj = np.mgrid[0:H, 0:W]
    x, y = jj + 0.5, ii + 0.5
    inner = (x > lo) & (x < hi) & (y > lo) & (y < hi)
    outside = (x < lo) | (x > hi) | (y < lo) | (y > hi)
    assert inner.sum() >= 100 or (H, W) == (16, 16)
    assert (count[inner] == 1).all(), name            # never 0 (a crack), never 2 (drawn twice)
    assert (count[outside] == 0).all() and (count <= 1).all()
    assert ((pix >= 0) == (count == 1)).all()
    if "latticeA" in name:                            # centres ON vertices and edges are among them
        assert inner[4, 4] and count[4, 4] == 1 and count[3, 4] == 1 and count[3, 3] == 1


@pytest.mark.parametrize("K", vc.STACK_K)
def test_duplicate_stack_goes_to_the_lowest_index(K):
    name = "dups%d-screen_w-48x64" % K
    pix = vc.model_case(name)[0]
    assert set(np.unique(pix).tolist()) == {-1, 1}    # face 0 is farther; 1 .. K are the same triangle
    pix = vc.model_case("stack%d-screen_w-48x64" % K)[0]
    assert (pix >= 0).sum() > 50


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_host_sim_equals_the_model_bit_for_bit(sim, name):
    v, f, M, H, W, body, hair = vc.case(name)
    want_pix, want_vis, seen, seen_head, head = vc.model_case(name)
    pix, visp, cnt, cnt_head, tiles = _sim_view(sim, v, f, M, H, W, body, hair)
    assert np.array_equal(pix, want_pix)
    assert np.array_equal(visp, want_vis)
    assert np.array_equal(cnt, seen.astype(np.int32)) and np.array_equal(cnt_head, seen_head.astype(np.int32))
    got_head = np.full((H, W), 7, np.uint8)
    sim.ghrsim_vis_head_mask(H, W, _p(body), _p(hair), _p(got_head))
    assert np.array_equal(got_head, head.astype(np.uint8))
    # without masks head holds nowhere; the counts are ADDED to
    pix2, vis2, cnt2, cnt_head2, _ = _sim_view(sim, v, f, M, H, W, None, None, cnt, cnt_head)
    assert np.array_equal(pix2, want_pix) and not vis2.any()
    assert np.array_equal(cnt2, 2 * seen.astype(np.int32)) and np.array_equal(cnt_head2, seen_head.astype(np.int32))
    if name.startswith(("stack", "dups")):
        K = int(name.split("-")[0].lstrip("stackdup"))
        assert tiles[1 * 4 + 1] == K + (1 if name.startswith("dups") else 0) and tiles.sum() == tiles[5]
    if name == "bad-camera-130x250":
        assert tiles.min() == 1                       # the face larger than the image is in the big list: every tile walks it


@pytest.mark.parametrize("kind", vc.MASK_KINDS)
def test_host_sim_head_mask_on_every_kind_and_size(sim, kind):
    for H, W in vc.SIZES:
        body, hair = vc.masks(kind, H, W)
        got = np.full((H, W), 7, np.uint8)
        sim.ghrsim_vis_head_mask(H, W, _p(body), _p(hair), _p(got))
        want = vc.model_head(body, hair)
        assert np.array_equal(got, want.astype(np.uint8)), (kind, H, W)
        t = vis.head_mask(torch.from_numpy(body), torch.from_numpy(hair), fused=False)
        assert np.array_equal(t.numpy(), want), (kind, H, W)
    if kind == "corners":                             # the window is clipped: a lit corner lights 3 x 3, the centre 5 x 5
        body, hair = vc.masks(kind, 48, 64)
        want = vc.model_head(body, hair)
        assert want[:3, :3].all() and not want[3, 0] and want[22:27, 30:35].all() and want.sum() == 9 * 3 + 25
    if kind == "threshold":
        body, hair = vc.masks(kind, 48, 64)
        assert vc.model_head(body, hair).any() and not vc.model_head(np.full_like(body, 127), hair).any()


def test_sanitized_stand_alone_program_runs_the_cases_clean(tmp_path):
    """ghr_visibility_selfcheck: the per-element functions and the table walk under AddressSanitizer and
    UndefinedBehaviorSanitizer, as a program of its own (exact-size buffers)."""
    san = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    if os.path.basename(hp.host_cxx()) == "g++":
        san += ["-static-libasan", "-static-libubsan"]
    exe = hp.compile_hostsim("ghr_visibility_selfcheck_san", "ghr_visibility_selfcheck.cpp", san, DEPS)
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as fh:
        for name in CASES:
            v, f, M, H, W, body, hair = vc.case(name)
            pix, visp, seen, seen_head, head = vc.model_case(name)
            fh.write(np.array([len(v), len(f), H, W, 1], np.int32).tobytes())
            fh.write(np.concatenate([M, [vc.NEAR]]).astype(np.float32).tobytes())
            for arr in (v, f, body, hair, pix, visp, seen.astype(np.uint8), seen_head.astype(np.uint8), head.astype(np.uint8)):
                fh.write(np.ascontiguousarray(arr).tobytes())
    res = subprocess.run([exe, path], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "%d cases ok" % len(CASES) in res.stdout and "runtime error" not in res.stderr, res.stdout + res.stderr


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_torch_comparator_equals_the_model_on_cpu_tensors(name):
    v, f, M, H, W, body, hair = vc.case(name)
    want_pix, want_vis, seen, seen_head, _ = vc.model_case(name)
    pix = vis.rasterize_mesh((v, f), M, H, W, fused=False)
    assert pix.dtype == torch.int32 and np.array_equal(pix.numpy(), want_pix)
    cnt, cnt_head, planes = vis.vertex_visibility((v, f), [(M, H, W), (M, H, W)], [(body, hair), None], fused=False)
    assert np.array_equal(planes[0].numpy(), want_vis) and not planes[1].any()
    assert np.array_equal(cnt.numpy(), 2 * seen.astype(np.int32)) and np.array_equal(cnt_head.numpy(), seen_head.astype(np.int32))


def test_torch_comparator_does_not_depend_on_its_chunks():
    v, f, M, H, W, _, _ = vc.case("torus-front-17x33")
    a = vis._rasterize_torch(torch.from_numpy(v.copy()), torch.from_numpy(f.copy()).long(), M, H, W, vc.NEAR, chunk_elems=7)
    assert np.array_equal(a.numpy(), vc.model_case("torus-front-17x33")[0])


def test_fused_forms_refuse_cpu():
    v, f, M, H, W, _, _ = vc.case("box-front-16x16")
    with pytest.raises(RuntimeError, match="no CPU path"):
        vis.rasterize_mesh((v, f), M, H, W, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        vis.vertex_visibility((v, f), [(M, H, W)], device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        vis.head_mask(torch.zeros(4, 4, dtype=torch.uint8), torch.zeros(4, 4, dtype=torch.uint8))


def test_visible_vertex_mask_on_hand_made_counts():
    #            never seen | seen once, bare | always seen, half hair | mostly hair | seen in 1 of 20 | exactly at both thresholds
    cnt = np.array([0, 1, 20, 20, 1, 2], np.int32)
    cnt_head = np.array([0, 1, 10, 9, 1, 1], np.int32)
    got = vis.visible_vertex_mask(torch.from_numpy(cnt), torch.from_numpy(cnt_head), 20)
    #  0 / 0 is NaN: false in the first term, 0 / 20 < 0.1 in the second;  1 / 20 < 0.1;  1 - 10 / 20 = 0.5 is not > 0.5;
    #  1 - 9 / 20 > 0.5;  2 / 20 = 0.1 is not < 0.1 in float32 and 1 - 1 / 2 is not > 0.5
    assert got.tolist() == [True, True, False, True, True, False]
    assert np.array_equal(got.numpy(), vc.model_vertex_mask(cnt, cnt_head, 20))
    assert vis.visible_vertex_mask(torch.from_numpy(cnt), torch.from_numpy(cnt_head), 20, prob_thr=0.4, n_views_thr=0.0).tolist() == \
        [False, False, True, True, False, True]


def _hand_scalp():
    """a 3 x 3 grid of scalp vertices (8 faces) somewhere inside a 12-vertex head"""
    scalp_idx = np.array([2, 3, 4, 6, 7, 8, 9, 10, 11])
    g = lambda r, c: 3 * r + c  # noqa: E731
    faces = []
    for r in range(2):
        for c in range(2):
            faces += [[g(r, c), g(r, c + 1), g(r + 1, c + 1)], [g(r, c), g(r + 1, c + 1), g(r + 1, c)]]
    head_v = np.arange(36, dtype=np.float32).reshape(12, 3) / 8
    return scalp_idx, np.asarray(faces), head_v


def test_cut_scalp_on_a_hand_checked_mesh():
    scalp_idx, faces, _ = _hand_scalp()
    mask = np.ones(12, bool)
    mask[4] = False                                    # scalp vertex 2 (the top right corner) goes
    kept, nf = bs.cut_scalp(mask, scalp_idx, faces)
    assert kept.tolist() == [0, 1, 3, 4, 5, 6, 7, 8]
    assert nf.tolist() == [[0, 1, 3], [0, 3, 2], [1, 4, 3], [2, 3, 6], [2, 6, 5], [3, 4, 7], [3, 7, 6]]   # face (1, 2, 5) went
    # a seam group takes the minimum of its members: vertex 8 follows vertex 2; a second group is applied after the first
    kept, nf = bs.cut_scalp(torch.from_numpy(mask), torch.from_numpy(scalp_idx), torch.from_numpy(faces), [[2, 8], [8, 6, 7]])
    assert kept.tolist() == [0, 1, 3, 4, 5]
    assert nf.tolist() == [[0, 1, 3], [0, 3, 2], [1, 4, 3]]
    kept, nf = bs.cut_scalp(np.zeros(12, bool), scalp_idx, faces)
    assert kept.shape == (0,) and nf.shape == (0, 3)


def test_scalp_uv_mask_and_write_scalp_data_round_trip(tmp_path):
    from PIL import Image
    scalp_idx, faces, head_v = _hand_scalp()
    kept, nf = bs.cut_scalp(np.ones(12, bool), scalp_idx, faces)
    # the UV map: the grid over [-0.5, 0.5] x [-0.75, 0.25]; pixel (r, c) of the script's image samples uv = 2 (r, c) / 255 - 1
    uv = np.array([[-0.5 + 0.5 * c, -0.75 + 0.5 * r] for r in range(3) for c in range(3)], np.float32)
    m = bs.scalp_uv_mask(uv, nf, fused=False)
    assert m.shape == (256, 256, 1) and m.dtype == np.uint8 and set(np.unique(m).tolist()) == {0, 255}
    r, c = np.mgrid[0:256, 0:256]
    u, w = 2 * r / 255.0 - 1, 2 * c / 255.0 - 1
    img = (u > -0.5) & (u < 0.5) & (w > -0.75) & (w < 0.25)          # the script's img[r, c], off the boundary
    edge = (np.abs(np.abs(u) - 0.5) < 1e-6) | (np.abs(w + 0.75) < 1e-6) | (np.abs(w - 0.25) < 1e-6)
    want = np.flip(img.T, axis=0)
    sure = ~np.flip(edge.T, axis=0)
    assert np.array_equal((m[:, :, 0] > 0)[sure], want[sure]) and want.sum() > 10000
    planes = {"cam_a": np.where(np.add.outer(np.arange(20), np.arange(30)) % 7 < 3, 255, 0).astype(np.uint8)}
    out = bs.write_scalp_data(str(tmp_path), head_v[scalp_idx], kept, nf, planes, m)
    assert sorted(os.listdir(out)) == ["cut_scalp_verts.pickle", "dif_mask.png", "scalp.obj", "vis"]
    v, f = read_obj(os.path.join(out, "scalp.obj"))
    assert np.allclose(v, head_v[scalp_idx][kept], atol=1e-6) and np.array_equal(f, nf)
    with open(os.path.join(out, "cut_scalp_verts.pickle"), "rb") as fh:
        assert [int(i) for i in pickle.load(fh)] == kept.tolist()
    assert np.array_equal(np.asarray(Image.open(os.path.join(out, "dif_mask.png"))), m[:, :, 0])
    jpg = np.asarray(Image.open(os.path.join(out, "vis", "cam_a.jpg")))
    assert jpg.shape == (20, 30) and np.abs(jpg.astype(int) - planes["cam_a"]).mean() < 40


def test_seam_pairs_file_is_read(tmp_path):
    p = tmp_path / "seams.json"
    p.write_text('{"groups": [[2, 8], [8, 6, 7]]}')
    assert bs.load_seam_pairs(str(p)) == [[2, 8], [8, 6, 7]]


def test_views_from_projections_reproduces_a_known_camera():
    K = np.array([[1.9, 0.01, 1.02], [0.0, 2.1, 0.97], [0.0, 0.0, 1.0]])      # in units of half the image, as the script's pickle
    R, t = vc._look_at((0.4, -0.3, 2.5), (0.0, 0.1, 0.0))
    for scale in (1.0, -3.5):                                              # a projection is defined up to a factor
        P = scale * K @ np.concatenate([R, t[:, None]], 1)
        K2, R2, t2 = vis.decompose_projection(P)
        assert np.allclose(K2, K, atol=1e-12) and np.allclose(R2, R, atol=1e-12) and np.allclose(t2, t, atol=1e-12)
    P4 = np.eye(4)
    P4[:3] = K @ np.concatenate([R, t[:, None]], 1)
    views = vis.views_from_projections({"a": torch.from_numpy(P4)}, {"a": (48, 64)})
    M, H, W = views["a"]
    assert (H, W) == (48, 64) and M.dtype == np.float32 and M.shape == (12,)
    Kp = np.array([[64 * 1.9 / 2, 64 * 0.01, 64 * (1.02 / 2 + 0.5)], [0, 48 * 2.1 / 2, 48 * (0.97 / 2 + 0.5)], [0, 0, 1]])
    assert np.allclose(M.reshape(3, 4), Kp @ np.concatenate([R, t[:, None]], 1), rtol=1e-6, atol=1e-6)
    with pytest.raises(ValueError, match="not finite"):
        vis.decompose_projection(np.full((3, 4), np.nan))
    with pytest.raises(ValueError, match="does not reproduce"):
        vis.decompose_projection(np.concatenate([np.zeros((3, 3)), np.ones((3, 1))], 1))


def test_view_matrix_from_camera_puts_pixel_centres_at_half():
    from gaussianhaircut_amd.utils import synthetic as syn
    cam = syn.make_view(syn.CONFIGS["tiny"], torch.device("cpu"))
    M, H, W = vis.view_matrix_from_camera(cam)
    assert (H, W) == (cam.image_height, cam.image_width)
    X = np.array([0.2, -0.1, 0.3, 1.0])
    p_view = X @ cam.world_view_transform.double().numpy()                  # the renderer's row-vector convention
    ndc = p_view[0] / (p_view[2] * np.tan(float(cam.FoVx) / 2)), p_view[1] / (p_view[2] * np.tan(float(cam.FoVy) / 2))
    pix = ((ndc[0] + 1) * W - 1) / 2, ((ndc[1] + 1) * H - 1) / 2           # ndc2pix: pixel k at the integer k
    xyw = M.reshape(3, 4).astype(np.float64) @ X
    assert np.allclose([xyw[0] / xyw[2] - 0.5, xyw[1] / xyw[2] - 0.5], pix, atol=1e-3) and np.isclose(xyw[2], p_view[2], atol=1e-5)


def test_c_abi_refusals_launch_nothing():
    L = _lib.lib()
    b = ctypes.c_size_t(0)
    assert L.ghr_vis_sizes(10, 20, 48, 64, ctypes.byref(b)) == _lib.GHR_OK and b.value > 0 and b.value % 16 == 0
    small = b.value
    assert L.ghr_vis_sizes(0, 0, 0, 0, ctypes.byref(b)) == _lib.GHR_OK and 0 < b.value < small
    assert L.ghr_vis_sizes(10, 20, 48, 64, None) == _lib.GHR_E_INVALID
    for bad in ((-1, 1, 1, 1), (1, -1, 1, 1), (1, 1, -1, 1), (1, 1, 1, -1)):
        assert L.ghr_vis_sizes(*bad, ctypes.byref(b)) == _lib.GHR_E_INVALID
        assert b"negative" in L.ghr_last_error()
    assert L.ghr_vis_sizes(1, 1, 65536, 65536, ctypes.byref(b)) == _lib.GHR_E_INVALID
    assert b"H * W" in L.ghr_last_error()
    assert L.ghr_vis_sizes(1, 2 ** 30, 1024, 1024, ctypes.byref(b)) == _lib.GHR_E_INVALID
    assert b"tile lists" in L.ghr_last_error()
    fake = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before anything is enqueued
    M = (ctypes.c_float * 12)(*([1.0] * 12))
    ok = dict(V=8, vertices=fake, F=12, faces=fake, M=ctypes.byref(M), near=1e-3, H=48, W=64, body=fake, hair=fake, ws=fake,
              pix=fake, vis=fake, cnt=fake, cnt_head=fake)

    def call(**kw):
        a = dict(ok, **kw)
        return L.ghr_vis_view(None, a["V"], a["vertices"], a["F"], a["faces"], a["M"], a["near"], a["H"], a["W"], a["body"],
                              a["hair"], a["ws"], a["pix"], a["vis"], a["cnt"], a["cnt_head"])
    for kw, why in ((dict(V=-1), b"negative"), (dict(F=-1), b"negative"), (dict(H=-1), b"negative"), (dict(vertices=None), b"vertices"),
                    (dict(faces=None), b"faces"), (dict(M=None), b"M is NULL"), (dict(near=float("nan")), b"near"),
                    (dict(body=None), b"together"), (dict(hair=None), b"together"), (dict(ws=None), b"workspace is NULL"),
                    (dict(ws=ctypes.c_void_p(4104)), b"16-B aligned"), (dict(pix=None), b"pix_to_face"),
                    (dict(cnt=None), b"together"), (dict(H=65536, W=65536), b"H * W")):
        assert call(**kw) == _lib.GHR_E_INVALID, kw
        assert why in L.ghr_last_error(), (kw, L.ghr_last_error())
    assert L.ghr_vis_head_mask(None, 48, 64, None, fake, fake) == _lib.GHR_E_INVALID
    assert L.ghr_vis_head_mask(None, 48, 64, fake, fake, None) == _lib.GHR_E_INVALID
    assert L.ghr_vis_head_mask(None, -1, 64, fake, fake, fake) == _lib.GHR_E_INVALID
    assert L.ghr_vis_head_mask(None, 0, 64, None, None, None) == _lib.GHR_OK


def test_scalp_tool_writes_the_four_products_from_a_synthetic_scene(tmp_path):
    """tools/between_stages.py scalp --composed on a small scene in the reference's layout: an icosphere head, six cameras in the
    reference's pickle format, mask PNGs; its products against the library calls made by hand."""
    import importlib.util
    from PIL import Image
    from tests import mesh_cases as mc
    spec = importlib.util.spec_from_file_location("between_stages_tool", os.path.join(hp.ROOT, "tools", "between_stages.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    v, f = mc.icosphere(2)
    H, W = 48, 64
    data, flame = tmp_path / "data", tmp_path / "flame"
    for kind in ("body", "hair"):
        os.makedirs(data / "masks_2" / kind)
    with open(tmp_path / "head.obj", "w") as fh:
        fh.write("".join("v %.9g %.9g %.9g\n" % tuple(p) for p in v) + "".join("f %d %d %d\n" % tuple(t + 1) for t in f))
    cams, views, masks = {}, [], []
    for k in range(6):
        a = 2 * np.pi * k / 6
        R, t = vc._look_at((3 * np.sin(a), 0.4, 3 * np.cos(a)), (0.0, 0.0, 0.0))
        Kh = np.array([[2.4 * H / W, 0, 0.02], [0, 2.4, -0.01], [0, 0, 1.0]])     # in units of half the image, centres at the integers
        P = np.eye(4)
        P[:3] = Kh @ np.concatenate([R, t[:, None]], 1)
        cams["v%02d" % k] = torch.from_numpy(P.T.copy())                          # stored transposed, as the reference's pickle
        Kp = np.array([[W * Kh[0, 0] / 2, 0, W * (Kh[0, 2] / 2 + 0.5)], [0, H * Kh[1, 1] / 2, H * (Kh[1, 2] / 2 + 0.5)], [0, 0, 1]])
        views.append((vis.view_matrix(Kp, R, t), H, W))
        body, hair = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
        body[4:44, 12:52] = 255
        hair[4:20 + 2 * k, 12:52] = 255
        masks.append((body, hair))
        Image.fromarray(body).save(data / "masks_2" / "body" / ("v%02d.png" % k))
        Image.fromarray(hair).save(data / "masks_2" / "hair" / ("v%02d.png" % k))
    with open(tmp_path / "cams.pkl", "wb") as fh:
        pickle.dump(cams, fh)
    scalp_idx = np.nonzero(v[:, 1] < 0.2)[0]                                      # (image y points down: the top of the head)
    local = np.full(len(v), -1)
    local[scalp_idx] = np.arange(len(scalp_idx))
    sf = local[f[(local[f] >= 0).all(1)]]
    uv = (v[scalp_idx][:, [0, 2]] * 0.9).astype(np.float32)
    np.save(tmp_path / "idx.npy", scalp_idx); np.save(tmp_path / "faces.npy", sf); np.save(tmp_path / "uv.npy", uv)
    (tmp_path / "seams.json").write_text('{"groups": [[0, 1], [2, 3, 4]]}')
    tool.main(["scalp", "--composed", "--mesh", str(tmp_path / "head.obj"), "--cams", str(tmp_path / "cams.pkl"), "--path_to_data", str(data),
               "--out_dir", str(flame), "--scalp_idx", str(tmp_path / "idx.npy"), "--scalp_faces", str(tmp_path / "faces.npy"),
               "--scalp_uvs", str(tmp_path / "uv.npy"), "--seam_pairs", str(tmp_path / "seams.json")])
    out = flame / "scalp_data"
    assert sorted(os.listdir(out)) == ["cut_scalp_verts.pickle", "dif_mask.png", "scalp.obj", "vis"]
    assert sorted(os.listdir(out / "vis")) == ["v%02d.jpg" % k for k in range(6)]
    # by hand, from the views the pickle was made of (the tool's matrices come back from the decomposition: equal to rounding,
    # and no vertex of this scene sits on a threshold)
    cnt, cnt_head = np.zeros(len(v), np.int32), np.zeros(len(v), np.int32)
    for (M, _, _), (body, hair) in zip(views, masks):
        _, _, seen, seen_head, _ = vc.model_view(v, f, M, H, W, body, hair)
        cnt += seen
        cnt_head += seen_head
    kept, nf = bs.cut_scalp(vc.model_vertex_mask(cnt, cnt_head, 6), scalp_idx, sf, [[0, 1], [2, 3, 4]])
    assert 0 < len(kept) < len(scalp_idx)
    with open(out / "cut_scalp_verts.pickle", "rb") as fh:
        assert [int(i) for i in pickle.load(fh)] == kept.tolist()
    ov, of = read_obj(str(out / "scalp.obj"))
    assert np.array_equal(of, nf) and np.allclose(ov, v[scalp_idx][kept], atol=1e-6)
    dif = np.asarray(Image.open(out / "dif_mask.png"))
    assert np.array_equal(dif, bs.scalp_uv_mask(uv[kept], nf, fused=False)[:, :, 0]) and 0 < (dif > 0).mean() < 1
