"""The strand stage's prior term (gaussianhaircut_amd/strand_prior.py, csrc/ghr_sds.h) without a GPU.

 1. tests/golden/reference_sds_golden.npz is the REFERENCE'S OWN initialize_gaussians_hair (use_sds) on seeded inputs.  The
    float64 restatement of tests/sds_cases.py is the arbiter: its float32 run and the composed form (fused=False) on CPU tensors
    equal the golden's texture and d_dirs within 1e-5 max|f64| + 3 |golden - f64|, and the conditions on the inputs hold (every
    relative gap among a texel's five smallest distances >= 1e-5, no csim within 1e-4 of 0.9, >= 10 % of them on each side).
 2. the product's GHR_HD functions and host walks of the kernels' loops (tests/hostsim/ghr_hostsim_sds.cpp) on the golden and
    on the small shapes: neighbour indices and inverted lists bit for bit against the restatement's stable sort, every float
    within 1e-5 max|f64| + 3 |float32 restatement - f64|; the same walks in a stand-alone program built with
    -fsanitize=address,undefined (nothing sanitized is loaded here).
 3. the C ABI: the four symbols, declared and exported, every refusal answered before the runtime is touched, ABI 20.
 4. the model and the trainer on CPU tensors: nothing changes without a prior; with one, loss == base + lambda_dsds Lsds and
    _dirs.grad gains exactly the prior's gradient."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd import strand_prior as sp
from tests import helpers as hp
from tests import sds_cases as sc

SMALL, case = sc.SMALL, sc.case


@pytest.fixture(scope="module")
def golden():
    return sc.golden_case()


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
def test_conditions_on_the_golden_inputs(golden):
    gap, knee, above = sc.input_conditions(golden["r64"], golden["N"])
    print("smallest relative gap %.3e, nearest csim to 0.9 at %.3e, %.1f %% above 0.9" % (gap, knee, 100 * above))
    assert gap >= 1e-5 and knee >= 1e-4 and 0.1 <= above <= 0.9
    assert len(set(golden["idx"].tolist())) == golden["N"]           # no strand twice: the reference's unstable sort decided nothing


def _against_golden(name, tex, d_dirs, loss, golden):
    r64, want, idx = golden["r64"], golden["want"], golden["idx"]
    sc.assert_within(name + " texture", tex, r64["texture"], want["texture"])
    sc.assert_within(name + " d_dirs", d_dirs, r64["d_dirs"], want["d_dirs"])          # every element of all S rows
    mask = torch.ones(golden["S"], dtype=torch.bool)
    mask[idx] = False
    assert float(d_dirs[mask].abs().max()) == 0.0                      # strands that were not drawn get nothing
    assert abs(float(loss) - float(want["loss"])) <= 1e-5 * abs(float(r64["loss"])) + 3 * abs(float(want["loss"]) - float(r64["loss"]))


def test_float32_restatement_equals_the_reference_golden(golden):
    r32 = golden["r32"]
    assert torch.equal(r32["nbr"], golden["r64"]["nbr"])
    _against_golden("restatement", r32["texture"], r32["d_dirs"], r32["loss"], golden)


def test_composed_form_on_cpu_tensors_equals_the_reference_golden(golden):
    T0 = golden["T0"]
    prior = sp.StrandPrior(sc.make_encoder(golden["W"]), lambda t: ((t - T0) ** 2).mean(dim=(1, 2, 3)), golden["uvs"],
                           golden["local2world"], golden["G"], golden["scale"], fused=False)
    dirs = golden["dirs"].clone().requires_grad_(True)
    loss = prior(dirs, idx=golden["idx"])
    loss.backward()
    nbr, _ = sp.neighbours_composed(golden["uvs"][golden["idx"]], golden["G"])
    assert torch.equal(nbr, golden["r64"]["nbr"])
    _against_golden("composed", prior.last_texture, dirs.grad, loss.detach(), golden)
    assert prior.last_idx is golden["idx"] and prior.last_texture.shape == (1, 64, 32, 32)


@pytest.mark.parametrize("name", sorted(SMALL))
def test_composed_form_on_the_small_shapes(name):
    c = case(name)
    r64, r32 = c["r64"], c["r32"]
    if c["S"] > 1:
        gap, knee, _ = sc.input_conditions(r64, c["N"], exact_ties=True)   # (idx is drawn with replacement here)
        assert gap >= 1e-5 and knee >= 1e-4, (gap, knee)
    T0 = c["T0"]
    prior = sp.StrandPrior(sc.make_encoder(c["W"]), lambda t: ((t - T0) ** 2).mean(dim=(1, 2, 3)), c["uvs"], c["local2world"], c["G"],
                           c["scale"], num_guiding=c["N"], channels=c["C"], fused=False)
    dirs = c["dirs"].clone().requires_grad_(True)
    prior(dirs, idx=c["idx"]).backward()
    nbr, _ = sp.neighbours_composed(c["uvs"][c["idx"]], c["G"])
    assert torch.equal(nbr, r64["nbr"])
    start, entries = sp.inverted_lists(nbr, c["N"])
    assert torch.equal(start.long(), r64["start"]) and torch.equal(entries.long(), r64["entries"])
    sc.assert_within("texture", prior.last_texture, r64["texture"], r32["texture"])
    sc.assert_within("d_dirs", dirs.grad, r64["d_dirs"], r32["d_dirs"])
    if name == "one-strand":
        assert torch.equal(nbr, torch.arange(4).expand(9, 4))          # the tie rule is all there is


def test_draw_and_size_refusals():
    uvs, l2w = torch.zeros(5, 2), torch.eye(3).expand(5, 3, 3)
    enc, loss = (lambda e: e.flatten(1)), (lambda t: t)
    with pytest.raises(ValueError, match="G \\* G"):
        sp.StrandPrior(enc, loss, uvs, l2w, 2, 1.0, num_guiding=5)
    with pytest.raises(ValueError, match="needs 4"):
        sp.StrandPrior(enc, loss, uvs, l2w, 2, 1.0, num_guiding=3)
    with pytest.raises(ValueError, match="G \\* G"):
        sp.latent_texture(torch.zeros(5, 2), torch.zeros(5, 3), torch.zeros(5, 2, 3), 2, fused=False)
    with pytest.raises(ValueError, match="needs 4"):
        sp.latent_texture(torch.zeros(3, 2), torch.zeros(3, 3), torch.zeros(3, 2, 3), 2, fused=False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sp.latent_texture(torch.zeros(4, 2), torch.zeros(4, 3), torch.zeros(4, 2, 3), 2, fused=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sp.guiding_strands_local(torch.zeros(5, 2, 3), l2w, torch.zeros(4, dtype=torch.int64), 1.0, fused=True)
    g = torch.Generator().manual_seed(3)
    p = sp.StrandPrior(enc, loss, uvs, l2w, 3, 1.0, num_guiding=8, channels=2, generator=g, fused=False)
    a = p.draw(5, "cpu")
    assert a.shape == (8,) and a.dtype == torch.int64 and int(a.min()) >= 0 and int(a.max()) < 5
    assert torch.equal(a, torch.randint(0, 5, (8,), generator=torch.Generator().manual_seed(3)))
    m = torch.randn(4, 3, 3, dtype=torch.float64) + 2 * torch.eye(3, dtype=torch.float64)
    assert torch.allclose(sp.inverse3(m), torch.linalg.inv(m), rtol=1e-10, atol=1e-12)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
DEPS = ["ghr_hostsim_sds.cpp", "ghr_hostsim_haar.h", "ghr_sds.h", "ghr_haar.h"]


@pytest.fixture(scope="module")
def sim():
    L = ctypes.CDLL(hp.compile_hostsim("libghr_hostsim_sds.so", "ghr_hostsim_sds.cpp", ["-O2", "-fPIC", "-shared"], DEPS))
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.ghrsim_sds_local.argtypes = [i32, i32, i32, vp, vp, i32, vp, f32, vp, vp]
    L.ghrsim_sds_local_backward.argtypes = [i32, i32, i32, vp, i32, vp, vp, f32, vp, vp, vp]
    L.ghrsim_sds_texture.argtypes = [i32] * 4 + [vp] * 13
    L.ghrsim_sds_texture_backward.argtypes = [i32] * 4 + [vp] * 13
    L.ghrsim_sds_top4.argtypes = [i32, vp, vp, vp, vp]
    L.ghrsim_sds_inv3.argtypes = [vp, vp]
    L.ghrsim_sds_alpha.argtypes = L.ghrsim_sds_alpha_dc.argtypes = [f32]
    L.ghrsim_sds_alpha.restype = L.ghrsim_sds_alpha_dc.restype = f32
    assert L.ghrsim_sds_wave() == 64
    return L


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _np(t, dtype=np.float32):
    return np.ascontiguousarray(t.detach().cpu().numpy().astype(dtype))


def _sim_block(sim, c, inverse=True):
    """steps 1 - 4 and their backward through the host walks; the encoder and the loss in PyTorch float32"""
    S, N, n, C, G = c["S"], c["N"], c["n"], c["C"], c["G"]
    GG = G * G
    frames = _np(torch.linalg.inv(c["local2world"].double()).float() if inverse else c["local2world"])
    dirs, idx = _np(c["dirs"]), _np(c["idx"], np.int64)
    e, v = np.full((N, n + 1, 3), np.nan, np.float32), np.full((N, n, 3), np.nan, np.float32)
    sim.ghrsim_sds_local(S, N, n, _p(dirs), _p(frames), int(inverse), _p(idx), c["scale"], _p(e), _p(v))
    et = torch.from_numpy(e).requires_grad_(True)
    z = sc.make_encoder(c["W"])(et)[:, :C]
    uvg = _np(c["uvs"][c["idx"]])
    centres = _np(sp.texel_centres(G, "cpu"))
    zn = _np(z)
    st = dict(nbr=np.full((GG, 4), -1, np.int32), w=np.full((GG, 4), np.nan, np.float32), csim=np.full(N, np.nan, np.float32),
              alpha=np.full(N, np.nan, np.float32), alpha_q=np.full(GG, np.nan, np.float32), count=np.full(N, -1, np.int32),
              start=np.full(N + 1, -1, np.int32), list=np.full(4 * GG, -1, np.int32))
    tex = np.full((1, C, G, G), np.nan, np.float32)
    sim.ghrsim_sds_texture(N, n, C, G, _p(uvg), _p(centres), _p(zn), _p(v), *[_p(st[k]) for k in ("nbr", "w", "csim", "alpha", "alpha_q",
                                                                                                   "count", "start", "list")], _p(tex))
    d_tex = _np(2 * (torch.from_numpy(tex) - c["T0"]) / tex.size)
    scratch_a, scratch_c = np.full(GG, np.nan, np.float32), np.full(N, np.nan, np.float32)
    d_z, d_v = np.full((N, C), np.nan, np.float32), np.full((N, n, 3), np.nan, np.float32)
    sim.ghrsim_sds_texture_backward(N, n, C, G, _p(zn), _p(v), *[_p(st[k]) for k in ("nbr", "w", "csim", "alpha_q", "start", "list")],
                                    _p(d_tex), _p(scratch_a), _p(scratch_c), _p(d_z), _p(d_v))
    (d_e,) = torch.autograd.grad(z, et, torch.from_numpy(d_z))
    sidx, order = torch.sort(c["idx"], stable=True)
    d_dirs = np.zeros((S, n, 3), np.float32)
    sidx_n, order_n, d_e_n = _np(sidx, np.int64), _np(order, np.int64), _np(d_e)  # (named: they must outlive the call)
    sim.ghrsim_sds_local_backward(S, N, n, _p(frames), int(inverse), _p(sidx_n), _p(order_n), c["scale"], _p(d_e_n), _p(d_v), _p(d_dirs))
    T = torch.from_numpy
    return dict(e=T(e), v=T(v), texture=T(tex), d_dirs=T(d_dirs), d_z=T(d_z), d_v=T(d_v), d_e=d_e, d_tex=T(d_tex), z=T(zn), uvg=T(uvg),
                centres=T(centres), frames=T(frames), sidx=sidx, order=order, **{k: T(a) for k, a in st.items()})


def _check_sim(got, c):
    r64, r32 = c["r64"], c["r32"]
    GG = c["G"] ** 2
    assert torch.equal(got["nbr"].long(), r64["nbr"])
    assert torch.equal(got["start"].long(), r64["start"]) and torch.equal(got["list"].long(), r64["entries"])
    assert torch.equal(got["count"].long(), r64["start"][1:] - r64["start"][:-1]) and int(got["start"][-1]) == 4 * GG
    for k in ("e", "v", "w", "csim", "alpha", "alpha_q", "texture", "d_dirs"):
        sc.assert_within(k, got[k], r64[k], r32[k])


def test_host_walks_on_the_golden(sim, golden):
    got = _sim_block(sim, golden)
    _check_sim(got, golden)
    _against_golden("host walk", got["texture"], got["d_dirs"], ((got["texture"] - golden["T0"]) ** 2).mean(), golden)


@pytest.mark.parametrize("name", sorted(SMALL))
def test_host_walks_on_the_small_shapes(sim, name):
    c = case(name)
    _check_sim(_sim_block(sim, c), c)
    if name in ("duplicates", "G3-N9"):                                 # the in-kernel adjugate inverse of the frame
        got = _sim_block(sim, c, inverse=False)
        sc.assert_within("e (frames inverted per strand)", got["e"], c["r64"]["e"], c["r32"]["e"])
        sc.assert_within("d_dirs (frames inverted per strand)", got["d_dirs"], c["r64"]["d_dirs"], c["r32"]["d_dirs"])


def test_per_element_functions(sim):
    # the insertion: ties go to the lower index whatever the order of arrival; NaN distances still leave four real indices
    d = np.array([0.5, 0.25, 0.5, 0.25, 0.25, 1.0, 0.25], np.float32)
    for perm in (np.arange(7), np.arange(7)[::-1], np.array([3, 6, 0, 5, 1, 2, 4])):
        od, og = np.zeros(4, np.float32), np.zeros(4, np.int32)
        dp, gp = np.ascontiguousarray(d[perm]), np.ascontiguousarray(perm.astype(np.int32))
        sim.ghrsim_sds_top4(7, _p(dp), _p(gp), _p(od), _p(og))
        assert og.tolist() == [1, 3, 4, 6] and od.tolist() == [0.25] * 4
    nan = np.full(6, np.nan, np.float32)
    six = np.arange(6, dtype=np.int32)
    sim.ghrsim_sds_top4(6, _p(nan), _p(six), _p(od), _p(og))
    assert og.tolist() == [0, 1, 2, 3]
    m = (np.random.default_rng(1).standard_normal((3, 3)) + 2 * np.eye(3)).astype(np.float32)
    o = np.zeros((3, 3), np.float32)
    sim.ghrsim_sds_inv3(_p(m), _p(o))
    assert np.allclose(o, np.linalg.inv(m.astype(np.float64)), rtol=1e-5, atol=1e-6)
    assert np.array_equal(o, sp.inverse3(torch.from_numpy(m)).numpy())   # the composed form has the same expressions
    for cs in (-0.5, 0.0, 0.3, 0.9, np.nextafter(np.float32(0.9), np.float32(1)), 0.95, 1.0):
        c64 = float(np.float32(cs))
        want = 1 - 1.63 * c64 ** 5 if np.float32(cs) <= np.float32(0.9) else 0.4 - 0.4 * c64
        dwant = -8.15 * c64 ** 4 if np.float32(cs) <= np.float32(0.9) else -0.4
        assert abs(sim.ghrsim_sds_alpha(cs) - want) < 1e-6 and abs(sim.ghrsim_sds_alpha_dc(cs) - dwant) < 1e-5


def test_sanitized_stand_alone_program_runs_the_walks_clean(sim, tmp_path):
    """ghr_sds_selfcheck: the per-element functions and the walks under AddressSanitizer and UndefinedBehaviorSanitizer, as a
    program of its own (exact-size buffers)."""
    san = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    if os.path.basename(hp.host_cxx()) == "g++":
        san += ["-static-libasan", "-static-libubsan"]
    exe = hp.compile_hostsim("ghr_sds_selfcheck_san", "ghr_sds_selfcheck.cpp", san, DEPS)
    path = str(tmp_path / "cases.bin")
    names = sorted(SMALL)
    with open(path, "wb") as fh:
        for name in names:
            c = case(name)
            got = _sim_block(sim, c)
            tol = 1e-5 * max(float(c["r64"]["texture"].abs().max()), float(c["r64"]["e"].abs().max()))
            fh.write(np.array([c["S"], c["N"], c["n"], c["C"], c["G"], 1], np.int32).tobytes())
            fh.write(np.array([c["scale"], tol], np.float32).tobytes())
            for arr, dt in ((c["dirs"], np.float32), (got["frames"], np.float32), (c["idx"], np.int64), (got["sidx"], np.int64),
                            (got["order"], np.int64), (got["uvg"], np.float32), (got["centres"], np.float32), (got["z"], np.float32),
                            (got["d_tex"], np.float32), (got["d_e"], np.float32), (c["r64"]["nbr"], np.int32), (c["r64"]["start"], np.int32),
                            (c["r64"]["entries"], np.int32), (got["texture"], np.float32), (got["e"], np.float32)):
                fh.write(_np(arr, dt).tobytes())
    res = subprocess.run([exe, path], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "%d cases ok" % len(names) in res.stdout and "runtime error" not in res.stderr, res.stdout + res.stderr


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
NAMES = ("ghr_sds_local", "ghr_sds_local_backward", "ghr_sds_texture", "ghr_sds_texture_backward")


def test_c_abi_symbols_are_declared_and_exported():
    L = _lib.lib()
    with open(os.path.join(hp.ROOT, "include", "ghr.h")) as fh:
        hdr = fh.read()
    for n in NAMES:
        assert re.search(r"\bint %s\(" % n, hdr) and n in _lib.EXPORTS and hasattr(L, n), n
    assert L.ghr_abi_version() == 20 == _lib.ABI_VERSION and "#define GHR_ABI_VERSION 20" in hdr
    assert "ghr_sds.h" in _lib.HEADERS


def test_c_abi_refusals_launch_nothing():
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before anything is enqueued
    INV = _lib.GHR_E_INVALID

    def local(S=9, N=5, n=3, dirs=fake, frames=fake, idx=fake, e=fake, v=fake):
        return L.ghr_sds_local(None, S, N, n, dirs, frames, 0, idx, 1.0, e, v)

    def local_b(S=9, N=5, n=3, frames=fake, sidx=fake, order=fake, d_e=fake, d_v=fake, d_dirs=fake):
        return L.ghr_sds_local_backward(None, S, N, n, frames, 0, sidx, order, 1.0, d_e, d_v, d_dirs)

    def tex(N=5, n=3, C=2, G=3, **kw):
        a = dict(dict.fromkeys(("uvg", "centres", "z", "v", "nbr", "w", "csim", "alpha", "alpha_q", "count", "start", "list", "texture"), fake), **kw)
        return L.ghr_sds_texture(None, N, n, C, G, *[a[k] for k in ("uvg", "centres", "z", "v", "nbr", "w", "csim", "alpha", "alpha_q",
                                                                     "count", "start", "list", "texture")])

    def tex_b(N=5, n=3, C=2, G=3, **kw):
        names = ("z", "v", "nbr", "w", "csim", "alpha_q", "start", "list", "d_texture", "dalpha_q", "d_csim", "d_z", "d_v")
        a = dict(dict.fromkeys(names, fake), **kw)
        return L.ghr_sds_texture_backward(None, N, n, C, G, *[a[k] for k in names])

    for fn, cases in ((local, [(dict(N=3), b"N < 4"), (dict(n=0), b"n < 1"), (dict(S=0), b"S < 1"), (dict(S=-1), b"negative"),
                               (dict(dirs=None), b"NULL"), (dict(frames=None), b"NULL"), (dict(idx=None), b"NULL"), (dict(e=None), b"e or v"),
                               (dict(v=None), b"e or v"), (dict(N=2 ** 25), b"32-bit")]),
                      (local_b, [(dict(N=3), b"N < 4"), (dict(n=0), b"n < 1"), (dict(S=0), b"S < 1"), (dict(frames=None), b"NULL"),
                                 (dict(sidx=None), b"NULL"), (dict(order=None), b"NULL"), (dict(d_dirs=None), b"d_dirs")]),
                      (tex, [(dict(N=3), b"N < 4"), (dict(n=0), b"n < 1"), (dict(C=0), b"C < 1"), (dict(G=2), b"G * G < N"),
                             (dict(G=-3), b"negative"), (dict(N=10, G=3), b"G * G < N"), (dict(uvg=None), b"NULL"), (dict(centres=None), b"NULL"),
                             (dict(z=None), b"NULL"), (dict(v=None), b"NULL"), (dict(nbr=None), b"saved-state"), (dict(count=None), b"saved-state"),
                             (dict(list=None), b"saved-state"), (dict(texture=None), b"texture is NULL"), (dict(G=20000), b"32-bit")]),
                      (tex_b, [(dict(N=3), b"N < 4"), (dict(n=0), b"n < 1"), (dict(C=0), b"C < 1"), (dict(G=2), b"G * G < N"),
                               (dict(z=None), b"NULL"), (dict(start=None), b"saved-state"), (dict(d_texture=None), b"d_texture"),
                               (dict(dalpha_q=None), b"dalpha_q"), (dict(d_csim=None), b"dalpha_q"), (dict(d_z=None), b"d_z")])):
        for kw, why in cases:
            assert fn(**kw) == INV, (fn.__name__, kw)
            assert why in L.ghr_last_error(), (fn.__name__, kw, L.ghr_last_error())
    assert local_b(d_e=None, d_v=None) == _lib.GHR_OK                    # nothing arrives: nothing is launched


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def _scene_with_ground_truth():
    from gaussianhaircut_amd.gaussian_renderer import render_hair
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    from gaussianhaircut_amd.trainer import PIPE
    from gaussianhaircut_amd.utils import synthetic as syn
    from tests.test_api_cpu import _hair_scene
    opt = OptimizationParams()
    opt.lambda_dorient, opt.lambda_dmask, opt.lambda_dsds = 0.1, 0.1, 0.01   # run.sh
    spec, head, hair, cam = _hair_scene()
    _, _, gt_hair, _ = _hair_scene()
    from tests.oracle_backend import oracle_rasterizer
    with torch.no_grad(), oracle_rasterizer():
        gt_hair._dirs.mul_(1.1)
        gt_hair.initialize_gaussians_hair()
        pkg = render_hair(cam, head, gt_hair, PIPE, syn.background())
        cam.original_image, cam.original_mask = pkg["render"].clamp(0, 1).detach(), pkg["mask"].clamp(0, 1).detach()
        cam.original_orient_angle = pkg["orient_angle"].detach()
        cam.original_orient_conf = torch.ones_like(pkg["orient_conf"]).detach()
    hair.training_setup(opt, fused=False)
    return opt, head, hair, cam


def _tiny_prior(hair, seed=11):
    return sc.tiny_prior(hair._dirs.shape[0], hair._dirs.shape[1], seed=seed, fused=False)


def _one_step(hair, head, cam, opt, cams=None):
    """one strand_training_step; returns (loss, _dirs.grad as the optimizer saw it, the kwargs of every rebuild)"""
    from gaussianhaircut_amd.trainer import PIPE, strand_training_step
    from gaussianhaircut_amd.utils import synthetic as syn
    from tests.oracle_backend import oracle_rasterizer
    seen, calls = {}, []
    step0, init0 = hair.optimizer.step, hair.initialize_gaussians_hair
    hair.optimizer.step = lambda *a, **k: (seen.update(g=hair._dirs.grad.detach().clone()), step0(*a, **k))[1]
    hair.initialize_gaussians_hair = lambda *a, **k: (calls.append((a, k)), init0(*a, **k))[1]
    try:
        with oracle_rasterizer():
            loss = strand_training_step(head, hair, cams or [cam], syn.background(), opt, 1, pipe=PIPE)
    finally:
        hair.optimizer.step = step0
        del hair.initialize_gaussians_hair
    return loss.detach().clone(), seen["g"], calls


def test_without_a_prior_the_step_is_the_one_it_was():
    import copy
    opt, head, hair, cam = _scene_with_ground_truth()
    assert hair.use_sds is False and hair.prior is None and hair.Lsds is None
    loss, grad, calls = _one_step(hair, head, cam, opt, cams=[cam, copy.copy(cam)])
    assert calls == [((), {}), ((), {})] and hair.Lsds is None           # the rebuilds are called as they always were
    assert loss.dim() == 0 and bool(torch.isfinite(loss)) and float(grad.abs().max()) > 0


def test_with_a_prior_the_loss_and_the_gradient_gain_exactly_its_term():
    import copy
    opt, head, hair, cam = _scene_with_ground_truth()
    base_loss, base_grad, _ = _one_step(hair, head, cam, opt)
    opt, head, hair, cam = _scene_with_ground_truth()                      # the same scene again, untouched by the step above
    hair.attach_prior(_tiny_prior(hair))
    assert hair.use_sds is True
    dirs0 = hair._dirs.detach().clone()
    loss, grad, calls = _one_step(hair, head, cam, opt)
    assert calls == [((), {})]
    idx = hair.prior.last_idx
    d = dirs0.clone().requires_grad_(True)
    Lsds = _tiny_prior(hair)(d, idx=idx)
    (Lsds * opt.lambda_dsds).backward()
    Lsds = Lsds.detach()
    assert float(Lsds) > 0 and torch.equal(hair.Lsds.detach(), Lsds.detach())
    assert torch.equal(loss, base_loss + Lsds.detach() * opt.lambda_dsds)
    assert float(d.grad.abs().max()) > 0 and torch.equal(grad, base_grad + d.grad)
    # two views: the prior is evaluated once, by the step's first rebuild, and its term is added once, whole
    opt, head, hair, cam = _scene_with_ground_truth()
    two_base, _, _ = _one_step(hair, head, cam, opt, cams=[cam, copy.copy(cam)])
    opt, head, hair, cam = _scene_with_ground_truth()
    hair.attach_prior(_tiny_prior(hair))
    two, _, calls = _one_step(hair, head, cam, opt, cams=[cam, copy.copy(cam)])
    assert calls == [((), {}), ((), {"prior": False})]
    assert torch.equal(hair.prior.last_idx, idx)
    assert abs(float(two) - float(two_base) - opt.lambda_dsds * float(Lsds)) <= 1e-6 * abs(float(two))
    hair.attach_prior(None)
    assert hair.use_sds is False and hair.Lsds is None


def test_lambda_dsds_has_the_reference_default():
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    assert OptimizationParams().lambda_dsds == 0.0                         # arguments/__init__.py; run.sh passes 0.01
