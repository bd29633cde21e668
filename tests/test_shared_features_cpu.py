"""The per-strand SH segment (csrc/ghr_shared.h) on the CPU, through tests/hostsim/ghr_hostsim_shared.cpp: the product's own
`__host__ __device__` row functions with strand-indexed coefficients against the same rows with expanded arrays, and the fold
against project_bwd_sh's stored rows summed by rows_reduce_one.

Bars (set by the feature's contract, include/ghr.h): every per-row output -- records, radii, rects, depths, NDC means, d_xyz,
d_scaling, d_rotation, d_dir3d, d_conf, d_means2D, the camera cotangents -- bit-identical; the per-strand feature gradients equal as
floats (==, +0 and -0 alike: a row without gradient contributes +0 to the fold where the stored row may hold -0; NaN in the same
places)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import helpers as hp
from tests import shared_feature_cases as sc


def _build():
    """as tests/test_latent_stage.py builds its library"""
    src = os.path.join(hp.ROOT, "tests", "hostsim", "ghr_hostsim_shared.cpp")
    out_dir = os.path.join(hp.ROOT, "tests", "hostsim", "_build")
    so = os.path.join(out_dir, "libghr_hostsim_shared.so")
    csrc = os.path.join(hp.ROOT, "gaussianhaircut_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(out_dir, exist_ok=True)
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-x", "hip", "-O2", "-std=c++17", "-ffp-contract=off",
                        "-fPIC", "-shared", "-o", so, src], check=True)
    return so


@pytest.fixture(scope="module")
def sim():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    import torch  # noqa: F401  (one HIP runtime for every HIP-linked library of the process)
    return ctypes.CDLL(_build())


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _args(sce, f_dc, f_rest, deg, keep):
    a = hp.ModelArgsC()
    arr = dict(xyz=hp.np32(sce["xyz"]), log_scales=hp.np32(sce["scaling"]), rotations=hp.np32(sce["rotation"]),
               orient_conf_log=hp.np32(sce["conf"]), dir3d=hp.np32(sce["dir"]), features_dc=hp.np32(f_dc),
               features_rest=hp.np32(f_rest), view=hp.np32(sce["view"]).reshape(-1), proj=hp.np32(sce["proj"]).reshape(-1),
               campos=hp.np32(sce["campos"]))
    keep.append(arr)
    for k, v in arr.items():
        setattr(a, k, v.ctypes.data if v.size else arr["xyz"].ctypes.data)
    a.P, a.W, a.H = sce["P"], sce["W"], sce["H"]
    a.sh_degree, a.sh_coeffs, a.mode, a.row0 = deg, sce["K"], 1, 0
    a.const_opacity, a.const_label, a.const_conf = 1.0, 1.0, 0.0
    a.scale_modifier, a.tan_fovx, a.tan_fovy, a.conic_eps = 1.0, sce["tanfovx"], sce["tanfovy"], 1e-7
    a.focal_x, a.focal_y = a.W / (2.0 * a.tan_fovx), a.H / (2.0 * a.tan_fovy)
    return a


def _forward(sim, a, n_seg):
    P = a.P
    o = dict(rec=np.full((P, 16), np.nan, np.float32), radii=np.full(P, -1, np.int32), means2D=np.full((P, 3), np.nan, np.float32),
             depths=np.full(P, np.nan, np.float32), rects=np.full((P, 4), 0xFFFFFFFF, np.uint32))
    sim.ghrsim_shared_forward(ctypes.byref(a), n_seg, *[_p(o[k]) for k in ("rec", "radii", "means2D", "depths", "rects")])
    return o


def _backward(sim, a, n_seg, radii, gacc, S, K):
    P = a.P
    nan = lambda *s: np.full(s, np.nan, np.float32)  # noqa: E731
    o = dict(d_means2D=nan(P, 3), d_xyz=nan(P, 3), d_scaling=nan(P, 3), d_rotation=nan(P, 4), d_conf=nan(P), d_dir=nan(P, 3),
             d_fdc=nan(P, 3), d_frest=nan(P, 3 * (K - 1)), d_rgb=nan(P, 3), cam=nan(P, 32))
    flag = sim.ghrsim_shared_backward(ctypes.byref(a), n_seg, _p(radii), _p(gacc), *[_p(o[k]) for k in (
        "d_means2D", "d_xyz", "d_scaling", "d_rotation", "d_conf", "d_dir", "d_fdc", "d_frest", "d_rgb", "cam")])
    return o, int(flag)


ROW_KEYS = ("d_means2D", "d_xyz", "d_scaling", "d_rotation", "d_conf", "d_dir", "cam")


@pytest.mark.parametrize("n_seg", [1, 2, 99])
@pytest.mark.parametrize("K,deg", [(1, 0), (16, 0), (16, 2), (16, 3)])
def test_strand_indexed_rows_and_the_fold_equal_the_expanded_form(sim, n_seg, K, deg):
    S = 5
    sce = sc.make_scene(S, n_seg, K, 0)
    P, keep = sce["P"], []
    a_sh = _args(sce, sce["f_dc"], sce["f_rest"], deg, keep)
    a_ex = _args(sce, sc.expanded(sce["f_dc"], n_seg), sc.expanded(sce["f_rest"], n_seg), deg, keep)
    f_sh, f_ex = _forward(sim, a_sh, n_seg), _forward(sim, a_ex, 0)
    for k in f_ex:
        assert f_sh[k].tobytes() == f_ex[k].tobytes(), k
    radii = f_ex["radii"]
    behind = sc.behind_strand(S)
    rows_b = slice(behind * n_seg, (behind + 1) * n_seg)
    assert (radii[rows_b] == 0).all() and (radii[: behind * n_seg] > 0).any()

    rng = np.random.default_rng(7 + n_seg + K + deg)
    gacc = rng.standard_normal((P, 16)).astype(np.float32)
    gacc[radii <= 0] = 0.0     # K8 leaves no gradient on a culled row
    for plant in (None, "nan"):
        g = gacc.copy()
        victim = None
        if plant:
            victim = int(np.flatnonzero(radii[n_seg: 2 * n_seg] > 0)[0]) + n_seg   # a visible row of strand 1
            g[victim, 6] = np.nan                                               # dL/d(red) of that row
        b_ex, flag_ex = _backward(sim, a_ex, 0, radii, g, S, K)
        b_sh, flag_sh = _backward(sim, a_sh, n_seg, radii, g, S, K)
        for k in ROW_KEYS:
            assert b_sh[k].tobytes() == b_ex[k].tobytes(), (k, plant)
        assert np.isnan(b_sh["d_fdc"]).all() and np.isnan(b_sh["d_frest"]).all()      # the factored form stores no feature row
        ref_dc = np.full((S, 3), np.nan, np.float32)
        ref_rest = np.full((S, 3 * (K - 1)), np.nan, np.float32)
        sim.ghrsim_shared_rows_reduce(S, n_seg, 3, _p(b_ex["d_fdc"]), _p(ref_dc))
        if K > 1:
            sim.ghrsim_shared_rows_reduce(S, n_seg, 3 * (K - 1), _p(b_ex["d_frest"]), _p(ref_rest))
        dc, rest = np.full((S, 3), np.nan, np.float32), np.full((S, 3 * (K - 1)), np.nan, np.float32)
        xyz, campos = hp.np32(sce["xyz"]), hp.np32(sce["campos"])
        flag_fold = sim.ghrsim_shared_fold(S, n_seg, deg, K, _p(xyz), _p(campos), _p(b_sh["d_rgb"]), _p(dc), _p(rest))
        assert sc.same_floats(dc, ref_dc) and sc.same_floats(rest, ref_rest), plant
        # the strand behind the camera: exact zeros; bands above the active degree: zeros
        assert (dc[behind] == 0).all() and (rest[behind] == 0).all()
        n_act = (deg + 1) ** 2
        if plant is None:
            assert flag_fold == 0 and flag_sh == 0 and flag_ex == 0
            assert np.isfinite(dc).all() and np.isfinite(rest).all()
            assert (rest.reshape(S, K - 1, 3)[:, max(n_act - 1, 0):] == 0).all()
            front = np.concatenate([dc.reshape(S, 1, 3), rest.reshape(S, K - 1, 3)], axis=1)[:behind, :min(n_act, K)]
            assert (np.abs(front).max(axis=(0, 2)) > 0).all()                         # every active band carries a gradient
        else:
            assert flag_fold == 1 and flag_sh == 1 and flag_ex == 1
            bad = np.isnan(np.concatenate([dc, rest], axis=1)).any(axis=1)
            assert bad.tolist() == [s == 1 for s in range(S)]                         # NaN in that strand only
            assert np.isnan(dc[1, 0])


def test_a_row_without_gradient_is_not_evaluated(sim):
    """d_rgb == 0 contributes +0 even where the direction is undefined (a Gaussian AT the camera centre: 0 / 0)"""
    n_seg, K, deg = 3, 16, 3
    campos = np.array([0.5, -1.0, 2.0], np.float32)
    xyz = np.stack([campos, campos + 1, campos]).astype(np.float32)
    d_rgb = np.array([[0, 0, 0], [0.5, -2.0, 0.0], [0, 0, 0]], np.float32)
    dc, rest = np.full((1, 3), np.nan, np.float32), np.full((1, 45), np.nan, np.float32)
    assert sim.ghrsim_shared_fold(1, n_seg, deg, K, _p(xyz), _p(campos), _p(d_rgb), _p(dc), _p(rest)) == 0
    assert np.isfinite(dc).all() and np.isfinite(rest).all() and dc[0, 0] > 0 and dc[0, 1] < 0 and dc[0, 2] == 0
    # all rows without gradient: +0 everywhere
    dc[:], rest[:] = np.nan, np.nan
    z = np.zeros((3, 3), np.float32)
    assert sim.ghrsim_shared_fold(1, n_seg, deg, K, _p(xyz), _p(campos), _p(z), _p(dc), _p(rest)) == 0
    assert not np.signbit(dc).any() and (dc == 0).all() and not np.signbit(rest).any() and (rest == 0).all()
