"""The camera bank's device functions (csrc/ghr_camera.h: cam_compose_row, cam_compose_bwd_row, cam_adam_row -- `__host__
__device__`) on the CPU, through tests/hostsim/ghr_hostsim_camera.cpp, against the reference's golden under the bar of
tests/test_camera_bank.py, and the Adam row against torch.optim.Adam at the project's rtol 2e-6 / atol 1e-7
(tests/test_gpu_loss_adam.py::test_fused_adam_matches_torch_adam_and_nan_guard).

``compose_case`` and ``adam_scenario`` are written against a small array interface (``SimApi`` here) so that
tests/test_gpu_camera_bank.py runs the same cases through the C ABI on the device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import helpers as hp
from tests.golden import make_reference_camera_bank_golden as mk
from tests.test_camera_bank import PARAMS, bank_from, check, check_grad_row, gold, sub  # noqa: F401  (gold: fixture)

COT = ("view", "full", "proj", "center", "fovx", "fovy")   # order of the C ABI's cotangent pointers
OUT_SLICES = dict(view=slice(0, 16), full=slice(16, 32), proj=slice(32, 48), center=slice(48, 51), fovx=slice(51, 52),
                  fovy=slice(52, 53))
ADAM_RTOL, ADAM_ATOL = 2e-6, 1e-7


def _build():
    """as helpers.HostSim._build compiles its file"""
    src = os.path.join(hp.ROOT, "tests", "hostsim", "ghr_hostsim_camera.cpp")
    out_dir = os.path.join(hp.ROOT, "tests", "hostsim", "_build")
    so = os.path.join(out_dir, "libghr_hostsim_camera.so")
    csrc = os.path.join(hp.ROOT, "gaussianhaircut_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(out_dir, exist_ok=True)
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-x", "hip", "-O2", "-std=c++17", "-ffp-contract=off",
                        "-fPIC", "-shared", "-o", so, src], check=True)
    return so


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


class SimApi:
    """numpy in, numpy out; the three calls of include/ghr.h's camera bank on the CPU"""

    def __init__(self):
        import torch  # noqa: F401  (one HIP runtime for every HIP-linked library of the process)
        self.L = ctypes.CDLL(_build())

    def compose(self, param, first, n, consts, params):
        out = np.full((n, 53), np.nan, np.float32)
        self.L.ghrsim_cam_compose(param, first, n, _p(consts), consts.shape[1], _p(params), params.shape[1], _p(out), 53)
        return out

    def backward(self, param, first, n, consts, params, cot, grads, touched, mask=3):
        cot = [None if cot.get(k) is None else np.ascontiguousarray(cot[k], dtype=np.float32) for k in COT]
        grads, touched = grads.copy(), touched.copy()
        self.L.ghrsim_cam_compose_bwd(param, first, n, _p(consts), consts.shape[1], _p(params), params.shape[1], *[_p(c) for c in cot],
                                      _p(grads), grads.shape[1], _p(touched), mask)
        return grads, touched

    def adam(self, param, st, lrs, mask=3):
        """st: dict of numpy arrays p, g, m, v [N, W], steps, touched [N] int32 -- updated in place"""
        self.L.ghrsim_cam_adam(param, len(st["steps"]), _p(st["p"]), _p(st["g"]), _p(st["m"]), _p(st["v"]), st["p"].shape[1],
                               _p(st["steps"]), _p(st["touched"]), ctypes.c_float(lrs[0]), ctypes.c_float(lrs[1]),
                               ctypes.c_float(lrs[2]), ctypes.c_double(0.9), ctypes.c_double(0.999), ctypes.c_float(1e-15), mask)


@pytest.fixture(scope="module")
def sim():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not found")
    return SimApi()


def bank_rows(ref, use_barf, N):
    """constants and parameter rows of an N-camera bank whose row j is the golden's case j % 6"""
    bank = bank_from(ref, use_barf)
    idx = np.arange(N) % len(bank)
    return np.ascontiguousarray(bank.consts.numpy()[idx]), np.ascontiguousarray(bank.params.numpy()[idx]), idx


WHICH = {"all": (("view", "full", "center", "fovx", "fovy"), "grad"), "view": (("view",), "gradview"), "proj": (("proj",), "gradproj")}


def compose_case(api, ref, use_barf, N, first, n, which="all"):
    """Rows [first, first + n) of an N-camera bank through compose and backward, with the five cotangents the reference's loss
    reads, with world_view_transform's alone or with projection_matrix's alone; returns the worst err / bar (outputs, gradients)."""
    param = 1 if use_barf else 0
    consts, params, idx = bank_rows(ref, use_barf, N)
    case = idx[first:first + n]
    out = api.compose(param, first, n, consts, params)
    worst_o = 0.0
    for r, c in enumerate(case):
        for name, sl in OUT_SLICES.items():
            worst_o = max(worst_o, check(out[r, sl].reshape(ref[name + "64"][c].shape), ref[name + "64"][c], ref[name + "32"][c],
                                         "%s row %d (case %d)" % (name, first + r, c)))
    names, gkey = WHICH[which]
    cot = {k: np.stack([ref["cot_" + k][c] for c in case]).astype(np.float32) for k in names}
    W = params.shape[1]
    rng = np.random.default_rng(5)
    grads0 = rng.standard_normal((N, W)).astype(np.float32)
    grads0[first] = np.nan   # a stale NaN in a row whose mark is down is overwritten, not added to
    touched0 = np.zeros(N, np.int32)
    grads, touched = api.backward(param, first, n, consts, params, cot, grads0, touched0)
    inside = np.zeros(N, bool)
    inside[first:first + n] = True
    assert np.array_equal(grads[~inside].view(np.uint32), grads0[~inside].view(np.uint32))   # bit for bit
    assert np.array_equal(touched, inside.astype(np.int32))
    g64, g32 = gkey + "64", gkey + "32"
    worst_g = 0.0
    for r, c in enumerate(case):
        worst_g = max(worst_g, check_grad_row(grads[first + r], ref[g64][c], ref[g32][c], use_barf, "grad row %d (case %d)" % (first + r, c)))
    # a second backward into the now touched rows ADDS: twice the gradient, to the last bit (x + x is exact)
    grads2, touched2 = api.backward(param, first, n, consts, params, cot, grads, touched)
    assert np.array_equal(grads2[inside], 2 * grads[inside]) and np.array_equal(touched2, touched)
    assert np.array_equal(grads2[~inside].view(np.uint32), grads0[~inside].view(np.uint32))
    return worst_o, worst_g


@pytest.mark.parametrize("use_barf", PARAMS)
def test_hostsim_compose_and_backward_reproduce_the_reference_camera(sim, gold, use_barf):
    ref = sub(gold, use_barf)
    worst = [0.0, 0.0]
    for N, first, n, which in ((6, 0, 6, "all"), (6, 0, 6, "view"), (6, 0, 6, "proj"), (6, 2, 1, "all"), (8, 2, 5, "view"), (8, 2, 5, "proj")):
        o, g = compose_case(sim, ref, use_barf, N, first, n, which)
        worst = [max(worst[0], o), max(worst[1], g)]
    print("camera bank, host-sim, use_barf=%s: worst err / bar outputs %.3g gradients %.3g" % (use_barf, worst[0], worst[1]))


@pytest.mark.parametrize("use_barf", PARAMS)
def test_hostsim_backward_leaves_frozen_groups_alone(sim, gold, use_barf):
    ref = sub(gold, use_barf)
    consts, params, idx = bank_rows(ref, use_barf, 6)
    rd = 3 if use_barf else 6
    cot = {k: ref["cot_" + k].astype(np.float32) for k in ("view", "full", "center", "fovx", "fovy")}
    full, _ = sim.backward(int(use_barf), 0, 6, consts, params, cot, np.zeros_like(params), np.zeros(6, np.int32), mask=3)
    pose, _ = sim.backward(int(use_barf), 0, 6, consts, params, cot, np.ones_like(params), np.zeros(6, np.int32), mask=1)
    fov, _ = sim.backward(int(use_barf), 0, 6, consts, params, cot, np.ones_like(params), np.zeros(6, np.int32), mask=2)
    assert np.array_equal(pose[:, :rd + 3], full[:, :rd + 3]) and not pose[:, rd + 3:].any()
    assert np.array_equal(fov[:, rd + 3:], full[:, rd + 3:]) and not fov[:, :rd + 3].any()


# ---- Adam ------------------------------------------------------------------------------------------------------------------
ADAM_N = 130
ADAM_TOUCHED = [[0], [1], [0, 64, 129], [], [0], list(range(ADAM_N))]


def adam_scenario(api, use_barf):
    """Six steps with injected gradients against torch.optim.Adam(lr=0, eps=1e-15) over 3 N parameters in three groups with
    distinct, changing learning rates (torch side: .grad = None for cameras nobody viewed), then the NaN rule, then a stale NaN
    in a row nobody viewed."""
    param, rd = int(use_barf), 3 if use_barf else 6
    W, N = rd + 5, ADAM_N
    g = torch.Generator().manual_seed(77)
    p0 = torch.randn(N, W, generator=g)
    st = dict(p=p0.numpy().copy(), g=np.full((N, W), 123.0, np.float32), m=np.zeros((N, W), np.float32),
              v=np.zeros((N, W), np.float32), steps=np.zeros(N, np.int32), touched=np.zeros(N, np.int32))
    cols = (slice(0, rd), slice(rd, rd + 3), slice(rd + 3, W))
    tp = [[torch.nn.Parameter(p0[i, s].clone()) for i in range(N)] for s in cols]
    lrs = [1e-3, 3.2e-3, 2e-3]
    topt = torch.optim.Adam([{"params": tp[k], "lr": lrs[k]} for k in range(3)], lr=0.0, eps=1e-15)

    def compare(what):
        for k, s in enumerate(cols):
            for name, key in (("p", None), ("m", "exp_avg"), ("v", "exp_avg_sq")):
                ref = torch.stack([(q.detach() if key is None else topt.state[q][key] if q in topt.state and topt.state[q] else
                                    torch.zeros_like(q)) for q in tp[k]]).numpy()
                np.testing.assert_allclose(st[name][:, s], ref, rtol=ADAM_RTOL, atol=ADAM_ATOL, err_msg="%s %s group %d" % (what, name, k))

    def one_step(rows, lrs):
        gr = torch.randn(N, W, generator=g) * 1e-2
        for i in range(N):
            for k, s in enumerate(cols):
                tp[k][i].grad = gr[i, s].clone() if i in rows else None
        for k in range(3):
            topt.param_groups[k]["lr"] = lrs[k]
        st["g"][rows] = gr.numpy()[rows]
        st["touched"][rows] = 1
        return gr

    counts = np.zeros(N, np.int32)
    for t, rows in enumerate(ADAM_TOUCHED):
        lrs = [lrs[0], lrs[1] * 0.8, lrs[2]] if t != 2 else [lrs[0] * 2.0, lrs[1] * 0.8, lrs[2] * 0.5]   # the schedule moves
        one_step(rows, lrs)
        topt.step()
        api.adam(param, st, lrs)
        counts[rows] += 1
        assert np.array_equal(st["steps"], counts), t
        assert not st["touched"].any() and not st["g"][rows].any()
        if t < 5:   # rows nobody has viewed yet: gradients neither read nor written
            never = np.ones(N, bool)
            never[sum(ADAM_TOUCHED[:t + 1], [])] = False
            assert (st["g"][never] == 123.0).all()
        compare("step %d" % (t + 1))
    assert st["steps"][0] == 4 and st["steps"][2] == 1 and st["steps"][64] == 2 and st["steps"][129] == 2
    # a NaN in a viewed row: nothing moves for any camera, no count advances, gradients and marks are cleared
    keep = {k: v.copy() for k, v in st.items()}
    one_step([3, 70], lrs)
    st["g"][70, W - 1] = np.nan
    api.adam(param, st, lrs)
    for k in ("p", "m", "v", "steps"):
        assert np.array_equal(st[k], keep[k]), k
    assert not st["touched"].any() and not st["g"][[3, 70]].any()
    # a stale NaN in a row nobody viewed is ignored
    st["g"][5, 0] = np.nan
    one_step([7], lrs)
    topt.step()
    api.adam(param, st, lrs)
    counts[7] += 1
    assert np.array_equal(st["steps"], counts) and np.isnan(st["g"][5, 0])
    compare("step behind a stale NaN")


@pytest.mark.parametrize("use_barf", PARAMS)
def test_hostsim_adam_row_matches_torch_adam_with_per_camera_step_counts(sim, use_barf):
    adam_scenario(sim, use_barf)
