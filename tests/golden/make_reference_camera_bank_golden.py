"""Generates tests/golden/reference_camera_bank_golden.npz from THE REFERENCE'S OWN ``Camera`` (src/scene/cameras.py:21-154,
with ``lie.se3_to_SE3`` of src/utils/camera_opt_utils.py:84-141 behind it), loaded read-only from /root/reference BY FILE PATH
(the package's ``scene/__init__`` pulls plyfile), ``easydict`` stubbed, the "cuda" factories redirected to the CPU:

    python tests/golden/make_reference_camera_bank_golden.py        # build container only (needs /root/reference)

For both parametrisations (``use_barf`` True: se(3); False: ortho-6D): cameras 5 .. 10 of the 32-camera ring rolled by 20 degrees,
64 x 48, their residuals perturbed by seeded normals of scale 0, 1e-3, 1e-2, 0.1, 0.5, 1.5 (the FoV residual a tenth of that),
seeded normal cotangents on world_view_transform, full_proj_transform, camera_center, FoVx and FoVy.  Stored per case: the inputs,
the reference's fp32 outputs and residual gradients (all five cotangents, world_view_transform's alone, and one on
projection_matrix alone), and the same from an
IEEE-double restatement (``compose64`` below, the camera centre through a 4x4 inverse) -- the arbiter, as in
reference_camera_golden.npz.  Numeric arrays only; nothing of the reference is copied.

``compose64`` / ``vjp64`` are also what the tests push other cotangents through (tests/test_gpu_camera_bank.py)."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference/src"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SCALES = (0.0, 1e-3, 1e-2, 0.1, 0.5, 1.5)
RING, FIRST, W, H, ROLL = 32, 5, 64, 48, 20.0
TAGS = {True: "se3/", False: "ortho6d/"}
OUTPUTS = ("view", "full", "center", "fovx", "fovy", "proj")
ZNEAR, ZFAR = 0.01, 100.0


def _poly64(s, offset):
    """sum_k (-1)^k s^k / (2 k + offset)!, k = 0 .. 10, in double (exact rational coefficients, rounded once)"""
    from fractions import Fraction
    from math import factorial
    acc = torch.zeros_like(s)
    for k in range(10, -1, -1):
        acc = acc * s + float(Fraction((-1) ** k, factorial(2 * k + offset)))
    return acc


def compose64(use_barf, w2c, fov0, rot, trans, fov_res):
    """The reference's camera in IEEE double: (view, full, center, FoVx, FoVy, proj) from W2C [4,4], FoV0 [2] and the residuals
    (all float64 tensors).  The series are the reference's eleven terms, in theta^2."""
    dd = dict(dtype=torch.float64)
    if use_barf:
        wx = torch.zeros(3, 3, **dd)
        wx = wx.index_put((torch.tensor([2, 0, 1]), torch.tensor([1, 2, 0])), rot).index_put((torch.tensor([1, 2, 0]), torch.tensor([2, 0, 1])), -rot)
        s = (rot * rot).sum()
        A, B, C = _poly64(s, 1), _poly64(s, 2), _poly64(s, 3)
        eye = torch.eye(3, **dd)
        R, V = eye + A * wx + B * wx @ wx, eye + B * wx + C * wx @ wx
        top = torch.cat([R, V @ trans[:, None]], dim=1)
    else:
        x_raw, y_raw = rot[0:3], rot[3:6]
        x = x_raw / x_raw.norm().clamp(min=1e-12)
        f = (x * y_raw).sum() / (torch.clamp((x * x).sum(), min=1e-8) + 1e-10)
        u = y_raw - f * x
        y = u / u.norm().clamp(min=1e-12)
        z = torch.linalg.cross(x, y)
        top = torch.cat([torch.stack([x, y, z], -1), trans[:, None]], dim=1)
    residual = torch.cat([top, torch.tensor([[0.0, 0.0, 0.0, 1.0]], **dd)], dim=0)
    view = (w2c @ residual).transpose(0, 1)
    fov = fov0 + fov_res
    t = torch.tan(fov / 2)
    P = torch.zeros(4, 4, **dd)
    P[2, 3], P[2, 2], P[3, 2] = 1.0, ZFAR / (ZFAR - ZNEAR), -(ZFAR * ZNEAR) / (ZFAR - ZNEAR)   # (transposed)
    e = torch.zeros(2, 4, 4, **dd)
    e[0, 0, 0] = e[1, 1, 1] = 1.0
    proj = P + e[0] / t[0] + e[1] / t[1]
    full = view @ proj
    center = torch.linalg.inv(view)[3, :3]
    return view, full, center, fov[0], fov[1], proj


def vjp64(use_barf, consts_row, params_row, cot):
    """dL/d(params row) in double.  consts_row: the bank's constants row (W2C[16] | FoV0[2] | ...), params_row: rot | trans | fov;
    cot: {"view" | "full" | "center" | "fovx" | "fovy" | "proj": cotangent} (absent = none).  Returns (outputs, gradient) as numpy."""
    c = torch.as_tensor(np.asarray(consts_row, dtype=np.float64))
    p = torch.as_tensor(np.asarray(params_row, dtype=np.float64)).clone().requires_grad_(True)
    rd = 3 if use_barf else 6
    outs = compose64(use_barf, c[:16].view(4, 4), c[16:18], p[:rd], p[rd:rd + 3], p[rd + 3:])
    loss = torch.zeros((), dtype=torch.float64)
    for n, t in zip(OUTPUTS, outs):
        if cot.get(n) is not None:
            loss = loss + (t * torch.as_tensor(np.asarray(cot[n], dtype=np.float64)).reshape(t.shape)).sum()
    g = torch.autograd.grad(loss, p, allow_unused=True)[0]
    return {n: t.detach().numpy() for n, t in zip(OUTPUTS, outs)}, (torch.zeros_like(p) if g is None else g).numpy()


def case_inputs(use_barf):
    """The seeded inputs of one parametrisation (our generator only supplies INPUTS): ring cameras' (R, T, FoV), parameter rows,
    cotangents."""
    from gaussianhaircut_amd.scene.cameras import ring_cameras
    cams = ring_cameras(RING, W, H, roll_deg=ROLL)[FIRST:FIRST + len(SCALES)]
    g = torch.Generator().manual_seed(1234 + int(use_barf))
    rd = 3 if use_barf else 6
    init = torch.zeros(rd + 5)
    if not use_barf:
        init[:6] = torch.eye(3, 3)[:2].reshape(-1)
    params = torch.stack([init + s * torch.randn(rd + 5, generator=g) * torch.tensor([1.0] * (rd + 3) + [0.1] * 2) for s in SCALES])
    n = len(SCALES)
    cot = dict(view=torch.randn(n, 4, 4, generator=g), full=torch.randn(n, 4, 4, generator=g), center=torch.randn(n, 3, generator=g),
               fovx=torch.randn(n, generator=g), fovy=torch.randn(n, generator=g))
    cot["proj"] = torch.randn(n, 4, 4, generator=g)   # (drawn last: the five above are the ones the reference's loss reads)
    return cams, params, cot


def _patch_cuda_factories():
    def wrap(fn):
        def inner(*a, **k):
            if str(k.get("device", "")).startswith("cuda"):
                k["device"] = "cpu"
            return fn(*a, **k)
        return inner
    for name in ("zeros", "ones", "arange", "tensor", "empty", "full", "eye"):
        setattr(torch, name, wrap(getattr(torch, name)))
    torch.Tensor.cuda = lambda self, *a, **k: self


def main():
    assert os.path.isdir(REF), "run in the build container (needs /root/reference)"
    _patch_cuda_factories()
    ed = types.ModuleType("easydict")
    ed.EasyDict = dict
    sys.modules["easydict"] = ed
    sys.path.insert(0, REF)
    for m in [k for k in sys.modules if k == "utils" or k.startswith("utils.")]:
        del sys.modules[m]
    spec = importlib.util.spec_from_file_location("ref_scene_cameras", os.path.join(REF, "scene", "cameras.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    out = {}
    worst_out = worst_grad = 0.0
    for use_barf in (True, False):
        tag = TAGS[use_barf]
        cams, params, cot = case_inputs(use_barf)
        rd = 3 if use_barf else 6
        res = {k: [] for k in ("w2c", "fov0", "R", "T", "grad32", "grad64", "gradview32", "gradview64", "gradproj32", "gradproj64")}
        for n in OUTPUTS:
            res[n + "32"], res[n + "64"] = [], []
        for i, c in enumerate(cams):
            img, one = torch.zeros(3, H, W), torch.zeros(1, H, W)
            rc = ref.Camera(i, c.R, c.T, float(c.FoVx), float(c.FoVy), W, H, img, one, one, one, one, one, c.image_name, i,
                            data_device="cpu", trainable_cameras=True, use_barf=use_barf, trainable_intrinsics=True)
            rc._rotation_res.data = params[i, :rd].clone()
            rc._translation_res.data = params[i, rd:rd + 3].clone()
            rc._fov_res.data = params[i, rd + 3:].clone()
            leaves = [rc._rotation_res, rc._translation_res, rc._fov_res]

            def grads(loss):
                gs = torch.autograd.grad(loss, leaves, allow_unused=True)
                return torch.cat([torch.zeros_like(p) if g_ is None else g_ for g_, p in zip(gs, leaves)]).numpy()

            o32 = dict(view=rc.world_view_transform, full=rc.full_proj_transform, center=rc.camera_center, fovx=rc.FoVx.reshape(()),
                       fovy=rc.FoVy.reshape(()), proj=rc.projection_matrix)
            loss = sum((o32[n] * cot[n][i]).sum() for n in ("view", "full", "center", "fovx", "fovy"))
            res["grad32"].append(grads(loss))
            res["gradview32"].append(grads((rc.world_view_transform * cot["view"][i]).sum()))
            res["gradproj32"].append(grads((rc.projection_matrix * cot["proj"][i]).sum()))
            w2c = rc._colmap_transform.detach().numpy().astype(np.float32)
            fov0 = np.array([float(rc._FoVx), float(rc._FoVy)], dtype=np.float32)   # (fp32 values, read exactly)
            crow = np.concatenate([w2c.reshape(-1), fov0]).astype(np.float64)
            c64 = {n: cot[n][i].numpy() for n in ("view", "full", "center", "fovx", "fovy")}
            o64, g64 = vjp64(use_barf, crow, params[i].numpy(), c64)
            _, gv64 = vjp64(use_barf, crow, params[i].numpy(), dict(view=c64["view"]))
            res["grad64"].append(g64)
            res["gradview64"].append(gv64)
            res["gradproj64"].append(vjp64(use_barf, crow, params[i].numpy(), dict(proj=cot["proj"][i].numpy()))[1])
            for n in OUTPUTS:
                res[n + "32"].append(o32[n].detach().numpy().astype(np.float32))
                res[n + "64"].append(o64[n])
                worst_out = max(worst_out, float(np.abs(res[n + "32"][-1] - o64[n]).max() / np.abs(o64[n]).max()))
            worst_grad = max(worst_grad, float(np.abs(res["grad32"][-1] - g64).max() / np.abs(g64).max()))
            res["w2c"].append(w2c)
            res["fov0"].append(fov0)
            res["R"].append(np.asarray(c.R, dtype=np.float64))
            res["T"].append(np.asarray(c.T, dtype=np.float64))
        for k, v in res.items():
            out[tag + k] = np.stack(v)
        out[tag + "params"] = params.numpy()
        for n, t in cot.items():
            out[tag + "cot_" + n] = t.numpy()
    dst = os.path.join(HERE, "reference_camera_bank_golden.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes;", len(out), "arrays")
    print("the reference's own fp32 chain vs the double restatement, of max: outputs %.3g, gradients %.3g" % (worst_out, worst_grad))


if __name__ == "__main__":
    main()
