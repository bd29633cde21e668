"""Minimal camera carrying exactly the fields ``render()`` and the model's projection helpers consume
(reference: ``src/scene/cameras.py:72-80`` / ``MiniCam``): image size, FoV, ``world_view_transform`` (= W2C^T),
``full_proj_transform`` (= view @ proj, row-vector convention) and ``camera_center``; plus optional ground truth."""
from __future__ import annotations

import contextlib
import ctypes
import math
from typing import Optional

import numpy as np
import torch

from ..utils.graphics_utils import getProjectionMatrix, getWorld2View2


class Camera:
    def __init__(self, R, T, FoVx, FoVy, width, height, znear=0.01, zfar=100.0, device="cpu", image_name="synthetic"):
        self.image_width, self.image_height = int(width), int(height)
        # tensors, like the reference (trainable FoV there): render() calls torch.tan(FoV * 0.5).item()
        self.FoVx = torch.tensor(float(FoVx), dtype=torch.float32, device=device)
        self.FoVy = torch.tensor(float(FoVy), dtype=torch.float32, device=device)
        self.znear, self.zfar = znear, zfar
        self.image_name = image_name
        self.R, self.T = np.asarray(R, dtype=np.float64), np.asarray(T, dtype=np.float64)   # as src/scene/cameras.py:37-38
        w2c = torch.tensor(getWorld2View2(np.asarray(R), np.asarray(T)), dtype=torch.float32)
        self.world_view_transform = w2c.transpose(0, 1).contiguous().to(device)
        self.projection_matrix = getProjectionMatrix(znear, zfar, float(FoVx), float(FoVy)).transpose(0, 1).to(device)
        self.full_proj_transform = (self.world_view_transform @ self.projection_matrix).contiguous()
        self.camera_center = torch.inverse(self.world_view_transform.cpu())[3, :3].to(device)
        self.original_image: Optional[torch.Tensor] = None
        self.original_mask: Optional[torch.Tensor] = None
        self.original_orient_angle: Optional[torch.Tensor] = None
        self.original_orient_conf: Optional[torch.Tensor] = None

    def to(self, device):
        for k, v in list(self.__dict__.items()):
            if isinstance(v, torch.nn.Parameter):
                self.__dict__[k] = torch.nn.Parameter(v.detach().to(device), requires_grad=v.requires_grad)
            elif isinstance(v, torch.Tensor):
                self.__dict__[k] = v.to(device)
        return self


def ortho2rotation(poses: torch.Tensor) -> torch.Tensor:
    """6D rotation parametrisation -> rotation matrix with columns (x, y, z): Gram-Schmidt of the two 3-vectors, z = x cross y
    (semantics of the reference's ``ortho2rotation``, src/scene/cameras.py:170-197, incl. its clamp(|x|^2, 1e-8) + 1e-10)."""
    x_raw, y_raw = poses[..., 0:3], poses[..., 3:6]
    x = torch.nn.functional.normalize(x_raw, dim=-1)
    factor = (x * y_raw).sum(-1, keepdim=True) / (torch.clamp((x ** 2).sum(-1, keepdim=True), min=1e-8) + 1e-10)
    y = torch.nn.functional.normalize(y_raw - factor * x, dim=-1)
    z = torch.cross(x, y, dim=-1)
    return torch.stack([x, y, z], -1)


class TrainableCamera(Camera):
    """A camera whose pose and field of view are functions of trainable residuals, as the reference trains them by default
    (src/arguments/__init__.py:61-62; parametrisation of src/scene/cameras.py:85-151, the ``use_barf = False`` branch):
    ``world_view_transform = (W2C @ [[R(rotation_res), translation_res], [0, 1]])^T``, ``FoV = FoV0 + fov_res``.  The reference
    rebuilds every matrix on every property access (and inverts a 4x4 for the camera centre); here ``tensors()`` builds all
    five once per call under autograd -- ``render()`` asks for them once per view (``fused.camera_inputs``) -- and the
    properties are thin views of the same computation for code that reads them one by one.  BARF's se(3) parametrisation
    (utils/camera_opt_utils.py), the reference's default, is what ``CameraBank`` below composes -- one launch per view, with the
    cameras' own Adam; this class stays the PyTorch-composed ortho-6D form (``bench.py`` times it)."""

    def __init__(self, R, T, FoVx, FoVy, width, height, znear=0.01, zfar=100.0, device="cpu", image_name="synthetic",
                 trainable_cameras=True, trainable_intrinsics=True):
        base = Camera(R, T, FoVx, FoVy, width, height, znear, zfar, device, image_name)
        dev = torch.device(device)
        fixed = dict(base.__dict__)
        self._colmap_transform = fixed.pop("world_view_transform").transpose(0, 1).contiguous()   # W2C
        self._FoVx, self._FoVy = fixed.pop("FoVx"), fixed.pop("FoVy")
        for k in ("projection_matrix", "full_proj_transform", "camera_center"):
            fixed.pop(k)
        self.__dict__.update(fixed)  # image size, znear / zfar, R / T, name, ground-truth slots
        self.trainable_cameras, self.trainable_intrinsics = bool(trainable_cameras), bool(trainable_intrinsics)
        self._rotation_res = torch.nn.Parameter(torch.eye(3, 3)[:2].reshape(-1).clone().to(dev), requires_grad=self.trainable_cameras)
        self._translation_res = torch.nn.Parameter(torch.zeros(3, device=dev), requires_grad=self.trainable_cameras)
        self._fov_res = torch.nn.Parameter(torch.zeros(2, device=dev), requires_grad=self.trainable_intrinsics)
        P0 = torch.zeros(4, 4)
        P0[2, 3], P0[2, 2], P0[3, 2] = 1.0, zfar / (zfar - znear), -(zfar * znear) / (zfar - znear)  # (already transposed)
        self._proj_const = P0.to(dev)
        e = torch.zeros(2, 4, 4)
        e[0, 0, 0] = e[1, 1, 1] = 1.0
        self._proj_slots = e.to(dev)
        self._bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]], device=dev)

    def parameters(self):
        return [self._rotation_res, self._translation_res, self._fov_res]

    def tensors(self):
        """(world_view_transform, full_proj_transform, camera_center, FoVx, FoVy, projection_matrix), one graph."""
        R_a = ortho2rotation(self._rotation_res)
        residual = torch.cat([torch.cat([R_a, self._translation_res[:, None]], dim=1), self._bottom], dim=0)
        view = (self._colmap_transform @ residual).transpose(0, 1)
        fov = torch.stack([self._FoVx, self._FoVy]) + self._fov_res
        inv_tan = 1.0 / torch.tan(fov * 0.5)   # P[0,0] = 2 n / (2 n tan(FoVx / 2)), graphics_utils.py:64-65
        proj = self._proj_const + (self._proj_slots * inv_tan[:, None, None]).sum(0)
        full = view @ proj
        # camera centre: the reference inverts the 4x4 (cameras.py:150); for a rigid transform inverse(view)[3, :3] = -t R^T
        center = -(view[3, :3] @ view[:3, :3].transpose(0, 1))
        return view, full, center, fov[0], fov[1], proj

    world_view_transform = property(lambda self: self.tensors()[0])
    full_proj_transform = property(lambda self: self.tensors()[1])
    camera_center = property(lambda self: self.tensors()[2])
    FoVx = property(lambda self: self.tensors()[3])
    FoVy = property(lambda self: self.tensors()[4])
    projection_matrix = property(lambda self: self.tensors()[5])


# ---------------------------------------------------------------------------------------------------------------------
# The camera bank: all trainable cameras of a scene as rows of flat buffers, composed / back-propagated / stepped by the three
# kernels of csrc/ghr_camera.h (include/ghr.h: ghr_camera_compose, ghr_camera_compose_backward, ghr_camera_adam_step).
def _sinc_family(s, offset):
    """sum_k (-1)^k s^k / (2 k + offset)!, k = 0 .. 10, by Horner's rule in s = theta^2: offset 1 is sin(t) / t, 2 is
    (1 - cos t) / t^2, 3 is (t - sin t) / t^3 -- the eleven-term polynomials the reference's se(3) exponential uses
    (utils/camera_opt_utils.py, nth = 10).  No square root and no division by theta: value and gradient are finite at w = 0."""
    coeff = [(-1.0) ** k / math.factorial(2 * k + offset) for k in range(11)]
    acc = torch.full_like(s, coeff[-1])
    for c in reversed(coeff[:-1]):
        acc = acc * s + c
    return acc


_SO3_GENERATORS = torch.tensor([[[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]],
                                [[0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [-1.0, 0.0, 0.0]],
                                [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]]])


def _cross_matrix(w):
    """[w]x = sum_k w_k G_k with the three generators of so(3)"""
    return torch.einsum("k,kij->ij", w, _SO3_GENERATORS.to(device=w.device, dtype=w.dtype))


def compose_camera_torch(use_barf, consts, rotation_res, translation_res, fov_res):
    """One camera of a ``CameraBank`` in PyTorch ops (the A/B comparator of the kernels, and the form CPU tensors take): the six
    tensors of ``tensors()`` from a constants row (include/ghr.h) and the three residuals.  Semantics of src/scene/cameras.py:
    94-154 for both parametrisations; the camera centre in the closed form -t R^T of the rigid transform."""
    W2C = consts[:16].view(4, 4)
    if use_barf:
        wx, s = _cross_matrix(rotation_res), (rotation_res * rotation_res).sum()
        A, B, C = _sinc_family(s, 1), _sinc_family(s, 2), _sinc_family(s, 3)
        eye, wx2 = torch.eye(3, dtype=consts.dtype, device=consts.device), wx @ wx
        R, V = eye + A * wx + B * wx2, eye + B * wx + C * wx2
        top = torch.cat([R, V @ translation_res[:, None]], dim=1)
    else:
        top = torch.cat([ortho2rotation(rotation_res), translation_res[:, None]], dim=1)
    bottom = torch.zeros(1, 4, dtype=consts.dtype, device=consts.device)
    bottom[0, 3] = 1.0
    view = (W2C @ torch.cat([top, bottom], dim=0)).transpose(0, 1)
    fov = consts[16:18] + fov_res
    znear = consts[18]
    right = torch.tan(fov / 2) * znear
    inv_tan = 2.0 * znear / (right - (-right))   # graphics_utils.py:55-65
    e = torch.zeros(5, 4, 4, dtype=consts.dtype, device=consts.device)
    e[0, 0, 0] = e[1, 1, 1] = e[2, 2, 2] = e[3, 3, 2] = e[4, 2, 3] = 1.0
    proj = e[0] * inv_tan[0] + e[1] * inv_tan[1] + e[2] * consts[19] + e[3] * consts[20] + e[4]
    full = view @ proj
    center = -(view[3, :3] @ view[:3, :3].transpose(0, 1))
    return view, full, center, fov[0], fov[1], proj


@torch.no_grad()
def pack_row_message_torch(grads, touched, message):
    """``k_cam_pack`` in PyTorch ops: ``message [N, width + 1]`` from ``grads [N, width]`` and ``touched [N]``."""
    W = grads.shape[1]
    t = touched != 0
    message[:, :W] = torch.where(t[:, None], grads, torch.zeros_like(grads))   # (selected, not multiplied: a stale NaN is dropped)
    message[:, W] = t.to(message.dtype)
    return message


@torch.no_grad()
def merge_ranks_torch(gathered, grads, touched):
    """``k_cam_merge`` in PyTorch ops: the ranks' messages ``gathered [G, N, width + 1]`` into ``grads`` / ``touched``, in place."""
    W = grads.shape[1]
    acc, seen = grads.clone(), torch.zeros_like(touched, dtype=torch.bool)
    for q in range(gathered.shape[0]):
        val, tq = gathered[q, :, :W], gathered[q, :, W] != 0
        acc = torch.where(tq[:, None], torch.where(seen[:, None], acc + val, val), acc)
        seen |= tq
    grads.copy_(acc)
    touched.copy_(torch.where(seen, torch.ones_like(touched), touched))


class _BankCompose(torch.autograd.Function):
    """``BankCamera.tensors()`` on a ROCm device: forward = one ghr_camera_compose of the camera's row, backward = one
    ghr_camera_compose_backward that writes into the bank's gradient row.  The only autograd input is the bank's anchor (a
    scalar leaf that makes autograd record the node); it gets no gradient -- nothing dense for autograd to accumulate."""

    @staticmethod
    def forward(ctx, anchor, bank, index):
        out = bank._compose_rows(index, 1)[0]
        ctx.bank, ctx.index = bank, index
        ctx.set_materialize_grads(False)
        return CameraBank._split(out)

    @staticmethod
    def backward(ctx, d_view, d_full, d_center, d_fovx, d_fovy, d_proj):
        ctx.bank._backward_rows(ctx.index, 1, d_view, d_full, d_proj, d_center, d_fovx, d_fovy)
        return None, None, None


class BankCamera:
    """Camera ``index`` of a ``CameraBank``: quacks like the reference's ``Camera`` (image size, znear / zfar, image_name, the
    ``original_*`` ground-truth slots, ``_rotation_res`` / ``_translation_res`` / ``_fov_res`` -- views of the bank's parameter
    row) with all six tensors from ONE evaluation (``tensors()``; ``fused.camera_inputs`` asks for it once per view)."""

    def __init__(self, bank, index, width, height, image_name, R=None, T=None, znear=0.01, zfar=100.0):
        self.bank, self.index = bank, int(index)
        self.image_width, self.image_height = int(width), int(height)
        self.image_name, self.znear, self.zfar = image_name, znear, zfar
        self.R, self.T = R, T
        self.trainable_cameras, self.trainable_intrinsics, self.use_barf = bank.trainable_cameras, bank.trainable_intrinsics, bank.use_barf
        self.original_image: Optional[torch.Tensor] = None
        self.original_mask: Optional[torch.Tensor] = None
        self.original_orient_angle: Optional[torch.Tensor] = None
        self.original_orient_conf: Optional[torch.Tensor] = None
        self._frozen = None   # (key, tensors) of the last evaluation without a graph

    _rotation_res = property(lambda self: self.bank.params[self.index, :self.bank.rot_dim])
    _translation_res = property(lambda self: self.bank.params[self.index, self.bank.rot_dim:self.bank.rot_dim + 3])
    _fov_res = property(lambda self: self.bank.params[self.index, self.bank.rot_dim + 3:])

    def tensors(self):
        """(world_view_transform, full_proj_transform, camera_center, FoVx, FoVy, projection_matrix).  While the bank trains
        (``CameraBank.live``) and autograd records, they carry the graph to the bank's gradient row; otherwise they are constants,
        re-used until the bank's parameters change (a constant FoV is read by the host once, not once per view)."""
        bank = self.bank
        if bank.live and bank.train_mask and torch.is_grad_enabled():
            if bank.fused:
                return _BankCompose.apply(bank._anchor, bank, self.index)
            return bank._compose_torch_row(self.index)
        key = (bank._version, bank.params._version)
        if self._frozen is None or self._frozen[0] != key:
            with torch.no_grad():
                out = bank._compose_rows(self.index, 1)[0] if bank.fused else None
                t = CameraBank._split(out) if bank.fused else bank._compose_torch_row(self.index, graph=False)
            self._frozen = (key, t)
        return self._frozen[1]

    world_view_transform = property(lambda self: self.tensors()[0])
    full_proj_transform = property(lambda self: self.tensors()[1])
    camera_center = property(lambda self: self.tensors()[2])
    FoVx = property(lambda self: self.tensors()[3])
    FoVy = property(lambda self: self.tensors()[4])
    projection_matrix = property(lambda self: self.tensors()[5])


class CameraBank:
    """The residuals of all N cameras of a scene in one flat device buffer, their Adam moments and per-camera step counts beside
    it (the reference keeps three nn.Parameters per camera and a torch.optim.Adam over 3 N tensors: src/scene/cameras.py:83-92,
    src/train_gaussians.py:45-66).  ``use_barf``: BARF's se(3) residual (the reference's default) or the ortho-6D rotation.
    ``trainable_cameras`` / ``trainable_intrinsics`` off leave the pose / the FoV group frozen: it composes (at its initial
    value, or whatever was loaded), gets no gradient and no update.

    ``cameras``: ``Camera`` objects (their R, T, FoV, size, name and ground-truth slots are taken over) or
    ``(R, T, FoVx, FoVy, width, height, image_name)`` records.  ``bank[i]`` is a ``BankCamera``.

    On a ROCm device (``fused``, the default there) ``bank[i].tensors()`` is one launch, its backward one launch that writes
    dL/d(residuals) into row i of ``bank.grads`` and raises the row's ``touched`` mark, and ``step()`` one launch over all rows;
    the host reads nothing back.  On CPU tensors, or with ``fused=False``, the same semantics in PyTorch ops."""

    BETAS, EPS = (0.9, 0.999), 1e-15

    def __init__(self, cameras, use_barf=True, trainable_cameras=True, trainable_intrinsics=True, device="cpu", fused=None,
                 trans=np.array([0.0, 0.0, 0.0]), scale=1.0):
        from .. import _lib
        dev = torch.device(device)
        self.device, self.use_barf = dev, bool(use_barf)
        self.trainable_cameras, self.trainable_intrinsics = bool(trainable_cameras), bool(trainable_intrinsics)
        self.fused = (dev.type == "cuda") if fused is None else bool(fused)
        if self.fused and dev.type != "cuda":
            raise ValueError("CameraBank(fused=True) needs a ROCm device: the kernels have no CPU form (use fused=False)")
        self.parametrisation = _lib.CAMERA_SE3 if self.use_barf else _lib.CAMERA_ORTHO6D
        self.rot_dim = 3 if self.use_barf else 6
        self.width = self.rot_dim + 5
        self.train_mask = (_lib.CAMERA_TRAIN_POSE if self.trainable_cameras else 0) | \
                          (_lib.CAMERA_TRAIN_FOV if self.trainable_intrinsics else 0)
        rows, self._cams = [], []
        for i, c in enumerate(cameras):
            if isinstance(c, (tuple, list)):
                R, T, fx, fy, w, h, name = c
                gt = {}
            else:
                R, T, fx, fy, w, h, name = c.R, c.T, float(c.FoVx), float(c.FoVy), c.image_width, c.image_height, c.image_name
                gt = {k: getattr(c, k, None) for k in ("original_image", "original_mask", "original_orient_angle", "original_orient_conf")}
            znear, zfar = 0.01, 100.0
            w2c = getWorld2View2(np.asarray(R), np.asarray(T), trans, scale)   # cameras.py:72
            # P[2][2], P[2][3] of getProjectionMatrix: Python doubles stored into an fp32 tensor (graphics_utils.py:69-70)
            rows.append(list(w2c.reshape(-1)) + [float(fx), float(fy), znear, zfar / (zfar - znear), -(zfar * znear) / (zfar - znear)])
            cam = BankCamera(self, i, w, h, name, np.asarray(R, dtype=np.float64), np.asarray(T, dtype=np.float64), znear, zfar)
            for k, v in gt.items():
                setattr(cam, k, v.to(dev) if isinstance(v, torch.Tensor) else v)
            self._cams.append(cam)
        N = len(rows)
        self.consts = torch.tensor(np.asarray(rows, dtype=np.float64).reshape(N, _lib.CAMERA_CONST), dtype=torch.float32, device=dev)
        init = torch.zeros(self.width)
        if not self.use_barf:
            init[:6] = torch.eye(3, 3)[:2].reshape(-1)
        self.params = init.repeat(N, 1).contiguous().to(dev)
        self.grads, self.exp_avg, self.exp_avg_sq = (torch.zeros(N, self.width, device=dev) for _ in range(3))
        self.steps = torch.zeros(N, dtype=torch.int32, device=dev)     # Adam step count of each camera
        self.touched = torch.zeros(N, dtype=torch.int32, device=dev)   # its gradient row holds this step's gradient
        self._anchor = torch.zeros((), device=dev, requires_grad=True)
        cols = torch.tensor([self.trainable_cameras] * (self.rot_dim + 3) + [self.trainable_intrinsics] * 2, device=dev)
        self._train_cols = cols
        self._version, self.live = 0, True
        self.opt = None
        self._lr = (0.0, 0.0, 0.0)
        self.replicated, self._group, self._message = False, None, None

    def __len__(self):
        return len(self._cams)

    def __getitem__(self, i) -> BankCamera:
        return self._cams[i]

    def __iter__(self):
        return iter(self._cams)

    # ---- compose ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _split(out):
        """one output row (include/ghr.h) -> the six tensors of ``tensors()``"""
        return (out[0:16].view(4, 4), out[16:32].view(4, 4), out[48:51], out[51], out[52], out[32:48].view(4, 4))

    def _check_rows(self, first, n):
        if first < 0 or n < 0 or first + n > len(self):
            raise IndexError("CameraBank: rows [%d, %d) of %d cameras" % (first, first + n, len(self)))

    def _compose_rows(self, first, n):
        from .. import _lib
        from ..diff_gaussian_rasterization import _ptr, _stream
        self._check_rows(first, n)
        out = torch.empty(n, _lib.CAMERA_OUT, device=self.device)
        _lib.check(_lib.lib().ghr_camera_compose(_stream(), self.parametrisation, len(self), int(first), int(n), _ptr(self.consts),
                                                 _lib.CAMERA_CONST, _ptr(self.params), self.width, _ptr(out), _lib.CAMERA_OUT))
        return out

    def _backward_rows(self, first, n, d_view, d_full, d_proj, d_center, d_fovx, d_fovy):
        from .. import _lib
        from ..diff_gaussian_rasterization import _stream
        self._check_rows(first, n)
        keep = [None if d is None else d.contiguous() for d in (d_view, d_full, d_proj, d_center, d_fovx, d_fovy)]
        for d, k in zip(keep, (16, 16, 16, 3, 1, 1)):
            if d is not None and (d.dtype != torch.float32 or d.numel() != n * k or d.device != self.device):
                raise ValueError("CameraBank: a cotangent is not %d fp32 values per camera on the bank's device" % k)
        ptrs = [None if d is None else ctypes.c_void_p(d.data_ptr()) for d in keep]
        _lib.check(_lib.lib().ghr_camera_compose_backward(
            _stream(), self.parametrisation, len(self), int(first), int(n), ctypes.c_void_p(self.consts.data_ptr()), _lib.CAMERA_CONST,
            ctypes.c_void_p(self.params.data_ptr()), self.width, *ptrs, ctypes.c_void_p(self.grads.data_ptr()), self.width,
            ctypes.c_void_p(self.touched.data_ptr()), self.train_mask))

    def _compose_torch_row(self, i, graph=True):
        rd = self.rot_dim
        p = self.params[i].detach().clone()
        if graph:
            p.requires_grad_(True)
            p.register_hook(lambda g, i=i: self._accumulate(i, g))
        return compose_camera_torch(self.use_barf, self.consts[i], p[:rd], p[rd:rd + 3], p[rd + 3:])

    @torch.no_grad()
    def _accumulate(self, i, g):
        """the PyTorch form of the backward kernel's last lines: assign to an untouched row, add to a touched one; frozen groups 0"""
        g = torch.where(self._train_cols, g, torch.zeros_like(g))
        self.grads[i] = torch.where(self.touched[i] != 0, self.grads[i] + g, g)
        self.touched[i] = 1

    @torch.no_grad()
    def compose_all(self):
        """All N cameras' tensors from one launch, without a graph: (world_view_transform [N,4,4], full_proj_transform [N,4,4],
        camera_center [N,3], FoVx [N], FoVy [N], projection_matrix [N,4,4]) -- for export and evaluation."""
        N = len(self)
        if self.fused:
            out = self._compose_rows(0, N)
            return (out[:, 0:16].view(N, 4, 4), out[:, 16:32].view(N, 4, 4), out[:, 48:51], out[:, 51], out[:, 52],
                    out[:, 32:48].view(N, 4, 4))
        rows = [self._compose_torch_row(i, graph=False) for i in range(N)]
        return tuple(torch.stack([r[k] for r in rows]) if N else torch.zeros(0, device=self.device) for k in range(6))

    # ---- the cameras' optimizer (src/train_gaussians.py:57-66,183-196) ------------------------------------------------------
    def training_setup(self, opt, spatial_lr_scale: float = 1.0):
        from ..utils.general_utils import get_expon_lr_func
        self.opt = opt
        self.iterations_cam = int(opt.iterations_cam)
        self._lr_rotation, self._lr_fov = float(opt.cam_rotation_lr), float(opt.cam_fov_lr)
        self._lr_translation = get_expon_lr_func(lr_init=opt.cam_translation_lr_init * spatial_lr_scale,
                                                 lr_final=opt.cam_translation_lr_final * spatial_lr_scale,
                                                 max_steps=opt.cam_lr_max_steps)
        return self

    def learning_rates(self, iteration):
        """(rotation, translation, fov) learning rates of ``iteration``: host floats, the translation's on its schedule"""
        return self._lr_rotation, float(self._lr_translation(iteration)), self._lr_fov

    @contextlib.contextmanager
    def step_scope(self, iteration=None):
        """The views of one training iteration (``trainer.training_step`` wraps them; a hand-written loop may):
        ``with bank.step_scope(iteration): render ...; loss.backward()``.  Inside, from ``opt.iterations_cam`` on, the cameras are
        constants (no graph: the views take the constant-camera path, no camera-gradient work for a ``step`` that no longer moves
        them); ``live`` is restored on the way out, so ``tensors()`` outside a scope always carries the graph.  If the body raises,
        what its backwards left in the gradient rows is dropped (``discard_gradients``).  ``iteration=None`` only does the latter."""
        if iteration is not None and self.opt is None:
            raise RuntimeError("CameraBank.training_setup(opt, spatial_lr_scale) has not been called")
        before = self.live
        if iteration is not None:
            self.live = iteration < self.iterations_cam
        try:
            yield self
        except BaseException:
            self.discard_gradients()
            raise
        finally:
            self.live = before

    @torch.no_grad()
    def discard_gradients(self):
        """Lowers every touched mark: the next backward into a row assigns it, ``step`` passes it by."""
        self.touched.zero_()

    def step(self, iteration, lrs=None):
        """One Adam step of every camera viewed since the last one, at ``iteration``'s learning rates (``lrs`` overrides them);
        nothing at ``iteration >= opt.iterations_cam``.  A NaN in a viewed camera's gradient skips the whole step; the viewed
        cameras' gradients and marks are cleared either way."""
        if self.opt is None:
            raise RuntimeError("CameraBank.training_setup(opt, spatial_lr_scale) has not been called")
        if iteration >= self.iterations_cam or not self.train_mask or not len(self):
            return  # (decided from the iteration and the configuration alone: every rank of a replicated bank returns alike)
        if self.replicated:
            self.exchange_gradients()
        lr = tuple(float(x) for x in (lrs if lrs is not None else self.learning_rates(iteration)))
        self._lr = lr
        if self.fused:
            from .. import _lib
            from ..diff_gaussian_rasterization import _stream
            vp = lambda t: ctypes.c_void_p(t.data_ptr())
            _lib.check(_lib.lib().ghr_camera_adam_step(_stream(), self.parametrisation, len(self), vp(self.params), vp(self.grads),
                                                       vp(self.exp_avg), vp(self.exp_avg_sq), self.width, vp(self.steps),
                                                       vp(self.touched), lr[0], lr[1], lr[2], self.BETAS[0], self.BETAS[1],
                                                       self.EPS, self.train_mask))
        else:
            self._step_torch(lr)
        self._version += 1

    @torch.no_grad()
    def _step_torch(self, lr):
        """k_cam_adam in PyTorch ops (no host decision either)"""
        rd, (b1, b2) = self.rot_dim, self.BETAS
        t, col = self.touched != 0, self._train_cols
        bad = (torch.isnan(self.grads) & t[:, None] & col[None]).any()
        upd = t & ~bad
        steps = self.steps + upd.to(torch.int32)
        sf = steps.clamp(min=1).double()
        bias1, b2s = 1.0 - b1 ** sf, torch.sqrt(1.0 - b2 ** sf).float()
        lrs = torch.tensor([lr[0]] * rd + [lr[1]] * 3 + [lr[2]] * 2, dtype=torch.float64, device=self.device)
        ss = (lrs[None] / bias1[:, None]).float()
        g = self.grads
        m = self.exp_avg + (g - self.exp_avg) * float(np.float32(1.0 - b1))
        v = self.exp_avg_sq * float(np.float32(b2)) + float(np.float32(1.0 - b2)) * g * g
        p = self.params - ss * (m / (torch.sqrt(v) / b2s[:, None] + self.EPS))
        sel = upd[:, None] & col[None]
        self.params.copy_(torch.where(sel, p, self.params))
        self.exp_avg.copy_(torch.where(sel, m, self.exp_avg))
        self.exp_avg_sq.copy_(torch.where(sel, v, self.exp_avg_sq))
        self.steps.copy_(steps)
        self.grads.copy_(torch.where(t[:, None], torch.zeros_like(g), g))
        self.touched.zero_()

    # ---- one bank on every rank (view-parallel training) ---------------------------------------------------------------------------
    def replicate(self, group=None):
        """Makes this bank one replica of a bank that every rank of ``group`` holds; returns ``self``.  One small object collective
        checks that all ranks hold the same number of cameras, parametrisation, ``train_mask`` and image names (``ValueError``
        otherwise); then rank 0's ``params``, ``exp_avg``, ``exp_avg_sq`` and ``steps`` are broadcast (DDP's rule).  From here on
        ``step()`` starts with ``exchange_gradients()`` and ``trainer.training_step(camera_bank=...)`` takes the bank on more than
        one rank.  Every rank then calls ``step()`` in every iteration, also a rank without a view."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("CameraBank.replicate: torch.distributed is not initialised")
        G = dist.get_world_size(group)
        mine = (len(self), self.parametrisation, self.train_mask, [c.image_name for c in self._cams])
        every = [None] * G
        dist.all_gather_object(every, mine, group=group)
        for r, other in enumerate(every):
            if other != every[0]:
                what = [n for n, a, b in zip(("number of cameras", "parametrisation", "train_mask", "image names"), other, every[0])
                        if a != b]
                raise ValueError("CameraBank.replicate: rank %d's bank differs from rank 0's in %s" % (r, ", ".join(what)))
        src = 0 if group is None else dist.get_global_rank(group, 0)
        with torch.no_grad():
            for t in (self.params, self.exp_avg, self.exp_avg_sq, self.steps):
                dist.broadcast(t, src=src, group=group)
        self.replicated, self._group, self._message = True, group, None
        self._version += 1
        return self

    @torch.no_grad()
    def exchange_gradients(self):
        """The gradient rows of all ranks of a replicated bank, merged into every replica's ``grads`` / ``touched``; a collective:
        every rank calls it (``step()`` does, first thing), also one whose views touched no row.

        *Pack*: ``[N, width + 1]``: a touched row is its gradient row followed by ``1.0``, an untouched row all zeros -- stale
        contents of ``grads``, a stale NaN included, never travel.  *Gather*: one ``all_gather_into_tensor`` to ``[G, N, width +
        1]`` (at most 48 B per camera and rank).  *Merge*: per row and column the ranks are walked in ascending order; the first
        touched rank's value is assigned, later touched ranks' values are added in that order; ``touched[row]`` becomes 1 if any
        rank touched the row; rows no rank touched are left exactly as they are.  Pack and merge are one launch each on a fused
        bank (``k_cam_pack``, ``k_cam_merge``), the same rule in PyTorch ops otherwise.

        Consequences: a row touched by exactly one rank arrives with that rank's bits, so the viewed cameras of a step from equal
        state equal a one-rank step over the same global views bit for bit.  The same camera viewed on two ranks is DEFINED as the
        sum in rank order (on one rank two views of one camera stay refused -- two streams would race for the row; across ranks
        there is no race).  ``step()``'s NaN rule sees the same rows on every rank, so all ranks skip or step alike, and replicas
        that were bit-identical stay so."""
        import torch.distributed as dist
        if not self.replicated:
            raise RuntimeError("CameraBank.exchange_gradients: the bank is not replicated (CameraBank.replicate)")
        N, W = len(self), self.width
        if N == 0:
            return
        G = dist.get_world_size(self._group)
        if self._message is None or self._message[1].shape[0] != G:
            self._message = (torch.empty(N, W + 1, device=self.params.device), torch.empty(G, N, W + 1, device=self.params.device))
        msg, gathered = self._message
        if self.fused:
            from .. import _lib
            from ..diff_gaussian_rasterization import _on_device, _stream
            vp = lambda t: ctypes.c_void_p(t.data_ptr())
            with _on_device(self.params.device):
                _lib.check(_lib.lib().ghr_camera_pack_row_message(_stream(), N, W, vp(self.grads), W, vp(self.touched), vp(msg)))
                dist.all_gather_into_tensor(gathered.view(-1), msg.view(-1), group=self._group)
                _lib.check(_lib.lib().ghr_camera_merge_ranks(_stream(), N, W, G, vp(gathered), vp(self.grads), W,
                                                             vp(self.touched)))
            return
        pack_row_message_torch(self.grads, self.touched, msg)
        dist.all_gather_into_tensor(gathered.view(-1), msg.view(-1), group=self._group)
        merge_ranks_torch(gathered, self.grads, self.touched)

    # ---- persistence --------------------------------------------------------------------------------------------------------
    def state_dict(self):
        return {"use_barf": self.use_barf, "image_names": [c.image_name for c in self._cams],
                "params": self.params.detach().clone(), "exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(),
                "steps": self.steps.clone()}

    @torch.no_grad()
    def load_state_dict(self, sd):
        if bool(sd["use_barf"]) != self.use_barf or tuple(sd["params"].shape) != tuple(self.params.shape):
            raise ValueError("CameraBank.load_state_dict: another parametrisation or number of cameras")
        if list(sd["image_names"]) != [c.image_name for c in self._cams]:
            raise ValueError("CameraBank.load_state_dict: the cameras' image names differ")
        for k in ("params", "exp_avg", "exp_avg_sq", "steps"):
            getattr(self, k).copy_(sd[k].to(self.device))
        self.grads.zero_()
        self.touched.zero_()
        self._version += 1

    @torch.no_grad()
    def reference_pickles(self):
        """What the reference's loop dumps at a checkpoint (src/train_gaussians.py:203-208): ``((params_cam_rotation,
        params_cam_translation, params_cam_fov), projection_all)`` -- dicts image_name -> tensor (CPU copies; the residual dicts of
        a frozen group are empty, as there), the matrices from one ``compose_all()``."""
        rd, P = self.rot_dim, self.params.detach().cpu()
        names = [c.image_name for c in self._cams]
        rot = {n: P[i, :rd].clone() for i, n in enumerate(names)} if self.trainable_cameras else {}
        tra = {n: P[i, rd:rd + 3].clone() for i, n in enumerate(names)} if self.trainable_cameras else {}
        fov = {n: P[i, rd + 3:].clone() for i, n in enumerate(names)} if self.trainable_intrinsics else {}
        full = self.compose_all()[1].cpu()
        return (rot, tra, fov), {n: full[i].clone() for i, n in enumerate(names)}

    @torch.no_grad()
    def load_reference_pickles(self, dicts):
        """Takes the three dicts of a reference ``cameras/<iteration>.pkl`` (every camera of the bank must be in each non-empty
        one; the moments and step counts are left alone, as the reference's restart leaves them at zero)."""
        rd = self.rot_dim
        for d, lo, hi in zip(dicts, (0, rd, rd + 3), (rd, rd + 3, rd + 5)):
            if not d:
                continue
            for i, c in enumerate(self._cams):
                v = torch.as_tensor(d[c.image_name]).detach().reshape(-1).to(device=self.device, dtype=torch.float32)
                if v.numel() != hi - lo:
                    raise ValueError("CameraBank.load_reference_pickles: %s has %d values, the bank's parametrisation %d" %
                                     (c.image_name, v.numel(), hi - lo))
                self.params[i, lo:hi] = v
        self._version += 1


def make_camera(width, height, fovy_deg=40.0, distance=4.0, device="cpu") -> Camera:
    """camera at (0,0,-distance) looking down +z; FoVx from the aspect ratio."""
    fovy = math.radians(fovy_deg)
    fovx = 2 * math.atan(math.tan(fovy / 2) * width / height)
    return Camera(np.eye(3), np.array([0.0, 0.0, distance]), fovx, fovy, width, height, device=device)


def ring_cameras(n, width, height, radius=4.0, fovy_deg=40.0, device="cpu", roll_deg=0.0, cls=None):
    """SURVEY.md 8(d) cfg 4: azimuth 360*k/n, elevation 10*sin(2*pi*k/n) degrees, looking at the origin.
    ``roll_deg`` turns every camera about its own viewing axis (COLMAP poses are never upright: the parity tests use it
    so that all nine entries of the view rotation are non-trivial)."""
    cams = []
    fovy = math.radians(fovy_deg)
    fovx = 2 * math.atan(math.tan(fovy / 2) * width / height)
    for k in range(n):
        az, el = 2 * math.pi * k / n, math.radians(10.0) * math.sin(2 * math.pi * k / n)
        c = radius * np.array([math.cos(el) * math.sin(az), math.sin(el), -math.cos(el) * math.cos(az)])
        fwd = -c / np.linalg.norm(c)
        right = np.cross(np.array([0.0, 1.0, 0.0]), fwd)
        right /= np.linalg.norm(right)
        up = np.cross(fwd, right)
        if roll_deg:
            cr, sr = math.cos(math.radians(roll_deg)), math.sin(math.radians(roll_deg))
            right, up = cr * right + sr * up, -sr * right + cr * up
        R_c2w = np.stack([right, up, fwd], axis=1)  # columns = camera axes in world
        T = -R_c2w.T @ c
        cams.append((cls or Camera)(R_c2w, T, fovx, fovy, width, height, device=device, image_name="ring%03d" % k))
    return cams


def interpolate_poses(frames, R, T, fovx, fovy, speed_up: int = 4, max_frames: int = 300, frame_offset: int = 0) -> dict:
    """The camera path of ``readColmapSceneInfo(interpolate_cameras=True)`` (``src/scene/dataset_readers.py:160-193``) as arrays.
    ``frames [k]``: the key cameras' frame numbers, strictly increasing, at least two; ``R [k, 3, 3]`` (the transposed rotation, as
    ``Camera.R`` keeps it), ``T [k, 3]``, ``fovx [k]``, ``fovy [k]``.  Every integer ``i`` of ``[frames[0], frames[-1])`` gets a
    pose: the rotation from scipy's ``RotationSpline`` over the frame numbers; ``T`` and the two FoVs blended between the
    neighbouring keys ``j`` and ``j + 1`` as ``alpha * prev + (1 - alpha) * next`` with ``alpha = 1 - (i - frames[j]) / (frames[j
    + 1] - frames[j])``.  Of that list every ``speed_up``-th entry is kept and then ``[frame_offset : frame_offset + max_frames]``.
    Returns float64 arrays ``frame [n]``, ``R [n, 3, 3]``, ``T [n, 3]``, ``fovx [n]``, ``fovy [n]`` and ``key [n]`` (the ``j``)."""
    from scipy.spatial.transform import Rotation, RotationSpline
    f = np.asarray(frames)
    if f.ndim != 1 or f.shape[0] < 2:
        raise ValueError("interpolate_poses: at least two key cameras are needed, got %s" % (f.shape,))
    if not np.all(f == np.round(f)):
        raise ValueError("interpolate_poses: frame numbers must be integers")
    f = f.astype(np.int64)
    if not np.all(np.diff(f) > 0):
        raise ValueError("interpolate_poses: frame numbers must be strictly increasing, got %s" % (f.tolist(),))
    k = f.shape[0]
    R = np.asarray(R, np.float64).reshape(k, 3, 3)
    T = np.asarray(T, np.float64).reshape(k, 3)
    fovx, fovy = np.asarray(fovx, np.float64).reshape(k), np.asarray(fovy, np.float64).reshape(k)
    if int(speed_up) < 1 or int(max_frames) < 0 or int(frame_offset) < 0:
        raise ValueError("interpolate_poses: speed_up >= 1, max_frames >= 0 and frame_offset >= 0 are needed")
    i = np.arange(f[0], f[-1], dtype=np.int64)
    R_i = RotationSpline(f.astype(np.float64), Rotation.from_matrix(R))(i.astype(np.float64)).as_matrix()
    j = np.searchsorted(f, i, side="right") - 1          # the last key at or before frame i
    alpha = 1 - (i - f[j]) / (f[j + 1] - f[j])
    blend = lambda v: (v[j].T * alpha + v[j + 1].T * (1 - alpha)).T   # noqa: E731
    take = slice(None, None, int(speed_up))
    cut = slice(int(frame_offset), int(frame_offset) + int(max_frames))
    pick = lambda v: np.ascontiguousarray(v[take][cut], np.float64)   # noqa: E731
    return dict(frame=pick(i), R=pick(R_i), T=pick(blend(T)), fovx=pick(blend(fovx)), fovy=pick(blend(fovy)), key=pick(j))


def interpolated_cameras(keys, speed_up: int = 4, max_frames: int = 300, frame_offset: int = 0, device="cpu", znear=0.01,
                         zfar=100.0) -> list:
    """``Camera``s along the path ``interpolate_poses`` makes of the key cameras ``keys``: objects with ``R``, ``T`` (numpy, as
    ``Camera`` keeps them), ``FoVx``, ``FoVy`` (a float or a 0-d tensor), ``image_width``, ``image_height`` and ``image_name``, a
    string with ``int(image_name)`` the frame number.  The keys are sorted by ``image_name`` as strings, as the reference sorts
    them; a path camera has the size of the key before it and ``image_name = '%06d' % frame``.  What the reference's ``CameraInfo``
    carries besides -- the blended ``uid``, ``image`` and ``image_path`` -- has no counterpart in ``Camera`` and is not reproduced."""
    keys = sorted(keys, key=lambda c: c.image_name)
    if len(keys) < 2:
        raise ValueError("interpolated_cameras: at least two key cameras are needed, got %d" % len(keys))
    p = interpolate_poses([int(c.image_name) for c in keys], np.stack([np.asarray(c.R, np.float64) for c in keys]),
                          np.stack([np.asarray(c.T, np.float64).reshape(3) for c in keys]), [float(c.FoVx) for c in keys],
                          [float(c.FoVy) for c in keys], speed_up, max_frames, frame_offset)
    cams = []
    for n in range(p["frame"].shape[0]):
        key = keys[int(p["key"][n])]
        cams.append(Camera(p["R"][n], p["T"][n], p["fovx"][n], p["fovy"][n], key.image_width, key.image_height, znear=znear,
                           zfar=zfar, device=device, image_name="%06d" % int(p["frame"][n])))
    return cams


PARITY_CAMERAS = ("front", "ring5", "ring13roll")


def parity_camera(name, width, height, device="cpu") -> Camera:
    """The cameras every oracle- / reference-pinned parity test runs: the SURVEY front camera (identity rotation), view 5
    of BASELINE configs[3]'s 32-camera ring (azimuth 56 deg: a rotation about y plus a small pitch), and view 13 of that
    ring rolled by 20 deg about its viewing axis (a full 3x3 rotation, as world_view_transform built from COLMAP poses is
    in the reference: src/scene/cameras.py:72-80).  With R = I a transposed W in computeCov2D (forward.cu:74-113,
    backward.cu:144-274) or in the model's T = W J would be invisible."""
    if name == "front":
        return make_camera(width, height, device=device)
    if name == "ring5":
        return ring_cameras(32, width, height, device=device)[5]
    if name == "ring13roll":
        return ring_cameras(32, width, height, device=device, roll_deg=20.0)[13]
    raise KeyError(name)
