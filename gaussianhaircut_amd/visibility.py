"""Which vertices of the head mesh do the training views see (csrc/ghr_visibility.h): the rasterizer and the
counts of ``src/preprocessing/extract_non_visible_head_scalp.py`` -- the step between the stages that decides which scalp
vertices hair may grow from.

``rasterize_mesh`` gives ``pix_to_face`` of one view, ``vertex_visibility`` the per-vertex counts over many views and each view's
``vis`` plane, ``visible_vertex_mask`` the script's threshold.  ``fused=True`` launches the HIP kernels (ROCm tensors only: there
is no CPU path); ``fused=False`` evaluates the PyTorch-composed comparator on any device: the same float32 expressions in the same
operand order, brute force over all faces in pixel chunks -- the tile lists change which faces a pixel looks at, never the winner.

The definition (pixel centres at +0.5, exact complementary edge predicates, largest inverse depth, lower face index among
equals) is this package's own and is stated at the top of ``csrc/ghr_visibility.h``; away from silhouettes and depth ties it agrees
with every sound rasterizer, pytorch3d's included.  A view is ``(M, H, W)`` with ``M`` the row-major 3 x 4 matrix that takes a
world point to ``(x w, y w, w)`` in pixels.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib

NEAR = 1e-3


# ---------------------------------------------------------------------------------------------------------------- views
def view_matrix(K, R, t) -> np.ndarray:
    """``K [R | t]`` as float32 [12] for OpenCV-style intrinsics ``K`` (3 x 3, in the convention in which pixel (i, j) covers
    [j, j + 1) x [i, i + 1): its centre is sampled at +0.5) and world-to-camera ``R``, ``t``.  Formed in float64, rounded once."""
    K, R, t = np.asarray(K, np.float64).reshape(3, 3), np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    return np.ascontiguousarray((K @ np.concatenate([R, t[:, None]], axis=1)).astype(np.float32).reshape(12))


def view_matrix_from_camera(cam):
    """(M, H, W) of one of this package's cameras: ``world_view_transform`` (stored transposed), the FoVs and the image size.  The
    Gaussian rasterizer's pixel k sits at NDC (2 k + 1) / S - 1, which is k + 0.5 here: fx = W / (2 tan(FoVx / 2)), cx = W / 2."""
    W, H = int(cam.image_width), int(cam.image_height)
    w2c = cam.world_view_transform.detach().double().cpu().numpy().T
    K = np.array([[W / (2.0 * np.tan(float(cam.FoVx) / 2.0)), 0.0, W / 2.0],
                  [0.0, H / (2.0 * np.tan(float(cam.FoVy) / 2.0)), H / 2.0],
                  [0.0, 0.0, 1.0]])
    return view_matrix(K, w2c[:3, :3], w2c[:3, 3]), H, W


def _rq3(A):
    """A = K R with K upper triangular with a positive diagonal and R orthogonal (numpy's QR of the reversed matrix)."""
    Q, U = np.linalg.qr(np.flipud(A).T)
    K, R = np.fliplr(np.flipud(U.T)), np.flipud(Q.T)
    D = np.diag(np.where(np.diag(K) < 0, -1.0, 1.0))
    return K @ D, D @ R


def decompose_projection(P):
    """P (3 x 4) -> (K, R, t) with K[2, 2] = 1, det R = +1 and K [R | t] proportional to P (checked)."""
    P = np.asarray(P, np.float64).reshape(3, 4)
    if not np.isfinite(P).all():
        raise ValueError("decompose_projection: P is not finite")
    K, R = _rq3(P[:, :3])
    sign = 1.0
    if np.linalg.det(R) < 0:
        R, sign = -R, -1.0
    if not (np.abs(np.diag(K)) > 1e-12 * np.abs(K).max()).all():
        raise ValueError("decompose_projection: K [R | t] does not reproduce P (its left 3 x 3 block is singular)")
    t = sign * np.linalg.solve(K, P[:, 3])
    back = sign * (K @ np.concatenate([R, t[:, None]], axis=1))
    if not np.allclose(back, P, rtol=1e-9, atol=1e-9 * np.abs(P).max()):
        raise ValueError("decompose_projection: K [R | t] does not reproduce P")
    return K / K[2, 2], R, t


def views_from_projections(P_by_name, size_by_name) -> dict:
    """name -> (M, H, W) from the script's cameras pickle (its lines 116-150): every 3 x 4 projection is decomposed into K, R, t;
    fx, fy, cx, cy are halved, 0.5 is added to cx and cy, and the rows are scaled by the image's (W, H) -- the pickle's
    intrinsics are in units of half the image, with pixel centres at the integers.  ``size_by_name``: name -> (H, W)."""
    out = {}
    for name, P in P_by_name.items():
        P = np.asarray(P.detach().cpu().numpy() if isinstance(P, torch.Tensor) else P, np.float64)
        K, R, t = decompose_projection(P[:3, :4])
        H, W = (int(x) for x in size_by_name[name])
        K = K.copy()
        K[0, 0] /= 2; K[1, 1] /= 2; K[0, 2] /= 2; K[1, 2] /= 2
        K[0, 2] += 0.5; K[1, 2] += 0.5
        K[0] *= W; K[1] *= H
        out[name] = (view_matrix(K, R, t), H, W)
    return out


# ---------------------------------------------------------------------------------------------------------------- helpers
def _mesh_arrays(mesh):
    v, f = (mesh.vertices, mesh.faces) if hasattr(mesh, "vertices") else mesh
    v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    f = f.detach().cpu().numpy() if isinstance(f, torch.Tensor) else np.asarray(f)
    return np.array(v, np.float32).reshape(-1, 3), np.array(f, np.int32).reshape(-1, 3)  # (copies: torch wants them writable)


def _plane(x, H, W, device):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x))
    assert t.dtype == torch.uint8 and tuple(t.shape) == (H, W), (t.dtype, tuple(t.shape), (H, W))
    return t.to(device).contiguous()


def _device(device, fused):
    return torch.device(device if device is not None else ("cuda:0" if fused else "cpu"))


def vis_workspace_bytes(V: int, Fc: int, H: int, W: int) -> int:
    b = ctypes.c_size_t(0)
    _lib.check(_lib.lib().ghr_vis_sizes(int(V), int(Fc), int(H), int(W), ctypes.byref(b)))
    return int(b.value)


# ---------------------------------------------------------------------------------------------------------------- composed
def head_mask_torch(body, hair):
    """bool [H, W]: (max5x5(body) >= 128) and not (max5x5(hair) >= 128); max_pool2d pads with -inf, i.e. clips the window."""
    if body.numel() == 0:
        return torch.zeros(body.shape, dtype=torch.bool, device=body.device)
    mb = F.max_pool2d(body[None, None].float(), 5, stride=1, padding=2)[0, 0]
    mh = F.max_pool2d(hair[None, None].float(), 5, stride=1, padding=2)[0, 0]
    return (mb >= 128) & ~(mh >= 128)


def _rasterize_torch(v, f, M, H, W, near, chunk_elems: int = 1 << 22):
    """pix_to_face [H, W] int32 of the definition, brute force; v [V, 3] float32 and f [F, 3] int64 tensors on one device."""
    dev = v.device
    out = torch.full((H * W,), -1, dtype=torch.int32, device=dev)
    V, Fc = v.shape[0], f.shape[0]
    if H * W == 0 or Fc == 0 or V == 0:
        return out.reshape(H, W)
    m = [float(x) for x in np.asarray(M, np.float32).reshape(12)]
    nr = float(np.float32(near))
    X = [v[:, c] for c in range(3)]
    xp = (m[0] * X[0] + m[1] * X[1]) + (m[2] * X[2] + m[3])
    yp = (m[4] * X[0] + m[5] * X[1]) + (m[6] * X[2] + m[7])
    w = (m[8] * X[0] + m[9] * X[1]) + (m[10] * X[2] + m[11])
    sx, sy, q = xp / w, yp / w, torch.ones_like(w) / w   # (a division, not reciprocal(): correctly rounded)
    valid = torch.isfinite(w) & (w > nr)
    in_range = ((f >= 0) & (f < V)).all(dim=1)
    fi = torch.where(in_range[:, None], f, torch.zeros_like(f))
    u = [sx[fi[:, k]] for k in range(3)]
    t = [sy[fi[:, k]] for k in range(3)]
    qq = [q[fi[:, k]] for k in range(3)]
    never = ~in_range | (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])
    never = never | ~(valid[fi[:, 0]] & valid[fi[:, 1]] & valid[fi[:, 2]])
    never = never | ((u[1] - u[0]) * (t[2] - t[0]) - (t[1] - t[0]) * (u[2] - u[0]) == 0)  # mesh_flat
    ulo, uhi = torch.fmin(torch.fmin(u[0], u[1]), u[2]), torch.fmax(torch.fmax(u[0], u[1]), u[2])
    vlo, vhi = torch.fmin(torch.fmin(t[0], t[1]), t[2]), torch.fmax(torch.fmax(t[0], t[1]), t[2])
    flips = [f[:, k] > f[:, (k + 1) % 3] for k in range(3)]
    face_id = torch.arange(Fc, device=dev)
    neg_inf = torch.tensor(float("-inf"), dtype=torch.float32, device=dev)
    chunk = max(1, chunk_elems // Fc)
    for s in range(0, H * W, chunk):
        p = torch.arange(s, min(s + chunk, H * W), device=dev)
        px = ((p % W).float() + 0.5)[:, None]
        py = ((p // W).float() + 0.5)[:, None]
        side, e = [], []
        for k in range(3):
            k1 = (k + 1) % 3
            flip = flips[k]
            au, av = torch.where(flip, u[k1], u[k]), torch.where(flip, t[k1], t[k])
            bu, bv = torch.where(flip, u[k], u[k1]), torch.where(flip, t[k], t[k1])
            dx, dy = bu - au, bv - av
            E = dx * (py - av) - dy * (px - au)
            left = (E > 0) | ((E == 0) & ((dy < 0) | ((dy == 0) & (dx > 0))))
            side.append(left != flip)
            e.append(torch.where(flip, -E, E))
        d = ((e[1] * qq[0] + e[2] * qq[1]) + e[0] * qq[2]) / ((e[0] + e[1]) + e[2])
        in_box = (px >= ulo) & (px <= uhi) & (py >= vlo) & (py <= vhi)
        covers = ~never & in_box & (side[0] == side[1]) & (side[1] == side[2]) & ~torch.isnan(d)
        d = torch.where(covers, d, neg_inf)
        dmax = d.max(dim=1).values
        first = torch.where(d == dmax[:, None], face_id, Fc).min(dim=1).values   # the lowest index among the equals
        out[p] = torch.where(dmax > neg_inf, first, -1).to(torch.int32)
    return out.reshape(H, W)


def _view_torch(v, f, M, H, W, near, body, hair, cnt, cnt_head):
    pix = _rasterize_torch(v, f, M, H, W, near)
    head = head_mask_torch(body, hair) if body is not None else torch.zeros((H, W), dtype=torch.bool, device=v.device)
    won = pix >= 0
    vis = torch.where(won & head, 255, 0).to(torch.uint8)
    for sel, acc in ((won, cnt), (won & head, cnt_head)):
        if acc is not None and bool(sel.any()):
            acc[torch.unique(f[torch.unique(pix[sel]).long()])] += 1
    return pix, vis


# ---------------------------------------------------------------------------------------------------------------- fused
def _view_fused(v, f32, M, H, W, near, body, hair, ws, cnt, cnt_head):
    from .diff_gaussian_rasterization import _on_device, _ptr, _stream
    dev = v.device
    pix = torch.empty((H, W), dtype=torch.int32, device=dev)
    vis = torch.empty((H, W), dtype=torch.uint8, device=dev)
    Mc = (ctypes.c_float * 12)(*[float(x) for x in np.asarray(M, np.float32).reshape(12)])
    with _on_device(dev):
        _lib.check(_lib.lib().ghr_vis_view(_stream(), v.shape[0], _ptr(v) if v.shape[0] else None, f32.shape[0],
                                           _ptr(f32) if f32.shape[0] else None, ctypes.byref(Mc), float(near), H, W,
                                           _ptr(body) if body is not None else None, _ptr(hair) if hair is not None else None,
                                           _ptr(ws), _ptr(pix) if H * W else None, _ptr(vis) if H * W else None,
                                           _ptr(cnt) if cnt is not None else None, _ptr(cnt_head) if cnt_head is not None else None))
    return pix, vis


# ---------------------------------------------------------------------------------------------------------------- public
@torch.no_grad()
def vertex_visibility(mesh, views, masks=None, fused: bool = True, near: float = NEAR, device=None):
    """``views``: a sequence of (M, H, W); ``masks``: a sequence of (body, hair) uint8 [H, W] planes (or None: no head mask, as
    for every entry that is None).  Returns (cnt [V] int32: the views that see each vertex, cnt_head [V] int32: those that see it
    through the head mask, the list of the views' ``vis`` planes, uint8 [H, W]: 255 where the mesh shows through the head)."""
    dev = _device(device, fused)
    if fused and dev.type != "cuda":
        raise RuntimeError("vertex_visibility(fused=True) needs a ROCm device: the kernels have no CPU path (fused=False is the "
                           "PyTorch form)")
    va, fa = _mesh_arrays(mesh)
    v = torch.from_numpy(va).to(dev)
    f32 = torch.from_numpy(fa).to(dev)
    cnt = torch.zeros(len(va), dtype=torch.int32, device=dev)
    cnt_head = torch.zeros(len(va), dtype=torch.int32, device=dev)
    views = list(views)
    masks = [None] * len(views) if masks is None else list(masks)
    assert len(masks) == len(views), (len(masks), len(views))
    planes = []
    if fused:
        Hm, Wm = max([int(h) for _, h, _ in views] + [0]), max([int(w) for _, _, w in views] + [0])
        ws = torch.empty(vis_workspace_bytes(len(va), len(fa), Hm, Wm), dtype=torch.uint8, device=dev)
    else:
        f64 = f32.long()
    for (M, H, W), mk in zip(views, masks):
        H, W = int(H), int(W)
        body, hair = (None, None) if mk is None else (_plane(mk[0], H, W, dev), _plane(mk[1], H, W, dev))
        if fused:
            _, vis = _view_fused(v, f32, M, H, W, near, body, hair, ws, cnt, cnt_head)
        else:
            _, vis = _view_torch(v, f64, M, H, W, near, body, hair, cnt, cnt_head)
        planes.append(vis)
    return cnt, cnt_head, planes


@torch.no_grad()
def rasterize_mesh(mesh, M, H, W, near: float = NEAR, fused: bool = True, device=None):
    """pix_to_face [H, W] int32 of ``mesh`` (a HeadMesh or (vertices, faces)) under the view (M, H, W): the winning face of every
    pixel, -1 where there is none."""
    dev = _device(device, fused)
    if fused and dev.type != "cuda":
        raise RuntimeError("rasterize_mesh(fused=True) needs a ROCm device: the kernels have no CPU path (fused=False is the "
                           "PyTorch form)")
    va, fa = _mesh_arrays(mesh)
    v, f32 = torch.from_numpy(va).to(dev), torch.from_numpy(fa).to(dev)
    H, W = int(H), int(W)
    if not fused:
        return _rasterize_torch(v, f32.long(), M, H, W, near)
    ws = torch.empty(vis_workspace_bytes(len(va), len(fa), H, W), dtype=torch.uint8, device=dev)
    return _view_fused(v, f32, M, H, W, near, None, None, ws, None, None)[0]


@torch.no_grad()
def head_mask(body, hair, fused: bool = True):
    """bool [H, W] from two uint8 planes on one device."""
    if not fused:
        return head_mask_torch(body, hair)
    if not body.is_cuda:
        raise RuntimeError("head_mask(fused=True) needs tensors on a ROCm device: the kernel has no CPU path")
    from .diff_gaussian_rasterization import _on_device, _ptr, _stream
    H, W = body.shape
    body, hair = body.contiguous(), hair.contiguous()
    out = torch.empty((H, W), dtype=torch.uint8, device=body.device)
    with _on_device(body.device):
        _lib.check(_lib.lib().ghr_vis_head_mask(_stream(), H, W, _ptr(body), _ptr(hair), _ptr(out)))
    return out.bool()


def visible_vertex_mask(cnt, cnt_head, n_views: int, prob_thr: float = 0.5, n_views_thr: float = 0.1):
    """The script's lines 89-91 in float32: ``(1 - cnt_head / cnt > prob_thr) or (cnt / n_views < n_views_thr)``; 0 / 0 is NaN
    and compares false in the first term (such a vertex is still marked by the second)."""
    c, ch = torch.as_tensor(cnt).float(), torch.as_tensor(cnt_head).float()
    return torch.logical_or(1 - ch / c > prob_thr, c / n_views < n_views_thr)
