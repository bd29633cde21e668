"""The strand stage's prior term (src/scene/gaussian_model_strands.py:456-515, src/train_strands.py:139-147).

Every iteration of the reference's third stage draws 1000 guiding strands, takes them into their scalp-local frames, encodes
them, blends a ``[1, 64, G, G]`` latent texture from each texel's four nearest guiding strands by HAAR's cosine-similarity rule
and asks a diffusion model for a loss on it.  The two networks are the caller's callables here (``encoder``, ``prior_loss``);
what lies between them is HIP (csrc/ghr_sds.h): ``guiding_strands_local`` and ``latent_texture`` are autograd functions on ROCm
tensors, one launch each way for the local frame, three each way for the texture.  ``fused=False`` is the PyTorch-composed
comparator -- the same float32 expressions, a STABLE sort so that it shares the tie rule (among equal distances the lower
guiding index first) -- and the only form for CPU tensors.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch
import torch.nn.functional as F

from . import _lib

K = 4
DIST_EPS = 1e-7
CSIM_KNEE = 0.9


def _use_fused(fused, t) -> bool:
    if fused is None:
        return bool(t.is_cuda)
    if fused and not t.is_cuda:
        raise RuntimeError("strand_prior: the HIP form has no CPU path (fused=False is the composed form)")
    return bool(fused)


def _check_sizes(N: int, G: Optional[int]):
    if N < K:
        raise ValueError("N = %d guiding strands: a texel needs %d" % (N, K))
    if G is not None and G * G < N:
        raise ValueError("G * G = %d < N = %d: guiding strand g takes its blending coefficient from texel number g" % (G * G, N))


def inverse3(m: torch.Tensor) -> torch.Tensor:
    """[..., 3, 3] inverse as adjugate over determinant, the expressions of ``sds_inv3`` (csrc/ghr_sds.h)."""
    a = [m[..., i // 3, i % 3] for i in range(9)]
    c00, c01, c02 = a[4] * a[8] - a[5] * a[7], a[5] * a[6] - a[3] * a[8], a[3] * a[7] - a[4] * a[6]
    r = 1.0 / ((a[0] * c00 + a[1] * c01) + a[2] * c02)
    rows = [c00 * r, (a[2] * a[7] - a[1] * a[8]) * r, (a[1] * a[5] - a[2] * a[4]) * r,
            c01 * r, (a[0] * a[8] - a[2] * a[6]) * r, (a[2] * a[3] - a[0] * a[5]) * r,
            c02 * r, (a[1] * a[6] - a[0] * a[7]) * r, (a[0] * a[4] - a[1] * a[3]) * r]
    return torch.stack(rows, dim=-1).reshape(m.shape)


def texel_centres(G: int, device, dtype=torch.float32) -> torch.Tensor:
    """[G]: the midpoints of ``linspace(-1, 1, G + 1)``, formed on ``device`` as the reference forms them."""
    grid = torch.linspace(start=-1, end=1, steps=int(G) + 1, device=device, dtype=dtype)
    return (grid[1:] + grid[:-1]) / 2


_CENTRES = {}


def _centres_cached(G: int, device) -> torch.Tensor:
    key = (int(G), str(device))
    if key not in _CENTRES:
        _CENTRES[key] = texel_centres(G, device).contiguous()
    return _CENTRES[key]


# ---- step 1: the local frame ------------------------------------------------------------------------------------------------------
def _local_composed(dirs, frames, idx, scale, frames_are_inverse):
    M = frames[idx] if frames_are_inverse else inverse3(frames[idx])
    d = dirs[idx]
    P = torch.cat([torch.zeros_like(d[:, :1]), torch.cumsum(d, dim=1)], dim=1)
    e = (M[:, None] @ P[..., None])[..., 0] * scale
    v = (M[:, None] @ d[..., None])[..., 0] * scale
    return e, v


class _GuidingLocal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dirs, frames, idx, scale, frames_are_inverse):
        from .diff_gaussian_rasterization import _on_device, _ptr, _stream
        S, n = int(dirs.shape[0]), int(dirs.shape[1])
        N = int(idx.shape[0])
        e = torch.empty((N, n + 1, 3), dtype=torch.float32, device=dirs.device)
        v = torch.empty((N, n, 3), dtype=torch.float32, device=dirs.device)
        with _on_device(dirs.device):
            _lib.check(_lib.lib().ghr_sds_local(_stream(), S, N, n, _ptr(dirs), _ptr(frames), int(frames_are_inverse), _ptr(idx),
                                                float(scale), _ptr(e), _ptr(v)))
        ctx.save_for_backward(frames, idx)
        ctx.meta = (S, N, n, float(scale), int(frames_are_inverse))
        ctx.set_materialize_grads(False)
        return e, v

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_e, d_v):
        from .diff_gaussian_rasterization import _on_device, _ptr, _stream
        if not ctx.needs_input_grad[0] or (d_e is None and d_v is None):
            return None, None, None, None, None
        frames, idx = ctx.saved_tensors
        S, N, n, scale, inv = ctx.meta
        d_e = None if d_e is None else d_e.contiguous().float()
        d_v = None if d_v is None else d_v.contiguous().float()
        # strands drawn more than once: a stable sort groups them with their guiding indices ascending (plumbing; the sums are
        # the kernel's).  The dense zero-filled result is what autograd adds to the rasterizer's gradient of the same parameter.
        sorted_idx, order = torch.sort(idx, stable=True)
        d_dirs = torch.zeros((S, n, 3), dtype=torch.float32, device=frames.device)
        with _on_device(frames.device):
            _lib.check(_lib.lib().ghr_sds_local_backward(_stream(), S, N, n, _ptr(frames), inv, _ptr(sorted_idx), _ptr(order), scale,
                                                         None if d_e is None else _ptr(d_e), None if d_v is None else _ptr(d_v),
                                                         _ptr(d_dirs)))
        return d_dirs, None, None, None, None


def guiding_strands_local(dirs, local2world, idx, scale_decoder, fused=None, frames_are_inverse: bool = False):
    """``(e [N, n + 1, 3], v [N, n, 3])``: the guiding strands ``idx`` of ``dirs [S, n, 3]`` in their scalp-local frames, scaled:
    ``e[g, j] = local2world[idx[g]]^-1 (sum_{i < j} dirs[idx[g], i]) scale`` (the encoder's input), ``v`` the same of the segments.
    Computed from ``dirs`` directly -- the reference subtracts the origins from the points it added them to, which costs bits.
    ``frames_are_inverse``: ``local2world`` holds the inverses already (``StrandPrior`` inverts once, in float64)."""
    if dirs.dim() != 3 or dirs.shape[-1] != 3 or dirs.shape[1] < 1:
        raise ValueError("dirs must be [S, n, 3] with n >= 1")
    S = int(dirs.shape[0])
    if tuple(local2world.shape) != (S, 3, 3):
        raise ValueError("local2world must be [S, 3, 3]")
    if idx.dim() != 1 or idx.dtype != torch.int64:
        raise ValueError("idx must be a 1-D int64 tensor")
    _check_sizes(int(idx.shape[0]), None)
    if not _use_fused(fused, dirs):
        return _local_composed(dirs, local2world, idx, scale_decoder, frames_are_inverse)
    if dirs.dtype != torch.float32:
        raise RuntimeError("strand_prior: the HIP form takes float32")
    return _GuidingLocal.apply(dirs.contiguous(), local2world.detach().float().contiguous(), idx.contiguous(), float(scale_decoder),
                               bool(frames_are_inverse))


# ---- step 3: the texture ------------------------------------------------------------------------------------------------------------
def neighbours_composed(uvs_gdn, G: int):
    """``(nbr [G G, 4] int64, w [G G, 4])``: each texel's four nearest guiding strands under a STABLE sort of the squared UV
    distances (ties: the lower guiding index first) and their normalised inverse-distance weights."""
    c = texel_centres(G, uvs_gdn.device, uvs_gdn.dtype)
    uvs_sds = torch.stack(torch.meshgrid(c, c, indexing='xy'), dim=-1).view(-1, 2)
    dist = ((uvs_sds.view(-1, 1, 2) - uvs_gdn.view(1, -1, 2)) ** 2).sum(-1)
    knn_dist, knn_idx = torch.sort(dist, dim=1, stable=True)
    w = 1 / (knn_dist[:, :K] + DIST_EPS)
    return knn_idx[:, :K], w / w.sum(dim=-1, keepdim=True)


def inverted_lists(nbr, N: int):
    """``(start [N + 1], entries)`` int32: for each guiding strand the ``4 q + k`` that chose it, ascending."""
    flat = nbr.reshape(-1)
    _, entries = torch.sort(flat, stable=True)
    start = torch.zeros(N + 1, dtype=torch.int64, device=nbr.device)
    start[1:] = torch.cumsum(torch.bincount(flat, minlength=N), 0)
    return start.to(torch.int32), entries.to(torch.int32)


def csim_alpha_composed(v, nbr):
    """``(csim [N], alpha [N])`` of the texels ``q < N`` from their neighbours' segment vectors."""
    N = int(v.shape[0])
    knn_v = v[nbr[:N]]
    csim_full = F.cosine_similarity(knn_v[:, :, None], knn_v[:, None, :], dim=-1).mean(-1)
    j, k = torch.triu_indices(K, K, device=v.device)
    csim = csim_full[:, j, k].mean(-1)
    return csim, torch.where(csim <= CSIM_KNEE, 1 - 1.63 * csim ** 5, 0.4 - 0.4 * csim)


def _texture_composed(uvs_gdn, z, v, G):
    N, C = int(z.shape[0]), int(z.shape[1])
    nbr, w = neighbours_composed(uvs_gdn.detach(), G)
    _, alpha = csim_alpha_composed(v, nbr)
    alpha_q = (alpha[nbr] * w).sum(dim=1)[:, None]
    z_q = z[nbr[:, 0]] * alpha_q + (z[nbr] * w[:, :, None]).sum(dim=1) * (1 - alpha_q)
    return z_q.view(1, G, G, C).permute(0, 3, 1, 2)


class _LatentTexture(torch.autograd.Function):
    """-> texture and, not differentiable, the saved state (nbr, w, csim, alpha, alpha_q, start, list) for inspection."""

    @staticmethod
    def forward(ctx, uvg, z, v, centres):
        from .diff_gaussian_rasterization import _on_device, _ptr, _stream
        dev = z.device
        N, C, n, G = int(z.shape[0]), int(z.shape[1]), int(v.shape[1]), int(centres.shape[0])
        GG = G * G
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        nbr, w = torch.empty((GG, K), **i32), torch.empty((GG, K), **f32)
        csim, alpha, alpha_q = torch.empty(N, **f32), torch.empty(N, **f32), torch.empty(GG, **f32)
        ints = torch.empty(2 * N + 1 + K * GG, **i32)  # count | start | list
        count, start, lst = ints[:N], ints[N:2 * N + 1], ints[2 * N + 1:]
        texture = torch.empty((1, C, G, G), **f32)
        with _on_device(dev):
            _lib.check(_lib.lib().ghr_sds_texture(_stream(), N, n, C, G, _ptr(uvg), _ptr(centres), _ptr(z), _ptr(v), _ptr(nbr), _ptr(w),
                                                  _ptr(csim), _ptr(alpha), _ptr(alpha_q), _ptr(count), _ptr(start), _ptr(lst),
                                                  _ptr(texture)))
        ctx.save_for_backward(z, v, nbr, w, csim, alpha_q, start, lst)
        ctx.meta = (N, n, C, G)
        ctx.mark_non_differentiable(nbr, w, csim, alpha, alpha_q, start, lst)
        ctx.set_materialize_grads(False)  # (or autograd zero-fills a cotangent for each of the seven state outputs: seven launches)
        return texture, nbr, w, csim, alpha, alpha_q, start, lst

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_texture, *_):
        from .diff_gaussian_rasterization import _on_device, _ptr, _stream
        if d_texture is None:
            return None, None, None, None
        z, v, nbr, w, csim, alpha_q, start, lst = ctx.saved_tensors
        N, n, C, G = ctx.meta
        dev = z.device
        d_texture = d_texture.contiguous().float()
        scratch = torch.empty(G * G + N, dtype=torch.float32, device=dev)
        d_z = torch.empty_like(z)
        d_v = torch.empty_like(v) if ctx.needs_input_grad[2] else None
        with _on_device(dev):
            _lib.check(_lib.lib().ghr_sds_texture_backward(_stream(), N, n, C, G, _ptr(z), _ptr(v), _ptr(nbr), _ptr(w), _ptr(csim),
                                                           _ptr(alpha_q), _ptr(start), _ptr(lst), _ptr(d_texture), _ptr(scratch[:G * G]),
                                                           _ptr(scratch[G * G:]), _ptr(d_z), None if d_v is None else _ptr(d_v)))
        return None, d_z, d_v, None


def latent_texture(uvs_gdn, z, v, grid: int, fused=None, return_state: bool = False):
    """``[1, C, G, G]`` latent texture from the guiding strands' UVs ``[N, 2]``, latent codes ``z [N, C]`` and local segment vectors
    ``v [N, n, 3]``; ``G = grid``.  Gradients flow to ``z`` and, through the blending coefficients, to ``v``; the UVs carry none.
    ``alpha[g]`` is computed from the neighbourhood of TEXEL number ``g`` (the reference's indexing), hence ``G * G >= N``.
    ``return_state`` (HIP form): also the dict of the saved neighbour indices, weights, similarities and inverted lists."""
    G = int(grid)
    if z.dim() != 2 or z.shape[1] < 1 or v.dim() != 3 or v.shape[-1] != 3 or v.shape[1] < 1 or v.shape[0] != z.shape[0]:
        raise ValueError("z must be [N, C] and v [N, n, 3] with C, n >= 1")
    if tuple(uvs_gdn.shape) != (int(z.shape[0]), 2):
        raise ValueError("uvs_gdn must be [N, 2]")
    _check_sizes(int(z.shape[0]), G)
    if not _use_fused(fused, z):
        if return_state:
            raise ValueError("return_state belongs to the HIP form")
        return _texture_composed(uvs_gdn, z, v, G)
    if z.dtype != torch.float32 or v.dtype != torch.float32:
        raise RuntimeError("strand_prior: the HIP form takes float32")
    out = _LatentTexture.apply(uvs_gdn.detach().float().contiguous(), z.contiguous(), v.contiguous(), _centres_cached(G, z.device))
    if return_state:
        return out[0], dict(zip(("nbr", "w", "csim", "alpha", "alpha_q", "start", "list"), out[1:]))
    return out[0]


# ---- steps 1 - 4 ------------------------------------------------------------------------------------------------------------------------
class StrandPrior:
    """``prior(dirs) -> Lsds``: draw ``num_guiding`` strands, local frames, ``encoder(e)[:, :channels]``, the latent texture,
    ``prior_loss(texture).mean()``.  The noise, sigma and mask the reference draws belong to ``prior_loss``.  ``local2world`` is
    inverted once, here, in float64 and then rounded (the reference inverts in float32 every iteration)."""

    def __init__(self, encoder: Callable, prior_loss: Callable, uvs, local2world, grid: int, scale_decoder: float,
                 num_guiding: int = 1000, channels: int = 64, generator=None, fused=None):
        _check_sizes(int(num_guiding), int(grid))
        if int(channels) < 1:
            raise ValueError("channels < 1")
        self.encoder, self.prior_loss = encoder, prior_loss
        self.uvs = uvs.detach().float().contiguous()
        self.world2local = torch.linalg.inv(local2world.detach().double()).float().contiguous()
        self.grid, self.scale_decoder = int(grid), float(scale_decoder)
        self.num_guiding, self.channels = int(num_guiding), int(channels)
        self.generator, self.fused = generator, fused
        self.last_idx = self.last_texture = None

    def draw(self, S: int, device) -> torch.Tensor:
        return torch.randint(low=0, high=S, size=(self.num_guiding,), device=device, generator=self.generator)

    def __call__(self, dirs, idx=None):
        idx = self.draw(int(dirs.shape[0]), dirs.device) if idx is None else idx
        e, v = guiding_strands_local(dirs, self.world2local, idx, self.scale_decoder, fused=self.fused, frames_are_inverse=True)
        z = self.encoder(e)[:, :self.channels]
        texture = latent_texture(self.uvs[idx], z, v, self.grid, fused=self.fused)
        self.last_idx, self.last_texture = idx, texture.detach()
        return self.prior_loss(texture).mean()
