"""The textured strand generator: what lies between the strand decoder and the colour decoder of the reference's
``strands_generator`` (src/scene/gaussian_model_latent_strands.py:442-484, gaussian_model_strands.py:521-576,
export_strands.py:43-55, arguments/hair_strands_textured.yaml).  NeuralHaircut's ``OptimizableTexturedStrands`` is not vendored
in the reference, so the generator is DEFINED here, from those call sites and the published ``grid_sample`` formula.

Once, on the host in float64: a tangent frame per scalp face (``scalp_frames``), ``max_num_strands`` roots drawn on the mesh
(``sample_roots``), and each root's bilinear taps in the latent texture with the inverted texel lists (``texture_taps``).  Per
iteration: a draw of roots, the fetch of the ``[1, C, T, T]`` texture at them (``sample_texture``), the caller's decoders, and the
running sum of the decoded local segments taken through each root's frame (``strands_to_world``).  On a ROCm tensor both pieces
and their backward are HIP (csrc/ghr_texstrands.h): the texture's gradient is assigned whole, in a fixed order, without atomics.
``fused=False`` is the PyTorch-composed comparator -- the SAME stored taps, an index gather, the weighted sum in the same order,
``cumsum`` and ``matmul`` -- and the only form for CPU tensors.

With ``num_guiding_strands`` only the draw's first ``N`` roots are fetched from the texture; every other root's
latent row is blended from its four nearest guides in UV by HAAR's cosine-similarity rule (``blend_from_guides``,
csrc/ghr_guides.h), as the reference's generator is configured by ``arguments/hair_strands_textured.yaml``.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional

import torch

from . import _lib


def _use_fused(fused, t) -> bool:
    if fused is None:
        return bool(t.is_cuda)
    if fused and not t.is_cuda:
        raise RuntimeError("strand_generator: the HIP form has no CPU path (fused=False is the composed form)")
    return bool(fused)


def _check_on(device, dtype, **tensors):
    """the HIP form hands raw pointers to the kernels: every buffer on the data's device, in the type the kernels read"""
    for name, t in tensors.items():
        if t.device != device or (dtype is not None and t.dtype != dtype):
            raise ValueError("%s must be a %s tensor on %s, got %s on %s" % (name, dtype or "floating-point", device, t.dtype, t.device))


# ---- once: frames, roots, taps (host, float64) ------------------------------------------------------------------------------------
def _faces64(vertices, faces, vertex_uvs):
    """(frames [F, 3, 3], sampling weights [F]: the area, 0 for a degenerate face) in float64 on the CPU"""
    v, uv, f = vertices.detach().double().cpu(), vertex_uvs.detach().double().cpu(), faces.detach().long().cpu()
    if v.dim() != 2 or v.shape[1] != 3 or uv.shape != (v.shape[0], 2) or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError("scalp must be (vertices [V, 3], faces [F, 3], vertex_uvs [V, 2])")
    if f.numel() and (int(f.min()) < 0 or int(f.max()) >= v.shape[0]):
        raise ValueError("a face names a vertex outside 0 .. V - 1")
    va, vb, vc = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    e1, e2 = vb - va, vc - va
    d1, d2 = uv[f[:, 1]] - uv[f[:, 0]], uv[f[:, 2]] - uv[f[:, 0]]
    det = d1[:, 0] * d2[:, 1] - d2[:, 0] * d1[:, 1]
    traw = (d2[:, 1:2] * e1 - d1[:, 1:2] * e2) * torch.sign(det)[:, None]
    cross = torch.linalg.cross(e1, e2)
    area2 = cross.norm(dim=-1)
    nrm = cross / area2.clamp_min(1e-300)[:, None]
    t = traw - (traw * nrm).sum(-1, keepdim=True) * nrm
    tlen = t.norm(dim=-1)
    valid = (area2 > 0) & (det != 0) & (tlen > 0) & torch.isfinite(area2) & torch.isfinite(det) & torch.isfinite(tlen)
    t = t / tlen.clamp_min(1e-300)[:, None]
    b = torch.linalg.cross(nrm, t)
    frames = torch.stack([t, b, nrm], dim=-1)
    frames = torch.where(valid[:, None, None], frames, torch.eye(3, dtype=torch.float64).expand_as(frames))
    return frames, torch.where(valid, area2 * 0.5, torch.zeros_like(area2))


def scalp_frames(vertices, faces, vertex_uvs) -> torch.Tensor:
    """``[F, 3, 3]`` float32 ``local2world`` of every face, columns (tangent along +u, bitangent, normal): orthonormal and
    right-handed, computed in float64 and then rounded.  A face of zero area or with a zero UV determinant gets the identity."""
    return _faces64(vertices, faces, vertex_uvs)[0].float()


def sample_roots(vertices, faces, vertex_uvs, max_num_strands: int, generator=None) -> dict:
    """``max_num_strands`` roots on the scalp: faces by ``torch.multinomial`` on their float64 areas (degenerate faces weigh 0),
    barycentrics ``(1 - sqrt(r1), sqrt(r1) (1 - r2), sqrt(r1) r2)``.  -> ``origins [Smax, 3]``, ``uvs [Smax, 2]``,
    ``face_idx [Smax]``, ``local2world [Smax, 3, 3]`` (float32 CPU tensors, int64 indices)."""
    Smax = int(max_num_strands)
    if Smax < 1:
        raise ValueError("max_num_strands < 1")
    if not bool(torch.isfinite(vertex_uvs).all()):
        raise ValueError("a vertex UV is not finite")
    frames, areas = _faces64(vertices, faces, vertex_uvs)
    if not float(areas.sum()) > 0:
        raise ValueError("the scalp has no face to sample: every face is degenerate")
    face_idx = torch.multinomial(areas, Smax, replacement=True, generator=generator)
    r = torch.rand(Smax, 2, dtype=torch.float64, generator=generator)
    s1 = torch.sqrt(r[:, 0])
    bary = torch.stack([1 - s1, s1 * (1 - r[:, 1]), s1 * r[:, 1]], dim=-1)
    f = faces.detach().long().cpu()[face_idx]
    v, uv = vertices.detach().double().cpu(), vertex_uvs.detach().double().cpu()
    origins = (v[f] * bary[..., None]).sum(1)
    uvs = (uv[f] * bary[..., None]).sum(1)
    return dict(origins=origins.float(), uvs=uvs.float(), face_idx=face_idx, local2world=frames[face_idx].float().contiguous())


class Taps(NamedTuple):
    """per root: ``x0, y0`` int32 and ``fx, fy`` float32; per texel ``q = y T + x`` the inverted list ``list[start[q]:start[q+1]]``
    of ``4 r + k``, ascending, of the (root, tap) pairs inside the texture"""
    x0: torch.Tensor
    y0: torch.Tensor
    fx: torch.Tensor
    fy: torch.Tensor
    start: torch.Tensor
    list: torch.Tensor
    T: int

    def to(self, device):
        return Taps(*[t.to(device) for t in self[:6]], self.T)


def texture_taps(uvs, texture_size: int) -> Taps:
    """The bilinear taps of ``uvs [Smax, 2]`` in a ``T x T`` texture (``align_corners=False``, ``padding_mode="zeros"``), from
    coordinates formed in float64 -- ``F.grid_sample`` forms them in float32 -- and the inverted lists, in integers only."""
    T = int(texture_size)
    if T < 1:
        raise ValueError("texture_size < 1")
    u = uvs.detach().double().cpu()
    if u.dim() != 2 or u.shape[1] != 2:
        raise ValueError("uvs must be [Smax, 2]")
    if not bool(torch.isfinite(u).all()):
        raise ValueError("a UV is not finite")
    xy = ((u + 1) * T - 1) / 2
    lo = torch.floor(xy)
    frac = (xy - lo).float()
    cell = lo.clamp(-2, T).to(torch.int32)  # beyond -2 or T every tap is dropped all the same
    x0, y0 = cell[:, 0].contiguous(), cell[:, 1].contiguous()
    Smax = int(u.shape[0])
    k = torch.arange(4).repeat(Smax)
    r = torch.arange(Smax).repeat_interleave(4)
    xk, yk = x0.long()[r] + (k & 1), y0.long()[r] + (k >> 1)
    inside = (xk >= 0) & (xk < T) & (yk >= 0) & (yk < T)
    q = (yk * T + xk)[inside]
    entries = (4 * r + k)[inside]
    order = torch.sort(q, stable=True)[1]
    start = torch.zeros(T * T + 1, dtype=torch.int64)
    start[1:] = torch.cumsum(torch.bincount(q, minlength=T * T), 0)
    return Taps(x0, y0, frac[:, 0].contiguous(), frac[:, 1].contiguous(), start.to(torch.int32), entries[order].to(torch.int32), T)


def tap_weight(k: int, fx, fy):
    """float32 weight of tap ``k``: ``ts_weight`` (csrc/ghr_texstrands.h)"""
    return (fx if k & 1 else 1 - fx) * (fy if k >> 1 else 1 - fy)


# ---- per iteration: the fetch ------------------------------------------------------------------------------------------------------
def _fetch_composed(texture, taps: Taps, idx):
    T, C = taps.T, int(texture.shape[1])
    flat = texture[0].reshape(C, T * T)
    x0, y0 = taps.x0[idx].long(), taps.y0[idx].long()
    fx, fy = taps.fx[idx].to(texture.dtype), taps.fy[idx].to(texture.dtype)
    z = None
    for k in range(4):
        xk, yk = x0 + (k & 1), y0 + (k >> 1)
        inside = (xk >= 0) & (xk < T) & (yk >= 0) & (yk < T)
        t = flat[:, yk.clamp(0, T - 1) * T + xk.clamp(0, T - 1)].t()
        term = torch.where(inside[:, None], tap_weight(k, fx, fy)[:, None] * t, torch.zeros_like(t))  # a dropped tap is skipped
        z = term if z is None else z + term
    return z


class _TexFetch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, texture, x0, y0, fx, fy, start, lst, idx):
        from .diff_gaussian_rasterization import _on_device, _ptr, _stream
        C, T = int(texture.shape[1]), int(texture.shape[2])
        Smax, S = int(x0.shape[0]), int(idx.shape[0])
        z = torch.empty((S, C), dtype=torch.float32, device=texture.device)
        with _on_device(texture.device):
            _lib.check(_lib.lib().ghr_ts_fetch(_stream(), Smax, S, T, C, _ptr(texture), _ptr(x0), _ptr(y0), _ptr(fx), _ptr(fy), _ptr(idx),
                                               _ptr(z)))
        ctx.save_for_backward(fx, fy, start, lst, idx)
        ctx.meta = (Smax, S, T, C)
        return z

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_z):
        from .diff_gaussian_rasterization import _on_device, _ptr, _stream
        if not ctx.needs_input_grad[0]:
            return (None,) * 8
        fx, fy, start, lst, idx = ctx.saved_tensors
        Smax, S, T, C = ctx.meta
        d_z = d_z.contiguous().float()
        pos = torch.empty(Smax, dtype=torch.int32, device=d_z.device)
        d_texture = torch.empty((1, C, T, T), dtype=torch.float32, device=d_z.device)  # every element is assigned by the kernel
        with _on_device(d_z.device):
            _lib.check(_lib.lib().ghr_ts_fetch_backward(_stream(), Smax, S, T, C, _ptr(fx), _ptr(fy), _ptr(start),
                                                        _ptr(lst) if lst.numel() else None, int(lst.numel()), _ptr(idx), _ptr(d_z),
                                                        _ptr(pos), _ptr(d_texture)))
        return (d_texture,) + (None,) * 7


def sample_texture(texture, taps: Taps, idx, fused=None, validate: bool = True):
    """``z [S, C]``: the texture ``[1, C, T, T]`` at the roots ``idx`` through their stored taps,
    ``((w0 t0 + w1 t1) + w2 t2) + w3 t3`` with the taps outside the texture skipped.  ``idx`` may hold no root twice: the
    gradient's sum per texel runs over roots, not rows (``validate`` checks it, with a device synchronisation)."""
    if texture.dim() != 4 or texture.shape[0] != 1 or texture.shape[2] != taps.T or texture.shape[3] != taps.T:
        raise ValueError("texture must be [1, C, %d, %d]" % (taps.T, taps.T))
    if idx.dim() != 1 or idx.dtype != torch.int64 or idx.numel() < 1:
        raise ValueError("idx must be a 1-D int64 tensor of at least one root")
    Smax = int(taps.x0.shape[0])
    if idx.numel() > Smax:
        raise ValueError("more roots drawn than there are")
    if validate:
        if int(idx.min()) < 0 or int(idx.max()) >= Smax:
            raise ValueError("idx names a root outside 0 .. Smax - 1")
        if int(torch.unique(idx).numel()) != int(idx.numel()):
            raise ValueError("idx holds a root twice")
    if not _use_fused(fused, texture):
        return _fetch_composed(texture, taps, idx)
    if texture.dtype != torch.float32:
        raise RuntimeError("strand_generator: the HIP form takes float32")
    dev, T = texture.device, taps.T
    _check_on(dev, torch.int32, x0=taps.x0, y0=taps.y0, start=taps.start, list=taps.list)
    _check_on(dev, torch.float32, fx=taps.fx, fy=taps.fy)
    _check_on(dev, torch.int64, idx=idx)
    if any(tuple(t.shape) != (Smax,) for t in (taps.y0, taps.fx, taps.fy)) or tuple(taps.start.shape) != (T * T + 1,) or \
            taps.list.dim() != 1 or taps.list.numel() > 4 * Smax:
        raise ValueError("taps must be x0, y0, fx, fy [Smax], start [T T + 1] and list [<= 4 Smax]")
    return _TexFetch.apply(texture.contiguous(), *[t.contiguous() for t in taps[:6]], idx.contiguous())


# ---- per iteration: to world -------------------------------------------------------------------------------------------------------
def _world_composed(v, local2world, origins, idx, inv_scale):
    pl = torch.cat([torch.zeros_like(v[:, :1]), torch.cumsum(v, dim=1)], dim=1) * inv_scale
    M = local2world[idx].to(v.dtype)
    p = origins[idx].to(v.dtype)[:, None] + (M[:, None] @ pl[..., None])[..., 0]
    return p, pl


class _ToWorld(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, local2world, origins, idx, inv_scale, want_local):
        from .diff_gaussian_rasterization import _on_device, _ptr, _stream
        S, n, Smax = int(v.shape[0]), int(v.shape[1]), int(origins.shape[0])
        p = torch.empty((S, n + 1, 3), dtype=torch.float32, device=v.device)
        pl = torch.empty_like(p) if want_local else None
        with _on_device(v.device):
            _lib.check(_lib.lib().ghr_ts_world(_stream(), Smax, S, n, _ptr(v), _ptr(local2world), _ptr(origins), _ptr(idx),
                                               float(inv_scale), _ptr(p), None if pl is None else _ptr(pl)))
        ctx.save_for_backward(local2world, idx)
        ctx.meta = (Smax, S, n, float(inv_scale))
        ctx.set_materialize_grads(False)
        return p, pl

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_p, d_pl):
        from .diff_gaussian_rasterization import _on_device, _ptr, _stream
        if not ctx.needs_input_grad[0] or (d_p is None and d_pl is None):
            return (None,) * 6
        local2world, idx = ctx.saved_tensors
        Smax, S, n, inv_scale = ctx.meta
        d_p = None if d_p is None else d_p.contiguous().float()
        d_pl = None if d_pl is None else d_pl.contiguous().float()
        d_v = torch.empty((S, n, 3), dtype=torch.float32, device=local2world.device)
        with _on_device(local2world.device):
            _lib.check(_lib.lib().ghr_ts_world_backward(_stream(), Smax, S, n, _ptr(local2world), _ptr(idx), inv_scale,
                                                        None if d_p is None else _ptr(d_p), None if d_pl is None else _ptr(d_pl),
                                                        _ptr(d_v)))
        return (d_v,) + (None,) * 5


def strands_to_world(v, local2world, origins, idx, scale_decoder: float = 1.0, fused=None, return_local: bool = False):
    """``p [S, n + 1, 3]``: ``p[s, j] = origins[idx[s]] + local2world[idx[s]] Pl[s, j]`` with ``Pl[s, 0] = 0`` and
    ``Pl[s, j] = (sum_{i < j} v[s, i]) / scale_decoder``; with ``return_local`` also ``Pl``.  ``v [S, n, 3]`` are the decoder's
    local segments; origins ``[Smax, 3]`` and frames ``[Smax, 3, 3]`` are buffers and carry no gradient."""
    if v.dim() != 3 or v.shape[-1] != 3 or v.shape[1] < 1:
        raise ValueError("v must be [S, n, 3] with n >= 1")
    Smax = int(origins.shape[0])
    if tuple(origins.shape) != (Smax, 3) or tuple(local2world.shape) != (Smax, 3, 3):
        raise ValueError("origins must be [Smax, 3] and local2world [Smax, 3, 3]")
    if idx.dim() != 1 or idx.dtype != torch.int64 or idx.shape[0] != v.shape[0]:
        raise ValueError("idx must be a 1-D int64 tensor, one root per strand")
    inv_scale = 1.0 / float(scale_decoder)
    if not _use_fused(fused, v):
        p, pl = _world_composed(v, local2world.detach(), origins.detach(), idx, inv_scale)
    else:
        if v.dtype != torch.float32:
            raise RuntimeError("strand_generator: the HIP form takes float32")
        _check_on(v.device, None, local2world=local2world, origins=origins)
        _check_on(v.device, torch.int64, idx=idx)
        p, pl = _ToWorld.apply(v.contiguous(), local2world.detach().float().contiguous(), origins.detach().float().contiguous(),
                               idx.contiguous(), inv_scale, bool(return_local))
    return (p, pl) if return_local else p


# ---- per iteration: the other strands from the guides ------------------------------------------------------------------------------
GUIDE_K = 4
GUIDE_STATE = ("nbr", "w", "csim", "alpha", "alpha_s", "start", "list")


def guide_neighbours_composed(uvs, N: int):
    """``(nbr [S, 4] int64, w [S, 4])``: every drawn root's four nearest of the first ``N`` roots under a STABLE sort of the
    squared UV distances (ties: the lower guide first) and their normalised inverse-distance weights."""
    from .strand_prior import DIST_EPS
    dist = ((uvs.view(-1, 1, 2) - uvs[:N].view(1, -1, 2)) ** 2).sum(-1)
    knn_dist, knn_idx = torch.sort(dist, dim=1, stable=True)
    w = 1 / (knn_dist[:, :GUIDE_K] + DIST_EPS)
    return knn_idx[:, :GUIDE_K], w / w.sum(dim=-1, keepdim=True)


def _blend_composed(uvs, z_g, v_g):
    from .strand_prior import csim_alpha_composed, inverted_lists
    N = int(z_g.shape[0])
    nbr, w = guide_neighbours_composed(uvs.detach(), N)
    csim, alpha = csim_alpha_composed(v_g, nbr)  # of the guides s < N: their own neighbourhoods
    alpha_s = (alpha[nbr] * w).sum(dim=1)
    a, nb, wi = alpha_s[N:, None], nbr[N:], w[N:]
    z_i = z_g[nb[:, 0]] * a + (z_g[nb] * wi[:, :, None]).sum(dim=1) * (1 - a)
    start, lst = inverted_lists(nbr, N)
    state = (nbr.to(torch.int32), w, csim.detach(), alpha.detach(), alpha_s.detach(), start, lst)
    return torch.cat([z_g, z_i], dim=0), state


class _GuidesBlend(torch.autograd.Function):
    """-> z and, not differentiable, the saved state (nbr, w, csim, alpha, alpha_s, start, list) for inspection."""

    @staticmethod
    def forward(ctx, uvs, z_g, v_g):
        from .diff_gaussian_rasterization import _on_device, _ptr, _stream
        dev = z_g.device
        S, N, C, n = int(uvs.shape[0]), int(z_g.shape[0]), int(z_g.shape[1]), int(v_g.shape[1])
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        nbr, w = torch.empty((S, GUIDE_K), **i32), torch.empty((S, GUIDE_K), **f32)
        csim, alpha, alpha_s = torch.empty(N, **f32), torch.empty(N, **f32), torch.empty(S, **f32)
        ints = torch.empty(2 * N + 1 + 2 * GUIDE_K * S, **i32)  # count | start | list | the lists in arrival order
        count, start = ints[:N], ints[N:2 * N + 1]
        lst, unsorted = ints[2 * N + 1:2 * N + 1 + GUIDE_K * S], ints[2 * N + 1 + GUIDE_K * S:]
        z = torch.empty((S, C), **f32)
        with _on_device(dev):
            _lib.check(_lib.lib().ghr_guides_blend(_stream(), S, N, n, C, _ptr(uvs), _ptr(z_g), _ptr(v_g), _ptr(nbr), _ptr(w), _ptr(csim),
                                                   _ptr(alpha), _ptr(alpha_s), _ptr(count), _ptr(start), _ptr(unsorted), _ptr(lst),
                                                   _ptr(z)))
        ctx.save_for_backward(z_g, v_g, nbr, w, csim, alpha_s, start, lst)
        ctx.meta = (S, N, n, C)
        ctx.mark_non_differentiable(nbr, w, csim, alpha, alpha_s, start, lst)
        ctx.set_materialize_grads(False)  # (or autograd zero-fills a cotangent for each of the seven state outputs)
        return z, nbr, w, csim, alpha, alpha_s, start, lst

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_z, *_):
        from .diff_gaussian_rasterization import _on_device, _ptr, _stream
        if d_z is None or not (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
            return None, None, None
        z_g, v_g, nbr, w, csim, alpha_s, start, lst = ctx.saved_tensors
        S, N, n, C = ctx.meta
        dev = z_g.device
        d_z = d_z.contiguous().float()
        scratch = torch.empty(S + N, dtype=torch.float32, device=dev)
        d_zg = torch.empty_like(z_g)
        d_vg = torch.empty_like(v_g) if ctx.needs_input_grad[2] else None
        with _on_device(dev):
            _lib.check(_lib.lib().ghr_guides_blend_backward(_stream(), S, N, n, C, _ptr(z_g), _ptr(v_g), _ptr(nbr), _ptr(w), _ptr(csim),
                                                            _ptr(alpha_s), _ptr(start), _ptr(lst), _ptr(d_z), _ptr(scratch[:S]),
                                                            _ptr(scratch[S:]), _ptr(d_zg), None if d_vg is None else _ptr(d_vg)))
        return None, d_zg if ctx.needs_input_grad[1] else None, d_vg


def blend_from_guides(uvs, z_g, v_g, fused=None, return_state: bool = False):
    """``z [S, C]``: the latent rows of one draw whose first ``N = z_g.shape[0]`` roots are the guides.  ``uvs [S, 2]`` are the
    drawn roots' UVs (guides first), ``z_g [N, C]`` the guides' fetched rows, ``v_g [N, n, 3]`` their decoded local segments.
    ``z[:N] = z_g``; a row ``s >= N`` is ``z_g[nbr_0] alpha_s + (sum_k w_k z_g[nbr_k]) (1 - alpha_s)`` over its four nearest
    guides in UV, ``alpha_s = sum_k w_k alpha[nbr_k]`` and ``alpha[g]`` HAAR's coefficient of the cosine similarity among guide
    ``g``'s own four neighbours.  Gradients flow to ``z_g`` and, through the coefficients, to ``v_g``; the UVs carry none.
    ``return_state``: also the dict of neighbour indices, weights, similarities and the guides' inverted lists."""
    if z_g.dim() != 2 or z_g.shape[1] < 1 or v_g.dim() != 3 or v_g.shape[-1] != 3 or v_g.shape[1] < 1 or v_g.shape[0] != z_g.shape[0]:
        raise ValueError("z_g must be [N, C] and v_g [N, n, 3] with C, n >= 1")
    N = int(z_g.shape[0])
    if uvs.dim() != 2 or uvs.shape[1] != 2 or uvs.shape[0] < N:
        raise ValueError("uvs must be [S, 2] with S >= N, the guides first")
    if N < GUIDE_K:
        raise ValueError("N = %d guiding strands: a strand needs %d" % (N, GUIDE_K))
    if not _use_fused(fused, z_g):
        z, state = _blend_composed(uvs, z_g, v_g)
    else:
        if z_g.dtype != torch.float32 or v_g.dtype != torch.float32:
            raise RuntimeError("strand_generator: the HIP form takes float32")
        _check_on(z_g.device, None, uvs=uvs, v_g=v_g)
        z, *state = _GuidesBlend.apply(uvs.detach().float().contiguous(), z_g.contiguous(), v_g.contiguous())
    return (z, dict(zip(GUIDE_STATE, state))) if return_state else z


# ---- the generator -----------------------------------------------------------------------------------------------------------------
class TexturedStrands(torch.nn.Module):
    """``generator(iteration) -> {"points", "features", "orient_conf", "L_diff"}``, the contract ``GaussianModelLatentStrands``
    reads.  Its one own parameter is ``texture [1, Cg + Ca, T, T]`` (zeros); roots, frames, taps and lists are buffers; the
    decoders and ``prior_loss`` are the caller's and, where they are Modules, submodules.  ``features`` / ``orient_conf`` come
    from ``color_decoder(z_app[:, 1:])`` split ``3 | 3 ((deg + 1)^2 - 1) | 1``; ``L_diff = prior_loss(texture[:, :Cg])``.
    ``num_guiding_strands`` (``None`` / ``0``: none; else at least 4): the first ``min(num_guiding_strands, S)`` roots of a draw are
    the guides, the only rows fetched from the texture; the others are ``blend_from_guides`` of them and the decoder runs on the
    two groups in turn.  ``last_num_guiding`` is the ``N`` of the last call (0 when every strand was fetched)."""

    def __init__(self, scalp, strand_decoder: Callable, color_decoder: Optional[Callable] = None, prior_loss: Optional[Callable] = None,
                 num_strands: int = 10_000, max_num_strands: int = 50_000, texture_size: int = 256, geometry_channels: int = 64,
                 appearance_channels: int = 65, scale_decoder: float = 1.0, sh_degree: int = 3, generator=None, fused: bool = True,
                 num_guiding_strands: Optional[int] = None):
        super().__init__()
        S, Smax, Cg, Ca = int(num_strands), int(max_num_strands), int(geometry_channels), int(appearance_channels)
        if not 1 <= S <= Smax:
            raise ValueError("num_strands must be in 1 .. max_num_strands")
        if Cg < 1 or Ca < 0:
            raise ValueError("geometry_channels < 1 or appearance_channels < 0")
        Ng = 0 if num_guiding_strands is None else int(num_guiding_strands)
        if Ng < 0 or 0 < Ng < GUIDE_K:
            raise ValueError("num_guiding_strands must be None, 0 or at least %d: a strand is blended from %d guides" % (GUIDE_K, GUIDE_K))
        vertices, faces, vertex_uvs = scalp
        roots = sample_roots(vertices, faces, vertex_uvs, Smax, generator)
        taps = texture_taps(roots["uvs"], texture_size)
        self.num_strands, self.max_num_strands, self.texture_size = S, Smax, int(texture_size)
        self.geometry_channels, self.appearance_channels = Cg, Ca
        self.scale_decoder, self.sh_degree = float(scale_decoder), int(sh_degree)
        self.generator, self.fused = generator, bool(fused)
        self.strand_decoder, self.color_decoder, self.prior_loss = strand_decoder, color_decoder, prior_loss
        self.texture = torch.nn.Parameter(torch.zeros(1, Cg + Ca, taps.T, taps.T))
        for name in ("origins", "uvs", "face_idx", "local2world"):
            self.register_buffer(name, roots[name])
        for name in Taps._fields[:6]:
            self.register_buffer("tap_" + name, getattr(taps, name))
        self.num_guiding_strands, self.last_num_guiding = Ng, 0
        self.guides_fused = None  # None: the blend takes the form the fetch takes; False: the composed blend beside the HIP fetch
        self.last_idx = None

    @property
    def taps(self) -> Taps:
        return Taps(*[getattr(self, "tap_" + name) for name in Taps._fields[:6]], self.texture_size)

    def draw(self, num: Optional[int] = None) -> torch.Tensor:
        """``randperm(Smax)[:num]`` under the module's generator: no root twice"""
        num = self.num_strands if num is None else int(num)
        if not 1 <= num <= self.max_num_strands:
            raise ValueError("num_strands must be in 1 .. max_num_strands")
        dev = self.generator.device if self.generator is not None else self.texture.device
        return torch.randperm(self.max_num_strands, generator=self.generator, device=dev)[:num].to(self.texture.device)

    def _strands(self, idx, want_local):
        fused = self.fused and self.texture.is_cuda
        S, Cg = int(idx.shape[0]), self.geometry_channels
        N = min(self.num_guiding_strands, S)
        if N == 0 or S <= N:  # no guiding, or every strand is a guide
            N = 0
            z = sample_texture(self.texture, self.taps, idx, fused=fused, validate=False)
            v = self.strand_decoder(z[:, :Cg])
        else:  # the first N roots are fetched and decoded; the others' rows are blended from them, then decoded
            z_g = sample_texture(self.texture, self.taps, idx[:N], fused=fused, validate=False)
            v_g = self.strand_decoder(z_g[:, :Cg])
            if v_g.dim() != 3 or v_g.shape[0] != N or v_g.shape[-1] != 3:
                raise ValueError("strand_decoder must return [S, n, 3], got %s" % (tuple(v_g.shape),))
            z = blend_from_guides(self.uvs[idx], z_g, v_g, fused=fused if self.guides_fused is None else fused and self.guides_fused)
            v = torch.cat([v_g, self.strand_decoder(z[N:, :Cg])], dim=0)
        z_geom, z_app = z[:, :Cg], z[:, Cg:]
        if v.dim() != 3 or v.shape[0] != idx.shape[0] or v.shape[-1] != 3:
            raise ValueError("strand_decoder must return [S, n, 3], got %s" % (tuple(v.shape),))
        self.last_num_guiding = N
        out = strands_to_world(v, self.local2world, self.origins, idx, self.scale_decoder, fused=fused, return_local=want_local)
        self.last_idx = idx
        return out, z_geom, z_app

    def appearance(self, z_app):
        """``(features [S, 3 (deg + 1)^2], orient_conf [S, 1])`` of the colour decoder, as gaussian_model_latent_strands.py:471"""
        K3 = 3 * (self.sh_degree + 1) ** 2
        o = self.color_decoder(z_app[:, 1:])
        if o.dim() != 2 or o.shape[1] != K3 + 1:
            raise ValueError("color_decoder must return [S, %d], got %s" % (K3 + 1, tuple(o.shape)))
        return o[:, :K3], o[:, K3:]

    def _diffusion(self) -> dict:
        if self.prior_loss is None:
            return {}
        return {"L_diff": self.prior_loss(self.texture[:, :self.geometry_channels])}

    def forward(self, iteration=0) -> dict:
        p, _, z_app = self._strands(self.draw(), False)
        out = {"points": p}
        if self.color_decoder is not None:
            out["features"], out["orient_conf"] = self.appearance(z_app)
        out.update(self._diffusion())
        return out

    def forward_reference(self, iteration=0):
        """the reference's 7-tuple ``(p, uvs, local2world, p_local, z_geom, z_app, diffusion_dict)``"""
        idx = self.draw()
        (p, pl), z_geom, z_app = self._strands(idx, True)
        return p, self.uvs[idx], self.local2world[idx], pl, z_geom, z_app, self._diffusion()

    @torch.no_grad()
    def forward_inference(self, num_strands: int):
        """the reference's 6-tuple ``(p, uvs, local2world, p_local, z_geom, z_app)`` of ``num_strands`` roots"""
        idx = self.draw(num_strands)
        (p, pl), z_geom, z_app = self._strands(idx, True)
        return p, self.uvs[idx], self.local2world[idx], pl, z_geom, z_app
