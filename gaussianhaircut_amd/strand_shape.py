"""The strand stage's shape term: stretch, bend and neighbour coherence of explicit strands, a geometric prior that
needs no network.  The reference keeps strands hair-like with a pretrained decoder and a diffusion prior; a model made by
``GaussianModelStrands.create_from_polylines`` optimises the segment vectors ``_dirs [S, n, 3]`` themselves and nothing else keeps a
segment from stretching, a strand from kinking or two neighbours from crossing.

``StrandShape(origins, dirs, ...)`` computes once: a rest length per strand (the mean segment length, float64, rounded once), the
4 nearest other roots of every root (``-1`` beyond ``radius`` or where fewer exist), the number ``M`` of valid pairs and the
inverted lists of the backward.  Then

    shape.terms(dirs) -> [3]   the means (stretch, bend, coherence); the definition is at the top of csrc/ghr_shape.h
    shape(dirs)       -> (weights * terms).sum()

On a ROCm device with ``fused=True`` the three means and their backward are one ``autograd.Function`` over two HIP calls
(``ghr_shape_forward`` / ``ghr_shape_backward``: no ``[S, 4, n, 3]`` gather, no floating-point atomics, the same bits every run);
``fused=False`` is the PyTorch-composed comparator -- the same float32 expressions with torch's reductions -- and the only form on
CPU tensors.  Attach it with ``GaussianModelStrands.attach_shape``; ``trainer.strand_training_step`` then adds
``Lshape * opt.lambda_dshape`` to the first view's loss when ``opt.lambda_dshape`` is there and not 0.
"""
from __future__ import annotations

import math

import torch

from . import _lib

K = 4
DEAD = 1e-4  # GHR_SHAPE_DEAD (csrc/ghr_shape.h), applied in float32
_ROWS = 2048  # query rows per pass of the composed neighbour search


def _fusable(t: torch.Tensor) -> bool:
    return t.is_cuda and t.dtype == torch.float32


def nearest_roots(roots: torch.Tensor, radius=None, fused: bool = True) -> torch.Tensor:
    """``roots [S, 3]`` float32 -> ``[S, 4]`` int32: the 4 nearest other roots by ``((dx*dx)+(dy*dy))+(dz*dz)``, ascending, equal
    distances to the lower index; ``-1`` where the squared distance exceeds ``radius**2`` (float32) or fewer than 4 exist."""
    roots = roots.detach().reshape(-1, 3).float().contiguous()
    S = int(roots.shape[0])
    r2 = math.inf if radius is None else float(torch.tensor(float(radius), dtype=torch.float32).square())
    if not r2 > 0:
        raise ValueError("StrandShape: radius must be positive, got %r" % (radius,))
    if fused and _fusable(roots):
        from .diff_gaussian_rasterization import _on_device, _ptr, _stream
        nbr = torch.empty((S, K), dtype=torch.int32, device=roots.device)
        with _on_device(roots.device):
            _lib.check(_lib.lib().ghr_shape_neighbours(_stream(), S, _ptr(roots), r2, _ptr(nbr)))
        return nbr
    out = torch.full((S, K), -1, dtype=torch.int32, device=roots.device)
    inf = torch.tensor(math.inf, dtype=torch.float32, device=roots.device)
    for lo in range(0, S, _ROWS):
        q = roots[lo:lo + _ROWS]
        dx, dy, dz = (roots[None, :, c] - q[:, None, c] for c in range(3))
        d2 = ((dx * dx) + (dy * dy)) + (dz * dz)
        rows = torch.arange(q.shape[0], device=roots.device)
        d2[rows, rows + lo] = inf  # a root is not its own neighbour; a candidate at +inf or NaN is never taken
        d, j = torch.sort(d2, dim=1, stable=True)
        d, j = d[:, :K], j[:, :K]
        keep = (d < inf) & ~(d > r2)
        out[lo:lo + _ROWS, :d.shape[1]] = torch.where(keep, j, torch.full_like(j, -1)).to(torch.int32)
    return out


def inverted_lists(nbr: torch.Tensor):
    """``nbr [S, 4]`` -> ``start [S + 1]``, ``list``: per strand the entries ``4 t + k`` with ``nbr[t][k] == s``, ascending (integer
    torch ops; a stable sort keeps the entries of one strand in ascending order)."""
    S = int(nbr.shape[0])
    flat = nbr.reshape(-1).to(torch.int64)
    e = torch.nonzero(flat >= 0).reshape(-1)
    chosen = flat[e]
    order = torch.sort(chosen, stable=True).indices
    counts = torch.bincount(chosen, minlength=S)[:S] if S > 0 else torch.zeros(0, dtype=torch.int64, device=nbr.device)
    start = torch.zeros(S + 1, dtype=torch.int64, device=nbr.device)
    start[1:] = torch.cumsum(counts, 0)
    return start.to(torch.int32), e[order].to(torch.int32).contiguous()


class _ShapeTerms(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dirs, shape):
        from .diff_gaussian_rasterization import _on_device, _ptr, _stream
        dirs = dirs.contiguous()
        S, n = shape.S, int(dirs.shape[1])
        partial = torch.empty((S, 3), dtype=torch.float32, device=dirs.device)
        E = torch.empty(3, dtype=torch.float32, device=dirs.device)  # (every element is written)
        with _on_device(dirs.device):
            _lib.check(_lib.lib().ghr_shape_forward(_stream(), S, n, _ptr(dirs), _ptr(shape.rest), _ptr(shape.nbr), shape.M,
                                                    _ptr(partial), _ptr(E)))
        ctx.shape = shape
        ctx.save_for_backward(dirs)
        return E

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dE):
        from .diff_gaussian_rasterization import _on_device, _ptr, _stream
        (dirs,) = ctx.saved_tensors
        shape = ctx.shape
        dE = dE.contiguous().float()
        d_dirs = torch.empty_like(dirs)
        lists = shape.list if shape.list.numel() else shape.list.new_zeros(1)  # (an empty list still needs an address)
        with _on_device(dirs.device):
            _lib.check(_lib.lib().ghr_shape_backward(_stream(), shape.S, int(dirs.shape[1]), _ptr(dirs), _ptr(shape.rest), _ptr(shape.nbr),
                                                     _ptr(shape.start), _ptr(lists), shape.M, _ptr(dE), _ptr(d_dirs)))
        return d_dirs, None


class StrandShape:
    def __init__(self, origins, dirs, neighbours=4, radius=None, rest=None, weights=(1.0, 1.0, 1.0), fused: bool = True):
        if int(neighbours) != K:
            raise ValueError("StrandShape: neighbours must be 4 (the kernels' K), got %r" % (neighbours,))
        if dirs.dim() != 3 or dirs.shape[-1] != 3 or dirs.shape[1] < 1:
            raise ValueError("StrandShape: dirs must be [S, n, 3] with n >= 1, got %s" % (tuple(dirs.shape),))
        roots = origins.detach().reshape(-1, 3)
        if roots.shape[0] != dirs.shape[0]:
            raise ValueError("StrandShape: %d roots for %d strands" % (roots.shape[0], dirs.shape[0]))
        if len(weights) != 3:
            raise ValueError("StrandShape: three weights (stretch, bend, coherence), got %r" % (weights,))
        dev = dirs.device
        self.S, self.n = int(dirs.shape[0]), int(dirs.shape[1])
        self.fused = bool(fused)
        self.radius = radius
        if rest is None:
            rest = torch.linalg.vector_norm(dirs.detach().double(), dim=-1).mean(dim=1)
        rest = torch.as_tensor(rest, device=dev).detach().reshape(-1).to(torch.float32).contiguous()
        if rest.shape[0] != self.S or not bool((rest > 0).all()):
            raise ValueError("StrandShape: rest must hold one positive length per strand")
        self.rest = rest
        self.nbr = nearest_roots(roots.to(dev), radius, fused=self.fused).contiguous()
        self.start, self.list = inverted_lists(self.nbr)
        self.M = int((self.nbr >= 0).sum())  # once per model: the only host read
        self.weights = torch.tensor([float(w) for w in weights], dtype=torch.float32, device=dev)

    @classmethod
    def from_model(cls, hair, **kw):
        """over a strand model's roots ``pts_origins`` and its segment vectors ``_dirs`` as they are now"""
        return cls(hair.pts_origins, hair._dirs, **kw)

    def divisors(self, n=None):
        n = self.n if n is None else int(n)
        return float(self.S * n), float(self.S * (n - 1)) if n > 1 else 0.0, float(n * self.M) if self.M > 0 else 0.0

    def terms(self, dirs: torch.Tensor) -> torch.Tensor:
        if dirs.dim() != 3 or int(dirs.shape[0]) != self.S or dirs.shape[-1] != 3 or dirs.shape[1] < 1:
            raise ValueError("StrandShape: dirs must be [%d, n, 3], got %s" % (self.S, tuple(dirs.shape)))
        if dirs.device != self.rest.device:  # (the kernels would be handed the tables' addresses on another device)
            raise ValueError("StrandShape: dirs on %s, the tables on %s: build the term on the device it is evaluated on"
                             % (dirs.device, self.rest.device))
        if self.fused and _fusable(dirs):
            if self.S == 0:
                return dirs.sum() * torch.zeros(3, device=dirs.device)
            return _ShapeTerms.apply(dirs, self)
        return self.terms_composed(dirs)

    def terms_composed(self, dirs: torch.Tensor) -> torch.Tensor:
        """The definition in torch ops of ``dirs``' dtype, torch's reductions; the dead rule is decided in ``dirs``' dtype too."""
        d = dirs
        S, n = self.S, int(d.shape[1])
        dt = d.dtype
        rest = self.rest.to(dt)[:, None]
        div = self.divisors(n)
        zero = d.sum() * 0.0
        if S == 0:
            return torch.stack([zero, zero, zero])
        sq = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        pos = sq > 0
        length = torch.where(pos, torch.sqrt(torch.where(pos, sq, torch.ones_like(sq))), torch.zeros_like(sq))
        E0 = (length / rest - 1.0).square().sum() / div[0]
        E1 = zero
        if n > 1:
            e = d[:, 1:] - d[:, :-1]
            E1 = ((((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])) / (rest * rest)).sum() / div[1]
        E2 = zero
        if self.M > 0:
            alive = length.detach() > torch.tensor(DEAD, dtype=torch.float32).to(dt).to(d.device) * rest
            u = torch.where(alive[..., None], d / torch.where(alive, length, torch.ones_like(length))[..., None], torch.zeros_like(d))
            valid = self.nbr >= 0
            ut = u[self.nbr.clamp(min=0).long()]                                   # [S, 4, n, 3]
            dot = (u[:, None, :, 0] * ut[..., 0] + u[:, None, :, 1] * ut[..., 1]) + u[:, None, :, 2] * ut[..., 2]
            E2 = ((1.0 - dot) * valid[:, :, None].to(dt)).sum() / div[2]
        return torch.stack([E0, E1, E2])

    def __call__(self, dirs: torch.Tensor) -> torch.Tensor:
        t = self.terms(dirs)
        return (self.weights.to(t.dtype) * t).sum()


def smooth_polylines(points: torch.Tensor, iterations: int, lr=None, fused: bool = True, shape=None, **kw) -> torch.Tensor:
    """``iterations`` Adam steps on the shape term alone over the polylines ``points [S, L, 3]``: the roots stay, the segment
    vectors move.  ``lr`` defaults to a hundredth of the mean rest length (Adam moves an element by about ``lr`` a step); ``kw``
    goes to ``StrandShape``, unless ``shape`` is one built over these polylines already.  Returns the new points (a way to see
    the term act without training).  The term knows no head mesh: points may move towards it."""
    if points.dim() != 3 or points.shape[-1] != 3 or points.shape[1] < 2:
        raise ValueError("smooth_polylines: points must be [S, L, 3] with L >= 2, got %s" % (tuple(points.shape),))
    pts = points.detach().float()
    origins = pts[:, :1]
    dirs = (pts[:, 1:] - pts[:, :-1]).contiguous().requires_grad_(True)
    if int(iterations) < 1 or pts.shape[0] == 0:
        return pts.clone()
    if shape is None:
        shape = StrandShape(origins, dirs, fused=fused, **kw)
    o = torch.optim.Adam([dirs], lr=float(shape.rest.mean()) * 0.01 if lr is None else float(lr))
    for _ in range(int(iterations)):
        o.zero_grad(set_to_none=True)
        shape(dirs).backward()
        o.step()
    with torch.no_grad():
        return torch.cat([origins, origins + torch.cumsum(dirs, dim=1)], dim=1)
