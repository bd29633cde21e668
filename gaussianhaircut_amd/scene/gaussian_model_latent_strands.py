"""Module path of the reference's ``src/scene/gaussian_model_latent_strands.py``, which defines ``GaussianModelHair``
(imported by its ``scene/__init__.py:18``, ``gaussian_renderer/__init__.py:17`` and ``train_latent_strands.py:21``;
``GaussianModelCurves`` is the class of ``gaussian_model_strands.py``).

The Gaussian side of the latent-strand stage.  The strand prior that decodes a latent texture into polylines is out of scope
(DESIGN 8): here it is any callable ``generator(iteration) -> dict`` (``strand_generator.TexturedStrands`` is one, with
the networks left to the caller: DESIGN 8p).  What the reference does with the generator's
output at the top of every iteration (:451-499) is in scope and fused (csrc/ghr_latent.h):
  * points ``p [S, L, 3]`` -> ``_xyz / _rotation / _scaling / _dir`` of the ``S (L - 1)`` segment Gaussians, one kernel each way;
  * per-strand appearance ``repeat``-ed over the segments, one kernel each way (the backward sums a strand's rows in order).
On a non-ROCm device, or with ``fused=False``, the same tensors come from the PyTorch expressions of the reference.

``shared_appearance=True`` (or ``GHR_LATENT_SHARED_FEATURES=1``; off by default) goes one step further for per-strand SH
features on a ROCm device: they are not expanded at all.  ``_features_dc`` / ``_features_rest`` stay ``[S, ., 3]``,
``feature_rows_per_strand`` says how many Gaussians share a row, and ``render_hair`` projects them with the kernels of
csrc/ghr_shared.h, whose backward returns the per-strand gradients directly.  ``get_features`` still returns ``[P, K, 3]``."""
from __future__ import annotations

import os

import torch

from .. import _lib
from ..utils.general_utils import parallel_transport
from .gaussian_model_strands import GaussianModelStrands

FUSED_LATENT_BUILD = os.environ.get("GHR_FUSED_LATENT_BUILD", "1") != "0"
SHARED_FEATURES = os.environ.get("GHR_LATENT_SHARED_FEATURES", "0") == "1"


def _fusable(t) -> bool:
    return t.is_cuda and t.dtype == torch.float32


class _PointsBuild(torch.autograd.Function):
    """points [S,L,3] -> xyz [P,3], rotation [P,4], scaling [P,3], direction rows [P,3] of the P = S (L-1) segment Gaussians."""

    @staticmethod
    def forward(ctx, p, scale):
        from ..diff_gaussian_rasterization import _on_device, _ptr, _stream
        p = p.contiguous()
        S, L = int(p.shape[0]), int(p.shape[1])
        P = S * (L - 1)
        f32 = dict(dtype=torch.float32, device=p.device)
        xyz, rot, scaling, rows = (torch.empty((P, 3), **f32), torch.empty((P, 4), **f32), torch.empty((P, 3), **f32),
                                   torch.empty((P, 3), **f32))
        with _on_device(p.device):
            _lib.check(_lib.lib().ghr_strand_points_build(_stream(), S, L, _ptr(p), float(scale), _ptr(xyz), _ptr(rot),
                                                          _ptr(scaling), _ptr(rows)))
        ctx.save_for_backward(p)
        ctx.set_materialize_grads(False)  # an output nobody differentiated arrives as None (the kernel takes NULL)
        return xyz, rot, scaling, rows

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_xyz, d_rot, d_scaling, d_rows):
        from ..diff_gaussian_rasterization import _on_device, _ptr, _stream
        (p,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0] or (d_xyz is None and d_rot is None and d_scaling is None and d_rows is None):
            return None, None
        S, L = int(p.shape[0]), int(p.shape[1])
        cots = [None if g is None else g.contiguous().float() for g in (d_xyz, d_rot, d_scaling, d_rows)]
        d_p = torch.empty_like(p)
        with _on_device(p.device):
            _lib.check(_lib.lib().ghr_strand_points_build_backward(_stream(), S, L, _ptr(p),
                                                                   *[None if g is None else _ptr(g) for g in cots], _ptr(d_p)))
        return d_p, None


class _RowsExpand(torch.autograd.Function):
    """src [S,C] -> [S n_seg, C], every strand's row repeated over its segments; backward: the in-order sum of a strand's rows."""

    @staticmethod
    def forward(ctx, src, n_seg):
        from ..diff_gaussian_rasterization import _on_device, _ptr, _stream
        src = src.contiguous()
        S, C = int(src.shape[0]), int(src.shape[1])
        dst = torch.empty((S * n_seg, C), dtype=torch.float32, device=src.device)
        with _on_device(src.device):
            _lib.check(_lib.lib().ghr_strand_rows_expand(_stream(), S, int(n_seg), C, _ptr(src), _ptr(dst)))
        ctx.shape = (S, int(n_seg), C)
        return dst

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from ..diff_gaussian_rasterization import _on_device, _ptr, _stream
        S, n_seg, C = ctx.shape
        g = g.contiguous().float()
        out = torch.empty((S, C), dtype=torch.float32, device=g.device)
        with _on_device(g.device):
            _lib.check(_lib.lib().ghr_strand_rows_reduce(_stream(), S, n_seg, C, _ptr(g), _ptr(out)))
        return out, None


def expand_rows(src, n_seg: int, fused: bool = True):
    """``src.view(S, 1, C).repeat(1, n_seg, 1).view(-1, C)`` (:465-467)."""
    if fused and _fusable(src):
        return _RowsExpand.apply(src, int(n_seg))
    S, C = src.shape
    return src.view(S, 1, C).repeat(1, n_seg, 1).reshape(S * n_seg, C)


def build_from_points(p, scale: float, fused: bool = True):
    """(xyz, rotation, scaling, dir) of the segment Gaussians of the polylines ``p [S, L, 3]`` (:451-452, 490-499, 110-115)."""
    if fused and _fusable(p):
        return _PointsBuild.apply(p, float(scale))
    xyz = (p[:, 1:] + p[:, :-1]).reshape(-1, 3) * 0.5
    d = (p[:, 1:] - p[:, :-1]).reshape(-1, 3)
    x_axis = torch.cat([torch.ones_like(xyz[:, :1]), torch.zeros_like(xyz[:, :2])], dim=-1)
    rot = parallel_transport(x_axis, d).view(-1, 4)
    scaling = torch.cat([d.norm(dim=-1, keepdim=True) * 0.5, torch.ones_like(xyz[:, :2]) * scale], dim=-1)
    return xyz, rot, scaling, d


class GaussianModelLatentStrands(GaussianModelStrands):
    """Owns no strand parameters: ``generator(iteration)`` returns a dict with
      ``points`` [S, L, 3]; ``features`` [S, K 3] (per strand) or [S (L-1), K 3] (per segment), split ``dc | rest`` as the
      reference splits ``z_app``; optional ``orient_conf`` (log space, [S, 1] or [S (L-1), 1]); optional ``L_diff``.
    ``color_decoder`` is whatever module the caller wants in the checkpoint next to the generator (it may be None)."""

    def __init__(self, sh_degree: int, generator=None, color_decoder=None, scale: float = 1e-3, fused: bool = True,
                 shared_appearance: bool = False, num_guiding_strands=None):
        super().__init__(sh_degree, scale=scale)
        if num_guiding_strands is None:  # the generator's own setting (strand_generator.TexturedStrands has one), else none
            num_guiding_strands = getattr(generator, "num_guiding_strands", 0)
        self.num_guiding_strands = int(num_guiding_strands or 0)
        self.shared_appearance = bool(shared_appearance) or SHARED_FEATURES
        self.feature_rows_per_strand = 0  # > 1: _features_dc / _features_rest hold one row per STRAND (set by _split)
        self.active_sh_degree = self.max_sh_degree  # the reference's constructor (:64)
        self.strands_generator = generator
        self.color_decoder = color_decoder
        self.fused = bool(fused)
        self.scheduler = None
        self.LDiff = None
        self.num_strands = self.strand_length = 0

    def _split(self, out):
        K3 = 3 * (self.max_sh_degree + 1) ** 2
        S, n_seg = self.num_strands, self.strand_length - 1
        feats = out["features"]
        if feats.dim() != 2 or feats.shape[1] != K3 or feats.shape[0] not in (S, S * n_seg):
            raise ValueError("features must be [S, %d] or [S (L-1), %d], got %s" % (K3, K3, tuple(feats.shape)))
        fused = self.fused and FUSED_LATENT_BUILD
        dc, rest = feats[:, :3], feats[:, 3:]
        self.feature_rows_per_strand = 0
        if feats.shape[0] == S and n_seg > 1 and self.shared_appearance and fused and _fusable(feats):
            # per strand and kept so: the projection indexes them by strand (csrc/ghr_shared.h), its backward returns [S, ., 3]
            self.feature_rows_per_strand = n_seg
            self._features_dc = dc.reshape(S, 1, 3)
            self._features_rest = rest.reshape(S, (self.max_sh_degree + 1) ** 2 - 1, 3)
        elif feats.shape[0] == S and n_seg > 1:
            # per strand (one segment a strand: both readings are the same rows).  Split first, on the [S, K 3] rows, so that each
            # expanded tensor is contiguous and its gradient reaches the reduce without a slice's zero-padded copy
            dc, rest = expand_rows(dc, n_seg, fused), expand_rows(rest, n_seg, fused)
        if self.feature_rows_per_strand == 0:
            self._features_dc = dc.reshape(S * n_seg, 1, 3)
            self._features_rest = rest.reshape(S * n_seg, (self.max_sh_degree + 1) ** 2 - 1, 3)
        conf = out.get("orient_conf")
        if conf is None:
            conf = torch.zeros((S * n_seg, 1), dtype=feats.dtype, device=feats.device)
        elif conf.shape[0] == S and n_seg > 1:
            conf = expand_rows(conf.reshape(S, 1), n_seg, fused)
        self._orient_conf = conf.reshape(S * n_seg, 1)

    def _split_guiding(self):
        """:456-461, :477-482: the first ``num_guiding_strands`` strands' rows as views (the full tensors without guiding);
        per-strand feature storage keeps one row per guide."""
        N = min(self.num_guiding_strands, self.num_strands)
        if N == 0:
            self._xyz_gdn, self._dir_gdn = self._xyz, self._dir
            self._features_dc_gdn, self._features_rest_gdn = self._features_dc, self._features_rest
            return
        n_seg = self.strand_length - 1
        self._xyz_gdn, self._dir_gdn = self._xyz[:N * n_seg], self._dir[:N * n_seg]
        rows = N if self.feature_rows_per_strand > 1 else N * n_seg
        self._features_dc_gdn, self._features_rest_gdn = self._features_dc[:rows], self._features_rest[:rows]

    @property
    def get_features_gdn(self):
        """:132-135: ``[rows, K, 3]`` of the guiding strands, in the storage ``_features_dc_gdn`` has"""
        return torch.cat((self._features_dc_gdn, self._features_rest_gdn), dim=1)

    @property
    def get_features(self):
        """[P, K, 3] whatever the storage: per-strand rows are ``repeat``-ed (:465-467) for the generic render path and any
        other reader."""
        f = torch.cat((self._features_dc, self._features_rest), dim=1)
        n = self.feature_rows_per_strand
        if n > 1:
            S, K = f.shape[0], f.shape[1]
            f = f.view(S, 1, K, 3).repeat(1, n, 1, 1).reshape(S * n, K, 3)
        return f

    def initialize_gaussians_hair(self, iteration=0, num_strands=-1):
        """:451-499: call the generator, build the segment Gaussians, expand per-strand appearance, set ``LDiff``."""
        out = self.strands_generator(iteration)
        p = out["points"]
        if p.dim() != 3 or p.shape[-1] != 3 or p.shape[1] < 2:
            raise ValueError("points must be [S, L >= 2, 3], got %s" % (tuple(p.shape),))
        self.num_strands, self.strand_length = int(p.shape[0]), int(p.shape[1])
        self.__dict__.pop("_pts_value", None)
        self._pts = p
        self._xyz, self._rotation, self._scaling, self._dir = build_from_points(p, self.scale, self.fused and FUSED_LATENT_BUILD)
        self._split(out)
        self._split_guiding()
        self.LDiff = out.get("L_diff")
        return out

    def _modules(self):
        return self.strands_generator, self.color_decoder

    def capture(self):
        """The reference's six slots (:84-92)."""
        gen, dec = self._modules()
        sd = lambda m: m.state_dict() if hasattr(m, "state_dict") else None  # noqa: E731
        return (self._scaling, self.active_sh_degree, sd(gen), sd(dec),
                self.optimizer.state_dict() if self.optimizer is not None else None,
                self.scheduler.state_dict() if self.scheduler is not None else None)

    def restore(self, model_args, training_args=None):
        """:94-107."""
        self._scaling, self.active_sh_degree, gen_dict, clr_dict, opt_dict, shd_dict = model_args
        gen, dec = self._modules()
        if gen_dict is not None:
            gen.load_state_dict(gen_dict)
        if clr_dict is not None and dec is not None:
            dec.load_state_dict(clr_dict)
        if training_args is not None:
            self.training_setup(training_args)
        if opt_dict is not None and self.optimizer is not None:
            self.optimizer.load_state_dict(opt_dict)
        if shd_dict is not None and self.scheduler is not None:
            self.scheduler.load_state_dict(shd_dict)

    def training_setup(self, training_args, training_args_hair=None):
        """:517-519: AdamW over the generator's and the colour decoder's parameters, cosine schedule down to 1e-4."""
        lr = training_args_hair["general"]["lr"] if training_args_hair is not None else getattr(training_args, "latent_lr", 1e-3)
        params = [q for m in self._modules() if hasattr(m, "parameters") for q in m.parameters()]
        self.optimizer = torch.optim.AdamW(params, lr)
        self.scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(self.optimizer, T_max=training_args.iterations, eta_min=1e-4)

    def update_learning_rate(self, iteration):
        """:611-612 of the reference: the scheduler's step is the learning-rate update of this stage."""
        if self.scheduler is not None:
            self.scheduler.step()


GaussianModelHair = GaussianModelLatentStrands  # the reference's class name in THIS module
