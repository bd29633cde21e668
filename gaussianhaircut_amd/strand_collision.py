"""The strand stage's collision term: a penalty on strand points inside the head mesh, or nearer to it than a
margin.  The reference has no such term -- it prunes strands after training (``between_stages.prune_strands``) and its own
creation-time test is commented out (src/scene/gaussian_model_strands.py:552-563); this one keeps the strands outside while
they are optimised.

``HeadCollision(mesh, margin, stride, fused)`` is a callable ``pts [S, L, 3] -> scalar``:

    Lpen = mean(max(margin - sd, 0)^2)  over the points  pts[:, 1:][:, ::stride]

with ``sd = mesh.signed_distance`` (negative inside; HIP forward and backward on a ROCm device, ``csrc/ghr_meshdist.h``).  The root
``pts[:, 0]`` is fixed and lies on the scalp, so it is left out.  0 when no point is taken.  The reductions are torch's.

Attach it to the strand model with ``GaussianModelStrands.attach_collision``; ``trainer.strand_training_step`` then adds
``Lpen * opt.lambda_dpen`` to the first view's loss when ``opt.lambda_dpen`` is not 0.  Unattached, nothing of this module runs.
"""
from __future__ import annotations

import torch

from .mesh import HeadMesh, signed_distance


class HeadCollision:
    def __init__(self, mesh: HeadMesh, margin: float = 0.0, stride: int = 1, fused: bool = True):
        if int(stride) < 1:
            raise ValueError("HeadCollision: stride must be >= 1, got %r" % (stride,))
        self.mesh = mesh
        self.margin = float(margin)
        self.stride = int(stride)
        self.fused = bool(fused)

    def points(self, pts: torch.Tensor) -> torch.Tensor:
        """The points the term looks at: every ``stride``-th from the first free one."""
        assert pts.dim() == 3 and pts.shape[-1] == 3, pts.shape
        return pts[:, 1:][:, ::self.stride]

    def __call__(self, pts: torch.Tensor) -> torch.Tensor:
        taken = self.points(pts)
        if taken.numel() == 0:
            return pts.sum() * 0.0  # (keeps the graph: a backward through it gives zeros)
        sd = signed_distance(taken, self.mesh, fused=self.fused)
        return torch.clamp(self.margin - sd, min=0.0).square().mean()
