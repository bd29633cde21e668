"""Shapes, clouds and argument combinations shared by tests/test_chamfer_cpu.py, tests/test_gpu_chamfer.py and
tests/golden/make_reference_chamfer_golden.py (gaussianhaircut_amd/nearest.py, utils/loss_chamfer_utils.py).

SIZES: 64 is a block of the search, 4096 a superblock; one off on either side of each, the smallest clouds, and 8193 (two
superblocks and a block of one point).  Every (Px, Py) of SIZES x SIZES is a case of every cloud kind.

Cloud kinds (``cloud(kind, Px, Py)`` -> float32 CPU tensors x [Px, 3], y [Py, 3], and the expected idx where the kind fixes it):
  uniform     both uniform in [-1, 1]^3
  strands     polylines of 33 points, 0.01 apart; x is y's construction moved by less than a segment
  outside     x entirely outside y's bounding box: the seed is poor and every lane starts far away
  duplicates  y repeats ceil(Py / 3) base points (so y[j], y[j + nb], y[j + 2 nb] are equal), x[i] = y[i mod Py]: distance 0 and
              the index of the LOWEST duplicate
  lattice     y: distinct points of an integer lattice in a shuffled order, x: lattice points moved by 0.5 along 1, 2 or 3 axes,
              where 2, 4 or 8 candidates tie exactly in fp32 (all coordinates are small multiples of 0.5); the lowest index wins
  onecell     everything but one far point shares one Morton cell: all those keys are equal and the seed is block 0
TIE_KINDS are those where equal distances occur by construction; the others are random and tie-free for practical purposes.
"""
import itertools
import os

import numpy as np
import torch

SIZES = (1, 2, 63, 64, 65, 4095, 4096, 4097, 8193)
SMALL_SIZES = (1, 2, 63, 64, 65)   # what the CPU tests brute-force
KINDS = ("uniform", "strands", "outside", "duplicates", "lattice", "onecell")
TIE_KINDS = ("duplicates", "lattice")
SHAPES = tuple(itertools.product(SIZES, SIZES))
SMALL_SHAPES = tuple(itertools.product(SMALL_SIZES, SMALL_SIZES))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_chamfer_golden.npz")


def _gen(kind, Px, Py):
    return torch.Generator().manual_seed(1000003 * KINDS.index(kind) + 8209 * Px + Py)


def _polyline_points(n, g):
    strands = (n + 32) // 33
    roots = torch.rand(strands, 3, generator=g) * 0.2
    dirs = torch.nn.functional.normalize(torch.randn(strands, 3, generator=g), dim=1)
    curl = torch.randn(strands, 3, generator=g) * 0.002
    t = torch.arange(33, dtype=torch.float32)[None, :, None]
    pts = roots[:, None] + 0.01 * t * dirs[:, None] + curl[:, None] * torch.sin(0.4 * t)
    return pts.reshape(-1, 3)[:n].contiguous()


def cloud(kind, Px, Py):
    """-> dict(x, y, idx): idx is the expected int64 [Px] answer for 'duplicates', None otherwise."""
    g = _gen(kind, Px, Py)
    idx = None
    if kind == "uniform":
        x, y = torch.rand(Px, 3, generator=g) * 2 - 1, torch.rand(Py, 3, generator=g) * 2 - 1
    elif kind == "strands":
        pts = _polyline_points(max(Px, Py), g)
        y = pts[:Py].clone()
        x = pts[:Px] + torch.tensor([0.004, -0.002, 0.001])
    elif kind == "outside":
        x, y = torch.rand(Px, 3, generator=g) + 10.0, torch.rand(Py, 3, generator=g) * 2 - 1
    elif kind == "duplicates":
        nb = (Py + 2) // 3
        base = torch.rand(nb, 3, generator=g) * 2 - 1
        j = torch.arange(Py)
        y = base[j % nb]
        i = torch.arange(Px) % Py
        x = y[i]
        idx = (i % nb).to(torch.int64)
    elif kind == "lattice":
        n = 2
        while n ** 3 < Py:
            n += 1
        cells = torch.randperm(n ** 3, generator=g)[:Py]
        y = torch.stack((cells // (n * n), (cells // n) % n, cells % n), dim=1).to(torch.float32)
        i = torch.arange(Px)
        moves = torch.tensor([[0.5, 0.0, 0.0], [0.5, 0.5, 0.0], [0.5, 0.5, 0.5], [0.0, 0.5, 0.5]])
        x = y[i % Py] + moves[i % 4]
    elif kind == "onecell":
        x, y = torch.rand(Px, 3, generator=g) * 0.4, torch.rand(Py, 3, generator=g) * 0.4
        if Py >= 2:
            y[-1] = 1.0e6
        elif Px >= 2:
            x[-1] = 1.0e6
    else:
        raise KeyError(kind)
    return dict(x=x.contiguous(), y=y.contiguous(), idx=idx)


def normals_for(P, seed):
    g = torch.Generator().manual_seed(77 + seed)
    return torch.randn(P, 3, generator=g)


def brute_rule(x, y, norm):
    """The stated rule in numpy float32, one query at a time: smallest d, then lowest index.  For small clouds only."""
    x, y = x.numpy().astype(np.float32), y.numpy().astype(np.float32)
    dist, idx = np.zeros(len(x), np.float32), np.zeros(len(x), np.int64)
    for i in range(len(x)):
        dx, dy, dz = y[:, 0] - x[i, 0], y[:, 1] - x[i, 1], y[:, 2] - x[i, 2]
        d = (dx * dx + dy * dy) + dz * dz if norm == 2 else (np.abs(dx) + np.abs(dy)) + np.abs(dz)
        best = 0
        for j in range(1, len(y)):
            if d[j] < d[best]:
                best = j
        dist[i], idx[i] = d[best], best
    return dist, idx


# ---- the golden's argument combinations ------------------------------------------------------------------------------------------
GOLDEN_N, GOLDEN_P1, GOLDEN_P2, GOLDEN_C = 2, 97, 130, 5
GOLDEN_LENGTHS = ((97, 61), (130, 88))
# name -> (uses: subset of "nwvfl" = normals, both weights, y_weights only, features, lengths; keyword arguments)
GOLDEN_CASES = {
    "defaults": ("", {}),
    "single": ("", dict(single_directional=True)),
    "normals": ("n", {}),
    "normals_signed": ("n", dict(abs_cosine=False)),
    "l1": ("", dict(norm=1)),
    "weights": ("w", {}),
    "y_weights_only": ("v", {}),
    "lengths_normals": ("nl", {}),
    "per_point": ("nl", dict(point_reduction=None, batch_reduction=None)),
    "sum_sum": ("n", dict(point_reduction="sum", batch_reduction="sum")),
    "per_cloud": ("nw", dict(batch_reduction=None)),
    "everything": ("nwfl", {}),
    "l1_sum_mean": ("nw", dict(norm=1, point_reduction="sum")),
}
GOLDEN_ERRORS = {
    "zero_x_weights": ("zx", {}),
    "zero_y_weights": ("zy", dict(point_reduction=None, batch_reduction=None)),
}
TERM_COEFF = (1.0, 0.5, 0.25)   # the scalar that is differentiated: sum over terms and directions of coeff * term.sum()


def golden_inputs():
    """Seeded float32 inputs of the golden (the .npz stores them too; this is how they were made)."""
    g = torch.Generator().manual_seed(20240607)
    N, P1, P2, C = GOLDEN_N, GOLDEN_P1, GOLDEN_P2, GOLDEN_C
    return dict(x=torch.rand(N, P1, 3, generator=g), y=torch.rand(N, P2, 3, generator=g),
                x_normals=torch.randn(N, P1, 3, generator=g), y_normals=torch.randn(N, P2, 3, generator=g),
                x_features=torch.randn(N, P1, C, generator=g), y_features=torch.randn(N, P2, C, generator=g),
                x_weights=torch.rand(N, P1, generator=g) + 0.25, y_weights=torch.rand(N, P2, generator=g) + 0.25)


def golden_kwargs(uses, inp, dtype, device="cpu", requires_grad=True):
    """The tensors one case passes to chamfer_distance, fresh copies in ``dtype`` (weights are modified in place)."""
    def t(name, grad):
        v = inp[name].to(device=device, dtype=dtype).clone()
        return v.requires_grad_(True) if grad and requires_grad else v

    kw = dict(x=t("x", True), y=t("y", True))
    if "n" in uses:
        kw.update(x_normals=t("x_normals", True), y_normals=t("y_normals", True))
    if "f" in uses:
        kw.update(x_features=t("x_features", False), y_features=t("y_features", False))
    if "w" in uses:
        kw.update(x_weights=t("x_weights", False), y_weights=t("y_weights", False))
    if "v" in uses:
        kw.update(y_weights=t("y_weights", False))
    if "l" in uses:
        kw.update(x_lengths=torch.tensor(GOLDEN_LENGTHS[0], device=device), y_lengths=torch.tensor(GOLDEN_LENGTHS[1], device=device))
    if "zx" in uses:
        kw.update(x_weights=torch.zeros_like(t("x_weights", False)))
    if "zy" in uses:
        kw.update(x_weights=t("x_weights", False), y_weights=torch.zeros_like(t("y_weights", False)))
    return kw


def scalar_of(result):
    """The differentiated scalar: every distance / normals / features term of both directions, summed with TERM_COEFF."""
    total = 0.0
    for pair, c in zip(result[:3], TERM_COEFF):
        for term in pair:
            if term is not None:
                total = total + c * term.sum()
    return total


def reduce64(t, w, lengths, point_reduction, batch_reduction):
    """The reduction pipeline in float64 numpy on per-point magnitudes t [N, P] (weights already inside t); w: the direction's
    multiplied weights or None."""
    if point_reduction is None:
        return t
    t = t.sum(1)
    if point_reduction == "mean":
        t = t / np.maximum(lengths, 1)
    if batch_reduction is not None:
        t = t.sum()
        if batch_reduction == "mean":
            t = t / (w.sum() if w is not None else max(len(lengths), 1))
    return t


def load_golden():
    z = np.load(GOLDEN, allow_pickle=False)
    return {k: z[k] for k in z.files}
