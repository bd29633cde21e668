"""Inputs, the float64 reference and the acceptance criteria of the per-pixel tests of the fused loss (csrc/ghr_loss.h).
CPU only: plain PyTorch, nothing of the kernels.  Used by tests/test_loss_cases_cpu.py (which shows that the reference itself,
run in float32, sits far inside the bars) and by tests/test_gpu_loss_shapes.py (the kernels against it).

The shape table.  Both forms of every kernel place things by tiles, halos, strips, row batches and segments; each shape is the
smallest at which one of those decisions goes another way.

Marching form (W % 4 == 0: one wave per 32-column strip and segment of 32 rows, 8 output rows per pass, a window of twelve
float4 per row = columns bx-8 .. bx+39, the first batch of a segment = the ten rows above it):
  (1, 4)    one row and one float4: of the first pass's 18 input rows one is inside the image, every row batch but one outside
  (3, 8)    image no taller than the window radius: the ten rows above AND the five below a pixel's rows are padding
  (5, 12)   the same at exactly the radius
  (8, 28)   exactly one pass; a strip under 32 columns whose right halo (columns 28..39) lies inside the aligned window but
            outside the image
  (9, 32)   one row into a second pass; one full strip whose right halo is all outside
  (11, 36)  a second strip of one float4 whose left halo is real data
  (32, 64)  exactly one segment and two full strips
  (33, 64)  a second segment of one row; its ten rows above belong to the other segment (read, filtered, but not `own`: the
            L1 term must count them once)
  (40, 68)  a second segment of one pass; three strips, the last of one float4
  (9, 260)  nine strips on a grid padded to 16: the strip-to-XCD remap has empty strips between used ones
  (20, 36)  the segment-length test's own shape: at 8 rows per segment three segments, the last of half a pass

Tile form (any W; 32 x 16 tiles with a 5-pixel halo):
  (1, 1)    smallest image
  (6, 5)    image smaller than the window
  (10, 11)  image about the size of the window
  (16, 33)  a second tile of one column
  (17, 31)  a second tile row of one row
  (26, 42)  exactly a tile plus its halo

The criteria.  Gradients are compared per element, per channel group, and with the `special` pixels (zero direction and zero
confidence, as the rasterizer leaves at empty pixels) as a group of their own: there the reference's confidence gradient is
-(1 / 1e-7) * m, about 1e7 times the scale factor, against at most about 23 times it where conf >= 0.05 -- one `max|ref|` over
the whole plane is a bar two thousand times the ordinary values."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from gaussianhaircut_amd.gaussian_renderer import orient_angle_from
from gaussianhaircut_amd.utils import loss_utils as lu

MARCH_SHAPES = ((1, 4), (3, 8), (5, 12), (8, 28), (9, 32), (11, 36), (32, 64), (33, 64), (40, 68), (9, 260))
TILE_SHAPES = ((1, 1), (6, 5), (10, 11), (16, 33), (17, 31), (26, 42))
SEGMENT_SHAPES = ((20, 36), (33, 64), (40, 68))
ALL_SHAPES = MARCH_SHAPES + TILE_SHAPES + ((20, 36),)
# what a shape has to be for its row of the table above to hold (checked by test_loss_cases_cpu.py):
# marching: (strips, grid columns, segments at 32 rows, rows of the last segment, columns of the last strip)
MARCH_GEOMETRY = {(1, 4): (1, 8, 1, 1, 4), (3, 8): (1, 8, 1, 3, 8), (5, 12): (1, 8, 1, 5, 12), (8, 28): (1, 8, 1, 8, 28),
                  (9, 32): (1, 8, 1, 9, 32), (11, 36): (2, 8, 1, 11, 4), (32, 64): (2, 8, 1, 32, 32), (33, 64): (2, 8, 2, 1, 32),
                  (40, 68): (3, 8, 2, 8, 4), (9, 260): (9, 16, 1, 9, 4), (20, 36): (2, 8, 1, 20, 4)}
# tile: (tile columns, tile rows, columns of the last tile, rows of the last tile)
TILE_GEOMETRY = {(1, 1): (1, 1, 1, 1), (6, 5): (1, 1, 5, 6), (10, 11): (1, 1, 11, 10), (16, 33): (2, 1, 1, 16),
                 (17, 31): (1, 2, 31, 1), (26, 42): (2, 2, 10, 10)}
# The seed of a case is 7 H + W unless listed here.  A seed may be changed by looking at the INPUTS alone: both channels of
# the binary gt_mask need a set pixel (a term that is masked away everywhere checks nothing; test_loss_cases_cpu.py asserts
# it).  No shape of the table needs another seed.
SEEDS = {}

BLENDED = (0.8, 0.2, 0.2, 0.1)
ONE_HOT = ((1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0))
WEIGHTS = (BLENDED,) + ONE_HOT

GRAD_BAR = 2e-4      # of a group's max|ref|: the project's gradient bar
VALUE_BAR = 5e-6     # of max(1, |ref|): the project's bar for the stage-1 loss
STATS_ATOL = 2e-6    # the project's bar for the cached window moments
KINK = 2e-3
SAFE_DIR, SAFE_ANGLE = (0.3, 0.1), 0.15
GROUPS = (("image", (0, 1, 2)), ("mask", (3, 4)), ("dir", (5, 6)), ("conf", (8,)), ("zero planes", (7, 9)))


def seed_of(H, W):
    return SEEDS.get((H, W), 7 * H + W)


def kink_distance_mask(r, gt_angle):
    """[H, W] bool, float64 arithmetic: pixels within KINK of a point where the orientation term's gradient jumps -- the
    wrapped difference changing branch (|diff| = 0.5) or sign (diff = 0), the mirror flipping (u0 = 0), the clamp of u1
    engaging (|u1| = 0.999; from 0.997 on, 1 / sqrt(1 - u1^2) also amplifies rounding)."""
    d = r[5:7].double()
    u = d / d.norm(dim=0, keepdim=True).clamp_min(1e-12)
    angle = orient_angle_from(r[5:8].double())[0]
    a = (angle - gt_angle[0].double()).abs()
    return ((a - 0.5).abs() < KINK) | (a < KINK) | (u[0].abs() < KINK) | (u[1].abs() > 0.997)


def near_kink(case):
    """the pixels of a case that sit near a kink.  At a special pixel the direction is EXACTLY zero in every precision
    (u = 0 / eps = 0, mirror = +1, angle = 0.5: nothing is rounded, so nothing can fall on the other side) and every
    direction derivative carries the factor conf = 0; only the two criteria on the wrapped difference apply there."""
    r, gt_angle, special = case["renders"], case["gt_angle"], case["special"]
    a = (orient_angle_from(r[5:8].double())[0] - gt_angle[0].double()).abs()
    on_diff = ((a - 0.5).abs() < KINK) | (a < KINK)
    return torch.where(special, on_diff, kink_distance_mask(r, gt_angle))


def make_case(H, W, seed=None):
    """The inputs of test_fused_stage1_loss_with_orientation_matches_torch (smooth ground truth + noise, binary gt_mask)
    with gt_oconf = rand + 0.05, no pixel near a kink of the orientation term, and (H >= 6) the top H // 6 rows `special`:
    zero direction, zero confidence.  float32 CPU tensors."""
    seed = seed_of(H, W) if seed is None else seed
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(3, H // 4 + 2, W // 4 + 2, generator=g)
    gt = F.interpolate(base[None], size=(H, W), mode="bilinear")[0]
    r = torch.zeros(10, H, W)
    r[0:3] = (gt + 0.15 * torch.randn(3, H, W, generator=g)).clamp(-0.2, 1.3)
    r[3:5] = torch.rand(2, H, W, generator=g)
    r[5:8] = torch.randn(3, H, W, generator=g) * 0.3          # 2D direction (+ unused z)
    r[8] = torch.rand(H, W, generator=g) * 2 + 0.05           # orientation confidence >= 0.05
    r[9] = torch.rand(H, W, generator=g) * 5
    gt_mask = (torch.rand(2, H, W, generator=g) > 0.35).float()
    gt_angle = torch.rand(1, H, W, generator=g)
    gt_oconf = torch.rand(1, H, W, generator=g) + 0.05
    special = torch.zeros(H, W, dtype=torch.bool)
    if H >= 6:
        special[: H // 6] = True
        r[5:7, : H // 6] = 0.0
        r[8, : H // 6] = 0.0
    case = dict(H=H, W=W, seed=seed, renders=r, gt_image=gt.contiguous(), gt_mask=gt_mask, gt_angle=gt_angle,
                gt_oconf=gt_oconf, special=special)
    bad = near_kink(case)
    case["replaced"] = float(bad.float().mean())
    ordinary = bad & ~special
    r[5, ordinary], r[6, ordinary] = SAFE_DIR
    gt_angle[0, bad] = SAFE_ANGLE
    assert not bool(near_kink(case).any()), "a pixel near a kink remains"
    return case


def _terms(case, mask_colours, dtype):
    """the four terms of src/train_gaussians.py:126-140 and the gradient of EACH w.r.t. the packed render, in `dtype`"""
    r = case["renders"].to(dtype).requires_grad_(True)
    gt_image, gt_mask = case["gt_image"].to(dtype), case["gt_mask"].to(dtype)
    gt_angle, gt_oconf = case["gt_angle"].to(dtype), case["gt_oconf"].to(dtype)
    image, mask, cov2d, oconf, _ = r.split([3, 2, 3, 1, 1], dim=0)
    m = gt_mask[1:] if mask_colours else torch.ones_like(gt_mask[1:])
    l1 = lu.l1_loss(image, gt_image, mask=m)
    lssim = 1.0 - lu.ssim(image * m, gt_image * m)
    lmask = lu.l1_loss(mask, gt_mask)
    weight = torch.ones_like(gt_mask[:1]) * gt_oconf
    lo = lu.or_loss(orient_angle_from(cov2d), gt_angle, oconf, weight=weight, mask=gt_mask[:1])
    terms, grads = [], []
    for t in (l1, lssim, lmask, lo):
        if bool(torch.isnan(t)):   # train_gaussians.py:134: a NaN term is replaced by zero -- it moves nothing
            terms.append(0.0)
            grads.append(np.zeros(tuple(r.shape), dtype=np.float64))
            continue
        g, = torch.autograd.grad(t, r, retain_graph=True)
        terms.append(float(t.detach().double()))
        grads.append(g.detach().double().numpy())
    return terms, grads


_cache = {}


def composed(case, w, mask_colours, dtype=torch.float64):
    """loss, the four terms, the packed [10, H, W] gradient (float64 numpy whatever `dtype` the graph ran in)"""
    key = (case["H"], case["W"], case["seed"], bool(mask_colours), dtype, bool((case["gt_oconf"] == 0).all()))
    if key not in _cache:
        _cache[key] = _terms(case, mask_colours, dtype)
    terms, grads = _cache[key]
    loss = sum(float(wi) * t for wi, t in zip(w, terms))
    grad = sum(float(wi) * g for wi, g in zip(w, grads))
    return loss, tuple(terms), grad


def reference64(case, w, mask_colours):
    """The reference's formulas (utils/loss_utils.l1_loss, ssim, or_loss, gaussian_renderer.orient_angle_from, NaN -> 0) in
    float64 with autograd on the CPU: loss, (Ll1, Lssim, Lmask, Lorient), the packed gradient, and the window moments
    mu2 = w * y, E[y^2] = w * y^2 of the (masked) ground truth from conv2d, [3, H, W] each."""
    loss, terms, grad = composed(case, w, mask_colours, torch.float64)
    y = case["gt_image"].double() * (case["gt_mask"][1:].double() if mask_colours else 1.0)
    win = lu._window(11, 3, y)
    mu2 = F.conv2d(y[None], win, padding=5, groups=3)[0].numpy()
    e22 = F.conv2d((y * y)[None], win, padding=5, groups=3)[0].numpy()
    return dict(loss=loss, terms=terms, grad=grad, mu2=mu2, e22=e22)


def check_grad(got, ref, special, what=""):
    """Per channel group, ordinary and special pixels apart, each against ITS OWN max|ref|: every element within
    GRAD_BAR * scale; a group whose reference is all zero must be exactly zero; `got` finite everywhere.  Returns the
    largest error / scale met (for reports)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    special = np.asarray(special, dtype=bool)
    assert got.shape == ref.shape and got.shape[1:] == special.shape, (what, got.shape, ref.shape, special.shape)
    assert np.isfinite(got).all(), (what, "not finite at", np.argwhere(~np.isfinite(got))[:4].tolist())
    worst = 0.0
    for name, planes in GROUPS:
        for kind, sel in (("ordinary", ~special), ("special", special)):
            if not sel.any():
                continue
            x, y = got[list(planes)][:, sel], ref[list(planes)][:, sel]
            scale = np.abs(y).max()
            if scale == 0.0:
                assert not x.any(), (what, name, kind, "reference is zero, got", float(np.abs(x).max()))
                continue
            err = np.abs(x - y).max()
            assert err <= GRAD_BAR * scale, (what, name, kind, "err / scale = %.3g" % (err / scale), "scale = %.3g" % scale)
            worst = max(worst, err / scale)
    return worst


def float32_error(case, w, mask_colours):
    """{(group, "ordinary" | "special"): max|float32 - float64| / max|float64| over that group} of the composed form run in
    float32: what plain float32 arithmetic of the same formulas costs at this case.  Groups that are empty or all zero are
    left out."""
    ref = composed(case, w, mask_colours, torch.float64)[2]
    g32 = composed(case, w, mask_colours, torch.float32)[2]
    special = case["special"].numpy()
    out = {}
    for name, planes in GROUPS:
        for kind, sel in (("ordinary", ~special), ("special", special)):
            if sel.any() and np.abs(ref[list(planes)][:, sel]).max() > 0:
                x, y = g32[list(planes)][:, sel], ref[list(planes)][:, sel]
                out[(name, kind)] = float(np.abs(x - y).max() / np.abs(y).max())
    return out


def check_grad_whole_plane(got, ref):
    """The criterion check_grad replaces (one scale per group over the whole plane): kept to show what it lets through."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    for name, planes in GROUPS:
        x, y = got[list(planes)], ref[list(planes)]
        scale = max(np.abs(y).max(), 1e-30)
        if np.abs(x - y).max() > GRAD_BAR * scale:
            return False
    return True


def check_value(got, ref, what=""):
    err = abs(float(got) - float(ref))
    assert math.isfinite(float(got)) and err <= VALUE_BAR * max(1.0, abs(float(ref))), (what, float(got), float(ref), err)
    return err / max(1.0, abs(float(ref)))
