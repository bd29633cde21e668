"""Inputs and checks of the synthetic ground truth (ghr_gt_from_render) that its CPU and GPU tests share.

A case is a packed [10,H,W] render: random values with a block of planted ones at its first pixels (as many as the image holds).
  colour and mask channels 0-4: ``(k + 0.5) / 255`` -- the rounding boundary of level k -- and its two float32 neighbours for
      k in 0, 1, 63, 127, 128, 200, 254, then 0, 1, a negative value and a value above 1; each channel starts the list at another
      offset, so a pixel combines different ones;
  direction channels 5-6: (0, 0), a negative x (the mirror), |y| / norm within 1e-3 of 1 on both sides (the clamp), a norm of 1e-20;
  confidence channel 8: 0, 1e-3 and 1e6 against hair values above 1.
Everything is finite, and every ``conf * hair`` is 0 or at least 1e-30 in magnitude (no subnormal product for a flush to change).

The bars.  Image, mask and confidence planes are compared bit for bit: bytes by integer-exact float32 steps (``v * 255 + 0.5``,
clamp, truncate), table values, and single correctly rounded products.  The angle plane goes through sqrt, a reciprocal and acos,
which differ between the device, the host and torch in the last places: it is held to the rule of tests/test_eval_cpu.py
against a float64 model -- an element is *fragile* when ``255 v64 + 0.5`` lies within FRAGILE_MARGIN of an integer; every other
element's level is exact, a fragile one may be off by one; on the random part of the input at most FRAGILE_SHARE of the plane
may be fragile, which ``make_packed`` guarantees by trying seeds against the float64 model until one holds (the planted
directions sit on the clamp and at zero by design and are exempt from the share, not from the one level)."""
import functools

import numpy as np
import torch

from tests.test_eval_cpu import FRAGILE_MARGIN, FRAGILE_SHARE, expected_levels

SHAPES = ((1, 1), (1, 3), (1, 4), (1, 5), (3, 64), (2, 255), (7, 257), (9, 260), (53, 37), (64, 64))   # (H, W)
LEVELS = (0, 1, 63, 127, 128, 200, 254)
DIRECTIONS = ((0.0, 0.0), (-0.5, 0.3), (-0.2, -0.7), (4e-4, 1.0), (-4e-4, -1.0), (0.03, 0.9996), (0.0548, 0.9985), (6e-21, 8e-21), (-6e-21, 8e-21))
CONFS = ((0.0, 1.5), (1e-3, 1.25), (1e6, 1.5), (1e6, 2.0))   # (confidence, hair)


def t255():
    return (torch.arange(256, dtype=torch.int32).to(torch.uint8) / 255.0).numpy()


def planted_values():
    vals = []
    for k in LEVELS:
        c = np.float32((k + 0.5) / 255)
        vals += [np.nextafter(c, np.float32(-1)), c, np.nextafter(c, np.float32(2))]
    return np.array(vals + [0.0, 1.0, -0.3, 1.7], np.float32)


def orient64(packed):
    """the float64 model of the ``orients`` product, [1,H,W]"""
    from gaussianhaircut_amd.gaussian_renderer import orient_angle_from
    p = torch.from_numpy(np.asarray(packed)).double()
    return (orient_angle_from(p[5:8]) * p[3:4]).numpy()


def _raw(H, W, seed):
    g = np.random.default_rng(seed)
    N = H * W
    p = (g.random((10, N)) * 1.4 - 0.2).astype(np.float32)
    p[5:8] = g.standard_normal((3, N)).astype(np.float32)
    p[8] = (g.random(N) ** 2 * 40).astype(np.float32)
    p[8, 7::13] = 0
    vals = planted_values()
    n = min(N, len(vals))
    for c in range(5):
        p[c, :n] = np.roll(vals, 5 * c)[:n]
    nd = min(N, len(DIRECTIONS))
    d = np.array(DIRECTIONS, np.float32)
    p[5, :nd], p[6, :nd] = d[:nd, 0], d[:nd, 1]
    p[3, :nd] = np.float32(1.0)       # the planted directions at full hair: their angle reaches the byte undimmed
    nc = min(max(N - nd, 0), len(CONFS))
    for i in range(nc):
        p[8, nd + i], p[3, nd + i] = CONFS[i]
    prod = p[8].astype(np.float64) * p[3].astype(np.float64)
    assert np.isfinite(p).all() and ((prod == 0) | (np.abs(prod) >= 1e-30)).all()
    planted = np.zeros(N, bool)
    planted[:nd] = True
    return p.reshape(10, H, W), planted.reshape(H, W)


@functools.lru_cache(maxsize=None)
def _case(H, W):
    for seed in range(200):
        p, planted = _raw(H, W, 7000 + seed)
        _, fragile = expected_levels(orient64(p))
        rest = fragile[:, :, 0][~planted]
        if rest.size == 0 or rest.mean() <= FRAGILE_SHARE:
            return p, planted
    raise AssertionError("no seed keeps the fragile share of a %d x %d angle plane under %g" % (H, W, FRAGILE_SHARE))


def make_packed(H, W):
    """(packed float32 [10,H,W], bool [H,W]: the pixels with a planted direction); the same arrays on every call"""
    p, planted = _case(H, W)
    return p.copy(), planted.copy()


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_angle(got, packed, planted, what):
    """the fragile rule on an angle plane [1,H,W] of table values; returns the number of elements off by one level"""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == (1,) + packed.shape[1:], (what, got.dtype, got.shape)
    table = t255()
    level = np.rint(got[0].astype(np.float64) * 255).astype(np.int64)
    assert ((level >= 0) & (level <= 255)).all() and same_bits(table[np.clip(level, 0, 255)], got[0]), (what, "not a / 255 table value")
    exp, fragile = expected_levels(orient64(packed))
    exp, fragile = exp[:, :, 0], fragile[:, :, 0]
    rest = fragile[~planted]
    share = float(rest.mean()) if rest.size else 0.0
    d = np.abs(level - exp)
    print("%s angle: fragile %.2f %% of the random part, off by one at %d fragile elements" % (what, 100 * share, int((d > 0).sum())))
    assert share <= FRAGILE_SHARE, (what, share)
    assert (d[~fragile] == 0).all(), (what, int((d[~fragile] != 0).sum()))
    assert (d[fragile] <= 1).all(), (what, int(d.max()))
    return int((d > 0).sum())


def check_resized_plane(got, src, dist, what):
    """DESIGN.md 8e's bar for a bilinearly resized float plane: ``|got - f64| <= 3 |torch32 - f64| + 9 * 2^-24 max|v|``, f64 the same
    blend in double from the float32 source coordinates, ``dist`` = |torch32 - f64|.  Returns the worst err / bar."""
    from tests.golden.make_reference_loader_golden import bilinear64
    got = np.asarray(got)
    h, w = got.shape[-2:]
    assert got.dtype == np.float32 and dist.shape == (h, w), (what, got.dtype, got.shape, dist.shape)
    f64 = bilinear64(src, w, h)
    vmax = float(np.abs(np.asarray(src, np.float64)).max())
    err = np.abs(got.reshape(h, w).astype(np.float64) - f64)
    bar = 3.0 * np.asarray(dist, np.float64) + 9 * 2.0 ** -24 * vmax
    print("%s: resized plane worst |got - f64| = %.3g = %.2f x 2^-24 max|v|, worst err / bar %.3g"
          % (what, float(err.max()), float(err.max() / (2.0 ** -24 * vmax)), float((err / bar).max())))
    assert (err <= bar).all(), (what, float((err / bar).max()))
    return float((err / bar).max())


def torch32_dist(src, w, h):
    """|F.interpolate in float32 on the CPU - f64| of a plane, [h, w]"""
    from tests.golden.make_reference_loader_golden import bilinear64
    p32 = torch.nn.functional.interpolate(torch.from_numpy(np.asarray(src, np.float32))[None, None], size=(h, w), mode="bilinear")[0, 0].numpy()
    return np.abs(p32 - bilinear64(np.asarray(src, np.float32), w, h)).astype(np.float32)
