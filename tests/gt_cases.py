"""Shapes and inputs of the resize tests (tests/test_ground_truth_cpu.py, tests/test_gpu_ground_truth.py).

Each shape is the smallest at which one decision of ``ghr_resample_u8`` or its kernels goes another way.  (in_w, in_h), channels,
(out_w, out_h):

  (37, 53) x3 -> (18, 26)   the ``// 2`` case: 11 taps, odd sizes, rows of 159 and 54 bytes (no multiple of four: the vertical
                            pass goes byte by byte), both passes with the uint8 intermediate
  (37, 53) x3 -> (9, 13)    the ``// 4`` case: 19 taps
  (37, 53) x1 -> (18, 26), (9, 13)   the same for a mask: one channel; 11 taps take the direct horizontal kernel, 19 the staged
  (16, 20) x3 -> (33, 41)   an upscale: 5 taps, neighbouring outputs share their window
  (64, 48) x1 -> (64, 24)   the vertical pass alone; rows of 64 bytes: its four-bytes-per-thread form
  (64, 48) x3 -> (32, 48)   the horizontal pass alone
  (5, 7)   x3 -> (1, 1)     every window clipped on both sides, n < ksize; all weights positive (no saturation possible)
  (1, 1)   x1 -> (4, 5)     one source pixel: one tap everywhere
  (200, 3) x3 -> (25, 3)    33 taps, the horizontal pass alone over three rows
  (3, 200) x1 -> (3, 25)    33 taps down a column three bytes wide
  (64, 64) x3 -> (8, 8)     ``-r 8``; rows of 24 bytes after the first pass: the four-byte form after a horizontal pass
  (31, 29) x1 -> (30, 28)   a scale just above 1: windows of 5 and 6 taps
  (150, 11) x3 -> (70, 11) crosses the staged horizontal kernel's workgroup edges: 64 output columns, 8 rows; the last
                            workgroup holds 6 columns and 3 rows
  (95, 5)  x3 -> (10, 5)    39 taps, more than the staged horizontal kernel takes (33): the direct one, 4 rows a workgroup
  (90, 2)  x1 -> (10, 2)    37 taps: the direct kernel with one channel
  (350, 9) x3 -> (350, 4)   crosses the vertical kernel's workgroup edge (1024 bytes of a row) byte by byte: 1050 bytes
  (344, 9) x3 -> (344, 4)   the same in the four-byte form: 1032 bytes
  (37, 53) x3 -> (37, 53)   equal sizes: a copy, no launch

Inputs: random bytes with every third row drawn from {0, 255} only, so that the negative lobes of the bicubic weights push sums
below 0 and above 255.  A window of more than 11 taps (a scale above 2) averages such rows out -- and two random rows out of
three hold a vertical sum near the middle whatever the third does -- so no output of those cases could clip, however the seed
fell.  They draw from {0, 255} in bars instead: 255 where both coordinates fall into a bar as wide as the filter's central lobe
(two output pixels), 0 in the gaps of the same width, and one pixel in twenty replaced by a random byte.  A window centred on
a bar sums to about 1.08 * 255, one centred on a gap to about -0.08 * 255.
``saturates`` says whether the unclipped accumulators of a case (from the comparator, on the CPU) clip on
both sides; it must wherever an axis has a negative coefficient -- with positive weights only an output is a convex combination
of bytes and cannot leave 0 ... 255."""
import numpy as np
import torch

SHAPES = (((37, 53), 3, (18, 26)), ((37, 53), 3, (9, 13)), ((37, 53), 1, (18, 26)), ((37, 53), 1, (9, 13)), ((16, 20), 3, (33, 41)),
          ((64, 48), 1, (64, 24)), ((64, 48), 3, (32, 48)), ((5, 7), 3, (1, 1)), ((1, 1), 1, (4, 5)), ((200, 3), 3, (25, 3)),
          ((3, 200), 1, (3, 25)), ((64, 64), 3, (8, 8)), ((31, 29), 1, (30, 28)), ((150, 11), 3, (70, 11)), ((95, 5), 3, (10, 5)), ((90, 2), 1, (10, 2)), ((350, 9), 3, (350, 4)),
          ((344, 9), 3, (344, 4)), ((37, 53), 3, (37, 53)))


def case_id(case):
    (iw, ih), c, (ow, oh) = case
    return "%dx%dx%d-%dx%d" % (iw, ih, c, ow, oh)


def make_input(case, seed=0):
    (iw, ih), c, _ = case
    g = np.random.default_rng(1000 * iw + 10 * ih + c + seed)
    (ow, oh) = case[2]
    a = g.integers(0, 256, (ih, iw, c) if c == 3 else (ih, iw), dtype=np.uint8)
    if iw <= 2 * ow and ih <= 2 * oh:
        a[::3] = g.choice(np.array([0, 255], np.uint8), a[::3].shape)
        return a

    def bars(n_in, n_out):
        fs = max(n_in / n_out, 1.0)
        u = (np.arange(n_in) + 0.5) / fs - 0.5   # in output pixels: bars centred on outputs 0, 4, 8, ..., gaps on 2, 6, ...
        return (np.floor((u + 1) / 2) % 2 == 0) if n_in != n_out else np.ones(n_in, bool)
    bar = (bars(ih, oh)[:, None] & bars(iw, ow)[None, :]).astype(np.uint8) * 255
    keep = g.random((ih, iw)) < 0.05
    if c == 3:
        bar, keep = bar[:, :, None].repeat(3, 2), keep[:, :, None].repeat(3, 2)
    return np.where(keep, a, bar)


def has_negative_weights(case):
    from gaussianhaircut_amd import ground_truth as gt
    (iw, ih), _, (ow, oh) = case
    return any(a != b and (gt.resample_coefficients(a, b)[1] < 0).any() for a, b in ((iw, ow), (ih, oh)))


def saturates(case, image):
    """(some accumulator below 0, some above 255) over the passes the case runs, from the comparator's int32 sums"""
    from gaussianhaircut_amd import ground_truth as gt
    (iw, ih), _, (ow, oh) = case
    t = torch.from_numpy(image)
    low = high = False
    for axis, a, b in ((1, iw, ow), (0, ih, oh)):
        if a == b:
            continue
        bounds, coef = gt.resample_coefficients(a, b)
        acc = gt.resample_axis_torch(t, axis, bounds, coef, accumulators=True) >> gt.PRECISION_BITS
        low, high = low or bool((acc < 0).any()), high or bool((acc > 255).any())
        t = gt.resample_axis_torch(t, axis, bounds, coef)
    return low, high
