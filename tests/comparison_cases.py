"""Shared by tests/test_comparison_cpu.py and tests/test_gpu_comparison.py: the golden file, the all-pairs image, the layout table
and the strip written out by hand.  Nothing here imports Pillow or the package's kernels."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "comparison_frames.npz")
_gold = None


def gold():
    global _gold
    if _gold is None:
        with np.load(GOLDEN) as z:
            _gold = {k: z[k] for k in z.files}
    return _gold


def golden_names():
    return sorted(k[:-len("_frame")] for k in gold() if k.endswith("_frame"))


def golden_case(name):
    """(photograph, strand render, render, out_short, expected frame)"""
    g = gold()
    return g[name + "_gt"], g[name + "_preview"], g[name + "_render"], int(g[name + "_short"]), g[name + "_frame"]


def all_pairs():
    """tests/golden/make_comparison_golden.py's image: 256 x 256 RGBA, alpha = the row, the column's value permuted three ways"""
    a, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    return np.stack([v, 255 - v, (v * 7 + 3) % 256, a], -1).astype(np.uint8)


def over_white_formula(rgba):
    """the issue's formula on int64"""
    c, a = rgba[:, :, :3].astype(np.int64), rgba[:, :, 3:4].astype(np.int64)
    t = c * a + 255 * (255 - a) + 128
    return (((t >> 8) + t) >> 8).astype(np.uint8)


# (name, strand render (wb, hb), render (w, h)) -> what the middle panel must be: (resized (rw, rh), pad l, t, r, b, crop l, t).
# The landscape renders (w > h) have no photograph that fits (the rule needs w <= h): they are laid out with gt_size=None.
LAYOUTS = [
    ("square, crop left and right", (40, 40), (9, 16), (16, 16), (0, 0, 0, 0), (4, 0)),          # 7 / 2 = 3.5 -> 4
    ("portrait, crop top and bottom", (10, 31), (7, 9), (9, 27), (0, 0, 0, 0), (1, 9)),
    ("narrow, odd deficit", (5, 21), (16, 9), (9, 37), (3, 0, 4, 0), (0, 14)),                    # 7 = 3 + 4
    ("narrow, even deficit", (5, 21), (17, 9), (9, 37), (4, 0, 4, 0), (0, 14)),                   # 8 = 4 + 4
    ("difference 1", (9, 9), (8, 9), (9, 9), (0, 0, 0, 0), (0, 0)),                               # 0.5 -> 0
    ("difference 3", (9, 9), (6, 9), (9, 9), (0, 0, 0, 0), (2, 0)),                               # 1.5 -> 2
    ("difference 5", (9, 9), (4, 9), (9, 9), (0, 0, 0, 0), (2, 0)),                               # 2.5 -> 2
    ("no resize, no crop", (12, 12), (12, 12), (12, 12), (0, 0, 0, 0), (0, 0)),
    ("truncating short edge", (7, 9), (5, 6), (6, 7), (0, 0, 0, 0), (0, 0)),                      # int(6 * 9 / 7) = 7; 0.5 -> 0 twice
]


def strip_by_hand(gt, preview, render, pad_left, pad_top, crop_left, crop_top):
    """ghr.h's words, pixel by pixel: the middle panel's (y, x) is preview (y + crop_top - pad_top, x + crop_left - pad_left), zero
    outside"""
    h, w = render.shape[:2]
    ph, pw = preview.shape[:2]
    mid = np.zeros((h, w, 3), np.uint8)
    for y in range(h):
        for x in range(w):
            sy, sx = y + crop_top - pad_top, x + crop_left - pad_left
            if 0 <= sy < ph and 0 <= sx < pw:
                mid[y, x] = preview[sy, sx]
    return np.concatenate([gt, mid, render], axis=1)
