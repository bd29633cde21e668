"""Writes tests/golden/comparison_frames.npz: seeded random uint8 inputs of the comparison video's frame assembly and the frames
Pillow makes of them.

    python tests/golden/make_comparison_golden.py

Pillow alone does the pixel work -- Image.new / paste / convert / resize(BICUBIC) / crop -- and the size and crop rules are those of
torchvision's Resize(int) and CenterCrop on PIL images, restated here from their documented behaviour:

* Resize(size): the shorter edge becomes size, the longer int(size * long / short); an image already of that size is returned.
* CenterCrop((h, w)): an axis shorter than the crop is padded with black, (d) // 2 before and (d + 1) // 2 after for a deficit d;
  the window starts at int(round((size - crop) / 2.0)) per axis of the padded image.

A case is (photograph, strand render, render, out_short); the file holds <name>_gt, <name>_preview, <name>_render, <name>_short,
<name>_frame and over_white_rgb, the image of all_pairs() over white (the input itself is not stored: it is a formula, which
tests/comparison_cases.py repeats).  Recorded with Pillow 12.2.0.
"""
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))

# name: (photograph (w, h), strand render (w, h, channels), render (w, h), out_short)
# The photograph's rule (Resize(w) must give exactly w x h) holds only for a render with w <= h, and there both edges of the resized
# strand render are >= h >= w: CenterCrop's padding cannot occur in a whole frame.  It is tested on the strip alone.
CASES = {
    "square_rgba": ((18, 32), (40, 40, 4), (9, 16), 12),      # a square strand render: 16 x 16, cut left and right by 7: 3.5 -> 4
    "portrait_rgb": ((14, 18), (10, 31, 3), (7, 9), 8),       # portrait: 9 x 27, cut 1 | 1 and 9 | 9
    "landscape_rgba": ((7, 9), (31, 10, 4), (7, 9), 9),       # landscape: 27 x 9, cut left by 10; the photograph is not resized
    "identity": ((12, 12), (12, 12, 4), (12, 12), 12),        # wb == hb == h: no resize, no cut; the strip 36 x 12 is the frame
    "upscale": ((5, 7), (6, 4, 4), (10, 14), 20),             # every resize enlarges; 21 x 14, cut left by 11: 5.5 -> 6
    "half_of_one": ((16, 18), (9, 9, 4), (8, 9), 5),          # a difference of 1: 0.5 -> 0
    "half_of_five": ((8, 18), (9, 9, 3), (4, 9), 6),          # a difference of 5: 2.5 -> 2
    "truncated": ((7, 9), (7, 9, 4), (5, 6), 4),              # int(5 * 9 / 7) = 6 and int(6 * 9 / 7) = 7: both truncate
}


def short_edge(w, h, size):
    if w <= h:
        return size, int(size * h / w)
    return int(size * w / h), size


def resize(im, size):
    return im if im.size == tuple(size) else im.resize(size, Image.BICUBIC)


def over_white(rgba):
    im = Image.fromarray(rgba, "RGBA")
    canvas = Image.new("RGBA", im.size, "WHITE")
    canvas.paste(im, (0, 0), im)
    return canvas.convert("RGB")


def center_crop(im, w, h):
    iw, ih = im.size
    if w > iw or h > ih:
        left, top = ((w - iw) // 2 if w > iw else 0), ((h - ih) // 2 if h > ih else 0)
        right, bottom = ((w - iw + 1) // 2 if w > iw else 0), ((h - ih + 1) // 2 if h > ih else 0)
        padded = Image.new("RGB", (iw + left + right, ih + top + bottom), (0, 0, 0))
        padded.paste(im, (left, top))
        im = padded
        iw, ih = im.size
    top, left = int(round((ih - h) / 2.0)), int(round((iw - w) / 2.0))
    return im.crop((left, top, left + w, top + h))


def frame(gt, preview, render, out_short):
    h, w = render.shape[:2]
    strand = over_white(preview) if preview.shape[2] == 4 else Image.fromarray(preview, "RGB")
    strand = center_crop(resize(strand, short_edge(strand.size[0], strand.size[1], h)), w, h)
    photo = Image.fromarray(gt, "RGB")
    photo = resize(photo, short_edge(photo.size[0], photo.size[1], w))
    assert photo.size == (w, h), (photo.size, (w, h))
    strip = Image.fromarray(np.concatenate([np.asarray(photo), np.asarray(strand), render], axis=1), "RGB")
    return np.asarray(resize(strip, short_edge(3 * w, h, out_short)))


def all_pairs():
    """256 x 256 RGBA: alpha = the row, and the three colour bytes the column permuted three ways, so every (alpha, value) pair
    occurs in every channel"""
    a, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    return np.stack([v, 255 - v, (v * 7 + 3) % 256, a], -1).astype(np.uint8)


def main():
    g = np.random.default_rng(20240607)
    out = {}
    rgba = all_pairs()
    out["over_white_rgb"] = np.asarray(over_white(rgba))   # (the input is all_pairs(): tests/comparison_cases.py rebuilds it)
    for name, ((wg, hg), (wb, hb, cb), (w, h), short) in CASES.items():
        gt = g.integers(0, 256, (hg, wg, 3), dtype=np.uint8)
        preview = g.integers(0, 256, (hb, wb, cb), dtype=np.uint8)
        if cb == 4:   # alphas 0 and 255 are as common in a render as the ones in between
            preview[:, :, 3] = np.where(g.random((hb, wb)) < 0.3, 0, np.where(g.random((hb, wb)) < 0.4, 255, preview[:, :, 3]))
        render = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
        out[name + "_gt"], out[name + "_preview"], out[name + "_render"] = gt, preview, render
        out[name + "_short"] = np.int64(short)
        out[name + "_frame"] = frame(gt, preview, render, short)
    np.savez_compressed(os.path.join(HERE, "comparison_frames.npz"), **out)
    print("comparison_frames.npz: %d cases, %d bytes" % (len(CASES), os.path.getsize(os.path.join(HERE, "comparison_frames.npz"))))


if __name__ == "__main__":
    main()
