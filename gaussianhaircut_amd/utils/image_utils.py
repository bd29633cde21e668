"""Image metrics and the orientation colouring of the evaluation scripts (reference: ``src/utils/image_utils.py:15-37``)."""
from __future__ import annotations

import torch


def mse(img1, img2):
    return ((img1 - img2) ** 2).reshape(img1.shape[0], -1).mean(1, keepdim=True)


def psnr(img1, img2):
    """Per channel (image_utils.py:18-20); an exact match is ``inf``."""
    return 20 * torch.log10(1.0 / torch.sqrt(mse(img1, img2)))


def vis_orient(orient_angle, mask):
    """[1,H,W] angle / pi in [0,1] -> [3,H,W] colouring times ``mask`` (image_utils.py:22-37): red vertical, green horizontal,
    magenta / teal the two diagonals, composed as BGR and returned as RGB."""
    deg = orient_angle * 180

    def ramp(at):
        return torch.clamp(1 - torch.abs(deg - at) / 45., 0, 1)

    red = ramp(0.) + ramp(180.)
    green, magenta, teal = ramp(90.), ramp(45.), ramp(135.)
    b, g, r = magenta + teal, green + teal, red + magenta   # [0,0,1] red + [0,1,0] green + [1,0,1] magenta + [1,1,0] teal
    return torch.cat([r, g, b], dim=0) * mask
