"""The convention check of the synthetic captures: one comb of strands seen by the three places that speak of a 2D
hair orientation -- the capture's angle byte, the Gaussian rasterizer's ``orient_angle`` and the Gabor bank's degree byte.

The comb: N straight strands in the plane z = 0 in front of the SURVEY camera (128 x 128, 40 degrees, distance 4), 4.5 pixels apart at
the centre, turning by half a degree per strand from ``phi0`` (their spacing stays within 3.9 ... 5.1 pixels over the frame), dark,
as wide as the light gaps between them (half_width 1.125 over the white background): alternately dark and light bands of 2.25 pixels,
stripes of period 4.5 beside the bank's 1 / 0.23 = 4.35; no head.  (Measured while choosing it: with dark and light strands abutting,
period 9, the bank's byte is 3 degrees off in the median and 30 at the 99th percentile: it is not made for that frequency.)
``measure(phi0, device)`` runs the CPU forms (the oracle backend of tests/oracle_backend.py, fused=False) on "cpu" and the
product's on a ROCm device."""
import math

import numpy as np
import torch

from gaussianhaircut_amd import orientation as ori
from gaussianhaircut_amd import synthetic_capture as cap
from gaussianhaircut_amd import visibility as vis
from gaussianhaircut_amd.gaussian_renderer import render
from gaussianhaircut_amd.scene.cameras import make_camera
from gaussianhaircut_amd.scene.gaussian_model import GaussianModel
from gaussianhaircut_amd.utils import synthetic as syn
from gaussianhaircut_amd.utils.general_utils import inverse_sigmoid, parallel_transport

SIZE, N_STRANDS, POINTS, SPACING, TURN, HALF_WIDTH, HALF_LENGTH, SIGMA_ACROSS = 128, 27, 32, 4.5, 0.5, 1.125, 62.0, 1.5
PHI0 = (25.0, 70.0, 115.0, 160.0)
MIN_PIXELS = 1000
# MEASURED with measure(phi0, "cpu"): phi0 -> ((a) median, 99th percentile), ((b) median, 99th percentile), degrees
CPU_MEASURED = {25.0: ((0.44, 0.54), (0.0, 5.1)), 70.0: ((0.44, 0.55), (0.0, 5.0)), 115.0: ((0.45, 0.55), (0.0, 6.0)),
                160.0: ((0.44, 0.55), (0.0, 5.0))}


def comb(phi0):
    """(points float32 [N, L, 3], colours float32 [N, 3]) in world units; the camera's pixel is 4 tan(20 deg) / 64 of them at z = 0"""
    px = 4.0 * math.tan(math.radians(20.0)) / (SIZE / 2.0)
    i = np.arange(N_STRANDS) - N_STRANDS // 2
    phi = np.radians(phi0 + TURN * i)
    d = np.stack([np.sin(phi), np.cos(phi)], 1)                        # byte k is the screen direction (sin k, cos k), y down
    nrm = np.array([math.cos(math.radians(phi0)), -math.sin(math.radians(phi0))])
    t = np.linspace(-HALF_LENGTH, HALF_LENGTH, POINTS)
    xy = (SPACING * i)[:, None, None] * nrm[None, None] + t[None, :, None] * d[:, None]
    pts = np.concatenate([xy * px, np.zeros((N_STRANDS, POINTS, 1))], -1).astype(np.float32)
    col = np.full((N_STRANDS, 3), 0.12)
    return np.ascontiguousarray(pts), np.ascontiguousarray(col.astype(np.float32))


def gaussians(points, device):
    """free strand-aligned Gaussians of the comb's segments, as utils.synthetic.strand_gaussian_params builds them: the mean at
    the segment's middle, scale (|dir| / 2, w, w), the quaternion that carries x to dir, opacity and label 0.999"""
    p = torch.from_numpy(points)
    d = (p[:, 1:] - p[:, :-1]).reshape(-1, 3)
    xyz = ((p[:, 1:] + p[:, :-1]) * 0.5).reshape(-1, 3)
    P = xyz.shape[0]
    x_axis = torch.zeros_like(d)
    x_axis[:, 0] = 1
    rot = parallel_transport(x_axis, d)
    w = SIGMA_ACROSS * 4.0 * math.tan(math.radians(20.0)) / (SIZE / 2.0)
    scales = torch.cat([d.norm(dim=-1, keepdim=True) * 0.5, torch.full((P, 2), w)], dim=-1)
    feats = torch.zeros(P, 16, 3)
    feats[:, 0, :] = 0.4
    big = torch.full((P, 1), 0.999)
    m = GaussianModel(3)
    m.create_from_tensors(*(x.to(device) for x in (xyz, feats, torch.log(scales), rot, inverse_sigmoid(big), inverse_sigmoid(big),
                                                   torch.zeros(P, 1))), spatial_lr_scale=1.0)
    m.active_sh_degree = 3
    return m


def _circular(a, b):
    d = np.abs(a.astype(np.float64) - b.astype(np.float64)) % 180.0
    return np.minimum(d, 180.0 - d)


def measure(phi0, device):
    """dict(pixels, a=(median, p99), b=(median, p99), signed_a, signed_b): the circular differences in degrees on the pixels where
    the capture's hair byte is 255 and the rendered hair mask is > 0.9; signed_*: the median of the signed difference (other -
    capture, wrapped to -90 ... 90) -- a systematic offset or a mirrored angle shows there"""
    from tests.projection_shared import FUSED, GENERIC
    dev = torch.device(device)
    on_gpu = dev.type == "cuda"
    points, colours = comb(phi0)
    cam = make_camera(SIZE, SIZE, fovy_deg=40.0, distance=4.0, device=dev)
    cv = cap.capture_view(points, vis.view_matrix_from_camera(cam), colors=colours, half_width=HALF_WIDTH, fused=on_gpu, device=dev)
    model = gaussians(points, dev)
    with torch.no_grad():
        if on_gpu:
            pkg = render(cam, model, FUSED, syn.background(dev))
        else:
            from tests.oracle_backend import oracle_rasterizer
            with oracle_rasterizer():
                pkg = render(cam, model, GENERIC, syn.background(dev))
        rendered = (pkg["orient_angle"][0] * 180.0).cpu().numpy()
        mask = pkg["mask"][0].cpu().numpy()
    bank = ori.orientation_maps(cv.image, fused=on_gpu)[0].cpu().numpy()
    byte = cv.angle.cpu().numpy()
    on = (cv.mask_hair.cpu().numpy() == 255) & (mask > 0.9)
    out = dict(pixels=int(on.sum()))
    for key, other in (("a", rendered), ("b", bank)):
        d = _circular(other[on], byte[on])
        signed = (other[on].astype(np.float64) - byte[on] + 90.0) % 180.0 - 90.0
        out[key] = (float(np.median(d)), float(np.percentile(d, 99)))
        out["signed_" + key] = float(np.median(signed))
    return out
