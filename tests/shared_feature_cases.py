"""Scenes for the per-strand SH segment (csrc/ghr_shared.h; ghr_model_forward_segment_shared / ghr_model_backward_segment_shared):
seeded polylines in front of a ring camera, one strand wholly behind the camera (whenever there is more than one strand), per-strand
features, optionally a frozen head.  CPU tensors; tests/test_shared_features_cpu.py runs them through the host simulator,
tests/test_gpu_shared_features.py through the C ABI.

The cases are (S, n_seg, K, n_head), each the smallest shape at which one indexing decision goes another way."""
import math

import numpy as np
import torch

from gaussianhaircut_amd.scene.cameras import ring_cameras
from gaussianhaircut_amd.scene.gaussian_model_latent_strands import build_from_points

CASES = [
    (1, 1, 16, 0),      # one row
    (300, 1, 9, 0),     # every row its own strand, more strands than a forward workgroup: equals the ordinary call on the SAME arrays
    (130, 2, 1, 0),     # K = 1: no `rest` block at all
    (7, 3, 16, 300),    # strands straddling wave and workgroup ends; the head's padding displaces row0 to 512
    (3, 99, 16, 1),     # the reference's 99 segments: 297 rows = one forward workgroup + 41
    (4, 63, 4, 0), (4, 64, 4, 0), (4, 65, 4, 0),          # strand ends on / before / after the 64-row wave of backward and fold
    (2, 255, 16, 0), (2, 256, 16, 0), (2, 257, 16, 0),    # the same around the 256-row forward workgroup
    (1, 700, 16, 0),    # S = 1: workgroups and waves wholly inside one strand
]
W = H = 64
SCALE = 4e-3


def case_id(c):
    return "S%d_seg%d_K%d_head%d" % c


def behind_strand(S):
    """index of the strand behind the camera, or None (a single strand is in front: it carries the case's gradients)"""
    return S - 1 if S > 1 else None


def wave_crossing_strand(S, n_seg):
    """a strand in front of the camera whose rows lie in two 64-row waves of the backward / fold, or (none exists: n_seg = 1, or 2
    at even alignment, or one row) the first strand"""
    last_front = S - 1 if S == 1 else S - 2
    for s in range(last_front + 1):
        if (s * n_seg) // 64 != (s * n_seg + n_seg - 1) // 64:
            return s
    return 0


def make_scene(S, n_seg, K, n_head, seed=0):
    """dict of CPU float32 tensors: xyz / scaling / rotation / dir [P,.], conf [P], f_dc [S,1,3], f_rest [S,K-1,3], head (dict or
    None), and the camera: view / proj [4,4], campos [3], tanfovx, tanfovy, sh_degree."""
    g = torch.Generator().manual_seed(1000 * seed + 31 * S + n_seg)
    cam = ring_cameras(8, W, H, device="cpu", roll_deg=20.0)[3]
    c = cam.camera_center.float()
    unit = torch.nn.functional.normalize
    roots = unit(torch.randn(S, 1, 3, generator=g), dim=-1) * 0.8
    step_len = min(0.02, 1.2 / max(n_seg, 1))
    steps = unit(torch.randn(S, 1, 3, generator=g), dim=-1) * step_len + torch.randn(S, n_seg, 3, generator=g) * step_len * 0.3
    pts = roots + torch.cat([torch.zeros(S, 1, 3), torch.cumsum(steps, dim=1)], dim=1)
    b = behind_strand(S)
    if b is not None:
        pts[b] = pts[b] * 0.2 + c * 1.5  # the camera looks at the origin from c: 1.5 c lies behind it
    xyz, rot, scaling, d = build_from_points(pts, SCALE, fused=False)
    P = S * n_seg
    out = dict(S=S, n_seg=n_seg, K=K, P=P, n_head=n_head, points=pts,
               xyz=xyz.contiguous(), rotation=rot.contiguous(), scaling=scaling.contiguous(), dir=d.contiguous(),
               conf=torch.rand(P, generator=g) * 0.5 + 0.25,
               f_dc=torch.randn(S, 1, 3, generator=g) * 0.3 + 0.2, f_rest=torch.randn(S, K - 1, 3, generator=g) * 0.2,
               view=cam.world_view_transform.float().contiguous(), proj=cam.full_proj_transform.float().contiguous(),
               campos=c.contiguous(), tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
               sh_degree=int(round(math.sqrt(K))) - 1, W=W, H=H, head=None)
    if n_head > 0:
        hx = unit(torch.randn(n_head, 3, generator=g), dim=-1) * 0.6
        out["head"] = dict(xyz=hx, scaling=torch.rand(n_head, 3, generator=g) * 0.02 + 0.005,
                           rotation=unit(torch.randn(n_head, 4, generator=g), dim=-1),
                           opacity=torch.rand(n_head, generator=g) * 0.5 + 0.2,
                           fdc=torch.randn(n_head, 1, 3, generator=g) * 0.3, frest=torch.randn(n_head, K - 1, 3, generator=g) * 0.2)
    return out


def expanded(t, n_seg):
    """[S, ...] -> [S n_seg, ...] with torch.repeat, as src/scene/gaussian_model_latent_strands.py:465-467"""
    S = t.shape[0]
    return t.reshape(S, 1, -1).repeat(1, n_seg, 1).reshape((S * n_seg,) + tuple(t.shape[1:])).contiguous()


def same_floats(a, b):
    """equal as floats: ==, +0 and -0 alike, NaN in the same places"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(np.isnan(a), np.isnan(b))) and bool((a[~np.isnan(a)] == b[~np.isnan(b)]).all())
