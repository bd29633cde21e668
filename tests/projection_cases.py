"""Boundary shapes of the fused projection pair (csrc/ghr_project.h: k_project, k_project_bwd<CAM, ADAM>, k_sh_grad_from_views,
k_cam_fold) and their float64 arbiter.  Importable without a GPU: tests/test_projection_cases_cpu.py checks here that the
reference alone has the properties tests/test_gpu_projection_shapes.py relies on.

What the shapes walk.  A row of the coefficient slab is 3 (K - 1) floats: 9, 24 or 45 for K = 4, 9, 16 (none for K = 1).  The
slab routines move `nb` rows in 16-byte pieces and finish with a scalar loop over the last `nb * row % 4` floats.  9 and 45 are
1 mod 4, so that remainder is nb % 4: the forward workgroup (256 rows) ends with nb = P % 256, the backward wave (64 rows) with
nb = P % 64.  (A slab shorter than one piece, n_floats < 4, cannot occur: one row is at least 9 floats.)
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import numpy as np
import torch

from gaussianhaircut_amd.gaussian_renderer import render
from gaussianhaircut_amd.utils import synthetic as syn
from tests.projection_shared import GENERIC, PARAMS, make_trainable


class Case(NamedTuple):
    name: str
    P: int
    max_deg: int   # K = (max_deg + 1)^2 coefficients stored
    active: int    # active degree
    W: int
    H: int
    owned: bool    # model.training_setup(): the arrays are views of FusedAdam's flat buffers (no padding between groups)
    seed: int = 0
    log_scale: float = math.log(0.07)


# P walks one lane (1, 2, 3), the backward wave's end (63, 64, 65, 127, 129) and the forward workgroup's end (255, 256, 257, 513);
# K every row width; active == max (the last coefficients carry gradient) and active < max (3 / 1, 2 / 0: exact zeros above).
# Tail remainders, last backward wave | last forward workgroup:
#   1: P = 1, 65, 129, 257, 513 | 1, 65, 129, 257, 513     2: P = 2 | 2     3: P = 3, 63, 127, 255 | 3, 63, 127, 255
# (K = 4 and K = 16 each at all three).  Owned models: P = 63, 65, 257 (P % 4 != 0: features_rest and its gradient start
# 8 bytes off a 16-byte boundary), P = 2 (remainder 2 for the fused update) and P = 64 (aligned).
SHAPES = [
    Case("p1_k16", 1, 3, 3, 64, 48, False, seed=3),
    Case("p1_k1", 1, 0, 0, 64, 48, False, seed=3),
    Case("p2_k4_owned", 2, 1, 1, 64, 48, True, seed=5),
    Case("p2_k16", 2, 3, 3, 64, 48, False, seed=5),
    Case("p3_k4", 3, 1, 1, 64, 48, False, seed=6),
    Case("p3_k9", 3, 2, 2, 64, 48, False, seed=6),
    Case("p3_k16", 3, 3, 3, 64, 48, False, seed=6),
    Case("p63_k16_owned", 63, 3, 3, 64, 48, True, seed=11),
    Case("p63_k4", 63, 1, 1, 70, 37, False, seed=12),
    Case("p64_k4_owned", 64, 1, 1, 64, 48, True, seed=13),
    Case("p64_k9", 64, 2, 0, 64, 48, False, seed=14),
    Case("p65_k4_owned", 65, 1, 1, 64, 48, True, seed=15),
    Case("p65_k16", 65, 3, 3, 70, 37, False, seed=16),
    Case("p127_k16", 127, 3, 1, 64, 48, False, seed=17),
    Case("p129_k4", 129, 1, 1, 64, 48, False, seed=18),
    Case("p129_k1", 129, 0, 0, 64, 48, False, seed=19),
    Case("p255_k9", 255, 2, 2, 64, 48, False, seed=20),
    Case("p255_k4", 255, 1, 1, 64, 48, False, seed=21),
    Case("p256_k16", 256, 3, 3, 64, 48, False, seed=22),
    Case("p257_k16_owned", 257, 3, 3, 64, 48, True, seed=23),
    Case("p257_k4", 257, 1, 1, 64, 48, False, seed=24),
    Case("p513_k16", 513, 3, 3, 64, 48, False, seed=25),
    Case("p513_k4", 513, 1, 1, 64, 48, False, seed=26),
]
BY_NAME = {c.name: c for c in SHAPES}
OWNED = [c for c in SHAPES if c.owned]
# 1, 1, 1, 2, 3, 5 columns of the camera partial table
CAMERA_CASES = ["p1_k16", "p63_k16_owned", "p64_k9", "p65_k16", "p129_k4", "p257_k16_owned"]

# ---- planted edge rows (cases with P >= 63; the P = 1 .. 3 cases stay random) -------------------------------------------------
ROW_CLAMP_X, ROW_CLAMP_Y, ROW_BEHIND, ROW_CUT, ROW_Q3, ROW_QSMALL, ROW_OP_HI, ROW_OP_LO, ROW_TIE = range(9)
N_PLANTED = 9
CLAMP_FACTOR = 1.11      # tx / tz = 1.11 * 1.3 tan(FoVx / 2): 11 % beyond the clamp, 44 % beyond the image's edge
TIE_SCALES = (0.12, 0.12, 0.06)
CAM_DISTANCE = 4.0       # syn.make_view's front camera: t = xyz + (0, 0, 4)
FOVY = math.radians(40.0)


def spec_of(case: Case):
    return syn.WorkloadSpec(case.name, case.P, case.W, case.H, case.seed, "random", case.log_scale)


def planted(case: Case) -> bool:
    return case.P >= 63


def tan_half_fov(case: Case):
    tfy = math.tan(FOVY / 2)
    return tfy * case.W / case.H, tfy


@torch.no_grad()
def plant_edge_rows(model, case: Case):
    """Overwrites rows 0 .. 8 of a model built by syn.make_model (any device); values are the same floats everywhere."""
    tfx, tfy = tan_half_fov(case)
    f = lambda *v: torch.tensor(v, dtype=torch.float32, device=model._xyz.device)
    ident = f(1.0, 0.0, 0.0, 0.0)
    # beyond the 1.3 tan(FoV / 2) clamp in x / in y, long along that axis so that the ellipse still reaches the image
    model._xyz[ROW_CLAMP_X] = f(CLAMP_FACTOR * 1.3 * tfx * CAM_DISTANCE, 0.05, 0.0)
    model._scaling[ROW_CLAMP_X] = torch.log(f(0.45, 0.1, 0.08))
    model._xyz[ROW_CLAMP_Y] = f(0.05, CLAMP_FACTOR * 1.3 * tfy * CAM_DISTANCE, 0.0)
    model._scaling[ROW_CLAMP_Y] = torch.log(f(0.1, 0.45, 0.08))
    for r in (ROW_CLAMP_X, ROW_CLAMP_Y):
        model._rotation[r] = ident
        model._opacity[r] = 1.0
    # behind the near plane: view z = 0.1 < 0.2
    model._xyz[ROW_BEHIND] = f(0.1, -0.1, 0.1 - CAM_DISTANCE)
    # red is cut by clamp_min(sh + 0.5, 0): its value is 0.282 * -3 + 0.5 = -0.35 whatever the direction (no higher red
    # coefficients); green and blue stay well above 0
    model._xyz[ROW_CUT] = f(0.2, 0.15, 0.0)
    model._scaling[ROW_CUT] = torch.log(f(0.12, 0.1, 0.08))
    model._opacity[ROW_CUT] = 2.0
    model._features_dc[ROW_CUT, 0] = f(-3.0, 1.0, 1.0)
    if model._features_rest.shape[1]:
        model._features_rest[ROW_CUT] *= 0.3
        model._features_rest[ROW_CUT, :, 0] = 0.0
    # quaternions of length 3 and 1e-3 (the kernels normalise, and differentiate the normalisation)
    model._rotation[ROW_Q3] = torch.nn.functional.normalize(model._rotation[ROW_Q3], dim=0) * 3.0
    model._rotation[ROW_QSMALL] = torch.nn.functional.normalize(model._rotation[ROW_QSMALL], dim=0) * 1e-3
    model._opacity[ROW_OP_HI] = 12.0
    model._opacity[ROW_OP_LO] = -12.0
    # (the four in front of the cloud, apart from each other, so that none hides behind a random neighbour)
    for r, (x, y) in ((ROW_Q3, (-0.5, -0.4)), (ROW_QSMALL, (0.5, -0.4)), (ROW_OP_HI, (-0.6, 0.5)), (ROW_OP_LO, (0.6, 0.5))):
        model._xyz[r] = f(x, y, -1.2)
        model._scaling[r] = torch.log(f(0.09, 0.06, 0.04))
    model._opacity[ROW_Q3] = 1.0
    model._opacity[ROW_QSMALL] = 1.0
    # two exactly equal longest scales: the strand direction follows the FIRST maximum (gaussian_model.py:384-388)
    model._xyz[ROW_TIE] = f(-0.3, 0.2, 0.1)
    model._scaling[ROW_TIE] = torch.log(f(*TIE_SCALES))
    model._opacity[ROW_TIE] = 1.5
    return model


def build_model(case: Case, dev="cpu", owned=None):
    """The case's model on `dev`; `owned` (default: the case's) hands its arrays to FusedAdam's flat buffers."""
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    model = syn.make_model(spec_of(case), dev, sh_degree=case.max_deg)
    if planted(case):
        plant_edge_rows(model, case)
    model.active_sh_degree = case.active
    if case.owned if owned is None else owned:
        model.training_setup(OptimizationParams())
    return model


def build_view(case: Case, dev="cpu", trainable=False, index=None):
    """The front camera of syn.make_view, or view `index` of ring_cameras(2, ...)."""
    if index is None:
        cam = syn.make_view(spec_of(case), dev)
    else:
        from gaussianhaircut_amd.scene.cameras import ring_cameras
        cam = ring_cameras(2, case.W, case.H, device=dev)[index]
    return make_trainable(cam, split=True) if trainable else cam


def loss_weights(case: Case, seed=41):
    """dL/d(renders_packed) [10, H, W]: the loss is (renders_packed * weights).sum()."""
    return torch.randn(10, case.H, case.W, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


# world_view_transform: the leaf's total gradient; view_direct: the part it receives as the projection's own input
CAM_NAMES = ("world_view_transform", "view_direct", "FoVx", "FoVy")


def camera_grads(cam):
    """{name: tensor} of a build_view(..., trainable=True) camera after backward"""
    return dict(world_view_transform=cam.view_leaf.grad, view_direct=cam.world_view_transform.grad, FoVx=cam.FoVx.grad,
                FoVy=cam.FoVy.grad)


def _collect(model, cam, trainable):
    g = {n: getattr(model, n).grad.detach().numpy().astype(np.float64).copy() for n in PARAMS}
    if trainable:
        for n, t in camera_grads(cam).items():
            g[n] = t.detach().numpy().astype(np.float64).copy()
    return g


def arbiter(case: Case, weights, trainable=False, index=None, drop=None):
    """The project's float64 arbiter for one view (tests/oracle_backend.py; leg B of tests/test_gpu_fused_fullsize.py): the
    float32 chain through the CPU oracle, then the same chain in IEEE double composited over the float32 run's lists.  The loss is
    (renders_packed * weights).sum() with zero weight on the named pixels `st32.fragile | (n_contrib64 != st32.n_contrib)` and
    on `drop` ([H, W] bool: the caller's flipped Gaussians' boxes) -- on every side.
    Returns dict(g32, g64: gradients of the eight parameter tensors (+ CAM_NAMES with `trainable`),
    named [H, W] bool, weights: the effective ones, radii: the float32 chain's, means2d: its pixel means, state: the oracle's)."""
    from tests import oracle_backend as ob
    H, W = case.H, case.W
    bg = syn.background("cpu")

    mc, cc = build_model(case, "cpu", owned=False), build_view(case, "cpu", trainable, index)
    with ob.oracle_rasterizer():
        pc = render(cc, mc, GENERIC, bg)
    st32 = ob.LAST["state"]
    keep = mc.filter_points(cc)
    m64, c64 = ob.double_chain(mc, cc, keep)
    if trainable:
        make_trainable(c64, split=True)
    with ob.oracle_rasterizer64(st32):
        p64 = render(c64, m64, GENERIC, bg.double())
    named = (np.asarray(st32.fragile).reshape(H, W).astype(bool) |
             (np.asarray(ob.LAST["n_contrib64"]) != np.asarray(st32.n_contrib)).reshape(H, W))
    off = named if drop is None else (named | np.asarray(drop, bool))
    w_eff = weights * torch.from_numpy(~off).to(weights.dtype)
    (p64.renders_packed * w_eff.double()).sum().backward()
    g64 = _collect(m64, c64, trainable)
    (pc.renders_packed * w_eff).sum().backward()
    g32 = _collect(mc, cc, trainable)
    vs = pc["viewspace_points"].detach().numpy()
    pix = np.stack([((vs[:, 0] + 1) * W - 1) * 0.5, ((vs[:, 1] + 1) * H - 1) * 0.5], axis=1)
    return dict(g32=g32, g64=g64, named=named, weights=w_eff, radii=pc["radii"].numpy().copy(), means2d=pix, state=st32,
                keep=keep.numpy().copy())


@functools.lru_cache(maxsize=None)
def arbiter_cached(name: str, trainable=False, index=None):
    """arbiter() of a case with its own loss_weights and nothing dropped: computed once, shared, never written to."""
    case = BY_NAME[name]
    return arbiter(case, loss_weights(case), trainable, index)


def last_coeff_rows(case: Case):
    """(first row above the active degree, number of rows) of features_rest's middle axis"""
    return (case.active + 1) ** 2 - 1, (case.max_deg + 1) ** 2 - 1


def branch_margins(case: Case):
    """The planted rows' predicates recomputed in float64 from the model's float32 values: dict of signed margins, each of
    which must be >= 1e-3 for the row to take the branch it was built for in either precision."""
    model = build_model(case, "cpu", owned=False)
    tfx, tfy = (math.tan(float(v) * 0.5) for v in (build_view(case).FoVx.double(), build_view(case).FoVy.double()))
    xyz = model._xyz.detach().double().numpy()
    t = xyz + np.array([0.0, 0.0, CAM_DISTANCE])
    rx, ry = t[:, 0] / t[:, 2], t[:, 1] / t[:, 2]
    m = {}
    m["clamp_x beyond the limit"] = abs(rx[ROW_CLAMP_X]) - 1.3 * tfx
    m["clamp_x inside in y"] = 1.3 * tfy - abs(ry[ROW_CLAMP_X])
    m["clamp_y beyond the limit"] = abs(ry[ROW_CLAMP_Y]) - 1.3 * tfy
    m["clamp_y inside in x"] = 1.3 * tfx - abs(rx[ROW_CLAMP_Y])
    m["behind the near plane"] = 0.2 - t[ROW_BEHIND, 2]
    others = [r for r in range(N_PLANTED) if r not in (ROW_CLAMP_X, ROW_CLAMP_Y, ROW_BEHIND)]
    m["the others in front of the near plane"] = float((t[others, 2] - 0.2).min())
    m["the others inside the clamp"] = float(min((1.3 * tfx - np.abs(rx[others])).min(), (1.3 * tfy - np.abs(ry[others])).min()))
    # the cut channel: clamp_min(sh + 0.5, 0) in double
    from gaussianhaircut_amd.utils.sh_utils import eval_sh
    K = (case.max_deg + 1) ** 2
    feats = model.get_features.detach().double()
    d = torch.from_numpy(xyz) - torch.tensor([0.0, 0.0, -CAM_DISTANCE], dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True)
    rgb = (eval_sh(case.active, feats.transpose(1, 2).reshape(-1, 3, K), d) + 0.5).numpy()
    m["cut channel below the clamp"] = -0.05 - rgb[ROW_CUT, 0]
    m["other channels above the clamp"] = float(rgb[ROW_CUT, 1:].min())
    return m
