"""`-m gpu`: the fused projection pair (csrc/ghr_project.h) at the ends of its workgroups, against float64.

k_project, k_project_bwd<CAM, ADAM>, k_sh_grad_from_views and k_cam_fold on the shapes of tests/projection_cases.py: one lane, the
backward wave's end, the forward workgroup's end, every row width of the coefficient slab, the scalar tails of slab_load /
slab_to_lds / slab_dma / slab_out / slab_out_adam at remainders 1, 2 and 3, and optimizer-owned models whose features_rest starts
off a 16-byte boundary.  Per Gaussian and per element, not per image: a wrong tail corrupts the last Gaussian's highest SH
coefficients (or their Adam moments), one row in hundreds.

Bars.  Forward state and camera gradients: DESIGN.md 8i's, |got - f64| <= 1e-5 max|f64| + 3 |composed float32 - f64|.  Parameter
gradients: leg B of tests/test_gpu_fused_fullsize.py, |HIP - f64| <= 3 |oracle32 - f64| + hp.TOL (|f64| + row max) + FLOOR x
tensor max.  tests/test_projection_cases_cpu.py shows that the reference alone is non-zero where a tail would be corrupted.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd.gaussian_renderer import render
from gaussianhaircut_amd.utils import synthetic as syn
from tests import projection_cases as pc
from tests.projection_shared import FUSED, GENERIC, PARAMS, _pixel_mask, row_unit

pytestmark = pytest.mark.gpu

IDS = [c.name for c in pc.SHAPES]
OWNED_IDS = [c.name for c in pc.OWNED]
PATTERN = 0x7FC0BEEF  # a quiet NaN no arithmetic produces


def _dev():
    return torch.device("cuda:0")


def _ptr(t):
    return None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _max_flips(P):
    return max(2, int(1e-3 * P))


def _reference(case, trainable=False, index=None):
    """The arbiter of one view with the Gaussians whose radius differs between the device chains (FUSED, GENERIC) or from the
    oracle chain counted and their boxes dropped on all sides.  Without flips (the usual outcome) the shared cached arbiter."""
    dev = _dev()
    a = pc.arbiter_cached(case.name, trainable, index)
    with torch.no_grad():
        cam = pc.build_view(case, dev, False, index)
        rf = render(cam, pc.build_model(case, dev, owned=False), FUSED, syn.background(dev))["radii"].cpu().numpy()
        rg = render(cam, pc.build_model(case, dev, owned=False), GENERIC, syn.background(dev))["radii"].cpu().numpy()
    m1, n1 = _pixel_mask(a["state"], case.H, case.W, rf, rg, a["means2d"])
    m2, n2 = _pixel_mask(a["state"], case.H, case.W, rf, a["radii"], a["means2d"])
    assert n1 + n2 <= _max_flips(case.P), (n1, n2)
    if n1 + n2 == 0:
        return a
    drop = m1 | m2
    assert (drop | a["named"]).mean() < 0.05
    return pc.arbiter(case, pc.loss_weights(case), trainable, index, drop=drop)


def _param_grads(model):
    out = {}
    for n in PARAMS:
        t = getattr(model, n)
        if t.numel():
            out[n] = t.grad.detach().cpu().numpy().astype(np.float64).copy()
    return out


def _check_param_grads(tag, got, refs, first_off, n_rows, planted, report):
    """Leg B's criterion for every element; `refs`: the views' arbiter results (their float64 gradients and their oracle32
    distances add up).  Then the exact zeros."""
    failed = []
    for k, a in got.items():
        r = sum(x["g64"][k] for x in refs).reshape(len(a), -1)
        d32 = sum(np.abs(x["g32"][k] - x["g64"][k]) for x in refs).reshape(r.shape)
        a = a.reshape(r.shape)
        assert np.isfinite(a).all(), (tag, k)
        bar = 3.0 * d32 + row_unit(r)
        pos = bar > 0  # (a tensor that is zero altogether -- every row above the active degree -- has a bar of 0: exact match)
        ratio = float(np.where(pos, np.abs(a - r) / np.where(pos, bar, 1.0), np.where(a == r, 0.0, np.inf)).max())
        own = float(np.where(pos, d32 / np.where(pos, row_unit(r), 1.0), 0.0).max())
        report.append("%s %s: worst |HIP - f64| / bar %.3f, oracle32 chain / row criterion %.3f" % (tag, k, ratio, own))
        if not (np.abs(a - r) <= bar).all():
            i, j = np.unravel_index(np.argmax(np.abs(a - r) - bar), r.shape)
            failed.append((k, int(i), int(j), float(a[i, j]), float(r[i, j]), ratio))
    print("\n".join(report), flush=True)
    assert not failed, failed
    if n_rows:
        rest = got["_features_rest"].reshape(-1, n_rows, 3)
        assert not rest[:, first_off:].any(), "rows above the active degree must be exact zeros"
    if planted:
        for k, a in got.items():
            assert not a[pc.ROW_BEHIND].any(), (k, "the culled row")
        dc = got["_features_dc"].reshape(-1, 3)
        assert dc[pc.ROW_CUT, 0] == 0.0 and dc[pc.ROW_CUT, 1] != 0.0 and dc[pc.ROW_CUT, 2] != 0.0
        if n_rows and first_off:
            assert not got["_features_rest"].reshape(-1, n_rows, 3)[pc.ROW_CUT, :, 0].any()


def _bar_8i(got, f64, comp32, scale=None):
    f64 = np.asarray(f64, np.float64)
    scale = np.abs(f64).max(initial=0.0) if scale is None else scale
    return np.abs(np.asarray(got, np.float64) - f64) <= 1e-5 * scale + 3.0 * np.abs(np.asarray(comp32, np.float64) - f64)


# ---------------------------------------------------------------------------------------------------------------------------------
# forward, per Gaussian
def _rects_of(pix, radii, W, H):
    """auxiliary.h:46-56 in float32, from float32 pixel means and integer radii"""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    px, py, rad = pix[:, 0].astype(np.float32), pix[:, 1].astype(np.float32), radii.astype(np.float32)

    def tile(v, g):
        return np.clip(np.trunc(v / np.float32(16)).astype(np.int64), 0, g)

    r = np.stack([tile(px - rad, gx), tile(py - rad, gy), tile(px + rad + np.float32(15), gx), tile(py + rad + np.float32(15), gy)],
                 axis=1)
    r[radii == 0] = 0
    return r


@pytest.mark.parametrize("name", IDS)
def test_forward_state_per_gaussian(name):
    from tests.gpu_helpers import inspect_fused
    from tests.test_project_fused import to_double, torch_pipeline
    case, dev = pc.BY_NAME[name], _dev()
    P, W, H = case.P, case.W, case.H
    model, cam = pc.build_model(case, dev), pc.build_view(case, dev)
    pf = render(cam, model, FUSED, syn.background(dev))
    torch.cuda.synchronize()
    ins = inspect_fused(pf.renders_packed, P, W, H, int(pf.count))
    radii = ins["radii"]
    assert radii.shape == (P,) and np.array_equal(radii, pf["radii"].cpu().numpy())
    # ---- the float64 projection and the composed float32 one on the device
    m64, c64 = to_double(pc.build_model(case, "cpu", owned=False), pc.build_view(case, "cpu"))
    with torch.no_grad():
        ref = [t.detach().numpy() for t in torch_pipeline(m64, c64)]
        m32 = pc.build_model(case, dev, owned=False)
        comp = [t.detach().cpu().numpy() for t in torch_pipeline(m32, cam)]
        pg = render(cam, m32, GENERIC, syn.background(dev))
    radii_g = pg["radii"].cpu().numpy()

    def pixels(ndc):
        ndc = ndc.astype(np.float64)
        return np.stack([((ndc[:, 0] + 1.0) * W - 1.0) * 0.5, ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5], axis=1)

    def record(t):  # (conic, means2D, colours, opacity, keep) -> [P, 16] in the layout of the packed record
        conic, m2d, colours, opac = t[:4]
        return np.concatenate([pixels(m2d), conic.astype(np.float64), opac.astype(np.float64).reshape(P, 1),
                               colours.astype(np.float64)], axis=1)

    rec64, rec32 = record(ref), record(comp)
    keep64, keep32 = ref[4].astype(bool), comp[4].astype(bool)
    # ---- radii and tile rects are the GENERIC path's, flips counted
    rect_g = _rects_of(pixels(pg["viewspace_points"].cpu().numpy()).astype(np.float32), radii_g, W, H)
    rg = ins["rects"]
    rect_f = np.stack([rg[:, 0] & 0xffff, rg[:, 1] & 0xffff, rg[:, 0] >> 16, rg[:, 1] >> 16], axis=1).astype(np.int64)
    flipped = (radii != radii_g) | (rect_f != rect_g).any(axis=1) | ((radii > 0) != keep64) | (keep32 != keep64)
    assert flipped.sum() <= _max_flips(P), (int(flipped.sum()), np.nonzero(flipped)[0][:8])
    vis = (radii > 0) & ~flipped
    assert vis.sum() >= max(1, 0.9 * P - 1)
    if not pc.planted(case):   # one to three lanes: every Gaussian is visible in double, none may be culled or left out
        assert keep64.all() and np.array_equal(radii > 0, keep64) and vis.all(), (radii, keep64, flipped)
    # ---- culled rows: radius 0, zero rect, all-zero record
    culled = radii == 0
    assert not ins["rec"][culled].any() and not rect_f[culled].any() and not rg[culled, :2].any()
    if pc.planted(case):
        assert culled[pc.ROW_BEHIND] and not flipped[:pc.N_PLANTED].any()
        others = [r for r in range(pc.N_PLANTED) if r != pc.ROW_BEHIND]
        assert (radii[others] > 0).all()
    # ---- every visible Gaussian's record, element by element, per quantity
    groups = dict(pixel_mean=(0, 2), conic=(2, 5), opacity=(5, 6), rgb=(6, 9), label=(9, 10), one=(10, 11), dir2d=(11, 14),
                  conf=(14, 15), depth=(15, 16))
    got = ins["rec"].astype(np.float64)
    bad = {}
    for q, (a, b) in groups.items():
        g, r, c = got[vis, a:b], rec64[vis, a:b], rec32[vis, a:b]
        ok = _bar_8i(g, r, c)
        if q == "dir2d" and pc.planted(case):
            # the row with two equal longest scales is judged WITHOUT the composed term: the composed chain picks its axis by an
            # argsort that may take either of the two on the device, and 3 |composed - f64| would then excuse any choice of the
            # kernel's.  1e-5 of the tensor's largest entry covers the kernel's own rounding (a dozen float32 operations on a
            # value no larger than that entry).
            t = int(np.count_nonzero(vis[:pc.ROW_TIE]))
            assert vis[pc.ROW_TIE]
            ok[t] = np.abs(g[t] - r[t]) <= 1e-5 * np.abs(r).max()
        if not ok.all():
            bad[q] = (int((~ok).sum()), float(np.abs(g - r).max()), float(np.abs(c - r).max()))
    d_ok = _bar_8i(ins["depths"][vis], rec64[vis, 15], rec32[vis, 15])
    assert not bad and d_ok.all(), (bad, int((~d_ok).sum()))
    assert (got[vis, 10] == 1.0).all() and (got[vis, 13] == 0.0).all()
    # the NDC means are written for every row, culled ones included
    vs = pf["viewspace_points"].detach().cpu().numpy()
    assert _bar_8i(vs[:, :2], ref[1][:, :2], comp[1][:, :2]).all()


@pytest.mark.parametrize("name", ["p1_k16", "p3_k4", "p65_k16", "p257_k4", "p513_k16", "p129_k1"])
def test_rows_up_to_the_next_multiple_of_256_are_culled_padding(name):
    """The padding contract of a segment's forward (include/ghr.h, ghr_model_forward_segment): workspace rows between the end of
    the segment and the next multiple of 256 get radius 0 and zero rects; nothing past them is written."""
    from gaussianhaircut_amd.gaussian_renderer.fused import _model_args
    case, dev = pc.BY_NAME[name], _dev()
    P, W, H = case.P, case.W, case.H
    rows = (P + 255) // 256 * 256
    total = rows + 256                                   # one more block of rows that nobody may touch
    model, cam = pc.build_model(case, dev, owned=False), pc.build_view(case, dev)
    params = [getattr(model, n).detach().contiguous() for n in
              ("_xyz", "_scaling", "_rotation", "_opacity", "_label", "_orient_conf", "_features_dc", "_features_rest")]
    gb, ib = _lib.forward_sizes(total, W, H, False)
    geom = torch.full((gb,), 0xAB, dtype=torch.uint8, device=dev)
    img = torch.zeros((ib,), dtype=torch.uint8, device=dev)
    radii = torch.full((total,), -7, dtype=torch.int32, device=dev)
    m2d = torch.full((total, 3), float("nan"), dtype=torch.float32, device=dev)
    bg = syn.background(dev)
    m = _model_args(P, W, H, case.active, (case.max_deg + 1) ** 2, params, cam.world_view_transform.contiguous(),
                    cam.full_proj_transform.contiguous(), cam.camera_center.contiguous(), bg, 1.0,
                    math.tan(float(cam.FoVx) * 0.5), math.tan(float(cam.FoVy) * 0.5), 1e-12, False)
    _lib.check(_lib.lib().ghr_model_forward_segment(_stream(), ctypes.byref(m), total, 1, _ptr(geom), _ptr(img), _ptr(radii),
                                                    _ptr(m2d)))
    torch.cuda.synchronize()
    v = _lib.WsView()
    _lib.check(_lib.lib().ghr_ws_inspect(total, W, H, 0, 0, _ptr(geom), _ptr(img), None, ctypes.byref(v)))
    off = int(v.rects) - geom.data_ptr()
    rects = geom[off:off + 16 * total].view(torch.int32).cpu().numpy().reshape(total, 4)
    r = radii.cpu().numpy()
    with torch.no_grad():
        expect = render(cam, model, FUSED, bg)["radii"].cpu().numpy()
    assert np.array_equal(r[:P], expect)
    assert not r[P:rows].any() and not rects[P:rows].any()
    assert (r[rows:] == -7).all() and (rects[rows:].view(np.uint8) == 0xAB).all()
    assert np.isnan(m2d[P:].cpu().numpy()).all() and np.isfinite(m2d[:P].cpu().numpy()).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# backward, every element of every raw-parameter gradient
@pytest.mark.parametrize("name", IDS)
def test_backward_every_gradient_element(name):
    case, dev = pc.BY_NAME[name], _dev()
    ref = _reference(case)
    model, cam = pc.build_model(case, dev), pc.build_view(case, dev)
    pkg = render(cam, model, FUSED, syn.background(dev))
    (pkg.renders_packed * ref["weights"].to(dev)).sum().backward()
    torch.cuda.synchronize()
    if case.owned:
        assert model.optimizer.direct_backwards == 1 and int(model.optimizer.state_dev[1]) == 0
    first_off, n_rows = pc.last_coeff_rows(case)
    _check_param_grads(name, _param_grads(model), [ref], first_off, n_rows, pc.planted(case), [])


# ---------------------------------------------------------------------------------------------------------------------------------
# accumulation: two views through the direct gradient sink
def _guard_flat_grad(opt, guard=64):
    """Moves the optimizer's flat gradient buffer between two guard areas filled with PATTERN (same 16-byte phase as before:
    `guard` is a multiple of four floats); the parameters' .grad views follow.  Returns the whole allocation as int32."""
    n = opt.flat_grad.numel()
    whole = torch.full((n + 2 * guard,), PATTERN, dtype=torch.int32, device=opt.flat_grad.device)
    inner = whole[guard:guard + n].view(torch.float32)
    inner.zero_()
    opt.flat_grad = inner
    off = 0
    for g in opt.param_groups:
        for p in g["params"]:
            p.grad = inner[off:off + p.numel()].view(p.shape)
            off += p.numel()
    assert off == n  # the groups tile the buffer: no word of it lies outside the model's arrays
    opt._mark_zero()
    return whole, guard, n


@pytest.mark.parametrize("name", OWNED_IDS)
def test_two_views_accumulate_through_the_direct_sink(name):
    case, dev = pc.BY_NAME[name], _dev()
    refs = [_reference(case, index=i) for i in (0, 1)]
    model = pc.build_model(case, dev)
    opt = model.optimizer
    opt.direct_grads = True
    whole, guard, n = _guard_flat_grad(opt)
    assert opt.flat_grad.data_ptr() % 16 == 0
    rest = model._features_rest
    assert rest.grad.data_ptr() % 16 == (0 if case.P % 2 == 0 else 8)   # xyz and f_dc lie in front: 24 P bytes
    assert rest.data_ptr() % 16 == rest.grad.data_ptr() % 16
    bg = syn.background(dev)
    for i in (0, 1):
        pkg = render(pc.build_view(case, dev, index=i), model, FUSED, bg)
        (pkg.renders_packed * refs[i]["weights"].to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert opt.direct_backwards == 2 and int(opt.state_dev[1]) == 0
    w = whole.cpu().numpy()
    assert (w[:guard] == PATTERN).all() and (w[guard + n:] == PATTERN).all(), "a store outside the gradient buffer"
    assert not (w[guard:guard + n] == PATTERN).any() and np.isfinite(w[guard:guard + n].view(np.float32)).all()
    first_off, n_rows = pc.last_coeff_rows(case)
    _check_param_grads(name + " two views", _param_grads(model), refs, first_off, n_rows, False, [])
    got = _param_grads(model)
    if pc.planted(case):   # (the row behind the first camera is in front of the second)
        dc = got["_features_dc"].reshape(-1, 3)
        assert dc[pc.ROW_CUT, 0] == 0.0 and dc[pc.ROW_CUT, 1] != 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the optimizer update fused into the last projection backward, at the tails
def _same_bits(a, b):
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


@pytest.mark.parametrize("name", OWNED_IDS)
def test_adam_fused_into_the_backward_is_bit_identical_at_the_tails(name):
    """tests/test_gpu_fused.py::test_adam_fused_into_the_last_projection_backward_is_bit_identical at the owned cases: a
    single-view step, a two-view step (the accumulate branch of slab_out_adam) and a step with NaN gradients."""
    from gaussianhaircut_amd.scene.cameras import ring_cameras
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    from gaussianhaircut_amd.trainer import make_ground_truth, training_step
    case, dev = pc.BY_NAME[name], _dev()
    opt = OptimizationParams()
    opt.lambda_dorient = 0.1
    cams = ring_cameras(2, case.W, case.H, device=dev)
    bg = syn.background(dev)
    gt = pc.build_model(case, dev, owned=False)
    with torch.no_grad():
        gt._features_dc.add_(0.3)
        gt._xyz.add_(0.01)
    make_ground_truth(gt, cams, bg)
    plan = [[cams[0]], [cams[0], cams[1]], [cams[1]]]
    bad_row = min(3, case.P - 1)
    _lib.lib().ghr_set_deterministic(1)
    try:
        runs = {}
        for fused in (True, False):
            model = pc.build_model(case, dev, owned=False)
            model.training_setup(opt)
            o = model.optimizer
            trace = []
            for it, views in enumerate(plan):
                if it == 2:
                    with torch.no_grad():
                        model._opacity[bad_row] = float("nan")
                training_step(model, views, bg, opt, it + 1, fuse_adam=fused)
                torch.cuda.synchronize()
                assert model._xyz.data_ptr() == o.flat_param.data_ptr()
                trace.append((o.flat_param.clone(), o.exp_avg.clone(), o.exp_avg_sq.clone(), int(o.state_dev[0])))
            assert o.fused_steps == (len(plan) if fused else 0), o.fused_steps
            if fused:
                # the NaN step was undone on the device: the `out` set (now current) holds the `in` set's bits
                f = o._fuse
                assert _same_bits(o.flat_param, f["p"]) and _same_bits(o.exp_avg, f["m"]) and _same_bits(o.exp_avg_sq, f["v"])
            runs[fused] = trace
        for it, (a, b) in enumerate(zip(runs[True], runs[False])):
            assert a[3] == b[3], (it, a[3], b[3])
            for what, x, y in zip(("p", "m", "v"), a[:3], b[:3]):
                assert _same_bits(x, y), (it, what, int((x != y).sum()), np.nonzero((x != y).cpu().numpy())[0][:8])
        assert [t[3] for t in runs[True]] == [1, 2, 2]
        # the NaN step left everything alone (but for the logit this test overwrote in front of it)
        before = [t.clone() for t in runs[True][1][:3]]
        nr = (case.max_deg + 1) ** 2 - 1
        before[0][6 * case.P + 3 * nr * case.P + bad_row] = float("nan")   # xyz | f_dc | f_rest | opacity
        for k in range(3):
            assert _same_bits(runs[True][2][k], before[k]), k
        assert not _same_bits(runs[True][1][0], runs[True][0][0])
        # the moments of the last Gaussian's last coefficients moved in both real steps
        if case.max_deg:
            P, nr = case.P, (case.max_deg + 1) ** 2 - 1
            end = 6 * P + 3 * nr * P     # xyz | f_dc | f_rest
            assert (runs[True][1][1][end - 3:end] != 0).all() and (runs[True][1][2][end - 3:end] != 0).all()
    finally:
        _lib.lib().ghr_set_deterministic(0)


# ---------------------------------------------------------------------------------------------------------------------------------
# camera cotangents: CAM -> cam_butterfly -> one column per 64 rows -> k_cam_fold
@pytest.mark.parametrize("name", pc.CAMERA_CASES)
def test_camera_cotangents(name):
    case, dev = pc.BY_NAME[name], _dev()
    ref = _reference(case, trainable=True)
    model, cam = pc.build_model(case, dev, owned=False), pc.build_view(case, dev, trainable=True)
    pkg = render(cam, model, FUSED, syn.background(dev))
    (pkg.renders_packed * ref["weights"].to(dev)).sum().backward()
    torch.cuda.synchronize()
    got = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in pc.camera_grads(cam).items()}
    g64, g32 = ref["g64"], ref["g32"]
    assert not got["view_direct"][:, 3].any(), got["view_direct"]
    report = []
    for k in ("world_view_transform", "view_direct"):
        ok = _bar_8i(got[k], g64[k], g32[k])
        report.append("%s %s: worst |HIP - f64| %.3g of max, oracle32 %.3g" % (
            name, k, np.abs(got[k] - g64[k]).max() / np.abs(g64[k]).max(), np.abs(g32[k] - g64[k]).max() / np.abs(g64[k]).max()))
        assert ok.all(), (k, got[k], g64[k], g32[k])
    fov = lambda g: np.array([float(g["FoVx"]), float(g["FoVy"])])
    report.append("%s FoV: HIP %s f64 %s oracle32 %s" % (name, fov(got), fov(g64), fov(g32)))
    print("\n".join(report), flush=True)
    assert _bar_8i(fov(got), fov(g64), fov(g32)).all(), report[-1]
    # the model's gradients of the same pass: the CAM instantiations are different kernels
    first_off, n_rows = pc.last_coeff_rows(case)
    _check_param_grads(name + " CAM", _param_grads(model), [ref], first_off, n_rows, pc.planted(case), [])


CAM_VIEW = [4 * (c // 3) + c % 3 for c in range(12)]
CAM_PROJ = [16 + 4 * (c // 3) + (3 if c % 3 == 2 else c % 3) for c in range(12)]
CAM_ZERO = [4 * r + 3 for r in range(4)] + [16 + 4 * r + 2 for r in range(4)]


def _fold(table, fov=None, guard=16):
    dev = table.device
    buf = torch.full((_lib.CAM_GRADS + 2 * guard,), float("nan"), dtype=torch.float32, device=dev)
    d_cam = buf[guard:guard + _lib.CAM_GRADS]
    _lib.check(_lib.lib().ghr_camera_grad_fold(_stream(), _ptr(table), table.shape[1], _ptr(d_cam),
                                               _ptr(fov[0]) if fov else None, _ptr(fov[1]) if fov else None))
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert np.isnan(b[:guard]).all() and np.isnan(b[guard + _lib.CAM_GRADS:]).all()
    return b[guard:guard + _lib.CAM_GRADS].astype(np.float64)


def _partials(n_slots, seed):
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (torch.rand(_lib.CAM_PARTIALS, n_slots, generator=g) * 9.0 - 6.0)   # 1e-6 .. 1e3
    sign = torch.where(torch.rand(_lib.CAM_PARTIALS, n_slots, generator=g) < 0.5, -1.0, 1.0)
    return (mag * sign).float().contiguous()


@pytest.mark.parametrize("n_slots", [1, 2, 63, 64, 1023, 1024, 1025, 8191, 8192, 8193, 16385])
def test_camera_grad_fold_sums_every_column(n_slots):
    """k_cam_fold alone: the `i < n_slots ? i : n_slots - 1` clamp, the 8 x 1024 trip and its second round.  One rounding to
    float plus the double accumulation's own bound: |got - S| <= 2^-24 |S| + n_slots 2^-53 sum |v|."""
    t = _partials(n_slots, 100 + n_slots)
    got = _fold(t.to(_dev()))
    v = t.numpy().astype(np.float64)
    S, A = v.sum(axis=1), np.abs(v).sum(axis=1)
    expect, slack = np.zeros(_lib.CAM_GRADS), np.zeros(_lib.CAM_GRADS)
    for idx, comps in ((CAM_VIEW, range(0, 12)), (CAM_PROJ, range(12, 24)), ([35, 36], (24, 25)), ([32, 33, 34], (26, 27, 28))):
        for i, c in zip(idx, comps):
            expect[i] = S[c]
            slack[i] = 2.0 ** -24 * abs(S[c]) + n_slots * 2.0 ** -53 * A[c]
    written = sorted(CAM_VIEW + CAM_PROJ + [32, 33, 34, 35, 36])
    assert sorted(written + CAM_ZERO) == list(range(_lib.CAM_GRADS))
    assert (np.abs(got - expect)[written] <= slack[written]).all(), (got - expect, slack)
    assert (np.abs(expect[written]) > 0).all()
    assert not got[CAM_ZERO].any() and not np.signbit(got[CAM_ZERO]).any()


@pytest.mark.parametrize("n_slots", [1, 1025])
def test_camera_grad_fold_with_fov_pointers(n_slots):
    dev = _dev()
    t = _partials(n_slots, 7 + n_slots)
    fx, fy = np.float32(0.93), np.float32(0.71)
    fov = (torch.tensor([fx], device=dev), torch.tensor([fy], device=dev))
    got = _fold(t.to(dev), fov)
    plain = _fold(t.to(dev))
    assert np.array_equal(got[:35], plain[:35])
    S = t.numpy().astype(np.float64).sum(axis=1)[24:26]
    f64 = S * 0.5 * (1.0 + np.tan(np.array([fx, fy], np.float64) * 0.5) ** 2)
    tt = np.tan(np.array([fx, fy], np.float32) * np.float32(0.5)).astype(np.float32)
    c32 = S.astype(np.float32) * (np.float32(0.5) * (np.float32(1.0) + tt * tt))
    assert _bar_8i(got[35:37], f64, c32).all(), (got[35:37], f64, c32)


# ---------------------------------------------------------------------------------------------------------------------------------
# k_sh_grad_from_views alone (it shares slab_out<64>)
@pytest.mark.parametrize("K", [1, 4, 9, 16])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 127])
def test_sh_grad_from_views_against_float64_autograd(P, K):
    from gaussianhaircut_amd.utils.sh_utils import eval_sh
    dev = _dev()
    max_deg = int(math.isqrt(K)) - 1
    g = torch.Generator().manual_seed(1000 * K + P)
    xyz = (torch.rand(P, 3, generator=g) * 2 - 1) * 1.3
    campos = torch.nn.functional.normalize(torch.randn(3, 3, generator=g), dim=1) * 4.0
    d_rgb = torch.randn(3, P, 3, generator=g)
    d_rgb[1, ::5] = 0.0          # rows without a gradient in view 1 are skipped by the kernel
    old_dc, old_rest = torch.randn(P, 1, 3, generator=g), torch.randn(P, max(K - 1, 0), 3, generator=g)
    xyz_d, cam_d, g_d = xyz.to(dev), campos.to(dev).contiguous(), d_rgb.to(dev).contiguous()

    def autograd_sum(dtype, device, deg, n_views):
        sh = torch.zeros(P, 3, K, dtype=dtype, device=device, requires_grad=True)
        x, c, gr = xyz.to(device, dtype), campos.to(device, dtype), d_rgb.to(device, dtype)
        loss = 0.0
        for v in range(n_views):
            d = x - c[v][None]
            d = d / d.norm(dim=1, keepdim=True)
            loss = loss + (eval_sh(deg, sh, d) * gr[v]).sum()
        loss.backward()
        return sh.grad.detach().transpose(1, 2)   # [P, K, 3]

    L = _lib.lib()
    degs = sorted({max_deg, max(max_deg - 1, 0), 0})
    for deg in degs:
        for n_views in (1, 3):
            r64 = autograd_sum(torch.float64, "cpu", deg, n_views).numpy()
            c32 = autograd_sum(torch.float32, dev, deg, n_views)
            for accumulate in (0, 1):
                # outputs between guards; the guard in front is 1 .. 4 floats: assigning AND accumulating (the 16-byte
                # read-modify-write of slab_out, its scalar tail, the dc read-add-write) meet every 4-byte phase
                for gd in (1, 2, 3, 4):
                    bufs = []
                    for old in (old_dc, old_rest):
                        b = torch.full((old.numel() + gd + 8,), float("nan"), dtype=torch.float32, device=dev)
                        if accumulate:
                            b[gd:gd + old.numel()] = old.reshape(-1).to(dev)
                        bufs.append(b)
                    dc, rest = bufs[0][gd:gd + 3 * P], bufs[1][gd:gd + 3 * (K - 1) * P]
                    _lib.check(L.ghr_sh_grad_from_views(_stream(), P, deg, K, _ptr(xyz_d), n_views, _ptr(cam_d), 3, _ptr(g_d), 3 * P,
                                                        _ptr(dc), _ptr(rest) if K > 1 else None, accumulate, None, 0))
                    torch.cuda.synchronize()
                    for b, n in zip(bufs, (3 * P, 3 * (K - 1) * P)):
                        h = b.cpu().numpy()
                        assert np.isnan(h[:gd]).all() and np.isnan(h[gd + n:]).all(), "a store outside the output"
                    got = np.concatenate([dc.cpu().numpy().reshape(P, 1, 3), rest.cpu().numpy().reshape(P, K - 1, 3)], axis=1)
                    old = torch.cat([old_dc, old_rest], dim=1)
                    ref = r64 + (old.double().numpy() if accumulate else 0.0)
                    cmp32 = (c32 + old.to(dev) if accumulate else c32).cpu().numpy()
                    tag = (P, K, deg, n_views, accumulate, gd)
                    assert np.isfinite(got).all(), tag
                    ok = _bar_8i(got, ref, cmp32)
                    assert ok.all(), (tag, int((~ok).sum()), float(np.abs(got - ref).max()), float(np.abs(cmp32 - ref).max()))
                    above = got[:, (deg + 1) ** 2:]
                    if accumulate:   # untouched old values
                        assert np.array_equal(above, old.numpy()[:, (deg + 1) ** 2:]), tag
                    else:
                        assert not above.any(), tag
