"""The per-strand SH segment on the device (csrc/ghr_shared.h), through the C ABI and end to end.

Per case of tests/shared_feature_cases.py: the forward with `_shared` on the per-strand arrays against ghr_model_forward_segment on
arrays expanded with torch.repeat -- radii, means2D, records, rects, depths, tile ranges, point list and image bit-identical;
then ONE ghr_render_backward and both projection backward forms over the same gradient lines (K8's scheduling order does not enter)
-- every per-row gradient bit-identical, the per-strand feature gradients equal as floats to ghr_strand_rows_reduce of the
ordinary form's rows.  Outputs land in NaN-filled buffers between NaN guards.  No element is excluded anywhere."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd.utils import synthetic as syn
from tests import helpers as hp
from tests import shared_feature_cases as sc

pytestmark = pytest.mark.gpu
GUARD = 8  # rows of NaN in front of and behind every output


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _seg(sce, t, P, row0, cam, eps, consts):
    m = _lib.ModelArgs()
    m.P, m.W, m.H, m.sh_degree, m.sh_coeffs = int(P), sce["W"], sce["H"], sce["sh_degree"], sce["K"]
    m.xyz, m.log_scales, m.rotations = _ptr(t["xyz"]), _ptr(t["scaling"]), _ptr(t["rotation"])
    m.opacity_logit = _ptr(t.get("opacity"))
    m.orient_conf_log, m.dir3d = _ptr(t.get("conf")), _ptr(t.get("dir"))
    m.features_dc, m.features_rest = _ptr(t["fdc"]), _ptr(t["frest"])
    m.viewmatrix, m.projmatrix, m.campos, m.background = [_ptr(cam[k]) for k in ("view", "proj", "campos", "bg")]
    m.scale_modifier, m.tan_fovx, m.tan_fovy, m.conic_eps = 1.0, sce["tanfovx"], sce["tanfovy"], eps
    m.mode, m.row0 = 1, int(row0)
    m.const_opacity, m.const_label, m.const_conf = consts
    return m


class Run:
    """one rasterizer state of head + hair; `shared`: the hair segment's coefficients stay per strand"""

    def __init__(self, sce, dev, shared):
        L = _lib.lib()
        self.L, self.sce, self.shared, self.dev = L, sce, shared, dev
        S, n_seg, P, n_head, W, H = sce["S"], sce["n_seg"], sce["P"], sce["n_head"], sce["W"], sce["H"]
        f = lambda t: t.to(dev).float().contiguous()  # noqa: E731
        self.cam = dict(view=f(sce["view"]), proj=f(sce["proj"]), campos=f(sce["campos"]), bg=syn.background(dev))
        fdc, frest = f(sce["f_dc"]), f(sce["f_rest"])
        if not shared and n_seg > 1:
            fdc, frest = f(sc.expanded(sce["f_dc"], n_seg)), f(sc.expanded(sce["f_rest"], n_seg))
        assert fdc.shape[0] == (S if shared or n_seg == 1 else P)     # (n_seg = 1: the SAME arrays, no expansion involved)
        self.hair = dict(xyz=f(sce["xyz"]), scaling=f(sce["scaling"]), rotation=f(sce["rotation"]), dir=f(sce["dir"]),
                         conf=f(sce["conf"]), fdc=fdc, frest=frest)
        K = sce["K"]
        if n_head:
            self.head = {k: f(v) for k, v in sce["head"].items()}
        else:
            z = lambda *s: torch.zeros(s, device=dev)  # noqa: E731
            self.head = dict(xyz=z(0, 3), scaling=z(0, 3), rotation=z(0, 4), opacity=z(0), fdc=z(0, 1, 3), frest=z(0, K - 1, 3))
        self.row0 = (n_head + 255) // 256 * 256
        self.rows = rows = self.row0 + P
        self.sf = _lib.SharedFeatures()
        self.sf.n_strands, self.sf.rows_per_strand = S, n_seg
        self.m_head = _seg(sce, self.head, n_head, 0, self.cam, 1e-12, (1.0, 0.0, 0.0))
        self.m_hair = _seg(sce, self.hair, P, self.row0, self.cam, 1e-7, (1.0, 1.0, 0.0))
        gb, ib = _lib.forward_sizes(rows, W, H, False)
        self.geom = torch.zeros(gb, dtype=torch.uint8, device=dev)
        self.img = torch.zeros(ib, dtype=torch.uint8, device=dev)
        self.radii = torch.full((rows,), -7, dtype=torch.int32, device=dev)
        self.m2d = torch.full((rows, 3), float("nan"), device=dev)
        self.pinned = torch.zeros(1, dtype=torch.int32).pin_memory()
        chk = _lib.check
        chk(L.ghr_model_forward_segment(_stream(), ctypes.byref(self.m_head), rows, 1, _ptr(self.geom), _ptr(self.img),
                                        _ptr(self.radii), _ptr(self.m2d)))
        if shared:
            chk(L.ghr_model_forward_segment_shared(_stream(), ctypes.byref(self.m_hair), ctypes.byref(self.sf), rows, 0,
                                                   _ptr(self.geom), _ptr(self.img), _ptr(self.radii), _ptr(self.m2d)))
        else:
            chk(L.ghr_model_forward_segment(_stream(), ctypes.byref(self.m_hair), rows, 0, _ptr(self.geom), _ptr(self.img),
                                            _ptr(self.radii), _ptr(self.m2d)))
        chk(L.ghr_model_forward_finish(_stream(), rows, W, H, 0, _ptr(self.geom), _ptr(self.img),
                                       ctypes.c_void_p(self.pinned.data_ptr())))
        torch.cuda.synchronize()
        self.R = R = int(np.uint32(self.pinned[0].item()))
        self.va = va = _lib.ViewArgs()
        va.P, va.W, va.H, va.C, va.background = rows, W, H, 10, _ptr(self.cam["bg"])
        self.bin = torch.zeros(_lib.binning_size(R, W, H), dtype=torch.uint8, device=dev)
        self.out = torch.full((10, H, W), float("nan"), device=dev)
        chk(L.ghr_forward_stage2(_stream(), ctypes.byref(va), R, _ptr(self.geom), _ptr(self.img), _ptr(self.bin), _ptr(self.out),
                                 None))
        torch.cuda.synchronize()

    def state(self):
        from tests.gpu_helpers import _slice
        v = _lib.WsView()
        rows, W, H, R = self.rows, self.sce["W"], self.sce["H"], self.R
        _lib.check(self.L.ghr_ws_inspect(rows, W, H, 0, R, _ptr(self.geom), _ptr(self.img), _ptr(self.bin) if R else None,
                                         ctypes.byref(v)))
        T = ((W + 15) // 16) * ((H + 15) // 16)
        hair = slice(self.row0, self.rows)
        vis = self.radii.cpu().numpy()[hair] > 0
        depths = _slice(self.geom, v.depths, 4 * rows, torch.float32).numpy()[hair]
        return dict(radii=self.radii.cpu().numpy(), means2D=self.m2d.cpu().numpy(), image=self.out.cpu().numpy(),
                    rec=_slice(self.geom, v.rec, 64 * rows, torch.float32).numpy().reshape(rows, 16)[hair],
                    rects=_slice(self.geom, v.rects, 16 * rows, torch.int32).numpy().reshape(rows, 4)[hair],
                    depths_visible=depths[vis],                 # (a culled row's depth is not stored)
                    tile_start=_slice(self.img, v.tile_start, 4 * (T + 1), torch.int32).numpy(),
                    point_list=_slice(self.bin, v.point_list, 4 * R, torch.int32).numpy() if R else np.zeros(0, np.int32))

    def render_backward(self, dL):
        self.scratch = torch.full((max(self.R, 1), _lib.GRAD_STRIDE), float("nan"), device=self.dev)
        _lib.check(self.L.ghr_render_backward(_stream(), self.rows, self.sce["W"], self.sce["H"], self.R, _ptr(self.cam["bg"]),
                                              _ptr(self.geom), _ptr(self.img), _ptr(self.bin), _ptr(dL), _ptr(self.scratch), 0))
        torch.cuda.synchronize()


def _guarded(rows, width, dev):
    return torch.full((rows + 2 * GUARD, width), float("nan"), device=dev)


def _projection_backward(run, other, shared, with_cam):
    """the hair segment's projection backward of `other`'s form over `run`'s state and gradient lines -> dict of numpy arrays"""
    L, sce, dev = run.L, run.sce, run.dev
    S, n_seg, P, K, n_head = sce["S"], sce["n_seg"], sce["P"], sce["K"], sce["n_head"]
    rows, row0 = run.rows, run.row0
    F = S if shared else other.hair["fdc"].shape[0]
    buf = dict(d_means2D=_guarded(rows, 3, dev), d_xyz=_guarded(P, 3, dev), d_scaling=_guarded(P, 3, dev),
               d_rotation=_guarded(P, 4, dev), d_conf=_guarded(P, 1, dev), d_dir=_guarded(P, 3, dev),
               d_fdc=_guarded(F, 3, dev), d_frest=_guarded(F, 3 * (K - 1), dev), d_rgb=_guarded(P, 3, dev))
    p = {k: ctypes.c_void_p(v.data_ptr() + 4 * GUARD * v.shape[1]) for k, v in buf.items()}
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    m_hair, m_head = other.m_hair, other.m_head
    table = None
    if with_cam:
        slots = [int(L.ghr_camera_slots(n)) for n in (n_head, P)]
        table = torch.full((_lib.CAM_PARTIALS, sum(slots)), float("nan"), device=dev)
        for m, s0 in ((m_head, 0), (m_hair, slots[0])):
            m.cam_partial, m.cam_slot0, m.cam_slots = _ptr(table), s0, sum(slots)
        m_head.cam_only, m_head.detach_means2D = 1, 1
        if n_head:
            _lib.check(L.ghr_model_backward_segment(_stream(), ctypes.byref(m_head), rows, _ptr(run.radii), _ptr(run.geom),
                                                    _ptr(run.scratch), *([None] * 10), 0, None, run.scratch.shape[0],
                                                    _ptr(run.bin), run.R))
    common = (rows, _ptr(run.radii), _ptr(run.geom), _ptr(run.scratch), p["d_means2D"], p["d_xyz"], p["d_scaling"],
              p["d_rotation"], None, None, p["d_conf"], p["d_fdc"], p["d_frest"] if K > 1 else None, p["d_dir"])
    if shared:
        _lib.check(L.ghr_model_backward_segment_shared(_stream(), ctypes.byref(m_hair), ctypes.byref(other.sf), *common,
                                                       _ptr(flag), run.scratch.shape[0], _ptr(run.bin), run.R, p["d_rgb"]))
    else:
        _lib.check(L.ghr_model_backward_segment(_stream(), ctypes.byref(m_hair), *common, 0, _ptr(flag), run.scratch.shape[0],
                                                _ptr(run.bin), run.R))
    torch.cuda.synchronize()
    out = {}
    for k, v in buf.items():
        a = v.cpu().numpy()
        assert np.isnan(a[:GUARD]).all() and np.isnan(a[-GUARD:]).all(), k       # the guards on both sides are untouched
        out[k] = a[GUARD:-GUARD]
    # d_means2D is indexed by workspace row: exactly the hair rows are written
    assert np.isnan(out["d_means2D"][:row0]).all() and np.isfinite(out["d_means2D"][row0:]).all()
    out["d_means2D"] = out["d_means2D"][row0:]
    out["flag"] = int(flag.item())
    if with_cam:
        d_cam = torch.full((_lib.CAM_GRADS,), float("nan"), device=dev)
        _lib.check(L.ghr_camera_grad_fold(_stream(), _ptr(table), table.shape[1], _ptr(d_cam), None, None))
        out["d_cam"] = d_cam.cpu().numpy()
        for m in (m_head, m_hair):
            m.cam_partial, m.cam_slot0, m.cam_slots, m.cam_only, m.detach_means2D = None, 0, 0, 0, 0
    if not shared:
        # ghr_strand_rows_reduce of the ordinary form's rows (n_seg = 1: the rows themselves)
        red = {}
        for k, C in (("d_fdc", 3), ("d_frest", 3 * (K - 1))):
            src = buf[k][GUARD:GUARD + F].contiguous()
            dst = torch.full((S, C), float("nan"), device=dev)
            if C > 0:
                _lib.check(L.ghr_strand_rows_reduce(_stream(), S, P // S if F == P else 1, C, _ptr(src), _ptr(dst)))
            red[k] = dst.cpu().numpy()
        out["red"] = red
    return out


ROW_KEYS = ("d_means2D", "d_xyz", "d_scaling", "d_rotation", "d_dir", "d_conf")


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_gpu_shared_segment_equals_the_expanded_form(case):
    S, n_seg, K, n_head = case
    dev = torch.device("cuda:0")
    sce = sc.make_scene(*case)
    P = sce["P"]
    a, b = Run(sce, dev, True), Run(sce, dev, False)
    # 1. forward parity
    sa, sb = a.state(), b.state()
    assert a.R == b.R
    for k in sb:
        assert sa[k].tobytes() == sb[k].tobytes(), k
    hair_radii = sb["radii"][a.row0:]
    behind = sc.behind_strand(S)
    if behind is not None:
        assert (hair_radii[behind * n_seg:(behind + 1) * n_seg] == 0).all()
    assert (hair_radii > 0).any() and a.R > 0 and np.isfinite(sb["image"]).all()
    # 2. backward parity: ONE gradient walk, both projection backward forms over its lines
    g = torch.Generator().manual_seed(5)
    dL = torch.randn(10, sce["H"], sce["W"], generator=g).to(dev)
    a.render_backward(dL)
    with_cam = case == (7, 3, 16, 300)
    ga = _projection_backward(a, a, True, with_cam)
    gb = _projection_backward(a, b, False, with_cam)
    for k in ROW_KEYS + (("d_cam",) if with_cam else ()):
        assert ga[k].tobytes() == gb[k].tobytes() and np.isfinite(gb[k]).all(), k
    assert ga["flag"] == 0 and gb["flag"] == 0
    dc, rest = ga["d_fdc"], ga["d_frest"]
    assert dc.shape == (S, 3) and np.isfinite(dc).all() and np.isfinite(rest).all()       # exactly S rows, all written
    assert sc.same_floats(dc, gb["red"]["d_fdc"])
    if K > 1:
        assert sc.same_floats(rest, gb["red"]["d_frest"])
    # the factored table is the ordinary form's dL/d(rgb): zero exactly on the rows without gradient
    assert np.isfinite(ga["d_rgb"]).all() and (ga["d_rgb"][hair_radii <= 0] == 0).all()
    # 3. non-vacuity, on the ordinary side
    n_act = (sce["sh_degree"] + 1) ** 2
    ref = np.concatenate([gb["red"]["d_fdc"].reshape(S, 1, 3), gb["red"]["d_frest"].reshape(S, K - 1, 3)], axis=1)
    s = sc.wave_crossing_strand(S, n_seg)
    assert (np.abs(ref[s, :n_act]).max(axis=1) > 0).all(), s
    if behind is not None:
        assert (ref[behind] == 0).all() and (gb["d_fdc"][behind * n_seg:(behind + 1) * n_seg] == 0).all()


def test_gpu_shared_fold_carries_non_finite_factors_and_raises_the_flag():
    """NaN in the red channel of every gradient line: NaN in the red column of every strand the view sees, exact zeros for the
    strand behind the camera, the same floats as the ordinary form, nan_flag raised by both (the one-strand-only case runs on the
    host simulator, tests/test_shared_features_cpu.py)"""
    case = (4, 65, 4, 0)
    S, n_seg, K, _ = case
    dev = torch.device("cuda:0")
    sce = sc.make_scene(*case)
    a, b = Run(sce, dev, True), Run(sce, dev, False)
    g = torch.Generator().manual_seed(5)
    a.render_backward(torch.randn(10, sce["H"], sce["W"], generator=g).to(dev))
    a.scratch[:, 6] = float("nan")       # channel 6 of a packed line: dL/d(red)
    ga = _projection_backward(a, a, True, False)
    gb = _projection_backward(a, b, False, False)
    assert ga["flag"] == 1 and gb["flag"] == 1
    assert sc.same_floats(ga["d_fdc"], gb["red"]["d_fdc"]) and sc.same_floats(ga["d_frest"], gb["red"]["d_frest"])
    assert np.isnan(ga["d_fdc"][:S - 1, 0]).all() and np.isfinite(ga["d_fdc"][:, 1:]).all()
    assert (ga["d_fdc"][S - 1] == 0).all() and (ga["d_frest"][S - 1] == 0).all()


# --------------------------------------------------------------------------------------------------------------- end to end
FUSED = SimpleNamespace(debug=False, fused_projection=True)
GENERIC = SimpleNamespace(debug=False, fused_projection=False)


def _scene(dev, fused=True, l_diff=None, shared=False):
    """tests/test_gpu_latent_stage.py::_scene with the option: 40 strands x 10 segments, toy generator"""
    from gaussianhaircut_amd.gaussian_renderer import render_hair
    from gaussianhaircut_amd.scene.gaussian_model_latent_strands import GaussianModelLatentStrands
    from tests.test_api_cpu import _hair_scene
    from tests.test_gpu_latent_stage import ToyGenerator
    spec, head, strands, cam = _hair_scene(dev)
    pts = strands._pts.detach()
    hair = GaussianModelLatentStrands(3, ToyGenerator(pts, 16, l_diff), None, fused=fused, shared_appearance=shared)
    bg = syn.background(dev)
    with torch.no_grad():
        gt = GaussianModelLatentStrands(3, ToyGenerator(pts * 1.03, 16), None)
        gt.strands_generator.lin.bias.add_(0.3)
        gt.initialize_gaussians_hair(0)
        pkg = render_hair(cam, head, gt, FUSED, bg)
        cam.original_image = pkg["render"].clamp(0, 1).detach()
        cam.original_mask = pkg["mask"].clamp(0, 1).detach()
        cam.original_orient_angle = pkg["orient_angle"].detach()
        cam.original_orient_conf = torch.ones_like(pkg["orient_conf"]).detach()
    return head, hair, cam, bg


def test_gpu_latent_stage_with_per_strand_features_end_to_end():
    from gaussianhaircut_amd.gaussian_renderer import render_hair
    from gaussianhaircut_amd.trainer import latent_strand_training_step, latent_view_loss
    from tests.test_gpu_latent_stage import _graph_has, _opt
    dev = torch.device("cuda:0")
    L = _lib.lib()
    L.ghr_set_deterministic(1)
    try:
        res = {}
        for form in ("shared", "fused", "composed"):
            head, hair, cam, bg = _scene(dev, form != "composed", "real", shared=form == "shared")
            hair.initialize_gaussians_hair(1)
            if form == "shared":
                assert hair.feature_rows_per_strand == 10 and tuple(hair._features_dc.shape) == (40, 1, 3)
                assert tuple(hair._features_rest.shape) == (40, 15, 3) and tuple(hair.get_features.shape) == (400, 16, 3)
                assert not _graph_has(hair._features_dc, "_RowsExpand") and not _graph_has(hair._features_rest, "_RowsExpand")
                assert _graph_has(hair._orient_conf, "_RowsExpand")        # 1 of 49 floats keeps today's path
            elif form == "fused":
                assert hair.feature_rows_per_strand == 0 and _graph_has(hair._features_dc, "_RowsExpand")
            pkg = render_hair(cam, head, hair, FUSED, bg)
            assert type(pkg.renders_packed.grad_fn).__name__.startswith("_RenderHairFused")
            loss = latent_view_loss(pkg, cam, _opt(), l_diff=hair.LDiff, fused=form != "composed")
            loss.backward()
            res[form] = (loss.detach().cpu().numpy(), {n: q.grad.detach().cpu().numpy()
                                                       for n, q in hair.strands_generator.named_parameters()})
        (ls, gs), (lf, gf), (lc_, gc) = res["shared"], res["fused"], res["composed"]
        assert ls.tobytes() == lf.tobytes()                                   # the loss has the same bits
        assert set(gs) == set(gf)
        for n in gf:
            assert sc.same_floats(gs[n], gf[n]) and np.abs(gf[n]).max() > 0, n  # every generator gradient equal as floats
        assert hp.image_close(np.float64(ls), np.float64(lc_)).all()
        hp.assert_grads_close(gs, gc)
        # three training steps leave the same parameter bits as with the option off
        finals = {}
        for shared in (True, False):
            head, hair, cam, bg = _scene(dev, True, None, shared=shared)
            hair.training_setup(_opt())
            for i in range(3):
                latent_strand_training_step(head, hair, [cam], bg, _opt(), i + 1, pipe=FUSED)
            assert (hair.feature_rows_per_strand == 10) == shared
            finals[shared] = {n: q.detach().cpu().numpy() for n, q in hair.strands_generator.named_parameters()}
        for n in finals[False]:
            assert finals[True][n].tobytes() == finals[False][n].tobytes(), n
        # the generic path on the shared model reads get_features: the same picture as on the default model
        pk = {}
        with torch.no_grad():
            for shared in (True, False):
                head, hair, cam, bg = _scene(dev, True, None, shared=shared)
                hair.initialize_gaussians_hair(1)
                pk[shared] = render_hair(cam, head, hair, GENERIC, bg)
        for k in ("render", "mask", "orient_angle", "orient_conf", "radii"):
            assert torch.equal(pk[True][k], pk[False][k]), k
    finally:
        L.ghr_set_deterministic(0)
