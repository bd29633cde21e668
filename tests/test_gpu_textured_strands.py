"""The textured strand generator on the GPU (csrc/ghr_texstrands.h through gaussianhaircut_amd/strand_generator.py).

Both forms -- the HIP one and the PyTorch-composed float32 one on the device -- are held against the float64 arbiter of
tests/texstrands_cases.py under DESIGN.md 8i's bar,
    |got - f64| <= 1e-5 max|f64| + 3 |composed float32 on the device - f64|      elementwise;
``pos`` and the inverted lists are compared bit for bit.  Shapes (tests/texstrands_cases.py SHAPES): T T around the 64-texel
workgroup, C around the 64-channel pass, Smax and S around the wave, L - 1 around the scan's 64 lanes; every root at one UV, UVs
at the four corners, on texel centres, beyond the texture, a draw that leaves a texel's whole list out."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd import strand_generator as sg
from tests import texstrands_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FUSED = SimpleNamespace(debug=False, fused_projection=True)
GUARD = 64


def _run(c, fused, d_p=True, d_pl=True):
    tex = c["texture"].to(DEV).requires_grad_(True)
    taps, idx = c["taps"].to(DEV), c["idx"].to(DEV)
    z = sg.sample_texture(tex, taps, idx, fused=fused)
    (d_tex,) = torch.autograd.grad(z, tex, c["d_z"].to(DEV))
    v = c["v"].to(DEV).requires_grad_(True)
    p, pl = sg.strands_to_world(v, c["local2world"].to(DEV), c["origins"].to(DEV), idx, c["scale"], fused=fused, return_local=True)
    cots = [g for g, on in ((c["d_p"], d_p), (c["d_pl"], d_pl)) if on]
    outs = [o for o, on in ((p, d_p), (pl, d_pl)) if on]
    (d_v,) = torch.autograd.grad(outs, v, [g.to(DEV) for g in cots])
    return dict(z=z.detach(), d_texture=d_tex, p=p.detach(), p_local=pl.detach(), d_v=d_v)


@pytest.mark.parametrize("name", sorted(tc.SHAPES))
def test_both_forms_against_float64(name):
    c = tc.case(name)
    r64 = c["r64"]
    comp, fused = _run(c, False), _run(c, True)
    for k in ("z", "d_texture", "p", "p_local", "d_v"):
        tc.assert_within("composed " + k, comp[k], r64[k], comp[k])
        tc.assert_within("fused " + k, fused[k], r64[k], comp[k])
    assert torch.equal(fused["p"][:, 0].cpu(), c["origins"][c["idx"]]) and float(fused["p_local"][:, 0].abs().max()) == 0.0
    again = _run(c, True)                                                # two passes give the same bits
    for k in ("z", "d_texture", "p", "p_local", "d_v"):
        assert torch.equal(again[k], fused[k]), k
    if c["mode"] == "beyond":
        assert float(fused["z"].abs().max()) == 0.0 and float(fused["d_texture"].abs().max()) == 0.0
    if c["mode"] == "leftout":                                           # the texel of the roots that were not drawn gets zeros
        tp = c["taps"]
        for k in range(4):
            assert float(fused["d_texture"][0, :, int(tp.y0[0]) + (k >> 1), int(tp.x0[0]) + (k & 1)].abs().max()) == 0.0


@pytest.mark.parametrize("name", ["L2", "L3", "L65", "L66", "L100", "L130", "Smax65-S32"])
def test_each_cotangent_of_the_points_alone(name):
    c = tc.case(name)
    for kw in (dict(d_p=True, d_pl=False), dict(d_p=False, d_pl=True)):
        r64 = tc.restate(c, **kw)
        comp, fused = _run(c, False, **kw), _run(c, True, **kw)
        assert float(r64["d_v"].abs().max()) > 0
        tc.assert_within("composed d_v %s" % kw, comp["d_v"], r64["d_v"], comp["d_v"])
        tc.assert_within("fused d_v %s" % kw, fused["d_v"], r64["d_v"], comp["d_v"])


@pytest.mark.parametrize("name", ["T65", "C129", "Smax300-S150", "one", "leftout"])
def test_texture_gradient_does_not_depend_on_the_order_of_the_draw(name):
    c = dict(tc.case(name))
    a = _run(c, True)["d_texture"]
    perm = torch.randperm(c["S"], generator=torch.Generator().manual_seed(2))
    c["idx"], c["d_z"] = c["idx"][perm], c["d_z"][perm]
    assert torch.equal(_run(c, True)["d_texture"], a)


def _guarded(numel, dtype):
    fill = float("nan") if dtype == torch.float32 else -7
    buf = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, ctypes.c_void_p(buf.data_ptr() + GUARD * buf.element_size())


def _body(name, buf, numel):
    head, body, tail = buf[:GUARD], buf[GUARD:GUARD + numel], buf[GUARD + numel:]
    if buf.dtype == torch.float32:
        assert bool(torch.isnan(head).all()) and bool(torch.isnan(tail).all()), name
        assert not bool(torch.isnan(body).any()), name                  # every element was ASSIGNED
    else:
        assert bool((head == -7).all()) and bool((tail == -7).all()) and not bool((body == -7).any()), name
    return body


@pytest.mark.parametrize("name", sorted(tc.SHAPES))
def test_outputs_land_in_nan_filled_buffers_between_guards(name):
    c = tc.case(name)
    Smax, S, T, C, n = c["Smax"], c["S"], c["T"], c["C"], c["n"]
    L = _lib.lib()
    f32, i32 = torch.float32, torch.int32
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    tp, idx = c["taps"].to(DEV), c["idx"].to(DEV)
    tex, d_z, v = c["texture"].to(DEV).contiguous(), c["d_z"].to(DEV).contiguous(), c["v"].to(DEV).contiguous()
    l2w, org = c["local2world"].to(DEV).contiguous(), c["origins"].to(DEV).contiguous()
    d_p, d_pl = c["d_p"].to(DEV).contiguous(), c["d_pl"].to(DEV).contiguous()   # (named: they must outlive the call)
    assert tp.start.cpu().numpy().tobytes() == c["r64"]["start"].numpy().tobytes()
    assert tp.list.cpu().numpy().tobytes() == c["r64"]["list"].numpy().tobytes()
    sizes = dict(z=(S * C, f32), pos=(Smax, i32), d_texture=(C * T * T, f32), p=(S * (n + 1) * 3, f32), p_local=(S * (n + 1) * 3, f32),
                 d_v=(S * n * 3, f32))
    b = {k: _guarded(*s) for k, s in sizes.items()}
    _lib.check(L.ghr_ts_fetch(stream, Smax, S, T, C, p(tex), p(tp.x0), p(tp.y0), p(tp.fx), p(tp.fy), p(idx), b["z"][1]))
    _lib.check(L.ghr_ts_fetch_backward(stream, Smax, S, T, C, p(tp.fx), p(tp.fy), p(tp.start), p(tp.list) if tp.list.numel() else None,
                                       int(tp.list.numel()), p(idx), p(d_z), b["pos"][1], b["d_texture"][1]))
    _lib.check(L.ghr_ts_world(stream, Smax, S, n, p(v), p(l2w), p(org), p(idx), 1.0 / c["scale"], b["p"][1], b["p_local"][1]))
    _lib.check(L.ghr_ts_world_backward(stream, Smax, S, n, p(l2w), p(idx), 1.0 / c["scale"], p(d_p), p(d_pl), b["d_v"][1]))
    body = {k: _body(k, b[k][0], sizes[k][0]) for k in sizes}
    r64 = c["r64"]
    assert torch.equal(body["pos"].long().cpu(), r64["pos"])
    comp = _run(c, False)
    for k in ("z", "d_texture", "p", "p_local", "d_v"):
        tc.assert_within(k, body[k].view(r64[k].shape), r64[k], comp[k])
    pw, ppw = _guarded(S * (n + 1) * 3, f32)                              # p_local = NULL: only p is written
    _lib.check(L.ghr_ts_world(stream, Smax, S, n, p(v), p(l2w), p(org), p(idx), 1.0 / c["scale"], ppw, None))
    assert torch.equal(_body("p alone", pw, S * (n + 1) * 3), body["p"])


def test_an_index_outside_the_roots_reads_nothing():
    c = tc.case("T5")
    idx = c["idx"].clone()
    idx[2] = c["Smax"] + 100
    z = sg.sample_texture(c["texture"].to(DEV), c["taps"].to(DEV), idx.to(DEV), validate=False)
    p = sg.strands_to_world(c["v"].to(DEV), c["local2world"].to(DEV), c["origins"].to(DEV), idx.to(DEV), c["scale"])
    keep = [i for i in range(c["S"]) if i != 2]
    assert bool(torch.isnan(z[2]).all()) and bool(torch.isfinite(z[keep]).all())
    assert bool(torch.isnan(p[2]).all()) and bool(torch.isfinite(p[keep]).all())
    with pytest.raises(ValueError, match="outside"):
        sg.sample_texture(c["texture"].to(DEV), c["taps"].to(DEV), idx.to(DEV))
    with pytest.raises(ValueError, match="twice"):
        sg.sample_texture(c["texture"].to(DEV), c["taps"].to(DEV), torch.tensor([1, 1], device=DEV))


def test_buffers_on_another_device_or_of_another_type_are_refused_in_python():
    c = tc.case("T5")
    tex, taps, idx = c["texture"].to(DEV), c["taps"].to(DEV), c["idx"].to(DEV)
    v, l2w, org = c["v"].to(DEV), c["local2world"].to(DEV), c["origins"].to(DEV)
    with pytest.raises(ValueError, match="x0 must be"):
        sg.sample_texture(tex, c["taps"], idx)                              # taps as texture_taps returns them: on the CPU
    with pytest.raises(ValueError, match="idx must be"):
        sg.sample_texture(tex, taps, c["idx"], validate=False)
    with pytest.raises(ValueError, match="fx must be"):
        sg.sample_texture(tex, taps._replace(fx=taps.fx.double()), idx)
    with pytest.raises(ValueError, match="start must be"):
        sg.sample_texture(tex, taps._replace(start=taps.start.long()), idx)
    with pytest.raises(ValueError, match="taps must be"):
        sg.sample_texture(tex, taps._replace(start=taps.start[:-1]), idx)
    with pytest.raises(ValueError, match="origins must be"):
        sg.strands_to_world(v, l2w, c["origins"], idx, c["scale"])
    with pytest.raises(ValueError, match="local2world must be"):
        sg.strands_to_world(v, c["local2world"], org, idx, c["scale"])
    with pytest.raises(ValueError, match="idx must be"):
        sg.strands_to_world(v, l2w, org, c["idx"], c["scale"])
    p64 = sg.strands_to_world(v, l2w.double(), org.double(), idx, c["scale"])   # frames of another float type are converted
    assert torch.equal(p64, sg.strands_to_world(v, l2w, org, idx, c["scale"]))


def test_against_grid_sample_on_the_device():
    """F.grid_sample is the second comparator: its float32 coordinates cost about 1e-5 of the range at T = 256 (printed), the
    stored float64 taps 4 * 2^-24 of it (asserted against F.grid_sample in double on the CPU)."""
    import torch.nn.functional as F
    T, C, Smax = 256, 4, 5000
    g = torch.Generator().manual_seed(12)
    uvs = torch.rand(Smax, 2, generator=g) * 2.1 - 1.05
    tex = torch.rand(1, C, T, T, generator=g) * 2 - 1
    taps = sg.texture_taps(uvs, T).to(DEV)
    idx = torch.arange(Smax, device=DEV)
    want = F.grid_sample(tex.double(), uvs.double().view(1, 1, Smax, 2), mode="bilinear", padding_mode="zeros", align_corners=False)[0, :, 0].t()
    got = sg.sample_texture(tex.to(DEV), taps, idx, fused=True).cpu().double()
    gs = F.grid_sample(tex.to(DEV), uvs.to(DEV).view(1, 1, Smax, 2), mode="bilinear", padding_mode="zeros", align_corners=False)[0, :, 0].t()
    err, err_gs = float((got - want).abs().max()), float((gs.cpu().double() - want).abs().max())
    print("T = 256: HIP fetch %.3e, F.grid_sample(float32) on the device %.3e of the range" % (err, err_gs))
    # 4 * 2^-24 for fx, fy rounded to float32 (the CPU test's bound); in float32 each term w_k t_k carries at most four half-ulp
    # roundings (1 - fx, 1 - fy, their product, the product with t): 2 * 2^-24 of max|t| over the four terms, whose weights sum
    # to 1; the three additions at most 1.5 * 2^-24 more: together under 8 * 2^-24
    assert err <= (4 + 4) * 2.0 ** -24 * float(tex.abs().max())


# ---- the module in the latent-strand stage ----------------------------------------------------------------------------------------
LAMBDA_DIFF = 0.5


def _sphere_scalp():
    """tc.scalp_grid()'s chart wrapped on most of a sphere of radius 0.9 around the head of tests.test_api_cpu._hair_scene"""
    import math
    _, faces, uv = tc.scalp_grid(9, 7)
    lon, lat = uv[:, 0] * math.pi, uv[:, 1] * math.pi / 2
    verts = 0.9 * torch.stack([torch.cos(lat) * torch.sin(lon), torch.sin(lat), torch.cos(lat) * torch.cos(lon)], -1)
    return verts, faces, uv


def _tiny(device, fused, dtype=torch.float32):
    target = torch.rand(1, 6, 16, 16, generator=torch.Generator().manual_seed(4)).to(device=device, dtype=dtype)
    gen = sg.TexturedStrands(_sphere_scalp(), tc.Linear3(6, 7), tc.LinearColour(4), lambda t: ((t - target) ** 2).mean(), num_strands=64,
                             max_num_strands=200, texture_size=16, geometry_channels=6, appearance_channels=5, scale_decoder=2.0,
                             generator=torch.Generator().manual_seed(3), fused=fused)
    with torch.no_grad():
        gen.texture.copy_(torch.rand(gen.texture.shape, generator=torch.Generator().manual_seed(5)) * 2 - 1)
    gen = gen.to(device)
    return gen.to(dtype) if dtype != torch.float32 else gen


GENERIC = SimpleNamespace(debug=False, fused_projection=False)
MAPS = ("original_image", "original_mask", "original_orient_angle", "original_orient_conf")


def _head_and_camera(dev):
    from gaussianhaircut_amd.scene.cameras import make_camera
    from gaussianhaircut_amd.utils import synthetic as syn
    spec = syn.CONFIGS["tiny"]
    head = syn.make_model(spec, dev)
    with torch.no_grad():
        head._label[: spec.P // 2] = -4.0
        head._label[spec.P // 2:] = 4.0
    head.precompute_head()
    return head, make_camera(48, 32, fovy_deg=40.0, distance=4.0, device=dev), syn.background(dev)


def _scene(fused):
    from gaussianhaircut_amd.gaussian_renderer import render_hair
    from gaussianhaircut_amd.scene.gaussian_model_latent_strands import GaussianModelLatentStrands
    dev = torch.device(DEV)
    head, cam, bg = _head_and_camera(dev)
    hair = GaussianModelLatentStrands(3, _tiny(dev, fused), None, fused=fused)
    with torch.no_grad():                                                # ground truth: another texture, recoloured
        gt = GaussianModelLatentStrands(3, _tiny(dev, fused), None, fused=fused)
        gt.strands_generator.texture.mul_(0.5)
        gt.strands_generator.color_decoder.lin.bias.add_(0.3)
        gt.strands_generator.generator.manual_seed(3)
        gt.initialize_gaussians_hair(0)
        pkg = render_hair(cam, head, gt, FUSED, bg)
        cam.original_image, cam.original_mask = pkg["render"].clamp(0, 1).detach(), pkg["mask"].clamp(0, 1).detach()
        cam.original_orient_angle = pkg["orient_angle"].detach()
        cam.original_orient_conf = torch.ones_like(pkg["orient_conf"]).detach()
    return head, hair, cam, bg


def _opt():
    return SimpleNamespace(lambda_dl1=1.0, lambda_dmask=0.1, lambda_dorient=0.1, lambda_dsds=LAMBDA_DIFF, use_gt_orient_conf=True,
                           train_orient_conf=True, iterations=100, latent_lr=1e-3)


def _recorded_step(fused):
    """one latent_strand_training_step; records the draw, the generator's outputs, the cotangents that reach them, the loss and
    texture.grad as the optimizer saw it"""
    from gaussianhaircut_amd.trainer import latent_strand_training_step
    head, hair, cam, bg = _scene(fused)
    gen, rec = hair.strands_generator, {}
    fwd = gen.forward

    def forward(iteration=0):
        out = fwd(iteration)
        rec["idx"] = gen.last_idx.cpu().clone()
        for k in ("points", "features", "orient_conf"):
            rec[k] = out[k].detach().cpu().clone()
            out[k].register_hook(lambda g, k=k: rec.__setitem__("d_" + k, g.detach().cpu().clone()))
        return out
    gen.forward = forward
    hair.training_setup(_opt())
    step0 = hair.optimizer.step
    hair.optimizer.step = lambda *a, **k: (rec.__setitem__("texture_grad", gen.texture.grad.detach().cpu().clone()), step0(*a, **k))[1]
    rec["loss"] = float(latent_strand_training_step(head, hair, [cam], bg, _opt(), 1, pipe=FUSED))
    rec.update({k: getattr(cam, k).detach().cpu().clone() for k in MAPS})
    hair.optimizer.step = step0
    del gen.forward
    more = [float(latent_strand_training_step(head, hair, [cam], bg, _opt(), i, pipe=FUSED)) for i in (2, 3)]
    assert all(x == x and abs(x) < float("inf") for x in more), more
    return rec


def _float64_of(rec):
    """the generator's part of the step in float64 on the run's own draw and the cotangents that reached its outputs"""
    gen = _tiny("cpu", False, torch.float64)
    idx = rec["idx"]
    z = sg.sample_texture(gen.texture, gen.taps, idx, fused=False)
    v = gen.strand_decoder(z[:, :6])
    p = sg.strands_to_world(v, gen.local2world, gen.origins, idx, gen.scale_decoder, fused=False)
    feats, conf = gen.appearance(z[:, 6:])
    l_diff = gen.prior_loss(gen.texture[:, :6])
    total = (p * rec["d_points"].double()).sum() + (feats * rec["d_features"].double()).sum() + LAMBDA_DIFF * l_diff
    if "d_orient_conf" in rec:
        total = total + (conf * rec["d_orient_conf"].double()).sum()
    (g,) = torch.autograd.grad(total, gen.texture)
    return dict(points=p.detach(), features=feats.detach(), orient_conf=conf.detach(), texture_grad=g)


def _float64_loss(rec):
    """The step's loss in float64 on the run's own draw and ground-truth maps: the generator, the build of the segment Gaussians,
    the projection and the loss in float64 from the same raw parameters, composited in double (oracle/ghr_oracle64.c) over the
    lists of a float32 run of the same scene through the CPU oracle -- the arbiter of tests/test_gpu_fused_fullsize.py."""
    from gaussianhaircut_amd.gaussian_renderer import render_hair
    from gaussianhaircut_amd.scene.gaussian_model_latent_strands import GaussianModelLatentStrands
    from gaussianhaircut_amd.trainer import latent_view_loss
    from tests import oracle_backend as ob
    head, cam, bg = _head_and_camera("cpu")
    for k in MAPS:
        setattr(cam, k, rec[k])
    idx = rec["idx"]

    def hair_of(dtype):
        gen = _tiny("cpu", False, dtype)
        gen.draw = lambda num=None: idx.clone()
        hair = GaussianModelLatentStrands(3, gen, None, fused=False)
        hair.initialize_gaussians_hair(1)
        return hair
    with torch.no_grad():
        hair32 = hair_of(torch.float32)
        with ob.oracle_rasterizer():
            render_hair(cam, head, hair32, GENERIC, bg)
        st32 = ob.LAST["state"]
        keep_head, keep_hair = head.filter_points(cam), hair32.filter_points(cam)
        head64, cam64 = ob.double_chain(head, cam, keep_head)
        head64.precompute_head()
        hair64 = hair_of(torch.float64)
        hair64.filter_points = lambda _cam: keep_hair
        with ob.oracle_rasterizer64(st32):
            pkg = render_hair(cam64, head64, hair64, GENERIC, bg.double())
        n_flip = int((ob.LAST["n_contrib64"] != st32.n_contrib).sum())
        loss = latent_view_loss(pkg, cam64, _opt(), l_diff=hair64.LDiff, fused=False)
    assert loss.dtype == torch.float64 and torch.equal(hair64.strands_generator.last_idx, idx)
    return float(loss), n_flip


def test_one_iteration_of_the_latent_strand_stage_with_the_generator():
    """latent_strand_training_step with linear stand-in decoders at Smax 200, S 64, L 8, T 16 on a 32 x 48 view.  points, the
    colour decoder's outputs and texture.grad of the HIP run and of the composed run are each held against the float64 generator
    on that run's own draw and cotangents, under the bar with the composed run's distance; two further iterations run to a
    finite loss.  The step's loss of both runs is held under the same bar against the whole iteration in float64
    (_float64_loss): |loss - f64| <= 1e-5 |f64| + 3 |composed - f64|."""
    L = _lib.lib()
    L.ghr_set_deterministic(1)
    try:
        comp, fused = _recorded_step(False), _recorded_step(True)
    finally:
        L.ghr_set_deterministic(0)
    assert torch.equal(comp["idx"], fused["idx"])
    c64, f64 = _float64_of(comp), _float64_of(fused)
    for k in ("points", "features", "orient_conf", "texture_grad"):
        ref = (comp[k].double() - c64[k]).abs()
        for name, got, want in (("composed", comp, c64), ("fused", fused, f64)):
            err = (got[k].double() - want[k]).abs()
            bar = 1e-5 * want[k].abs().max() + 3 * ref
            print("%s %s: max err %.3e, max|f64| %.3e, composed err %.3e" % (name, k, float(err.max()), float(want[k].abs().max()), float(ref.max())))
            assert bool(torch.isfinite(got[k]).all()) and bool((err <= bar).all()), (name, k, float((err - bar).max()))
    assert float(f64["texture_grad"][:, :6].abs().max()) > 0 and float(f64["texture_grad"][:, 6:].abs().max()) > 0
    (lc64, flips_c), (lf64, flips_f) = _float64_loss(comp), _float64_loss(fused)
    err_c, err_f = abs(comp["loss"] - lc64), abs(fused["loss"] - lf64)
    print("loss: composed %.9g (f64 %.12g, the double walk stops elsewhere on %d pixels), fused %.9g (f64 %.12g, %d pixels)" % (
        comp["loss"], lc64, flips_c, fused["loss"], lf64, flips_f))
    assert err_f <= 1e-5 * abs(lf64) + 3 * err_c and err_c <= 1e-5 * abs(lc64) + 3 * err_c, (err_c, err_f)
