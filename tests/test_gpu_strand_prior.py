"""The strand stage's prior term on the GPU (csrc/ghr_sds.h through gaussianhaircut_amd/strand_prior.py).

Both forms -- the HIP one and the PyTorch-composed float32 one on the device -- are held against the float64 restatement of
tests/sds_cases.py under the project's arbiter criterion (tests/test_gpu_camera_bank.py):
    |got - f64| <= 1e-5 max|f64| + 3 |composed float32 on the device - f64|      elementwise.
Neighbour indices and inverted lists are compared bit for bit against the restatement's stable sort.  Shapes: the smallest at
which a mapping decision changes (tests/sds_cases.py SMALL), one strand drawn for every guiding strand (all distances tie),
planted duplicates, and the golden's full size once."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd import strand_prior as sp
from tests import sds_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FUSED = SimpleNamespace(debug=False, fused_projection=True)


def _run(c, fused, z_detached=False, v_detached=False):
    """steps 1 - 4 and the backward on the device; the pieces are called one by one so that each can be looked at"""
    dirs = c["dirs"].to(DEV).requires_grad_(True)
    idx = c["idx"].to(DEV)
    w2l = torch.linalg.inv(c["local2world"].double()).float().to(DEV)
    e, v = sp.guiding_strands_local(dirs, w2l, idx, c["scale"], fused=fused, frames_are_inverse=True)
    z = sc.make_encoder(c["W"].to(DEV))(e)[:, :c["C"]]
    zt, vt = (z.detach() if z_detached else z), (v.detach() if v_detached else v)
    uvg = c["uvs"].to(DEV)[idx]
    if fused:
        tex, state = sp.latent_texture(uvg, zt, vt, c["G"], fused=True, return_state=True)
    else:
        tex, state = sp.latent_texture(uvg, zt, vt, c["G"], fused=False), None
    loss = ((tex - c["T0"].to(DEV)) ** 2).mean()
    (d_dirs,) = torch.autograd.grad(loss, dirs)
    return dict(e=e.detach(), v=v.detach(), texture=tex.detach(), d_dirs=d_dirs, state=state, loss=loss.detach())


def _check_case(c, exact_ties=True):
    r64 = c["r64"]
    if c["S"] > 1:
        gap, knee, _ = sc.input_conditions(r64, c["N"], exact_ties=exact_ties)
        assert gap >= 1e-5 and knee >= 1e-4, (gap, knee)
    comp, fused = _run(c, False), _run(c, True)
    st = fused["state"]
    assert st["nbr"].dtype == torch.int32 and torch.equal(st["nbr"].long().cpu(), r64["nbr"])
    assert torch.equal(st["start"].long().cpu(), r64["start"]) and torch.equal(st["list"].long().cpu(), r64["entries"])
    nbr_c, _ = sp.neighbours_composed(c["uvs"].to(DEV)[c["idx"].to(DEV)], c["G"])
    assert torch.equal(nbr_c.cpu(), r64["nbr"])
    for k in ("e", "v", "texture", "d_dirs"):
        sc.assert_within("composed " + k, comp[k], r64[k], comp[k])
        sc.assert_within("fused " + k, fused[k], r64[k], comp[k])
    for k in ("w", "csim", "alpha", "alpha_q"):
        sc.assert_within("fused " + k, st[k].reshape(r64[k].shape), r64[k], c["r32"][k])
    again = _run(c, True)                                               # gather-form: a second pass gives the same bits
    for k in ("e", "v", "texture", "d_dirs"):
        assert torch.equal(again[k], fused[k]), k
    return comp, fused


@pytest.mark.parametrize("name", sorted(sc.SMALL))
def test_both_forms_against_float64_on_the_small_shapes(name):
    c = sc.case(name)
    comp, fused = _check_case(c)
    if name == "one-strand":
        assert torch.equal(fused["state"]["nbr"].cpu(), torch.arange(4, dtype=torch.int32).expand(9, 4))
    if name == "duplicates":                                             # strand 3 was drawn four times: its row is the sum of four
        assert float(fused["d_dirs"][3].abs().max()) > 0 and float(fused["d_dirs"][4].abs().max()) == 0.0


def test_both_forms_at_the_golden_size():
    c = sc.golden_case()
    comp, fused = _check_case(c, exact_ties=False)
    want, idx = c["want"], c["idx"]
    r64 = c["r64"]
    for name, got in (("composed", comp), ("fused", fused)):             # and against the reference's own float32 run
        sc.assert_within(name + " texture against the golden", got["texture"], r64["texture"], want["texture"])
        sc.assert_within(name + " d_dirs against the golden", got["d_dirs"], r64["d_dirs"], want["d_dirs"])
    mask = torch.ones(c["S"], dtype=torch.bool)
    mask[idx] = False
    assert float(fused["d_dirs"].cpu()[mask].abs().max()) == 0.0


@pytest.mark.parametrize("name", ["G3-N9", "G8-N64", "n65", "C65", "duplicates"])
def test_each_cotangent_alone(name):
    c = sc.case(name)
    for kw in (dict(z_detached=True), dict(v_detached=True)):           # d_texture through alpha only / with alpha frozen
        r64 = sc.restate_case(c, **kw)
        comp, fused = _run(c, False, **kw), _run(c, True, **kw)
        assert float(r64["d_dirs"].abs().max()) > 0
        sc.assert_within("composed d_dirs %s" % kw, comp["d_dirs"], r64["d_dirs"], comp["d_dirs"])
        sc.assert_within("fused d_dirs %s" % kw, fused["d_dirs"], r64["d_dirs"], comp["d_dirs"])
    # the local frame: d_e alone, d_v alone
    g = torch.Generator().manual_seed(3)
    ce, cv = torch.randn(c["N"], c["n"] + 1, 3, generator=g), torch.randn(c["N"], c["n"], 3, generator=g)
    w2l = torch.linalg.inv(c["local2world"].double())
    for which in ("e", "v"):
        d64 = c["dirs"].double().requires_grad_(True)
        d = d64[c["idx"]]
        P = torch.cat([torch.zeros(c["N"], 1, 3, dtype=torch.float64), torch.cumsum(d, 1)], 1)
        out64 = torch.einsum("gab,gjb->gja", w2l[c["idx"]], P if which == "e" else d) * c["scale"]
        (want,) = torch.autograd.grad((out64 * (ce if which == "e" else cv).double()).sum(), d64)
        got = {}
        for fused in (False, True):
            dirs = c["dirs"].to(DEV).requires_grad_(True)
            e, v = sp.guiding_strands_local(dirs, w2l.float().to(DEV), c["idx"].to(DEV), c["scale"], fused=fused, frames_are_inverse=True)
            (got[fused],) = torch.autograd.grad(((e if which == "e" else v) * (ce if which == "e" else cv).to(DEV)).sum(), dirs)
        sc.assert_within("composed d_dirs from d_%s" % which, got[False], want, got[False])
        sc.assert_within("fused d_dirs from d_%s" % which, got[True], want, got[False])


def test_frames_inverted_in_the_kernel():
    c = sc.case("duplicates")
    d64 = c["dirs"].double().requires_grad_(True)
    e64, v64 = sp._local_composed(d64, c["local2world"].double(), c["idx"], c["scale"], False)
    (g64,) = torch.autograd.grad(e64.sum() + (v64 * v64).sum(), d64)
    got = {}
    for fused in (False, True):
        dirs = c["dirs"].to(DEV).requires_grad_(True)
        e, v = sp.guiding_strands_local(dirs, c["local2world"].to(DEV), c["idx"].to(DEV), c["scale"], fused=fused)
        (g,) = torch.autograd.grad(e.sum() + (v * v).sum(), dirs)
        got[fused] = (e.detach(), v.detach(), g)
    for k, (name, want) in enumerate((("e", c["r64"]["e"]), ("v", c["r64"]["v"]), ("d_dirs", g64))):
        sc.assert_within("composed " + name, got[False][k], want, got[False][k])
        sc.assert_within("fused " + name, got[True][k], want, got[False][k])


GUARD = 64


def _guarded(numel, dtype):
    fill = float("nan") if dtype == torch.float32 else -7
    buf = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, ctypes.c_void_p(buf.data_ptr() + GUARD * buf.element_size())


def _guards_intact_and_filled(name, buf, numel):
    head, body, tail = buf[:GUARD], buf[GUARD:GUARD + numel], buf[GUARD + numel:]
    if buf.dtype == torch.float32:
        assert bool(torch.isnan(head).all()) and bool(torch.isnan(tail).all()), name
        assert not bool(torch.isnan(body).any()), name
    else:
        assert bool((head == -7).all()) and bool((tail == -7).all()) and not bool((body == -7).any()), name
    return body


@pytest.mark.parametrize("name", ["G2-N4", "G8-N63", "G9-N65", "n65", "C65", "duplicates"])
def test_outputs_land_in_nan_filled_buffers_between_guards(name):
    c = sc.case(name)
    S, N, n, C, G = c["S"], c["N"], c["n"], c["C"], c["G"]
    GG = G * G
    L = _lib.lib()
    f32, i32 = torch.float32, torch.int32
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dirs, idx = c["dirs"].to(DEV).contiguous(), c["idx"].to(DEV)
    w2l = torch.linalg.inv(c["local2world"].double()).float().to(DEV).contiguous()
    e, pe = _guarded(N * (n + 1) * 3, f32)
    v, pv = _guarded(N * n * 3, f32)
    _lib.check(L.ghr_sds_local(stream, S, N, n, p(dirs), p(w2l), 1, p(idx), c["scale"], pe, pv))
    eb = _guards_intact_and_filled("e", e, N * (n + 1) * 3).view(N, n + 1, 3)
    vb = _guards_intact_and_filled("v", v, N * n * 3).view(N, n, 3).contiguous()
    z = sc.make_encoder(c["W"].to(DEV))(eb)[:, :C].contiguous()
    uvg = c["uvs"].to(DEV)[idx].contiguous()
    centres = sp.texel_centres(G, DEV).contiguous()
    sizes = dict(nbr=(4 * GG, i32), w=(4 * GG, f32), csim=(N, f32), alpha=(N, f32), alpha_q=(GG, f32), count=(N, i32), start=(N + 1, i32),
                 list=(4 * GG, i32), texture=(C * GG, f32))
    b = {k: _guarded(*s) for k, s in sizes.items()}
    _lib.check(L.ghr_sds_texture(stream, N, n, C, G, p(uvg), p(centres), p(z), p(vb), *[b[k][1] for k in sizes]))
    body = {k: _guards_intact_and_filled(k, b[k][0], sizes[k][0]) for k in sizes}
    r64 = c["r64"]
    assert torch.equal(body["nbr"].view(GG, 4).long().cpu(), r64["nbr"]) and torch.equal(body["list"].long().cpu(), r64["entries"])
    sc.assert_within("texture", body["texture"].view(1, C, G, G), r64["texture"], c["r32"]["texture"])
    d_tex = (2 * (body["texture"].view(1, C, G, G) - c["T0"].to(DEV)) / (C * GG)).contiguous()
    bw = {k: _guarded(*s) for k, s in dict(dalpha_q=(GG, f32), d_csim=(N, f32), d_z=(N * C, f32), d_v=(N * n * 3, f32)).items()}
    saved = [ctypes.c_void_p(body[k].data_ptr()) for k in ("nbr", "w", "csim", "alpha_q", "start", "list")]
    _lib.check(L.ghr_sds_texture_backward(stream, N, n, C, G, p(z), p(vb), *saved, p(d_tex), *[bw[k][1] for k in bw]))
    for k, numel in (("dalpha_q", GG), ("d_csim", N), ("d_z", N * C), ("d_v", N * n * 3)):
        _guards_intact_and_filled(k, bw[k][0], numel)
    sidx, order = torch.sort(idx, stable=True)
    dd = torch.zeros(S * n * 3 + 2 * GUARD, dtype=f32, device=DEV)
    d_v = bw["d_v"][0][GUARD:GUARD + N * n * 3].contiguous()
    _lib.check(L.ghr_sds_local_backward(stream, S, N, n, p(w2l), 1, p(sidx), p(order), c["scale"], None, p(d_v),
                                        ctypes.c_void_p(dd.data_ptr() + 4 * GUARD)))
    assert float(dd[:GUARD].abs().max()) == 0.0 and float(dd[-GUARD:].abs().max()) == 0.0
    rows = dd[GUARD:-GUARD].view(S, n, 3)
    drawn = torch.zeros(S, dtype=torch.bool, device=DEV)
    drawn[idx] = True
    assert bool(torch.isfinite(rows).all()) and float(rows[~drawn].abs().max() if bool((~drawn).any()) else 0.0) == 0.0


def test_an_index_outside_the_model_reads_nothing():
    c = sc.case("G3-N5")
    idx = c["idx"].clone()
    idx[2] = c["S"] + 100
    e, v = sp.guiding_strands_local(c["dirs"].to(DEV), c["local2world"].to(DEV), idx.to(DEV), c["scale"])
    assert bool(torch.isnan(e[2]).all()) and bool(torch.isnan(v[2]).all()) and bool(torch.isfinite(e[[0, 1, 3, 4]]).all())


# ---- the trainer --------------------------------------------------------------------------------------------------------------------
def _scene(opt_fused=True):
    from gaussianhaircut_amd.gaussian_renderer import render_hair
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    from gaussianhaircut_amd.utils import synthetic as syn
    from tests.test_api_cpu import _hair_scene
    dev = torch.device(DEV)
    opt = OptimizationParams()
    opt.lambda_dorient, opt.lambda_dmask, opt.lambda_dsds = 0.1, 0.1, 0.01
    bg = syn.background(dev)
    spec, head, hair, cam = _hair_scene(dev)
    _, _, gt_hair, _ = _hair_scene(dev)
    with torch.no_grad():
        gt_hair._features_dc.add_(0.4)
        gt_hair._dirs.mul_(1.1)
        gt_hair.initialize_gaussians_hair()
        pkg = render_hair(cam, head, gt_hair, FUSED, bg)
        cam.original_image, cam.original_mask = pkg["render"].clamp(0, 1).detach(), pkg["mask"].clamp(0, 1).detach()
        cam.original_orient_angle = pkg["orient_angle"].detach()
        cam.original_orient_conf = torch.ones_like(pkg["orient_conf"]).detach()
    hair.training_setup(opt, fused=opt_fused)
    return opt, bg, head, hair, cam


def _params(hair):
    return [p.detach().clone() for p in (hair._dirs, hair._features_dc, hair._features_rest, hair._orient_conf)]


def test_training_step_with_a_prior_is_reproducible_on_every_path():
    """Three iterations of strand_training_step with a prior attached give the same parameters bit for bit whether the SH update
    rides in the backward (FUSE_STRAND_ADAM) or not, whether the prior draws its guiding strands itself or is handed the same
    ones, and when the run is repeated; the prior moves the strands; a NaN out of the prior's loss skips the step on both paths."""
    from gaussianhaircut_amd import trainer
    from gaussianhaircut_amd.trainer import strand_training_step
    lib = _lib.lib()
    lib.ghr_set_deterministic(1)
    saved = trainer.FUSE_STRAND_ADAM
    try:
        res, drawn = {}, []
        for mode in ("fuse-adam", "fuse-adam again", "classic", "classic, idx handed in", "no prior"):
            trainer.FUSE_STRAND_ADAM = mode.startswith("fuse-adam")
            opt, bg, head, hair, cam = _scene()
            S, n = hair._dirs.shape[0], hair._dirs.shape[1]
            if mode != "no prior":
                prior = sc.tiny_prior(S, n, device=DEV)
                if mode == "classic, idx handed in":
                    draws = iter(drawn)
                    prior.draw = lambda S_, dev_: next(draws).clone()
                hair.attach_prior(prior)
            trace = []
            for i in range(3):
                loss = strand_training_step(head, hair, [cam], bg, opt, i + 1, pipe=FUSED)
                trace.append(_params(hair))
                if mode == "fuse-adam":
                    drawn.append(hair.prior.last_idx.clone())
                    assert bool(torch.isfinite(loss)) and float(hair.Lsds.detach()) > 0
            o = hair.optimizer
            assert o.fused_steps == (3 if trainer.FUSE_STRAND_ADAM else 0), (mode, o.fused_steps)
            if mode in ("fuse-adam", "classic"):
                # a NaN out of the prior's loss: it reaches _dirs.grad through autograd and the step is skipped
                real = hair.prior.prior_loss
                hair.prior.prior_loss = lambda t: real(t) * float("nan")
                strand_training_step(head, hair, [cam], bg, opt, 4, pipe=FUSED)
                hair.prior.prior_loss = real
                torch.cuda.synchronize()
                for x, y in zip(trace[-1], _params(hair)):
                    assert torch.equal(x, y), mode
                assert int(o.state_dev[0]) == 3 and int(o.state_dev[1]) == 0 and float(o.flat_grad.abs().max()) == 0.0, mode
                strand_training_step(head, hair, [cam], bg, opt, 5, pipe=FUSED)   # and the next one goes through again
                assert int(o.state_dev[0]) == 4 and not torch.equal(trace[-1][0], _params(hair)[0]), mode
            res[mode] = trace
        for mode in ("fuse-adam again", "classic", "classic, idx handed in"):
            for it, (ta, tb) in enumerate(zip(res["fuse-adam"], res[mode])):
                for x, y in zip(ta, tb):
                    assert torch.equal(x, y), (mode, it, float((x - y).abs().max()))
        assert not torch.equal(res["fuse-adam"][0][0], res["no prior"][0][0])   # the term reaches the strand directions
        assert torch.equal(res["fuse-adam"][0][1], res["no prior"][0][1])       # and, in the first step, nothing else
    finally:
        trainer.FUSE_STRAND_ADAM = saved
        lib.ghr_set_deterministic(0)


def test_training_steps_through_the_composed_prior_on_the_device():
    """Three iterations of strand_training_step with the composed prior (fused=False) and with the HIP one, from the same start
    and the same draws: in every iteration each run's Lsds is held against the float64 restatement on that run's own strand
    directions under the arbiter's bar, |Lsds - f64| <= 1e-5 |f64| + 3 |composed - f64|; the composed run takes the same path
    through the trainer (late-group NaN mark, SH update in the backward) and moves the strands."""
    from gaussianhaircut_amd.trainer import strand_training_step
    runs = {}
    for fused in (False, True):
        opt, bg, head, hair, cam = _scene()
        prior = sc.tiny_prior(hair._dirs.shape[0], hair._dirs.shape[1], device=DEV, fused=fused)
        hair.attach_prior(prior)
        ti, rows = prior.test_inputs, []
        for i in range(3):
            dirs0 = hair._dirs.detach().cpu().clone()
            loss = strand_training_step(head, hair, [cam], bg, opt, i + 1, pipe=FUSED)
            idx = prior.last_idx.cpu()
            f64 = sc.restate(dirs0, ti["local2world"], ti["uvs"], idx, ti["scale"], ti["G"], ti["C"], ti["W"], ti["T0"])
            rows.append((idx, float(hair.Lsds.detach()), float(f64["loss"]), f64["texture"], prior.last_texture.cpu()))
            assert bool(torch.isfinite(loss)) and not torch.equal(dirs0, hair._dirs.detach().cpu())
        assert hair.optimizer.fused_steps == 3 and int(hair.optimizer.state_dev[1]) == 0
        runs[fused] = rows
    for it, (c, f) in enumerate(zip(runs[False], runs[True])):
        assert torch.equal(c[0], f[0]), it                              # the same guiding strands were drawn
        err_c, err_f = abs(c[1] - c[2]), abs(f[1] - f[2])
        print("iteration %d: Lsds composed %.9g (f64 %.9g), HIP %.9g (f64 %.9g)" % (it, c[1], c[2], f[1], f[2]))
        assert err_f <= 1e-5 * abs(f[2]) + 3 * err_c and err_c <= 1e-5 * abs(c[2]) + 3 * err_c, (it, err_c, err_f)
        sc.assert_within("iteration %d composed texture" % it, c[4], c[3], c[4])
        bar = 1e-5 * f[3].abs().max() + 3 * (c[4].double() - c[3]).abs()
        assert bool(((f[4].double() - f[3]).abs() <= bar).all()), it
