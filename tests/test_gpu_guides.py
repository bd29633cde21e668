"""Guiding strands of the textured generator on the GPU (csrc/ghr_guides.h through gaussianhaircut_amd/strand_generator.py;
DESIGN.md 8q).

Both forms -- the HIP one and the PyTorch-composed float32 one on the device -- are held against the float64 arbiter of
tests/guides_cases.py under DESIGN.md 8i's bar,
    |got - f64| <= 1e-5 max|f64| + 3 |composed float32 on the device - f64|      elementwise;
``nbr``, ``start`` and ``list`` are compared bit for bit, and a second pass gives the same bits.  Shapes (tests/guides_cases.py
SMALL): N around the wave's 64 lanes, the rows beside the guides around a workgroup's four waves, n and C around 64, two guides
at one UV, a root at equal distances, S = N + 1, one mid case."""
import ctypes

import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd import strand_generator as sg
from tests import guides_cases as gc
from tests import texstrands_cases as tc
from tests.sds_cases import assert_within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
FLOATS = ("w", "csim", "alpha", "alpha_s")
OUT = ("z", "d_zg", "d_vg")


def _run(c, fused, z_detached=False, v_detached=False):
    z_g = c["z_g"].to(DEV).requires_grad_(not z_detached)
    v_g = c["v_g"].to(DEV).requires_grad_(not v_detached)
    z, st = sg.blend_from_guides(c["uvs"].to(DEV), z_g, v_g, fused=fused, return_state=True)
    (z * c["d_z"].to(DEV)).sum().backward()
    zero = torch.zeros_like
    return dict(z=z.detach(), d_zg=zero(z_g) if z_g.grad is None else z_g.grad, d_vg=zero(v_g) if v_g.grad is None else v_g.grad, **st)


def _state_equals(got, r64):
    assert got["nbr"].dtype == torch.int32 and torch.equal(got["nbr"].long().cpu(), r64["nbr"])
    assert torch.equal(got["start"].long().cpu(), r64["start"]) and torch.equal(got["list"].long().cpu(), r64["entries"])


@pytest.mark.parametrize("name", sorted(gc.SMALL))
def test_both_forms_against_float64(name):
    c = gc.case(name)
    r64 = c["r64"]
    comp, fused = _run(c, False), _run(c, True)
    _state_equals(comp, r64)
    _state_equals(fused, r64)
    for k in OUT + FLOATS:
        assert_within("composed " + k, comp[k], r64[k], comp[k])
        assert_within("fused " + k, fused[k], r64[k], comp[k])
    assert torch.equal(fused["z"][:c["N"]].cpu(), c["z_g"])                # a guide's row is its fetched row
    again = _run(c, True)                                                  # two passes give the same bits
    for k in OUT + FLOATS + ("nbr", "start", "list"):
        assert torch.equal(again[k], fused[k]), k


@pytest.mark.parametrize("name", ["N5", "N65", "rows65", "n65", "C129", "same-uv"])
@pytest.mark.parametrize("which", ["z", "v"])
def test_each_cotangent_alone(name, which):
    c = gc.case(name)
    r64, _ = gc.detached(name, which)
    kw = dict(z_detached=which == "z", v_detached=which == "v")
    comp, fused = _run(c, False, **kw), _run(c, True, **kw)
    live = "d_vg" if which == "z" else "d_zg"
    assert float(r64[live].abs().max()) > 0
    assert_within("composed " + live, comp[live], r64[live], comp[live])
    assert_within("fused " + live, fused[live], r64[live], comp[live])
    assert_within("fused z", fused["z"], r64["z"], comp["z"])


def _guarded(numel, dtype):
    fill = float("nan") if dtype == torch.float32 else -7
    buf = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, ctypes.c_void_p(buf.data_ptr() + GUARD * buf.element_size())


def _body(name, buf, numel):
    head, body, tail = buf[:GUARD], buf[GUARD:GUARD + numel], buf[GUARD + numel:]
    if buf.dtype == torch.float32:
        assert bool(torch.isnan(head).all()) and bool(torch.isnan(tail).all()), name
        assert not bool(torch.isnan(body).any()), name                    # every element was ASSIGNED
    else:
        assert bool((head == -7).all()) and bool((tail == -7).all()) and not bool((body == -7).any()), name
    return body


@pytest.mark.parametrize("name", sorted(gc.SMALL))
def test_outputs_land_in_nan_filled_buffers_between_guards(name):
    c = gc.case(name)
    S, N, n, C = c["S"], c["N"], c["n"], c["C"]
    L = _lib.lib()
    f32, i32 = torch.float32, torch.int32
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    uvs, z_g, v_g, d_z = [c[k].to(DEV).contiguous() for k in ("uvs", "z_g", "v_g", "d_z")]   # (named: they must outlive the calls)
    sizes = dict(nbr=(4 * S, i32), w=(4 * S, f32), csim=(N, f32), alpha=(N, f32), alpha_s=(S, f32), count=(N, i32), start=(N + 1, i32),
                 unsorted=(4 * S, i32), list=(4 * S, i32), z=(S * C, f32), dalpha_s=(S, f32), d_csim=(N, f32), d_zg=(N * C, f32),
                 d_vg=(N * n * 3, f32))
    b = {k: _guarded(*s) for k, s in sizes.items()}
    _lib.check(L.ghr_guides_blend(stream, S, N, n, C, p(uvs), p(z_g), p(v_g), *[b[k][1] for k in ("nbr", "w", "csim", "alpha", "alpha_s", "count",
                                                                                                   "start", "unsorted", "list", "z")]))
    _lib.check(L.ghr_guides_blend_backward(stream, S, N, n, C, p(z_g), p(v_g), *[b[k][1] for k in ("nbr", "w", "csim", "alpha_s", "start", "list")],
                                           p(d_z), *[b[k][1] for k in ("dalpha_s", "d_csim", "d_zg", "d_vg")]))
    body = {k: _body(k, b[k][0], sizes[k][0]) for k in sizes}
    r64 = c["r64"]
    assert torch.equal(body["nbr"].view(S, 4).long().cpu(), r64["nbr"])
    assert torch.equal(body["start"].long().cpu(), r64["start"]) and torch.equal(body["list"].long().cpu(), r64["entries"])
    assert int(body["count"].abs().max()) == 0                              # counted up, then down again
    assert torch.equal(torch.sort(body["unsorted"])[0].cpu(), torch.arange(4 * S, dtype=i32))
    comp = _run(c, False)
    for k in OUT:
        assert_within(k, body[k].view(r64[k].shape), r64[k], comp[k])
    dz, dzp = _guarded(N * C, f32)                                          # d_vg = NULL: d_zg alone, the same bits
    _lib.check(L.ghr_guides_blend_backward(stream, S, N, n, C, p(z_g), p(v_g), *[b[k][1] for k in ("nbr", "w", "csim", "alpha_s", "start", "list")],
                                           p(d_z), b["dalpha_s"][1], b["d_csim"][1], dzp, None))
    assert torch.equal(_body("d_zg alone", dz, N * C), body["d_zg"])


def test_buffers_on_another_device_or_of_another_type_are_refused_in_python():
    c = gc.case("N5")
    uvs, z_g, v_g = c["uvs"].to(DEV), c["z_g"].to(DEV), c["v_g"].to(DEV)
    with pytest.raises(ValueError, match="uvs must be"):
        sg.blend_from_guides(uvs.cpu(), z_g, v_g, fused=True)
    with pytest.raises(ValueError, match="v_g must be"):
        sg.blend_from_guides(uvs, z_g, v_g.cpu(), fused=True)
    with pytest.raises(RuntimeError, match="float32"):
        sg.blend_from_guides(uvs, z_g.double(), v_g.double(), fused=True)


# ---- the module in the latent-strand stage ----------------------------------------------------------------------------------------
S_STEP, N_STEP, T_STEP, SMAX_STEP = 40, 9, 8, 120


def _tiny(device, fused, dtype=torch.float32):
    """tests/test_gpu_textured_strands.py's generator at S 40, T 8 with 9 guiding strands"""
    from tests import test_gpu_textured_strands as tgs
    target = torch.rand(1, 6, T_STEP, T_STEP, generator=torch.Generator().manual_seed(4)).to(device=device, dtype=dtype)
    gen = sg.TexturedStrands(tgs._sphere_scalp(), tc.Linear3(6, 7), tc.LinearColour(4), lambda t: ((t - target) ** 2).mean(),
                             num_strands=S_STEP, max_num_strands=SMAX_STEP, texture_size=T_STEP, geometry_channels=6, appearance_channels=5,
                             scale_decoder=2.0, generator=torch.Generator().manual_seed(3), fused=fused, num_guiding_strands=N_STEP)
    with torch.no_grad():
        gen.texture.copy_(torch.rand(gen.texture.shape, generator=torch.Generator().manual_seed(5)) * 2 - 1)
    gen = gen.to(device)
    return gen.to(dtype) if dtype != torch.float32 else gen


def _float64_of(rec):
    """the generator's part of the step in float64 on the run's own draw and the cotangents that reached its outputs, with the
    restatement of tests/guides_cases.py between the fetch and the second decoder call"""
    from tests import test_gpu_textured_strands as tgs
    gen = _tiny("cpu", False, torch.float64)
    idx, N = rec["idx"], N_STEP
    z_g = sg.sample_texture(gen.texture, gen.taps, idx[:N], fused=False)
    v_g = gen.strand_decoder(z_g[:, :6])
    uv = gen.uvs[idx]
    r = gc.restate(uv, z_g, v_g, torch.zeros(S_STEP, 11))
    gap, knee, _ = gc.conditions(r)
    assert gap >= 1e-5 and knee >= 1e-4, (gap, knee)                        # float32 and float64 choose the same neighbours
    nbr, w = r["nbr"], r["w"]                                                # (integers and UV-only weights: no gradient)
    a = v_g[nbr[:N]]
    u = a / gc._clamped_norm(a)
    full = (u[:, :, None] * u[:, None, :]).sum(-1).mean(-1)
    csim = torch.stack([full[:, j, k] for j in range(4) for k in range(j, 4)], -1).mean(-1)
    alpha = torch.where(csim <= 0.9, 1 - 1.63 * csim ** 5, 0.4 - 0.4 * csim)
    ai = (alpha[nbr] * w).sum(1)[N:, None]
    z = torch.cat([z_g, z_g[nbr[N:, 0]] * ai + (z_g[nbr[N:]] * w[N:, :, None]).sum(1) * (1 - ai)])
    assert torch.allclose(z.detach(), r["z"], rtol=1e-12, atol=1e-14)
    v = torch.cat([v_g, gen.strand_decoder(z[N:, :6])])
    p = sg.strands_to_world(v, gen.local2world, gen.origins, idx, gen.scale_decoder, fused=False)
    feats, conf = gen.appearance(z[:, 6:])
    l_diff = gen.prior_loss(gen.texture[:, :6])
    total = (p * rec["d_points"].double()).sum() + (feats * rec["d_features"].double()).sum() + tgs.LAMBDA_DIFF * l_diff
    if "d_orient_conf" in rec:
        total = total + (conf * rec["d_orient_conf"].double()).sum()
    (g,) = torch.autograd.grad(total, gen.texture)
    return dict(points=p.detach(), features=feats.detach(), orient_conf=conf.detach(), texture_grad=g, nbr=nbr)


def _guide_texels(gen, idx):
    tp, T = gen.taps, gen.texture_size
    mask = torch.zeros(T, T, dtype=torch.bool)
    for r in idx[:N_STEP].tolist():
        for k in range(4):
            x, y = int(tp.x0[r]) + (k & 1), int(tp.y0[r]) + (k >> 1)
            if 0 <= x < T and 0 <= y < T:
                mask[y, x] = True
    return mask


def test_one_iteration_of_the_latent_strand_stage_with_guiding_strands(monkeypatch):
    """latent_strand_training_step with linear stand-in decoders at Smax 120, S 40, N 9, L 8, T 8 on a 32 x 48 view, through the
    recorded step and the float64 iteration of tests/test_gpu_textured_strands.py with this file's generator in place of its own.
    points, the colour decoder's outputs and texture.grad of the HIP run and of the composed run are each held against the float64
    generator on that run's own draw and cotangents, and the step's loss of both against the whole iteration in float64:
    |loss - f64| <= 1e-5 |f64| + 3 |composed - f64|.  A second HIP run gives the same bits.  The appearance channels of
    texture.grad, which no prior term reaches, are zero outside the guides' texels."""
    from tests import test_gpu_textured_strands as tgs
    monkeypatch.setattr(tgs, "_tiny", _tiny)
    L = _lib.lib()
    L.ghr_set_deterministic(1)
    try:
        comp, fused, again = tgs._recorded_step(False), tgs._recorded_step(True), tgs._recorded_step(True)
    finally:
        L.ghr_set_deterministic(0)
    assert torch.equal(comp["idx"], fused["idx"]) and comp["points"].shape == (S_STEP, 8, 3)
    assert again["loss"] == fused["loss"] and torch.equal(again["texture_grad"], fused["texture_grad"])      # reproducible
    assert torch.equal(again["points"], fused["points"]) and torch.equal(again["features"], fused["features"])
    c64, f64 = _float64_of(comp), _float64_of(fused)
    for k in ("points", "features", "orient_conf", "texture_grad"):
        ref = (comp[k].double() - c64[k]).abs()
        for name, got, want in (("composed", comp, c64), ("fused", fused, f64)):
            err = (got[k].double() - want[k]).abs()
            bar = 1e-5 * want[k].abs().max() + 3 * ref
            print("%s %s: max err %.3e, max|f64| %.3e, composed err %.3e" % (name, k, float(err.max()), float(want[k].abs().max()), float(ref.max())))
            assert bool(torch.isfinite(got[k]).all()) and bool((err <= bar).all()), (name, k, float((err - bar).max()))
    mask = _guide_texels(_tiny("cpu", False), fused["idx"])
    assert int((~mask).sum()) > 0
    for rec in (comp, fused):
        app = rec["texture_grad"][0, 6:]
        assert float(app[:, ~mask].abs().max()) == 0.0 and float(app[:, mask].abs().max()) > 0
    assert float(f64["texture_grad"][0, 6:][:, ~mask].abs().max()) == 0.0
    (lc64, flips_c), (lf64, flips_f) = tgs._float64_loss(comp), tgs._float64_loss(fused)
    err_c, err_f = abs(comp["loss"] - lc64), abs(fused["loss"] - lf64)
    print("loss: composed %.9g (f64 %.12g, the double walk stops elsewhere on %d pixels), fused %.9g (f64 %.12g, %d pixels)" % (
        comp["loss"], lc64, flips_c, fused["loss"], lf64, flips_f))
    assert err_f <= 1e-5 * abs(lf64) + 3 * err_c and err_c <= 1e-5 * abs(lc64) + 3 * err_c, (err_c, err_f)


def test_the_texture_gradient_is_zero_outside_the_guides_texels_and_the_model_keeps_guiding_views():
    from gaussianhaircut_amd.scene.gaussian_model_latent_strands import GaussianModelLatentStrands
    for fused in (False, True):
        gen = _tiny(DEV, fused)
        gen.prior_loss = None                                                # (the prior term reaches every texel)
        out = gen(1)
        assert gen.last_num_guiding == N_STEP
        ((out["points"] ** 2).sum() + out["features"].sum() + out["orient_conf"].sum()).backward()
        g = gen.texture.grad[0].cpu()
        mask = _guide_texels(_tiny("cpu", False), gen.last_idx.cpu())
        assert float(g[:, ~mask].abs().max()) == 0.0 and float(g[:6][:, mask].abs().max()) > 0 and float(g[6:][:, mask].abs().max()) > 0
    for shared in (False, True):
        hair = GaussianModelLatentStrands(3, _tiny(DEV, True), None, fused=True, shared_appearance=shared)
        hair.initialize_gaussians_hair(1)
        P = N_STEP * 7
        rows = N_STEP if shared else P
        assert hair.num_guiding_strands == N_STEP and (hair.feature_rows_per_strand > 1) == shared
        assert hair._xyz_gdn.shape == (P, 3) and hair._dir_gdn.shape == (P, 3) and hair._xyz_gdn.data_ptr() == hair._xyz.data_ptr()
        assert hair._features_dc_gdn.shape == (rows, 1, 3) and hair._features_rest_gdn.shape == (rows, 15, 3)
        assert hair.get_features_gdn.shape == (rows, 16, 3)
        assert torch.equal(hair.get_features_gdn, torch.cat((hair._features_dc, hair._features_rest), dim=1)[:rows])
