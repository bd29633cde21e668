"""`-m gpu`: the path bench.py times -- the FUSED render() (k_project -> binning -> k_render_fwd) -> loss -> backward
(k_render_bwd -> k_project_bwd) -- against the ORACLE CHAIN at BASELINE.json's full sizes (cfg2 100k blobs, cfg3 500k
strands, cfg5 2M strands, 1920x1080):

    CPU fp32 PyTorch projection of gaussianhaircut_amd.scene (pinned to outputs of the reference's own Python,
    tests/test_reference_golden.py)  ->  oracle.rasterize_forward / backward (tests/oracle_backend.py; pinned to the
    reference's CUDA, tests/test_reference_cuda_golden.py)  ->  PyTorch autograd to the raw parameters.

No quantile acceptance.  Differently rounded projection arithmetic may flip a discrete decision of K1 (radius ceil,
tile rect, cull): those Gaussians are COUNTED (bound 1e-4 of P) and the pixels of the tiles they touch are masked
together with the oracle's fragile pixels (alpha / T within 2e-5 of a threshold); the mask is applied by giving those
pixels zero weight in the loss on BOTH sides, which removes them exactly.  Everything else must agree:
K1 state bit for bit (depth keys, pixel means) or to 1e-5 (conic, opacity), the sorted tile lists exactly, the image to
1e-4, every raw-parameter gradient to 1e-4 * (|ref| + largest |ref| of its row) plus a floor for cancellation noise
(leg A: seeded random dL/dout).  Leg B (the real stage-1 loss) is arbitrated by the same chain evaluated in IEEE double
(oracle/ghr_oracle64.c): |HIP - f64| <= 3 |oracle32 - f64| + the row criterion, for every element.
"""
import math

import numpy as np
import pytest
import torch

from gaussianhaircut_amd.gaussian_renderer import _package, render
from gaussianhaircut_amd.utils import synthetic as syn
from tests import helpers as hp
from tests.projection_shared import FLOOR, FUSED, GENERIC, PARAMS, _row_close

pytestmark = pytest.mark.gpu


def _assert_rows(name, a, b, tol=hp.TOL, floor=FLOOR):
    assert np.isfinite(a).all(), name
    ok = _row_close(a, b, tol, floor)
    if not ok.all():
        a2, b2 = a.reshape(len(a), -1), b.reshape(len(b), -1)
        r, c = np.unravel_index(np.argmax(np.abs(a2 - b2) * ~ok), ok.shape)
        raise AssertionError("%s: %d of %d elements off; worst row %d col %d got %g ref %g (row max %g, tensor max %g)" %
                             (name, (~ok).sum(), ok.size, r, c, a2[r, c], b2[r, c], np.abs(b2[r]).max(), np.abs(b2).max()))


def _chains(cfg, dev, deg=3, cam="front"):
    """Forward of both chains + the stage-by-stage comparison.  Returns what the loss legs need."""
    from tests import oracle_backend as ob
    from tests.gpu_helpers import inspect_fused
    spec = syn.CONFIGS[cfg]
    W, H = spec.W, spec.H
    mc, mg = syn.make_model(spec, "cpu"), syn.make_model(spec, dev)
    mc.active_sh_degree = mg.active_sh_degree = deg
    cc, cg = syn.make_view(spec, "cpu", cam), syn.make_view(spec, dev, cam)
    with ob.oracle_rasterizer():
        pc = render(cc, mc, GENERIC, syn.background("cpu"))
    st = ob.LAST["state"]
    keep = mc.filter_points(cc).numpy()
    idx = np.nonzero(keep)[0]
    pg = render(cg, mg, FUSED, syn.background(dev))
    torch.cuda.synchronize()
    P = spec.P
    R = int(pg.count)
    ins = inspect_fused(pg.renders_packed, P, W, H, R)

    # ---- K1 state: radii, and for every Gaussian both chains rasterize identically: depth key bits, pixel mean bits,
    # conic / opacity values
    radii_c, radii_g = pc["radii"].numpy(), ins["radii"]
    assert np.array_equal(radii_g, pg["radii"].cpu().numpy())
    rect_c = np.zeros((P, 4), np.int64)  # x0, y0, x1, y1 of the oracle chain (auxiliary.h:46-56), recomputed from its state
    gx, gy = (W + 15) // 16, (H + 15) // 16
    xy, rad = st.xy.astype(np.float32), st.radii.astype(np.int64)
    def tile(v, g):
        return np.clip(np.trunc(v / np.float32(16)).astype(np.int64), 0, g)
    rect_c[idx, 0] = tile(xy[:, 0] - rad.astype(np.float32), gx)
    rect_c[idx, 1] = tile(xy[:, 1] - rad.astype(np.float32), gy)
    rect_c[idx, 2] = tile(xy[:, 0] + rad.astype(np.float32) + np.float32(16) - np.float32(1), gx)
    rect_c[idx, 3] = tile(xy[:, 1] + rad.astype(np.float32) + np.float32(16) - np.float32(1), gy)
    rect_c[radii_c == 0] = 0
    area_c = (rect_c[:, 2] - rect_c[:, 0]) * (rect_c[:, 3] - rect_c[:, 1])
    assert np.array_equal(area_c[idx], st.tiles_touched.astype(np.int64))
    rg = ins["rects"]
    rect_g = np.stack([rg[:, 0] & 0xffff, rg[:, 1] & 0xffff, rg[:, 0] >> 16, rg[:, 1] >> 16], axis=1).astype(np.int64)
    rect_g[radii_g == 0] = 0
    flipped = (radii_c != radii_g) | (rect_c != rect_g).any(axis=1)
    n_flip = int(flipped.sum())
    assert n_flip <= max(2, int(1e-4 * P)), "K1 decisions differ for %d of %d Gaussians" % (n_flip, P)
    same = (radii_c > 0) & ~flipped
    kept_pos = np.full(P, -1, np.int64)
    kept_pos[idx] = np.arange(idx.size)
    j = kept_pos[same]
    assert (j >= 0).all()
    np.testing.assert_array_equal(ins["depths"][same].view(np.uint32), st.depths[j].view(np.uint32))
    np.testing.assert_array_equal(ins["rec"][same, 0:2].view(np.uint32), st.xy[j].view(np.uint32))
    co_g, co_c = ins["rec"][same, 2:6], st.conic_opacity[j]
    rel = np.abs(co_g - co_c) / (np.abs(co_c).max(axis=1, keepdims=True) + 1e-30)
    assert rel.max() < 5e-6, "conic / opacity of k_project vs the host projection: %g" % rel.max()

    # ---- binning: the tile lists are identical once the flipped Gaussians are taken out of both
    pl_c = idx[st.point_list.astype(np.int64)]
    pl_g = ins["point_list"].astype(np.int64)
    np.testing.assert_array_equal(pl_g[~flipped[pl_g]], pl_c[~flipped[pl_c]])
    if n_flip == 0:
        assert R == st.num_rendered
        ts = ins["tile_start"]
        r = np.stack([ts[:-1], ts[1:]], axis=1).astype(np.uint32)
        r[ts[:-1] == ts[1:]] = 0
        np.testing.assert_array_equal(r, st.ranges)

    # ---- pixel mask: oracle-fragile pixels + every pixel of a tile a flipped Gaussian touches in either chain
    mask = st.fragile.reshape(H, W).astype(bool).copy()
    assert mask.mean() < 2e-3
    for g_ in np.nonzero(flipped)[0]:
        for rc in (rect_c[g_], rect_g[g_]):
            mask[16 * rc[1]:16 * rc[3], 16 * rc[0]:16 * rc[2]] = True
    assert mask.mean() < 5e-3, "masked fraction %g" % mask.mean()
    ok = ~mask.reshape(-1)
    if n_flip == 0:
        np.testing.assert_array_equal(ins["n_contrib"][ok], st.n_contrib[ok])

    # ---- image (all 10 channels of the packed output, and the derived orientation angle), tolerance 1e-4
    img_c = pc.renders_packed.detach().numpy().reshape(10, -1)[:, ok]
    img_g = pg.renders_packed.detach().cpu().numpy().reshape(10, -1)[:, ok]
    assert np.isfinite(img_g).all()
    close = hp.image_close(img_g, img_c)
    assert close.all(), "%d px-channels off, max err %g" % ((~close).sum(), np.abs(img_g - img_c).max())
    ang_c = pc["orient_angle"].detach().numpy().reshape(-1)[ok]
    ang_g = pg["orient_angle"].detach().cpu().numpy().reshape(-1)[ok]
    # |d acos| <= 22.4 |dx| inside the clamp; only compare where the 2D direction is not ~0 (normalize of a null vector)
    nrm = np.linalg.norm(pc.renders_packed.detach().numpy().reshape(10, -1)[5:7, :][:, ok], axis=0)
    assert (np.abs(ang_g - ang_c)[nrm > 1e-2] < 1e-3).all()
    vs_c, vs_g = pc["viewspace_points"].detach().numpy(), pg["viewspace_points"].detach().cpu().numpy()
    assert np.abs(vs_g[keep][:, :2] - vs_c[keep][:, :2]).max() < 1e-5
    stats = dict(n_flip=n_flip, masked=float(mask.mean()), R=R, img_err=float(np.abs(img_g - img_c).max()),
                 conic_rel=float(rel.max()))
    return spec, (mc, cc, pc), (mg, cg, pg), torch.from_numpy(mask), stats


def ob_state_n_contrib(pkg):
    from tests import oracle_backend as ob
    return ob.LAST["state"].n_contrib


def _grads(model, pkg):
    g = {n: getattr(model, n).grad.detach().cpu().numpy().copy() for n in PARAMS}
    g["viewspace"] = pkg["viewspace_points"].grad.detach().cpu().numpy().copy()
    for n in PARAMS:
        getattr(model, n).grad = None
    pkg["viewspace_points"].grad = None
    return g


# cameras: scene/cameras.py:parity_camera (rotated / rolled ring views: k_project's T = W J, the strand direction and the SH
# view direction all see a full 3x3 view rotation there, as with the COLMAP poses of src/scene/cameras.py:72-80)
@pytest.mark.parametrize("cfg,cam", [("cfg2", "front"), ("cfg3", "front"), ("cfg5", "front"), ("cfg3", "ring13roll"),
                                     ("cfg2", "ring5")])
def test_fused_render_loss_backward_vs_oracle_chain_full_size(oracle_mod, cfg, cam):
    from gaussianhaircut_amd.fused_loss import stage1_loss
    from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
    from gaussianhaircut_amd.trainer import view_loss
    dev = torch.device("cuda:0")
    spec, (mc, cc, pc), (mg, cg, pg), mask, stats = _chains(cfg, dev, cam=cam)
    H, W = spec.H, spec.W

    # ---- leg A: a seeded linear functional of the 10 output planes (dL/dout ~ N(0,1), SURVEY 8(d) cfg 2), zero on the
    # masked pixels.  Exercises k_render_bwd + k_project_bwd alone.
    w = syn.grad_image(spec, 101) * (H * W)
    w[:, mask] = 0.0
    (pc.renders_packed * w).sum().backward(retain_graph=True)
    (pg.renders_packed * w.to(dev)).sum().backward(retain_graph=True)
    gc, gg = _grads(mc, pc), _grads(mg, pg)
    for k in gc:
        _assert_rows("legA " + k, gg[k], gc[k])

    # ---- leg B: the stage-1 loss of train_gaussians.py:126-140 (masked L1 + SSIM + mask L1 + orientation, run.sh
    # weights) towards the render of a perturbed model.  The SSIM window couples neighbouring pixels, so the masked
    # pixels are neutralised by VALUE as well: both chains see the oracle chain's numbers there, without gradient.
    # The loss itself has kinks (|x - gt| at 0, the wrapped orientation difference at 0 and +-1/2, the mirror sign and
    # the acos clamp of gaussian_renderer/__init__.py:102-105): pixels where the oracle chain sits within 2e-4 of one
    # are "loss-fragile" -- the two chains may legitimately take different branches there -- and join the mask.
    opt = OptimizationParams()
    opt.lambda_dorient = 0.1
    gt = syn.make_model(spec, dev)
    with torch.no_grad():
        gen = torch.Generator().manual_seed(202)
        gt._features_dc.add_(0.3)
        gt._xyz.add_(0.002 * torch.randn(gt._xyz.shape, generator=gen).to(dev))
        gt._rotation.add_(0.05 * torch.randn(gt._rotation.shape, generator=gen).to(dev))
        pgt = render(cg, gt, FUSED, syn.background(dev))
        # the maps are pushed away from the model's own render (scale + offset) so that |x - gt| and the wrapped
        # orientation difference sit at a kink only by coincidence, as with real photographs
        maps = dict(original_image=(pgt["render"] * 0.85 + 0.03).clamp(0, 1),
                    original_mask=(pgt["mask"] * 0.9 + 0.02).clamp(0, 1),
                    original_orient_angle=torch.remainder(pgt["orient_angle"] + 0.013, 1.0),
                    original_orient_conf=torch.ones_like(pgt["orient_conf"]))
    for k, v in maps.items():
        setattr(cg, k, v.detach().contiguous())
        setattr(cc, k, v.detach().cpu().contiguous())
    del gt, pgt
    with torch.no_grad():
        eps = 2e-4  # twice the image tolerance: the chains' own values may differ by up to 1e-4
        pk = pc.renders_packed.detach()
        lf = ((pk[0:3] - cc.original_image).abs() < eps).any(dim=0) & (cc.original_mask[1] > 0)
        lf |= ((pk[3:5] - cc.original_mask).abs() < eps).any(dim=0)
        d2 = pk[5:7]
        nrm = d2.norm(dim=0)
        hair = cc.original_mask[0] > 0                       # weight of the orientation term (train_gaussians.py:130)
        ydir = d2[1].abs() / nrm.clamp_min(1e-30)
        dd = pc["orient_angle"].detach()[0] - cc.original_orient_angle[0]
        kink = torch.stack([dd.abs(), (dd - 0.5).abs(), (dd + 0.5).abs(), (dd - 1).abs(), (dd + 1).abs()]).min(dim=0).values
        lf |= hair & ((nrm < 1e-3) | (d2[0].abs() < 1e-4 * nrm) | ((ydir - (1 - 1e-3)).abs() < eps) | (kink < eps))
        has_splats = torch.from_numpy((ob_state_n_contrib(pc) > 0).reshape(H, W))
        stats["loss_fragile"] = float((lf & has_splats).float().mean())
        print("fullsize", cfg, stats, flush=True)
        assert stats["loss_fragile"] < 4e-2, stats
        mask = mask | lf
    # ---- the arbiter's forward pass (see below): the same chain in IEEE double.  Its inputs are the double projection's
    # -- up to 2.5e-6 (conic of a needle) from the fp32 chains' -- and T = prod (1 - alpha) amplifies that by
    # alpha / (1 - alpha) per factor: on a few pixels the stop decision T (1 - alpha) < 1e-4 (forward.cu:375-380) falls
    # the other way in double although fp32 arithmetic noise alone (the oracle's `fragile` flag) would not flip it.
    # Those pixels are COUNTED (bound 2e-3 of the frame) and leave all three chains like the other named pixels.
    from tests import oracle_backend as ob
    st32 = ob.LAST["state"]
    m64, c64 = ob.double_chain(mc, cc, mc.filter_points(cc))
    with ob.oracle_rasterizer64(st32):
        p64 = render(c64, m64, GENERIC, syn.background("cpu").double())
    flip64 = torch.from_numpy((ob.LAST["n_contrib64"] != st32.n_contrib).reshape(H, W))
    stats["double_walk_decides_otherwise"] = float((flip64 & ~mask).float().mean())
    assert stats["double_walk_decides_otherwise"] < 2e-3, stats
    mask = mask | flip64
    frozen = pc.renders_packed.detach()
    packed_c = torch.where(mask[None], frozen, pc.renders_packed)
    packed_g = torch.where(mask[None].to(dev), frozen.to(dev), pg.renders_packed)
    packed_c.retain_grad()
    packed_g.retain_grad()
    loss_c = view_loss(_package(packed_c, pc["viewspace_points"], pc["radii"]), cc, opt, fused=False)
    loss_g = stage1_loss(packed_g, cg.original_image, cg.original_mask, cg.original_orient_angle,
                         cg.original_orient_conf, opt.lambda_dl1, opt.lambda_dssim, opt.lambda_dmask,
                         opt.lambda_dorient)
    assert abs(float(loss_g.detach()) - float(loss_c.detach())) <= 2e-5 * abs(float(loss_c.detach())), (float(loss_g), float(loss_c))
    loss_c.backward()
    loss_g.backward()
    # dL/d(packed output) of the two loss implementations on the unmasked pixels (the fused loss has its own parity
    # tests against PyTorch, tests/test_gpu_loss_adam.py; here it locates a disagreement, should one appear)
    dc = packed_c.grad.numpy().reshape(10, -1)
    dg = packed_g.grad.cpu().numpy().reshape(10, -1)
    keep_px = ~mask.numpy().reshape(-1)
    dd = np.abs(dg - dc)[:, keep_px]
    ch, px = np.unravel_index(np.argmax(dd), dd.shape)
    stats["dL_err_of_max"] = float(dd.max() / np.abs(dc).max())
    stats["dL_worst"] = (int(ch), int(np.nonzero(keep_px)[0][px]), float(dg[:, keep_px][ch, px]), float(dc[:, keep_px][ch, px]))
    print("fullsize", cfg, stats, flush=True)
    assert stats["dL_err_of_max"] < 1e-4, stats
    gc, gg = _grads(mc, pc), _grads(mg, pg)
    # ---- the arbiter: the SAME chain evaluated in IEEE double -- PyTorch projection in float64 from
    # the same raw parameters, the oracle's compositing walk compiled in double (oracle/ghr_oracle64.c) over the fp32
    # oracle's lists, the same loss in double, the same masked pixels.  The reference's T <- T / (1 - alpha) turns a
    # relative difference eps in alpha into eps alpha / (1 - alpha) (x 99 at the clamp), which a smooth loss sums
    # coherently: two fp32 chains may differ by 1e-3 of a row there and both be right.  Round 2 argued that with a
    # conditioning-aware tolerance; here it is measured: the HIP path must be no further from the double result than
    # 3 x the fp32 oracle chain is, plus the 1e-4 row criterion (+ the cancellation floor) -- for EVERY element.
    packed_64 = torch.where(mask[None], frozen.double(), p64.renders_packed)
    loss_64 = view_loss(_package(packed_64, p64["viewspace_points"], p64["radii"]), c64, opt, fused=False)
    assert abs(float(loss_64.detach()) - float(loss_c.detach())) <= 2e-5 * abs(float(loss_64.detach()))
    loss_64.backward()
    g64 = {n: getattr(m64, n).grad.detach().numpy() for n in PARAMS}
    g64["viewspace"] = p64["viewspace_points"].grad.detach().numpy()
    bad, worst, outl = {}, {}, {}
    for k in gc:
        a, b, r = (x.reshape(len(x), -1).astype(np.float64) for x in (gg[k], gc[k], g64[k]))
        rows = np.abs(r).max(axis=1, keepdims=True)
        bar = 3.0 * np.abs(b - r) + hp.TOL * (np.abs(r) + rows) + FLOOR * np.abs(r).max()
        off = np.abs(a - r) > bar
        # how far each fp32 chain is from the double one, in units of the plain row criterion (reported, not judged)
        unit = hp.TOL * (np.abs(r) + rows) + FLOOR * np.abs(r).max()
        worst[k] = (float((np.abs(a - r) / unit).max()), float((np.abs(b - r) / unit).max()))
        if off.any():
            # The fp32 oracle is not a level reference for sums: it accumulates each Gaussian's gradient in DOUBLE and
            # rounds once (oracle/ghr_oracle.c, K8), the HIP path adds fp32 line by line.  On a row whose pixel terms cancel
            # (SSIM's dL/dpixel changes sign inside a splat) that alone is worth a few 1e-4 of the row.  Such elements are
            # counted and bounded: at most 1e-5 of a tensor (measured: 7 of 1.2e8 elements on cfg5, none on cfg2 / cfg3),
            # none further than 10 x the bar.
            i, j = np.unravel_index(np.argmax((np.abs(a - r) - bar) / bar), off.shape)
            rec = (int(off.sum()), int(i), int(j), float(a[i, j]), float(b[i, j]), float(r[i, j]), float(rows[i, 0]),
                   float((np.abs(a - r) / bar).max()))
            outl[k] = rec
            if off.sum() > max(3, int(1e-5 * off.size)) or (np.abs(a - r) > 10.0 * bar).any():
                bad[k] = rec
    print("fullsize", cfg, "legB distance from the double chain in units of the 1e-4 row criterion (HIP, fp32 oracle chain):",
          {k: (round(v[0], 2), round(v[1], 2)) for k, v in worst.items()}, flush=True)
    print("fullsize", cfg, "legB elements beyond 3 x oracle32 + row criterion (count, row, col, HIP, oracle32, f64, row max, "
          "worst / bar):", outl, flush=True)
    assert not bad, "further from the double chain than allowed: %s" % bad
    print("fullsize", cfg, stats, "loss", float(loss_c.detach()))
