"""Time of one frame of the strand preview (gaussianhaircut_amd.strand_view), HIP kernels against the PyTorch-composed form, in
ONE process on one GPU:

    python tools/strandviewstep.py > profiles/strand_preview.txt

30 000 strands of 100 points grown from a UV sphere of 9976 faces (116 x 44: the face count of the reference's head mesh, which is
not redistributable), 1080 x 1920, a ring of cameras at radius 3.4.  Forms, all at supersample 1 on the same frames:
  fused     rasterize_strands(fused=True): 8h's mesh raster (ghr_vis_view), the face depth and ghr_strandview_raster, plus
            ghr_strandview_shade -- one frame as render_strands makes it, without the resolve;
  raster    ghr_strandview_raster alone (its fill and five kernels) on planes made before;
  composed  rasterize_strands(fused=False) and the composed shader, over the first STRANDVIEWSTEP_COMPOSED_FRAMES frames (default
            1) with larger chunks than its default: it takes seconds per frame.
and, with self-shadowing (a light map of STRANDVIEWSTEP_LIGHT_SIZE, default 1024, the light following the camera):
  shadowed    the light pass (ghr_vis_view and the face depth in the light view, ghr_strandview_opacity), then the fused frame with
              ghr_strandview_shade_shadowed in the place of ghr_strandview_shade -- a frame as render_strands(shadows=True) makes
              it, without the resolve and without the fit of the light view (one per frame, made before anything is timed);
  light       ghr_strandview_opacity alone (its fill and five kernels) on every frame's light view;
  composed_s  the composed light pass, raster and shadowed shader over the same first frames.
Each figure is the device time between two events around a pass over the frames, after a warm-up of every form; the forms
alternate and every round is printed.  The planes and bytes of the forms are compared for equality before anything is timed.
The floor beside the figures is derived, not measured."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianhaircut_amd import _lib  # noqa: E402
from gaussianhaircut_amd import strand_view as sv  # noqa: E402
from gaussianhaircut_amd import visibility as vis  # noqa: E402
from tests import mesh_cases as mc  # noqa: E402
from tests import strand_view_cases as sc  # noqa: E402
from tests.visibility_cases import _look_at  # noqa: E402

HBM_BPS = 6.29e12  # measured float4 copy rate of the part (8.0e12 spec)


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def ring(n, H, W, radius=3.4):
    f = 1.6 * min(H, W) / 2.0
    K = np.array([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1.0]])
    return [vis.view_matrix(K, *_look_at((radius * np.sin(a), 0.35, radius * np.cos(a)), (0.0, 0.0, 0.0)))
            for a in 2 * np.pi * np.arange(n) / n]


def main():
    assert torch.cuda.is_available(), "strandviewstep needs a ROCm GPU (a CPU run measures nothing)"
    dev = torch.device("cuda:0")
    S, L = int(os.environ.get("STRANDVIEWSTEP_STRANDS", 30000)), int(os.environ.get("STRANDVIEWSTEP_POINTS", 100))
    H, W = (int(x) for x in os.environ.get("STRANDVIEWSTEP_SIZE", "1080x1920").split("x"))
    n_frames, n_cmp = int(os.environ.get("STRANDVIEWSTEP_FRAMES", 16)), int(os.environ.get("STRANDVIEWSTEP_COMPOSED_FRAMES", 1))
    rounds, r = 2, 0.75
    LS = int(os.environ.get("STRANDVIEWSTEP_LIGHT_SIZE", sv.SHADOW_SIZE))
    v, f = mc.uv_sphere(116, 44)
    pts = torch.from_numpy(sc.hair(S, L, 1, through=False)).to(dev)
    views = ring(n_frames, H, W)
    vd, fd = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    print("STRANDVIEWSTEP strands=%d points=%d segments=%d faces=%d %dx%d frames=%d (composed form over the first %d) half_width=%g"
          % (S, L, S * (L - 1), len(f), H, W, n_frames, n_cmp, r))

    def frame(M, fused):
        if fused:
            planes = sv.rasterize_strands(pts, M, H, W, mesh=(vd, fd), half_width=r, device=dev)
            return planes, sv._shade_fused(pts, vd, fd, H, W, planes[0], planes[2], sv.MODES["kajiya"], sv.shading_for_view(M), None)
        pix = vis._rasterize_torch(vd, fd.long(), M, H, W, vis.NEAR)
        qf = sv._face_depth_torch(vd, fd.long(), M, H, W, vis.NEAR, pix)
        planes = sv._rasterize_torch(pts, M, H, W, r, 0.0, vis.NEAR, pix, qf, chunk_elems=1 << 29)
        return planes, sv._shade_torch(pts, vd, fd.long(), H, W, planes[0], planes[2], sv.MODES["kajiya"], sv.shading_for_view(M))

    shadings = [sv.shading_for_view(M) for M in views]
    lights = [sv.light_view(pts, (vd, fd), light=sh["light"], size=LS) for sh in shadings]

    def shadowed(k, fused):
        M, sh, (Ml, Hl, Wl, rho) = views[k], shadings[k], lights[k]
        layer = rho / sv.SHADOW_LAYERS_PER_RADIUS
        if fused:
            sm = sv._shadow_map(pts, vd, fd, Ml, Hl, Wl, sv.SHADOW_HALF_WIDTH, layer, vis.NEAR, True)
            planes = sv.rasterize_strands(pts, M, H, W, mesh=(vd, fd), half_width=r, device=dev)
            return sm, sv._shade_shadowed_fused(pts, vd, fd, H, W, planes[0], planes[2], planes[1], sv.MODES["kajiya"], sh, None, sm,
                                                sv.SHADOW_KAPPA, sv.SHADOW_BIAS)
        qfl = sv._face_depth_torch(vd, fd.long(), Ml, Hl, Wl, vis.NEAR, vis._rasterize_torch(vd, fd.long(), Ml, Hl, Wl, vis.NEAR))
        q0, layers = sv._opacity_torch(pts, Ml, Hl, Wl, sv.SHADOW_HALF_WIDTH, layer, vis.NEAR, chunk_elems=1 << 29)
        sm = sv.ShadowMap(Ml, Hl, Wl, float(vis.NEAR), q0, layers, qfl, float(np.float32(layer)))
        pix = vis._rasterize_torch(vd, fd.long(), M, H, W, vis.NEAR)
        qf = sv._face_depth_torch(vd, fd.long(), M, H, W, vis.NEAR, pix)
        planes = sv._rasterize_torch(pts, M, H, W, r, 0.0, vis.NEAR, pix, qf, chunk_elems=1 << 29)
        return sm, sv._shade_torch(pts, vd, fd.long(), H, W, planes[0], planes[2], sv.MODES["kajiya"], sh, t=planes[1], shadow=sm,
                                   kappa=sv.SHADOW_KAPPA, bias=sv.SHADOW_BIAS)

    # the raster alone, on planes made before
    fr = sv._frames_for(S, L, H, W, len(v), len(f), dev)
    pix0, _ = vis._view_fused(vd, fd, views[0], H, W, vis.NEAR, None, None, fr.vis_ws, None, None)
    out = [torch.empty((H, W), dtype=dt, device=dev) for dt in (torch.int32, torch.float32, torch.int32, torch.float32)]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    Mcs = [sv._mc(M) for M in views]
    _lib.check(_lib.lib().ghr_strandview_face_depth(stream, len(v), ptr(vd), len(f), ptr(fd), ctypes.byref(Mcs[0]), float(vis.NEAR), H, W,
                                                    ptr(pix0), ptr(fr.qf)))

    def raster_only():
        for Mc in Mcs:      # (the head planes are those of frame 0: the strand work is each frame's own)
            _lib.check(_lib.lib().ghr_strandview_raster(stream, S, L, ptr(pts), ctypes.byref(Mc), float(vis.NEAR), H, W, r, 0.0, ptr(pix0),
                                                        ptr(fr.qf), ptr(fr.ws), *[ptr(t) for t in out]))

    lfr = sv._light_frames_for(S, L, LS, LS, len(v), len(f), dev)
    lq0 = torch.empty((LS, LS), dtype=torch.float32, device=dev)
    llayers = torch.empty((LS, LS, 4), dtype=torch.int32, device=dev)
    Lcs = [sv._mc(lv[0]) for lv in lights]

    def light_only():
        for Mc, lv in zip(Lcs, lights):
            _lib.check(_lib.lib().ghr_strandview_opacity(stream, S, L, ptr(pts), ctypes.byref(Mc), float(vis.NEAR), LS, LS,
                                                         sv.SHADOW_HALF_WIDTH, lv[3] / sv.SHADOW_LAYERS_PER_RADIUS, ptr(lfr.ws),
                                                         lfr.ws.numel(), ptr(lq0), ptr(llayers)))

    forms = {"fused": (lambda: [frame(M, True) for M in views], n_frames), "raster": (raster_only, n_frames),
             "composed": (lambda: [frame(M, False) for M in views[:n_cmp]], n_cmp),
             "shadowed": (lambda: [shadowed(k, True) for k in range(n_frames)], n_frames), "light": (light_only, n_frames),
             "composed_s": (lambda: [shadowed(k, False) for k in range(n_cmp)], n_cmp)}
    for M in views[:n_cmp]:
        (pa, ra), (pb, rb) = frame(M, True), frame(M, False)
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(pa, pb)) and torch.equal(ra, rb), "the forms disagree"
    seg = frame(views[0], True)[0][0]
    print("STRANDVIEWSTEP forms equal on %d frames (four planes and the bytes); frame 0: strand pixels %d, head pixels %d of %d"
          % (n_cmp, int((seg >= 0).sum()), int((frame(views[0], True)[0][2] >= 0).sum()), H * W))
    for k in range(n_cmp):
        (ma, ra), (mb, rb) = shadowed(k, True), shadowed(k, False)
        assert torch.equal(ma.q0.view(torch.int32), mb.q0.view(torch.int32)) and torch.equal(ma.layers, mb.layers) and \
            torch.equal(ma.qfl.view(torch.int32), mb.qfl.view(torch.int32)) and torch.equal(ra, rb), "the shadowed forms disagree"
    ma, ra = shadowed(0, True)
    plain = frame(views[0], True)[1]
    print("STRANDVIEWSTEP shadowed forms equal on %d frames (q0, the layer counts, qfl and the bytes); frame 0: light map %dx%d, texels "
          "with strands %d, layer counts %s, pixels darker than unshadowed %d"
          % (n_cmp, LS, LS, int((ma.q0 > 0).sum()), ma.layers.sum(dim=(0, 1)).tolist(), int((ra < plain).any(dim=2).sum())))
    for name, (fn, _) in forms.items():
        if not name.startswith("composed"):     # (the composed forms have just run: the equality checks above are their warm-up)
            fn()
    best = {}
    for rd in range(rounds):
        for name, (fn, n) in forms.items():
            per = timed(fn) / n
            best[name] = min(best.get(name, per), per)
            print("STRANDVIEWSTEP round %d %-8s %.4f ms per frame" % (rd, name, per))
    # derived: every segment's 32-B record written once and read once, at least one 4-B list entry per segment written and read,
    # 16 B of planes and 3 B of picture per pixel
    K = S * (L - 1)
    floor = (2 * 32.0 * K + 2 * 4.0 * K + 19.0 * H * W) / HBM_BPS * 1e3
    print("STRANDVIEWSTEP floor (DERIVED: traffic at the measured copy rate) %.5f ms per frame; fused %.4f, raster alone %.4f, "
          "composed %.4f ms per frame; fused / composed = %.5f" % (floor, best["fused"], best["raster"], best["composed"],
                                                                  best["fused"] / best["composed"]))
    print("STRANDVIEWSTEP shadows: shadowed %.4f, light pass alone %.4f, composed %.4f ms per frame; shadowed / fused = %.3f; "
          "shadowed / composed = %.5f" % (best["shadowed"], best["light"], best["composed_s"], best["shadowed"] / best["fused"],
                                          best["shadowed"] / best["composed_s"]))


if __name__ == "__main__":
    main()
