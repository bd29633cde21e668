"""Time of one iteration of the latent-strand stage, fused (csrc/ghr_latent.h) against composed (the PyTorch expressions of
src/scene/gaussian_model_latent_strands.py:451-499 and src/train_latent_strands.py:130-152) and against `shared` (the fused
form with per-strand SH features read inside the projection, csrc/ghr_shared.h: GaussianModelLatentStrands(shared_appearance=True)),
in ONE process on one GPU:

    python tools/latentstep.py [out-file, default profiles/latent_stage.txt]

The three forms alternate, two passes; the spread of the `fused` form between the passes is printed next to the figures (it is the
yardstick: the same code with the option off).  Peak allocated memory is taken per form over its timed iterations.

Size: 30 000 strands x 100 points + 100 000 frozen head Gaussians at 1920 x 1080 -- the strand stage's bench size, CHOSEN HERE, not
read from a reference config.  The generator is a toy: a parameter tensor of points, a per-strand code and one linear layer to
the 48 SH coefficients and the log confidence.  The renderer is the fused one in both forms; what differs is what stands in front
of it (points -> Gaussians, per-strand appearance -> rows) and behind it (the loss).  Each figure is the device time between two
events, after warm-up; the forms alternate and the mean of the second round is printed.  The parts are timed on their own
through the same autograd functions with the step's tensors."""
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianhaircut_amd.gaussian_renderer import render_hair  # noqa: E402
from gaussianhaircut_amd.scene import gaussian_model_latent_strands as gml  # noqa: E402
from gaussianhaircut_amd.scene.cameras import ring_cameras  # noqa: E402
from gaussianhaircut_amd.trainer import latent_strand_training_step, latent_view_loss  # noqa: E402
from gaussianhaircut_amd.utils import synthetic as syn  # noqa: E402

S, L, N_HEAD, K = 30_000, 100, 100_000, 16
PIPE = SimpleNamespace(debug=False, fused_projection=True)


class Toy(torch.nn.Module):
    def __init__(self, points):
        super().__init__()
        g = torch.Generator().manual_seed(4)
        self.points = torch.nn.Parameter(points.clone())
        self.code = torch.nn.Parameter(torch.randn(points.shape[0], 8, generator=g).to(points.device))
        self.lin = torch.nn.Linear(8, 3 * K + 1).to(points.device)
        with torch.no_grad():
            self.lin.weight.mul_(0.3)

    def forward(self, iteration):
        z = self.lin(self.code)
        return {"points": self.points * 1.0, "features": z[:, :-1], "orient_conf": z[:, -1:]}


def timed(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def projection_parts(head, model, cam, bg, opt):
    """Device time of the hair segment's projection launches in `model`'s form -- k_project / k_project_bwd on expanded arrays, or
    k_shared_proj_fwd / k_shared_proj_bwd + k_shared_sh_fold on per-strand ones -- through the C ABI on the state of one real step
    (its gradient lines included: a zero d_rgb table would let the fold skip every row)."""
    import ctypes
    from gaussianhaircut_amd import _lib
    from gaussianhaircut_amd.gaussian_renderer import fused as fz
    from gaussianhaircut_amd.diff_gaussian_rasterization import _ptr, _stream
    lib = _lib.lib()
    model.initialize_gaussians_hair(0)
    pkg = render_hair(cam, head, model, PIPE, bg)
    latent_view_loss(pkg, cam, opt).backward(retain_graph=True)
    ctx = pkg.renders_packed.grad_fn
    xyz, scaling, rotation, dirs, conf, fdc, frest, view, proj, campos, bgt, radii_ws, geom, img, binb = ctx.saved_tensors
    n_head, n_hair, row0, rows = ctx.dims
    cfg, K, dev = ctx.cfg, ctx.K, xyz.device
    hair = dict(xyz=xyz, scaling=scaling, rotation=rotation, dir=dirs, conf=conf, fdc=fdc, frest=frest)
    m = fz._seg_args(n_hair, row0, cfg["W"], cfg["H"], cfg["sh_degree"], K, hair, [view, proj, campos, bgt, ctx.fov], cfg,
                     cfg["eps_hair"], (1.0, 1.0, 0.0))
    sf = fz._shared_features(cfg, n_hair)
    f32 = dict(dtype=torch.float32, device=dev)
    F = fdc.shape[0]
    d = dict(m2d=torch.empty((rows, 3), **f32), xyz=torch.empty((n_hair, 3), **f32), sc=torch.empty((n_hair, 3), **f32),
             rot=torch.empty((n_hair, 4), **f32), conf=torch.empty((n_hair, 1), **f32), dir=torch.empty((n_hair, 3), **f32),
             fdc=torch.empty((F, 1, 3), **f32), frest=torch.empty((F, K - 1, 3), **f32), rgb=torch.empty((n_hair, 3), **f32))
    pad = row0 - n_head
    radii_p = fz._ptr_rows(radii_ws, -pad, 4)
    scratch = ctx.scratch
    common = (rows, radii_p, _ptr(geom), _ptr(scratch), _ptr(d["m2d"]), _ptr(d["xyz"]), _ptr(d["sc"]), _ptr(d["rot"]), None, None,
              _ptr(d["conf"]), _ptr(d["fdc"]), _ptr(d["frest"]), _ptr(d["dir"]))

    def bwd():
        if sf is not None:
            _lib.check(lib.ghr_model_backward_segment_shared(_stream(), ctypes.byref(m), ctypes.byref(sf), *common, None,
                                                             scratch.shape[0], _ptr(binb), ctx.cap, _ptr(d["rgb"])))
        else:
            _lib.check(lib.ghr_model_backward_segment(_stream(), ctypes.byref(m), *common, 0, None, scratch.shape[0], _ptr(binb),
                                                      ctx.cap))

    def fold():
        _lib.check(lib.ghr_shared_sh_fold(_stream(), ctypes.byref(sf), cfg["sh_degree"], K, _ptr(xyz), _ptr(campos), _ptr(d["rgb"]),
                                          _ptr(d["fdc"]), _ptr(d["frest"]), None))
    out = {}
    timed(bwd, 3)
    out["bwd"] = timed(bwd, 20)
    if sf is not None:
        timed(fold, 3)
        out["fold"] = timed(fold, 20)
    # the forward launch into a workspace of its own (the step's state stays as the backward needs it); `first` = 1: the
    # counters are reset in front of every launch, in both forms
    gbytes, ibytes = _lib.forward_sizes(rows, cfg["W"], cfg["H"], False)
    geom2, img2 = torch.empty((gbytes,), dtype=torch.uint8, device=dev), torch.empty((ibytes,), dtype=torch.uint8, device=dev)
    radii2, m2d2 = torch.empty((rows,), dtype=torch.int32, device=dev), torch.empty((rows, 3), **f32)

    def fwd():
        if sf is not None:
            _lib.check(lib.ghr_model_forward_segment_shared(_stream(), ctypes.byref(m), ctypes.byref(sf), rows, 1, _ptr(geom2),
                                                            _ptr(img2), _ptr(radii2), _ptr(m2d2)))
        else:
            _lib.check(lib.ghr_model_forward_segment(_stream(), ctypes.byref(m), rows, 1, _ptr(geom2), _ptr(img2), _ptr(radii2),
                                                     _ptr(m2d2)))
    timed(fwd, 3)
    out["fwd"] = timed(fwd, 20)
    del pkg
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                   "profiles", "latent_stage.txt")
    dev = torch.device("cuda:0")
    spec = syn.CONFIGS["cfg3"]
    bg = syn.background(dev)
    head = syn.make_model(spec, dev)
    with torch.no_grad():
        head._label[:N_HEAD] = -4.0
        head._label[N_HEAD:] = 4.0
    head.precompute_head()
    g = torch.Generator().manual_seed(9)
    unit = torch.nn.functional.normalize
    step = torch.randn(S, L - 1, 3, generator=g) * 0.003 + unit(torch.randn(S, 1, 3, generator=g), dim=-1) * 0.01
    pts = (unit(torch.randn(S, 1, 3, generator=g), dim=-1) + torch.cat([torch.zeros(S, 1, 3), torch.cumsum(step, dim=1)], dim=1)).to(dev)
    cam = ring_cameras(1, spec.W, spec.H, device=dev)[0]
    opt = SimpleNamespace(lambda_dl1=1.0, lambda_dmask=0.1, lambda_dorient=0.1, lambda_dsds=0.0, use_gt_orient_conf=True,
                          train_orient_conf=True, iterations=10 ** 6, latent_lr=1e-4)
    with torch.no_grad():
        gt = gml.GaussianModelLatentStrands(3, Toy(pts * 1.02))
        gt.initialize_gaussians_hair(0)
        pkg = render_hair(cam, head, gt, PIPE, bg)
        cam.original_image, cam.original_mask = pkg["render"].clamp(0, 1).detach(), pkg["mask"].clamp(0, 1).detach()
        cam.original_orient_angle = pkg["orient_angle"].detach()
        cam.original_orient_conf = torch.ones_like(pkg["orient_conf"]).detach()
        del gt, pkg
    models = {}
    for name, fused in (("fused", True), ("composed", False), ("shared", True)):
        m = gml.GaussianModelLatentStrands(3, Toy(pts), fused=fused, shared_appearance=name == "shared")
        m.training_setup(opt)
        models[name] = m
    it = [0]

    def fused_step():
        it[0] += 1
        latent_strand_training_step(head, models["fused"], [cam], bg, opt, it[0], pipe=PIPE)

    def composed_step():
        it[0] += 1
        m = models["composed"]
        m.initialize_gaussians_hair(it[0])
        m.update_learning_rate(it[0])
        loss = latent_view_loss(render_hair(cam, head, m, PIPE, bg), cam, opt, fused=False)
        loss.backward()
        o = m.optimizer
        for param in o.param_groups[0]['params']:
            if param.grad is not None and param.grad.isnan().any():
                o.zero_grad()
        o.step()
        o.zero_grad(set_to_none=True)

    def shared_step():
        it[0] += 1
        latent_strand_training_step(head, models["shared"], [cam], bg, opt, it[0], pipe=PIPE)

    steps = {"fused": fused_step, "composed": composed_step, "shared": shared_step}
    res, passes, peak = {}, ({}, {}), {}
    for rnd in range(2):
        for name, fn in steps.items():
            timed(fn, 3 if rnd == 0 else 1)
            torch.cuda.reset_peak_memory_stats()
            res[name] = passes[rnd][name] = timed(fn, 8)
            peak[name] = torch.cuda.max_memory_allocated()
    assert models["shared"].feature_rows_per_strand == L - 1 and models["fused"].feature_rows_per_strand == 0
    spread = abs(passes[0]["fused"] - passes[1]["fused"])
    proj = {name: projection_parts(head, models[name], cam, bg, opt) for name in ("fused", "shared")}

    # the parts, on the step's tensors
    P = S * (L - 1)
    parts = {}
    for name, fused in (("fused", True), ("composed", False)):
        p = pts.clone().requires_grad_(True)
        cots = [torch.randn(P, n, device=dev) for n in (3, 4, 3, 3)]

        def build():
            return gml.build_from_points(p * 1.0, 1e-3, fused)
        outs = build()

        def build_bwd():
            torch.autograd.grad(outs, p, cots, retain_graph=True)
        srcs = [torch.randn(S, c, device=dev, requires_grad=True) for c in (3, 3 * K - 3, 1)]   # dc | rest | confidence
        gs = [torch.randn(P, c, device=dev) for c in (3, 3 * K - 3, 1)]

        def expand():
            return [gml.expand_rows(t, L - 1, fused) for t in srcs]
        ex = expand()

        def reduce():
            torch.autograd.grad(ex, srcs, gs, retain_graph=True)
        with torch.no_grad():
            m = models["fused"]
            m.initialize_gaussians_hair(0)
            packed = render_hair(cam, head, m, PIPE, bg).renders_packed.detach()
        r = packed.clone().requires_grad_(True)
        pk = {"render": r[0:3], "mask": r[3:5], "orient_conf": r[8:9]}
        from gaussianhaircut_amd.gaussian_renderer import orient_angle_from

        def loss_fwd():
            if fused:
                from gaussianhaircut_amd.fused_loss import latent_loss
                return latent_loss(r, cam, opt)
            q = dict(pk, orient_angle=orient_angle_from(r[5:8]))
            return latent_view_loss(q, cam, opt, fused=False)
        lv = loss_fwd()

        def loss_bwd():
            torch.autograd.grad(lv, r, retain_graph=True)
        for key, fn in (("build fwd", build), ("build bwd", build_bwd), ("expand fwd", expand), ("reduce bwd", reduce),
                        ("loss fwd", loss_fwd), ("loss bwd", loss_bwd)):
            timed(fn, 3)
            parts[(name, key)] = timed(fn, 20)

    lines = ["latent-strand stage, one iteration: %d strands x %d points + %d frozen head Gaussians = %d Gaussians, 1 view %dx%d"
             % (S, L, N_HEAD, P + N_HEAD, spec.W, spec.H),
             "(the size is the strand stage's bench size, chosen here, not read from a reference config; toy generator: points parameter,",
             " per-strand code, one linear layer; fused renderer in both forms; device time between two events, mean of 8 iterations)",
             "device: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__),
             "",
             "iteration  fused %.3f ms   composed %.3f ms   (%.2fx)" % (res["fused"], res["composed"], res["composed"] / res["fused"]),
             "iteration  shared %.3f ms  (fused - shared = %.3f ms; the fused form's two passes: %.3f / %.3f ms, spread %.3f ms)"
             % (res["shared"], res["fused"] - res["shared"], passes[0]["fused"], passes[1]["fused"], spread),
             "peak allocated, MB   fused %.0f   composed %.0f   shared %.0f" % tuple(peak[k] / 1e6 for k in ("fused", "composed", "shared")),
             "",
             "the hair segment's projection launches on the step's own state, ms (mean of 20)",
             "%-34s %10s %10s" % ("", "expanded", "per strand"),
             "%-34s %10.4f %10.4f" % ("projection forward", proj["fused"]["fwd"], proj["shared"]["fwd"]),
             "%-34s %10.4f %10.4f" % ("projection backward (+ fold)", proj["fused"]["bwd"], proj["shared"]["bwd"]),
             "fold alone %.4f ms: %d rows x 24 B = %.1f MB read, %.0f GB/s (derived floor at 8 TB/s: %.1f us, reached to %.0f %%)"
             % (proj["shared"]["fold"], P, P * 24 / 1e6, P * 24 / 1e6 / proj["shared"]["fold"], P * 24 / 8e6,
                100.0 * (P * 24 / 8e6) / (proj["shared"]["fold"] * 1e3)),
             "",
             "parts, ms (mean of 20; the composed form includes the `p * 1.0` / angle ops a caller also pays)",
             "%-12s %10s %10s" % ("", "fused", "composed")]
    for key in ("build fwd", "build bwd", "expand fwd", "reduce bwd", "loss fwd", "loss bwd"):
        lines.append("%-12s %10.4f %10.4f" % (key, parts[("fused", key)], parts[("composed", key)]))
    lines.append("expand + reduce, fused: %.4f ms (the copy a per-strand read inside the projection kernels would save)"
                 % (parts[("fused", "expand fwd")] + parts[("fused", "reduce bwd")]))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
