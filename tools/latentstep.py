"""Time of one iteration of the latent-strand stage, fused (csrc/ghr_latent.h) against composed (the PyTorch expressions of
src/scene/gaussian_model_latent_strands.py:451-499 and src/train_latent_strands.py:130-152), in ONE process on one GPU:

    python tools/latentstep.py [out-file, default profiles/latent_stage.txt]

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
    for name, fused in (("fused", True), ("composed", False)):
        m = gml.GaussianModelLatentStrands(3, Toy(pts), fused=fused)
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

    steps = {"fused": fused_step, "composed": composed_step}
    res = {}
    for rnd in range(2):
        for name, fn in steps.items():
            timed(fn, 3 if rnd == 0 else 1)
            res[name] = timed(fn, 8)

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
