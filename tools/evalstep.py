"""Time of the evaluation pass, HIP kernels against the PyTorch-composed comparator (gaussianhaircut_amd.evaluation, fused=True /
fused=False), in ONE process on one GPU:

    python tools/evalstep.py [views] > profiles/eval_pass.txt

cfg3 (500k strand-aligned Gaussians, 1080p), `views` ring cameras supervised by a perturbed copy of the model.  Each figure is
the device time between two events around the whole pass (issue and execution; evaluate_views ends with its one read of the
table), after a warm-up pass of each form; the forms alternate and the second round is the one printed.  "tail" is the same with
the render taken out: the metric / product functions alone on one view's packed output, `views` times.  Launches per view are
counted by torch.profiler over a two-view pass (device kernel events; copies excluded)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianhaircut_amd import evaluation as ev  # noqa: E402
from gaussianhaircut_amd.gaussian_renderer import render  # noqa: E402
from gaussianhaircut_amd.scene.cameras import ring_cameras  # noqa: E402
from gaussianhaircut_amd.trainer import PIPE, make_ground_truth  # noqa: E402
from gaussianhaircut_amd.utils import synthetic as syn  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def kernel_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = 0
        for e in prof.events():
            if e.device_type == torch.autograd.DeviceType.CUDA and not any(s in e.name.lower() for s in ("memcpy", "memset", "copy")):
                n += 1
        return n
    except Exception as exc:   # the count is a by-product: say so rather than lose the timings
        print("EVALSTEP launch count not taken: %r" % (exc,))
        return None


def main():
    V = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    dev = torch.device("cuda:0")
    spec = syn.CONFIGS[os.environ.get("EVALSTEP_CFG", "cfg3")]
    bg = syn.background(dev)
    model = syn.make_model(spec, dev)
    cams = ring_cameras(V, spec.W, spec.H, device=dev)
    with torch.no_grad():
        gt = syn.make_model(spec, dev)
        g = torch.Generator(device="cpu").manual_seed(202)
        gt._xyz.add_((0.002 * torch.randn(gt._xyz.shape, generator=g)).to(dev))
        gt._features_dc.add_((0.1 * torch.randn(gt._features_dc.shape, generator=g)).to(dev))
        make_ground_truth(gt, cams, bg)
        del gt
        packed = render(cams[0], model, PIPE, bg).renders_packed.clone()
    c = cams[0]
    gts = (c.original_image, c.original_mask, c.original_orient_angle, c.original_orient_conf)
    table = torch.empty((V, 8), dtype=torch.float64, device=dev)
    scratch = torch.empty(ev.eval_scratch_floats(spec.W, spec.H), dtype=torch.float32, device=dev)
    block = torch.empty(ev.product_block_bytes(spec.W, spec.H), dtype=torch.uint8, device=dev)

    def render_only():
        with torch.no_grad():
            for cam in cams:
                render(cam, model, PIPE, bg)

    def tail_metrics(fused):
        with torch.no_grad():
            for v in range(V):
                if fused:
                    ev.metrics_fused(packed, *gts, row=table[v], scratch=scratch)
                else:
                    ev.metrics_torch(packed, *gts)

    def tail_products(fused):
        with torch.no_grad():
            for v in range(V):
                if fused:
                    ev.products_fused(packed, block).cpu()
                else:
                    ev.products_torch(packed)

    passes = [("render alone", render_only),
              ("evaluate_views fused", lambda: ev.evaluate_views(model, cams, bg, fused=True)),
              ("evaluate_views torch", lambda: ev.evaluate_views(model, cams, bg, fused=False)),
              ("metric tail fused", lambda: tail_metrics(True)),
              ("metric tail torch", lambda: tail_metrics(False)),
              ("render_products fused", lambda: [None for _ in ev.render_products(model, cams, bg, fused=True, copy=False)]),
              ("render_products torch", lambda: [None for _ in ev.render_products(model, cams, bg, fused=False)]),
              ("product tail fused (launch + D2H of 16 B/pixel, blocking)", lambda: tail_products(True)),
              ("product tail torch (7 float products to the host, 8-bit on the device)", lambda: tail_products(False))]
    print("EVALSTEP %s, %d x %d, %d views, one process, device events" % (spec.name, spec.W, spec.H, V))
    res = {}
    for rnd in range(2):
        for name, fn in passes:
            ms = timed(fn)
            if rnd == 1:
                res[name] = ms / V
                print("EVALSTEP %-75s %9.4f ms per view" % (name, ms / V))
    for a, b in (("evaluate_views", "evaluate_views"), ("metric tail", "metric tail"), ("render_products", "render_products")):
        f, t = res[a + " fused"], res[b + " torch"]
        print("EVALSTEP %s: fused is %.2fx the speed of torch (%s)" % (a, t / f, "faster" if f < t else "NOT faster"))
    two = cams[:2]
    for name, fn in (("evaluate_views fused", lambda: ev.evaluate_views(model, two, bg, fused=True)),
                     ("evaluate_views torch", lambda: ev.evaluate_views(model, two, bg, fused=False)),
                     ("render alone", lambda: [render(cam, model, PIPE, bg) for cam in two]),
                     ("render_products fused", lambda: [None for _ in ev.render_products(model, two, bg, fused=True, copy=False)]),
                     ("render_products torch", lambda: [None for _ in ev.render_products(model, two, bg, fused=False)])):
        with torch.no_grad():
            n = kernel_launches(fn)
        if n is not None:
            print("EVALSTEP launches per view, %-24s %6.1f" % (name, n / len(two)))


if __name__ == "__main__":
    main()
