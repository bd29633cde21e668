"""Time of the strand shape term (gaussianhaircut_amd.strand_shape.StrandShape) and of the strand-stage iteration
with it, in ONE process on one GPU:

    python tools/shapestep.py [out-file, default profiles/strand_shape.txt]

The workload is tools/meshdiststep.py's iteration scene: 30 000 strands x 99 segments with their roots on the unit sphere,
100 000 head Gaussians, one view.
  the term alone   forward + backward of ``shape(dirs)``, fused (ghr_shape_forward / ghr_shape_backward) against composed (the
                   PyTorch form, which gathers dirs[nbr] as [S, 4, n, 3]); the neighbour search (once per model) on its own;
  the iteration    strand_training_step without the term, with it fused, with it composed; launch counts from torch.profiler.
The forms alternate in one call, three rounds; each figure is the device time between two events.  The traffic floors beside the
figures are DERIVED: forward 12 S n (1 + K) bytes, backward 12 S n (2 + 2K) bytes on average, at 6.29 TB/s."""
import os
import statistics
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianhaircut_amd import strand_shape as ss  # noqa: E402

ROUNDS, ITERS = 3, 10
PIPE = SimpleNamespace(debug=False, fused_projection=True)
HBM = 6.29e12  # bytes per second, the figure the other floors use
K = 4


def timed(fn, n=1):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def launches(fn):
    """(kernels, of which k_shape_*, fills and copies) of one call"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    moves = sum(1 for e in ev if any(s in e.name.lower() for s in ("memcpy", "memset")))
    own = sum(1 for e in ev if "k_shape_" in e.name)
    return len(ev) - moves, own, moves


def main():
    assert torch.cuda.is_available(), "shapestep needs a ROCm GPU (a CPU run measures nothing)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "strand_shape.txt")
    dev = torch.device("cuda:0")
    S, SEG = int(os.environ.get("SHAPESTEP_STRANDS", 30000)), int(os.environ.get("SHAPESTEP_SEGMENTS", 99))
    do_step = os.environ.get("SHAPESTEP_ITERATION", "1") != "0"
    g = torch.Generator().manual_seed(9)
    unit = torch.nn.functional.normalize
    dirs = (torch.randn(S, SEG, 3, generator=g) * 0.003 + unit(torch.randn(S, 1, 3, generator=g), dim=-1) * 0.01).to(dev)
    origins = unit(torch.randn(S, 1, 3, generator=g), dim=-1).to(dev)
    med = statistics.median
    fmt = lambda xs: " / ".join("%.3f" % x for x in xs)  # noqa: E731
    spread = lambda xs: (max(xs) - min(xs)) / med(xs) * 100  # noqa: E731
    lines = ["strand shape term: %d strands x %d segments, K = %d neighbours over the roots" % (S, SEG, K),
             "device: %s, torch %s; device time between two events, %d alternating rounds" % (torch.cuda.get_device_name(0), torch.__version__, ROUNDS)]

    fused, composed = ss.StrandShape(origins, dirs, fused=True), ss.StrandShape(origins, dirs, fused=False)
    same = all(torch.equal(getattr(fused, k), getattr(composed, k)) for k in ("nbr", "start", "list"))
    lines.append("MEASURED: the HIP neighbour search and the composed one give %s tables (nbr, start, list); M = %d valid pairs"
                 % ("the same" if same else "DIFFERENT", fused.M))
    assert same
    param = dirs.clone().requires_grad_(True)

    def fwd_bwd(shape):
        param.grad = None
        shape(param).backward()

    with torch.no_grad():
        ef, ec = fused.terms(dirs), composed.terms(dirs)
    lines.append("MEASURED: E fused %s, composed %s" % (["%.9g" % x for x in ef.tolist()], ["%.9g" % x for x in ec.tolist()]))
    forms = {"fused fwd+bwd": (lambda: fwd_bwd(fused), ITERS), "composed fwd+bwd": (lambda: fwd_bwd(composed), ITERS),
             "fused fwd": (lambda: fused.terms(dirs), ITERS), "composed fwd": (lambda: composed.terms(dirs), ITERS),
             "neighbours HIP": (lambda: ss.nearest_roots(origins, None, fused=True), 2),
             "neighbours composed": (lambda: ss.nearest_roots(origins, None, fused=False), 1)}
    rounds = {k: [] for k in forms}
    for fn, _ in forms.values():
        fn()
    for _ in range(ROUNDS):
        for k, (fn, n) in forms.items():
            rounds[k].append(timed(fn, n))
    for k in forms:
        lines.append("MEASURED: %-20s median %.3f ms   rounds %s   spread %.1f %%" % (k, med(rounds[k]), fmt(rounds[k]), spread(rounds[k])))
    f_fwd, f_all = med(rounds["fused fwd"]), med(rounds["fused fwd+bwd"])
    floor_f, floor_b = 12.0 * S * SEG * (1 + K) / HBM * 1e3, 12.0 * S * SEG * (2 + 2 * K) / HBM * 1e3
    lines.append("MEASURED: composed / fused = %.1fx (fwd+bwd), %.1fx (fwd)" % (med(rounds["composed fwd+bwd"]) / f_all, med(rounds["composed fwd"]) / f_fwd))
    lines.append("DERIVED traffic floor at %.2f TB/s: forward 12 S n (1 + K) B = %.1f MB -> %.4f ms; backward 12 S n (2 + 2K) B = %.1f MB -> %.4f ms"
                 % (HBM / 1e12, 12.0 * S * SEG * (1 + K) / 1e6, floor_f, 12.0 * S * SEG * (2 + 2 * K) / 1e6, floor_b))
    lines.append("  the fused forward runs at %.0f %% of its floor, forward + backward at %.0f %% of the two floors' sum (the rows fit the caches: "
                 "the floor counts every byte as if it came from HBM)" % (floor_f / f_fwd * 100, (floor_f + floor_b) / f_all * 100))
    lines.append("  launches of one fused forward + backward: %d kernels (%d of them k_shape_*) + %d fills and copies" % launches(lambda: fwd_bwd(fused)))
    lines.append("  launches of one composed forward + backward: %d kernels + %d fills and copies" % launches(lambda: fwd_bwd(composed))[::2])

    if do_step:
        from gaussianhaircut_amd.gaussian_renderer import render_hair
        from gaussianhaircut_amd.scene.cameras import ring_cameras
        from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
        from gaussianhaircut_amd.scene.gaussian_model_strands import GaussianModelStrands
        from gaussianhaircut_amd.trainer import strand_training_step
        from gaussianhaircut_amd.utils import synthetic as syn
        spec = syn.CONFIGS["cfg3"]
        bg = syn.background(dev)
        n_head = 100_000
        head = syn.make_model(spec, dev)
        with torch.no_grad():
            head._label[:n_head] = -4.0
            head._label[n_head:] = 4.0
        head.precompute_head()
        feats = (torch.randn(S * SEG, 16, 3, generator=g) * 0.1).to(dev)
        cam = ring_cameras(1, spec.W, spec.H, device=dev)[0]
        steps, it = {}, [0]
        for name, form in (("without the term", None), ("with the term, fused", True), ("with the term, composed", False)):
            opt = OptimizationParams()
            opt.lambda_dorient, opt.lambda_dmask = 0.1, 0.1
            hair = GaussianModelStrands(3).create_from_strands(origins, dirs, feats)
            if form is None:
                with torch.no_grad():
                    hair.initialize_gaussians_hair()
                    p = render_hair(cam, head, hair, PIPE, bg)
                    cam.original_image, cam.original_mask = p["render"].clamp(0, 1).detach(), p["mask"].clamp(0, 1).detach()
                    cam.original_orient_angle = p["orient_angle"].detach()
                    cam.original_orient_conf = torch.ones_like(p["orient_conf"]).detach()
                    del p
            else:
                opt.lambda_dshape = 0.1
                hair.attach_shape(fused if form else composed)
            with torch.no_grad():
                hair._dirs.mul_(1.02)
            hair.training_setup(opt)

            def step(hair=hair, opt=opt):
                it[0] += 1
                strand_training_step(head, hair, [cam], bg, opt, it[0], pipe=PIPE)
            steps[name] = step
        step_rounds = {name: [] for name in steps}
        for fn in steps.values():
            timed(fn, 4)
        for _ in range(ROUNDS):
            for name, fn in steps.items():
                step_rounds[name].append(timed(fn, 2 * ITERS))
        lines += ["", "strand_training_step, %d strands x %d segments + %d head Gaussians, 1 view %dx%d, ms per iteration (MEASURED)"
                  % (S, SEG, n_head, spec.W, spec.H)]
        for name, fn in steps.items():
            lines.append("  %-26s median %.3f   rounds %s   spread %.1f %%   launches: %d kernels (%d of them k_shape_*) + %d fills and copies"
                         % ((name, med(step_rounds[name]), fmt(step_rounds[name]), spread(step_rounds[name])) + launches(fn)))
        base = med(step_rounds["without the term"])
        lines.append("  the term costs %.3f ms fused / %.3f ms composed of the iteration"
                     % (med(step_rounds["with the term, fused"]) - base, med(step_rounds["with the term, composed"]) - base))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
