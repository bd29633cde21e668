"""Time of the strand stage's prior block, forward + backward, HIP (csrc/ghr_sds.h) against composed (the PyTorch
expressions of gaussianhaircut_amd/strand_prior.py, fused=False), in ONE process on one GPU:

    python tools/sdsstep.py [out-file, default profiles/sds_texture.txt]

The block: draw N guiding strands, local frames, encoder, latent texture, prior loss, and the backward into a dense d_dirs.  The
forms alternate in one call, three rounds; each figure is the device time between two events over ITERS calls, and the medians of
the rounds are printed with their spread.  Launch counts come from torch.profiler over one call (device kernel events; fills and
copies are counted apart, and the kernels of csrc/ghr_sds.h are counted by name inside each trace).  The whole strand_training_step is timed with and without the term at the bench's strand-stage size.

Size: S = 30 000 strands, N = 1000 guiding strands, n = 99 segments, C = 64 channels, G = 32.  G = 32 is THIS PROJECT'S ASSUMPTION about
NeuralHaircut's `diffusion_input`: that code is not vendored and was not available when this was written.  The encoder is a
stand-in (one linear layer and tanh), the prior's loss a stand-in (quadratic towards a fixed texture): their cost is in both forms
alike and is also reported alone."""
import os
import statistics
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianhaircut_amd import strand_prior as sp  # noqa: E402

S, N, SEG, C, G = 30_000, 1000, 99, 64, 32
ITERS, ROUNDS = 20, 3
PIPE = SimpleNamespace(debug=False, fused_projection=True)


def timed(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def launches(fn):
    """(kernels, of which this package's k_sds_*, fills and copies) of one call"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    moves = sum(1 for e in ev if any(s in e.name.lower() for s in ("memcpy", "memset")))
    own = sum(1 for e in ev if "k_sds_" in e.name or "k_haar_" in e.name)  # (the texture's kernels: csrc/ghr_haar.h)
    return len(ev) - moves, own, moves


def make_prior(dev, fused, seed=5):
    g = torch.Generator().manual_seed(seed)
    uvs = (torch.rand(S, 2, generator=g) * 2 - 1).to(dev)
    q, _ = torch.linalg.qr(torch.randn(S, 3, 3, generator=g))
    W = (torch.randn(3 * (SEG + 1), C, generator=g) * 0.004).to(dev)
    T0 = (torch.rand(1, C, G, G, generator=g) * 2 - 1).to(dev)
    return sp.StrandPrior(lambda e: torch.tanh(e.flatten(1) @ W), lambda t: ((t - T0) ** 2).mean(dim=(1, 2, 3)), uvs, q.to(dev), G, 50.0,
                          num_guiding=N, channels=C, generator=torch.Generator(device=dev).manual_seed(seed), fused=fused), W, T0


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "sds_texture.txt")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(9)
    unit = torch.nn.functional.normalize
    dirs = (torch.randn(S, SEG, 3, generator=g) * 0.003 + unit(torch.randn(S, 1, 3, generator=g), dim=-1) * 0.01).to(dev).requires_grad_(True)
    priors = {name: make_prior(dev, fused)[0] for name, fused in (("fused", True), ("composed", False))}
    _, W, T0 = make_prior(dev, True)

    def block(name):
        def fn():
            dirs.grad = None
            priors[name](dirs).backward()
        return fn

    def stand_ins():  # the encoder and the loss alone, forward + backward, on tensors of the block's shapes
        e = torch.zeros(N, SEG + 1, 3, device=dev, requires_grad=True)
        z = torch.tanh(e.flatten(1) @ W)
        tex = z.t().reshape(1, C, 1, N)[..., :G].expand(1, C, G, G)
        (((tex - T0) ** 2).mean() + z.sum()).backward()

    def add36():  # the dense add autograd performs to join d_dirs with the rasterizer's gradient of the same parameter
        return a36 + b36
    a36, b36 = torch.zeros(S, SEG, 3, device=dev), torch.zeros(S, SEG, 3, device=dev)
    rounds = {"fused": [], "composed": []}
    for name in rounds:
        timed(block(name), 3)
    for _ in range(ROUNDS):
        for name in rounds:
            rounds[name].append(timed(block(name), ITERS))
    count = {name: launches(block(name)) for name in rounds}
    t_stand, t_add, t_zero = timed(stand_ins, ITERS), timed(add36, ITERS), timed(lambda: torch.zeros_like(a36), ITERS)
    count_stand = launches(stand_ins)

    # the pieces of the HIP form through their autograd functions
    idx = priors["fused"].draw(S, dev)
    w2l, uvg = priors["fused"].world2local, priors["fused"].uvs[idx]
    e, v = sp.guiding_strands_local(dirs, w2l, idx, 50.0, frames_are_inverse=True)
    z = torch.tanh(e.flatten(1) @ W).detach().requires_grad_(True)
    vd = v.detach().requires_grad_(True)
    tex = sp.latent_texture(uvg, z, vd, G)
    ce, cv, ct = torch.randn_like(e), torch.randn_like(v), torch.randn_like(tex)
    parts = {}
    for key, fn in (("local frame fwd", lambda: sp.guiding_strands_local(dirs, w2l, idx, 50.0, frames_are_inverse=True)),
                    ("local frame bwd (sort, fill, kernel)", lambda: torch.autograd.grad((e, v), dirs, (ce, cv), retain_graph=True)),
                    ("texture fwd", lambda: sp.latent_texture(uvg, z, vd, G)),
                    ("texture bwd", lambda: torch.autograd.grad(tex, (z, vd), ct, retain_graph=True))):
        timed(fn, 3)
        parts[key] = (timed(fn, ITERS), launches(fn))

    # the whole strand-stage iteration, with and without the term
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
    origins = unit(torch.randn(S, 1, 3, generator=g), dim=-1)
    feats = torch.randn(S * SEG, 16, 3, generator=g) * 0.1
    cam = ring_cameras(1, spec.W, spec.H, device=dev)[0]
    opt = OptimizationParams()
    opt.lambda_dorient, opt.lambda_dmask, opt.lambda_dsds = 0.1, 0.1, 0.01
    steps, it = {}, [0]
    for name in ("without the term", "with the term, HIP", "with the term, composed"):
        hair = GaussianModelStrands(3).create_from_strands(origins.to(dev), dirs.detach(), feats.to(dev))
        if name == "without the term":
            with torch.no_grad():
                hair.initialize_gaussians_hair()
                p = render_hair(cam, head, hair, PIPE, bg)
                cam.original_image, cam.original_mask = p["render"].clamp(0, 1).detach(), p["mask"].clamp(0, 1).detach()
                cam.original_orient_angle = p["orient_angle"].detach()
                cam.original_orient_conf = torch.ones_like(p["orient_conf"]).detach()
                del p
        else:
            hair.attach_prior(priors["fused" if name.endswith("HIP") else "composed"])
        with torch.no_grad():
            hair._dirs.mul_(1.02)
        hair.training_setup(opt)

        def step(hair=hair):
            it[0] += 1
            strand_training_step(head, hair, [cam], bg, opt, it[0], pipe=PIPE)
        steps[name] = step
    step_rounds = {name: [] for name in steps}
    for name, fn in steps.items():
        timed(fn, 4)
    for _ in range(ROUNDS):
        for name, fn in steps.items():
            step_rounds[name].append(timed(fn, ITERS))
    step_count = {name: launches(fn) for name, fn in steps.items()}

    med = lambda xs: statistics.median(xs)  # noqa: E731
    fmt_rounds = lambda xs: " / ".join("%.3f" % x for x in xs)  # noqa: E731
    fmt_count = lambda c: "%d kernels (%d of them k_sds_*) + %d fills and copies" % c  # noqa: E731
    in_bytes = N * SEG * 12 + N * 36 + N * 8          # the drawn strands' segments, frames, indices
    mid_bytes = 2 * (N * (SEG + 1) * 12 + N * SEG * 12) + 2 * N * C * 4 + 2 * C * G * G * 4 + 2 * 4 * G * G * 8
    dense_bytes = S * SEG * 12
    floor_us = (2 * in_bytes + mid_bytes + dense_bytes) / 6.29e6   # the project's measured copy rate, 6.29 TB/s
    lines = ["strand prior block, forward + backward: S = %d strands, N = %d guiding, n = %d segments, C = %d, G = %d" % (S, N, SEG, C, G),
             "(G = 32 is this project's assumption about NeuralHaircut's diffusion_input: that code is not vendored; the encoder is one",
             " linear layer + tanh, the prior's loss quadratic: stand-ins, in both forms alike)",
             "device: %s, torch %s; device time between two events over %d calls, %d alternating rounds" % (
                 torch.cuda.get_device_name(0), torch.__version__, ITERS, ROUNDS),
             "",
             "block  HIP      median %.3f ms   rounds %s   launches: %s" % (med(rounds["fused"]), fmt_rounds(rounds["fused"]), fmt_count(count["fused"])),
             "block  composed median %.3f ms   rounds %s   launches: %s" % (med(rounds["composed"]), fmt_rounds(rounds["composed"]),
                                                                            fmt_count(count["composed"])),
             "composed / HIP = %.2fx" % (med(rounds["composed"]) / med(rounds["fused"])),
             "the stand-in encoder and loss with their backward, alone, on a graph of their own (not the block's: its counts differ by a",
             " few kernels from what they are inside the block): %.3f ms (%s)" % (t_stand, fmt_count(count_stand)),
             "",
             "pieces of the HIP form, ms (mean of %d) and launches" % ITERS]
    for key, (t, c) in parts.items():
        lines.append("  %-38s %8.4f   %s" % (key, t, fmt_count(c)))
    lines += ["the dense d_dirs [S, n, 3] = %.1f MB: its zero fill %.4f ms, the add that joins it to the rasterizer's gradient %.4f ms" % (
                  dense_bytes / 1e6, t_zero, t_add),
              "DERIVED floor (not measured): %.2f MB of guiding-strand inputs read twice, %.2f MB between the kernels, %.1f MB dense gradient"
              % (in_bytes / 1e6, mid_bytes / 1e6, dense_bytes / 1e6),
              "  written once = %.1f us at the 6.29 TB/s copy rate the project's other floors use; the block is launch-bound, not bandwidth-bound" % floor_us,
              "",
              "strand_training_step, %d strands x %d segments + %d head Gaussians, 1 view %dx%d, ms per iteration" % (S, SEG, n_head, spec.W, spec.H)]
    for name in steps:
        lines.append("  %-26s median %.3f   rounds %s   launches: %s" % (name, med(step_rounds[name]), fmt_rounds(step_rounds[name]),
                                                                         fmt_count(step_count[name])))
    base = med(step_rounds["without the term"])
    lines.append("  the term costs %.3f ms (HIP) / %.3f ms (composed) of the iteration" % (
        med(step_rounds["with the term, HIP"]) - base, med(step_rounds["with the term, composed"]) - base))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
