"""The textured strand generator on one GPU, HIP (csrc/ghr_texstrands.h) against composed (the PyTorch expressions
of gaussianhaircut_amd/strand_generator.py, fused=False) against F.grid_sample, in ONE process:

    python tools/genstep.py check
    python tools/genstep.py time [out-file, default profiles/textured_strands.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ts -- python tools/genstep.py kernels
    python tools/genstep.py guiding [out-file, default profiles/textured_strands_guiding.txt]

``check``: at a small size, both forms against the float64 form under |got - f64| <= 1e-5 max|f64| + 3 |composed - f64|, two
backward passes bit-equal, a permuted draw bit-equal; prints the figures, exits non-zero on a miss.
``time``: at the sizes of the reference's arguments/hair_strands_textured.yaml (Smax 50 000, S 10 000, T 256, C 64 + 65, L 100)
the forms alternate in one call, three rounds; each round's figure is the median of ITERS calls, each timed between two device
events.  Launch counts come from torch.profiler over one call.  The decoders are stand-ins (one linear layer each): their cost is
in every form alike.  The whole latent_strand_training_step is timed with each form of the generator.
``kernels``: the four HIP pieces at the same sizes, ITERS calls each and nothing else: the run a kernel trace is taken of (a call's
time between events includes the host's enqueue, which at these sizes is most of it); its per-kernel times are kept in
profiles/textured_strands_kernels.txt, which ``time`` does not touch.
``guiding``: with num_guiding_strands = 1 000 of the 10 000 drawn, the blend alone (csrc/ghr_guides.h against the
composed form of ``blend_from_guides``), forward and backward, and the whole latent_strand_training_step with the blend in HIP,
with the blend composed and without guiding strands -- alternated in one call as ``time`` alternates its forms."""
import os
import statistics
import sys
from types import SimpleNamespace

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianhaircut_amd import strand_generator as sg  # noqa: E402

SMAX, S, T, CG, CA, L = 50_000, 10_000, 256, 64, 65, 100
ITERS, ROUNDS = 20, 3
COPY_RATE = 6.29e6  # bytes per microsecond: the project's measured copy rate
PIPE = SimpleNamespace(debug=False, fused_projection=True)


def scalp(nu=48, nv=40):
    """a chart of most of a sphere of radius 0.9: (nu x nv) vertices, two triangles a cell"""
    import math
    u, v = torch.meshgrid(torch.linspace(-0.9, 0.9, nu), torch.linspace(-0.9, 0.9, nv), indexing="ij")
    uv = torch.stack([u, v], -1).reshape(-1, 2)
    lon, lat = uv[:, 0] * math.pi, uv[:, 1] * math.pi / 2
    verts = 0.9 * torch.stack([torch.cos(lat) * torch.sin(lon), torch.sin(lat), torch.cos(lat) * torch.cos(lon)], -1)
    faces = []
    for i in range(nu - 1):
        for j in range(nv - 1):
            a, b, c, d = i * nv + j, (i + 1) * nv + j, (i + 1) * nv + j + 1, i * nv + j + 1
            faces += [[a, b, c], [a, c, d]]
    return verts, torch.tensor(faces, dtype=torch.int64), uv


class Decoder(torch.nn.Module):
    def __init__(self, c_in, shape, seed, gain):
        super().__init__()
        self.shape = shape
        n = 1
        for d in shape:
            n *= d
        self.lin = torch.nn.Linear(c_in, n)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            self.lin.weight.copy_(torch.randn(n, c_in, generator=g) * gain)
            self.lin.bias.copy_(torch.randn(n, generator=g) * gain)

    def forward(self, z):
        return self.lin(z).view(z.shape[0], *self.shape)


class GridSampleStrands(sg.TexturedStrands):
    """the same generator with F.grid_sample(float32) for the fetch: the third form"""

    def _strands(self, idx, want_local):
        uv = self.uvs[idx].view(1, 1, -1, 2)
        z = F.grid_sample(self.texture, uv, mode="bilinear", padding_mode="zeros", align_corners=False)[0, :, 0].t()
        z_geom, z_app = z[:, :self.geometry_channels], z[:, self.geometry_channels:]
        out = sg.strands_to_world(self.strand_decoder(z_geom), self.local2world, self.origins, idx, self.scale_decoder, fused=False,
                                  return_local=want_local)
        self.last_idx = idx
        return out, z_geom, z_app


def make_generator(dev, form, sizes=None, seed=7, num_guiding=None):
    smax, s, t, cg, ca, length = sizes or (SMAX, S, T, CG, CA, L)
    target = torch.rand(1, cg, t, t, generator=torch.Generator().manual_seed(seed + 1)).to(dev)
    cls = GridSampleStrands if form == "grid_sample" else sg.TexturedStrands
    gen = cls(scalp(), Decoder(cg, (length - 1, 3), seed + 2, 0.02), Decoder(ca - 1, (49,), seed + 3, 0.1),
              lambda tex: ((tex - target) ** 2).mean(), num_strands=s, max_num_strands=smax, texture_size=t, geometry_channels=cg,
              appearance_channels=ca, scale_decoder=2.0, generator=torch.Generator().manual_seed(seed), fused=(form == "HIP"),
              num_guiding_strands=num_guiding)
    with torch.no_grad():
        gen.texture.copy_(torch.rand(gen.texture.shape, generator=torch.Generator().manual_seed(seed + 4)) * 2 - 1)
    return gen.to(dev)


def timed_median(fn, n):
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def launches(fn):
    """(kernels, of which this package's k_ts_*, fills and copies) of one call"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    moves = sum(1 for e in ev if any(s in e.name.lower() for s in ("memcpy", "memset")))
    own = sum(1 for e in ev if any(s in e.name for s in ("k_ts_", "k_gd_", "k_haar_")))  # (the blend's kernels: csrc/ghr_haar.h)
    return len(ev) - moves, own, moves


def check():
    dev = torch.device("cuda:0")
    sizes = (300, 150, 65, 3, 2, 66)
    ok = True
    gens = {form: make_generator(dev, form, sizes) for form in ("HIP", "composed")}
    g64 = make_generator("cpu", "composed", sizes).double()
    idx = gens["HIP"].draw()
    res = {}
    for form, gen in list(gens.items()) + [("f64", g64)]:
        d = gen.texture.device
        i = idx.to(d)
        z = sg.sample_texture(gen.texture, gen.taps, i, fused=(form == "HIP"))
        p = sg.strands_to_world(gen.strand_decoder(z[:, :3]), gen.local2world, gen.origins, i, 2.0, fused=(form == "HIP"))
        w = torch.linspace(-1, 1, p.numel(), dtype=p.dtype, device=d).view(p.shape)
        (g,) = torch.autograd.grad((p * w).sum() + z[:, 3:].sum(), gen.texture)
        res[form] = dict(z=z.detach().cpu().double(), points=p.detach().cpu().double(), texture_grad=g.cpu().double())
    for k in ("z", "points", "texture_grad"):
        f64, ref = res["f64"][k], (res["composed"][k] - res["f64"][k]).abs()
        err = (res["HIP"][k] - f64).abs()
        good = bool((err <= 1e-5 * f64.abs().max() + 3 * ref).all())
        ok &= good
        print("%-12s HIP %.3e  composed %.3e  max|f64| %.3e  %s" % (k, float(err.max()), float(ref.max()), float(f64.abs().max()),
                                                                    "ok" if good else "MISS"))
    gen = gens["HIP"]
    d_z = torch.randn(idx.shape[0], 5, device=dev)
    grads = []
    for i, dz in ((idx, d_z), (idx, d_z), (idx.flip(0), d_z.flip(0))):
        z = sg.sample_texture(gen.texture, gen.taps, i)
        grads.append(torch.autograd.grad(z, gen.texture, dz)[0])
    same = torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])
    print("two passes and a permuted draw give the same bits: %s" % same)
    return 0 if ok and same else 1


def main_kernels():
    dev = torch.device("cuda:0")
    gen = make_generator(dev, "HIP")
    idx = gen.draw()
    d_z, d_p = torch.randn(S, CG + CA, device=dev), torch.randn(S, L, 3, device=dev)
    v = (torch.randn(S, L - 1, 3, device=dev) * 0.01).requires_grad_(True)
    for _ in range(ITERS):
        z = sg.sample_texture(gen.texture, gen.taps, idx, validate=False)
        torch.autograd.grad(z, gen.texture, d_z)
        p = sg.strands_to_world(v, gen.local2world, gen.origins, idx, 2.0)
        torch.autograd.grad(p, v, d_p)
    torch.cuda.synchronize()


def main_time(out_path):
    dev = torch.device("cuda:0")
    forms = ("HIP", "composed", "grid_sample")
    gens = {form: make_generator(dev, form) for form in forms}
    C = CG + CA
    idx = gens["HIP"].draw()
    d_z = torch.randn(S, C, device=dev)
    tex = gens["HIP"].texture
    taps, uvs = gens["HIP"].taps, gens["HIP"].uvs
    l2w, org = gens["HIP"].local2world, gens["HIP"].origins
    v = (torch.randn(S, L - 1, 3, device=dev) * 0.01).requires_grad_(True)
    d_p = torch.randn(S, L, 3, device=dev)

    def fetch(form):
        if form == "grid_sample":
            return F.grid_sample(tex, uvs[idx].view(1, 1, -1, 2), mode="bilinear", padding_mode="zeros", align_corners=False)[0, :, 0].t()
        return sg.sample_texture(tex, taps, idx, fused=(form == "HIP"), validate=False)

    def world(form):
        return sg.strands_to_world(v, l2w, org, idx, 2.0, fused=(form == "HIP"))

    pieces = {}
    for form in forms:
        z = fetch(form)
        pieces["fetch forward", form] = lambda form=form: fetch(form)
        pieces["fetch backward", form] = lambda z=z: torch.autograd.grad(z, tex, d_z, retain_graph=True)
        if form != "grid_sample":
            p = world(form)
            pieces["to-world forward", form] = lambda form=form: world(form)
            pieces["to-world backward", form] = lambda p=p: torch.autograd.grad(p, v, d_p, retain_graph=True)
    rounds = {k: [] for k in pieces}
    for fn in pieces.values():
        for _ in range(3):
            fn()
    for _ in range(ROUNDS):
        for k, fn in pieces.items():
            rounds[k].append(timed_median(fn, ITERS))
    counts = {k: launches(fn) for k, fn in pieces.items()}
    t_zero = timed_median(lambda: torch.zeros_like(tex), ITERS)

    # the whole latent-strand iteration with each form of the generator
    from gaussianhaircut_amd.gaussian_renderer import render_hair
    from gaussianhaircut_amd.scene.cameras import ring_cameras
    from gaussianhaircut_amd.scene.gaussian_model_latent_strands import GaussianModelLatentStrands
    from gaussianhaircut_amd.trainer import latent_strand_training_step
    from gaussianhaircut_amd.utils import synthetic as syn
    spec = syn.CONFIGS["cfg3"]
    bg = syn.background(dev)
    n_head = 100_000
    head = syn.make_model(spec, dev)
    with torch.no_grad():
        head._label[:n_head] = -4.0
        head._label[n_head:] = 4.0
    head.precompute_head()
    cam = ring_cameras(1, spec.W, spec.H, device=dev)[0]
    opt = SimpleNamespace(lambda_dl1=1.0, lambda_dmask=0.1, lambda_dorient=0.1, lambda_dsds=0.001, use_gt_orient_conf=True,
                          train_orient_conf=True, iterations=10 ** 6, latent_lr=1e-3)
    with torch.no_grad():
        gt = GaussianModelLatentStrands(3, make_generator(dev, "HIP", seed=21), None)
        gt.initialize_gaussians_hair(0)
        pk = render_hair(cam, head, gt, PIPE, bg)
        cam.original_image, cam.original_mask = pk["render"].clamp(0, 1).detach(), pk["mask"].clamp(0, 1).detach()
        cam.original_orient_angle = pk["orient_angle"].detach()
        cam.original_orient_conf = torch.ones_like(pk["orient_conf"]).detach()
        del gt, pk
    steps, it = {}, [0]
    for form in forms:
        hair = GaussianModelLatentStrands(3, gens[form], None)
        hair.training_setup(opt)

        def step(hair=hair):
            it[0] += 1
            latent_strand_training_step(head, hair, [cam], bg, opt, it[0], pipe=PIPE)
        steps[form] = step
    step_rounds = {form: [] for form in forms}
    for fn in steps.values():
        for _ in range(4):
            fn()
    for _ in range(ROUNDS):
        for form, fn in steps.items():
            step_rounds[form].append(timed_median(fn, ITERS))
    step_counts = {form: launches(fn) for form, fn in steps.items()}

    med = statistics.median
    fmt_rounds = lambda xs: " / ".join("%.4f" % x for x in xs)  # noqa: E731
    fmt_count = lambda c: "%d kernels (%d of them k_ts_*) + %d fills and copies" % c  # noqa: E731
    grad_bytes, row_bytes = C * T * T * 4, S * C * 4
    lines = ["textured strand generator: Smax = %d roots, S = %d drawn, T = %d, C = %d + %d, L = %d points per strand" % (SMAX, S, T, CG, CA, L),
             "(sizes of the reference's arguments/hair_strands_textured.yaml; the decoders are one linear layer each: stand-ins, in every",
             " form alike and outside the pieces timed here)",
             "device: %s, torch %s; each round = the median of %d calls, each between two device events; %d alternating rounds" % (
                 torch.cuda.get_device_name(0), torch.__version__, ITERS, ROUNDS),
             "",
             "pieces, ms: median of the rounds | rounds | launches of one call"]
    for (piece, form), xs in rounds.items():
        lines.append("  %-18s %-12s %8.4f | %s | %s" % (piece, form, med(xs), fmt_rounds(xs), fmt_count(counts[piece, form])))
    hip_b, comp_b, gs_b = (med(rounds["fetch backward", f]) for f in forms)
    lines += ["fetch backward: composed / HIP = %.2fx, grid_sample / HIP = %.2fx; the zero fill of a texture gradient alone (the HIP form has"
              % (comp_b / hip_b, gs_b / hip_b),
              "  none: every element is assigned) %.4f ms" % t_zero,
              "DERIVED floor of the fetch backward (not measured): %.1f MB of texture gradient written + %.2f MB of d_z rows read = %.1f us at"
              % (grad_bytes / 1e6, row_bytes / 1e6, (grad_bytes + row_bytes) / COPY_RATE),
              "  the %.2f TB/s copy rate the project's other floors use" % (COPY_RATE / 1e6),
              "",
              "latent_strand_training_step, %d strands x %d segments + %d head Gaussians, 1 view %dx%d, ms per iteration" % (S, L - 1, n_head, spec.W, spec.H)]
    for form in forms:
        lines.append("  generator %-12s median %.3f   rounds %s   launches: %s" % (form, med(step_rounds[form]), fmt_rounds(step_rounds[form]),
                                                                                   fmt_count(step_counts[form])))
    lines += ["the figures above include the host's enqueue of a call, which for the one- and two-launch HIP pieces is most of it; per-kernel",
              "device times come from a kernel trace of `tools/genstep.py kernels`, kept apart in profiles/textured_strands_kernels.txt",
              "not profiled: counters (--pmc); other sizes; real decoders"]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


NG = 1_000  # arguments/hair_strands_textured.yaml: extra_args.num_guiding_strands


def main_guiding(out_path):
    dev = torch.device("cuda:0")
    C, n = CG + CA, L - 1
    base = make_generator(dev, "HIP", num_guiding=NG)
    idx = base.draw()
    uvs = base.uvs[idx].contiguous()
    with torch.no_grad():
        z0 = sg.sample_texture(base.texture, base.taps, idx[:NG], validate=False)
        v0 = base.strand_decoder(z0[:, :CG])
    z_g, v_g = z0.clone().requires_grad_(True), v0.clone().requires_grad_(True)
    d_z = torch.randn(S, C, device=dev)
    forms = ("HIP", "composed")
    pieces = {}
    for form in forms:
        z = sg.blend_from_guides(uvs, z_g, v_g, fused=(form == "HIP"))
        pieces["blend forward", form] = lambda form=form: sg.blend_from_guides(uvs, z_g, v_g, fused=(form == "HIP"))
        pieces["blend backward", form] = lambda z=z: torch.autograd.grad(z, (z_g, v_g), d_z, retain_graph=True)
    rounds = {k: [] for k in pieces}
    for fn in pieces.values():
        for _ in range(3):
            fn()
    for _ in range(ROUNDS):
        for k, fn in pieces.items():
            rounds[k].append(timed_median(fn, ITERS))
    counts = {k: launches(fn) for k, fn in pieces.items()}
    agree = {}
    outs = {form: sg.blend_from_guides(uvs, z_g, v_g, fused=(form == "HIP"), return_state=True) for form in forms}
    agree["nbr"] = bool(torch.equal(outs["HIP"][1]["nbr"], outs["composed"][1]["nbr"]))
    agree["list"] = bool(torch.equal(outs["HIP"][1]["list"], outs["composed"][1]["list"]))
    agree["z"] = float((outs["HIP"][0] - outs["composed"][0]).detach().abs().max())
    lens = (outs["HIP"][1]["start"][1:] - outs["HIP"][1]["start"][:-1]).float()
    del pieces, outs

    # the whole latent-strand iteration: the blend in HIP, the blend composed beside the HIP fetch, no guiding strands
    from gaussianhaircut_amd.gaussian_renderer import render_hair
    from gaussianhaircut_amd.scene.cameras import ring_cameras
    from gaussianhaircut_amd.scene.gaussian_model_latent_strands import GaussianModelLatentStrands
    from gaussianhaircut_amd.trainer import latent_strand_training_step
    from gaussianhaircut_amd.utils import synthetic as syn
    spec = syn.CONFIGS["cfg3"]
    bg = syn.background(dev)
    n_head = 100_000
    head = syn.make_model(spec, dev)
    with torch.no_grad():
        head._label[:n_head] = -4.0
        head._label[n_head:] = 4.0
    head.precompute_head()
    cam = ring_cameras(1, spec.W, spec.H, device=dev)[0]
    opt = SimpleNamespace(lambda_dl1=1.0, lambda_dmask=0.1, lambda_dorient=0.1, lambda_dsds=0.001, use_gt_orient_conf=True,
                          train_orient_conf=True, iterations=10 ** 6, latent_lr=1e-3)
    with torch.no_grad():
        gt = GaussianModelLatentStrands(3, make_generator(dev, "HIP", seed=21), None)
        gt.initialize_gaussians_hair(0)
        pk = render_hair(cam, head, gt, PIPE, bg)
        cam.original_image, cam.original_mask = pk["render"].clamp(0, 1).detach(), pk["mask"].clamp(0, 1).detach()
        cam.original_orient_angle = pk["orient_angle"].detach()
        cam.original_orient_conf = torch.ones_like(pk["orient_conf"]).detach()
        del gt, pk
    gens = {"guiding, blend in HIP": base, "guiding, blend composed": make_generator(dev, "HIP", num_guiding=NG),
            "no guiding strands": make_generator(dev, "HIP")}
    gens["guiding, blend composed"].guides_fused = False
    steps, it = {}, [0]
    for name, gen in gens.items():
        hair = GaussianModelLatentStrands(3, gen, None)
        hair.training_setup(opt)

        def step(hair=hair):
            it[0] += 1
            latent_strand_training_step(head, hair, [cam], bg, opt, it[0], pipe=PIPE)
        steps[name] = step
    step_rounds = {name: [] for name in steps}
    for fn in steps.values():
        for _ in range(4):
            fn()
    for _ in range(ROUNDS):
        for name, fn in steps.items():
            step_rounds[name].append(timed_median(fn, ITERS))
    step_counts = {name: launches(fn) for name, fn in steps.items()}

    med = statistics.median
    fmt_rounds = lambda xs: " / ".join("%.4f" % x for x in xs)  # noqa: E731
    fmt_count = lambda c: "%d kernels (%d of them k_ts_* / k_gd_*) + %d fills and copies" % c  # noqa: E731
    lines = ["guiding strands of the textured generator: S = %d drawn roots of which N = %d guides, n = %d segments, C = %d + %d channels" % (
                 S, NG, n, CG, CA),
             "(sizes of the reference's arguments/hair_strands_textured.yaml; Smax = %d, T = %d; the decoders are one linear layer each)" % (SMAX, T),
             "device: %s, torch %s; each round = the median of %d calls, each between two device events; %d alternating rounds" % (
                 torch.cuda.get_device_name(0), torch.__version__, ITERS, ROUNDS),
             "",
             "the blend alone, ms: median of the rounds | rounds | launches of one call"]
    for (piece, form), xs in rounds.items():
        lines.append("  %-16s %-10s %8.4f | %s | %s" % (piece, form, med(xs), fmt_rounds(xs), fmt_count(counts[piece, form])))
    for piece in ("blend forward", "blend backward"):
        lines.append("%s: composed / HIP = %.2fx" % (piece, med(rounds[piece, "composed"]) / med(rounds[piece, "HIP"])))
    lines += ["the two forms on this draw: nbr equal %s, lists equal %s, max |z HIP - z composed| = %.3e" % (agree["nbr"], agree["list"], agree["z"]),
              "inverted lists: %d choices over %d guides, mean %.1f, longest %d (k_gd_lists ranks each list: work sum L^2 = %.2e compares)" % (
                  4 * S, NG, float(lens.mean()), int(lens.max()), float((lens * lens).sum())),
              "",
              "latent_strand_training_step, %d strands x %d segments + %d head Gaussians, 1 view %dx%d, ms per iteration" % (S, n, n_head, spec.W, spec.H)]
    for name in steps:
        lines.append("  %-26s median %.3f   rounds %s   launches: %s" % (name, med(step_rounds[name]), fmt_rounds(step_rounds[name]),
                                                                        fmt_count(step_counts[name])))
    lines += ["the figures include the host's enqueue of a call; the decoder runs on N and on S - N rows with guiding strands, on S rows without",
              "not profiled: a kernel trace of the k_gd_* kernels; counters (--pmc); other sizes; real decoders"]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "check":
        sys.exit(check())
    if mode == "kernels":
        sys.exit(main_kernels())
    if mode == "guiding":
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        sys.exit(main_guiding(sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "textured_strands_guiding.txt")))
    if mode == "time":
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        main_time(sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "textured_strands.txt"))
    else:
        sys.exit(__doc__)
