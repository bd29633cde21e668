"""Time of the head-mesh distance query (gaussianhaircut_amd.mesh.HeadMesh.closest_point) and of the strand-stage
iteration with the collision term, in ONE process on one GPU:

    python tools/meshdiststep.py [out-file, default profiles/mesh_distance.txt]

The query: 30 000 strands of 100 points grown from a UV sphere of 9976 faces (116 x 44: the face count of the reference's head
mesh, which is not redistributable; the cloud of tools/strandviewstep.py) against that sphere.
  fused     closest_point(fused=True): ghr_knn_keys, the key sort, k_meshdist_search -- the call as a caller makes it;
  search    ghr_mesh_closest alone on keys sorted before;
  composed  closest_point(fused=False) over MESHDISTSTEP_COMPOSED_QUERIES queries drawn at random (default 4096: a brute force
            over all faces), extrapolated linearly in Q -- marked as such.
The forms alternate in one call, three rounds; each figure is the device time between two events; the results of the forms are
compared for equality before anything is timed.  With a library built with -DGHR_MD_COUNT_BLOCKS
(tools/build_variant.sh mdcount -DGHR_MD_COUNT_BLOCKS; GHR_LIB_PATH=build/variants/libghr_mdcount.so; it exports
ghr_meshdist_read_counters, the product does not) the run prints the mean number of face blocks a wave scanned and of faces it
evaluated (those that passed the ballot on their own box).  The arithmetic
estimate beside the figures is DERIVED (instruction counts from the source), not measured.

The iteration: strand_training_step at the strand stage's size (tools/sdsstep.py's scene: 30 000 strands x 99 segments, 100 000
head Gaussians, one view) without the term, and with HeadCollision at stride 1 and 4 against the same sphere; launch counts from
torch.profiler over one call."""
import ctypes
import os
import statistics
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianhaircut_amd import _lib  # noqa: E402
from gaussianhaircut_amd.mesh import HeadMesh  # noqa: E402
from gaussianhaircut_amd.simple_knn import _C as _knn  # noqa: E402
from gaussianhaircut_amd.strand_collision import HeadCollision  # noqa: E402
from tests import mesh_cases as mc  # noqa: E402
from tests import strand_view_cases as sc  # noqa: E402

ROUNDS, ITERS = 3, 10
PIPE = SimpleNamespace(debug=False, fused_projection=True)
VALU_RATE = 256 * 64 * 2.4e9   # lane-instructions per second: 256 CUs x 64 lanes at 2.4 GHz, unpacked, no FMA (contraction is off)
PAIR_INSTR = 290               # counted from md_face: 3 edges x 45 + interior 95 + 4 divisions x ~12 + the take
BOUND_INSTR = 35               # a face's own box and its bound, per (query, face) pair of a scanned block: 12 min / max, 23 for the bound and the vote


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
    """(kernels, of which k_meshdist_*, fills and copies) of one call"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    moves = sum(1 for e in ev if any(s in e.name.lower() for s in ("memcpy", "memset")))
    own = sum(1 for e in ev if "k_meshdist_" in e.name)
    return len(ev) - moves, own, moves


def main():
    assert torch.cuda.is_available(), "meshdiststep needs a ROCm GPU (a CPU run measures nothing)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "mesh_distance.txt")
    dev = torch.device("cuda:0")
    S, L = int(os.environ.get("MESHDISTSTEP_STRANDS", 30000)), int(os.environ.get("MESHDISTSTEP_POINTS", 100))
    n_cmp = int(os.environ.get("MESHDISTSTEP_COMPOSED_QUERIES", 4096))
    do_step = os.environ.get("MESHDISTSTEP_ITERATION", "1") != "0"
    v, f = mc.uv_sphere(116, 44)
    mesh = HeadMesh(v, f)
    pts = torch.from_numpy(sc.hair(S, L, 1, through=False)).to(dev).reshape(-1, 3).contiguous()
    Q = pts.shape[0]
    lines = ["head-mesh closest point: Q = %d points (%d strands x %d) against a UV sphere of %d faces (%d blocks of 64)"
             % (Q, S, L, len(f), (len(f) + 63) // 64),
             "device: %s, torch %s; device time between two events, %d alternating rounds" % (torch.cuda.get_device_name(0), torch.__version__, ROUNDS)]

    got = mesh.closest_point(pts)
    sub = torch.randperm(Q, generator=torch.Generator().manual_seed(2))[:n_cmp].to(dev)
    want = mesh.closest_point(pts[sub], fused=False)
    assert all(torch.equal(a[sub].view(torch.int32) if a.dtype == torch.float32 else a[sub], b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(got, want)), "the forms disagree"
    lines.append("MEASURED: the forms give the same bits on %d of the queries (dist2, face, point)" % n_cmp)

    blob, bounds = mesh._tris_tables(dev)
    srt = _knn.sort_keys(_knn.keys(pts, bounds))
    out = (torch.empty(Q, device=dev), torch.empty(Q, dtype=torch.int32, device=dev), torch.empty(Q, 3, device=dev))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L_ = _lib.lib()

    def search_only():
        _lib.check(L_.ghr_mesh_closest(stream, ctypes.byref(mesh._tris_header), ptr(blob), Q, ptr(pts), ptr(srt.indices), ptr(srt.values),
                                       ptr(out[0]), ptr(out[1]), ptr(out[2])))

    forms = {"fused": (lambda: mesh.closest_point(pts), ITERS), "search": (search_only, ITERS),
             "composed": (lambda: mesh.closest_point(pts[sub], fused=False), 1)}
    rounds = {k: [] for k in forms}
    for fn, _ in forms.values():
        fn()
    for _ in range(ROUNDS):
        for k, (fn, n) in forms.items():
            rounds[k].append(timed(fn, n))
    med = statistics.median
    fmt = lambda xs: " / ".join("%.3f" % x for x in xs)  # noqa: E731
    for k in forms:
        lines.append("MEASURED: %-8s median %.3f ms   rounds %s%s" % (k, med(rounds[k]), fmt(rounds[k]),
                                                                      "   (over %d queries)" % n_cmp if k == "composed" else ""))
    extrapolated = med(rounds["composed"]) * Q / n_cmp
    lines.append("DERIVED (extrapolated linearly from %d queries): composed over all %d queries %.1f ms; composed / fused = %.0fx"
                 % (n_cmp, Q, extrapolated, extrapolated / med(rounds["fused"])))
    c = (ctypes.c_uint64 * 3)()
    nb = (len(f) + 63) // 64
    if hasattr(L_, "ghr_meshdist_read_counters"):
        L_.ghr_meshdist_read_counters(c)   # zero
        search_only()
        _lib.check(L_.ghr_meshdist_read_counters(c))
        blocks, faces = c[0] / max(c[1], 1), c[2] / max(c[1], 1)
        lines.append("MEASURED (counting build: its times above are not the product's): per wave of 64 queries %.2f face blocks scanned of %d, "
                     "%.1f faces evaluated of the %.0f in them (%d waves)" % (blocks, nb, faces, blocks * 64, c[1]))
        floor = Q * (faces * PAIR_INSTR + blocks * 64 * BOUND_INSTR) / VALU_RATE * 1e3
        lines.append("DERIVED arithmetic estimate: %d lane-instructions per evaluated (query, face) pair (counted from md_face's source, contraction "
                     "off) and %d per pair of a scanned block for the face's own bound, at %.3g lane-instructions/s (256 CUs x 64 lanes x 2.4 "
                     "GHz): %.3f ms" % (PAIR_INSTR, BOUND_INSTR, VALU_RATE, floor))
    else:
        lines.append("(no counting build loaded: blocks and faces per wave not measured in this run; the DERIVED floor needs them)")

    if do_step:
        from gaussianhaircut_amd.gaussian_renderer import render_hair
        from gaussianhaircut_amd.scene.cameras import ring_cameras
        from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams
        from gaussianhaircut_amd.scene.gaussian_model_strands import GaussianModelStrands
        from gaussianhaircut_amd.trainer import strand_training_step
        from gaussianhaircut_amd.utils import synthetic as syn
        SEG = 99
        g = torch.Generator().manual_seed(9)
        unit = torch.nn.functional.normalize
        dirs = (torch.randn(S, SEG, 3, generator=g) * 0.003 + unit(torch.randn(S, 1, 3, generator=g), dim=-1) * 0.01).to(dev)
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
        steps, it = {}, [0]
        for name, stride in (("without the term", None), ("with the term, stride 1", 1), ("with the term, stride 4", 4)):
            opt = OptimizationParams()
            opt.lambda_dorient, opt.lambda_dmask = 0.1, 0.1
            hair = GaussianModelStrands(3).create_from_strands(origins.to(dev), dirs, feats.to(dev))
            if stride is None:
                with torch.no_grad():
                    hair.initialize_gaussians_hair()
                    p = render_hair(cam, head, hair, PIPE, bg)
                    cam.original_image, cam.original_mask = p["render"].clamp(0, 1).detach(), p["mask"].clamp(0, 1).detach()
                    cam.original_orient_angle = p["orient_angle"].detach()
                    cam.original_orient_conf = torch.ones_like(p["orient_conf"]).detach()
                    del p
            else:
                opt.lambda_dpen = 0.1
                hair.attach_collision(HeadCollision(mesh, margin=0.005, stride=stride))
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
            lines.append("  %-26s median %.3f   rounds %s   launches: %d kernels (%d of them k_meshdist_*) + %d fills and copies"
                         % ((name, med(step_rounds[name]), fmt(step_rounds[name])) + launches(fn)))
        base = med(step_rounds["without the term"])
        lines.append("  the term costs %.3f ms (stride 1, %d points) / %.3f ms (stride 4, %d points) of the iteration"
                     % (med(step_rounds["with the term, stride 1"]) - base, S * SEG, med(step_rounds["with the term, stride 4"]) - base,
                        S * len(range(0, SEG, 4))))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
