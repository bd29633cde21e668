"""Time of one frame of the comparison video (gaussianhaircut_amd.comparison), HIP kernels against the torch-composed
comparator on the device and against Pillow on the host, in ONE process on one GPU:

    python tools/cmpstep.py > profiles/comparison_frames.txt

A frame at the sizes run.sh produces: a 576 x 1024 (w x h) Gaussian render, a 1920 x 1920 RGBA strand render and a 2160 x 3840
photograph, to a 1215 x 720 frame.  The forms are ALTERNATED: three rounds, each timing every form once; a form's figure is the
median over its three rounds of the round's median of 20 frames (after 3 warm-up frames the first time a form runs).  Device forms
are timed between two events around one call, inputs already on the device; "with upload and download" is a host clock from a
pinned host photograph to the frame in pinned host memory (the strand render and the Gaussian render are on the device already,
where the preview and the rasterizer leave them).  The host form (only where Pillow imports; 16 threads at the most, which Pillow
does not use) is the script's own sequence: paste over white, three resizes, crop, concatenate.  Launches per frame are counted
by torch.profiler over one call.  The floor is derived, not measured: the bytes each step has to move -- a two-pass resize reads
its input, writes and reads a uint8 intermediate and writes its output -- over 8 TB/s.

--path adds the other two parts of a path frame at small synthetic sizes' cost: one render_products view and one render_strands
picture at the render's size, so that the assembly's share of render + preview + assembly can be stated."""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussianhaircut_amd import comparison as cmp  # noqa: E402

RENDER, PREVIEW, PHOTO, OUT_SHORT = (576, 1024), (1920, 1920), (2160, 3840), 720
ROUNDS, WARMUP, FRAMES = 3, 3, 20
PEAK_BW = 8e12


def host_inputs(seed=0):
    g = np.random.default_rng(seed)

    def image(w, h, c):
        y, x = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
        base = 0.5 + 0.3 * np.sin(0.05 * (x * 0.8 + y * 0.6))
        a = np.clip(np.stack([base * (0.9 - 0.1 * k) for k in range(c)], -1) + 0.05 * g.standard_normal((h, w, c), dtype=np.float32), 0, 1)
        return (a * 255).astype(np.uint8)
    preview = image(*PREVIEW, 4)
    yy, xx = np.meshgrid(np.arange(PREVIEW[1]), np.arange(PREVIEW[0]), indexing="ij")
    preview[:, :, 3] = np.clip(900 - np.hypot(xx - PREVIEW[0] / 2, yy - PREVIEW[1] / 2), 0, 255).astype(np.uint8)   # a disc with a soft edge
    return image(*PHOTO, 3), preview, image(*RENDER, 3)


def resize_bytes(w0, h0, w, h, c=3):
    if (w0, h0) == (w, h):
        return 0
    return c * (w0 * h0 + 2 * h0 * w + w * h)


def frame_bytes(lay):
    over = PREVIEW[0] * PREVIEW[1] * (4 + 3)
    resizes = (resize_bytes(*PREVIEW, lay.preview_w, lay.preview_h) + resize_bytes(*PHOTO, lay.w, lay.h)
               + resize_bytes(3 * lay.w, lay.h, lay.out_w, lay.out_h))
    strip = 2 * 9 * lay.w * lay.h
    return over, resizes, strip


def times_event(fn, n):
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def times_host(fn, n, sync):
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def kernel_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                   and not any(s in e.name.lower() for s in ("memcpy", "memset", "copy")))
    except Exception as exc:   # the count is a by-product: say so rather than lose the timings
        print("CMPSTEP launch count not taken: %r" % (exc,))
        return None


def pillow_frame(photo, preview, render):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_comparison_golden as mk
    return mk.frame(photo, preview, render, OUT_SHORT)


def path_parts(dev):
    """one Gaussian render with its products and one strand picture at the render's size: the rest of a path frame"""
    import math
    from gaussianhaircut_amd import evaluation as ev
    from gaussianhaircut_amd import strand_view as sv
    from gaussianhaircut_amd import visibility as vis
    from gaussianhaircut_amd.scene import ring_cameras
    from gaussianhaircut_amd.utils import synthetic as syn
    W, H = RENDER
    spec = syn.WorkloadSpec("cmpstep_200k", 200_000, W, H, 3, "random", math.log(0.01))
    model, bg = syn.make_model(spec, dev), syn.background(dev)
    cams = ring_cameras(8, W, H, device=dev)
    origins, dirs = syn.strand_polylines(10_000, 99, 5)
    points = (origins + torch.cat([torch.zeros_like(origins), torch.cumsum(dirs, dim=1)], dim=1)).contiguous().to(dev)
    view = vis.view_matrix_from_camera(cams[1])
    render = lambda: list(ev.render_products(model, cams[1:2], bg))        # noqa: E731
    strands = lambda: sv.render_strands(points, view, device=dev)          # noqa: E731
    out = {}
    for name, fn in (("render_products, 200 000 Gaussians", render), ("render_strands, 10 000 strands of 100 points, 2 x 2 supersampled", strands)):
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        out[name] = statistics.median(times_host(fn, FRAMES, True))
    return out


def main():
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    photo, preview, render = host_inputs()
    d_photo, d_preview, d_render = (torch.from_numpy(a).to(dev) for a in (photo, preview, render))
    lay = cmp.comparison_layout(PHOTO, PREVIEW, RENDER, OUT_SHORT)
    out = torch.empty((lay.out_h, lay.out_w, 3), dtype=torch.uint8, device=dev)
    pin_photo = torch.from_numpy(photo).pin_memory()
    pin_frame = torch.empty((lay.out_h, lay.out_w, 3), dtype=torch.uint8).pin_memory()
    d_up = torch.empty_like(d_photo)

    def fused():
        return cmp.comparison_frame(d_photo, d_preview, d_render, OUT_SHORT, fused=True, out=out)

    def composed():
        return cmp.comparison_frame(d_photo, d_preview, d_render, OUT_SHORT, fused=False)

    def fused_io():
        d_up.copy_(pin_photo, non_blocking=True)
        cmp.comparison_frame(d_up, d_preview, d_render, OUT_SHORT, fused=True, out=out)
        pin_frame.copy_(out, non_blocking=True)

    try:
        import PIL
        pil = PIL.__version__
    except ImportError:
        pil = None
    print("CMPSTEP comparison_frame: render %d x %d, strand render %d x %d RGBA, photograph %d x %d -> frame %d x %d (w x h)"
          % (RENDER + PREVIEW + PHOTO + (lay.out_w, lay.out_h)))
    print("CMPSTEP %d rounds, the forms alternated; per round the median of %d frames; the figure is the median of the rounds" % (ROUNDS, FRAMES))
    a, b = fused().clone(), composed()
    print("CMPSTEP fused and comparator agree bit for bit: %s" % torch.equal(a, b))
    if pil:
        print("CMPSTEP fused and Pillow %s agree bit for bit: %s" % (pil, np.array_equal(a.cpu().numpy(), pillow_frame(photo, preview, render))))
    forms = [("fused, inputs on the device", fused, "event", FRAMES), ("fused, with upload and download", fused_io, "host", FRAMES),
             ("comparator on the device", composed, "event", FRAMES)]
    if pil:
        forms.append(("Pillow %s on the host" % pil, lambda: pillow_frame(photo, preview, render), "cpu", 5))
    for name, fn, kind, n in forms:
        for _ in range(WARMUP if kind != "cpu" else 1):
            fn()
    torch.cuda.synchronize()
    rounds = {name: [] for name, _, _, _ in forms}
    for r in range(ROUNDS):
        for name, fn, kind, n in forms:
            ts = times_event(fn, n) if kind == "event" else times_host(fn, n, kind == "host")
            rounds[name].append(statistics.median(ts))
            print("CMPSTEP round %d %-36s median %9.3f ms  (min %9.3f, max %9.3f)  [%d frames]" % (r + 1, name, statistics.median(ts), min(ts), max(ts), n))
    res = {name: statistics.median(v) for name, v in rounds.items()}
    for name, _, _, _ in forms:
        print("CMPSTEP %-44s %9.3f ms per frame" % (name, res[name]))
    over, resizes, strip = frame_bytes(lay)
    floor_ms = (over + resizes + strip) / PEAK_BW * 1e3
    print("CMPSTEP derived, not measured: over white %.1f MB + three resizes %.1f MB + strip %.1f MB = %.1f MB, %.4f ms at %.0f TB/s; "
          "the fused frame reaches %.1f %% of it" % (over / 1e6, resizes / 1e6, strip / 1e6, (over + resizes + strip) / 1e6, floor_ms,
                                                    PEAK_BW / 1e12, 100 * floor_ms / res["fused, inputs on the device"]))
    print("CMPSTEP derived, not measured: the photograph's upload %.1f MB and the frame's download %.1f MB" % (photo.nbytes / 1e6, 3 * lay.out_w * lay.out_h / 1e6))
    for name, fn in (("fused", fused), ("comparator", composed)):
        k = kernel_launches(fn)
        if k is not None:
            print("CMPSTEP launches per frame, %-12s %5d" % (name, k))
    if "--path" in sys.argv:
        parts = path_parts(dev)
        total = sum(parts.values()) + res["fused, with upload and download"]
        for name, ms in parts.items():
            print("CMPSTEP path frame: %-72s %9.3f ms (host clock, synchronised, median of %d)" % (name, ms, FRAMES))
        print("CMPSTEP path frame: the assembly with upload and download is %.1f %% of render + preview + assembly = %.3f ms"
              % (100 * res["fused, with upload and download"] / total, total))
    return 0


if __name__ == "__main__":
    sys.exit(main())
