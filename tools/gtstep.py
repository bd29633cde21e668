"""Time of the ground-truth loader per view, HIP kernels against the torch-composed comparator on the device and against
Pillow + the loadCam tail on the host (gaussianhaircut_amd.ground_truth, fused=True / fused=False), in ONE process on one GPU:

    python tools/gtstep.py > profiles/ground_truth_loader.txt

A view is a 2160 x 3840 (w x h) uint8 RGB image, two uint8 masks, the uint8 angle map and the float16 variance map; it is taken
to ``// 2`` and ``// 4`` by ``view_ground_truth``: four resizes (two launches each), one assembly launch.  Device figures are the
MEDIAN device time between two events around one call, over 20 calls after 3 warm-up calls of that form and size, inputs already
on the device.  "with upload" is a host clock from pageable host arrays to a device synchronise after the last launch, same
counts.  The host form (only where Pillow imports; torch limited to 16 threads) is Image.resize for the four 8-bit inputs,
F.interpolate for the variance and the same tail in torch on the CPU, host clock.  Launches per view are counted by
torch.profiler over one call (device kernel events; copies excluded).  The floor is derived, not measured: the bytes a resize
has to move -- input + uint8 intermediate (written and read) + output -- and the assembly's inputs + outputs, over 8 TB/s.

Per-kernel times come from a run of their own, in a fresh child process under the profiler:

    python tools/gtstep.py --rocprof       # rocprofv3 --kernel-trace --stats -- python tools/gtstep.py --kernels
"""
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussianhaircut_amd import ground_truth as gt  # noqa: E402

W0, H0 = 2160, 3840
FACTORS = (2, 4)
WARMUP, CALLS = 3, 20
PEAK_BW = 8e12
NAMES = ("image", "mask_hair", "mask_body", "angle", "var")


def host_view(seed=0):
    g = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H0, dtype=np.float32), np.arange(W0, dtype=np.float32), indexing="ij")
    base = 0.5 + 0.3 * np.sin(0.2 * (x * 0.8 + y * 0.6))
    image = (np.clip(np.stack([base * 0.9, base * 0.7, base * 0.5], -1) + 0.05 * g.standard_normal((H0, W0, 3), dtype=np.float32), 0, 1) * 255).astype(np.uint8)
    disc = np.clip(600 - 0.5 * np.hypot(x - W0 / 2, y - H0 / 2), 0, 255).astype(np.uint8)
    return dict(image=image, mask_hair=disc, mask_body=np.maximum(disc, 60).astype(np.uint8),
                angle=g.integers(0, 180, (H0, W0)).astype(np.uint8), var=(g.random((H0, W0), dtype=np.float32) * 2).astype(np.float16))


def resize_bytes(w0, h0, c, w, h):
    """input + intermediate (written, then read) + output of one two-pass resize"""
    return c * (w0 * h0 + 2 * h0 * w + w * h)


def view_bytes(f):
    w, h = W0 // f, H0 // f
    resizes = resize_bytes(W0, H0, 3, w, h) + 3 * resize_bytes(W0, H0, 1, w, h)
    assemble = w * h * (3 + 3) + 4 * W0 * H0 + 4 * 7 * w * h   # the resized bytes and the variance map (as float32) in, 7 planes out
    return resizes, assemble


def median_event_ms(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def median_host_ms(fn, sync, warmup=WARMUP, calls=CALLS):
    for _ in range(warmup):
        fn()
    if sync:
        torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def kernel_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                   and not any(s in e.name.lower() for s in ("memcpy", "memset", "copy")))
    except Exception as exc:   # the count is a by-product: say so rather than lose the timings
        print("GTSTEP launch count not taken: %r" % (exc,))
        return None


def host_form(view, w, h):
    """Pillow + the loadCam tail on the host, as the reference runs it"""
    from PIL import Image
    small = [torch.from_numpy(np.array(Image.fromarray(view[n]).resize((w, h)))) for n in NAMES[:4]]
    return gt._assemble_torch(*small, torch.from_numpy(view["var"]), False, False, True)


def kernels_only():
    """what the profiled child runs: five fused calls per factor"""
    dev = torch.device("cuda:0")
    view = {k: torch.from_numpy(v).to(dev) for k, v in host_view().items()}
    for f in FACTORS:
        for _ in range(5):
            gt.view_ground_truth(*(view[n] for n in NAMES), resolution=(W0 // f, H0 // f), fused=True)
        torch.cuda.synchronize()


def rocprof():
    out = tempfile.mkdtemp(prefix="gtstep_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "gt", "--",
           sys.executable, os.path.abspath(__file__), "--kernels"]
    res = subprocess.run(cmd, cwd=out, capture_output=True, text=True, timeout=600)
    if res.returncode != 0:
        print("GTSTEP rocprofv3 failed (%d): %s" % (res.returncode, (res.stdout + res.stderr)[-2000:]))
        return 1
    traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    if not traces:
        print("GTSTEP rocprofv3 wrote no kernel trace under %s" % out)
        return 1
    per = {}
    with open(traces[0]) as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            if "k_resample" not in name and "k_gt_" not in name:
                continue
            key = (name.split("(")[0], int(row["Grid_Size_X"]) if "Grid_Size_X" in row else int(row.get("Grid_Size", 0)),
                   int(row["Grid_Size_Y"]) if "Grid_Size_Y" in row else 0)
            per.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    print("GTSTEP per-kernel device times, rocprofv3 --kernel-trace, 5 fused calls per factor (us)")
    for (name, gx, gy), ts in sorted(per.items(), key=lambda kv: (kv[0][0], -kv[0][1], -kv[0][2])):
        print("GTSTEP   %-58s grid %8d x %-6d calls %3d  median %9.1f us  min %9.1f us" % (name, gx, gy, len(ts), statistics.median(ts), min(ts)))
    for f in FACTORS:
        r, a = view_bytes(f)
        print("GTSTEP   // %d floor at %.0f TB/s: the four resizes %.1f us (%.1f MB), the assembly %.1f us (%.1f MB)"
              % (f, PEAK_BW / 1e12, r / PEAK_BW * 1e6, r / 1e6, a / PEAK_BW * 1e6, a / 1e6))
    return 0


def main():
    if "--kernels" in sys.argv:
        return kernels_only()
    if "--rocprof" in sys.argv:
        return rocprof()
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    host = host_view()
    view = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    try:
        import PIL
        pil = PIL.__version__
    except ImportError:
        pil = None
    print("GTSTEP view_ground_truth, %d x %d (w x h) uint8 view, median of %d calls after %d warm-up calls" % (W0, H0, CALLS, WARMUP))
    for f in FACTORS:
        w, h = W0 // f, H0 // f
        tag = "GTSTEP // %d -> %4d x %-4d" % (f, w, h)
        fused = lambda: gt.view_ground_truth(*(view[n] for n in NAMES), resolution=(w, h), fused=True)               # noqa: E731
        comp = lambda: gt.view_ground_truth(*(view[n] for n in NAMES), resolution=(w, h), fused=False)               # noqa: E731
        fused_up = lambda: gt.view_ground_truth(*(torch.from_numpy(host[n]).to(dev) for n in NAMES), resolution=(w, h), fused=True)   # noqa: E731
        comp_up = lambda: gt.view_ground_truth(*(torch.from_numpy(host[n]).to(dev) for n in NAMES), resolution=(w, h), fused=False)  # noqa: E731
        a, b = fused(), comp()
        same = all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
        print("%s fused and comparator agree bit for bit on image, mask and angle: %s" % (tag, same))
        res = {}
        for name, fn, kind in (("fused, inputs on the device", fused, "event"), ("comparator on the device", comp, "event"),
                               ("fused, with upload", fused_up, "host"), ("comparator on the device, with upload", comp_up, "host")):
            med, lo, hi = median_event_ms(fn) if kind == "event" else median_host_ms(fn, True)
            res[name] = med
            print("%s %-42s median %9.3f ms  (min %9.3f, max %9.3f)" % (tag, name, med, lo, hi))
        if pil:
            med, lo, hi = median_host_ms(lambda: host_form(host, w, h), False, warmup=1, calls=5)
            res["host"] = med
            print("%s %-42s median %9.3f ms  (min %9.3f, max %9.3f)  [5 calls]" % (tag, "Pillow %s + loadCam tail on the host" % pil, med, lo, hi))
            up = res["fused, with upload"]
            print("%s fused with upload is %.2fx the speed of the host form (%s)" % (tag, med / up, "faster" if up < med else "NOT faster"))
        else:
            print("%s Pillow does not import here: the host form is not measured" % tag)
        r, asm = view_bytes(f)
        floor_ms = (r + asm) / PEAK_BW * 1e3
        print("%s bytes: resizes %.1f MB + assembly %.1f MB, floor %.4f ms at %.0f TB/s; the fused view reaches %.1f %% of it"
              % (tag, r / 1e6, asm / 1e6, floor_ms, PEAK_BW / 1e12, 100 * floor_ms / res["fused, inputs on the device"]))
        for name, fn in (("fused", fused), ("comparator", comp)):
            k = kernel_launches(fn)
            if k is not None:
                print("%s launches per view, %-12s %5d" % (tag, name, k))
    return 0


if __name__ == "__main__":
    sys.exit(main())
