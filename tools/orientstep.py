"""Time of the orientation maps, HIP kernels against the PyTorch-composed comparator (gaussianhaircut_amd.orientation,
fused=True / fused=False -- the latter with the reference's 64-pixel patch loop), in ONE process on one GPU:

    python tools/orientstep.py > profiles/orientation_maps.txt

Sizes 1024 x 1024 (the reference's) and 512 x 512, a textured uint8 RGB image on the device.  Each figure is the MEDIAN device
time between two events around one ``orientation_maps`` call, over 50 calls after 10 warm-up calls of that form and size; the
split into the difference of Gaussians and the bank is timed the same way for the fused form.  Launches per image are counted by
torch.profiler over one call (device kernel events; copies excluded).  The floor is derived, not measured:
2 * n_filters * ksize^2 FLOP per pixel (the zero-padded taps included) against the 157.3 TFLOP/s fp32 peak.

Per-kernel times come from a run of their own, in a fresh child process under the profiler:

    python tools/orientstep.py --rocprof       # rocprofv3 --kernel-trace --stats -- python tools/orientstep.py --kernels
"""
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussianhaircut_amd import orientation as ori  # noqa: E402

SIZES = (1024, 512)
WARMUP, CALLS = 10, 50
PEAK_FP32 = 157.3e12


def image(n, seed=0):
    g = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    a = 0.6 + 0.8 * np.sin(x / 23) + 0.5 * np.cos(y / 17)
    base = 0.5 + 0.3 * np.sin(2 * np.pi * 0.2 * (x * np.cos(a) + y * np.sin(a)))
    img = np.stack([base * 0.9, base * 0.7, base * 0.5], -1) + 0.05 * g.standard_normal((n, n, 3))
    return (np.clip(img, 0, 1) * 255).astype(np.uint8)


def median_ms(fn, warmup=WARMUP, calls=CALLS):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
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
        print("ORIENTSTEP launch count not taken: %r" % (exc,))
        return None


def kernels_only():
    """what the profiled child runs: two warm-up calls and three profiled ones of the fused form per size"""
    dev = torch.device("cuda:0")
    for n in SIZES:
        img = torch.from_numpy(image(n)).to(dev)
        for _ in range(5):
            ori.orientation_maps(img, fused=True)
        torch.cuda.synchronize()


def rocprof():
    out = tempfile.mkdtemp(prefix="orientstep_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "orient", "--",
           sys.executable, os.path.abspath(__file__), "--kernels"]
    res = subprocess.run(cmd, cwd=out, capture_output=True, text=True, timeout=600)
    if res.returncode != 0:
        print("ORIENTSTEP rocprofv3 failed (%d): %s" % (res.returncode, (res.stdout + res.stderr)[-2000:]))
        return 1
    traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    if not traces:
        print("ORIENTSTEP rocprofv3 wrote no kernel trace under %s" % out)
        return 1
    per = {}
    with open(traces[0]) as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            if "k_orient" not in name:
                continue
            key = (name.split("(")[0], int(row["Grid_Size_X"]) if "Grid_Size_X" in row else int(row.get("Grid_Size", 0)))
            per.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    print("ORIENTSTEP per-kernel device times, rocprofv3 --kernel-trace, 5 fused calls per size (median of the calls, us)")
    for (name, grid), ts in sorted(per.items(), key=lambda kv: (kv[0][0], -kv[0][1])):
        print("ORIENTSTEP   %-60s grid.x %8d  calls %2d  median %10.1f us  min %10.1f us" % (name, grid, len(ts), statistics.median(ts), min(ts)))
    return 0


def main():
    if "--kernels" in sys.argv:
        return kernels_only()
    if "--rocprof" in sys.argv:
        return rocprof()
    dev = torch.device("cuda:0")
    w, _ = ori.gabor_bank()
    Fn, K = w.shape[0], w.shape[-1]
    print("ORIENTSTEP orientation_maps, %d filters of %d x %d taps, uint8 RGB image on the device, median of %d calls after %d warm-up calls, "
          "device events" % (Fn, K, K, CALLS, WARMUP))
    for n in SIZES:
        img = torch.from_numpy(image(n)).to(dev)
        flop = 2.0 * Fn * K * K * n * n
        floor_ms = flop / PEAK_FP32 * 1e3
        plane = ori.dog_fused(img)
        res = {}
        for name, fn in (("fused", lambda: ori.orientation_maps(img, fused=True)),
                         ("torch (64-pixel patches)", lambda: ori.orientation_maps(img, fused=False)),
                         ("fused: difference of Gaussians alone", lambda: ori.dog_fused(img)),
                         ("fused: bank alone (arg-max, variance, angle, conf)", lambda: ori.gabor_fused(plane, ground_truth=True)),
                         ("torch: difference of Gaussians alone", lambda: ori.difference_of_gaussians(img, fused=False)),
                         ("torch: bank alone", lambda: ori.gabor_orientation(plane, fused=False))):
            med, lo, hi = median_ms(fn)
            res[name] = med
            print("ORIENTSTEP %4d x %-4d %-52s median %9.3f ms  (min %9.3f, max %9.3f)" % (n, n, name, med, lo, hi))
        f, t = res["fused"], res["torch (64-pixel patches)"]
        print("ORIENTSTEP %4d x %-4d fused is %.2fx the speed of torch (%s)" % (n, n, t / f, "faster" if f < t else "NOT faster"))
        bank = res["fused: bank alone (arg-max, variance, angle, conf)"]
        print("ORIENTSTEP %4d x %-4d bank: %.1f GFLOP, floor %.3f ms at %.1f TFLOP/s fp32; the bank kernel reaches %.1f %% of it (%.1f TFLOP/s)"
              % (n, n, flop / 1e9, floor_ms, PEAK_FP32 / 1e12, 100 * floor_ms / bank, flop / bank / 1e9))
        for name, fn in (("fused", lambda: ori.orientation_maps(img, fused=True)),
                         ("torch (64-pixel patches)", lambda: ori.orientation_maps(img, fused=False))):
            k = kernel_launches(fn)
            if k is not None:
                print("ORIENTSTEP %4d x %-4d launches per image, %-28s %6d" % (n, n, name, k))
    return 0


if __name__ == "__main__":
    sys.exit(main())
