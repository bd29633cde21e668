"""distCUDA2 timing (gaussianhaircut_amd/simple_knn, csrc/ghr_knn.h): 100k, 500k and 2M points, each as a uniform cloud and a
COLMAP-like one (utils/synthetic.colmap_like_cloud: a head-sized shell of uneven density with 1 % far outliers).  One JSON
line per case: the median of >= 20 device-event-timed whole calls, the split into keys (bounds + k_knn_keys), sort
(torch.sort) and boxes + search (ghr_knn_mean_dist2: k_knn_boxes and k_knn_search; their own split comes from a kernel
trace), and a checksum of the result.  At 100k and 200k (uniform) it also times the chunked GPU brute force of
tests/test_gpu_knn.py for comparison.

    python tools/knn_bench.py [--reps 20] [--sizes 100000,500000,2000000] [--no-brute] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianhaircut_amd.simple_knn import _C  # noqa: E402
from gaussianhaircut_amd.utils import synthetic as syn  # noqa: E402

DEV = torch.device("cuda:0")


def cloud(kind, P, seed):
    if kind == "uniform":
        g = torch.Generator().manual_seed(seed)
        return (torch.rand(P, 3, generator=g) * 2 - 1).to(DEV)
    return syn.colmap_like_cloud(P, seed)[0].to(DEV)


def timed(fn, reps):
    """median / min milliseconds of `reps` calls, each between two device events"""
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts)


def brute_once(pts):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tests.test_gpu_knn import brute
    return brute(pts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="100000,500000,2000000")
    ap.add_argument("--no-brute", action="store_true", help="skip the brute-force comparison (kernel traces)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    lines = []
    for P in [int(s) for s in a.sizes.split(",")]:
        for kind in ("uniform", "colmap_like"):
            pts = _C.prepare(cloud(kind, P, 1))
            for _ in range(3):  # warm-up: code objects, the sort's algorithm choice, allocator
                out = _C.distCUDA2(pts)
            torch.cuda.synchronize()
            whole, whole_min = timed(lambda: _C.distCUDA2(pts), a.reps)
            keys = _C.keys(pts)
            order = _C.sort_order(keys)
            t_keys, _ = timed(lambda: _C.keys(pts), a.reps)
            t_sort, _ = timed(lambda: _C.sort_order(keys), a.reps)
            t_search, _ = timed(lambda: _C.mean_dist2(pts, order), a.reps)
            rec = dict(case="%s_%d" % (kind, P), P=P, reps=a.reps, whole_ms_median=round(whole, 4),
                       whole_ms_min=round(whole_min, 4), keys_ms=round(t_keys, 4), sort_ms=round(t_sort, 4),
                       boxes_search_ms=round(t_search, 4),
                       checksum=hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()[:16],
                       mean_dist2=float(out.double().mean()))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    for P in () if a.no_brute else (100_000, 200_000):
        pts = cloud("uniform", P, 1)
        knn = _C.distCUDA2(pts)
        brute_once(pts[:1000])  # warm-up
        torch.cuda.synchronize()
        t_brute, _ = timed(lambda: brute_once(pts), 1)
        t_knn, _ = timed(lambda: _C.distCUDA2(pts), a.reps)
        same = bool((torch.from_numpy(brute_once(pts)).view(torch.int32) == knn.cpu().view(torch.int32)).all())
        rec = dict(case="brute_force_uniform_%d" % P, P=P, brute_ms=round(t_brute, 2), knn_ms=round(t_knn, 4),
                   speedup=round(t_brute / t_knn, 1), bit_identical=same)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")


if __name__ == "__main__":
    main()
