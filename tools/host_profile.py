"""Where the HOST's time per training step goes (round 6): cProfile over steps of a workload small enough that the GPU idles
(cfg1), so that wall time = host time.    python tools/host_profile.py [steps] [--native] [--bank]
``--native``: the views as one ``ghr_view_step`` call each (``training_step(native=True)``; the first warm-up step, which has no
capacity guess yet, still runs the Python way).  ``--bank``: the cameras are one ``scene.cameras.CameraBank`` that the step trains
(``camera_bank=``); with ``--native`` its views are one ``ghr_view_step_camera`` call each."""
import cProfile
import io
import os
import pstats
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianhaircut_amd.scene.cameras import CameraBank, ring_cameras  # noqa: E402
from gaussianhaircut_amd.scene.gaussian_model import OptimizationParams  # noqa: E402
from gaussianhaircut_amd.trainer import last_step_path, make_ground_truth, training_step  # noqa: E402
from gaussianhaircut_amd.utils import synthetic as syn  # noqa: E402


def main():
    argv = [a for a in sys.argv[1:] if a not in ("--native", "--bank")]
    native = True if "--native" in sys.argv[1:] else False
    banked = "--bank" in sys.argv[1:]
    K = int(argv[0]) if argv else 400
    dev = torch.device("cuda:0")
    spec = syn.CONFIGS["cfg1"]
    opt = OptimizationParams()
    opt.lambda_dorient = 0.1
    bg = syn.background(dev)
    model = syn.make_model(spec, dev)
    pool = ring_cameras(4, spec.W, spec.H, device=dev)
    with torch.no_grad():
        gt = syn.make_model(spec, dev)
        gt._features_dc.add_(0.2)
        make_ground_truth(gt, pool, bg)
    model.training_setup(opt)
    kw = {}
    if banked:
        bank = CameraBank(pool, use_barf=True, device=dev).training_setup(opt)
        pool, kw = list(bank), dict(camera_bank=bank)
    for i in range(50):
        training_step(model, [pool[i % 4]], bg, opt, i + 1, native=native, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(K):
        training_step(model, [pool[i % 4]], bg, opt, 51 + i, native=native, **kw)
    torch.cuda.synchronize()
    print("HOST %.4f ms per step (cfg1: the GPU idles; %s path%s)" %
          (1e3 * (time.perf_counter() - t0) / K, last_step_path(), ", camera bank" if banked else ""))
    pr = cProfile.Profile()
    pr.enable()
    for i in range(K):
        training_step(model, [pool[i % 4]], bg, opt, 51 + K + i, native=native, **kw)
    torch.cuda.synchronize()
    pr.disable()
    s = io.StringIO()
    pstats.Stats(pr, stream=s).sort_stats("tottime").print_stats(28)
    for line in s.getvalue().splitlines():
        if line.strip():
            print("HOST", line[:200])


if __name__ == "__main__":
    main()
