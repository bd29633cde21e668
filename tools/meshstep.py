"""Time of the head-mesh containment workloads (gaussianhaircut_amd.mesh), HIP kernels against the composed forms, in ONE process
on one GPU:

    python tools/meshstep.py > profiles/mesh_query.txt

The mesh is a UV sphere of 9976 faces (116 x 44: the face count of the reference's head mesh, which is not redistributable),
radius 1.  Workloads: the probe filter over P = 1 M Gaussians (centres over 1.25 x the box, scales of a few percent of it), `contains`
over 3 M points, and the grid build.  Forms of the probe filter: fused (k_gaussian_probe_outside), composed (the probes built
in PyTorch + k_mesh_contains + all) and, at P = 2000, the PyTorch brute force over all faces.  Each figure is the device time
between two events around `reps` calls, after a warm-up of every form; the forms alternate and every round is printed.
The floor beside the figures is derived, not measured: see the text printed with it."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianhaircut_amd.mesh import HeadMesh  # noqa: E402
from tests import mesh_cases as mc  # noqa: E402

HBM_BPS = 6.29e12      # measured float4 copy rate of the part (8.0e12 spec)
LANE_OPS = 78.6e12     # fp32 vector instructions x lanes per second: half the 157.3 TFLOPS that count an FMA as two
TRI_OPS = 80           # lane operations of one record against one query, counted in mesh_crossed (csrc/ghr_mesh.h)


def timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    assert torch.cuda.is_available(), "meshstep needs a ROCm GPU (a CPU run measures nothing)"
    dev = torch.device("cuda:0")
    P = int(os.environ.get("MESHSTEP_P", 1_000_000))
    Q = int(os.environ.get("MESHSTEP_Q", 3_000_000))
    rounds, reps = 3, 10
    v, f = mc.uv_sphere(116, 44)
    t0 = time.perf_counter()
    builds = 5
    for _ in range(builds):
        mesh = HeadMesh(v, f)
    build_ms = (time.perf_counter() - t0) * 1e3 / builds
    stats = mesh.grid_stats()
    mean_len = sum(m for m, _ in stats) / 3
    print("MESHSTEP mesh faces=%d G=%d blob=%.2f MB lists mean/max per axis: %s" % (
        len(f), mesh.grid, mesh.header.bytes / 1e6, " ".join("%.2f/%d" % s for s in stats)))
    print("MESHSTEP grid build (host, one thread, tables only; the upload is one copy of the blob): %.2f ms" % build_ms)

    xyz, s, r = (torch.from_numpy(a).to(dev) for a in mc.gaussians("icosphere2", P, seed=1))
    s = s * 0.5
    pts = torch.from_numpy(np.random.default_rng(3).uniform(-1.25, 1.25, (Q, 3)).astype(np.float32)).to(dev)
    forms = {
        "fused": lambda: mesh.probes_outside(xyz, s, r, fused=True),
        "composed": lambda: mesh.probes_outside(xyz, s, r, fused=False, fused_contains=True),
    }
    a, b = forms["fused"](), forms["composed"]()
    assert torch.equal(a, b), "the two forms disagree"
    print("MESHSTEP probe filter P=%d: %d kept of %d (forms equal)" % (P, int(a.sum()), P))
    for fn in forms.values():
        timed(fn, 2)
    best = {}
    for rd in range(rounds):
        for name, fn in forms.items():
            ms = timed(fn, reps)
            best[name] = min(best.get(name, ms), ms)
            print("MESHSTEP round %d probe filter %-8s %.3f ms" % (rd, name, ms))
    timed(lambda: mesh.contains(pts), 2)
    c_ms = min(timed(lambda: mesh.contains(pts), reps) for _ in range(rounds))
    print("MESHSTEP contains Q=%d fused %.3f ms (%.1f G queries/s)" % (Q, c_ms, Q / c_ms / 1e6))
    Pb = 2000
    brute = lambda: mesh.probes_outside(xyz[:Pb], s[:Pb], r[:Pb], fused=False, fused_contains=False)  # noqa: E731
    timed(brute, 1)
    b_ms = timed(brute, 3)
    print("MESHSTEP probe filter P=%d torch brute force %.3f ms (x %d = %.0f ms at P=%d)" % (Pb, b_ms, P // Pb, b_ms * P / Pb, P))

    # the derived floor: 40 B read + 1 B written per Gaussian at the measured copy rate, and 3 axes x the mean list length x 12
    # probes records at TRI_OPS lane operations each at the vector unit's rate (a probe outside the box walks nothing: fewer)
    t_mem = 41.0 * P / HBM_BPS * 1e3
    t_alu = 3 * mean_len * 12 * P * TRI_OPS / LANE_OPS * 1e3
    floor = max(t_mem, t_alu)
    print("MESHSTEP floor: traffic %.4f ms, arithmetic %.4f ms (mean list %.2f) -> %.4f ms; fused reaches %.1f %% of it, composed %.1f %%"
          % (t_mem, t_alu, mean_len, floor, 100 * floor / best["fused"], 100 * floor / best["composed"]))
    print("MESHSTEP fused / composed = %.3f" % (best["fused"] / best["composed"]))


if __name__ == "__main__":
    main()
