"""Time of the hair field and of growing strands through it (gaussianhaircut_amd.strand_growing; csrc/ghr_field.h), HIP against
the PyTorch-composed form, in ONE process on one GPU:

    python tools/growstep.py > profiles/strand_growing.txt
    tools/build_variant.sh nncount -DGHR_NN_COUNT_BLOCKS
    GHR_LIB_PATH=build/variants/libghr_nncount.so python tools/growstep.py >> profiles/strand_growing.txt

The cloud: 500 000 points sampled from tools/synthetic_capture.py's default groom (its strands' points, jittered; directions the
segment tangents with random signs).  Forms, alternated inside one call over three rounds, each the device time between two events
after a warm-up of every form:
    query    fused     field.query of 3 000 000 queries (the cloud's points, jittered, six times over), their key sort included
    grow     fused     grow_strands of 30 000 roots (the groom's own roots and outward normals), M = 400, L = 100
    query    composed  on a slice of the queries against the whole cloud; scaled up to all of them, printed as EXTRAPOLATED
The floor beside the figures is DERIVED, not measured: the pairs inside the radius (the sum of n over the queries, counted by the
query itself) times the lane operations of one pair (12 for the distance and the test every SCANNED pair pays are left out; an
inside pair costs about 40: the division, u, k, a, the dot, the sign, seven multiply-adds), at the part's fp32 vector rate.

With a library built with -DGHR_NN_COUNT_BLOCKS (it exports ghr_nn_read_counters; the product does not) the run prints the mean
number of blocks a wave scanned per walk instead of times: the counter's atomics are not in the product kernel."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussianhaircut_amd import _lib  # noqa: E402
from gaussianhaircut_amd import strand_growing as sg  # noqa: E402

LANE_RATE = 256 * 4 * 16 * 2.4e9   # 256 CUs x 4 SIMDs x 16 lanes a clock at 2.4 GHz: one fp32 vector operation per lane and clock
OPS_PER_PAIR = 40


def timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def scene(dev, P=500_000, S=30_000):
    spec = importlib.util.spec_from_file_location("synthetic_capture_tool", os.path.join(ROOT, "tools", "synthetic_capture.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    strands = tool.grown_hair(S, 24, 1)                                     # [S, 24, 3]
    g = np.random.default_rng(2)
    mids = 0.5 * (strands[:, 1:] + strands[:, :-1]).reshape(-1, 3)
    tang = (strands[:, 1:] - strands[:, :-1]).reshape(-1, 3)
    pick = g.choice(mids.shape[0], P, replace=False)
    pts = mids[pick] + g.normal(size=(P, 3)).astype(np.float32) * 0.002
    dirs = tang[pick] * g.choice([-1.0, 1.0], P)[:, None].astype(np.float32)
    field = sg.HairField(torch.from_numpy(pts).to(dev), torch.from_numpy(dirs).to(dev), torch.full((P,), 0.8, device=dev),
                         torch.from_numpy(g.random((P, 3)).astype(np.float32)).to(dev))
    roots = torch.from_numpy(strands[:, 0]).to(dev)
    normals = torch.nn.functional.normalize(roots, dim=1)
    q = torch.from_numpy(np.concatenate([pts + g.normal(size=(P, 3)).astype(np.float32) * 0.004 for _ in range(6)])).to(dev)
    t = torch.from_numpy(np.tile(dirs, (6, 1))).to(dev).contiguous()
    return field, roots.contiguous(), normals.contiguous(), q.contiguous(), t


def main():
    assert torch.cuda.is_available(), "growstep needs a ROCm GPU (a CPU run measures nothing)"
    dev = torch.device("cuda:0")
    L = _lib.lib()
    counting = hasattr(L, "ghr_nn_read_counters")
    field, roots, normals, q, t = scene(dev)
    r = field.default_radius()
    rho_min = field.default_rho_min(r)
    print("GROWSTEP cloud P=%d radius %.5g (default) step %.5g rho_min %.5g; Q=%d queries, S=%d roots" %
          (field.P, r, r / 2.5, rho_min, q.shape[0], roots.shape[0]))
    grow = lambda: sg.grow_strands(field, roots, normals, radius=r, rho_min=rho_min, max_steps=400, fused=True)  # noqa: E731
    query = lambda: field.query(q, t, radius=r, fused=True)  # noqa: E731
    if counting:
        c = (ctypes.c_uint64 * 2)()
        for name, fn in (("query", query), ("grow", grow)):
            L.ghr_nn_read_counters(c)   # zero
            fn()
            _lib.check(L.ghr_nn_read_counters(c))
            print("GROWSTEP %-6s counter build: %d blocks scanned in %d walks = %.2f per walk (of %d blocks; block 0 included)"
                  % (name, c[0], c[1], c[0] / max(c[1], 1), (field.P + 63) // 64))
        return
    slice_q = 4096
    forms = {"query fused": (query, 3, 1.0), "grow  fused": (grow, 1, 1.0),
             "query composed": (lambda: field.query(q[:slice_q], t[:slice_q], radius=r, fused=False), 1, q.shape[0] / slice_q)}
    n = query()[3]
    pairs = int(n.to(torch.int64).sum())
    out = grow()
    print("GROWSTEP query: %d pairs inside the radius (%.1f per query); grow: kept %d of %d strands, steps median %d longest %d" %
          (pairs, pairs / q.shape[0], int(out["keep"].sum()), roots.shape[0], int(out["steps"].float().median()), int(out["steps"].max())))
    a, b = query(), field.query(q[:slice_q], t[:slice_q], radius=r, fused=False)
    err = float(((a[0][:slice_q] - b[0]).abs() / b[0].clamp_min(1e-30)).max())
    assert torch.equal(a[3][:slice_q], b[3]) and err < 1e-5, ("the two forms disagree", err)
    for fn, _, _ in forms.values():
        timed(fn, 1)
    best = {}
    for rd in range(3):
        for form, (fn, reps, scale) in forms.items():
            ms = timed(fn, reps)
            best[form] = min(best.get(form, ms * scale), ms * scale)
            if scale == 1.0:
                print("GROWSTEP round %d %-15s %10.3f ms" % (rd, form, ms))
            else:
                print("GROWSTEP round %d %-15s %10.3f ms on %d of %d queries -> EXTRAPOLATED x %.1f = %.0f ms" %
                      (rd, form, ms, slice_q, q.shape[0], scale, ms * scale))
    floor = pairs * OPS_PER_PAIR / LANE_RATE * 1e3
    print("GROWSTEP query floor (DERIVED: %d inside pairs x %d lane operations at %.3g lane operations / s): %.3f ms; "
          "query reaches %.1f %% of it" % (pairs, OPS_PER_PAIR, LANE_RATE, floor, 100 * floor / best["query fused"]))
    print("GROWSTEP query fused / composed (EXTRAPOLATED) = %.5f" % (best["query fused"] / best["query composed"]))


if __name__ == "__main__":
    main()
