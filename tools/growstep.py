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
    guarded  fused     the same with mesh=, avoid=True (csrc/ghr_grow.h): the head is the 9976-face latitude-longitude unit sphere the
                       roots lie on; "grow  pruned" beside it is the unguarded trace with the same mesh= (both prune afterwards)
    query    composed  on a slice of the queries against the whole cloud; scaled up to all of them, printed as EXTRAPOLATED
The floor beside the figures is DERIVED, not measured: the pairs inside the radius (the sum of n over the queries, counted by the
query itself) times the lane operations of one pair (12 for the distance and the test every SCANNED pair pays are left out; an
inside pair costs about 40: the division, u, k, a, the dot, the sign, seven multiply-adds), at the part's fp32 vector rate.

With a library built with -DGHR_NN_COUNT_BLOCKS (it exports ghr_nn_read_counters; the product does not) the run prints the mean
number of blocks a wave scanned per walk instead of times: the counter's atomics are not in the product kernel.  With one built
with -DGHR_MD_COUNT_BLOCKS (ghr_meshdist_read_counters) it prints, for the guarded trace, the mesh searches the waves made and the
face blocks scanned and faces evaluated per search."""
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


def head_sphere(rad=1.0):
    """the 9976-face latitude-longitude sphere (116 x 44, the face count of the reference's head mesh) the default groom's roots
    lie on: its vertices are on the unit sphere, so every root is on or just above it"""
    from gaussianhaircut_amd.mesh import HeadMesh
    n_lon, n_lat = 116, 44
    v = [(0.0, 0.0, 1.0)]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        v += [(np.sin(th) * np.cos(2 * np.pi * j / n_lon), np.sin(th) * np.sin(2 * np.pi * j / n_lon), np.cos(th)) for j in range(n_lon)]
    v.append((0.0, 0.0, -1.0))
    f, last = [], len(v) - 1
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon  # noqa: E731
    for j in range(n_lon):
        f += [(0, ring(1, j), ring(1, j + 1)), (last, ring(n_lat - 1, j + 1), ring(n_lat - 1, j))]
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            f += [(ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)), (ring(i, j), ring(i + 1, j + 1), ring(i, j + 1))]
    return HeadMesh((np.asarray(v, np.float64) * rad).astype(np.float32), np.asarray(f, np.int32)), rad


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
    head, head_radius = head_sphere()
    grow = lambda: sg.grow_strands(field, roots, normals, radius=r, rho_min=rho_min, max_steps=400, fused=True)  # noqa: E731
    pruned = lambda: sg.grow_strands(field, roots, normals, radius=r, rho_min=rho_min, max_steps=400, fused=True, mesh=head)  # noqa: E731
    guarded = lambda: sg.grow_strands(field, roots, normals, radius=r, rho_min=rho_min, max_steps=400, fused=True, mesh=head,  # noqa: E731
                                      avoid=True)
    query = lambda: field.query(q, t, radius=r, fused=True)  # noqa: E731
    if hasattr(L, "ghr_meshdist_read_counters"):
        c = (ctypes.c_uint64 * 3)()
        L.ghr_meshdist_read_counters(c)   # zero
        out = guarded()
        _lib.check(L.ghr_meshdist_read_counters(c))
        print("GROWSTEP guarded counter build: %d mesh searches by %d waves (%.1f steps per wave); per search %.2f face blocks scanned "
              "of %d, %.1f faces evaluated; the strands made %d steps in all (%.1f live lanes per search)"
              % (c[1], (roots.shape[0] + 63) // 64, c[1] / ((roots.shape[0] + 63) // 64), c[0] / max(c[1], 1), (len(head.faces) + 63) // 64,
                 c[2] / max(c[1], 1), int((out["path"][:, 1:] != out["path"][:, :-1]).any(dim=2).sum()),
                 int((out["path"][:, 1:] != out["path"][:, :-1]).any(dim=2).sum()) / max(c[1], 1)))
        return
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
    forms = {"query fused": (query, 3, 1.0), "grow  fused": (grow, 1, 1.0), "grow  pruned": (pruned, 1, 1.0),
             "grow  guarded": (guarded, 1, 1.0),
             "query composed": (lambda: field.query(q[:slice_q], t[:slice_q], radius=r, fused=False), 1, q.shape[0] / slice_q)}
    n = query()[3]
    pairs = int(n.to(torch.int64).sum())
    out = grow()
    print("GROWSTEP query: %d pairs inside the radius (%.1f per query); grow: kept %d of %d strands, steps median %d longest %d" %
          (pairs, pairs / q.shape[0], int(out["keep"].sum()), roots.shape[0], int(out["steps"].float().median()), int(out["steps"].max())))
    po, go = pruned(), guarded()
    stop = torch.bincount(go["stop"].long(), minlength=3).tolist()
    print("GROWSTEP head: %d faces, radius %.4g; unguarded + prune keeps %d of %d (%.1f %%), steps median %d; guarded (margin %.5g) + "
          "prune keeps %d (%.1f %%), steps median %d longest %d; contact steps per strand mean %.1f median %d most %d, strands with a "
          "contact %d; stopped: %d out of steps, %d coasted out, %d head-on"
          % (len(head.faces), head_radius, int(po["keep"].sum()), roots.shape[0], 100.0 * int(po["keep"].sum()) / roots.shape[0],
             int(po["steps"].float().median()), go["margin"], int(go["keep"].sum()), 100.0 * int(go["keep"].sum()) / roots.shape[0],
             int(go["steps"].float().median()), int(go["steps"].max()), float(go["contacts"].float().mean()),
             int(go["contacts"].float().median()), int(go["contacts"].max()), int((go["contacts"] > 0).sum()), stop[0], stop[1], stop[2]))
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
    print("GROWSTEP guarded - pruned = %.3f ms (the guard inside the trace: the mesh search, the containment, the longer strands)"
          % (best["grow  guarded"] - best["grow  pruned"]))


if __name__ == "__main__":
    main()
