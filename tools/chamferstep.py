"""Time of the cross-cloud nearest-neighbour search and of chamfer_distance around it (gaussianhaircut_amd.nearest,
utils.loss_chamfer_utils; csrc/ghr_nn.h), HIP against the PyTorch-composed form, in ONE process on one GPU:

    python tools/chamferstep.py > profiles/chamfer.txt
    tools/build_variant.sh nncount -DGHR_NN_COUNT_BLOCKS
    GHR_LIB_PATH=build/variants/libghr_nncount.so python tools/chamferstep.py >> profiles/chamfer.txt

Workloads: `random` -- 100 000 x 100 000 points uniform in the unit cube; `strands` -- the segment midpoints of two grooms of
30 000 strands x 100 points (2 970 000 each), the second the first moved by a fraction of a segment per point.  Figures: `search`
(ghr_nn_search alone, keys and sorts given), `forward` (keys, the two sorts, search), `chamfer` (chamfer_distance with normals,
both directions, forward and backward).  Each is the device time between two events around `reps` calls, after a warm-up of every
form; the forms alternate inside one call and every round is printed.  The composed form is timed whole where it can finish
(`random`) and on a slice of the queries against the whole second cloud otherwise; a figure scaled up from a slice is printed as
EXTRAPOLATED.  The floor beside the figures is derived, not measured: see the text printed with it.

With a library built with -DGHR_NN_COUNT_BLOCKS (it exports ghr_nn_read_counters; the product does not) the run prints the mean
number of candidate blocks a wave scanned instead of times: the counter's atomics are not in the product kernel."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianhaircut_amd import _lib, nearest  # noqa: E402
from gaussianhaircut_amd.utils.loss_chamfer_utils import chamfer_distance  # noqa: E402

HBM_BPS = 6.29e12      # measured float4 copy rate of the part (8.0e12 spec)


def timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def clouds(dev):
    g = torch.Generator().manual_seed(1)
    out = {"random": (torch.rand(100_000, 3, generator=g).to(dev), torch.rand(100_000, 3, generator=g).to(dev), None, None)}
    S, L = 30_000, 100
    roots = torch.rand(S, 1, 3, generator=g) * 0.2
    steps = torch.nn.functional.normalize(torch.randn(S, 1, 3, generator=g), dim=2) * 0.002 + torch.randn(S, L - 1, 3, generator=g) * 0.0004
    a = roots + torch.cumsum(torch.cat((torch.zeros(S, 1, 3), steps), 1), 1)
    b = a + torch.randn(S, L, 3, generator=g) * 0.0005
    mids = [((p[:, :-1] + p[:, 1:]) * 0.5).reshape(-1, 3).contiguous().to(dev) for p in (a, b)]
    dirs = [(p[:, 1:] - p[:, :-1]).reshape(-1, 3).contiguous().to(dev) for p in (a, b)]
    out["strands"] = (mids[0], mids[1], dirs[0], dirs[1])
    return out


def search_only(x, y):
    """ghr_nn_search with the keys and sorts prepared once -> a callable"""
    Px, Py = x.shape[0], y.shape[0]
    kx, ky = nearest.union_keys(x, y)
    sx, sy = torch.sort(kx, stable=True), torch.sort(ky, stable=True)
    ws = torch.empty(_lib.nn_workspace_size(Px, Py), dtype=torch.uint8, device=x.device)
    dist = torch.empty(Px, dtype=torch.float32, device=x.device)
    idx = torch.empty(Px, dtype=torch.int32, device=x.device)
    p, s = nearest._ptr, nearest._stream

    def run():
        _lib.check(_lib.lib().ghr_nn_search(s(), Px, p(x), p(sx.indices), p(sx.values), Py, p(y), p(sy.indices), p(sy.values), 2,
                                            p(ws), p(dist), p(idx)))
        return dist, idx
    return run


def chamfer(x, y, xn, yn, fused):
    x, y = x[None].clone().requires_grad_(True), y[None].clone().requires_grad_(True)
    kw = {}
    if xn is not None:
        kw = dict(x_normals=xn[None].clone().requires_grad_(True), y_normals=yn[None].clone().requires_grad_(True))
    (cx, cy), (nx, ny), _, _ = chamfer_distance(x, y, **kw, fused=fused)
    loss = cx + cy if nx is None else cx + cy + nx + ny
    loss.backward()
    return loss


def main():
    assert torch.cuda.is_available(), "chamferstep needs a ROCm GPU (a CPU run measures nothing)"
    dev = torch.device("cuda:0")
    L = _lib.lib()
    counting = hasattr(L, "ghr_nn_read_counters")
    rounds = 3
    for name, (x, y, xn, yn) in clouds(dev).items():
        Px, Py = x.shape[0], y.shape[0]
        run = search_only(x, y)
        if counting:
            c = (ctypes.c_uint64 * 2)()
            L.ghr_nn_read_counters(c)   # zero
            for a, b, tag in ((x, y, "x->y"), (y, x, "y->x")):
                search_only(a, b)()
                _lib.check(L.ghr_nn_read_counters(c))
                print("CHAMFERSTEP %-8s %s counter build: %d candidate blocks scanned by %d waves = %.2f per wave (of %d blocks; seed included)"
                      % (name, tag, c[0], c[1], c[0] / max(c[1], 1), (b.shape[0] + 63) // 64))
            continue
        slice_q = Px if Px * Py <= 2e10 else max(64, int(6e9 // Py) // 64 * 64)
        forms = {
            "search   fused": (lambda: run(), 10, 1.0),
            "forward  fused": (lambda: nearest.search_hip(x, y, 2), 10, 1.0),
            "forward  composed": (lambda: nearest.nearest_composed(x[:slice_q], y, 2), 1, Px / slice_q),
            "chamfer  fused": (lambda: chamfer(x, y, xn, yn, True), 5, 1.0),
        }
        if slice_q == Px:
            forms["chamfer  composed"] = (lambda: chamfer(x, y, xn, yn, False), 1, 1.0)
        d, i = run()
        dc, ic = nearest.nearest_composed(x[:slice_q], y, 2)
        assert torch.equal(i[:slice_q].long(), ic) and torch.equal(d[:slice_q], dc), "the two forms disagree"
        print("CHAMFERSTEP %-8s Px=%d Py=%d: forms equal on %d queries (dist bits, idx)" % (name, Px, Py, slice_q))
        for fn, _, _ in forms.values():
            timed(fn, 1)
        best = {}
        for rd in range(rounds):
            for form, (fn, reps, scale) in forms.items():
                ms = timed(fn, reps)
                best[form] = min(best.get(form, ms * scale), ms * scale)
                if scale == 1.0:
                    print("CHAMFERSTEP %-8s round %d %-18s %10.3f ms" % (name, rd, form, ms))
                else:
                    print("CHAMFERSTEP %-8s round %d %-18s %10.3f ms on %d of %d queries -> EXTRAPOLATED x %.1f = %.0f ms"
                          % (name, rd, form, ms, slice_q, Px, scale, ms * scale))
        # derived floor of the search: every sorted point of both clouds read once (16 B), dist and idx written (8 B per query)
        floor = (16.0 * (Px + Py) + 8.0 * Px) / HBM_BPS * 1e3
        print("CHAMFERSTEP %-8s floor (DERIVED: 16 B per sorted point read, 8 B per query written, at the measured %.2f TB/s copy rate): "
              "%.4f ms; search reaches %.2f %% of it" % (name, HBM_BPS / 1e12, floor, 100 * floor / best["search   fused"]))
        print("CHAMFERSTEP %-8s forward fused / composed = %.5f%s" % (name, best["forward  fused"] / best["forward  composed"],
                                                                      "" if slice_q == Px else " (composed EXTRAPOLATED)"))


if __name__ == "__main__":
    main()
