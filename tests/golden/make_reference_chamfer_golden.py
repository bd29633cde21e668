"""Generates tests/golden/reference_chamfer_golden.npz by running THE REFERENCE'S OWN ``chamfer_distance``
(src/utils/loss_chamfer_utils.py, read-only, imported from /root/reference/src) on the CPU in float64.  Run once in the build
container (the reference does not exist where the GPU tests run; the committed .npz is what the tests read):

    python tests/golden/make_reference_chamfer_golden.py

The module imports pytorch3d, which is not installed; two stand-ins are placed in ``sys.modules`` first:
``pytorch3d.ops.knn`` with a brute-force ``knn_points`` / ``knn_gather`` in the inputs' dtype (squared L2 or L1 over every pair,
the lowest index among equal distances taken explicitly, padded query rows distance 0 and index 0 -- pytorch3d's conventions),
and ``pytorch3d.structures.pointclouds`` with an empty ``Pointclouds`` class.  The cases are random clouds, so the stand-in's tie
rule decides nothing: the script asserts that every query's two smallest distances differ by more than 1e-5 of the smaller.

Inputs and argument combinations: tests/chamfer_cases.py (``golden_inputs``, ``GOLDEN_CASES``, ``GOLDEN_ERRORS``); float32 values
evaluated in float64.  Stored per case ``<name>``: the returned terms ``<name>/<term>_<side>`` for term in dist, normals,
features, weights and side in x, y (absent where the reference returns None), the gradients ``<name>/d_<input>`` of
``chamfer_cases.scalar_of`` w.r.t. x, y and both normals, and for the error cases the exception's type and text.  Nothing from
the reference is copied into the repository -- only numeric outputs.
"""
import importlib.util
import os
import sys
import types
from collections import namedtuple

import numpy as np
import torch

REF = "/root/reference/src"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import chamfer_cases as cc  # noqa: E402

_KNN = namedtuple("KNN", "dists idx knn")
MIN_GAP = [float("inf")]


def knn_points(p1, p2, lengths1=None, lengths2=None, norm=2, K=1):
    assert K == 1
    N, P1, _ = p1.shape
    P2 = p2.shape[1]
    dists, idx = p1.new_zeros(N, P1, 1), torch.zeros(N, P1, 1, dtype=torch.int64)
    for n in range(N):
        l1 = P1 if lengths1 is None else int(lengths1[n])
        l2 = P2 if lengths2 is None else int(lengths2[n])
        diff = p2[n, None, :l2] - p1[n, :l1, None]
        d = (diff * diff).sum(-1) if norm == 2 else diff.abs().sum(-1)
        mn = d.min(-1, keepdim=True).values
        i = torch.where(d == mn, torch.arange(l2)[None], l2).min(-1).values
        two = torch.topk(d.detach(), 2, dim=-1, largest=False).values
        MIN_GAP[0] = min(MIN_GAP[0], float(((two[:, 1] - two[:, 0]) / two[:, 0]).min()))
        dists[n, :l1, 0] = d.gather(1, i[:, None])[:, 0]
        idx[n, :l1, 0] = i
    return _KNN(dists, idx, None)


def knn_gather(x, idx, lengths=None):
    N, M, U = x.shape
    _, L, K = idx.shape
    out = x[:, :, None].expand(N, M, K, U).gather(1, idx[:, :, :, None].expand(N, L, K, U))
    if lengths is not None:
        out = out * (torch.arange(K)[None, :] < lengths[:, None])[:, None, :, None].to(out.dtype)
    return out


def _reference():
    for name in ("pytorch3d", "pytorch3d.ops", "pytorch3d.ops.knn", "pytorch3d.structures", "pytorch3d.structures.pointclouds"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["pytorch3d.ops.knn"].knn_points = knn_points
    sys.modules["pytorch3d.ops.knn"].knn_gather = knn_gather
    sys.modules["pytorch3d.structures.pointclouds"].Pointclouds = type("Pointclouds", (), {})
    spec = importlib.util.spec_from_file_location("ref_loss_chamfer_utils", os.path.join(REF, "utils", "loss_chamfer_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = _reference()
    inp = cc.golden_inputs()
    out = {"in/" + k: v.numpy() for k, v in inp.items()}
    for name, (uses, extra) in cc.GOLDEN_CASES.items():
        kw = cc.golden_kwargs(uses, inp, torch.float64)
        res = ref.chamfer_distance(**kw, **extra)
        if "w" in uses:
            assert res[3][0] is kw["x_weights"] and res[3][1] is kw["y_weights"]
        cc.scalar_of(res).backward()
        for term, pair in zip(("dist", "normals", "features", "weights"), res):
            for side, v in zip("xy", pair):
                if v is not None:
                    out["%s/%s_%s" % (name, term, side)] = v.detach().numpy().astype(np.float64)
        for k in ("x", "y", "x_normals", "y_normals"):
            if k in kw and kw[k].grad is not None:
                out["%s/d_%s" % (name, k)] = kw[k].grad.numpy().astype(np.float64)
        print(name, sorted(k.split("/")[1] for k in out if k.startswith(name + "/")))
    for name, (uses, extra) in cc.GOLDEN_ERRORS.items():
        try:
            ref.chamfer_distance(**cc.golden_kwargs(uses, inp, torch.float64), **extra)
            raise SystemExit("%s: the reference did not raise" % name)
        except Exception as e:  # noqa: BLE001  (whatever the reference raises is the record)
            out["%s/error" % name] = np.array([type(e).__name__, str(e)])
            print(name, type(e).__name__, e)
    print("smallest relative gap between a query's two nearest candidates: %.3e" % MIN_GAP[0])
    assert MIN_GAP[0] > 1e-5
    path = cc.GOLDEN
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
