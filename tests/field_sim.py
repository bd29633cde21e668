"""ctypes front of tests/hostsim/ghr_hostsim_field.cpp: the host walk of csrc/ghr_field.h's kernels on numpy arrays."""
import ctypes

import numpy as np

from tests import helpers as hp

DEPS = ["ghr_hostsim_knn.cpp", "ghr_field.h", "ghr_nn.h", "ghr_knn.h"]


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def load():
    so = hp.compile_hostsim("libghr_hostsim_field.so", "ghr_hostsim_field.cpp", ["-O1", "-fPIC", "-shared"], DEPS)
    L = ctypes.CDLL(so)
    vp, i64, i32, f = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float
    L.ghrsim_knn_keys.argtypes = [i64, vp, vp, vp]
    L.ghrsim_field_query.argtypes = [i64] + [vp] * 5 + [i64, vp, vp, vp, f] + [vp] * 5
    L.ghrsim_field_trace.argtypes = [i64] + [vp] * 5 + [i64, vp, vp, vp, i32, f, f, f, f, i32] + [vp] * 4
    L.ghrsim_strands_resample.argtypes = [i64, i32, i32, vp, vp, vp]
    for n in ("ghrsim_knn_keys", "ghrsim_field_query", "ghrsim_field_trace", "ghrsim_strands_resample"):
        getattr(L, n).restype = None
    return L


def key_order(L, pts, bounds=None):
    """(order int64: the stable sort of the points' Morton keys over ``bounds`` -- None: their own --, bounds)"""
    pts = np.ascontiguousarray(pts, np.float32)
    if bounds is None:
        bounds = np.concatenate([pts.min(0), pts.max(0)]).astype(np.float32)
    keys = np.zeros(pts.shape[0], np.uint64)
    L.ghrsim_knn_keys(pts.shape[0], _p(pts), _p(bounds), _p(keys))
    return np.argsort(keys, kind="stable").astype(np.int64), bounds


def _cloud_args(L, cloud):
    order, _ = key_order(L, cloud["points"])
    return order, [cloud["points"].shape[0], _p(cloud["points"]), _p(order), _p(cloud["directions"]), _p(cloud["weights"]),
                   _p(cloud["colors"])]


def query(L, cloud, x, t, r2, qorder=None):
    """-> rho, v, c, n, scanned (blocks per wave)"""
    x, t = np.ascontiguousarray(x, np.float32).reshape(-1, 3), np.ascontiguousarray(t, np.float32).reshape(-1, 3)
    Q = x.shape[0]
    rho, v, c = np.full(Q, np.nan, np.float32), np.full((Q, 3), np.nan, np.float32), np.full((Q, 3), np.nan, np.float32)
    n, scanned = np.full(Q, -1, np.int32), np.zeros((Q + 63) // 64, np.uint32)
    order, args = _cloud_args(L, cloud)
    qo = None if qorder is None else np.ascontiguousarray(qorder, np.int64)
    L.ghrsim_field_query(*args, Q, _p(x), _p(t), _p(qo), float(r2), _p(rho), _p(v), _p(c), _p(n), _p(scanned))
    return rho, v, c, n, scanned


def trace(L, cloud, roots, normals, M, r2, h, beta, rho_min, max_coast, rorder=None):
    """-> path [S, M+1, 3], steps, rgb, log [S, M, 14] (NaN where a strand made no step)"""
    roots, normals = np.ascontiguousarray(roots, np.float32), np.ascontiguousarray(normals, np.float32)
    S = roots.shape[0]
    path, steps = np.full((S, M + 1, 3), np.nan, np.float32), np.full(S, -1, np.int32)
    rgb, log = np.full((S, 3), np.nan, np.float32), np.full((S, M, 14), np.nan, np.float32)
    order, args = _cloud_args(L, cloud)
    ro = None if rorder is None else np.ascontiguousarray(rorder, np.int64)
    L.ghrsim_field_trace(*args, S, _p(roots), _p(normals), _p(ro), M, float(r2), float(np.float32(h)), float(np.float32(beta)),
                         float(np.float32(rho_min)), max_coast, _p(path), _p(steps), _p(rgb), _p(log))
    return path, steps, rgb, log


def resample(L_, path, steps, L):
    path, steps = np.ascontiguousarray(path, np.float32), np.ascontiguousarray(steps, np.int32)
    S, M = path.shape[0], path.shape[1] - 1
    out = np.full((S, L, 3), np.nan, np.float32)
    L_.ghrsim_strands_resample(S, M, L, _p(path), _p(steps), _p(out))
    return out
