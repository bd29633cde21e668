"""ctypes front of tests/hostsim/ghr_hostsim_grow.cpp: the host walk of csrc/ghr_grow.h's kernel on numpy arrays."""
import ctypes

import numpy as np

from tests import field_sim as fs
from tests import helpers as hp

DEPS = ["ghr_hostsim_field.cpp"] + fs.DEPS + ["ghr_grow.h", "ghr_meshdist.h", "ghr_mesh.h"]
LOG = 29  # GROW_LOG


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def load():
    so = hp.compile_hostsim("libghr_hostsim_grow.so", "ghr_hostsim_grow.cpp", ["-O1", "-fPIC", "-shared"], DEPS)
    L = ctypes.CDLL(so)
    vp, i64, i32, f = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float
    L.ghrsim_knn_keys.argtypes = [i64, vp, vp, vp]
    L.ghrsim_field_trace.argtypes = [i64] + [vp] * 5 + [i64, vp, vp, vp, i32, f, f, f, f, i32] + [vp] * 4
    L.ghrsim_grow_guarded.argtypes = [i64] + [vp] * 7 + [i64, vp, vp, vp, i32, f, f, f, f, i32, f, i32] + [vp] * 6
    for n in ("ghrsim_knn_keys", "ghrsim_field_trace", "ghrsim_grow_guarded"):
        getattr(L, n).restype = None
    return L


def trace(L, cloud, mesh, roots, normals, M, r2, h, beta, rho_min, max_coast, margin, rorder=None, seed=-1):
    """mesh: a HeadMesh (its two host blobs are the walk's tables).
    -> path [S, M+1, 3], steps, rgb, contacts, stop, log [S, M, LOG] (NaN where a strand made no step)"""
    roots, normals = np.ascontiguousarray(roots, np.float32), np.ascontiguousarray(normals, np.float32)
    S = roots.shape[0]
    path, steps = np.full((S, M + 1, 3), np.nan, np.float32), np.full(S, -1, np.int32)
    rgb, log = np.full((S, 3), np.nan, np.float32), np.full((S, M, LOG), np.nan, np.float32)
    contacts, stop = np.full(S, -1, np.int32), np.full(S, 255, np.uint8)
    order, args = fs._cloud_args(L, cloud)
    ro = None if rorder is None else np.ascontiguousarray(rorder, np.int64)
    tris, grid = np.ascontiguousarray(mesh.tris_blob()), np.ascontiguousarray(mesh.grid_blob())
    L.ghrsim_grow_guarded(*args, _p(tris), _p(grid), S, _p(roots), _p(normals), _p(ro), M, float(r2), float(np.float32(h)),
                          float(np.float32(beta)), float(np.float32(rho_min)), max_coast, float(np.float32(margin)), seed, _p(path),
                          _p(steps), _p(rgb), _p(contacts), _p(stop), _p(log))
    return path, steps, rgb, contacts, stop, log
