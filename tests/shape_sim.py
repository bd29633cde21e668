"""ctypes front of tests/hostsim/ghr_hostsim_shape.cpp: the host walk of csrc/ghr_shape.h's kernels on numpy arrays."""
import ctypes

import numpy as np

from tests import helpers as hp

DEPS = ["ghr_shape.h"]


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def load():
    so = hp.compile_hostsim("libghr_hostsim_shape.so", "ghr_hostsim_shape.cpp", ["-O1", "-fPIC", "-shared"], DEPS)
    L = ctypes.CDLL(so)
    vp, i32, i64, f = ctypes.c_void_p, ctypes.c_int32, ctypes.c_longlong, ctypes.c_float
    L.ghrsim_shape_dead.restype = f
    L.ghrsim_shape_neighbours.argtypes = [i32, vp, f, vp]
    L.ghrsim_shape_forward.argtypes = [i32, i32, vp, vp, vp, i64, vp, vp]
    L.ghrsim_shape_backward.argtypes = [i32, i32, vp, vp, vp, vp, vp, i64, i64, vp, vp]
    for n in ("ghrsim_shape_neighbours", "ghrsim_shape_forward", "ghrsim_shape_backward"):
        getattr(L, n).restype = None
    return L


def neighbours(L, roots, r2=np.inf):
    roots = np.ascontiguousarray(roots, np.float32).reshape(-1, 3)
    nbr = np.full((roots.shape[0], 4), -7, np.int32)
    L.ghrsim_shape_neighbours(roots.shape[0], _p(roots), float(np.float32(r2)), _p(nbr))
    return nbr


def forward(L, dirs, rest, nbr):
    """-> partial [S, 3], E [3]"""
    dirs, rest, nbr = np.ascontiguousarray(dirs, np.float32), np.ascontiguousarray(rest, np.float32), np.ascontiguousarray(nbr, np.int32)
    S, n = dirs.shape[:2]
    partial, E = np.full((S, 3), np.nan, np.float32), np.full(3, np.nan, np.float32)
    L.ghrsim_shape_forward(S, n, _p(dirs), _p(rest), _p(nbr), int((nbr >= 0).sum()), _p(partial), _p(E))
    return partial, E


def backward(L, dirs, rest, nbr, start, lists, dE):
    dirs, rest, nbr = np.ascontiguousarray(dirs, np.float32), np.ascontiguousarray(rest, np.float32), np.ascontiguousarray(nbr, np.int32)
    start, lists = np.ascontiguousarray(start, np.int32), np.ascontiguousarray(lists, np.int32)
    dE = np.ascontiguousarray(dE, np.float32)
    S, n = dirs.shape[:2]
    out = np.full((S, n, 3), np.nan, np.float32)
    buf = lists if lists.size else np.zeros(1, np.int32)
    L.ghrsim_shape_backward(S, n, _p(dirs), _p(rest), _p(nbr), _p(start), _p(buf), lists.size, int((nbr >= 0).sum()), _p(dE), _p(out))
    return out
