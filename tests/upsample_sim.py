"""ctypes front of tests/hostsim/ghr_hostsim_upsample.cpp: the host walk of csrc/ghr_upsample.h's kernels on numpy arrays."""
import ctypes

import numpy as np

from tests import helpers as hp

DEPS = ["ghr_upsample.h", "ghr_shape.h"]


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def load():
    so = hp.compile_hostsim("libghr_hostsim_upsample.so", "ghr_hostsim_upsample.cpp", ["-O1", "-fPIC", "-shared"], DEPS)
    L = ctypes.CDLL(so)
    vp, i32, f = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    L.ghrsim_ups_near.argtypes = [i32, vp, i32, vp, f, vp, vp]
    L.ghrsim_ups_blend.argtypes = [i32, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp, f, f, i32, vp, vp, vp, vp]
    L.ghrsim_ups_near.restype = None
    L.ghrsim_ups_blend.restype = None
    return L


def near(L, guide_roots, child_origins, r2=np.inf):
    """-> nbr [N, 4] int32, nd2 [N, 4] float32"""
    gr = np.ascontiguousarray(guide_roots, np.float32).reshape(-1, 3)
    co = np.ascontiguousarray(child_origins, np.float32).reshape(-1, 3)
    N = co.shape[0]
    nbr, nd2 = np.full((N, 4), -7, np.int32), np.full((N, 4), np.nan, np.float32)
    L.ghrsim_ups_near(gr.shape[0], _p(gr), N, _p(co), float(np.float32(r2)), _p(nbr), _p(nd2))
    return nbr, nd2


def blend(L, gp, gM, gf, co, cM, nbr, nd2, eps2, tau):
    """tau None: the gate off.  -> dict(points [N, L, 3], weights [N, 4], features [N, F], valid [N] uint8)"""
    gp, gM = np.ascontiguousarray(gp, np.float32), np.ascontiguousarray(gM, np.float32)
    co, cM = np.ascontiguousarray(co, np.float32), np.ascontiguousarray(cM, np.float32)
    nbr, nd2 = np.ascontiguousarray(nbr, np.int32), np.ascontiguousarray(nd2, np.float32)
    G, Lp = gp.shape[:2]
    N = co.shape[0]
    gf = None if gf is None else np.ascontiguousarray(gf, np.float32).reshape(G, -1)
    F = 0 if gf is None else gf.shape[1]
    out, w = np.full((N, Lp, 3), np.nan, np.float32), np.full((N, 4), np.nan, np.float32)
    of, valid = np.full((N, F), np.nan, np.float32), np.full(N, 7, np.uint8)
    L.ghrsim_ups_blend(G, Lp, _p(gp), _p(gM), _p(gf) if F else None, F, N, _p(co), _p(cM), _p(nbr), _p(nd2), float(np.float32(eps2)),
                       0.0 if tau is None else float(np.float32(tau)), 0 if tau is None else 1, _p(out), _p(w), _p(of) if F else None,
                       _p(valid))
    return dict(points=out, weights=w, features=of, valid=valid)
