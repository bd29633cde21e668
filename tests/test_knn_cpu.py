"""The key-ordered cloud and its pruned block walk (csrc/ghr_knn.h, csrc/ghr_nn.h) without a GPU.

tests/hostsim/ghr_hostsim_knn.cpp compiles both headers as plain C++ and walks k_knn_boxes, k_knn_search and k_nn_search with a
64-lane wave kept in arrays: the product's GHR_HD functions and policies, the cloud carved by the product's layout function in a
poisoned buffer, every index checked, no block twice per wave.  Here its results are compared ON BITS with the stated contracts,
brute force in numpy float32:

 1. the cross-cloud search (docstring of nearest.py): smallest d, then lowest index, both norms, every cloud kind of
    tests/chamfer_cases.py at the small shapes and across block and superblock boundaries;
 2. distCUDA2 (docstring of simple_knn/_C.py): j != i by index, three FLT_MAX slots with strict entry, ((b0 + b1) + b2) / 3;
 3. the key of one point: a flat axis, an overflowed extent, NaN bounds and a NaN coordinate give 0 on that axis;
 4. the pruning is the shipped kernel's: on the `random` clouds of tools/chamferstep.py the walks scan exactly the number of
    blocks the counter build of the kernel recorded on the GPU (profiles/chamfer.txt);
 5. both workspace-size entries of the built library return the bytes of the formulas they had before there was a layout function;
 6. the same walks in a stand-alone program built with -fsanitize=address,undefined (nothing sanitized is loaded here)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from tests import chamfer_cases as cc
from tests import helpers as hp

DEPS = ["ghr_hostsim_knn.cpp", "ghr_knn.h", "ghr_nn.h"]
FLT_MAX = np.float32(3.4028234663852886e38)
BOUNDARY_PY, BOUNDARY_PX = (4095, 4096, 4097, 8193), (1, 65, 4097)


@pytest.fixture(scope="module")
def sim():
    L = ctypes.CDLL(hp.compile_hostsim("libghr_hostsim_knn.so", "ghr_hostsim_knn.cpp", ["-O2", "-fPIC", "-shared"], DEPS))
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    L.ghrsim_knn_layout.argtypes = [ctypes.c_uint64, vp]
    L.ghrsim_knn_keys.argtypes = [i64, vp, vp, vp]
    L.ghrsim_knn_mean_dist2.argtypes = [i64, vp, vp, vp, vp]
    L.ghrsim_nn_search.argtypes = [i64, vp, vp, vp, i64, vp, vp, vp, i32, vp, vp, vp]
    assert L.ghrsim_knn_wave() == 64
    return L


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _f32(t):
    return np.ascontiguousarray(t.numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32)


def _bounds(*clouds):
    return np.concatenate((np.min([c.min(0) for c in clouds], 0), np.max([c.max(0) for c in clouds], 0))).astype(np.float32)


def _key_sort(sim, pts, bounds):
    """ghr_knn_keys and the stable sort of simple_knn._C on the host -> (order int64, sorted keys uint64)"""
    keys = np.zeros(len(pts), np.uint64)
    sim.ghrsim_knn_keys(len(pts), _p(pts), _p(bounds), _p(keys))
    order = np.argsort(keys.view(np.int64), kind="stable").astype(np.int64)
    return order, np.ascontiguousarray(keys[order])


def _search(sim, x, y, norm):
    """nearest.search_hip's sequence on the host -> dist, idx, blocks scanned per wave"""
    b = _bounds(x, y)
    (ox, kx), (oy, ky) = _key_sort(sim, x, b), _key_sort(sim, y, b)
    dist, idx = np.full(len(x), np.nan, np.float32), np.full(len(x), -1, np.int32)
    scanned = np.zeros((len(x) + 63) // 64, np.uint32)
    sim.ghrsim_nn_search(len(x), _p(x), _p(ox), _p(kx), len(y), _p(y), _p(oy), _p(ky), norm, _p(dist), _p(idx), _p(scanned))
    return dist, idx, scanned


def _dist2(sim, pts, order=None):
    """distCUDA2's sequence on the host -> mean of the three nearest, blocks scanned per wave"""
    if order is None:
        order, _ = _key_sort(sim, pts, _bounds(pts))
    out, scanned = np.full(len(pts), np.nan, np.float32), np.zeros((len(pts) + 63) // 64, np.uint32)
    sim.ghrsim_knn_mean_dist2(len(pts), _p(pts), _p(order), _p(out), _p(scanned))
    return out, scanned


def _pair_d(x, y, norm):
    with np.errstate(over="ignore"):
        dx, dy, dz = y[None, :, 0] - x[:, None, 0], y[None, :, 1] - x[:, None, 1], y[None, :, 2] - x[:, None, 2]
        return (dx * dx + dy * dy) + dz * dz if norm == 2 else (np.abs(dx) + np.abs(dy)) + np.abs(dz)


def brute_rule(x, y, norm, rows=256):
    """chamfer_cases.brute_rule vectorised: numpy float32, smallest d, and argmin takes the FIRST minimum = the lowest index"""
    dist, idx = np.zeros(len(x), np.float32), np.zeros(len(x), np.int32)
    for s in range(0, len(x), rows):
        d = _pair_d(x[s:s + rows], y, norm)
        assert d.dtype == np.float32
        j = d.argmin(1)
        dist[s:s + rows], idx[s:s + rows] = d[np.arange(len(j)), j], j
    return dist, idx


def brute_mean3(p, rows=256):
    """The contract of simple_knn/_C.py in numpy float32: every j != i, slots at FLT_MAX, strict entry, ((b0 + b1) + b2) / 3."""
    P = len(p)
    out = np.zeros(P, np.float32)
    for s in range(0, P, rows):
        d = _pair_d(p[s:s + rows], p, 2)
        n = len(d)
        d[np.arange(n), s + np.arange(n)] = np.inf                       # j != i, by index
        d = np.concatenate((np.minimum(d, FLT_MAX), np.full((n, 3), FLT_MAX, np.float32)), 1)   # what cannot enter leaves FLT_MAX
        b = np.sort(np.partition(d, 2, 1)[:, :3], 1)
        with np.errstate(over="ignore"):
            out[s:s + rows] = ((b[:, 0] + b[:, 1]) + b[:, 2]) / np.float32(3.0)
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
def _check_search(sim, kind, Px, Py):
    c = cc.cloud(kind, Px, Py)
    x, y = _f32(c["x"]), _f32(c["y"])
    for norm in (2, 1):
        want_d, want_i = brute_rule(x, y, norm)
        dist, idx, scanned = _search(sim, x, y, norm)
        assert np.array_equal(_bits(dist), _bits(want_d)), (kind, Px, Py, norm)
        assert np.array_equal(idx, want_i), (kind, Px, Py, norm)
        assert scanned.min() >= 1 and scanned.max() <= (Py + 63) // 64
        if c["idx"] is not None:
            assert np.array_equal(idx, c["idx"].numpy()) and not dist.any(), (kind, Px, Py, norm)


@pytest.mark.parametrize("kind", cc.KINDS)
def test_cross_cloud_search_on_the_small_shapes(sim, kind):
    for Px, Py in cc.SMALL_SHAPES:
        _check_search(sim, kind, Px, Py)


@pytest.mark.parametrize("Py", BOUNDARY_PY)
@pytest.mark.parametrize("kind", cc.KINDS)
def test_cross_cloud_search_across_superblock_boundaries(sim, kind, Py):
    for Px in BOUNDARY_PX:
        _check_search(sim, kind, Px, Py)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def _uniform(P, seed=5):
    return (np.random.default_rng(seed + P).random((P, 3), np.float32) * 2 - 1).astype(np.float32)


@pytest.mark.parametrize("P", (1, 2, 3, 4, 5, 63, 64, 65, 4095, 4096, 4097, 8193))
def test_distcuda2_contract_on_uniform_clouds(sim, P):
    p = _uniform(P)
    out, scanned = _dist2(sim, p)
    want = brute_mean3(p)
    assert np.array_equal(_bits(out), _bits(want))
    if P <= 2:
        assert np.isposinf(out).all()                                       # FLT_MAX + FLT_MAX
    if P == 3:
        assert (out > FLT_MAX / np.float32(3.1)).all() and np.isfinite(out).all()
    assert scanned.min() >= 1 and scanned.max() <= (P + 63) // 64


def test_distcuda2_on_exact_duplicates_skips_every_other_box(sim):
    base = _uniform(5, seed=9)
    p = np.ascontiguousarray(base[np.arange(4097) % 5])
    out, scanned = _dist2(sim, p)
    assert np.array_equal(_bits(out), _bits(brute_mean3(p))) and not out.any()
    # a wave whose block holds one base point only has b2 = 0 after it, and boxdist >= 0 skips every other box; the five runs of
    # equal keys have four boundaries, so at most four blocks are mixed
    assert int((scanned == 1).sum()) >= len(scanned) - 4


def test_distcuda2_when_every_key_is_equal(sim):
    p = _uniform(4097, seed=11)
    p[7], p[4000] = 3.0e38, -3.0e38                                        # every extent overflows: every axis gives 0
    keys = np.ones(len(p), np.uint64)
    sim.ghrsim_knn_keys(len(p), _p(p), _p(_bounds(p)), _p(keys))
    assert not keys.any()
    out, _ = _dist2(sim, p)
    assert np.array_equal(_bits(out), _bits(brute_mean3(p)))
    assert np.isposinf(out[[7, 4000]]).all() and np.isfinite(np.delete(out, [7, 4000])).all()   # an overflowed d enters nowhere


def test_distcuda2_of_a_permuted_cloud_is_the_permuted_result(sim):
    p = _uniform(4097, seed=13)
    perm = np.random.default_rng(2).permutation(len(p))
    out, _ = _dist2(sim, p)
    out_p, _ = _dist2(sim, np.ascontiguousarray(p[perm]))
    assert np.array_equal(_bits(out_p), _bits(out[perm]))
    # a caller's bad permutation entry is read as 0 and nothing leaves the buffers (the walks check every index)
    order, _ = _key_sort(sim, p, _bounds(p))
    order[5], order[-1] = -1, len(p)
    _dist2(sim, p, order)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
AXIS_BITS = (0x1249249249249249 << 2, 0x1249249249249249 << 1, 0x1249249249249249)   # x, y, z


def _morton(q):
    k = 0
    for a in range(3):
        for b in range(21):
            k |= ((int(q[a]) >> b) & 1) << (3 * b + 2 - a)
    return k


def _keys(sim, pts, bounds):
    pts, bounds = _f32(pts), _f32(bounds)
    keys = np.zeros(len(pts), np.uint64)
    sim.ghrsim_knn_keys(len(pts), _p(pts), _p(bounds), _p(keys))
    return [int(k) for k in keys]


def test_key_of_one_point(sim):
    top = np.float32(2097151.0)
    pts = np.array([[0, 0, 0], [1, 2, 4], [0.25, 1.0, 3.0], [-5, 9, -1], [1, 0, 0], [0, 2, 0], [0, 0, 4]], np.float32)
    b = np.array([0, 0, 0, 1, 2, 4], np.float32)
    scale = top / (b[3:] - b[:3])
    want = [_morton(np.clip((p - b[:3]) * scale, 0, top).astype(np.int64)) for p in pts]        # (float32 throughout)
    assert _keys(sim, pts, b) == want
    assert want[0] == 0 and want[1] == 2 ** 63 - 1 and want[3] == AXIS_BITS[1]                    # out of range: clamped
    assert [want[4], want[5], want[6]] == list(AXIS_BITS)
    big = np.float32(3.0e38)
    nan = np.float32(np.nan)
    for axis in range(3):
        others = AXIS_BITS[(axis + 1) % 3] | AXIS_BITS[(axis + 2) % 3]
        for lo, hi in ((b[axis], b[axis]), (-big, big), (nan, b[3 + axis]), (b[axis], nan), (nan, nan)):   # flat, overflowed, NaN bounds
            bb = b.copy()
            bb[axis], bb[3 + axis] = lo, hi
            got = _keys(sim, pts, bb)
            assert all(k & AXIS_BITS[axis] == 0 for k in got), (axis, lo, hi)
            assert [k & others for k in got] == [k & others for k in want], (axis, lo, hi)
        q = pts.copy()
        q[:, axis] = nan                                                                          # a NaN coordinate
        got = _keys(sim, q, b)
        assert all(k & AXIS_BITS[axis] == 0 for k in got) and [k & others for k in got] == [k & others for k in want]
    assert all(0 <= k < 2 ** 63 for k in _keys(sim, np.full((4, 3), np.inf, np.float32), b))


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_walks_scan_the_blocks_the_shipped_kernel_recorded(sim):
    """tools/chamferstep.py's `random` clouds (seed 1, 100 000 x 100 000) against the totals of the GHR_NN_COUNT_BLOCKS build of the
    kernel that shipped, profiles/chamfer.txt: 45649 blocks x -> y and 46075 y -> x, 1563 waves each."""
    with open(os.path.join(hp.ROOT, "profiles", "chamfer.txt")) as fh:
        recorded = fh.read()
    assert "random   x->y counter build: 45649 candidate blocks scanned by 1563 waves" in recorded
    assert "random   y->x counter build: 46075 candidate blocks scanned by 1563 waves" in recorded
    g = torch.Generator().manual_seed(1)
    x, y = _f32(torch.rand(100_000, 3, generator=g)), _f32(torch.rand(100_000, 3, generator=g))
    for a, b, total in ((x, y, 45649), (y, x, 46075)):
        dist, idx, scanned = _search(sim, a, b, 2)
        assert len(scanned) == 1563 and int(scanned.sum(dtype=np.int64)) == total
        want_d, want_i = brute_rule(a[:256], b, 2)
        assert np.array_equal(_bits(dist[:256]), _bits(want_d)) and np.array_equal(idx[:256], want_i)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 63, 64, 65, 4095, 4096, 4097, 8193, 262144, 262145, 2 ** 31 - 1)


def _up(x):
    return (x + 255) // 256 * 256


def _cloud_bytes_before(P):
    """ghr_capi.hip before the layout function: up(P * sizeof(float4)) + up(nb * 2 * sizeof(float4)) + up(ns * 2 * sizeof(float4))"""
    nb = (P + 63) // 64
    ns = (nb + 63) // 64
    return _up(P * 16) + _up(nb * 2 * 16) + _up(ns * 2 * 16)


def test_workspace_sizes_are_the_bytes_they_were(sim):
    L = _lib.lib()
    b = ctypes.c_size_t(0)
    for P in SIZES:
        assert L.ghr_knn_workspace_size(P, ctypes.byref(b)) == _lib.GHR_OK
        assert b.value == _cloud_bytes_before(P) + 256, P
        lay = np.zeros(6, np.uint64)
        sim.ghrsim_knn_layout(P, _p(lay))
        nb = (P + 63) // 64
        assert [int(v) for v in lay] == [nb, (nb + 63) // 64, 0, _up(P * 16), _up(P * 16) + _up(nb * 32), _cloud_bytes_before(P)]
        for Py in SIZES:
            rc = L.ghr_nn_workspace_size(P, Py, ctypes.byref(b))
            if Py == 0:
                assert rc == _lib.GHR_E_INVALID and b"Py == 0" in L.ghr_last_error()
            else:
                assert rc == _lib.GHR_OK and b.value == _cloud_bytes_before(P) + _cloud_bytes_before(Py) + 256, (P, Py)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
SELFCHECK = (("uniform", 1, 1, 2), ("uniform", 65, 4097, 2), ("lattice", 4097, 65, 1), ("duplicates", 64, 8193, 1), ("onecell", 63, 4096, 2),
             ("strands", 130, 2, 1))


def test_sanitized_stand_alone_program_runs_the_walks_clean(tmp_path):
    """ghr_knn_selfcheck: keys, boxes and both walks under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its
    own (exact-size buffers), against the brute-force bits."""
    san = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    if os.path.basename(hp.host_cxx()) == "g++":
        san += ["-static-libasan", "-static-libubsan"]
    exe = hp.compile_hostsim("ghr_knn_selfcheck_san", "ghr_knn_selfcheck.cpp", san, DEPS)
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as fh:
        for kind, Px, Py, norm in SELFCHECK:
            c = cc.cloud(kind, Px, Py)
            x, y = _f32(c["x"]), _f32(c["y"])
            dist, idx = brute_rule(x, y, norm)
            fh.write(np.array([Px, Py, norm], np.int32).tobytes())
            for arr in (x, y, dist, idx, brute_mean3(y)):
                fh.write(arr.tobytes())
    res = subprocess.run([exe, path], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "%d cases ok" % len(SELFCHECK) in res.stdout and "runtime error" not in res.stderr, res.stdout + res.stderr
