"""`-m gpu`: tile scan, scatter, the tile sorts and the gradient walk at their list-length boundaries (tests/binning_cases.py:
scenes with exact list lengths, a numpy model of the binning; their ground is checked on the CPU in
tests/test_binning_cases_cpu.py).  Everything goes through the C ABI (GpuRun).

Every scene: tile rects against the reference's getRect formula, tile_start / keys / point_list against the model (bit for
bit), the gradient-slot layout, then forward -- and backward where stated -- against the oracle by the rules of
tests/helpers.py (fragile pixels left out of the image comparison, dL = 0 there).

  scene        what it pins
  sparse piles tile_sort_group<1,64> / <2,64> / <2,128> / <3,128> at 1 .. 1024 keys and tile_sort_wave_long (two and three
               LDS blocks, np2 2048 and 4096) at 1025 .. 3001, in a scene the host takes for sparse (R = 15 098 < 256 T);
               mask words of 64 (63 / 64 / 65), GHR_B3_LIST (511 / 512 / 513), GHR_B3_CACHE (2047 / 2048 / 2049); again with
               the fallback walk (GHR_K8=cell) and with the ordered walk (ghr_set_deterministic)
  dense piles  k_tile_sort_mid<512> (1025 .. 4096), k_tile_sort_big in one LDS block (.. 8192) and with global steps
               (.. 16 385), with GHR_NO_SORT_MID, GHR_TILE_ORDER=0 and =7: the same image, keys and lists, bit for bit
  rect areas   k_scatter's three ways with a rect (<= 4, 5 .. 8, > 8 tiles), the wave-uniform second turn, the
               two-instances-per-trip loop with a ragged last trip; k_tile_scan's scalar loads (15 tiles) and its vector
               loads with a scalar tail (28 tiles)
  many tiles   k_tile_scan's second round and its order from tile_start (T = 8280, 8281), next to T = 8192 exactly
  many rows    the gradient-slot scan in registers (4096 K1 workgroups) and through scan_1024 (4098)"""
import numpy as np
import pytest
import torch

from tests import binning_cases as bc
from tests import helpers as hp

pytestmark = pytest.mark.gpu

ENV_KNOBS = ("GHR_K8", "GHR_NO_SORT_MID", "GHR_TILE_ORDER")
_REF = {}          # scene -> inputs and oracle results, computed once
_DENSE_SEEN = {}   # environment -> (image, keys, point_list) of the dense piles
_ROWS = {}         # P -> the visible rows of many_rows(P)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)


def _reference(oracle_mod, name, build, backward=True):
    if name not in _REF:
        ri = build()
        out_o, radii_o, st_o = hp.oracle_forward(oracle_mod, ri, "B_sr")
        dL = ref = None
        if backward:
            dL = torch.randn(10, ri["H"], ri["W"], generator=torch.Generator().manual_seed(11)).numpy()
            dL[:, st_o.fragile.astype(bool)] = 0
            ref = hp.oracle_backward(oracle_mod, st_o, ri, dL, "B_sr")
        _REF[name] = (ri, out_o, radii_o, st_o, dL, ref)
    return _REF[name]


def _check_scene(run, out_o, radii_o, st_o):
    """The checks every scene gets; returns inspect()'s arrays."""
    from tests.test_gpu_parity import _check_forward
    ins = _check_forward(run, out_o, radii_o, st_o)
    gx, gy = (run.W + 15) // 16, (run.H + 15) // 16
    rects = ins["rects"]
    radii = run.radii.cpu().numpy()
    np.testing.assert_array_equal(rects[:, :2], bc.expected_rects(ins["rec"][:, 0:2], radii, gx, gy))
    model = bc.expected_binning(rects, ins["depths"].view(np.uint32), gx, gy)
    bc.assert_binning_equal(ins["tile_start"], ins["keys"], ins["point_list"], model)
    assert run.R == int(ins["tile_start"][-1])
    assert bc.check_slots(rects, run.P) == run.R
    return ins


def _run(oracle_mod, dev, name, build, backward=True):
    from tests.gpu_helpers import GpuRun, to_dev
    ri, out_o, radii_o, st_o, dL, ref = _reference(oracle_mod, name, build, backward)
    run = GpuRun(to_dev(ri, dev), "B_sr")
    ins = _check_scene(run, out_o, radii_o, st_o)
    if backward:
        hp.assert_grads_close(run.backward(torch.from_numpy(dL)), ref)
    return run, ins


def _counts(ins):
    return np.diff(ins["tile_start"].astype(np.int64))


def _assert_sparse(run, ins):
    counts, T = _counts(ins), 64
    want = np.zeros(T, np.int64)
    for tile, n in bc.sparse_counts():
        want[tile] = n
    np.testing.assert_array_equal(counts, want)
    assert run.R == 15098 < 256 * T
    assert {bc.sort_path(int(n), run.R, T) for n in counts if n > 1024} == {"tile_sort_wave_long"}


def test_sparse_piles_every_short_sort_and_the_long_wave_sort(oracle_mod, dev):
    run, ins = _run(oracle_mod, dev, "sparse", bc.sparse_piles)
    _assert_sparse(run, ins)


def test_sparse_piles_fallback_walk(oracle_mod, dev, monkeypatch):
    """k_render_bwd (GHR_K8=cell) over the same lists: its > 1024-instance path behind tile_sort_wave_long."""
    monkeypatch.setenv("GHR_K8", "cell")
    run, ins = _run(oracle_mod, dev, "sparse", bc.sparse_piles)
    _assert_sparse(run, ins)


def test_sparse_piles_ordered_walk_is_bit_reproducible(oracle_mod, dev):
    from gaussianhaircut_amd import _lib
    from tests.gpu_helpers import GpuRun, to_dev
    ri, out_o, radii_o, st_o, dL, ref = _reference(oracle_mod, "sparse", bc.sparse_piles)
    run = GpuRun(to_dev(ri, dev), "B_sr")
    _assert_sparse(run, _check_scene(run, out_o, radii_o, st_o))
    L = _lib.lib()
    assert L.ghr_set_deterministic(1) == 0
    try:
        runs = [run.backward(torch.from_numpy(dL)) for _ in range(2)]
    finally:
        assert L.ghr_set_deterministic(0) == 1
    hp.assert_grads_close(runs[0], ref)
    for k in runs[0]:
        assert np.array_equal(np.asarray(runs[0][k]).view(np.uint32), np.asarray(runs[1][k]).view(np.uint32)), k


@pytest.mark.parametrize("env", bc.DENSE_ENVS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()) or "default")
def test_dense_piles_mid_and_big_sorts_under_every_variant(oracle_mod, dev, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    run, ins = _run(oracle_mod, dev, "dense", bc.dense_piles)
    counts, T = _counts(ins), 16
    want = np.zeros(T, np.int64)
    for tile, n in bc.dense_counts():
        want[tile] = n
    np.testing.assert_array_equal(counts, want)
    assert run.R == 77826 >= 256 * T
    paths = {bc.sort_path(int(n), run.R, T, env) for n in counts if n}
    assert paths == {"tile_sort_group<3,128>", "k_tile_sort_big/lds", "k_tile_sort_big/global"} | \
        (set() if "GHR_NO_SORT_MID" in env else {"k_tile_sort_mid<512>"})
    # the variants choose launches and tile orders, never a result
    mine = (run.out.cpu().numpy(), ins["keys"], ins["point_list"])
    for other_env, other in _DENSE_SEEN.items():
        for a, b, what in zip(mine, other, ("image", "keys", "point_list")):
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                  b.view(np.uint32) if b.dtype == np.float32 else b), (what, env, other_env)
    _DENSE_SEEN[tuple(sorted(env.items()))] = mine


@pytest.mark.parametrize("W,H", bc.RECT_WH)
def test_rect_areas_three_ways_of_scatter(oracle_mod, dev, W, H):
    run, ins = _run(oracle_mod, dev, "rect_%d_%d" % (W, H), lambda: bc.rect_scene(W, H))
    area = bc.rect_areas(ins["rects"])
    assert set(area[area > 0].tolist()) == bc.RECT_AREAS[(W, H)]
    assert {bc.rect_class(int(a)) for a in area[area > 0]} == {"first turn", "second turn", "big"}
    big = area[128:256][area[128:256] > 8].sum()
    assert area[:128].max() <= 8 and big > 512 and big % 256 != 0


@pytest.mark.parametrize("W,H", bc.MANY_TILES_WH)
def test_many_tiles_across_the_scan_round(oracle_mod, dev, W, H):
    """Forward only.  The tile order itself is not visible from outside: what this pins is tile_start across the round
    boundary and that every tile's list is sorted and blended -- every tile was taken by exactly one workgroup."""
    run, ins = _run(oracle_mod, dev, "tiles_%d_%d" % (W, H), lambda: bc.many_tiles(W, H), backward=False)
    T = (W // 16) * (H // 16)
    want = np.zeros(T, np.int64)
    for tile, n in bc.many_tiles_counts(W, H):
        want[tile] = n
    np.testing.assert_array_equal(_counts(ins), want)
    assert bc.scan_paths(T, run.P)["rounds"] == (2 if T > 8192 else 1)
    assert want[0] and want[7] and want[8] and want[8191] and want[T - 1] and (T == 8192 or want[8192])


@pytest.mark.parametrize("P", bc.MANY_ROWS_P)
def test_many_k1_workgroups_slot_scan(oracle_mod, dev, P):
    def build():
        ri, _ROWS[P], _ = bc.many_rows(P)
        return ri

    run, ins = _run(oracle_mod, dev, "rows_%d" % P, build)
    rows = _ROWS[P]
    assert bc.scan_paths(16, P)["slots"] == ("registers" if P == 4096 * 256 else "scan_1024")
    radii = run.radii.cpu().numpy()
    vis = np.zeros(P, bool)
    vis[rows] = True
    assert (radii[vis] == 3).all() and (radii[~vis] == 0).all() and run.R == rows.size
    # the slot bases of the visible workgroups, first to last, are the running sum of their rows
    base = ins["rects"][rows, 3].astype(np.int64)
    blk = rows // 256
    per_blk = np.bincount(blk, minlength=(P + 255) // 256)
    np.testing.assert_array_equal(base, (np.cumsum(per_blk) - per_blk)[blk])
