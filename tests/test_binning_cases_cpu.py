"""The ground of the binning boundary tests (tests/binning_cases.py), on the CPU: the threshold table is the headers', every
list length takes the path its case is there for, the scenes give the oracle exactly the lists they were built for (and its
walk reaches their tails), and the numpy model of the binning reproduces the oracle's own ranges and point lists bit for
bit -- and rejects a swapped tie or a shifted range."""
import os
import re
import time

import numpy as np
import pytest

from tests import binning_cases as bc
from tests import helpers as hp

CSRC = os.path.join(hp.ROOT, "gaussianhaircut_amd", "csrc")
FRAG_LIMIT = 2e-3   # tests/test_gpu_parity.py, _check_forward
_CACHE = {}


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_threshold_table_is_the_headers():
    src = _src("ghr_binning.h") + _src("ghr_render_bwd3.h") + _src("ghr_device.h")
    defs = dict(re.findall(r"^#define[ \t]+(GHR_\w+)[ \t]+(\d+)u?\b", src, flags=re.M))
    for name, value in bc.THRESHOLDS.items():
        if name.startswith("GHR_"):
            assert int(defs[name]) == value, name
    binning, host = _src("ghr_binning.h"), _src("ghr_capi.hip")
    # the literals of k_tile_sort's dispatch, and what the instantiations' capacities come to
    assert re.search(r"if \(n <= %du\) tile_sort_group<1, 64," % bc.THRESHOLDS["SORT_1X64"], binning)
    assert re.search(r"if \(n <= GHR_SORT_SOLO\) \{", binning)
    assert re.search(r"if \(n <= %du\) tile_sort_group<2, 128," % bc.THRESHOLDS["SORT_2X128"], binning)
    assert re.search(r"else if \(n <= %du\) tile_sort_group<3, 128," % bc.THRESHOLDS["GHR_SORT_CAP"], binning)
    assert "k_tile_sort<%d>" % bc.THRESHOLDS["GHR_SORT_CAP"] in host
    assert "k_tile_sort_mid<%d>" % (bc.THRESHOLDS["GHR_SORT_MID_CAP"] // 8) in host and "(uint32_t)NT << 3" in binning
    assert "(size_t)R >= (size_t)GHR_SORT_BIG_MIN_AVG * (size_t)T" in host
    assert 'getenv("GHR_NO_SORT_MID") == nullptr' in host and 'getenv("GHR_TILE_ORDER")' in host
    assert re.search(r"#define GHR_B3_LIST \(64 \* GHR_B3_SEG_WORDS\)", _src("ghr_render_bwd3.h"))
    assert "n <= GHR_B3_CACHE" in _src("ghr_render_bwd3.h")
    # k_tile_scan: rounds of 8 * GHR_SCAN_BLOCK tiles, four slot counts per thread in registers; k_scatter's second turn
    assert "base += 8u * GHR_SCAN_BLOCK" in binning and "(uint32_t)T <= 8u * GHR_SCAN_BLOCK" in binning
    assert "per_b <= 4;" in binning and "(T & 3) == 0 && t0 + 8u <= (uint32_t)T" in binning
    assert "ballot_w64(area > %d)" % bc.SMALL_RECT_FIRST_TURN in binning and "full > GHR_BIG_RECT" in binning
    assert bc.B3_LIST == 512 and bc.SCAN_ROUND == 8192 and bc.SCAN_REG_BLOCKS == 4096


def test_every_length_takes_the_path_its_case_names():
    T, R = 64, sum(bc.SPARSE_LENGTHS)
    assert R == 15098 and R < 256 * T == 16384
    g = "tile_sort_group<%s>"
    want = [g % "1,64"] * 6 + [g % "2,64"] * 3 + [g % "2,128"] * 3 + [g % "3,128"] * 3 + ["tile_sort_wave_long"] * 5
    assert [bc.sort_path(n, R, T) for n in bc.SPARSE_LENGTHS] == want
    assert [bc.wave_long_blocks(n) for n in bc.SPARSE_LENGTHS[-5:]] == [(2, 2048), (2, 2048), (2, 2048), (3, 4096), (3, 4096)]
    T, R = 16, sum(bc.DENSE_LENGTHS)
    assert R == 77826 and R >= 256 * T
    mid, lds, glob = "k_tile_sort_mid<512>", "k_tile_sort_big/lds", "k_tile_sort_big/global"
    want = [g % "3,128"] + [mid] * 6 + [lds] * 3 + [glob] * 3
    for env in bc.DENSE_ENVS:
        got = [bc.sort_path(n, R, T, env) for n in bc.DENSE_LENGTHS]
        assert got == ([w if w != mid else lds for w in want] if "GHR_NO_SORT_MID" in env else want), env
    # every path of the table has a case
    named = {bc.sort_path(n, sum(bc.SPARSE_LENGTHS), 64) for n in bc.SPARSE_LENGTHS} | \
            {bc.sort_path(n, sum(bc.DENSE_LENGTHS), 16) for n in bc.DENSE_LENGTHS}
    assert named == {g % "1,64", g % "2,64", g % "2,128", g % "3,128", "tile_sort_wave_long", mid, lds, glob}
    # the gradient walk: one segment up to GHR_B3_LIST hits, ids and masks in LDS up to GHR_B3_CACHE, words of 64
    walks = {n: bc.walk_path(n) for n in bc.SPARSE_LENGTHS + bc.DENSE_LENGTHS}
    assert walks[63] == ("small", 1, 1) and walks[64] == ("small", 1, 1) and walks[65] == ("small", 2, 1)
    assert walks[511][1:] == (8, 1) and walks[512][1:] == (8, 1) and walks[513][1:] == (9, 2)
    assert walks[2047] == ("small", 32, 4) and walks[2048] == ("small", 32, 4) and walks[2049] == ("large", 33, 5)
    assert walks[16385] == ("large", 257, 33)
    # k_tile_scan: both load forms, one and two rounds, both slot scans
    scans = {(W, H): bc.scan_paths((W // 16) * (H // 16), 1000) for W, H in bc.MANY_TILES_WH}
    assert [(s["load"], s["rounds"], s["order"]) for s in scans.values()] == \
        [("vector", 1, "registers"), ("vector", 2, "tile_start"), ("scalar", 2, "tile_start")]
    assert bc.scan_paths(28, 301)["load"] == "vector+tail" and bc.scan_paths(15, 301)["load"] == "scalar"
    assert bc.scan_paths(64, 1000)["load"] == "vector" and bc.scan_paths(16, 1000)["load"] == "vector"
    assert [bc.scan_paths(16, P)["slots"] for P in bc.MANY_ROWS_P] == ["registers", "scan_1024"]
    assert [bc.scan_paths(16, P)["nblk"] for P in bc.MANY_ROWS_P] == [4096, 4098]
    # k_scatter's three ways with a rect
    for wh, areas in bc.RECT_AREAS.items():
        assert {bc.rect_class(a) for a in areas} == {"first turn", "second turn", "big"}
    assert [bc.rect_class(a) for a in (4, 5, 8, 9)] == ["first turn", "second turn", "second turn", "big"]


# ---- the scenes on the oracle ----------------------------------------------------------------------------------------
def _scene(name):
    if name == "sparse":
        return bc.sparse_piles(), bc.sparse_counts()
    if name == "dense":
        return bc.dense_piles(), bc.dense_counts()
    kind, a, b = name.split("_")
    if kind == "tiles":
        return bc.many_tiles(int(a), int(b)), bc.many_tiles_counts(int(a), int(b))
    if kind == "rect":
        return bc.rect_scene(int(a), int(b)), None
    raise KeyError(name)


def _oracle(oracle_mod, name):
    if name not in _CACHE:
        ri, counts = _scene(name)
        t0 = time.perf_counter()
        out, radii, st = hp.oracle_forward(oracle_mod, ri, "B_sr")
        _CACHE[name] = (ri, counts, out, radii, st, time.perf_counter() - t0)
    return _CACHE[name]


def _tile_counts(st):
    return (st.ranges[:, 1].astype(np.int64) - st.ranges[:, 0]).reshape(-1)


def _tail_reached(st, W, H, counts):
    """Per (tile, n): the largest n_contrib among the tile's pixels lies in the last 64 list positions."""
    gx = (W + 15) // 16
    nc = st.n_contrib.reshape(H, W).astype(np.int64)
    for tile, n in counts:
        ty, tx = divmod(tile, gx)
        reach = nc[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16].max()
        assert reach >= 1 and reach > n - 64, (tile, n, int(reach))


def _model_is_the_oracle(st, W, H):
    gx, gy = (W + 15) // 16, (H + 15) // 16
    rects = bc.expected_rects(st.xy, st.radii, gx, gy)
    assert bc.rect_areas(rects).sum() == st.num_rendered
    np.testing.assert_array_equal(bc.rect_areas(rects), st.tiles_touched.astype(np.int64) * (st.radii > 0))
    model = bc.expected_binning(rects, st.depths.view(np.uint32), gx, gy)
    bc.assert_binning_equal(bc.ranges_to_tile_start(st.ranges), None, st.point_list, model)
    pl = st.point_list.astype(np.uint64)
    np.testing.assert_array_equal(model[1], (st.depths.view(np.uint32).astype(np.uint64)[pl] << np.uint64(32)) | pl)
    return rects, model


PILE_SCENES = ["sparse", "dense"] + ["tiles_%d_%d" % wh for wh in bc.MANY_TILES_WH]


@pytest.mark.parametrize("name", PILE_SCENES)
def test_pile_scene_gives_the_oracle_the_intended_lists(oracle_mod, name):
    ri, counts, out, radii, st, secs = _oracle(oracle_mod, name)
    W, H = ri["W"], ri["H"]
    T = ((W + 15) // 16) * ((H + 15) // 16)
    assert (radii == 3).all() and (st.tiles_touched == 1).all()      # radius 3, a rect of exactly one tile
    want = np.zeros(T, np.int64)
    for tile, n in counts:
        want[tile] = n
    np.testing.assert_array_equal(_tile_counts(st), want)
    R = st.num_rendered
    if name == "sparse":
        assert len({t for t, _ in counts}) == 20 and R == 15098 and R < 256 * T
        assert {bc.sort_path(n, R, T) for _, n in counts if n > 1024} == {"tile_sort_wave_long"}
    elif name == "dense":
        assert len({t for t, _ in counts}) == 13 and R == 77826 and R >= 256 * T
        assert not any(bc.sort_path(n, R, T) == "tile_sort_wave_long" for _, n in counts)
    else:
        tiles = {t for t, _ in counts}
        assert {0, 7, 8, 8191, T - 1} <= tiles and (8192 in tiles) == (T > 8192) and 280 <= len(tiles) <= 310
        assert all(1 <= n <= 39 for _, n in counts) and R < 256 * T
        ts = bc.ranges_to_tile_start(st.ranges)
        if T > 8192:   # tile_start carries on across the round boundary
            assert ts[8192] == want[:8192].sum() > 0 and ts[T] - ts[8192] == want[8192:].sum() > 0
    frag = st.fragile.mean()
    assert frag <= FRAG_LIMIT, frag
    _tail_reached(st, W, H, counts)
    _model_is_the_oracle(st, W, H)
    print("%s: R %d, fragile share %.2e, oracle forward %.2f s" % (name, R, frag, secs))


@pytest.mark.parametrize("W,H", bc.RECT_WH)
def test_rect_scene_has_the_intended_areas_in_the_intended_rows(oracle_mod, W, H):
    ri, _, out, radii, st, secs = _oracle(oracle_mod, "rect_%d_%d" % (W, H))
    gx, gy = (W + 15) // 16, (H + 15) // 16
    assert (gx, gy) == {(100, 52): (7, 4), (75, 40): (5, 3)}[(W, H)] and W % 16 and H % 16
    rects, model = _model_is_the_oracle(st, W, H)
    specs = bc.rect_scene_specs(W, H)
    x0, x1, y0, y1 = bc.unpack_rects(rects)
    for i, s in enumerate(specs):
        assert (x0[i], x1[i], y0[i], y1[i]) == (s if s is not None else (0, 0, 0, 0)), (i, s)
        assert (radii[i] > 0) == (s is not None)
    area = bc.rect_areas(rects)
    assert set(area[area > 0].tolist()) == bc.RECT_AREAS[(W, H)]
    P = len(specs)
    assert P == 301 and P % 32 == 13
    # (a) a wave's 32 rows without a second turn, the next wave's with one
    assert area[0:32].max() <= 4 and area[0:32].min() >= 1
    assert ((area[32:64] > 4) & (area[32:64] <= 8)).any() and area[32:64].max() <= 8 and (area[32:64] <= 4).any()
    # (b) the big rects of one k_scatter workgroup (128 rows), which is also all its K1 workgroup (256 rows) has
    assert area[:128].max() <= 8
    big = area[128:256][area[128:256] > 8].sum()
    assert (area[128:256] <= 8).sum() == (area[128:256] == 0).sum()      # big rects and culled rows only
    assert big > 512 and big % 256 != 0   # a second trip of the two-instances-per-thread loop, and a ragged last one
    assert (area[256:] > 8).any() and (area[256:] <= 4).any()
    # (c) rects the image border cuts, on each side: the splat's pixel box reaches past the border its rect ends at
    live = radii > 0
    px, py, r = st.xy[:, 0], st.xy[:, 1], radii
    assert (live & (px - r < 0) & (x0 == 0)).any() and (live & (px + r > W - 1) & (x1 == gx)).any()
    assert (live & (py - r < 0) & (y0 == 0)).any() and (live & (py + r > H - 1) & (y1 == gy)).any()
    frag = st.fragile.mean()
    assert frag <= FRAG_LIMIT, frag
    covered = (st.n_contrib > 0).mean()
    assert covered > 0.5, covered
    print("rect %dx%d: R %d, fragile share %.2e, %.0f %% of the pixels blended, oracle forward %.2f s" %
          (W, H, st.num_rendered, frag, 100 * covered, secs))


@pytest.mark.parametrize("P", bc.MANY_ROWS_P)
def test_many_rows_scene_and_the_oracle_time_at_that_size(oracle_mod, P):
    ri, rows, counts = bc.many_rows(P)
    blocks = bc.many_rows_blocks(P)
    nblk = (P + 255) // 256
    assert ri["P"] == P and {0, 4095, nblk - 1} <= set(blocks) and len(blocks) == bc.MANY_ROWS_BLOCKS
    assert 2500 <= rows.size <= 3000 and (np.unique(rows // 256) == np.array(blocks)).all()
    t0 = time.perf_counter()
    out, radii, st = hp.oracle_forward(oracle_mod, ri, "B_sr")
    dL = np.random.default_rng(1).standard_normal((10, ri["H"], ri["W"])).astype(np.float32)
    dL[:, st.fragile.astype(bool)] = 0
    ref = hp.oracle_backward(oracle_mod, st, ri, dL, "B_sr")
    secs = time.perf_counter() - t0
    vis = np.zeros(P, bool)
    vis[rows] = True
    assert (radii[vis] == 3).all() and (radii[~vis] == 0).all()
    want = np.zeros(16, np.int64)
    for tile, n in counts:
        want[tile] = n
    np.testing.assert_array_equal(_tile_counts(st), want)
    assert st.num_rendered == rows.size and st.fragile.mean() <= FRAG_LIMIT
    assert not ref["dL_dopacity"][~vis].any() and (ref["dL_dopacity"][vis] != 0).mean() > 0.9
    _tail_reached(st, ri["W"], ri["H"], counts)
    _model_is_the_oracle(st, ri["W"], ri["H"])
    print("rows %d: fragile share %.2e, oracle forward + backward %.2f s" % (P, st.fragile.mean(), secs))
    assert secs < 10.0   # "within a few seconds": what lets the GPU test keep the oracle comparison at this P


@pytest.mark.parametrize("name", ["sparse", "dense"])
def test_pile_gradients_reach_nearly_every_gaussian(oracle_mod, name):
    ri, counts, out, radii, st, _ = _oracle(oracle_mod, name)
    dL = np.random.default_rng(2).standard_normal((10, ri["H"], ri["W"])).astype(np.float32)
    dL[:, st.fragile.astype(bool)] = 0
    ref = hp.oracle_backward(oracle_mod, st, ri, dL, "B_sr")
    assert (ref["dL_dopacity"] != 0).mean() > 0.95


def test_model_comparison_rejects_a_swapped_tie_and_a_shifted_range(oracle_mod):
    ri, counts, out, radii, st, _ = _oracle(oracle_mod, "sparse")
    rects, model = _model_is_the_oracle(st, ri["W"], ri["H"])
    ts = bc.ranges_to_tile_start(st.ranges)
    bits = st.depths.view(np.uint32)
    pl = st.point_list.copy()
    # two neighbours of equal depth inside one tile's list
    inside = np.ones(pl.size - 1, bool)
    inside[ts[1:-1][(ts[1:-1] > 0) & (ts[1:-1] < pl.size)] - 1] = False
    ties = np.nonzero(inside & (bits[pl[:-1]] == bits[pl[1:]]))[0]
    assert ties.size > 1000
    for i in (int(ties[0]), int(ties[-1])):
        bad = pl.copy()
        bad[i], bad[i + 1] = pl[i + 1], pl[i]
        with pytest.raises(AssertionError, match="point_list"):
            bc.assert_binning_equal(ts, None, bad, model)
        keys = model[1].copy()
        keys[i], keys[i + 1] = keys[i + 1], keys[i]
        with pytest.raises(AssertionError, match="keys"):
            bc.assert_binning_equal(ts, keys, pl, model)
    for t, d in ((1, 1), (len(ts) // 2, -1), (len(ts) - 1, 1)):
        bad = ts.copy()
        bad[t] = np.uint32(int(ts[t]) + d)
        with pytest.raises(AssertionError, match="tile_start"):
            bc.assert_binning_equal(bad, model[1], pl, model)
    bc.assert_binning_equal(ts, model[1], pl, model)
    # a dropped last key: the list one short
    with pytest.raises(AssertionError):
        bc.assert_binning_equal(ts, None, pl[:-1], model)


def test_check_slots_accepts_any_order_inside_a_workgroup_and_nothing_else():
    rng = np.random.default_rng(3)
    P = 700
    w, h = rng.integers(0, 4, P), rng.integers(1, 4, P)
    area = w * h
    rects = np.zeros((P, 4), np.uint32)
    rects[:, 0] = (2 + w) << 16 | 2
    rects[:, 1] = (1 + h) << 16 | 1
    rects[area == 0, :2] = 0
    blk = np.arange(P) // 256
    tot = np.bincount(blk, weights=area).astype(np.int64)
    rects[:, 3] = (np.cumsum(tot) - tot)[blk]
    for b in range(3):   # a random order inside each workgroup
        rows = np.nonzero(blk == b)[0]
        rows = rows[rng.permutation(rows.size)]
        rects[rows, 2] = np.cumsum(area[rows]) - area[rows]
    assert bc.check_slots(rects, P) == area.sum()
    vis = np.nonzero(area > 0)[0]
    bad = rects.copy()
    bad[vis[5], 2] += 1
    with pytest.raises(AssertionError):
        bc.check_slots(bad, P)
    bad = rects.copy()   # two workgroups' blocks exchanged: still a partition, but not in ascending order
    bad[blk == 0, 3], bad[blk == 1, 3] = tot[1], 0
    with pytest.raises(AssertionError, match="ascending|contiguous"):
        bc.check_slots(bad, P)
