"""Scenes whose tile lists have EXACT lengths, and a plain numpy model of the binning stage (tile rects, per-tile lists
sorted by (depth bits, index), gradient-slot layout), for the tests of csrc/ghr_binning.h at its list-length boundaries
(tests/test_binning_cases_cpu.py on the CPU oracle, tests/test_gpu_binning_shapes.py on the device).

Nothing here calls project kernel code: the scenes are inputs (mode B_sr, like ``_manual_inputs`` of
tests/test_gpu_parity.py), the model is the reference's getRect formula and a lexicographic sort.

The thresholds the cases sit on are kept in ``THRESHOLDS``; the CPU test reads the ``#define``s (and the literals of
k_tile_sort's dispatch) out of the headers and compares, so that a changed constant fails there instead of silently moving
a boundary out of the cases."""
from __future__ import annotations

import math

import numpy as np
import torch

TILE = 16

# ---- thresholds of the path between projection and blending (names as in the headers) --------------------------------
THRESHOLDS = dict(
    SORT_1X64=128,                 # k_tile_sort: tile_sort_group<1,64> up to here (literal in the kernel)
    GHR_SORT_SOLO=256,             # ... <2,64>, wave 0 alone
    SORT_2X128=512,                # ... <2,128> (literal in the kernel)
    GHR_SORT_CAP=1024,             # ... <3,128>; beyond: tile_sort_wave_long / the dense-tile kernels
    GHR_SORT_MID_CAP=4096,         # k_tile_sort_mid<512>
    GHR_SORT_BIG_CAP=8192,         # k_tile_sort_big: one LDS block; beyond: global flip / disperse steps
    GHR_SORT_BIG_MIN_AVG=256,      # the host launches the dense-tile kernels when R >= this * T
    GHR_SORT_BLOCK=128,
    GHR_B3_SEG_WORDS=8,            # GHR_B3_LIST = 64 * this = 512 hits per segment of the gradient walk
    GHR_B3_CACHE=2048,             # the gradient walk keeps ids and masks in LDS up to here (SMALL)
    GHR_BIG_RECT=8,                # k_scatter: rects of more tiles are expanded by the whole workgroup
    GHR_SCAN_BLOCK=1024,           # k_tile_scan: rounds of 8 * this tiles; slot counts in registers up to 4 * this workgroups
    GHR_BLOCK=256,                 # rows of a K1 workgroup
)
MASK_WORD = 64                     # list positions per cell-mask word
B3_LIST = MASK_WORD * THRESHOLDS["GHR_B3_SEG_WORDS"]
SCAN_ROUND = 8 * THRESHOLDS["GHR_SCAN_BLOCK"]             # tiles per round of k_tile_scan
SCAN_REG_BLOCKS = 4 * THRESHOLDS["GHR_SCAN_BLOCK"]        # K1 workgroups whose slot counts k_tile_scan scans in registers
SMALL_RECT_FIRST_TURN = 4          # k_scatter: ordinals q, q + 2 in the first turn, q + 4, q + 6 in the second


def sort_path(n: int, R: int, T: int, env=None) -> str:
    """The sort a tile's list of n keys goes through in a scene of R instances on T tiles (ghr_forward_stage2)."""
    env = env or {}
    t = THRESHOLDS
    if n == 0:
        return "empty"
    if n <= t["SORT_1X64"]:
        return "tile_sort_group<1,64>"
    if n <= t["GHR_SORT_SOLO"]:
        return "tile_sort_group<2,64>"
    if n <= t["SORT_2X128"]:
        return "tile_sort_group<2,128>"
    if n <= t["GHR_SORT_CAP"]:
        return "tile_sort_group<3,128>"
    if R < t["GHR_SORT_BIG_MIN_AVG"] * T:
        return "tile_sort_wave_long"
    if n <= t["GHR_SORT_MID_CAP"] and env.get("GHR_NO_SORT_MID") is None:
        return "k_tile_sort_mid<512>"
    return "k_tile_sort_big/lds" if n <= t["GHR_SORT_BIG_CAP"] else "k_tile_sort_big/global"


def wave_long_blocks(n: int):
    """(LDS blocks of GHR_SORT_CAP keys, np2) of tile_sort_wave_long."""
    cap = THRESHOLDS["GHR_SORT_CAP"]
    np2 = cap
    while np2 < n:
        np2 <<= 1
    return (n + cap - 1) // cap, np2


def walk_path(n: int):
    """The gradient walk (k_render_bwd_cells) over a list of n: (SMALL or not, mask words, segments of GHR_B3_LIST)."""
    words = (n + MASK_WORD - 1) // MASK_WORD
    seg = THRESHOLDS["GHR_B3_SEG_WORDS"]
    return ("small" if n <= THRESHOLDS["GHR_B3_CACHE"] else "large", words, (words + seg - 1) // seg)


def scan_paths(T: int, P: int):
    """k_tile_scan: (load form, rounds, order from registers or from tile_start, slot scan in registers or scan_1024)."""
    nblk = (P + THRESHOLDS["GHR_BLOCK"] - 1) // THRESHOLDS["GHR_BLOCK"]
    return dict(load="vector+tail" if T % 4 == 0 and T % 8 else ("vector" if T % 4 == 0 else "scalar"),
                rounds=(T + SCAN_ROUND - 1) // SCAN_ROUND,
                order="registers" if T <= SCAN_ROUND else "tile_start",
                slots="registers" if nblk <= SCAN_REG_BLOCKS else "scan_1024", nblk=nblk)


def rect_class(area: int) -> str:
    """k_scatter's three ways with a rect."""
    if area <= SMALL_RECT_FIRST_TURN:
        return "first turn"
    return "second turn" if area <= THRESHOLDS["GHR_BIG_RECT"] else "big"


# ---- inputs ----------------------------------------------------------------------------------------------------------
def _grid(W, H):
    return (W + TILE - 1) // TILE, (H + TILE - 1) // TILE


def _inputs(W, H, px, py, z, scales, opac, colors):
    """Isotropic Gaussians at pixel (px, py), world depth z, in front of the front camera (at z = -4 looking down +z:
    z_view = z + 4): x = (px - (W - 1) / 2) * z_view / focal."""
    from gaussianhaircut_amd.scene.cameras import make_camera
    from gaussianhaircut_amd.utils import synthetic as syn
    cam = make_camera(W, H, device="cpu")
    tanx, tany = math.tan(float(cam.FoVx) * 0.5), math.tan(float(cam.FoVy) * 0.5)
    fx, fy = W / (2.0 * tanx), H / (2.0 * tany)
    zv = np.asarray(z, np.float64) + 4.0
    xyz = np.stack([(np.asarray(px, np.float64) - (W - 1) / 2.0) * zv / fx,
                    (np.asarray(py, np.float64) - (H - 1) / 2.0) * zv / fy, np.asarray(z, np.float64)], axis=1)
    P = xyz.shape[0]
    rot = torch.zeros(P, 4)
    rot[:, 0] = 1
    s = torch.from_numpy(np.asarray(scales, np.float32)).reshape(P, 1).expand(P, 3).contiguous()
    return dict(P=P, W=W, H=H, means3D=torch.from_numpy(xyz.astype(np.float32)), means2D=torch.zeros(P, 3),
                colors=torch.from_numpy(np.asarray(colors, np.float32)),
                opacities=torch.from_numpy(np.asarray(opac, np.float32)).reshape(P, 1), cov3D=torch.zeros(P, 6),
                conic=torch.zeros(P, 3), scales=s, rotations=rot, bg=syn.background(), viewmatrix=cam.world_view_transform,
                projmatrix=cam.full_proj_transform, tanfovx=tanx, tanfovy=tany, campos=cam.camera_center)


PILE_SCALE = 1e-4      # radius 3 whatever the focal length: cov2D = 0.3 (the low-pass) + ~0
PILE_DEPTHS = 7        # depths k / 128, exact in fp32: massive ties


def pile_opacity(n):
    return max(0.008, min(0.5, 40.0 / n))


def piles(W, H, counts, seed=0, opacity=None, behind=0, rows=None):
    """For every (tile, n) of `counts`: n tiny Gaussians (radius 3, a rect of exactly one tile) with centres inside the
    inner 10 x 10 pixels of the tile.  Rows are shuffled.  `behind`: that many more rows behind the camera (culled);
    `rows`: where the visible ones go among all P rows (sorted positions, default: a seeded shuffle)."""
    rng = np.random.default_rng(seed)
    gx, gy = _grid(W, H)
    px, py, op = [], [], []
    for tile, n in counts:
        assert 0 <= tile < gx * gy and n > 0
        px.append(TILE * (tile % gx) + 3.01 + 9.98 * rng.random(n))
        py.append(TILE * (tile // gx) + 3.01 + 9.98 * rng.random(n))
        op.append(np.full(n, opacity if opacity is not None else pile_opacity(n)))
    px, py, op = np.concatenate(px), np.concatenate(py), np.concatenate(op)
    nv = px.size
    z = rng.integers(0, PILE_DEPTHS, nv) / 128.0
    perm = rng.permutation(nv)
    px, py, op, z = px[perm], py[perm], op[perm], z[perm]
    P = nv + behind
    if behind:
        where = np.sort(rng.choice(P, nv, replace=False)) if rows is None else np.asarray(rows)
        assert where.size == nv

        def spread(v, fill):
            a = np.full(P, fill, np.float64)
            a[where] = v
            return a

        px, py, op, z = spread(px, (W - 1) / 2.0), spread(py, (H - 1) / 2.0), spread(op, 0.5), spread(z, -10.0)
    colors = rng.random((P, 10))
    return _inputs(W, H, px, py, z, np.full(P, PILE_SCALE), op, colors)


# ---- sparse / dense piles ----------------------------------------------------------------------------------------------
SPARSE_WH = (128, 128)
SPARSE_LENGTHS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 3001)
DENSE_WH = (64, 64)
DENSE_LENGTHS = (1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 16384, 16385)
DENSE_ENVS = ({}, {"GHR_NO_SORT_MID": "1"}, {"GHR_TILE_ORDER": "0"}, {"GHR_TILE_ORDER": "7"})


def _seeded_tiles(T, k, seed):
    return [int(t) for t in np.random.default_rng(seed).permutation(T)[:k]]


def sparse_counts():
    gx, gy = _grid(*SPARSE_WH)
    return list(zip(_seeded_tiles(gx * gy, len(SPARSE_LENGTHS), 11), SPARSE_LENGTHS))


def dense_counts():
    gx, gy = _grid(*DENSE_WH)
    return list(zip(_seeded_tiles(gx * gy, len(DENSE_LENGTHS), 12), DENSE_LENGTHS))


def sparse_piles():
    return piles(*SPARSE_WH, sparse_counts(), seed=21)


def dense_piles():
    # (the seed: 3 fragile pixels of 4096 on the oracle; seeds 22 .. 31 give 3 .. 12, the limit of 2e-3 is 8)
    return piles(*DENSE_WH, dense_counts(), seed=27)


# ---- many tiles --------------------------------------------------------------------------------------------------------
MANY_TILES_WH = ((2048, 1024), (1472, 1440), (1456, 1456))   # T = 8192 (one full round), 8280 (% 4 == 0), 8281 (odd)
MANY_TILES_PICKS = 300


def many_tiles_counts(W, H):
    gx, gy = _grid(W, H)
    T = gx * gy
    rng = np.random.default_rng(31 + T)
    must = [t for t in (0, 7, 8, SCAN_ROUND - 1, SCAN_ROUND, T - 1) if t < T]
    rest = [int(t) for t in rng.permutation(T)[:MANY_TILES_PICKS] if t not in must]
    tiles = sorted(set(must + rest))
    return [(t, int(rng.integers(1, 40))) for t in tiles]


def many_tiles(W, H):
    return piles(W, H, many_tiles_counts(W, H), seed=32, opacity=0.3)


# ---- many K1 workgroups ------------------------------------------------------------------------------------------------
MANY_ROWS_WH = (64, 64)
MANY_ROWS_P = (SCAN_REG_BLOCKS * 256, SCAN_REG_BLOCKS * 256 + 257)   # nblk = 4096 (registers), 4098 (scan_1024)
MANY_ROWS_BLOCKS = 12
MANY_ROWS_PER_BLOCK = 250


def many_rows_blocks(P):
    nblk = (P + 255) // 256
    rng = np.random.default_rng(41 + nblk)
    must = [0, SCAN_REG_BLOCKS - 1, nblk - 1]
    rest = [int(b) for b in rng.permutation(nblk)[:MANY_ROWS_BLOCKS] if b not in must][:MANY_ROWS_BLOCKS - len(set(must))]
    return sorted(set(must + rest))


def many_rows(P):
    """P rows, all behind the camera but MANY_ROWS_PER_BLOCK (fewer in a ragged last block) in each of the seeded K1
    workgroups of many_rows_blocks(P)."""
    W, H = MANY_ROWS_WH
    gx, gy = _grid(W, H)
    rng = np.random.default_rng(42)
    rows = []
    for b in many_rows_blocks(P):
        size = min(256, P - 256 * b)
        rows.append(256 * b + np.sort(rng.choice(size, min(MANY_ROWS_PER_BLOCK, size), replace=False)))
    rows = np.concatenate(rows)
    per_tile = np.bincount(rng.integers(0, gx * gy, rows.size), minlength=gx * gy)
    counts = [(t, int(n)) for t, n in enumerate(per_tile) if n]
    return piles(W, H, counts, seed=43, behind=P - rows.size, rows=rows), rows, counts


# ---- rect areas --------------------------------------------------------------------------------------------------------
RECT_WH = ((100, 52), (75, 40))       # 7 x 4 tiles (a multiple of 4), 5 x 3 (odd); ragged right and bottom edges
RECT_AREAS = {(100, 52): {1, 2, 3, 4, 5, 6, 8, 9, 10, 12, 16, 20, 28}, (75, 40): {1, 2, 3, 4, 5, 6, 8, 9, 10, 12, 15}}


def _span(p, r, g):
    """getRect along one axis for centres p (array), in float32 like the reference: (lo, hi) tile indices."""
    p, r = np.asarray(p, np.float32), np.float32(r)
    lo = np.trunc((p - r) / np.float32(TILE)).astype(np.int64)
    hi = np.trunc((p + r + np.float32(TILE - 1)) / np.float32(TILE)).astype(np.int64)
    return np.minimum(g, np.maximum(0, lo)), np.minimum(g, np.maximum(0, hi))


def _solve_rect(gx, gy, x0, x1, y0, y1):
    """(px, py, radius) of an isotropic Gaussian whose tile rect is [x0, x1) x [y0, y1): the smallest radius for which
    both axes have a centre, the centre in the middle of its range (eighths of a pixel); None if there is none (a rect
    much longer than wide has to be cut by a border)."""
    for r in range(3, 80):
        found = []
        for g, a, b in ((gx, x0, x1), (gy, y0, y1)):
            p = np.arange(-r - 16.0, TILE * g + r + 16.0, 0.25) + 0.125
            lo, hi = _span(p, r, g)
            ok = p[(lo == a) & (hi == b)]
            if ok.size == 0:
                break
            found.append(float(ok[ok.size // 2]))
        if len(found) == 2:
            return found[0], found[1], r
    return None


def _scale_for_radius(r, focal, zv):
    """World scale for which ceil(3 sqrt(lambda_max)) == r: lambda = var + sqrt(0.1), var = (s focal / z)^2 + 0.3; aimed
    at r - 0.5 (r = 3 is what the low-pass alone gives)."""
    var = ((r - 0.5) / 3.0) ** 2 - math.sqrt(0.1)
    return math.sqrt(max(var - 0.3, 1e-8)) * zv / focal


_SOLVED = {}


def rect_shapes(gx, gy):
    """(w, h) tile shapes by area on a gx x gy grid."""
    out = {}
    for w in range(1, gx + 1):
        for h in range(1, gy + 1):
            out.setdefault(w * h, []).append((w, h))
    return out


def rect_scene_specs(W, H):
    """The rows of rect_scene as tile rects (x0, x1, y0, y1), in row order (no shuffle: the arrangement is the point):
      rows   0 ..  31  areas <= 4 only                     | k_scatter: a wave that skips the second turn ...
      rows  32 ..  63  areas 1 .. 8, every second one 5..8 | ... and the next one, which takes it
      rows  64 .. 127  areas 1 .. 8 mixed
      rows 128 .. 255  big rects only (areas > 8), total > 512 and no multiple of 256: the two-instances-per-trip loop
                       of k_scatter takes a second trip and ends in a ragged one; the rest of the rows are culled
      rows 256 .. 300  everything mixed (a second K1 workgroup, a last wave of 13 rows)"""
    gx, gy = _grid(W, H)
    rng = np.random.default_rng(51 + gx)
    shapes = rect_shapes(gx, gy)
    areas = sorted(RECT_AREAS[(W, H)])
    first = [a for a in areas if a <= SMALL_RECT_FIRST_TURN]
    second = [a for a in areas if SMALL_RECT_FIRST_TURN < a <= THRESHOLDS["GHR_BIG_RECT"]]
    big = [a for a in areas if a > THRESHOLDS["GHR_BIG_RECT"]]

    def place(area, k):
        opts = shapes[area]
        for o in range(len(opts)):   # the k-th shape of that area, at a seeded position where a Gaussian can have that rect
            w, h = opts[(k + o) % len(opts)]
            spots = [(x, y) for x in range(gx - w + 1) for y in range(gy - h + 1)]
            for j in rng.permutation(len(spots)):
                x0, y0 = spots[j]
                s = (x0, x0 + w, y0, y0 + h)
                if s + (gx, gy) not in _SOLVED:
                    _SOLVED[s + (gx, gy)] = _solve_rect(gx, gy, *s)
                if _SOLVED[s + (gx, gy)] is not None:
                    return s
        raise ValueError((gx, gy, area))

    specs = [place(first[k % len(first)], k) for k in range(32)]
    specs += [place((second if k % 2 else first)[(k // 2) % len(second if k % 2 else first)], k) for k in range(32)]
    specs += [place((first + second)[k % len(first + second)], k) for k in range(64)]
    full = max(big)
    blk = [place(a, k) for k, a in enumerate(big)]
    total = sum((s[1] - s[0]) * (s[3] - s[2]) for s in blk)
    k = 0
    while total <= 2 * THRESHOLDS["GHR_BLOCK"] + 64 or total % THRESHOLDS["GHR_BLOCK"] == 0:
        a = full if k % 3 else big[k % len(big)]
        blk.append(place(a, k))
        total += a
        k += 1
    assert len(blk) <= 128
    while len(blk) < 128:   # the rest of the workgroup: culled rows (None)
        blk.append(None)
    order = rng.permutation(128)
    specs += [blk[i] for i in order]
    specs += [place(areas[k % len(areas)], k) for k in range(45)]
    return specs


def rect_scene(W, H):
    gx, gy = _grid(W, H)
    specs = rect_scene_specs(W, H)
    rng = np.random.default_rng(52 + gx)
    P = len(specs)
    from gaussianhaircut_amd.scene.cameras import make_camera
    cam = make_camera(W, H, device="cpu")
    focal = H / (2.0 * math.tan(float(cam.FoVy) * 0.5))
    z = rng.integers(0, PILE_DEPTHS, P) / 128.0
    px, py, sc, op = np.zeros(P), np.zeros(P), np.zeros(P), np.zeros(P)
    for i, s in enumerate(specs):
        if s is None:
            px[i], py[i], sc[i], op[i], z[i] = (W - 1) / 2.0, (H - 1) / 2.0, 0.01, 0.5, -10.0
            continue
        px[i], py[i], r = _SOLVED[s + (gx, gy)]
        sc[i] = _scale_for_radius(r, focal, z[i] + 4.0)
        op[i] = 0.6 if r <= 8 else (0.25 if r <= 24 else 0.04)
    return _inputs(W, H, px, py, z, sc, op, rng.random((P, 10)))


# ---- the model ---------------------------------------------------------------------------------------------------------
def expected_rects(xy, radii, gx, gy):
    """The reference's getRect (auxiliary.h), packed as the device keeps it: [P, 2] uint32 (x0 | x1 << 16, y0 | y1 << 16);
    rows with radius 0 (culled) and empty rects are 0."""
    xy = np.asarray(xy, np.float32)
    r = np.asarray(radii).astype(np.float32)
    blk = np.float32(TILE)

    def axis(p, g):
        lo = np.trunc((p - r) / blk).astype(np.int64)                       # (int): towards zero
        hi = np.trunc((p + r + np.float32(TILE - 1)) / blk).astype(np.int64)
        return np.minimum(g, np.maximum(0, lo)), np.minimum(g, np.maximum(0, hi))

    x0, x1 = axis(xy[:, 0], gx)
    y0, y1 = axis(xy[:, 1], gy)
    dead = (np.asarray(radii) <= 0) | ((x1 - x0) * (y1 - y0) == 0)
    out = np.stack([x0 | (x1 << 16), y0 | (y1 << 16)], axis=1).astype(np.uint32)
    out[dead] = 0
    return out


def unpack_rects(rects):
    rects = np.asarray(rects).astype(np.int64)
    return rects[:, 0] & 0xffff, rects[:, 0] >> 16, rects[:, 1] & 0xffff, rects[:, 1] >> 16


def rect_areas(rects):
    x0, x1, y0, y1 = unpack_rects(rects)
    return (x1 - x0) * (y1 - y0)


def expected_binning(rects, depth_bits, gx, gy):
    """(tile_start[T + 1] uint32, keys[R] uint64, point_list[R] uint32): per tile the Gaussians whose rect contains it, in
    the order of (depth bits, index); key = depth_bits << 32 | index."""
    x0, x1, y0, y1 = unpack_rects(rects)
    w, area = x1 - x0, (x1 - x0) * (y1 - y0)
    vis = np.nonzero(area > 0)[0]
    a = area[vis]
    rep = np.repeat(vis, a)
    ordinal = np.arange(int(a.sum())) - np.repeat(np.cumsum(a) - a, a)
    tile = (y0[rep] + ordinal // w[rep]) * gx + x0[rep] + ordinal % w[rep]
    key = (np.asarray(depth_bits).astype(np.uint64)[rep] << np.uint64(32)) | rep.astype(np.uint64)
    order = np.lexsort((key, tile))
    T = gx * gy
    tile_start = np.concatenate([[0], np.cumsum(np.bincount(tile, minlength=T))]).astype(np.uint32)
    return tile_start, key[order], rep[order].astype(np.uint32)


def assert_binning_equal(tile_start, keys, point_list, model):
    """Bit for bit against expected_binning's triple (`keys` may be None: the oracle keeps another key)."""
    m_start, m_keys, m_list = model
    np.testing.assert_array_equal(np.asarray(tile_start, np.uint32), m_start, err_msg="tile_start")
    np.testing.assert_array_equal(np.asarray(point_list, np.uint32), m_list, err_msg="point_list")
    if keys is not None:
        np.testing.assert_array_equal(np.asarray(keys, np.uint64), m_keys, err_msg="keys")


def ranges_to_tile_start(ranges):
    """The oracle's (reference's) `ranges` -- (0, 0) for an empty tile -- as tile_start[T + 1]."""
    ranges = np.asarray(ranges).astype(np.int64)
    n = ranges[:, 1] - ranges[:, 0]
    start = np.concatenate([[0], np.cumsum(n)])
    live = n > 0
    assert (ranges[live, 0] == start[:-1][live]).all(), "ranges are not tile-major"
    return start.astype(np.uint32)


def check_slots(rects, P):
    """The gradient-slot layout: the ranges [rects[:, 2] + rects[:, 3], + area) of the visible Gaussians partition [0, R);
    those of K1 workgroup b (rows 256 b .. 256 b + 255) form one contiguous block, and the blocks lie in ascending b (the
    order inside a block is free).  Returns R."""
    rects = np.asarray(rects)
    assert rects.shape == (P, 4)
    area = rect_areas(rects)
    vis = np.nonzero(area > 0)[0]
    R = int(area.sum())
    if vis.size == 0:
        return 0
    base = rects[vis, 2].astype(np.int64) + rects[vis, 3].astype(np.int64)
    a = area[vis]
    order = np.argsort(base, kind="stable")
    b, aa = base[order], a[order]
    assert b[0] == 0, "slots do not start at 0"
    assert (b[1:] == b[:-1] + aa[:-1]).all(), "slot ranges overlap or leave a gap"
    assert b[-1] + aa[-1] == R, "slot ranges do not end at R"
    blk = vis // THRESHOLDS["GHR_BLOCK"]
    nblk = (P + THRESHOLDS["GHR_BLOCK"] - 1) // THRESHOLDS["GHR_BLOCK"]
    total = np.bincount(blk, weights=a, minlength=nblk).astype(np.int64)
    lo = np.full(nblk, np.iinfo(np.int64).max)
    hi = np.zeros(nblk, np.int64)
    np.minimum.at(lo, blk, base)
    np.maximum.at(hi, blk, base + a)
    live = total > 0
    first = np.cumsum(total) - total
    assert (hi[live] - lo[live] == total[live]).all(), "a K1 workgroup's slots are not contiguous"
    assert (lo[live] == first[live]).all(), "the K1 workgroups' blocks are not in ascending order"
    return R
