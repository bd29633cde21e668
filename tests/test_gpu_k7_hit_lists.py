"""`-m gpu`: k_render_fwd's per-cell hit lists (csrc/ghr_render_fwd.h) against the walk they replace and against the oracle.

The compositing kernel walks, per 64-entry word of a tile's list, the hits of each 4x4-pixel cell from a list in LDS that the
wave builds from its four ballots; ``GHR_K7_WALK=mask`` (read per call) selects the form before, which enumerates the bits of
the cell's 64-bit mask step by step.  Both must see the same entries in the same order, so every case runs twice:

  list walk against the mask walk   bit for bit: the ten output planes, final_T, n_contrib, and -- under
                                    ghr_set_deterministic(1) -- all eight gradient tensors of a backward pass (the gradient walk
                                    reads the cell-mask words and the per-cell last contributor the forward kernel leaves)
  list walk against the oracle      by the rules of tests/helpers.py: n_contrib exact, image and final_T within 1e-4, fragile
                                    pixels left out

Scenes are hand-built (mode A: the conics are given, and the projection takes a Gaussian's radius from its conic), 3 x 2 tiles
at 48 x 32 (whole tiles) and 37 x 21 pixels (a 5-pixel column of tiles and a 5-pixel row: partial tiles and partial cells).  An
entry is LOCAL -- radius <= 3 (variance <= 1) with its centre in the inner 10 x 10 pixels of a tile, or radius <= 6 in the inner
4 x 4: its rect is that tile -- or GLOBAL: so wide that its rect is the whole image, which is the only way a nearly singular or
extremely anisotropic conic comes.  A tile's list is the globals plus its own locals, in the order of their depths:

  lengths_a  lists of 0, 1, 63, 64, 65, 255 local entries of mixed kinds: blobs, needles, entries the cull rejects (opacity
             < 1/255) and entries it can only box-test (opacity at the threshold, an indefinite conic)
  lengths_b  64 flat globals in front -- in every tile a word in which every entry hits every cell -- followed by nothing, by
             ONE word whose 64 entries all hit one cell (the wave's three other cells get none), by a single entry, and by mixed
             locals up to 256, 257 and 300 entries
  opaque     stacks of opacity 0.85: twenty narrow ones on one cell, which finishes inside the first word while its neighbours
             go on through 300 entries; twelve flat ones centred on a tile, which finishes before its second batch of 256;
             eight globals with nearly singular and extremely anisotropic conics behind them (box test only)"""
import numpy as np
import pytest
import torch

from tests import binning_cases as bc
from tests import helpers as hp

pytestmark = pytest.mark.gpu

SIZES = ((48, 32), (37, 21))
_REF = {}   # (scene, W, H) -> inputs and oracle results, computed once


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _default_walk(monkeypatch):
    monkeypatch.delenv("GHR_K7_WALK", raising=False)


# ---- entries: (x, y) inside the tile, conic (a, b, c), opacity -----------------------------------------------------------
def _iso(v):
    return (1.0 / v, 0.0, 1.0 / v)


def _needle(angle, long_var=0.9, short_var=0.05):
    c, s = np.cos(angle), np.sin(angle)
    cov = np.array([[c * c * long_var + s * s * short_var, c * s * (long_var - short_var)],
                    [c * s * (long_var - short_var), s * s * long_var + c * c * short_var]])
    inv = np.linalg.inv(cov)
    return (inv[0, 0], inv[0, 1], inv[1, 1])


def _mixed(rng, n):
    """n local entries (variance + 0.32 <= 1: radius 3) of the kinds the cull distinguishes, in seeded order: (x, y) inside the tile, conic, opacity."""
    out = []
    for _ in range(n):
        x, y = 3.01 + 9.98 * rng.random(2)
        kind = rng.integers(0, 10)
        if kind < 4:
            e = (x, y, _iso(0.2 + 0.45 * rng.random()), 0.05 + 0.55 * rng.random())
        elif kind < 7:
            e = (x, y, _needle(np.pi * rng.random()), 0.1 + 0.6 * rng.random())
        elif kind == 7:
            e = (x, y, _iso(0.6), 0.003)                               # opacity < 1/255: the cull rejects it
        elif kind == 8:
            e = (x, y, _iso(0.6), 1.0005 / 255.0)                      # at the threshold: box test only (the whole plane)
        else:
            e = (6.01 + 3.98 * rng.random(), 6.01 + 3.98 * rng.random(), (-0.2, 0.0, 0.4), 0.3)   # indefinite (radius 5)
        out.append(e)
    return out


ONE_CELL = (9.5, 9.5)   # the middle of cell (wave 2, group 2) of a tile: pixels 8 .. 11
FLAT_TILE = 1           # the tile the flat opaque stack is centred on
ON_CELL = 20            # entries of the narrow opaque stack (variance 3.5: radius 6, the corner pixels finish on the 16th)


def _one_cell_word():
    """64 entries whose alpha >= 1/255 region (radius 0.81 around the middle of a cell) stays inside that cell."""
    return [(ONE_CELL[0], ONE_CELL[1], _iso(0.2), 0.02)] * 64


def _scene(scene, rng, W, H):
    """(globals, locals per tile): globals as (X, Y, conic, opacity) in image coordinates, in front of all locals."""
    if scene == "lengths_a":
        return [], [_mixed(rng, n) for n in (0, 1, 63, 64, 65, 255)]
    if scene == "lengths_b":
        flat = [(W * rng.random(), H * rng.random(), _iso(2000.0), 0.04) for _ in range(64)]
        return flat, [[], _one_cell_word(), _mixed(rng, 1), _mixed(rng, 192), _mixed(rng, 193), _mixed(rng, 236)]
    if scene == "opaque":
        on_cell = [(ONE_CELL[0], ONE_CELL[1], _iso(3.5), 0.85)] * ON_CELL
        stack = [(16.0 * FLAT_TILE + 8.0, 8.0, _iso(200.0), 0.85)] * 12
        odd = [(W * rng.random(), H * rng.random(), c, 0.4) for c in
               ((0.5, 0.49999, 0.5), (1.0, -0.99999, 1.0), (1e-6, 0.0, 1e3), (1e3, 0.0, 1e-6)) * 2]
        return stack + odd, [on_cell + _mixed(rng, 260), _mixed(rng, 280), on_cell + _mixed(rng, 25), [], _mixed(rng, 110),
                             _mixed(rng, 237)]
    raise ValueError(scene)


SCENES = ("lengths_a", "lengths_b", "opaque")
LENGTHS = dict(lengths_a=(0, 1, 63, 64, 65, 255), lengths_b=(64, 128, 65, 256, 257, 300), opaque=(300, 300, 65, 20, 130, 257))


def build_scene(scene, W, H):
    """Mode-A inputs.  Depths: a tile's on-cell stack (scene "opaque") first, then the globals, then its other locals."""
    rng = np.random.default_rng(101 + SCENES.index(scene))
    glob, tiles = _scene(scene, rng, W, H)
    gx = (W + 15) // 16
    assert gx == 3 and (H + 15) // 16 == 2 and len(tiles) == 6
    rows = [(X, Y, ON_CELL + k, c, o) for k, (X, Y, c, o) in enumerate(glob)]
    for t, entries in enumerate(tiles):
        for k, (x, y, c, o) in enumerate(entries):
            first = scene == "opaque" and k < ON_CELL and c == _iso(3.5)
            rows.append((16 * (t % gx) + x, 16 * (t // gx) + y, k if first else ON_CELL + len(glob) + k, c, o))
    P = len(rows)
    rows = [rows[i] for i in rng.permutation(P)]   # rows in no particular order: the lists come out by depth
    px, py, rank, conic, op = (np.asarray([r[j] for r in rows], np.float64) for j in range(5))
    ri = bc._inputs(W, H, px, py, rank / 1024.0, np.full(P, bc.PILE_SCALE), op, rng.random((P, 10)))
    ri["conic"] = torch.from_numpy(conic.astype(np.float32))
    return ri


def _reference(oracle_mod, scene, W, H):
    key = (scene, W, H)
    if key not in _REF:
        ri = build_scene(scene, W, H)
        out_o, radii_o, st_o = hp.oracle_forward(oracle_mod, ri, "A")
        _REF[key] = (ri, out_o, radii_o, st_o)
    return _REF[key]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _forward(ri, dev):
    from tests.gpu_helpers import GpuRun, to_dev
    run = GpuRun(to_dev(ri, dev), "A")
    ins = run.inspect()
    return run, dict(image=run.out.cpu().numpy(), final_T=ins["final_T"], n_contrib=ins["n_contrib"]), ins


def _tile_pixels(W, H, t):
    ys, xs = np.mgrid[0:H, 0:W]
    return ((xs // 16) + 3 * (ys // 16) == t)


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("scene", SCENES)
def test_list_walk_is_the_mask_walk_bit_for_bit_and_the_oracle(oracle_mod, dev, monkeypatch, scene, W, H):
    from gaussianhaircut_amd import _lib
    ri, out_o, radii_o, st_o = _reference(oracle_mod, scene, W, H)

    run_l, fwd_l, ins = _forward(ri, dev)
    monkeypatch.setenv("GHR_K7_WALK", "mask")
    run_m, fwd_m, _ = _forward(ri, dev)
    monkeypatch.delenv("GHR_K7_WALK")

    # the scene is what it claims to be
    np.testing.assert_array_equal(np.diff(ins["tile_start"].astype(np.int64)), LENGTHS[scene])

    # list walk against the mask walk: bit for bit
    for k in fwd_l:
        assert np.array_equal(_bits(fwd_l[k]), _bits(fwd_m[k])), k

    # list walk against the oracle
    np.testing.assert_array_equal(ins["point_list"], st_o.point_list)
    frag = st_o.fragile.reshape(-1).astype(bool)
    assert frag.mean() < 0.05   # (hand-placed scenes on ~1000 pixels: the limit of test_gpu_parity's manual scenes)
    ok = ~frag
    np.testing.assert_array_equal(fwd_l["n_contrib"][ok], st_o.n_contrib[ok])
    assert hp.image_close(fwd_l["final_T"][ok], st_o.final_T[ok]).all()
    got, ref = fwd_l["image"].reshape(10, -1)[:, ok], out_o.reshape(10, -1)[:, ok]
    assert np.isfinite(fwd_l["image"]).all()
    close = hp.image_close(got, ref)
    assert close.all(), "%d px-channels off, max err %g" % ((~close).sum(), np.abs(got - ref).max())

    # what the special words and the stacks are there for, read off n_contrib (a list position, 1-based)
    nc = fwd_l["n_contrib"].reshape(H, W).astype(np.int64)
    cell = np.zeros((H, W), bool)   # cell (wave 2, group 2) of tiles 0 and 1, which are whole tiles at both sizes
    cell[8:12, 8:12] = True
    t0, t1 = _tile_pixels(W, H, 0), _tile_pixels(W, H, 1)
    if scene == "lengths_b":
        assert (nc[t0] == 64).all()                                            # every pixel of every cell composites the word
        one = np.roll(cell, 16, axis=1)
        assert (nc[t1 & ~one] == 64).all() and nc[one].max() == 128            # one cell takes the second word, the others none
    if scene == "opaque":
        assert 0 < nc[cell].min() and nc[cell].max() <= ON_CELL    # the cell is finished inside the first word ...
        assert nc[t0 & ~cell].max() > 256                     # ... its neighbours walk on into the second batch
        assert 0 < nc[t1].min() and nc[t1].max() <= 12        # the whole tile is finished long before its second batch

    # the words and last contributors left for the gradient walk: an ordered backward pass, bit for bit
    dL = torch.randn(10, H, W, generator=torch.Generator().manual_seed(11))
    L = _lib.lib()
    assert L.ghr_set_deterministic(1) == 0
    try:
        g_l, g_m = run_l.backward(dL), run_m.backward(dL)
    finally:
        assert L.ghr_set_deterministic(0) == 1
    assert len(g_l) == 8
    for k in g_l:
        assert np.array_equal(_bits(g_l[k]), _bits(g_m[k])), k
