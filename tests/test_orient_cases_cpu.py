"""The integer-valued cases of tests/orient_cases.py validate themselves without a GPU: on every case the PyTorch-composed
comparator (``gabor_orientation(..., fused=False)``) and the host simulator (``ghrsim_orient_gabor``: the kernel's own
``orient_pick``) return the exact oracle's ``deg`` at every pixel and its variance within the derived bar
(``orient_cases.var_bar``).  That proves the cases well-posed and the oracle right before tests/test_gpu_orient_shapes.py spends
GPU time on them.  ``pack_bank`` is unpacked by the documented lane rule at every (F, K) of the grid."""
import numpy as np
import pytest

from tests import orient_cases as oc
from tests.test_orient_cpu import conf_numpy, sim, sim_gabor  # noqa: F401  (sim: fixture)


def _both(sim, c):
    from gaussianhaircut_amd import orientation as ori
    deg, var = ori.gabor_orientation(c.plane, c.bank(), fused=False)
    assert deg.dtype == np.uint8
    oc.check_exact(c, deg, var, "comparator")
    deg, var, conf = sim_gabor(sim, c.plane, c.weights, c.thetas)
    oc.check_exact(c, deg, var, "host-sim")
    exp = conf_numpy(var.astype(np.float16))
    assert (np.abs(conf - exp) <= 2 * np.spacing(exp)).all()


@pytest.mark.parametrize("K", oc.KSIZES)
@pytest.mark.parametrize("F", oc.N_FILTERS)
def test_random_banks_over_the_grid(sim, F, K):
    for H, W in oc.SHAPES:
        c = oc.random_case(F, K, H, W)
        assert c.A.max() > 0 and (c.plane[0] != 0).all() and (c.plane[-1] != 0).all() and (c.plane[:, 0] != 0).all() and (c.plane[:, -1] != 0).all()
        _both(sim, c)


@pytest.mark.parametrize("K", oc.SPECIAL_KSIZES)
@pytest.mark.parametrize("F", oc.SPECIAL_FILTERS)
def test_tie_banks_the_first_maximum_wins(sim, F, K):
    pairs = oc.tie_pairs(F)
    assert len(pairs) >= 6
    for what, (a, b) in pairs:
        c, share = oc.tie_case(F, K, a, b)
        print("tie bank (%d, %d) across a %s boundary, F=%d K=%d: tied maximum, first wins, at %.0f %% of the pixels" % (a, b, what, F, K, 100 * share))
        assert share >= oc.TIE_SHARE
        _both(sim, c)


def test_tie_pairs_cover_every_boundary_of_the_fold():
    """register, lane group, wave and tile, read off the kernel's index ``16 (wave + 4 t) + 4 kq + r``"""
    def parts(k):
        return dict(r=k % 4, kq=(k // 4) % 4, wave=(k // 16) % 4, t=k // 64)
    differ = {p: {n for n in "r kq wave t".split() if parts(p[0])[n] != parts(p[1])[n]} for _, p in oc.TIE_PAIRS}
    assert differ[(0, 1)] == differ[(2, 3)] == {"r"}
    assert differ[(3, 4)] == differ[(11, 12)] == {"r", "kq"}
    assert differ[(15, 16)] == differ[(47, 48)] == {"r", "kq", "wave"}
    assert differ[(63, 64)] == differ[(127, 128)] == differ[(191, 192)] == {"r", "kq", "wave", "t"}
    assert differ[(5, 21)] == {"wave"} and differ[(5, 69)] == {"t"}
    assert [p for _, p in oc.tie_pairs(17)] == [(0, 1), (2, 3), (3, 4), (11, 12), (15, 16), (0, 16)]
    assert len(oc.tie_pairs(256)) == len(oc.TIE_PAIRS) + 1 and oc.tie_pairs(256)[-1][1] == (0, 255)
    assert [oc.tiles_per_wave(F) for F in oc.N_FILTERS] == [1, 1, 1, 1, 2, 2, 3, 3, 4, 4]


@pytest.mark.parametrize("K", oc.SPECIAL_KSIZES)
@pytest.mark.parametrize("F", oc.SPECIAL_FILTERS)
def test_all_equal_and_ladder_banks(sim, F, K):
    c = oc.all_equal_case(F, K)
    assert not c.k.any()
    _both(sim, c)
    c = oc.ladder_case(F, K)
    assert np.array_equal(c.k, np.where(c.A[0] != 0, F - 1, 0))
    _both(sim, c)


def test_ladder_bank_is_exact_at_the_largest_bank_and_window():
    c = oc.ladder_case(256, 25)   # exact_maps asserts the exactness condition
    assert c.A.max() < oc.EXACT and (c.k == 255).any()


@pytest.mark.parametrize("K", oc.KSIZES)
@pytest.mark.parametrize("F", oc.N_FILTERS)
def test_pack_bank_round_trips_by_the_lane_rule(F, K):
    from gaussianhaircut_amd import _lib
    from gaussianhaircut_amd import orientation as ori
    w = oc.random_case(F, K, 1, 1).weights
    w = w + np.float32(0.5)   # no real element is zero: a swapped padding slot cannot hide
    p = ori.pack_bank(w)
    assert p.dtype == np.float32 and p.size == int(_lib.lib().ghr_orient_bank_floats(F, K))
    back, padding = oc.unpack_bank(p, F, K)
    assert np.array_equal(back, w)
    assert padding.size == p.size - F * K * K and not padding.any()
