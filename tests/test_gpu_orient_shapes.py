"""`-m gpu`: k_orient_gabor<NT> at every tile form, window size and tie, and k_orient_dog at its block edges.

The integer-valued cases of tests/orient_cases.py (validated on the CPU by tests/test_orient_cases_cpu.py) go through
``ghr_orient_gabor`` (C ABI, ctypes).  Every response is an exactly representable integer, so ``deg`` must equal the oracle's
first arg-max at EVERY pixel -- there is no undecided set -- and the planted ties pin ``orient_better``'s "first maximum wins"
across the register, lane-group, wave and tile folds of the epilogue.

Launch shapes.  A workgroup is a 16 x 8 pixel tile: (1, 1), (8, 16) exactly one, (9, 17) one past in both axes, (17, 33) 3 x 3.
``n_filters`` 1 ... 64 take NT = 1 (1, 16, 17: idle waves), 65 ... 128 NT = 2, 129 ... 192 NT = 3, 193 ... 256 NT = 4; ``ksize`` 1
and 3 have fewer taps than one or three k steps hold, 25 fills the LDS tile (40 x 32 floats).

Bars.  ``deg``: equal.  ``var``: ``|got - var64| <= (2 F + 8) 2^-24 var64`` and exactly 0 where ``var64 == 0`` -- derived in
tests/orient_cases.py from the roundings of the epilogue, with the float32 ``o``, ``thetas`` and ``pi`` as the oracle's inputs: one
per distance (squared), three for ``d * d * F``, F - 1 for each of the two sums in any order, one for the division; a wrong
theta for one real filter is about 1 / F relative.  ``angle``: ``float32(deg) / float32(180)`` bit for bit (today's rule for
every F).  ``conf``: within two float32 spacings of ``conf_numpy`` of the returned variance (through float16 unless
``via_half = 0``), the bar of tests/test_gpu_orient.py.  Every output sits in a poisoned buffer between guards: the floats in NaN,
``deg`` in a byte the oracle's ``deg`` does not hold."""
import ctypes

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from tests import orient_cases as oc
from tests import test_gpu_orient as tg
from tests.golden import make_reference_orient_golden as mk
from tests.test_orient_cpu import check_maps, check_plane, conf_numpy, gold  # noqa: F401  (gold: fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 64   # elements on either side of every output
NAMES = ("deg", "var", "angle", "conf")
DOG_SHAPES = ((1, 1), (1, 64), (1, 65), (4, 63), (5, 64), (3, 129))   # k_orient_dog works in blocks of 64 x 4


class Out:
    """a poisoned device buffer between two poisoned guards: float32 in NaN, bytes in ``poison``"""

    def __init__(self, n, dtype, poison):
        self.n, self.poison = int(n), poison
        self.buf = torch.full((self.n + 2 * GUARD,), poison, dtype=dtype, device=DEV)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())

    def _is_poison(self, a):
        return np.isnan(a) if a.dtype == np.float32 else a == self.poison

    def get(self, shape, written=True):
        """the payload; asserts the guards intact and the payload written everywhere (or nowhere)"""
        b = self.buf.cpu().numpy()
        assert self._is_poison(b[:GUARD]).all() and self._is_poison(b[GUARD + self.n:]).all(), "a guard was written"
        body = b[GUARD:GUARD + self.n]
        if written:
            assert not self._is_poison(body).any(), "a slot was left unwritten"
        else:
            assert self._is_poison(body).all(), "a buffer that was not passed was written"
        return body.reshape(shape).copy()


def run(case, want=NAMES, via_half=1):
    """one ghr_orient_gabor call; outputs not in ``want`` are passed as NULL and must stay poisoned.  Returns dict name -> array"""
    from gaussianhaircut_amd import orientation as ori
    H, W, n = case.H, case.W, case.H * case.W
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    plane, wd = up(case.plane), up(ori.pack_bank(case.weights))
    td = up(np.asarray(case.thetas, np.float64).astype(np.float32))
    L = _lib.lib()
    assert wd.numel() == int(L.ghr_orient_bank_floats(case.F, case.K))
    absent = sorted(set(range(256)) - set(np.unique(case.k).tolist()))
    outs = dict(deg=Out(n, torch.uint8, absent[0]), var=Out(n, torch.float32, float("nan")),
                angle=Out(n, torch.float32, float("nan")), conf=Out(n, torch.float32, float("nan")))
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    _lib.check(L.ghr_orient_gabor(None, W, H, p(plane), case.F, case.K, p(wd), p(td), *[outs[k].ptr if k in want else None for k in NAMES],
                                  via_half))
    torch.cuda.synchronize()
    return {k: outs[k].get((H, W), written=k in want) for k in NAMES}


def check_all(case, via_half=1):
    """the four outputs of one call against the oracle; returns (outputs, worst variance err / bar)"""
    r = run(case, via_half=via_half)
    worst = oc.check_exact(case, r["deg"], r["var"], "gpu")
    assert np.array_equal(r["angle"].view(np.uint32), (r["deg"].astype(np.float32) / np.float32(180)).view(np.uint32)), case.name
    exp = conf_numpy(r["var"].astype(np.float16) if via_half else r["var"])
    assert (np.abs(r["conf"] - exp) <= 2 * np.spacing(exp)).all(), case.name
    return r, worst


def same_bytes(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in NAMES)


@pytest.mark.parametrize("K", oc.KSIZES)
@pytest.mark.parametrize("F", oc.N_FILTERS)
def test_random_banks_over_the_grid(F, K):
    worst = max(check_all(oc.random_case(F, K, H, W))[1] for H, W in oc.SHAPES)
    _, w0 = check_all(oc.random_case(F, K, *oc.SPECIAL_SHAPE), via_half=0)
    print("NT=%d F=%d K=%d: variance worst err / bar %.3g over the shapes" % (oc.tiles_per_wave(F), F, K, max(worst, w0)))


@pytest.mark.parametrize("K", oc.SPECIAL_KSIZES)
@pytest.mark.parametrize("F", oc.SPECIAL_FILTERS)
def test_tie_banks_the_first_maximum_wins(F, K):
    for what, (a, b) in oc.tie_pairs(F):
        c, share = oc.tie_case(F, K, a, b)
        assert share >= oc.TIE_SHARE
        r, _ = check_all(c)
        tied = (c.A[a] == c.A[b]) & (c.A[a] == c.A.max(0)) & (c.k == a)
        assert (r["deg"][tied] == a).all(), (what, a, b)


@pytest.mark.parametrize("K", oc.SPECIAL_KSIZES)
@pytest.mark.parametrize("F", oc.SPECIAL_FILTERS)
def test_all_equal_and_ladder_banks(F, K):
    r, _ = check_all(oc.all_equal_case(F, K))
    assert not r["deg"].any()
    c = oc.ladder_case(F, K)
    r, _ = check_all(c)
    assert np.array_equal(r["deg"], np.where(c.A[0] != 0, F - 1, 0))


def test_null_outputs_leave_the_others_unchanged_and_untouched():
    c = oc.random_case(65, 17, *oc.SPECIAL_SHAPE)
    full, _ = check_all(c)
    for want in (("deg",), ("var",), ("angle",), ("conf",), ("angle", "conf")):
        r = run(c, want=want)   # asserts the unpassed buffers still poisoned, the passed ones written, all guards intact
        for k in want:
            assert np.array_equal(r[k].view(np.uint8), full[k].view(np.uint8)), (want, k)


@pytest.mark.parametrize("F,K", ((65, 17), (128, 3), (256, 25), (193, 17)))
def test_two_calls_give_the_same_bytes(F, K):
    c = oc.random_case(F, K, 17, 33)
    assert oc.tiles_per_wave(F) == (2 if F <= 128 else 4)
    assert same_bytes(run(c), run(c))


@pytest.mark.parametrize("num_filters,NT", ((96, 2), (256, 4)))
def test_float_banks_of_96_and_256_filters(gold, num_filters, NT):
    """the bars of test_a_second_bank_of_45_filters_and_11_taps at the two tile forms the float banks of that module do not take"""
    from gaussianhaircut_amd import orientation as ori
    bank = ori.gabor_bank(num_filters=num_filters)
    assert bank[0].shape[0] == num_filters and oc.tiles_per_wave(num_filters) == NT
    ref = tg._restated(gold["c2/image"], bank)
    deg, var = tg._gabor(tg._dev(ref["dog32"]), bank)
    assert deg.max() < num_filters
    check_maps(deg, var, ref, "gpu %d filters, ksize %d" % (num_filters, bank[0].shape[-1]))


@pytest.mark.parametrize("H,W", DOG_SHAPES)
def test_dog_at_block_boundaries(H, W):
    from gaussianhaircut_amd import orientation as ori
    rgb = mk.make_image(H, W, 100 * H + W)
    g = np.random.default_rng(H * 1000 + W)
    grey32 = (g.random((H, W)) * 255).astype(np.float32)
    grey_of_rgb = 0.2989 * rgb[:, :, 0] + 0.5870 * rgb[:, :, 1] + 0.1140 * rgb[:, :, 2]
    for what, image, grey64 in (("uint8 rgb", rgb, grey_of_rgb), ("float32 grey", grey32, grey32.astype(np.float64))):
        out = Out(H * W, torch.float32, float("nan"))
        res = ori.dog_fused(tg._dev(image), out=out.buf[GUARD:GUARD + H * W].view(H, W))
        assert res.data_ptr() == out.ptr.value
        torch.cuda.synchronize()
        ref = mk.difference_of_gaussians(grey64, 0.4, 10).astype(np.float32)
        check_plane(out.get((H, W)), ref, "gpu DoG %dx%d %s" % (H, W, what))
