"""Integer-valued cases for the Gabor bank kernel (csrc/ghr_orient.h, k_orient_gabor<NT>) and their exact oracle.  numpy only.

Plane and weights are small integers, so every response -- and every partial sum of its taps -- is an integer below 2^24: it has
ONE float32 value whatever order the matrix unit, the host simulator or the comparator adds the taps in.  ``deg`` is then defined
at every pixel with no undecided set: the first index of the largest |response| (``orient_better``).  That makes planted ties
checkable, which the float banks of tests/test_orient_cpu.py cannot do.

The kernel's filter index is ``16 (wave + 4 t) + 4 kq + r``: register r of lane group kq of wave ``wave``, tile t of that wave.
``TIE_PAIRS`` puts two equal maxima on either side of each of those boundaries.

Variance bar (``var_bar``), derived, not measured.  The oracle starts from the kernel's own float32 inputs (``o``, ``thetas``,
``pi``), so with u = 2^-24, to first order: each distance d carries one rounding (``o - theta``; where the wrapped form
``d -+ pi`` wins, that second subtraction is exact by Sterbenz's lemma) and enters squared; ``d * d * F_k`` adds at most three
more; a sum of F non-negative terms in any order adds at most F - 1; the sum of the responses adds at most F - 1; the division
adds one.  All terms are non-negative, so relative errors do not amplify: 2 + 3 + 2 (F - 1) + 1 = 2 F + 4, and the bar
``|got - var64| <= (2 F + 8) u var64`` leaves four roundings for the second-order terms.  (A wrapped distance inherits the
absolute rounding of ``o - theta``, which is relatively larger on a short distance -- but a short distance enters with the
weight d^2, the smallest of the sum.)  Where ``var64 == 0`` every term is exactly zero and so is the result.
"""
import functools
import math

import numpy as np

N_FILTERS = (1, 16, 17, 64, 65, 128, 129, 192, 193, 256)   # all four NT, both sides of each step, idle waves, padded tiles
KSIZES = (1, 3, 17, 25)
SHAPES = ((1, 1), (8, 16), (9, 17), (17, 33))              # one pixel; one workgroup tile; one past in both axes; 3 x 3 workgroups
SPECIAL_SHAPE = (9, 17)
SPECIAL_KSIZES = (1, 17)
SPECIAL_FILTERS = (17, 65, 129, 193, 256)
TIE_PAIRS = (("register", (0, 1)), ("register", (2, 3)), ("lane group", (3, 4)), ("lane group", (11, 12)),
             ("wave", (15, 16)), ("wave", (47, 48)), ("tile", (63, 64)), ("tile", (127, 128)), ("tile", (191, 192)),
             ("same lane and register, next wave", (5, 21)), ("same lane and register, next tile", (5, 69)))
TIE_SHARE = 0.5
EXACT = 2 ** 24


def tiles_per_wave(F):
    """NT of k_orient_gabor<NT>: the 16-filter tiles dealt over four waves"""
    return ((F + 15) // 16 + 3) // 4


def thetas_of(F):
    return math.pi * np.arange(F) / F


def tie_pairs(F):
    """the (boundary, (a, b)) that fit F filters, and the extremes"""
    out = [(what, p) for what, p in TIE_PAIRS if p[1] < F]
    if F > 1 and (0, F - 1) not in [p for _, p in out]:
        out.append(("extremes", (0, F - 1)))
    return out


# ---- the oracle ------------------------------------------------------------------------------------------------------------------

def responses(plane, weights):
    """int64 [F,H,W]: cross-correlation of the zero-padded plane with the bank; asserts the exactness condition"""
    P, Wt = np.asarray(plane), np.asarray(weights)
    assert np.array_equal(P, np.rint(P)) and np.array_equal(Wt, np.rint(Wt)), "the cases are integer-valued"
    P, Wt = P.astype(np.int64), Wt.astype(np.int64)
    F, K, K2 = Wt.shape
    assert K == K2 and K % 2 == 1
    H, W = P.shape
    win = np.lib.stride_tricks.sliding_window_view(np.pad(P, K // 2), (K, K)).reshape(H * W, K * K)
    resp = (Wt.reshape(F, K * K) @ win.T).reshape(F, H, W)
    # every partial sum of a response, in any order, is bounded by sum |w| |p|: all of them are exact float32 integers
    assert (np.abs(Wt).reshape(F, K * K) @ np.abs(win).T).max() < EXACT
    return resp


def exact_maps(plane, weights, thetas):
    """(k int64 [H,W], var64 float64 [H,W], A int64 [F,H,W]): the first arg-max of |response| and the circular variance in
    float64 from the float32 inputs the kernel's epilogue starts from"""
    A = np.abs(responses(plane, weights))
    assert A.max() < EXACT
    F = A.shape[0]
    k = A.argmax(0)   # numpy: the first maximum
    pi32 = np.float32(math.pi)
    o = (k.astype(np.float32) / np.float32(F) * pi32).astype(np.float64)
    assert (k.astype(np.float32) / np.float32(F) * pi32).dtype == np.float32
    th = np.asarray(thetas, np.float64).astype(np.float32).astype(np.float64)[:, None, None]
    pi = float(pi32)
    dist = np.minimum(np.abs(o[None] - th), np.minimum(np.abs(o[None] - th - pi), np.abs(o[None] - th + pi)))
    A64 = A.astype(np.float64)
    var64 = (dist * dist * A64).sum(0) / np.maximum(A64.sum(0), 1e-12)
    return k, var64, A


def var_bar(F, var64):
    return (2 * F + 8) * 2.0 ** -24 * var64


def check_exact(case, deg, var, what):
    """``deg`` equals the oracle's at EVERY pixel; ``var`` is within ``var_bar`` of it, and exactly 0 where it is 0.  Prints and
    returns the worst ``err / bar``."""
    deg, var = np.asarray(deg), np.asarray(var)
    assert deg.shape == case.k.shape and var.shape == case.k.shape and var.dtype == np.float32, (what, deg.shape, var.shape, var.dtype)
    wrong = deg.astype(np.int64) != case.k
    err, bar = np.abs(var.astype(np.float64) - case.var64), var_bar(case.F, case.var64)
    zero = case.var64 == 0
    worst = float((err[~zero] / bar[~zero]).max()) if not zero.all() else 0.0
    print("%s, %s (NT=%d): deg equal at %d of %d pixels, variance worst err / bar %.3g" % (what, case.name, case.NT, int((~wrong).sum()), wrong.size, worst))
    assert not wrong.any(), (what, case.name, int(wrong.sum()), np.argwhere(wrong)[:4].tolist())
    assert (var[zero] == 0).all(), (what, case.name)
    assert (err <= bar).all(), (what, case.name, worst)
    return worst


# ---- banks -----------------------------------------------------------------------------------------------------------------------

def _seed(*key):
    s = 0
    for v in key:
        s = s * 1009 + int(v) + 1
    return s


def make_plane(H, W, seed):
    """integers in [-8, 8], non-zero in the border rows and columns: the zero-padded halo matters"""
    g = np.random.default_rng(seed)
    p = g.integers(-8, 9, (H, W))
    edge = np.zeros((H, W), bool)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    fix = g.integers(1, 9, (H, W)) * g.choice((-1, 1), (H, W))
    return np.where(edge & (p == 0), fix, p).astype(np.float32)


class Case:
    def __init__(self, name, plane, weights, thetas=None):
        self.name = name
        self.plane = np.ascontiguousarray(plane, np.float32)
        self.weights = np.ascontiguousarray(weights, np.float32)
        self.F, self.K = self.weights.shape[0], self.weights.shape[-1]
        self.H, self.W = self.plane.shape
        self.NT = tiles_per_wave(self.F)
        self.thetas = thetas_of(self.F) if thetas is None else thetas
        self.k, self.var64, self.A = exact_maps(self.plane, self.weights, self.thetas)

    def bank(self):
        return self.weights, self.thetas

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def random_case(F, K, H, W):
    g = np.random.default_rng(_seed(1, F, K, H, W))
    return Case("random F=%d K=%d %dx%d" % (F, K, H, W), make_plane(H, W, _seed(2, F, K, H, W)), g.integers(-4, 5, (F, K, K)))


def _dense(g, K):
    """a filter of magnitudes up to 4 whose taps are all non-zero (at K = 1: magnitude >= 2, above every single-tap filter)"""
    lo = 2 if K == 1 else 1
    return g.integers(lo, 5, (K, K)) * g.choice((-1, 1), (K, K))


@functools.lru_cache(maxsize=None)
def tie_case(F, K, a, b):
    """filters a and b are the same dense filter (b negated when a + b is odd); every other filter has a single tap in {-1, 0, 1}.
    Returns (case, share): the share of pixels at which a and b are the tied maximum and a is the oracle's pick -- asserted, from
    the oracle alone, to be at least TIE_SHARE; a seed that fails is passed over."""
    H, W = SPECIAL_SHAPE
    assert 0 <= a < b < F
    for attempt in range(8):
        g = np.random.default_rng(_seed(3, F, K, a, b, attempt))
        w = np.zeros((F, K, K), np.int64)
        f = np.arange(F)
        w[f, g.integers(0, K, F), g.integers(0, K, F)] = g.integers(-1, 2, F)
        dense = _dense(g, K)
        w[a], w[b] = dense, -dense if (a + b) % 2 else dense
        c = Case("tie (%d, %d) F=%d K=%d" % (a, b, F, K), make_plane(H, W, _seed(4, F, K, a, b, attempt)), w)
        tied = (c.A[a] == c.A[b]) & (c.A[a] == c.A.max(0)) & (c.k == a) & (c.A[a] > 0)
        if tied.mean() >= TIE_SHARE:
            return c, float(tied.mean())
    raise AssertionError("no seed gives a tie bank for %s" % ((F, K, a, b),))


@functools.lru_cache(maxsize=None)
def all_equal_case(F, K):
    """every filter is the same: deg == 0 everywhere"""
    H, W = SPECIAL_SHAPE
    g = np.random.default_rng(_seed(5, F, K))
    c = Case("all equal F=%d K=%d" % (F, K), make_plane(H, W, _seed(6, F, K)), np.broadcast_to(_dense(g, K), (F, K, K)))
    assert not c.k.any() and c.A[0].any()
    return c


@functools.lru_cache(maxsize=None)
def ladder_case(F, K):
    """filter k is (k + 1) x one base filter: deg == F - 1 wherever the base response is non-zero, 0 where it is zero"""
    H, W = SPECIAL_SHAPE
    g = np.random.default_rng(_seed(7, F, K))
    base = g.integers(-4, 5, (K, K))
    if K == 1:
        base[:] = 3
    plane = make_plane(H, W, _seed(8, F, K))
    plane[H // 2, W // 2] = 0 if K == 1 else plane[H // 2, W // 2]   # one pixel whose base response is zero
    c = Case("ladder F=%d K=%d" % (F, K), plane, base[None] * np.arange(1, F + 1)[:, None, None])
    assert np.array_equal(c.k, np.where(c.A[0] != 0, F - 1, 0)) and (c.A[0] != 0).any()
    return c


# ---- the fragment order ------------------------------------------------------------------------------------------------------------

def unpack_bank(packed, F, K):
    """the documented lane rule of include/ghr.h, element by element: [tile][chunk][lane], lane l holds filter
    16 tile + (l & 15), tap 4 chunk + (l >> 4).  Returns (weights [F,K,K], padding: every element the rule maps to no filter
    or no tap)"""
    tiles, chunks = 4 * tiles_per_wave(F), (K * K + 3) // 4
    p = np.asarray(packed)
    assert p.shape == (tiles * chunks * 64,), (p.shape, tiles, chunks)
    t, c, l = np.meshgrid(np.arange(tiles), np.arange(chunks), np.arange(64), indexing="ij")
    filt, tap = (16 * t + (l & 15)).ravel(), (4 * c + (l >> 4)).ravel()
    real = (filt < F) & (tap < K * K)
    w = np.full((F, K * K), np.nan, p.dtype)
    w[filt[real], tap[real]] = p[real]
    return w.reshape(F, K, K), p[~real]
