"""Shared cases of the strand shape term (csrc/ghr_shape.h, gaussianhaircut_amd/strand_shape.py): the smallest shapes at which
the kernels can still go wrong, the planted inputs, a numpy model of the neighbour search and the list builder, and the float64
arbiter with the magnitudes the error bar is built on.

The bar of a float32 result against the arbiter is ``C * 2^-24 * mag`` where ``mag`` is the arbiter's sum of the absolute values of
everything that enters the element before any cancellation: both sides of ``len/rest - 1``, of ``d[i+1] - d[i]`` and of
``sum u_t - u (u . sum u_t)``.  It is not built on |gradient|: the stretch term at len ~ rest would have no meaningful bar.
"""
import functools

import numpy as np
import torch

EPS = 2.0 ** -24
DEAD = np.float32(1e-4)  # GHR_SHAPE_DEAD

# The largest ratio |composed float32 - arbiter| / (2^-24 mag) over every case, term and element, composed form on CPU tensors
# (StrandShape(fused=False)), measured 2026-10-21: 0.48 (E), 17.87 (d_dirs, at the hub of 516 summands; 5.44 on the other cases).
# C is four times the larger: the kernel's summation trees are different but equally long.
COMPOSED_RATIO = 17.87
C = 4 * COMPOSED_RATIO

PAIRS = [(1, 1), (1, 64), (2, 2), (2, 129), (5, 1), (5, 63), (5, 99), (63, 65), (64, 2), (65, 64), (65, 129), (130, 63), (130, 99)]


def f32_len(d):
    d = np.asarray(d, np.float32)
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], dtype=np.float32)


def alive_mask(dirs, rest):
    """the definition's dead rule, in float32"""
    return f32_len(dirs) > DEAD * np.asarray(rest, np.float32)[:, None]


def default_rest(dirs):
    return np.linalg.norm(np.asarray(dirs, np.float64), axis=-1).mean(axis=1).astype(np.float32)


def _axis_vector_of_length(target):
    """x with sqrtf(x*x) == target exactly (float32), searched over the few neighbours of target"""
    target = np.float32(target)
    x = target
    for _ in range(8):
        for cand in (x, np.nextafter(x, np.float32(0)), np.nextafter(x, np.float32(np.inf))):
            if f32_len(np.array([cand, 0, 0], np.float32)) == target:
                return cand
        x = np.nextafter(x, np.float32(np.inf))
    raise AssertionError("no float32 x with sqrt(x*x) == %r" % target)


def smooth_groom(S, n, seed):
    """roots scattered over a patch, strands that bend gently: a random walk of directions around a common heading"""
    rng = np.random.default_rng(seed)
    roots = rng.uniform(-0.1, 0.1, (S, 3)).astype(np.float32)
    heading = np.array([0.1, -1.0, 0.2]) + rng.normal(0, 0.15, (S, 1, 3))
    walk = np.cumsum(rng.normal(0, 0.05, (S, n, 3)), axis=1)
    d = heading + walk
    d = d / np.linalg.norm(d, axis=-1, keepdims=True) * rng.uniform(0.002, 0.004, (S, 1, 1))
    return roots, d.astype(np.float32)


def _plant(dirs, rest):
    """a segment of length exactly 0, one at exactly GHR_SHAPE_DEAD * rest (dead) and one an ulp above (alive), where they fit"""
    S, n = dirs.shape[:2]
    planted = {}
    if n >= 1:
        dirs[S - 1, n - 1] = 0.0
        planted["zero"] = (S - 1, n - 1)
    if n >= 3:
        thr = DEAD * rest[0]
        dirs[0, 1] = (_axis_vector_of_length(thr), 0, 0)
        planted["at"] = (0, 1)
        if S >= 2:
            thr = DEAD * rest[1]
            dirs[1, n // 2] = (0, _axis_vector_of_length(np.nextafter(thr, np.float32(np.inf))), 0)
            planted["above"] = (1, n // 2)
    return planted


def _case(name, roots, dirs, rest=None, radius=None, nbr=None, plant=True):
    dirs = np.ascontiguousarray(dirs, np.float32)
    rest = default_rest(dirs) if rest is None else np.ascontiguousarray(rest, np.float32)
    planted = _plant(dirs, rest) if plant else {}
    return dict(name=name, roots=np.ascontiguousarray(roots, np.float32), dirs=dirs, rest=rest, radius=radius, nbr=nbr, planted=planted)


def radius_roots():
    """with radius 1.5: root 4 has no neighbour, root 3 one (2), root 0 two (1, 5), roots 1, 2 and 5 three"""
    return np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [100, 0, 0], [1, 1, 0]], np.float32)


def lattice_roots(S):
    """an integer lattice: distances tie in every direction"""
    side = int(np.ceil(S ** (1 / 3)))
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return g[:S].astype(np.float32)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for k, (S, n) in enumerate(PAIRS):
        roots, dirs = smooth_groom(S, n, seed=100 + k)
        rng = np.random.default_rng(200 + k)
        # explicit rest lengths on every second case (the dead threshold is then planted against them), the default on the others
        rest = (default_rest(dirs) * rng.uniform(0.8, 1.25, S)).astype(np.float32) if k % 2 else None
        if k % 3 == 1:
            roots = lattice_roots(S)
        out.append(_case("S%d_n%d" % (S, n), roots, dirs, rest=rest, radius=(1.1 if k % 3 == 1 and S > 5 else None)))
    roots, dirs = smooth_groom(70, 2, seed=7)
    out.append(_case("coincident70", np.zeros((70, 3), np.float32) + np.float32(0.25), dirs))
    roots, dirs = smooth_groom(6, 5, seed=8)
    out.append(_case("radius", radius_roots(), dirs, radius=1.5))
    roots, dirs = smooth_groom(130, 65, seed=9)
    hub = np.zeros((130, 4), np.int32)
    hub[0] = -1
    out.append(_case("hub130", roots, dirs, nbr=hub))
    roots, dirs = smooth_groom(5, 3, seed=10)
    out.append(_case("alone", roots, dirs, nbr=np.full((5, 4), -1, np.int32)))          # M == 0
    return tuple(out)


# ---- the numpy model of the neighbour search and of the list builder ------------------------------------------------------------
def model_neighbours(roots, radius=None):
    roots = np.asarray(roots, np.float32).reshape(-1, 3)
    S = roots.shape[0]
    r2 = np.float32(np.inf) if radius is None else np.float32(radius) * np.float32(radius)
    out = np.full((S, 4), -1, np.int32)
    for s in range(S):
        dx, dy, dz = (roots[:, c] - roots[s, c] for c in range(3))
        d2 = ((dx * dx) + (dy * dy)) + (dz * dz)
        d2[s] = np.inf
        order = np.argsort(d2, kind="stable")[:4]
        for k, j in enumerate(order):
            if d2[j] < np.inf and not d2[j] > r2:
                out[s, k] = j
    return out


def model_lists(nbr):
    S = nbr.shape[0]
    per = [[] for _ in range(S)]
    for t in range(S):
        for k in range(4):
            if nbr[t, k] >= 0:
                per[nbr[t, k]].append(4 * t + k)
    start = np.zeros(S + 1, np.int32)
    start[1:] = np.cumsum([len(p) for p in per])
    return start, np.array([e for p in per for e in p], np.int32)


def case_nbr(case):
    return case["nbr"] if case["nbr"] is not None else model_neighbours(case["roots"], case["radius"])


# ---- the float64 arbiter ---------------------------------------------------------------------------------------------------------
def arbiter(dirs, rest, nbr):
    """-> E [3] float64, grads [3][S, n, 3] (d E_k / d dirs), mag_E [3], mag_g [3][S, n, 3]"""
    dirs, rest, nbr = np.asarray(dirs, np.float32), np.asarray(rest, np.float32), np.asarray(nbr)
    S, n = dirs.shape[:2]
    M = int((nbr >= 0).sum())
    alive = torch.from_numpy(alive_mask(dirs, rest))
    d = torch.from_numpy(dirs).double().requires_grad_(True)
    r = torch.from_numpy(rest).double()[:, None]
    valid = torch.from_numpy(nbr >= 0)
    idx = torch.from_numpy(np.maximum(nbr, 0)).long()
    length = torch.linalg.vector_norm(d, dim=-1)
    E0 = ((length / r - 1) ** 2).sum() / (S * n)
    E1 = (((d[:, 1:] - d[:, :-1]) ** 2).sum(-1) / r ** 2).sum() / (S * (n - 1)) if n > 1 else d.sum() * 0
    u = torch.where(alive[..., None], d / torch.where(alive, length, torch.ones_like(length))[..., None], torch.zeros_like(d))
    ut = u[idx]                                                        # [S, 4, n, 3]
    E2 = ((1 - (u[:, None] * ut).sum(-1)) * valid[:, :, None]).sum() / (n * M) if M > 0 else d.sum() * 0
    E = [E0, E1, E2]
    grads = [torch.autograd.grad(e, d, retain_graph=True, allow_unused=True)[0] for e in E]
    grads = [np.zeros((S, n, 3)) if g is None else g.numpy() for g in grads]
    # magnitudes
    D = dirs.astype(np.float64)
    R = rest.astype(np.float64)[:, None]
    ln = np.linalg.norm(D, axis=-1)
    A = alive.numpy()
    safe = np.where(ln > 0, ln, 1.0)
    q = np.where((ln > 0)[..., None], np.abs(D) / safe[..., None], 0.0)
    ua = np.where(A[..., None], q, 0.0)                               # |u|
    mE0 = ((ln / R + 1) ** 2).sum() / (S * n)
    pair = (np.abs(D[:, 1:]) + np.abs(D[:, :-1]))
    mE1 = ((pair ** 2).sum(-1) / R ** 2).sum() / (S * (n - 1)) if n > 1 else 0.0
    uta = ua[np.maximum(nbr, 0)] * (nbr >= 0)[:, :, None, None]      # [S, 4, n, 3]
    mE2 = ((1 + (ua[:, None] * uta).sum(-1)) * (nbr >= 0)[:, :, None]).sum() / (n * M) if M > 0 else 0.0
    mg0 = (2 * (ln / R + 1) / R)[..., None] * q / (S * n)
    mg1 = np.zeros_like(D)
    if n > 1:
        mg1[:, 1:] += pair
        mg1[:, :-1] += pair
        mg1 = mg1 * (2 / R ** 2)[..., None] / (S * (n - 1))
    mg2 = np.zeros_like(D)
    if M > 0:
        tot = uta.sum(1)                                              # own choices
        for t in range(S):
            for k in range(4):
                if nbr[t, k] >= 0:
                    tot[nbr[t, k]] += ua[t]                           # and whoever chose it
        mg2 = np.where(A[..., None], (tot + ua * (ua * tot).sum(-1, keepdims=True)) / safe[..., None], 0.0) / (n * M)
    return np.array([float(e.detach()) for e in E]), grads, np.array([mE0, mE1, mE2]), [mg0, mg1, mg2]


@functools.lru_cache(maxsize=None)
def arbiter_of(index):
    """the arbiter's answer of case `index`, computed once and shared"""
    c = cases()[index]
    return arbiter(c["dirs"], c["rest"], case_nbr(c))


COTANGENTS = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.7, 1.3, 0.45))


def ratios(E, grad_of, index):
    """the largest |x - arbiter| / (2^-24 mag) of E (per term) and of d_dirs (per element, per cotangent of COTANGENTS);
    grad_of(cot) -> [S, n, 3].  An element whose mag is 0 must be exactly the arbiter's."""
    E64, g64, mE, mg = arbiter_of(index)
    rE, rg = 0.0, 0.0
    for k in range(3):
        err = abs(float(E[k]) - E64[k])
        if mE[k] == 0:
            assert err == 0, (k, E[k], E64[k])
        else:
            rE = max(rE, err / (EPS * mE[k]))
    for cot in COTANGENTS:
        got = np.asarray(grad_of(cot), np.float64)
        assert np.isfinite(got).all()
        want = sum(w * g for w, g in zip(cot, g64))
        mag = sum(abs(w) * m for w, m in zip(cot, mg))
        err = np.abs(got - want)
        assert (err[mag == 0] == 0).all(), cot
        if (mag > 0).any():
            rg = max(rg, float((err[mag > 0] / (EPS * mag[mag > 0])).max()))
    return rE, rg
