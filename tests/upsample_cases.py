"""Shared cases of groom upsampling (csrc/ghr_upsample.h, gaussianhaircut_amd/strand_upsampling.py): the smallest shapes at which the
kernels can still go wrong, a numpy float32 model of the neighbour search, the float64 arbiter of the blend with the planted errors,
and the per-element bound.

The bound of a float32 result against the arbiter (the same formulas on the same float32 inputs, with the given nbr / nd2, in
float64) is derived, not tuned.  eps = 2^-24, n = L - 1, c = 8 n + 64: c eps bounds the roundings of one segment sum (n additions,
each segment's 2 + 5 + 5 operations against sums of absolute values that Cauchy-Schwarz bounds by den) and of forming one term; it
is generous on purpose.
    |d s_k| <= c eps                                 (D_k / den, |s_k| <= 1)
    |d q_k| <= c eps / (1 - tau) + 2 eps             (one subtraction, one division; the clamp is 1-Lipschitz; 0 without the gate)
    W >= a_0 >= a_k (nd2 ascending, q_k <= 1 = q_0), so d a_k / W <= d q_k and d W / W <= 3 max d q_k:
    |d w_k| <= E_w = 5 (c eps / (1 - tau) + 16 eps)  (without the gate: 5 x 16 eps -- the additions and divisions alone)
    per coordinate |d out[c][j]| <= sum_k (E_w + 16 eps w_k) |r_k[j]|_1 + 16 eps (|co|_inf + |Pl[j]|_1),
        r_k[j] = gM^T (gp[g_k][j] - gp[g_k][0]): a component of M^T d is rounded against sum_i |M_ic d_i| <= |d|_1 <= sqrt(3) |r|_1
        (M orthonormal), 1 + 3 sqrt(3) + 1 + 3 < 16 roundings with the product by w_k and the three additions; cM Pl and the
        addition of co: 3 + 1 roundings against |Pl|_1 and |co|_inf + |Pl|_1.
    features: sum_k (E_w + 16 eps w_k) |gf[g_k][f]|.
A constant here may only grow together with a written rounding count."""
import functools

import numpy as np

EPS = 2.0 ** -24
K = 4

# (G, L, N, F): every L of 2, 3, 64, 65, 66, 100, 129; every G of 1 .. 5, 255, 256, 257, 513; every N of 1, 3, 63, 64, 65, 255, 256,
# 257; every F of 0, 1, 3, 5
SHAPES = [(1, 2, 1, 0), (2, 3, 3, 1), (3, 64, 63, 3), (4, 65, 64, 5), (5, 66, 65, 0), (255, 100, 255, 1), (256, 129, 256, 3),
          (257, 66, 257, 3), (513, 3, 65, 5), (5, 100, 3, 3)]


def rotations(rng, count):
    """`count` proper rotations, float64 QR of Gaussian matrices, rounded to float32: non-identity, different per row"""
    q, r = np.linalg.qr(rng.normal(size=(count, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 2] *= np.sign(np.linalg.det(q))[:, None]
    return q.astype(np.float32)


def local_shapes(rng, G, L, seg):
    """[G, L, 3] local polylines from the origin: along +z, each guide tilted and curled by its own amounts (cosines between two
    guides' segments around 0.8 .. 0.95: similar, not equal)"""
    t = np.linspace(0.0, 1.0, L - 1)[None, :]
    tilt = rng.normal(0, 0.35, (G, 2, 1))
    curl = rng.uniform(0.1, 0.4, (G, 1))
    om = rng.uniform(3.0, 9.0, (G, 1))
    d = np.stack([tilt[:, 0] + curl * np.sin(om * t), tilt[:, 1] + curl * np.cos(om * t), np.ones_like(t) + 0 * curl], -1)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True) * seg
    return np.concatenate([np.zeros((G, 1, 3)), np.cumsum(d, axis=1)], axis=1)


def to_world(roots, frames, local):
    """gp = root + M local, float64, rounded once"""
    return (roots[:, None, :].astype(np.float64) + np.einsum("grc,glc->glr", frames.astype(np.float64), local)).astype(np.float32)


def _case(name, roots, local, co, seed, F=0, radius=None, tau=0.5, eps2=1e-9, plants=()):
    rng = np.random.default_rng(seed)
    G, N = roots.shape[0], co.shape[0]
    gM, cM = rotations(rng, G), rotations(rng, N)
    roots = np.ascontiguousarray(roots, np.float32)
    gp = to_world(roots, gM, local)
    gp[:, 0] = roots
    gf = rng.uniform(0, 1, (G, F)).astype(np.float32) if F else None
    return dict(name=name, gp=gp, gM=gM, gf=gf, co=np.ascontiguousarray(co, np.float32), cM=cM, radius=radius, tau=tau,
                eps2=float(np.float32(eps2)), plants=frozenset(plants) | {"cM_T"})


def lattice_guides():
    """five guides at squared distance 1 from the origin, one at (0, 0, 3), two further out"""
    return np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, 3], [4, 4, 4], [5, 4, 4]], np.float32)


def lattice_children():
    """the origin (five ties: the four lowest indices win), a guide's root (d2 == 0), (0, 0, 5) (d2 == r2 == 4 to guide 5: inside,
    and it alone), (9, 9, 9) (none inside), (0, 0, 2) (two ties at 1), (4.5, 4, 4) (two ties at 0.25)"""
    return np.array([[0, 0, 0], [1, 0, 0], [0, 0, 5], [9, 9, 9], [0, 0, 2], [4.5, 4, 4]], np.float32)


def count_guides():
    return np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [1, 1, 0]], np.float32)


def count_children():
    """with radius 1.5 (r2 = 2.25): 0, 1, 1, 2 (the second at d2 == r2), 4, 2, 3 guides inside"""
    return np.array([[100, 0, 0], [-1, 0, 0], [4, 0, 0], [-0.5, 0, 0], [0.5, 0, 0], [3.5, 0, 0], [2.5, 0, 0]], np.float32)


def shaped_locals(L, seg=0.05):
    """seven straight guides in their own frames: +z, +z turned by 45 degrees (s = 0.707 > tau) and by 75 degrees (s = 0.259 < tau),
    -z (s = -1), +z again (s = 1), one of zero length (A_k = 0), +z once more"""
    t = np.arange(L)[:, None] * seg
    z = np.array([0.0, 0.0, 1.0])
    turn = lambda deg: np.array([np.sin(np.radians(deg)), 0.0, np.cos(np.radians(deg))])  # noqa: E731
    return np.stack([t * z, t * turn(45), t * turn(75), -t * z, t * z, 0 * t * z, t * z])


def shaped_case(name, L, tau, seed, plants):
    """guides on the x axis at 0 .. 6; child c < 7 just off guide c (so that each kind is the nearest once, the zero-length guide
    included, and a later neighbour elsewhere) and child 7 half way between guides 0 and 1"""
    roots = np.stack([np.arange(7), np.zeros(7), np.zeros(7)], 1).astype(np.float32)
    co = np.array([[0.125, 0, 0], [1.125, 0.25, 0], [2.125, 0, 0], [2.875, 0, 0.25], [4.125, 0, 0], [4.875, 0, 0], [6.125, 0, 0],
                   [0.5, 0, 0]], np.float32)
    return _case(name, roots, shaped_locals(L), co, seed, F=3, tau=tau, eps2=1e-6, plants=plants)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for k, (G, L, N, F) in enumerate(SHAPES):
        rng = np.random.default_rng(300 + k)
        roots = rng.uniform(-0.1, 0.1, (G, 3))
        co = rng.uniform(-0.1, 0.1, (N, 3))
        plants = set()
        if G >= 2:
            plants.add("gate")
        if G >= 3:
            plants.add("swap")
        if G >= 5:
            plants.add("fifth")
        if L >= 64:
            plants.add("lane")
        out.append(_case("G%d_L%d_N%d_F%d" % (G, L, N, F), roots, local_shapes(rng, G, L, 0.004), co, 400 + k, F=F, plants=plants))
    rng = np.random.default_rng(350)
    g = lattice_guides()
    out.append(_case("lattice", g, local_shapes(rng, len(g), 65, 0.05), lattice_children(), 450, F=1, radius=2.0, eps2=1e-6,
                     plants={"gate", "swap", "lane"}))
    g = count_guides()
    out.append(_case("counts", g, local_shapes(rng, len(g), 3, 0.05), count_children(), 451, F=5, radius=1.5, eps2=1e-6,
                     plants={"gate", "swap"}))
    out.append(shaped_case("shapes_gated", 66, 0.5, 452, {"gate", "lane"}))
    out.append(shaped_case("shapes_low_tau", 3, -0.5, 453, {"gate"}))
    out.append(shaped_case("shapes_no_gate", 5, None, 454, ()))
    return tuple(out)


def r2_of(radius):
    return np.float32(np.inf) if radius is None else np.float32(radius) * np.float32(radius)


# ---- the numpy float32 model of the neighbour search -----------------------------------------------------------------------------
def model_neighbours(guide_roots, child_origins, radius=None, width=K):
    """-> nbr [N, width] int32, nd2 [N, width] float32: the `width` nearest guides (width = 5: what the planted error needs)"""
    gr = np.asarray(guide_roots, np.float32).reshape(-1, 3)
    co = np.asarray(child_origins, np.float32).reshape(-1, 3)
    r2 = r2_of(radius)
    nbr = np.full((co.shape[0], width), -1, np.int32)
    nd2 = np.full((co.shape[0], width), np.inf, np.float32)
    for c in range(co.shape[0]):
        dx, dy, dz = (gr[:, x] - co[c, x] for x in range(3))
        d2 = ((dx * dx) + (dy * dy)) + (dz * dz)
        d2 = np.where(d2 < np.inf, d2, np.float32(np.inf))
        for k, j in enumerate(np.argsort(d2, kind="stable")[:width]):
            if d2[j] < np.inf and not d2[j] > r2:
                nbr[c, k], nd2[c, k] = j, d2[j]
    return nbr, nd2


@functools.lru_cache(maxsize=None)
def neighbours_of(index, width=K):
    c = cases()[index]
    return model_neighbours(c["gp"][:, 0], c["co"], c["radius"], width)


def fifth_for_fourth(index):
    """the planted table: the fifth-nearest guide, and its distance, in place of the fourth"""
    nbr, nd2 = neighbours_of(index, 5)
    return np.ascontiguousarray(nbr[:, [0, 1, 2, 4]]), np.ascontiguousarray(nd2[:, [0, 1, 2, 4]])


# ---- the float64 arbiter -----------------------------------------------------------------------------------------------------------
PLANTS = ("swap", "cM_T", "gate", "lane", "fifth")


def arbiter(case, nbr, nd2, plant=None):
    """The definition in float64 on the case's float32 inputs with the given table.  -> dict(points [N, L, 3], weights [N, 4],
    features [N, F], valid [N], b_points [N, L, 3], b_weights [N, 4], b_features [N, F]: the bounds).  plant: one of PLANTS except
    "fifth" (which is a table: fifth_for_fourth) -- the same computation with that one error."""
    gp, gM = case["gp"].astype(np.float64), case["gM"].astype(np.float64)
    co, cM = case["co"].astype(np.float64), case["cM"].astype(np.float64)
    G, L = gp.shape[:2]
    N = co.shape[0]
    tau = None if case["tau"] is None else float(np.float32(case["tau"]))
    eps2 = float(np.float32(case["eps2"]))
    e4 = np.asarray(nbr, np.int64)
    ok = np.cumprod((e4 >= 0) & (e4 < G), axis=1).astype(bool)
    has = ok[:, 0]
    g = np.where(ok, e4, 0)
    P, M = gp[g], gM[g]                                                         # [N, 4, L, 3], [N, 4, 3, 3]
    local = lambda x: np.einsum("nkic,nkli->nklc", M, x)                        # noqa: E731  (M^T x)
    e = local(P[:, :, 1:] - P[:, :, :-1])
    D, A = (e * e[:, :1]).sum((-1, -2)), (e * e).sum((-1, -2))
    den = np.sqrt(A) * np.sqrt(A[:, :1])
    s = np.where(den > 0, D / np.where(den > 0, den, 1.0), 0.0)
    gated = tau is not None
    q = np.clip((s - tau) / (1 - tau), 0.0, 1.0) if gated and plant != "gate" else np.ones_like(s)
    q[:, 0] = 1.0
    d4 = np.where(ok, np.asarray(nd2, np.float32).astype(np.float64), 0.0)
    a = np.where(ok, q / (d4 + eps2), 0.0)
    W = a.sum(1)
    w = np.where(has[:, None], a / np.where(has, W, 1.0)[:, None], 0.0)
    if plant == "swap":
        w = w[:, [0, 2, 1, 3]]
    r = local(P - P[:, :, :1]) * ok[:, :, None, None]
    if plant == "lane":
        r = r.copy()
        for j in range(63, L, 64):
            r[:, :, j] = r[:, :, j - 1]
    Pl = (w[:, :, None, None] * r).sum(1)                                       # [N, L, 3]
    Mc = cM.transpose(0, 2, 1) if plant == "cM_T" else cM
    pts = co[:, None] + np.einsum("nrc,nlc->nlr", Mc, Pl)
    pts[:, 0] = co
    pts = np.where(has[:, None, None], pts, co[:, None])
    F = 0 if case["gf"] is None else case["gf"].shape[1]
    gf = np.zeros((G, 0)) if F == 0 else case["gf"].astype(np.float64)
    feat = gf[g] * ok[:, :, None]                                               # [N, 4, F]
    of = (w[:, :, None] * feat).sum(1)
    # the bounds
    n = L - 1
    c = 8 * n + 64
    E_w = 5 * (c * EPS / (1 - tau) + 16 * EPS) if gated else 5 * 16 * EPS
    per_k = (E_w + 16 * EPS * w) * ok                                           # [N, 4]
    r1 = np.abs(r).sum(-1)                                                      # [N, 4, L]
    b_pts = (per_k[:, :, None] * r1).sum(1) + 16 * EPS * (np.abs(co).max(1)[:, None] + np.abs(Pl).sum(-1))
    b_of = (per_k[:, :, None] * np.abs(feat)).sum(1)
    return dict(points=pts, weights=w, features=of, valid=has, b_points=np.repeat(b_pts[:, :, None], 3, 2), b_weights=E_w * ok,
                b_features=b_of)


@functools.lru_cache(maxsize=None)
def arbiter_of(index):
    """the arbiter's answer of case `index` on the model's table, computed once and shared"""
    nbr, nd2 = neighbours_of(index)
    return arbiter(cases()[index], nbr, nd2)


def excess(got, ref):
    """the largest |got - ref| / bound over points, weights and features (an element whose bound is 0 must be equal: then inf
    where it is not); got: dict(points, weights, features)"""
    worst = 0.0
    for key, b in (("points", "b_points"), ("weights", "b_weights"), ("features", "b_features")):
        x, y, bound = np.asarray(got[key], np.float64), ref[key], ref[b]
        if x.size == 0:
            continue
        assert x.shape == y.shape, (key, x.shape, y.shape)
        assert np.isfinite(x).all(), key
        err = np.abs(x - y)
        zero = bound == 0
        if (err[zero] > 0).any():
            return np.inf
        if (~zero).any():
            worst = max(worst, float((err[~zero] / bound[~zero]).max()))
    return worst
