"""Inputs and the ARBITER of the strand prior's tests (gaussianhaircut_amd/strand_prior.py, csrc/ghr_sds.h).

``restate`` is a PyTorch restatement of the block's definition written for these tests, generic in its dtype: in float64 it is
what every form is held against; in float32 it is one more form.  It shares no code with the package.
``recipe`` makes the inputs (the golden generator tests/golden/make_reference_sds_golden.py uses it too): UVs uniform in
[-1, 1]^2, orthonormal local2world from a QR, and -- in each strand's LOCAL frame -- segments 0.004 (u, v, 1) + noise of
amplitude 0.0002 + 0.004 (u + 1) / 2, so that neighbouring strands are nearly parallel at u = -1 (csim > 0.9) and not at u = +1.
The golden's inputs are stored in its fixture files whole; only the small cases are made from the recipe when the tests run.
"""
import numpy as np
import torch

K = 4
GOLDEN = dict(S=1200, N=1000, n=99, G=32, C=64, scale=50.0, seed=20251)


def recipe(S, n, seed, origin_radius=0.1):
    g = torch.Generator().manual_seed(seed)
    uvs = torch.rand(S, 2, generator=g) * 2 - 1
    q, r = torch.linalg.qr(torch.randn(S, 3, 3, generator=g, dtype=torch.float64))
    l2w = (q * torch.sign(torch.diagonal(r, dim1=-2, dim2=-1))[:, None, :]).float().contiguous()
    noise = torch.rand(S, n, 3, generator=g) * 2 - 1
    amp = (0.0002 + 0.004 * (uvs[:, 0] + 1) / 2)[:, None, None]
    base = torch.stack([uvs[:, 0], uvs[:, 1], torch.ones(S)], dim=-1)[:, None, :] * 0.004
    local = base + noise * amp
    lx, ly, lz = local[..., 0], local[..., 1], local[..., 2]
    R = l2w[:, None]
    dirs = torch.stack([(R[..., r_, 0] * lx + R[..., r_, 1] * ly) + R[..., r_, 2] * lz for r_ in range(3)], dim=-1).contiguous()
    origins = torch.nn.functional.normalize(torch.rand(S, 1, 3, generator=g) * 2 - 1, dim=-1) * origin_radius
    return dict(uvs=uvs, local2world=l2w, dirs=dirs, origins=origins)


def encoder_weights(n, C, seed, extra=3):
    """W of the stand-in encoder tanh(flatten(e) @ W): [3 (n + 1), C + extra] (the block takes the first C columns)"""
    g = torch.Generator().manual_seed(seed + 1)
    return torch.randn(3 * (n + 1), C + extra, generator=g) * 0.004


def target_texture(C, G, seed):
    g = torch.Generator().manual_seed(seed + 2)
    return torch.rand(1, C, G, G, generator=g) * 2 - 1


def make_encoder(W):
    return lambda e: torch.tanh(e.flatten(1) @ W.to(e.device, e.dtype))


def small_case(G, N, n, C, S=None, seed=0, idx=None):
    """a case of the recipe at a small size; idx drawn with replacement unless given"""
    S = max(N + 3, 8) if S is None else S
    inp = recipe(S, n, 1000 + seed)
    g = torch.Generator().manual_seed(5000 + seed)
    inp["idx"] = torch.randint(0, S, (N,), generator=g) if idx is None else torch.as_tensor(idx, dtype=torch.int64)
    inp["W"] = encoder_weights(n, C, seed) * (20.0 / max(n, 4))
    inp["T0"] = target_texture(C, G, seed)
    inp.update(G=G, N=N, n=n, C=C, S=S, scale=50.0)
    return inp


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def restate(dirs, local2world, uvs, idx, scale, G, C, W, T0, dtype=torch.float64, device="cpu", z_detached=False, v_detached=False,
            d_texture=None):
    """Steps 1 - 4 in ``dtype``.  Returns a dict of detached results; ``d_dirs`` is of ``((texture - T0)^2).mean()`` or, with
    ``d_texture``, of ``(texture * d_texture).sum()``."""
    dev = torch.device(device)
    dirs = dirs.detach().to(dev, dtype).requires_grad_(True)
    idx = idx.to(dev)
    Minv = torch.linalg.inv(local2world.to(dev).double()).to(dtype)[idx]
    uvg = uvs.to(dev, dtype)[idx]
    N, n = idx.shape[0], dirs.shape[1]
    d = dirs[idx]
    P = torch.cat([torch.zeros(N, 1, 3, dtype=dtype, device=dev), torch.cumsum(d, 1)], 1)
    e = torch.einsum("gab,gjb->gja", Minv, P) * scale
    v = torch.einsum("gab,gjb->gja", Minv, d) * scale
    z = torch.tanh(e.flatten(1) @ W.to(dev, dtype))[:, :C]
    zt, vt = (z.detach() if z_detached else z), (v.detach() if v_detached else v)
    edges = torch.linspace(-1, 1, G + 1, dtype=torch.float32, device=dev)      # float32 as the reference forms them, then widened
    c = ((edges[1:] + edges[:-1]) / 2).to(dtype)
    cx, cy = c.repeat(G), c.repeat_interleave(G)                                # texel q = row G + col at (c[col], c[row])
    d2 = (cx[:, None] - uvg[None, :, 0]) ** 2 + (cy[:, None] - uvg[None, :, 1]) ** 2
    sd, order = torch.sort(d2, dim=1, stable=True)
    nbr, kd = order[:, :K], sd[:, :K]
    w = 1 / (kd + 1e-7)
    w = w / w.sum(1, keepdim=True)
    a = vt[nbr[:N]]                                                              # [N, 4, n, 3]
    u = a / _clamped_norm(a)
    full = (u[:, :, None] * u[:, None, :]).sum(-1).mean(-1)                      # [N, 4, 4]
    pairs = [(j, k) for j in range(K) for k in range(j, K)]
    csim = torch.stack([full[:, j, k] for j, k in pairs], -1).mean(-1)
    alpha = torch.where(csim <= 0.9, 1 - 1.63 * csim ** 5, 0.4 - 0.4 * csim)
    alpha_q = (alpha[nbr] * w).sum(1, keepdim=True)
    z_q = zt[nbr[:, 0]] * alpha_q + (zt[nbr] * w[..., None]).sum(1) * (1 - alpha_q)
    texture = z_q.reshape(G, G, C).permute(2, 0, 1)[None]
    loss = ((texture - T0.to(dev, dtype)) ** 2).mean() if d_texture is None else (texture * d_texture.to(dev, dtype)).sum()
    (d_dirs,) = torch.autograd.grad(loss, dirs)
    flat = nbr.reshape(-1)
    entries = torch.sort(flat, stable=True)[1]
    start = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(torch.bincount(flat, minlength=N), 0)])
    out = dict(e=e, v=v, z=z, nbr=nbr, w=w, csim=csim, alpha=alpha, alpha_q=alpha_q[:, 0], texture=texture, loss=loss, d_dirs=d_dirs,
               sorted_d2=sd[:, :K + 1] if N > K else sd[:, :K], start=start, entries=entries)
    return {k: t.detach() for k, t in out.items()}


def _clamped_norm(a):
    """max(|a|, 1e-8) whose derivative is the norm's (the clamp passes it), as F.cosine_similarity has it"""
    nrm = a.norm(dim=-1, keepdim=True)
    return nrm + (nrm.detach().clamp_min(1e-8) - nrm.detach())


def input_conditions(r64, N, exact_ties=False):
    """(smallest relative gap among each texel's five smallest distances, smallest |csim - 0.9|, share of csim above 0.9).
    ``exact_ties``: gaps of exactly 0 -- a strand drawn twice, which ties in every precision and goes to the tie rule -- are
    left out of the smallest gap."""
    sd = r64["sorted_d2"]
    gaps = (sd[:, 1:] - sd[:, :-1]) / sd[:, 1:].clamp_min(1e-300)
    if exact_ties:
        gaps = torch.where(gaps == 0, torch.ones_like(gaps), gaps)
    gap = gaps.min()
    cs = r64["csim"]
    return float(gap), float((cs - 0.9).abs().min()), float((cs > 0.9).double().mean())


def arbiter_bar(f64, composed=None, golden=None):
    """elementwise bound 1e-5 max|f64| + 3 |other - f64| (``other``: the composed float32 form, or the golden)"""
    other = composed if composed is not None else golden
    return 1e-5 * f64.abs().max() + 3 * (other.double().cpu() - f64.cpu()).abs()


def assert_within(name, got, f64, other):
    got, f64 = got.detach().double().cpu(), f64.detach().double().cpu()
    bar = arbiter_bar(f64, other.detach())
    err = (got - f64).abs()
    worst = float((err - bar).max())
    print("%s: max |got - f64| = %.3e, max |other - f64| = %.3e, max|f64| = %.3e" % (
        name, float(err.max()), float((other.detach().double().cpu() - f64).abs().max()), float(f64.abs().max())))
    assert got.shape == f64.shape and bool(torch.isfinite(got).all()) and worst <= 0.0, (name, worst, float(err.max()))


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# the smallest sizes at which a mapping decision changes: G G against N against the wave's 64 lanes; n and C around 64
GN = [(2, 4), (3, 5), (3, 9), (8, 4), (8, 63), (8, 64), (9, 65), (12, 129)]
SMALL = {"G%d-N%d" % gn: dict(G=gn[0], N=gn[1], n=5, C=6) for gn in GN}
SMALL.update({"n%d" % n: dict(G=3, N=9, n=n, C=6) for n in (1, 2, 63, 64, 65, 99)})
SMALL.update({"C%d" % C: dict(G=3, N=7, n=4, C=C) for C in (1, 63, 64, 65)})
SMALL["one-strand"] = dict(G=3, N=6, n=5, C=6, S=1, idx=[0] * 6)                       # every distance ties
SMALL["duplicates"] = dict(G=4, N=12, n=7, C=6, S=9, idx=[3, 5, 3, 0, 8, 3, 5, 1, 3, 2, 7, 8])  # strand 3 four times


def restate_case(c, dtype=torch.float64, **kw):
    return restate(c["dirs"], c["local2world"], c["uvs"], c["idx"], c["scale"], c["G"], c["C"], c["W"], c["T0"], dtype=dtype, **kw)


_CASES = {}


def case(name):
    """the inputs of a small case with its float64 (``r64``) and float32 (``r32``) restatements, computed once"""
    if name not in _CASES:
        c = small_case(seed=sorted(SMALL).index(name), **SMALL[name])
        c["r64"], c["r32"] = restate_case(c), restate_case(c, torch.float32)
        _CASES[name] = c
    return _CASES[name]


def golden_case():
    """tests/golden/reference_sds_golden*.npz: the inputs, the reference's float32 results (``want``; ``d_dirs`` rebuilt whole from
    its drawn rows, the rest is zero) and the restatements, computed once"""
    import os
    if "golden" not in _CASES:
        here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        load = lambda tag: np.load(os.path.join(here, "reference_sds_golden%s.npz" % tag))  # noqa: E731
        g = load("")
        T = lambda a: torch.from_numpy(np.asarray(a))  # noqa: E731
        inp = {k: T(g[k]) for k in ("uvs", "local2world", "origins", "W", "T0", "idx")}
        inp["dirs"] = torch.cat([T(load("_dirs_a")["dirs"]), T(load("_dirs_b")["dirs"])])
        G = GOLDEN
        inp.update(scale=G["scale"], G=G["G"], C=G["C"], N=G["N"], n=G["n"], S=G["S"])
        assert inp["dirs"].shape == (G["S"], G["n"], 3) and inp["idx"].shape == (G["N"],)
        d_dirs = torch.zeros_like(inp["dirs"])
        d_dirs[inp["idx"]] = torch.cat([T(load("_ddirs_a")["d_dirs_rows"]), T(load("_ddirs_b")["d_dirs_rows"])])
        inp["want"] = dict(texture=T(g["texture"]), loss=T(g["loss"]), d_dirs=d_dirs)
        inp["r64"], inp["r32"] = restate_case(inp), restate_case(inp, torch.float32)
        _CASES["golden"] = inp
    return _CASES["golden"]


def quadratic_prior(T0):
    return lambda t: ((t - T0.to(t.device, t.dtype)) ** 2).mean(dim=(1, 2, 3))


def tiny_prior(S, n, device="cpu", seed=11, fused=None, loss=None):
    """a StrandPrior for a strand model of S strands of n segments: 8 guiding strands, a 3 x 3 texture of 4 channels"""
    from gaussianhaircut_amd.strand_prior import StrandPrior
    inp = recipe(S, n, 77)
    W, T0 = encoder_weights(n, 4, 5) * 10, target_texture(4, 3, 5)
    g = torch.Generator(device=device).manual_seed(seed)
    prior = StrandPrior(make_encoder(W.to(device)), loss or quadratic_prior(T0.to(device)), inp["uvs"].to(device),
                        inp["local2world"].to(device), 3, 50.0, num_guiding=8, channels=4, generator=g, fused=fused)
    prior.test_inputs = dict(uvs=inp["uvs"], local2world=inp["local2world"], W=W, T0=T0, G=3, C=4, scale=50.0)  # for restate()
    return prior
