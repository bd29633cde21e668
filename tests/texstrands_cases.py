"""Inputs and the ARBITER of the textured strand generator's tests (gaussianhaircut_amd/strand_generator.py,
csrc/ghr_texstrands.h).

``restate`` is a float64 restatement of the definition written for these tests.  It takes the stored taps as given -- ``x0, y0``
and ``fx, fy`` as float32 values, widened -- and shares no code with the package: the weights are formed, the taps gathered and
the lists walked here.  Every form (the HIP kernels, their host walks, the composed PyTorch form) is held against it under
    |got - f64| <= 1e-5 max|f64| + 3 |composed float32 - f64|        (DESIGN.md 8i's bar).
"""
import numpy as np
import torch

# UV layouts: what a kernel's tap logic can get wrong
UV_MODES = ("random", "one", "corners", "centres", "beyond", "leftout")


def scalp_grid(nu=5, nv=4, seed=0):
    """a small bent sheet of (nu x nv) vertices with UVs in [-0.9, 0.9]^2, two triangles a cell, and one degenerate face"""
    g = torch.Generator().manual_seed(seed)
    u, v = torch.meshgrid(torch.linspace(-0.9, 0.9, nu), torch.linspace(-0.9, 0.9, nv), indexing="ij")
    uv = torch.stack([u, v], -1).reshape(-1, 2)
    verts = torch.stack([uv[:, 0] * 0.1, uv[:, 1] * 0.08, 0.03 * torch.cos(2 * uv[:, 0]) + 0.01 * uv[:, 1] ** 2], -1)
    verts = verts + torch.randn(verts.shape, generator=g) * 1e-3
    faces = []
    for i in range(nu - 1):
        for j in range(nv - 1):
            a, b, c, d = i * nv + j, (i + 1) * nv + j, (i + 1) * nv + j + 1, i * nv + j + 1
            faces += [[a, b, c], [a, c, d]]
    faces.append([0, 0, 1])  # zero area
    return verts, torch.tensor(faces, dtype=torch.int64), uv


def uvs_for(mode, Smax, T, g):
    if mode == "random":
        return torch.rand(Smax, 2, generator=g) * 2 - 1
    if mode == "one":
        return torch.tensor([[0.123, -0.377]]).repeat(Smax, 1)
    if mode == "corners":
        c = torch.tensor([[-1.0, -1.0], [1.0, -1.0], [-1.0, 1.0], [1.0, 1.0]])
        return c[torch.arange(Smax) % 4]
    if mode == "centres":  # u = (2 i + 1) / T - 1: x = i exactly, fx = 0
        i = torch.randint(0, T, (Smax, 2), generator=g)
        return ((2 * i + 1).double() / T - 1).float()
    if mode == "beyond":   # finite, farther than 1 + 1/T on either side: every tap is dropped
        far = 1 + 1.0 / T + torch.rand(Smax, 2, generator=g) * 3 + 1e-3
        return far * torch.where(torch.rand(Smax, 2, generator=g) < 0.5, -1.0, 1.0)
    if mode == "leftout":  # the first quarter of the roots sits on one texel of its own; the draw will leave them all out
        uv = torch.rand(Smax, 2, generator=g) * 0.8 + 0.1
        uv[:max(Smax // 4, 1)] = torch.tensor([-0.61, -0.43])
        return uv
    raise ValueError(mode)


def make_case(T, C, Smax, S, L, mode="random", seed=0, scale=2.0):
    from gaussianhaircut_amd.strand_generator import texture_taps
    g = torch.Generator().manual_seed(9000 + seed)
    n = L - 1
    uvs = uvs_for(mode, Smax, T, g)
    q, r = torch.linalg.qr(torch.randn(Smax, 3, 3, generator=g, dtype=torch.float64))
    l2w = (q * torch.sign(torch.diagonal(r, dim1=-2, dim2=-1))[:, None, :]).float().contiguous()
    origins = (torch.rand(Smax, 3, generator=g) * 2 - 1) * 0.1
    if mode == "leftout":
        k = max(Smax // 4, 1)
        S = min(S, Smax - k) or 1
        idx = (k + torch.randperm(Smax - k, generator=g)[:S]) if Smax > k else torch.zeros(1, dtype=torch.int64)
    else:
        idx = torch.randperm(Smax, generator=g)[:S]
    S = int(idx.shape[0])
    c = dict(T=T, C=C, Smax=Smax, S=S, L=L, n=n, mode=mode, scale=scale, uvs=uvs, local2world=l2w, origins=origins, idx=idx,
             texture=torch.rand(1, C, T, T, generator=g) * 2 - 1, v=(torch.rand(S, n, 3, generator=g) * 2 - 1) * 0.01,
             d_z=torch.randn(S, C, generator=g), d_p=torch.randn(S, L, 3, generator=g), d_pl=torch.randn(S, L, 3, generator=g),
             taps=texture_taps(uvs, T))
    c["r64"] = restate(c)
    return c


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def lists_numpy(x0, y0, T):
    """(start [T T + 1], list) int32: per texel the 4 r + k inside the texture, ascending -- plain loops over integers"""
    x0, y0 = np.asarray(x0, np.int64), np.asarray(y0, np.int64)
    buckets = [[] for _ in range(T * T)]
    for r in range(len(x0)):
        for k in range(4):
            x, y = x0[r] + (k & 1), y0[r] + (k >> 1)
            if 0 <= x < T and 0 <= y < T:
                buckets[y * T + x].append(4 * r + k)
    start = np.zeros(T * T + 1, np.int32)
    start[1:] = np.cumsum([len(b) for b in buckets])
    return start, np.array([e for b in buckets for e in b], np.int32)


def restate(c, d_p=True, d_pl=True):
    """float64: z, d_texture (of sum z d_z, by a walk of the lists), p, p_local, d_v (of sum p d_p + sum p_local d_pl), pos"""
    T, C, S, Smax, n = c["T"], c["C"], c["S"], c["Smax"], c["n"]
    tp, idx = c["taps"], c["idx"]
    x0, y0 = tp.x0.long(), tp.y0.long()
    fx, fy = tp.fx.double(), tp.fy.double()
    tex = c["texture"].double()[0]
    w, inside, q = [], [], []
    for k in range(4):
        xk, yk = x0 + (k & 1), y0 + (k >> 1)
        inside.append((xk >= 0) & (xk < T) & (yk >= 0) & (yk < T))
        w.append((fx if k & 1 else 1 - fx) * (fy if k >> 1 else 1 - fy))
        q.append(yk.clamp(0, T - 1) * T + xk.clamp(0, T - 1))
    flat = tex.reshape(C, T * T)
    z = torch.zeros(S, C, dtype=torch.float64)
    for k in range(4):
        z += (w[k] * inside[k])[idx][:, None] * flat[:, q[k][idx]].t()
    pos = torch.full((Smax,), -1, dtype=torch.int64)
    pos[idx] = torch.arange(S)
    start, lst = lists_numpy(tp.x0.numpy(), tp.y0.numpy(), T)
    d_z = c["d_z"].double()
    d_tex = torch.zeros(C, T * T, dtype=torch.float64)
    wk = torch.stack(w, -1)                                              # [Smax, 4]
    for t in range(T * T):
        for e in lst[start[t]:start[t + 1]]:
            r, k = int(e) >> 2, int(e) & 3
            if pos[r] >= 0:
                d_tex[:, t] += wk[r, k] * d_z[pos[r]]
    v = c["v"].double().requires_grad_(True)
    inv = 1.0 / c["scale"]
    pl = torch.cat([torch.zeros(S, 1, 3, dtype=torch.float64), torch.cumsum(v, 1)], 1) * inv
    M = c["local2world"].double()[idx]
    p = c["origins"].double()[idx][:, None] + torch.einsum("sab,sjb->sja", M, pl)
    obj = (p * c["d_p"].double()).sum() * float(d_p) + (pl * c["d_pl"].double()).sum() * float(d_pl)
    (d_v,) = torch.autograd.grad(obj, v)
    return dict(z=z, d_texture=d_tex.reshape(1, C, T, T), p=p.detach(), p_local=pl.detach(), d_v=d_v, pos=pos,
                start=torch.from_numpy(start), list=torch.from_numpy(lst))


def assert_within(name, got, f64, other):
    """|got - f64| <= 1e-5 max|f64| + 3 |other - f64|, elementwise; prints the figures first"""
    got, f64, other = got.detach().double().cpu(), f64.detach().double().cpu(), other.detach().double().cpu()
    err, ref = (got - f64).abs(), (other - f64).abs()
    bar = 1e-5 * f64.abs().max() + 3 * ref
    print("%s: max |got - f64| = %.3e, max |other - f64| = %.3e, max|f64| = %.3e" % (
        name, float(err.max()) if err.numel() else 0.0, float(ref.max()) if ref.numel() else 0.0,
        float(f64.abs().max()) if f64.numel() else 0.0))
    assert got.shape == f64.shape and bool(torch.isfinite(got).all()) and bool((err <= bar).all()), (name, float((err - bar).max()))


# the smallest sizes at which the kernels can go wrong: T around the 64-texel workgroup (T T = 1, 4, 9, 25, 4096, 4225), C around
# the 64-channel pass, Smax / S around the wave, L - 1 around the scan's 64 lanes and two segments a lane
SHAPES = {}
for _T in (1, 2, 3, 5, 64, 65):
    SHAPES["T%d" % _T] = dict(T=_T, C=5, Smax=65, S=32, L=4)
for _C in (1, 63, 64, 65, 129):
    SHAPES["C%d" % _C] = dict(T=5, C=_C, Smax=63, S=31, L=3)
for _Smax in (1, 63, 64, 65, 300):
    for _S in sorted({1, max(_Smax // 2, 1), _Smax}):
        SHAPES["Smax%d-S%d" % (_Smax, _S)] = dict(T=3, C=3, Smax=_Smax, S=_S, L=3)
for _L in (2, 3, 65, 66, 100, 130):
    SHAPES["L%d" % _L] = dict(T=2, C=2, Smax=9, S=5, L=_L)
for _m in UV_MODES[1:]:
    SHAPES[_m] = dict(T=5, C=65, Smax=70, S=40, L=4, mode=_m)
SHAPES["one-T1"] = dict(T=1, C=2, Smax=64, S=64, L=2, mode="one")
SHAPES["corners-T1"] = dict(T=1, C=3, Smax=8, S=8, L=2, mode="corners")

_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = make_case(seed=sorted(SHAPES).index(name), **SHAPES[name])
    return _CASES[name]


class Linear3(torch.nn.Module):
    """stand-in strand decoder: one linear layer, [S, Cg] -> [S, n, 3]"""

    def __init__(self, Cg, n, seed=1):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.lin = torch.nn.Linear(Cg, 3 * n)
        with torch.no_grad():
            self.lin.weight.copy_(torch.randn(3 * n, Cg, generator=g) * 0.02)
            self.lin.bias.copy_(torch.randn(3 * n, generator=g) * 0.01)
        self.n = n

    def forward(self, z):
        return self.lin(z).view(z.shape[0], self.n, 3)


class LinearColour(torch.nn.Module):
    """stand-in colour decoder: [S, Ca - 1] -> [S, 3 (deg + 1)^2 + 1]"""

    def __init__(self, Cin, sh_degree=3, seed=2):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        out = 3 * (sh_degree + 1) ** 2 + 1
        self.lin = torch.nn.Linear(Cin, out)
        with torch.no_grad():
            self.lin.weight.copy_(torch.randn(out, Cin, generator=g) * 0.1)
            self.lin.bias.copy_(torch.randn(out, generator=g) * 0.1)

    def forward(self, z):
        return self.lin(z)


def tiny_generator(device="cpu", fused=True, prior=True, seed=3, Smax=200, S=64, L=8, T=16, Cg=6, Ca=5, dtype=torch.float32):
    """a TexturedStrands on scalp_grid() with the linear stand-ins and a quadratic prior, its texture filled from a seed"""
    from gaussianhaircut_amd.strand_generator import TexturedStrands
    g = torch.Generator().manual_seed(seed)
    target = torch.rand(1, Cg, T, T, generator=torch.Generator().manual_seed(seed + 1)).to(device=device, dtype=dtype)
    gen = TexturedStrands(scalp_grid(), Linear3(Cg, L - 1), LinearColour(Ca - 1), (lambda t: ((t - target) ** 2).mean()) if prior else None,
                          num_strands=S, max_num_strands=Smax, texture_size=T, geometry_channels=Cg, appearance_channels=Ca,
                          scale_decoder=2.0, generator=g, fused=fused)
    with torch.no_grad():
        gen.texture.copy_(torch.rand(gen.texture.shape, generator=torch.Generator().manual_seed(seed + 2)) * 2 - 1)
    gen = gen.to(device)
    if dtype != torch.float32:
        gen = gen.to(dtype)
    return gen
