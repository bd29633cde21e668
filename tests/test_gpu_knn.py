"""distCUDA2 (gaussianhaircut_amd/simple_knn, csrc/ghr_knn.h) on the MI355X: bit for bit against a brute force over every
pair, on clouds that stress the pruning (clusters with far outliers, lattice ties, exact duplicates, flat and linear
clouds, a far offset, squared distances that overflow), and deterministic across calls, streams and input order."""
import numpy as np
import pytest
import torch

from gaussianhaircut_amd.simple_knn import distCUDA2
from gaussianhaircut_amd.utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FLT_MAX = float(np.finfo(np.float32).max)


def brute(pts, queries=None):
    """The contract by brute force: separate torch elementwise ops in its order, the self pair set to inf, values clamped
    to FLT_MAX (a slot never takes them), three FLT_MAX slots appended for P <= 3, the three smallest by topk; the final
    ((b0 + b1) + b2) / 3 in numpy float32 (torch divides by a Python scalar as a multiplication by its reciprocal)."""
    P = pts.shape[0]
    qidx = torch.arange(P, device=pts.device) if queries is None else queries
    chunk = max(1, 2 ** 27 // max(P, 1))
    x, y, z = pts[:, 0][None], pts[:, 1][None], pts[:, 2][None]
    best = []
    for s in range(0, qidx.shape[0], chunk):
        qi = qidx[s:s + chunk]
        q = pts[qi]
        dx = x - q[:, 0:1]
        dy = y - q[:, 1:2]
        dz = z - q[:, 2:3]
        d = (dx * dx + dy * dy) + dz * dz
        del dx, dy, dz
        d[torch.arange(qi.shape[0], device=pts.device), qi] = float("inf")
        d = torch.cat((torch.clamp(d, max=FLT_MAX), torch.full((qi.shape[0], 3), FLT_MAX, device=pts.device)), 1)
        best.append(torch.topk(d, 3, dim=1, largest=False, sorted=True).values.cpu())
        del d
    b = torch.cat(best).numpy().astype(np.float32) if best else np.zeros((0, 3), np.float32)
    with np.errstate(over="ignore"):
        return ((b[:, 0] + b[:, 1]) + b[:, 2]) / np.float32(3.0)


def _uniform(P, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(P, 3, generator=g) * (hi - lo) + lo).to(DEV)


def _assert_bits(got, ref):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref.shape
    bad = got.view(np.int32) != ref.view(np.int32)
    assert not bad.any(), (int(bad.sum()), np.flatnonzero(bad)[:8], got[bad][:8], ref[bad][:8])


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 63, 64, 65, 4095, 4096, 4097, 100_000])
def test_uniform_clouds_match_the_brute_force_bit_for_bit(P):
    pts = _uniform(P, P)
    out = distCUDA2(pts)
    _assert_bits(out, brute(pts))
    if P <= 2:
        assert torch.isinf(out).all() and (out > 0).all()
    if P == 3:
        assert torch.isfinite(out).all() and (out > FLT_MAX / 4).all()


def _lattice():
    r = torch.arange(40, dtype=torch.float32)
    return torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)


def _copies():
    g = torch.Generator().manual_seed(5)
    three = torch.rand(3, 3, generator=g)
    pts = torch.cat((three.repeat(10_000, 1), torch.rand(50_000, 3, generator=g)))
    return pts[torch.randperm(pts.shape[0], generator=g)]


def _plane():
    g = torch.Generator().manual_seed(6)
    p = torch.rand(30_000, 3, generator=g)
    p[:, 2] = 0.5
    return p


def _line():
    g = torch.Generator().manual_seed(7)
    p = torch.zeros(30_000, 3)
    p[:, 0] = torch.rand(30_000, generator=g)
    return p


def _far():
    g = torch.Generator().manual_seed(8)
    return 1e4 + 1e-3 * torch.randn(20_000, 3, generator=g)


def _overflow():
    g = torch.Generator().manual_seed(9)
    return (torch.rand(20_000, 3, generator=g) * 2 - 1) * 1e20


CLOUDS = {
    "colmap_like_300k": lambda: syn.colmap_like_cloud(300_000, 1, n_duplicates=300)[0],
    "lattice_40cubed": _lattice,
    "3_points_x10000_plus_50k": _copies,
    "plane": _plane,
    "line": _line,
    "offset_1e4_noise_1e-3": _far,
    "spread_1e20_overflow": _overflow,
}


@pytest.mark.parametrize("name", list(CLOUDS))
def test_hard_clouds_match_the_brute_force_bit_for_bit(name):
    pts = CLOUDS[name]().to(DEV)
    out = distCUDA2(pts)
    ref = brute(pts)
    _assert_bits(out, ref)
    if name == "spread_1e20_overflow":
        assert np.isinf(ref).any() or (ref > 1e37).any()  # the case does reach overflowing squares


def test_two_million_points_against_the_brute_force_over_all_of_them():
    pts = syn.colmap_like_cloud(2_000_000, 2)[0].to(DEV)
    out = distCUDA2(pts)
    q = torch.randperm(pts.shape[0], generator=torch.Generator().manual_seed(3))[:4096].to(DEV)
    _assert_bits(out[q], brute(pts, q))


def test_bits_do_not_depend_on_the_call_the_stream_or_the_input_order():
    pts = syn.colmap_like_cloud(200_000, 4, n_duplicates=100)[0].to(DEV)
    a = distCUDA2(pts)
    b = distCUDA2(pts)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        c = distCUDA2(pts)
    torch.cuda.current_stream(DEV).wait_stream(side)
    perm = torch.randperm(pts.shape[0], generator=torch.Generator().manual_seed(4)).to(DEV)
    d = distCUDA2(pts[perm])
    for other in (b, c, d[torch.argsort(perm)]):
        assert torch.equal(a.view(torch.int32), other.view(torch.int32))


def test_dtypes_layouts_and_the_empty_cloud():
    pts = _uniform(5000, 11)
    ref = distCUDA2(pts)
    assert torch.equal(distCUDA2(pts.double()), ref)  # converted to fp32 first: the same points
    assert torch.equal(distCUDA2(pts.t().contiguous().t()), ref)  # non-contiguous
    out = distCUDA2(torch.empty(0, 3, device=DEV))
    assert out.shape == (0,) and out.dtype == torch.float32 and out.device == DEV


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_non_finite_coordinates_raise(bad):
    pts = _uniform(100, 12)
    pts[37, 1] = bad
    with pytest.raises(ValueError, match="non-finite"):
        distCUDA2(pts)


def test_shapes_are_checked():
    for shape in ((10, 2), (10,), (2, 10, 3)):
        with pytest.raises(ValueError):
            distCUDA2(torch.zeros(shape, device=DEV))
    with pytest.raises(ValueError):
        distCUDA2(torch.zeros(10, 3, dtype=torch.int32, device=DEV))
