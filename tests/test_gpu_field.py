"""The hair field, the strand trace and the resampling on the GPU (csrc/ghr_field.h), through the C ABI and through
strand_growing.py, on the shapes of tests/field_cases.py:

  * rho, v, c, n, path, steps, rgb and the resampled points equal the host walk (tests/hostsim/ghr_hostsim_field.cpp) BIT FOR BIT
    and meet the float64 arbiter under its bar; a second pass and permuted queries / roots give the same bits;
  * outputs are NaN-filled between guard words: every element is written and nothing beyond;
  * fused=True against fused=False under the bar; grow_strands end to end on the helix scene at S = 65."""
import ctypes

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd import strand_growing as sg
from gaussianhaircut_amd.simple_knn._C import _ptr, _stream
from tests import field_cases as fc
from tests import field_sim as fs
from tests.test_field_cpu import field_errors, teacher_forced

pytestmark = pytest.mark.gpu

GUARD = 64          # guard elements on either side of an output
POISON = 0x7fc00abc  # a NaN as float32, an impossible count as int32


@pytest.fixture(scope="module")
def sim():
    return fs.load()


def dev():
    return torch.device("cuda")


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def gpu_field(cloud):
    """the field on the GPU; ``cloud`` then holds the directions as the field holds them (normalised once more, on the device),
    so that the host walk and the arbiter work on the same bits"""
    fld = sg.HairField(D(cloud["points"]), D(cloud["directions"]), D(cloud["weights"]), D(cloud["colors"]))
    cloud["directions"] = fld.directions.cpu().numpy()
    assert np.array_equal(fld.points.cpu().numpy(), cloud["points"]) and np.array_equal(fld.weights.cpu().numpy(), cloud["weights"])
    return fld


class Guarded:
    """an output of ``numel`` 4-byte elements, every bit pattern POISON, between two runs of guard words"""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = shape, dtype
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), POISON, dtype=torch.int32, device=dev())

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + 4 * GUARD)

    def get(self):
        b = self.buf.cpu().numpy()
        assert np.all(b[:GUARD] == POISON) and np.all(b[GUARD + self.n:] == POISON), "a write outside the output"
        body = b[GUARD:GUARD + self.n]
        assert not np.any(body == POISON), "an element was not written"
        return body.view(self.dtype).reshape(self.shape).copy()


def abi_query(fld, x, t, r2, order=None):
    Q = x.shape[0]
    out = [Guarded((Q,), np.float32), Guarded((Q, 3), np.float32), Guarded((Q, 3), np.float32), Guarded((Q,), np.int32)]
    xd, td = D(x), D(t)
    od = None if order is None else D(np.ascontiguousarray(order, np.int64))
    _lib.check(_lib.lib().ghr_field_query(_stream(), fld.P, _ptr(fld.workspace()), Q, _ptr(xd), _ptr(td), _ptr(od), float(r2),
                                          *[o.ptr() for o in out]))
    torch.cuda.synchronize()
    return [o.get() for o in out]


def abi_trace(fld, roots, normals, M, r2, h, beta, rho_min, coast, order=None):
    S = roots.shape[0]
    out = [Guarded((S, M + 1, 3), np.float32), Guarded((S,), np.int32), Guarded((S, 3), np.float32)]
    rd, nd = D(roots), D(normals)
    od = None if order is None else D(np.ascontiguousarray(order, np.int64))
    f = lambda v: float(np.float32(v))
    _lib.check(_lib.lib().ghr_field_trace(_stream(), fld.P, _ptr(fld.workspace()), S, _ptr(rd), _ptr(nd), _ptr(od), M, float(r2), f(h),
                                          f(beta), f(rho_min), coast, *[o.ptr() for o in out]))
    torch.cuda.synchronize()
    return [o.get() for o in out]


def abi_resample(path, steps, L):
    S, M = path.shape[0], path.shape[1] - 1
    out = Guarded((S, L, 3), np.float32)
    pd, sd = D(path), D(np.ascontiguousarray(steps, np.int32))
    _lib.check(_lib.lib().ghr_strands_resample(_stream(), S, M, L, _ptr(pd), _ptr(sd), out.ptr()))
    torch.cuda.synchronize()
    return out.get()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- the field -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.ALL_QUERY_CASES)
def test_query_equals_the_host_walk_bit_for_bit_and_meets_the_arbiter(sim, name):
    c = fc.query_case(name)
    fld = gpu_field(c["cloud"])
    want = fs.query(sim, c["cloud"], c["x"], c["t"], c["r2"])[:4]
    got = abi_query(fld, c["x"], c["t"], c["r2"])
    for g, w, what in zip(got, want, ("rho", "v", "c", "n")):
        assert same_bits(g, w), what
    e = field_errors(got, fc.field64(c["cloud"], c["x"], c["t"], c["r2"]), c["cloud"])
    assert max(e) <= fc.BAR_FIELD, e
    Q = c["x"].shape[0]
    perm = np.random.default_rng(3).permutation(Q)
    for again in (abi_query(fld, c["x"], c["t"], c["r2"]), abi_query(fld, c["x"], c["t"], c["r2"], order=perm)):
        for g, w in zip(again, got):                                       # a second pass; the queries in another order
            assert same_bits(g, w)
    py = fld.query(D(c["x"]), D(c["t"]), radius=c["r"], fused=True)         # through Python (queries in key order past one wave)
    for g, w in zip(py, got):
        assert same_bits(g.cpu().numpy(), w)
    alone = abi_query(fld, c["x"][Q // 2:Q // 2 + 1], c["t"][Q // 2:Q // 2 + 1], c["r2"])
    for g, w in zip(alone, got):
        assert same_bits(g[0], w[Q // 2])


def test_fused_query_against_the_composed_form_under_the_bar():
    for name in ("P4097", "duplicates", "everything", "far_large_r"):
        c = fc.query_case(name)
        fld = gpu_field(c["cloud"])
        r = c["r"]
        a = [t.cpu().numpy() for t in fld.query(D(c["x"]), D(c["t"]), radius=r, fused=True)]
        b = [t.cpu().numpy().astype(np.float64) if i < 3 else t.cpu().numpy() for i, t in
             enumerate(fld.query(D(c["x"]), D(c["t"]), radius=r, fused=False))]
        e = field_errors(a, b, c["cloud"])
        print(name, "fused against composed, of the bar:", [x / fc.BAR_FIELD for x in e])
        assert max(e) <= fc.BAR_FIELD, (name, e)
    with pytest.raises(ValueError, match="fused=True"):
        fld.query(D(c["x"]).cpu(), D(c["t"]).cpu(), radius=r, fused=True)


# ---- the trace -------------------------------------------------------------------------------------------------------------------
def _host(sim, scene, M, coast, a):
    return fs.trace(sim, scene["cloud"], scene["roots"], scene["normals"], M, fc.r2_of(a["r"]), a["h"], a["beta"], a["rho_min"], coast)


def _gpu(fld, scene, M, coast, a, order=None):
    return abi_trace(fld, scene["roots"], scene["normals"], M, fc.r2_of(a["r"]), a["h"], a["beta"], a["rho_min"], coast, order)


@pytest.mark.parametrize("coast", fc.TRACE_COAST)
@pytest.mark.parametrize("S", fc.TRACE_S)
def test_trace_equals_the_host_walk_bit_for_bit_and_meets_the_arbiter(sim, S, coast):
    scene, a = fc.small_scene(S), fc.TRACE_ARGS
    fld = gpu_field(scene["cloud"])
    for M in fc.TRACE_M:
        want = _host(sim, scene, M, coast, a)
        got = _gpu(fld, scene, M, coast, a)
        for g, w, what in zip(got, want, ("path", "steps", "rgb")):
            assert same_bits(g, w), (what, M)
        e_field, e_point = teacher_forced(scene, (got[0], got[1], got[2], want[3]), M, coast, a)
        assert e_field <= fc.BAR_FIELD and e_point <= fc.BAR_POINT
        for L in fc.RESAMPLE_L:
            assert same_bits(abi_resample(got[0], got[1], L), fs.resample(sim, want[0], want[1], L)), (M, L)
    key_order, _ = fs.key_order(sim, scene["roots"])
    for order in (key_order, np.arange(S)[::-1].copy(), None):              # other company, other order, a second pass
        for g, w in zip(_gpu(fld, scene, 40, coast, a, order), got):
            assert same_bits(g, w)
    perm = np.random.default_rng(S).permutation(S)                          # permuted roots give the same rows
    moved = dict(scene, roots=scene["roots"][perm], normals=scene["normals"][perm])
    for g, w in zip(_gpu(fld, moved, 40, coast, a), got):
        assert same_bits(g, w[perm])


def test_gaps_and_a_strand_without_support_as_the_host_walk(sim):
    for name, (coast, k, _gap, crosses) in fc.GAP_CASES.items():
        scene, a = fc.line_scene(k), fc.LINE_ARGS
        fld = gpu_field(scene["cloud"])
        want, got = _host(sim, scene, a["M"], coast, a), _gpu(fld, scene, a["M"], coast, a)
        for g, w in zip(got, want):
            assert same_bits(g, w), name
        assert (got[1][0] > 17) == crosses
    scene = fc.small_scene(3)
    scene["roots"][1] = (30.0, 30.0, 30.0)
    got = _gpu(gpu_field(scene["cloud"]), scene, 7, 2, fc.TRACE_ARGS)
    assert got[1][1] == 0 and not got[2][1].any() and got[1][0] > 0
    for g, w in zip(got, _host(sim, scene, 7, 2, fc.TRACE_ARGS)):
        assert same_bits(g, w)


@pytest.mark.parametrize("L", fc.RESAMPLE_L)
def test_resampling_equals_the_host_walk_bit_for_bit(sim, L):
    steps = np.array(fc.resample_steps(L), np.int32)
    M = int(steps.max()) + 2
    path = np.random.default_rng(L).normal(size=(len(steps), M + 1, 3)).astype(np.float32)
    got = abi_resample(path, steps, L)
    assert same_bits(got, fs.resample(sim, path, steps, L))
    assert np.all(np.abs(got - fc.resample64(path, steps, L)) <= 8 * 2.0 ** -24 * np.abs(path).max())
    py = sg.resample_strands(D(path), D(steps), L)
    assert same_bits(py.cpu().numpy(), got)
    assert same_bits(sg.resample_strands(D(path), D(steps), L, fused=False).cpu().numpy(), got)   # the same expressions elementwise


def test_fused_step_against_the_composed_form_under_the_bar(sim):
    """one step from every state the walk visited (divergence along a trajectory never enters)"""
    scene, a = fc.small_scene(65), fc.TRACE_ARGS
    fld = gpu_field(scene["cloud"])
    log = _host(sim, scene, 40, 2, a)[3]
    made = ~np.isnan(log[..., 13])
    x, t = np.ascontiguousarray(log[made][:, 0:3]), np.ascontiguousarray(log[made][:, 3:6])
    kw = dict(L=2, radius=a["r"], step=a["h"], max_steps=1, rho_min=a["rho_min"], beta=a["beta"], max_coast=1, min_steps=0)
    f, c = sg.grow_strands(fld, D(x), D(t), fused=True, **kw), sg.grow_strands(fld, D(x), D(t), fused=False, **kw)
    assert torch.equal(f["steps"], c["steps"]) and int(f["steps"].sum()) > 1000
    e = float((f["path"][:, 1] - c["path"][:, 1]).abs().max()) / a["h"]
    print("fused against composed next point, of the bar:", e / fc.BAR_POINT)
    assert e <= fc.BAR_POINT


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_grow_strands_grows_the_helix_bundle():
    scene = fc.helix_scene(S=65)
    fld = gpu_field(scene["cloud"])
    out = sg.grow_strands(fld, D(scene["roots"]), D(scene["normals"]), radius=fc.HELIX_R, step=fc.HELIX_H)
    assert out["path"].shape == (65, 401, 3) and bool(out["keep"].all()) and out["points"].shape == (65, 100, 3)
    steps = out["steps"].cpu().numpy()
    fc.assert_grown_hair(out["path"].cpu().numpy(), steps, scene["curves"])
    pts = out["points"].cpu().numpy()
    assert np.all(pts[:, 0] == scene["roots"]) and np.array_equal(pts[:, -1], out["path"].cpu().numpy()[np.arange(65), steps])
    rgb = out["rgb"].cpu().numpy()
    assert rgb.shape == (65, 3) and rgb.min() >= 0 and rgb.max() <= 1       # a weighted mean of colours in [0, 1]
    from gaussianhaircut_amd.scene.gaussian_model_strands import GaussianModelStrands
    m = GaussianModelStrands(0).create_from_polylines(out["points"], out["rgb"])
    assert m.get_xyz.shape == (65 * 99, 3) and m.get_xyz.is_cuda


def test_the_look_defaults_are_the_composed_forms():
    scene = fc.small_scene(5)
    fld = gpu_field(scene["cloud"])
    cpu = sg.HairField(*[torch.from_numpy(scene["cloud"][k]) for k in ("points", "directions", "weights", "colors")])
    auto = fld.default_radius()
    assert abs(auto - cpu.default_radius(fused=False)) <= 1e-6 * auto and 0.001 < auto < 0.1
    rho_min = fld.default_rho_min(fc.HELIX_R)
    assert abs(rho_min - cpu.default_rho_min(fc.HELIX_R, fused=False)) <= 1e-5 * rho_min
    out = sg.grow_strands(fld, D(scene["roots"]), D(scene["normals"]), L=7, max_steps=9, min_steps=1)
    assert out["radius"] == auto and abs(out["step"] - auto / 2.5) <= 1e-7 and out["points"].shape[1:] == (7, 3)
