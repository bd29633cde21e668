"""The guarded trace on the GPU (csrc/ghr_grow.h), through the C ABI and through strand_growing.py, on the cases of
tests/grow_cases.py:

  * path, steps, rgb, contacts and stop equal the host walk (tests/hostsim/ghr_hostsim_grow.cpp) BIT FOR BIT on every case and at
    S = 1, 63, 64, 65, 130 roots; a second pass, a permuted root_order and NULL give the same bits;
  * outputs are NaN- and 0xFF-filled between guard words: every element is written and nothing beyond;
  * fused=True against fused=False under the bar, one step from every state the walk visited;
  * k_meshdist_search, whose wave loop the kernel shares, through HeadMesh.closest_point against the numpy model, bit for bit;
  * grow_strands(avoid=True) on the head scene at S = 65 with the CPU test's assertions."""
import ctypes

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd import strand_growing as sg
from gaussianhaircut_amd.simple_knn._C import _ptr, _stream
from tests import field_cases as fc
from tests import grow_cases as gc
from tests import grow_sim as gs
from tests.test_gpu_field import GUARD, D, Guarded, dev, gpu_field, same_bits
from tests.test_grow_guarded_cpu import assert_the_head_is_avoided, grow_pair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sim():
    return gs.load()


class GuardedBytes:
    """an output of ``n`` bytes, every one 0xFF (no stop reason), between two runs of guard bytes"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=dev())

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + GUARD)

    def get(self):
        b = self.buf.cpu().numpy()
        assert np.all(b[:GUARD] == 0xFF) and np.all(b[GUARD + self.n:] == 0xFF), "a write outside the output"
        body = b[GUARD:GUARD + self.n]
        assert not np.any(body == 0xFF), "an element was not written"
        return body.copy()


def own(c):
    """a case whose cloud this test may rewrite (gpu_field stores the directions as the field holds them)"""
    return dict(c, cloud=dict(c["cloud"]))


def abi_guarded(fld, mesh, c, order=None, roots=None, normals=None):
    roots, normals = c["roots"] if roots is None else roots, c["normals"] if normals is None else normals
    S, M = roots.shape[0], c["M"]
    out = [Guarded((S, M + 1, 3), np.float32), Guarded((S,), np.int32), Guarded((S, 3), np.float32), Guarded((S,), np.int32),
           GuardedBytes(S)]
    rd, nd = D(roots), D(normals)
    od = None if order is None else D(np.ascontiguousarray(order, np.int64))
    f = lambda v: float(np.float32(v))
    tris, _ = mesh._tris_tables(dev())
    grid = mesh._tables(dev())
    _lib.check(_lib.lib().ghr_field_trace_guarded(
        _stream(), fld.P, _ptr(fld.workspace()), ctypes.byref(mesh._tris_header), _ptr(tris), ctypes.byref(mesh.header), _ptr(grid), S,
        _ptr(rd), _ptr(nd), _ptr(od), M, float(fc.r2_of(c["r"])), f(c["h"]), f(c["beta"]), f(c["rho_min"]), c["max_coast"],
        f(c["margin"]), *[o.ptr() for o in out]))
    torch.cuda.synchronize()
    return [o.get() for o in out]


def host(sim, c):
    return gs.trace(sim, c["cloud"], gc.head_mesh(c["mesh_name"]), c["roots"], c["normals"], c["M"], fc.r2_of(c["r"]), c["h"], c["beta"],
                    c["rho_min"], c["max_coast"], c["margin"])


NAMES = ("path", "steps", "rgb", "contacts", "stop")


def bits_equal(got, want, why):
    for g, w, what in zip(got, want, NAMES):
        assert (np.array_equal(g, w) if g.dtype == np.uint8 else same_bits(g, w)), (what, why)


def check_against_the_walk(sim, c):
    c = own(c)
    fld, mesh = gpu_field(c["cloud"]), gc.head_mesh(c["mesh_name"])
    want = host(sim, c)[:5]
    got = abi_guarded(fld, mesh, c)
    bits_equal(got, want, "the host walk")
    S = c["roots"].shape[0]
    for order in (np.random.default_rng(S).permutation(S), np.arange(S)[::-1].copy(), None):   # other company; a second pass
        bits_equal(abi_guarded(fld, mesh, c, order), got, "root_order")
    return fld, mesh, c, got


@pytest.mark.parametrize("name", gc.ALL_CASES)
def test_every_output_equals_the_host_walk_bit_for_bit(sim, name):
    fld, mesh, c, got = check_against_the_walk(sim, gc.case(name))
    if name == "mixed":
        assert set(np.unique(got[4])) == {gc.STOP_STEPS, gc.STOP_COAST, gc.STOP_HEADON}
        perm = np.random.default_rng(2).permutation(c["roots"].shape[0])    # permuted roots give the same rows
        bits_equal(abi_guarded(fld, mesh, c, roots=c["roots"][perm], normals=c["normals"][perm]), [g[perm] for g in got], "moved")
        py = fld.trace_guarded_hip(mesh, D(c["roots"]), D(c["normals"]), c["M"], float(fc.r2_of(c["r"])), float(np.float32(c["h"])),
                                   float(np.float32(c["beta"])), float(np.float32(c["rho_min"])), c["max_coast"],
                                   float(np.float32(c["margin"])))
        bits_equal([t.cpu().numpy() for t in py], got, "through Python, roots in key order")


@pytest.mark.parametrize("S", (1, 63, 64, 65, 130))
def test_every_output_equals_the_host_walk_at_wave_tails(sim, S):
    check_against_the_walk(sim, gc.sized_scene(S))


def test_a_strand_that_is_not_finite_asks_nothing_and_every_element_is_written(sim):
    c = own(gc.sized_scene(65))
    c["roots"] = c["roots"].copy()
    c["roots"][3] = (np.inf, 0.0, 0.0)
    c["roots"][64] = (50.0, 50.0, 50.0)
    fld, mesh = gpu_field(c["cloud"]), gc.head_mesh(c["mesh_name"])
    S, M = 65, c["M"]
    out = [torch.full((S, M + 1, 3), 7.0, device=dev()), torch.full((S,), -1, dtype=torch.int32, device=dev()),
           torch.full((S, 3), 7.0, device=dev()), torch.full((S,), -1, dtype=torch.int32, device=dev()),
           torch.full((S,), 0xFF, dtype=torch.uint8, device=dev())]
    tris, _ = mesh._tris_tables(dev())
    f = lambda v: float(np.float32(v))
    rd, nd = D(c["roots"]), D(c["normals"])
    _lib.check(_lib.lib().ghr_field_trace_guarded(
        _stream(), fld.P, _ptr(fld.workspace()), ctypes.byref(mesh._tris_header), _ptr(tris), ctypes.byref(mesh.header),
        _ptr(mesh._tables(dev())), S, _ptr(rd), _ptr(nd), None, M, float(fc.r2_of(c["r"])), f(c["h"]),
        f(c["beta"]), f(c["rho_min"]), c["max_coast"], f(c["margin"]), *[_ptr(o) for o in out]))
    torch.cuda.synchronize()
    got = [o.cpu().numpy() for o in out]
    want = host(sim, c)[:5]
    for g, w, what in zip(got, want, NAMES):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), what      # (NaN rows included: the same bits)
    assert got[1][3] == 0 and got[3][3] == 0 and got[4][3] == gc.STOP_COAST and got[4][64] == gc.STOP_COAST


def test_fused_step_against_the_composed_form_under_the_bar(sim):
    """one step from every state the walk visited (divergence along a trajectory never enters)"""
    for name in ("mixed", "ico0", "planted_cube"):
        c = own(gc.case(name))
        fld, mesh = gpu_field(c["cloud"]), gc.head_mesh(c["mesh_name"])
        log = host(sim, c)[5]
        made = ~np.isnan(log[..., 25])
        x, t = np.ascontiguousarray(log[made][:, 0:3]), np.ascontiguousarray(log[made][:, 3:6])
        kw = dict(L=2, radius=c["r"], step=c["h"], max_steps=1, rho_min=c["rho_min"], beta=c["beta"], max_coast=1, min_steps=0,
                  mesh=mesh, avoid=True, margin=c["margin"])
        f = sg.grow_strands(fld, D(x), D(t), fused=True, **kw)
        g = sg.grow_strands(fld, D(x), D(t), fused=False, **kw)
        for k in ("steps", "contacts", "stop"):
            assert torch.equal(f[k], g[k]), (name, k)
        e = float((f["path"][:, 1] - g["path"][:, 1]).abs().max()) / c["h"]
        print(name, "fused against composed next point, of the bar:", e / gc.BAR_PUSH, "states", x.shape[0])
        assert e <= gc.BAR_PUSH


def test_the_mesh_search_still_answers_as_its_model():
    """k_meshdist_search after its wave loop moved into md_wave_search: one case on bits (tests/test_gpu_mesh_distance.py has the rest)"""
    from tests import mesh_distance_cases as mdc
    q, dist2, face, point = mdc.expected("ico4_5120")
    v, f, _ = mdc.meshes()["ico4_5120"]
    from gaussianhaircut_amd.mesh import HeadMesh
    got = HeadMesh(v, f).closest_point(D(q))
    assert same_bits(got[0].cpu().numpy(), dist2) and np.array_equal(got[1].cpu().numpy(), face)
    assert same_bits(got[2].cpu().numpy(), point)


def test_grow_strands_grows_around_the_head_only_with_avoid():
    scene = own(gc.head_scene())
    fld, mesh = gpu_field(scene["cloud"]), gc.head_mesh(scene["mesh_name"])
    plain, guarded = grow_pair(scene, fld, mesh, D, fused=True)
    assert guarded["path"].is_cuda and guarded["contacts"].dtype == torch.int32 and guarded["stop"].dtype == torch.uint8
    assert_the_head_is_avoided(scene, plain, guarded)
