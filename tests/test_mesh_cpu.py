"""Point-in-mesh containment (csrc/ghr_mesh.h, gaussianhaircut_amd/mesh.py) without a GPU.

Every result is a boolean or an integer: every comparison is exact.
 1. the numpy float32 MODEL of the definition (tests/mesh_cases.py) against a float64 winding-number truth on the closed case
    meshes, 20 000 random queries each: 0 disagreements per axis and for the majority, no query left out;
 2. the product's own grid builder and per-element functions compiled for the host (tests/hostsim/ghr_hostsim_mesh.cpp, every
    index checked) against the model, bit for bit, on every case -- tie lattice, box-edge points, points outside the box and
    non-finite queries included; the tables against their specification and against the library's own build;
 3. the same cases through a stand-alone program built with -fsanitize=address,undefined (nothing sanitized is loaded here);
 4. the PyTorch comparator (fused=False) on CPU tensors against the model; the refusals of the C ABI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from gaussianhaircut_amd.mesh import HeadMesh, ICO_VERTS, read_obj
from tests import helpers as hp
from tests import mesh_cases as mc

CASES = list(mc.meshes())
CLOSED = [n for n in CASES if mc.meshes()[n][3]]
DEPS = ["ghr_hostsim_mesh.cpp", "ghr_mesh.h"]


@pytest.fixture(scope="module")
def sim():
    L = ctypes.CDLL(hp.compile_hostsim("libghr_hostsim_mesh.so", "ghr_hostsim_mesh.cpp", ["-O2", "-fPIC", "-shared"], DEPS))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    L.ghrsim_mesh_sizes.argtypes = [i32, vp, i32, vp, i32, vp, vp]
    L.ghrsim_mesh_build.argtypes = [i32, vp, i32, vp, i32, vp, ctypes.c_ulonglong, vp]
    L.ghrsim_mesh_verify.argtypes = [vp, vp, vp]
    L.ghrsim_mesh_list_length.argtypes = [vp, i32, i32, i32]
    L.ghrsim_mesh_contains.argtypes = [vp, i64, vp, vp, vp]
    L.ghrsim_mesh_probe_points.argtypes = [i64, vp, vp, vp, i32, vp]
    L.ghrsim_mesh_probes_outside.argtypes = [vp, i64, vp, vp, vp, i32, vp]
    for n in ("ghrsim_mesh_sizes", "ghrsim_mesh_build", "ghrsim_mesh_verify", "ghrsim_mesh_list_length", "ghrsim_mesh_header_bytes"):
        getattr(L, n).restype = ctypes.c_int
    assert L.ghrsim_mesh_header_bytes() == ctypes.sizeof(_lib.MeshGrid)
    return L


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _sim_build(sim, v, f, G):
    h, why = _lib.MeshGrid(), ctypes.create_string_buffer(128)
    assert sim.ghrsim_mesh_sizes(len(v), _p(v), len(f), _p(f), G, ctypes.byref(h), why) == 0, why.value
    blob = np.zeros(int(h.bytes) // 16, dtype=[("a", "<u8"), ("b", "<u8")]).view(np.uint8)  # 16-B aligned
    assert blob.ctypes.data % 16 == 0
    assert sim.ghrsim_mesh_build(len(v), _p(v), len(f), _p(f), G, _p(blob), int(h.bytes), why) == 0, why.value
    return blob


@pytest.fixture(scope="module")
def blobs(sim):
    return {n: _sim_build(sim, *mc.meshes()[n][:3]) for n in CASES}


@pytest.fixture(scope="module")
def model():
    """name -> (inside, crossings) of the numpy model on the case's finite queries; computed once"""
    out = {}
    for n in CASES:
        v, f, _, _ = mc.meshes()[n]
        out[n] = mc.model_contains(v, f, mc.queries(n))
    return out


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CLOSED)
def test_model_agrees_with_the_winding_number_on_closed_meshes(name):
    v, f, _, _ = mc.meshes()[name]
    rng = np.random.default_rng(0)
    q = rng.uniform(-1.5, 1.5, (20000, 3))
    lo, hi = mc.mesh_box(v, f)
    if np.abs(np.concatenate([lo, hi])).max() > 1.5:  # the integer cube: the same cloud about its centre, 1.5 x its half extent
        q = (lo + hi) / 2 + q * (hi - lo).max() / 2
    q = q.astype(np.float32)
    truth = mc.winding_inside(v, f, q)
    inside, c = mc.model_contains(v, f, q)
    assert 0.01 * len(q) < truth.sum() < 0.9 * len(q)
    for a in range(3):
        assert int(((c[:, a] & 1).astype(bool) != truth).sum()) == 0, (name, a)
    assert int((inside != truth).sum()) == 0, name


def test_model_follows_the_half_open_rule_on_the_integer_cube():
    v, f, _, _ = mc.meshes()["cube"]
    lat = mc.cube_tie_lattice()
    for a in range(3):
        c = mc.model_crossings(v, f, lat[a])
        assert np.array_equal((c[:, a] & 1).astype(bool), mc.half_open_rule(lat[a], a)), a


def test_open_cylinder_is_decided_by_the_majority_not_by_one_ray():
    v, f, _, _ = mc.meshes()["cylinder"]
    q = np.array([[0.1, 0.2, 0.3], [-0.5, 0.3, -0.9], [0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [0.2, 0.1, 1.5]], np.float32)
    inside, c = mc.model_contains(v, f, q)
    assert inside.tolist() == [True, True, True, False, False]
    assert (c[:3, 2] == 0).all() and (c[:3, :2] & 1).all()  # the +z ray leaves through the opening: a single ray says outside


def test_single_triangle_and_flat_triangles_hold_nothing(model):
    assert not model["triangle"][0].any()
    v, f, _, _ = mc.meshes()["flat"]
    ref = mc.model_contains(v, f[:12], mc.queries("flat"))  # the closed box alone
    assert np.array_equal(model["flat"][0], ref[0]) and np.array_equal(model["flat"][1], ref[1])


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_grid_tables_meet_their_specification_and_are_the_librarys(sim, blobs, name):
    v, f, G, _ = mc.meshes()[name]
    blob = blobs[name]
    assert sim.ghrsim_mesh_verify(_p(v), _p(f), _p(blob)) == 0
    assert np.array_equal(blob, _sim_build(sim, v, f, G))          # deterministic
    mesh = HeadMesh(v, f, grid=G)                                   # the library's host builder: the same bytes
    assert np.array_equal(mesh.grid_blob(), blob)
    assert mesh.grid == (G or int(np.ceil(np.sqrt(len(f)))))
    for a, (mean, longest) in enumerate(mesh.grid_stats()):
        assert longest == max(sim.ghrsim_mesh_list_length(_p(blob), a, cu, cv) for cu in range(mesh.grid) for cv in range(mesh.grid))


@pytest.mark.parametrize("n", mc.STACK_SIZES)
def test_stack_puts_exactly_n_faces_into_one_cell(sim, blobs, n):
    blob = blobs["stack%d" % n]
    assert sim.ghrsim_mesh_list_length(_p(blob), 2, 3, 3) == n
    assert sim.ghrsim_mesh_list_length(_p(blob), 2, 0, 0) == 1 and sim.ghrsim_mesh_list_length(_p(blob), 2, 5, 2) == 0


def _sim_contains(sim, blob, q):
    q = np.ascontiguousarray(q, np.float32)
    inside, c = np.full(len(q), 7, np.uint8), np.full((len(q), 3), 0xFFFFFFFF, np.uint32)
    sim.ghrsim_mesh_contains(_p(blob), len(q), _p(q), _p(inside), _p(c))
    return inside, c


@pytest.mark.parametrize("name", CASES)
def test_host_sim_contains_equals_the_model_bit_for_bit(sim, blobs, model, name):
    q = mc.queries(name)
    assert len(q) >= 1000
    inside, c = _sim_contains(sim, blobs[name], q)
    assert np.array_equal(c, model[name][1])
    assert np.array_equal(inside, model[name][0].astype(np.uint8))


@pytest.mark.parametrize("name", CASES)
def test_host_sim_refuses_non_finite_and_far_queries(sim, blobs, name):
    q = mc.nonfinite_queries()
    inside, c = _sim_contains(sim, blobs[name], q)
    assert not inside.any() and not c.any()
    v, f, _, _ = mc.meshes()[name]
    assert not mc.model_contains(v, f, q)[0].any()


def test_host_sim_half_open_rule_on_the_cube(sim, blobs):
    lat = mc.cube_tie_lattice()
    for a in range(3):
        _, c = _sim_contains(sim, blobs["cube"], lat[a])
        assert np.array_equal((c[:, a] & 1).astype(bool), mc.half_open_rule(lat[a], a)), a


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["icosphere2", "cube", "cylinder", "stack65"])
def test_host_sim_probes_equal_the_model(sim, blobs, name, mode):
    v, f, _, _ = mc.meshes()[name]
    xyz, s, r = mc.gaussians(name, 300)
    pts = np.full((300, 12, 3), np.nan, np.float32)
    sim.ghrsim_mesh_probe_points(300, _p(xyz), _p(s), _p(r), mode, _p(pts))
    want = mc.model_probe_points(xyz, s, r, mode)
    assert np.array_equal(pts.view(np.uint32), want.view(np.uint32))
    out = np.full(300, 7, np.uint8)
    sim.ghrsim_mesh_probes_outside(_p(blobs[name]), 300, _p(xyz), _p(s), _p(r), mode, _p(out))
    want_out = mc.model_probes_outside(v, f, xyz, s, r, mode)
    assert np.array_equal(out, want_out.astype(np.uint8))
    if name in ("icosphere2", "cube"):
        assert 0 < want_out.sum() < 300


def test_probe_conventions(sim):
    """`reference` restates the script: v @ (diag(3 s) @ build_rotation(q)) + xyz with this package's build_rotation, which (as
    the reference's) returns the transposed rotation matrix -- the points R diag(3 s) v + xyz of the 3-sigma ellipsoid;
    `axis_scaled` is diag(3 s) R^T v + xyz.  Checked in float64 to the rounding of float32 (a batched matrix product fixes no
    summation order, so the script's own bits are not defined)."""
    from gaussianhaircut_amd.utils.general_utils import build_rotation, build_scaling_rotation
    xyz, s, r = mc.gaussians("icosphere2", 50)
    ico = torch.tensor(ICO_VERTS, dtype=torch.float64)
    assert np.array_equal(mc.ico_vertices(), np.asarray(ICO_VERTS, np.float32))
    M = build_scaling_rotation(torch.from_numpy(s).double() * 3, torch.from_numpy(r).double())
    script = (ico[None, :, None, :] @ M[:, None, :, :])[:, :, 0, :] + torch.from_numpy(xyz).double()[:, None]
    Rstd = build_rotation(torch.from_numpy(r).double()).transpose(1, 2)
    ell = torch.einsum("pji,pi,ki->pkj", Rstd, torch.from_numpy(s).double() * 3, ico) + torch.from_numpy(xyz).double()[:, None]
    axs = torch.einsum("pj,pij,ki->pkj", torch.from_numpy(s).double() * 3, Rstd, ico) + torch.from_numpy(xyz).double()[:, None]
    scale = float(np.abs(xyz).max() + 3 * s.max())
    got0, got1 = mc.model_probe_points(xyz, s, r, 0), mc.model_probe_points(xyz, s, r, 1)
    assert np.abs(got0 - script.numpy()).max() < 1e-5 * scale and np.abs(got0 - ell.numpy()).max() < 1e-5 * scale
    assert np.abs(got1 - axs.numpy()).max() < 1e-5 * scale
    assert np.abs(got0 - got1).max() > 1e-2 * s.max()   # the two conventions are different points
    for name in ("reference", "ellipsoid", "axis_scaled"):
        t = HeadMesh.probe_points(torch.from_numpy(xyz), torch.from_numpy(s), torch.from_numpy(r), name).numpy()
        assert np.array_equal(t.view(np.uint32), (got1 if name == "axis_scaled" else got0).view(np.uint32)), name


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def test_sanitized_stand_alone_program_runs_the_cases_clean(tmp_path, model):
    """ghr_mesh_selfcheck: the builder, the table check, contains and the probe function under AddressSanitizer and
    UndefinedBehaviorSanitizer, as a program of its own (exact-size buffers); the non-finite queries ride along."""
    san = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    if os.path.basename(hp.host_cxx()) == "g++":
        san += ["-static-libasan", "-static-libubsan"]
    exe = hp.compile_hostsim("ghr_mesh_selfcheck_san", "ghr_mesh_selfcheck.cpp", san, DEPS)
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as fh:
        for name in CASES:
            v, f, G, _ = mc.meshes()[name]
            q = np.concatenate([mc.queries(name), mc.nonfinite_queries()])
            inside = np.concatenate([model[name][0], np.zeros(len(mc.nonfinite_queries()), bool)]).astype(np.uint8)
            c = np.concatenate([model[name][1], np.zeros((len(mc.nonfinite_queries()), 3), np.uint32)])
            P = 64
            xyz, s, r = mc.gaussians(name, P)
            outs = [mc.model_probes_outside(v, f, xyz, s, r, m).astype(np.uint8) for m in (0, 1)]
            fh.write(np.array([len(v), len(f), G, len(q), P], np.int32).tobytes())
            for arr in (v, f, q, inside, c, xyz, s, r, outs[0], outs[1]):
                fh.write(np.ascontiguousarray(arr).tobytes())
    res = subprocess.run([exe, path], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "%d cases ok" % len(CASES) in res.stdout and "runtime error" not in res.stderr, res.stdout + res.stderr


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_torch_comparator_equals_the_model_on_cpu_tensors(model, name):
    v, f, G, _ = mc.meshes()[name]
    mesh = HeadMesh(v, f, grid=G)
    q = np.concatenate([mc.queries(name), mc.nonfinite_queries()])
    inside, c = mesh.contains(torch.from_numpy(q), fused=False, return_crossings=True)
    n = len(mc.queries(name))
    assert np.array_equal(c.numpy()[:n].astype(np.uint32), model[name][1]) and np.array_equal(inside.numpy()[:n], model[name][0])
    assert not inside.numpy()[n:].any() and not c.numpy()[n:].any()
    # chunking does not enter, shapes are kept
    i2 = mesh.contains(torch.from_numpy(q[:90]).reshape(9, 10, 3), fused=False)
    assert i2.shape == (9, 10) and np.array_equal(i2.reshape(-1).numpy(), inside.numpy()[:90])
    i3, _ = mesh._contains_torch(torch.from_numpy(q[:90]), chunk_elems=7)
    assert np.array_equal(i3.numpy(), inside.numpy()[:90])


def test_torch_probe_filter_equals_the_model_on_cpu_tensors():
    v, f, _, _ = mc.meshes()["icosphere2"]
    mesh = HeadMesh(v, f)
    xyz, s, r = mc.gaussians("icosphere2", 200)
    for name, mode in (("reference", 0), ("ellipsoid", 0), ("axis_scaled", 1)):
        got = mesh.probes_outside(torch.from_numpy(xyz), torch.from_numpy(s), torch.from_numpy(r), probe=name, fused=False)
        assert np.array_equal(got.numpy(), mc.model_probes_outside(v, f, xyz, s, r, mode)), name
    with pytest.raises(ValueError, match="probe must be one of"):
        mesh.probes_outside(torch.from_numpy(xyz), torch.from_numpy(s), torch.from_numpy(r), probe="sphere", fused=False)


def test_fused_forms_refuse_cpu_tensors():
    v, f, _, _ = mc.meshes()["cube"]
    mesh = HeadMesh(v, f)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.contains(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.probes_outside(torch.zeros(4, 3), torch.ones(4, 3), torch.ones(4, 4))


def test_c_abi_refusals_launch_nothing():
    L = _lib.lib()
    v, f, _, _ = mc.meshes()["cube"]
    h = _lib.MeshGrid()
    bad_f = f.copy(); bad_f[3, 1] = 8
    assert L.ghr_mesh_grid_sizes(8, _p(v), 12, _p(bad_f), 0, ctypes.byref(h)) == _lib.GHR_E_INVALID
    assert b"face index" in L.ghr_last_error()
    bad_v = v.copy(); bad_v[2, 1] = np.inf
    assert L.ghr_mesh_grid_sizes(8, _p(bad_v), 12, _p(f), 0, ctypes.byref(h)) == _lib.GHR_E_INVALID
    assert b"not finite" in L.ghr_last_error()
    assert L.ghr_mesh_grid_sizes(8, _p(v), 12, _p(f), 257, ctypes.byref(h)) == _lib.GHR_E_INVALID
    assert L.ghr_mesh_grid_sizes(8, _p(v), 12, _p(f), 0, ctypes.byref(h)) == _lib.GHR_OK and h.G == 4 and h.bytes > 0
    blob = np.zeros(int(h.bytes) // 8, np.uint64)
    assert L.ghr_mesh_grid_build(8, _p(v), 12, _p(f), 0, _p(blob), int(h.bytes) - 16) == _lib.GHR_E_INVALID
    assert b"bytes" in L.ghr_last_error()
    fake = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before a launch
    assert L.ghr_mesh_contains(None, None, fake, 4, fake, fake, None) == _lib.GHR_E_INVALID
    assert L.ghr_mesh_contains(None, ctypes.byref(h), None, 4, fake, fake, None) == _lib.GHR_E_INVALID
    assert L.ghr_mesh_contains(None, ctypes.byref(h), fake, -1, fake, fake, None) == _lib.GHR_E_INVALID
    assert L.ghr_mesh_contains(None, ctypes.byref(h), fake, 4, None, fake, None) == _lib.GHR_E_INVALID
    assert L.ghr_gaussian_probe_outside(None, ctypes.byref(h), fake, 4, fake, fake, fake, 2, fake) == _lib.GHR_E_INVALID
    assert b"probe" in L.ghr_last_error()
    assert L.ghr_gaussian_probe_outside(None, ctypes.byref(h), fake, 4, fake, None, fake, 0, fake) == _lib.GHR_E_INVALID
    broken = _lib.MeshGrid.from_buffer_copy(bytes(h)); broken.magic = 0
    assert L.ghr_mesh_contains(None, ctypes.byref(broken), fake, 4, fake, fake, None) == _lib.GHR_E_INVALID
    broken = _lib.MeshGrid.from_buffer_copy(bytes(h)); broken.off_list[2] = h.bytes
    broken.list_total[2] = 4
    assert L.ghr_mesh_contains(None, ctypes.byref(broken), fake, 4, fake, fake, None) == _lib.GHR_E_INVALID
    assert L.ghr_mesh_contains(None, ctypes.byref(h), fake, 0, None, None, None) == _lib.GHR_OK


def test_read_obj_fans_polygons_and_takes_the_vertex_index(tmp_path):
    p = tmp_path / "m.obj"
    p.write_text("# a quad, a pentagon, a triangle\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvn 0 0 1\nv 0.5 1.5 0.25\n"
                 "f 1/1/1 2/1/1 3/1/1 4/1/1\nf 1//1 2//1 3//1 5//1 4//1\nf -1 1/1 2\n\ng ignored\n")
    v, f = read_obj(str(p))
    assert v.dtype == np.float32 and v.shape == (5, 3) and v[4].tolist() == [0.5, 1.5, 0.25]
    assert f.dtype == np.int32 and f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 4], [0, 4, 3], [4, 0, 1]]
