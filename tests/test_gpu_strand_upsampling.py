"""Groom upsampling on the GPU (csrc/ghr_upsample.h through the C ABI and gaussianhaircut_amd/strand_upsampling.py).

 1. Through the C ABI on every case of tests/upsample_cases.py (G = 257, N = 257, L = 66, F = 3 among them): nbr, nd2, out, w, of and
    valid equal the host walk (tests/hostsim/ghr_hostsim_upsample.cpp) bit for bit; a second pass gives the same bits; every output
    lies NaN-filled between guard words: every element written, nothing beyond.  Only tables with every entry -1 or inside [0, G)
    go to the device.
 2. Through strand_upsampling.py: fused=True and fused=False on device tensors, each against the float64 arbiter under the derived
    bound of upsample_cases.py, and so against each other under twice it; nbr, valid and keep equal exactly.
 3. frames_at and the pruning by a head mesh through the HIP closest-point and containment kernels, against the composed forms."""
import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from tests import upsample_cases as uc
from tests import upsample_sim

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = uc.cases()
IDS = [c["name"] for c in CASES]
GUARD = 64  # words (bytes for valid) in front of and behind every output


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def sim():
    return upsample_sim.load()


def _guarded(words, dtype):
    """[GUARD | words | GUARD] on the device: the guards a pattern, the body NaN (float) / 0x7fc00000 (int32)"""
    buf = torch.full((words + 2 * GUARD,), 0x7fc00000, dtype=torch.int32, device=DEV)
    buf[:GUARD] = 0x5a5a5a5a
    buf[GUARD + words:] = 0x5a5a5a5a
    return buf, buf[GUARD:GUARD + words].view(dtype)


def _intact(buf, words):
    g = buf.cpu().numpy()
    body = g[GUARD:GUARD + words]
    return bool((g[:GUARD] == 0x5a5a5a5a).all() and (g[GUARD + words:] == 0x5a5a5a5a).all() and (body != 0x7fc00000).all())


def _guarded_bytes(count):
    buf = torch.full((count + 2 * GUARD,), 0xEE, dtype=torch.uint8, device=DEV)
    buf[:GUARD] = 0x5A
    buf[GUARD + count:] = 0x5A
    return buf, buf[GUARD:GUARD + count]


def _intact_bytes(buf, count):
    g = buf.cpu().numpy()
    return bool((g[:GUARD] == 0x5A).all() and (g[GUARD + count:] == 0x5A).all() and (g[GUARD:GUARD + count] != 0xEE).all())


def _ptr(t):
    return None if t is None else t.data_ptr()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_c_abi_equals_the_host_walk_bit_for_bit(sim, index):
    c = CASES[index]
    L = _lib.lib()
    G, Lp = c["gp"].shape[:2]
    N = c["co"].shape[0]
    F = 0 if c["gf"] is None else c["gf"].shape[1]
    stream = torch.cuda.current_stream().cuda_stream
    roots = np.ascontiguousarray(c["gp"][:, 0])
    r2 = float(uc.r2_of(c["radius"]))
    want_nbr, want_nd2 = upsample_sim.near(sim, roots, c["co"], r2)
    roots_d, co, cM, gp, gM, gf = (_dev(x) for x in (roots, c["co"], c["cM"], c["gp"], c["gM"], c["gf"]))
    for _ in range(2):
        nb, nbr = _guarded(4 * N, torch.int32)
        db, nd2 = _guarded(4 * N, torch.float32)
        _lib.check(L.ghr_upsample_neighbours(stream, G, _ptr(roots_d), N, _ptr(co), r2, _ptr(nbr), _ptr(nd2)))
        torch.cuda.synchronize()
        assert _intact(nb, 4 * N) and _intact(db, 4 * N)
        assert np.array_equal(nbr.cpu().numpy().reshape(N, 4), want_nbr), c["name"]
        assert np.array_equal(_bits(nd2).reshape(N, 4), _bits(want_nd2)), c["name"]
    assert ((want_nbr == -1) | ((want_nbr >= 0) & (want_nbr < G))).all()      # only such tables go to the device
    want = upsample_sim.blend(sim, c["gp"], c["gM"], c["gf"], c["co"], c["cM"], want_nbr, want_nd2, c["eps2"], c["tau"])
    nbr_d, nd2_d = _dev(want_nbr), _dev(want_nd2)
    tau, gate = (0.0, 0) if c["tau"] is None else (float(np.float32(c["tau"])), 1)
    for _ in range(2):
        ob, out = _guarded(3 * N * Lp, torch.float32)
        wb, w = _guarded(4 * N, torch.float32)
        fb, of = _guarded(N * F, torch.float32) if F else (None, None)
        vb, valid = _guarded_bytes(N)
        _lib.check(L.ghr_upsample_blend(stream, G, Lp, _ptr(gp), _ptr(gM), _ptr(gf), F, N, _ptr(co), _ptr(cM), _ptr(nbr_d), _ptr(nd2_d),
                                        c["eps2"], tau, gate, _ptr(out), _ptr(w), _ptr(of), _ptr(valid)))
        torch.cuda.synchronize()
        assert _intact(ob, 3 * N * Lp) and _intact(wb, 4 * N) and _intact_bytes(vb, N) and (not F or _intact(fb, N * F))
        assert np.array_equal(_bits(out), _bits(want["points"]).reshape(-1)), c["name"]
        assert np.array_equal(_bits(w), _bits(want["weights"]).reshape(-1)), c["name"]
        assert np.array_equal(valid.cpu().numpy(), want["valid"]), c["name"]
        if F:
            assert np.array_equal(_bits(of), _bits(want["features"]).reshape(-1)), c["name"]


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_fused_and_composed_agree_under_the_bound_on_device_tensors(index):
    from gaussianhaircut_amd import strand_upsampling as su
    c = CASES[index]
    ref = uc.arbiter_of(index)
    nbr, _ = uc.neighbours_of(index)
    got = {}
    for fused in (True, False):
        out = su.upsample_strands(_dev(c["gp"]), _dev(c["gM"]), _dev(c["co"]), _dev(c["cM"]), features=_dev(c["gf"]), radius=c["radius"],
                                  eps2=c["eps2"], tau=c["tau"], fused=fused)
        assert out["points"].device.type == "cuda" and out["eps2"] == c["eps2"]
        got[fused] = {k: v.cpu().numpy() for k, v in out.items() if isinstance(v, torch.Tensor)}
        ratio = uc.excess(got[fused], ref)
        print(c["name"], "fused" if fused else "composed", "largest error / bound %.4f" % ratio)
        assert ratio <= 1.0, (c["name"], fused, ratio)
        assert np.array_equal(got[fused]["nbr"], nbr) and np.array_equal(got[fused]["valid"], ref["valid"])
        assert np.array_equal(got[fused]["keep"], ref["valid"])
        assert np.array_equal(_bits(got[fused]["points"][:, 0]), _bits(c["co"]))
    for key, b in (("points", "b_points"), ("weights", "b_weights"), ("features", "b_features")):
        assert (np.abs(got[True][key].astype(np.float64) - got[False][key]) <= 2 * ref[b]).all(), (c["name"], key)
    # the default on a device tensor is the fused form: the same bits
    c0 = su.upsample_strands(_dev(c["gp"]), _dev(c["gM"]), _dev(c["co"]), _dev(c["cM"]), features=_dev(c["gf"]), radius=c["radius"],
                             eps2=c["eps2"], tau=c["tau"])
    assert np.array_equal(_bits(c0["points"]), _bits(got[True]["points"]))


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def test_frames_at_and_the_pruning_run_through_the_hip_mesh_kernels():
    from gaussianhaircut_amd import strand_generator as sgen
    from gaussianhaircut_amd import strand_upsampling as su
    from gaussianhaircut_amd.mesh import HeadMesh
    from tests import mesh_cases as mc
    from tests.test_strand_upsampling_cpu import _small_groom, _uv_scalp
    v, f, uv, frames, scalp = _uv_scalp()
    guides = torch.from_numpy(_small_groom())
    gM_cpu = su.frames_at(scalp, frames, guides[:, 0], fused=False)
    gM = su.frames_at(scalp, frames, guides[:, 0].to(DEV))                   # fused by default on a device tensor
    assert gM.device.type == "cuda" and torch.equal(gM.cpu(), gM_cpu)
    roots = sgen.sample_roots(torch.from_numpy(v), torch.from_numpy(f.astype(np.int64)), torch.from_numpy(uv), 300,
                              generator=torch.Generator().manual_seed(2))
    head = HeadMesh(*mc.uv_sphere(24, 10, radius=0.98))
    rgb = torch.rand(12, 3, generator=torch.Generator().manual_seed(1))
    dev = su.upsample_strands(guides.to(DEV), gM, roots["origins"].to(DEV), roots["local2world"].to(DEV), features=rgb.to(DEV), radius=1.0,
                              mesh=head)
    cpu = su.upsample_strands(guides, gM_cpu, roots["origins"], roots["local2world"], features=rgb, radius=1.0, mesh=head)
    assert torch.equal(dev["nbr"].cpu(), cpu["nbr"]) and torch.equal(dev["valid"].cpu(), cpu["valid"])
    assert 0 < int(dev["keep"].sum()) <= int(dev["valid"].sum()) < 300 and not bool((dev["keep"] & ~dev["valid"]).any())
    # the two forms' points differ by roundings only, so a strand changes sides of the pruning rule only at a point on the head
    assert int((dev["keep"].cpu() != cpu["keep"]).sum()) <= 1
