"""The per-strand SH segment without a GPU: its C-ABI surface and refusals (a refused call launches nothing, so host pointers
do), the model option on the CPU, and the compiled resources of its three kernels."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from gaussianhaircut_amd import _lib
from tests import helpers as hp
from tests import shared_feature_cases as sc

NEW = ("ghr_model_forward_segment_shared", "ghr_model_backward_segment_shared", "ghr_shared_sh_fold")


def test_new_symbols_are_declared_bound_and_exported_without_an_abi_bump():
    hdr = open(os.path.join(hp.ROOT, "include", "ghr.h")).read()
    L = _lib.lib()
    for n in NEW:
        assert re.search(r"\bint %s\(" % n, hdr) and n in _lib.EXPORTS and hasattr(L, n), n
    assert "typedef struct ghr_shared_features" in hdr
    assert int(L.ghr_abi_version()) == _lib.ABI_VERSION
    assert int(re.search(r"#define GHR_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION
    from tests.test_shared_features_cpu import _build
    sim = ctypes.CDLL(_build())
    assert ctypes.sizeof(_lib.SharedFeatures) == int(sim.ghrsim_shared_sizeof()) == 8


def _valid(S=3, n_seg=4, K=16):
    """a complete argument set on HOST memory (never launched: every call below is refused, or has P == 0)"""
    sce = sc.make_scene(S, n_seg, K, 0)
    keep = {k: hp.np32(sce[k]) for k in ("xyz", "scaling", "rotation", "dir", "conf", "f_dc", "f_rest", "view", "proj", "campos")}
    keep["bg"] = np.zeros(10, np.float32)
    p = lambda k: keep[k].ctypes.data  # noqa: E731
    m = _lib.ModelArgs()
    m.P, m.W, m.H, m.sh_degree, m.sh_coeffs = sce["P"], 64, 64, sce["sh_degree"], K
    m.xyz, m.log_scales, m.rotations, m.orient_conf_log, m.dir3d = p("xyz"), p("scaling"), p("rotation"), p("conf"), p("dir")
    m.features_dc, m.features_rest = p("f_dc"), p("f_rest")
    m.viewmatrix, m.projmatrix, m.campos, m.background = p("view"), p("proj"), p("campos"), p("bg")
    m.scale_modifier, m.tan_fovx, m.tan_fovy, m.conic_eps = 1.0, sce["tanfovx"], sce["tanfovy"], 1e-7
    m.mode, m.row0 = 1, 0
    m.const_opacity, m.const_label, m.const_conf = 1.0, 1.0, 0.0
    sf = _lib.SharedFeatures()
    sf.n_strands, sf.rows_per_strand = S, n_seg
    return m, sf, keep


def _calls(m, sf, d_rgb_ws=True, d_fdc=True, d_frest=True):
    L = _lib.lib()
    buf = np.zeros(64, np.float32)
    b = ctypes.c_void_p(buf.ctypes.data)
    fwd = L.ghr_model_forward_segment_shared(None, ctypes.byref(m), ctypes.byref(sf) if sf is not None else None, m.P, 0, b, b,
                                             b, b)
    msg_f = L.ghr_last_error().decode()
    bwd = L.ghr_model_backward_segment_shared(None, ctypes.byref(m), ctypes.byref(sf) if sf is not None else None, m.P, b, b, b,
                                              b, b, b, b, None, None, b, b if d_fdc else None, b if d_frest else None, b, None, 1,
                                              b, 1, b if d_rgb_ws else None)
    msg_b = L.ghr_last_error().decode()
    return (fwd, msg_f), (bwd, msg_b)


@pytest.mark.parametrize("what,field", [
    ("mode", "mode"), ("P", "n_strands * rows_per_strand"), ("n_seg0", "rows_per_strand"), ("n_seg_neg", "rows_per_strand"),
    ("adam_fuse", "adam_fuse"), ("cam_only", "cam_only"), ("d_rgb", "d_rgb"), ("sh_coeffs", "sh_coeffs"), ("sf", "ghr_shared_features")])
def test_both_calls_refuse_the_argument_set_and_name_the_field(what, field):
    m, sf, keep = _valid()
    dummy = keep["xyz"].ctypes.data
    if what == "mode":
        m.mode = 0
        m.opacity_logit = m.label_logit = dummy
    elif what == "P":
        m.P += 1
    elif what == "n_seg0":
        sf.rows_per_strand = 0
    elif what == "n_seg_neg":
        sf.rows_per_strand, sf.n_strands = -4, -3       # (the product would match P)
    elif what == "adam_fuse":
        m.adam_fuse = dummy
    elif what == "cam_only":
        m.cam_only, m.cam_partial, m.cam_slots = 1, dummy, 8
    elif what == "d_rgb":
        m.d_rgb = dummy
    elif what == "sh_coeffs":
        m.sh_coeffs, m.sh_degree = 10, 2
    elif what == "sf":
        sf = None
    for rc, msg in _calls(m, sf):
        assert rc == _lib.GHR_E_INVALID and field in msg and "_segment_shared" in msg, (rc, msg)


@pytest.mark.parametrize("kw,field", [(dict(d_rgb_ws=False), "d_rgb_ws"), (dict(d_fdc=False), "d_features_dc"),
                                      (dict(d_frest=False), "d_features_rest")])
def test_backward_refuses_missing_outputs(kw, field):
    m, sf, keep = _valid()
    (_, _), (rc, msg) = _calls(m, sf, **kw)
    assert rc == _lib.GHR_E_INVALID and field in msg, (rc, msg)


def test_an_empty_segment_is_ok_and_launches_nothing():
    m, sf, keep = _valid()
    m.P, sf.n_strands = 0, 0
    L = _lib.lib()
    b = ctypes.c_void_p(keep["xyz"].ctypes.data)
    # (`first` = 1 and host pointers: a counter reset or any launch would fail here without a GPU and fault with one)
    assert L.ghr_model_forward_segment_shared(None, ctypes.byref(m), ctypes.byref(sf), 0, 1, b, b, b, b) == _lib.GHR_OK
    assert L.ghr_model_backward_segment_shared(None, ctypes.byref(m), ctypes.byref(sf), 0, b, b, b, b, b, b, b, None, None, b,
                                               None, None, b, None, 1, b, 1, None) == _lib.GHR_OK


def test_the_fold_on_its_own_checks_its_arguments():
    L = _lib.lib()
    buf = np.zeros(64, np.float32)
    b = ctypes.c_void_p(buf.ctypes.data)
    sf = _lib.SharedFeatures()
    sf.n_strands, sf.rows_per_strand = 2, 3

    def call(sf_, deg=3, K=16, xyz=b, rest=b):
        rc = L.ghr_shared_sh_fold(None, ctypes.byref(sf_) if sf_ is not None else None, deg, K, xyz, b, b, b, rest, None)
        return rc, L.ghr_last_error().decode()
    for kw, field in ((dict(sf_=None), "ghr_shared_features"), (dict(sf_=sf, K=5), "sh_coeffs"), (dict(sf_=sf, deg=3, K=9), "sh_degree"),
                      (dict(sf_=sf, xyz=None), "NULL"), (dict(sf_=sf, rest=None), "NULL")):
        rc, msg = call(**kw)
        assert rc == _lib.GHR_E_INVALID and field in msg and "ghr_shared_sh_fold" in msg, (kw, rc, msg)
    sf.rows_per_strand = 0
    rc, msg = call(sf)
    assert rc == _lib.GHR_E_INVALID and "rows_per_strand" in msg
    sf.n_strands, sf.rows_per_strand = 0, 3
    assert call(sf, xyz=None)[0] == _lib.GHR_OK        # nothing to fold, nothing launched


# ------------------------------------------------------------------------------------------------------------------ the model
class _Gen:
    def __init__(self, pts, feats, conf):
        self.pts, self.feats, self.conf = pts, feats, conf

    def __call__(self, iteration):
        return {"points": self.pts, "features": self.feats, "orient_conf": self.conf}


def test_the_option_changes_nothing_on_the_cpu_and_get_features_expands():
    from gaussianhaircut_amd.scene.gaussian_model_latent_strands import GaussianModelLatentStrands
    g = torch.Generator().manual_seed(3)
    S, L, K = 6, 5, 16
    gen = _Gen(torch.randn(S, L, 3, generator=g), torch.randn(S, 3 * K, generator=g), torch.randn(S, 1, generator=g))
    a = GaussianModelLatentStrands(3, gen)
    b = GaussianModelLatentStrands(3, gen, shared_appearance=True)
    assert a.shared_appearance is False and b.shared_appearance is True
    a.initialize_gaussians_hair(0)
    b.initialize_gaussians_hair(0)
    assert b.feature_rows_per_strand == 0                 # a CPU tensor: today's expanded rows
    for n in ("_xyz", "_rotation", "_scaling", "_dir", "_features_dc", "_features_rest", "_orient_conf"):
        assert torch.equal(getattr(a, n), getattr(b, n)), n
    assert torch.equal(a.get_features, b.get_features) and a.get_features.shape == (S * (L - 1), K, 3)
    # per-strand storage (what _split keeps on a ROCm device): get_features is the `repeat` form
    f = gen.feats.reshape(S, K, 3)
    b._features_dc, b._features_rest, b.feature_rows_per_strand = f[:, :1], f[:, 1:], L - 1
    assert torch.equal(b.get_features, f.view(S, 1, K, 3).repeat(1, L - 1, 1, 1).view(-1, K, 3))
    assert torch.equal(b.get_features, a.get_features)
    from gaussianhaircut_amd.gaussian_renderer.fused import hair_feature_rows
    assert hair_feature_rows(a) == 1 and hair_feature_rows(b) == L - 1
    b.feature_rows_per_strand = 0                          # per-strand shapes WITHOUT the attribute are refused
    with pytest.raises(ValueError, match="feature_rows_per_strand"):
        hair_feature_rows(b)
    b.feature_rows_per_strand = 3                          # ... and with one that does not match
    with pytest.raises(ValueError, match="feature_rows_per_strand"):
        hair_feature_rows(b)


def test_the_environment_knob_is_off_by_default_and_turns_the_option_on(monkeypatch):
    from gaussianhaircut_amd.scene import gaussian_model_latent_strands as gml
    assert gml.SHARED_FEATURES == (os.environ.get("GHR_LATENT_SHARED_FEATURES", "0") == "1")   # read at import, like FUSED_LATENT_BUILD
    monkeypatch.setattr(gml, "SHARED_FEATURES", False)
    assert gml.GaussianModelLatentStrands(3).shared_appearance is False
    monkeypatch.setattr(gml, "SHARED_FEATURES", True)
    assert gml.GaussianModelLatentStrands(3).shared_appearance is True


# -------------------------------------------------------------------------------------------------------------- kernel resources
def test_the_three_kernels_compile_without_scratch_and_within_their_budgets():
    """Budgets from the occupancy each kernel is planned for (512 VGPRs and 160 KiB of LDS per SIMD / CU):
      k_shared_proj_fwd  k_project's: 256 threads, the 45 KiB coefficient / record staging area -> three workgroups per CU (<= 53 KiB
                         each), twelve waves per CU = three per SIMD, which 128 VGPRs allow with one to spare;
      k_shared_proj_bwd  k_project_bwd's: one wave per workgroup, 11.25 KiB of LDS, three waves per SIMD (168 VGPRs);
      k_shared_sh_fold   one wave per strand, 64 x 17 basis values + 64 x 3 factors = 5 KiB; latency-bound on the in-order walk, so
                         it wants every wave slot: eight per SIMD (64 VGPRs), 32 per CU (<= 5 KiB each)."""
    from tests.test_kernel_resources import _descriptors
    meta = _descriptors()
    budgets = {"k_shared_proj_fwd": (2, 128, 53 * 1024), "k_shared_proj_bwd": (2, 168, 11520), "k_shared_sh_fold": (1, 64, 5120)}
    for sub, (count, vgprs, lds) in budgets.items():
        ks = [v for k, v in meta.items() if sub in k]
        assert len(ks) == count, (sub, [k for k in meta if sub in k])
        for k in ks:
            assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (sub, k)
            assert k["vgpr_count"] <= vgprs and k["group_segment_fixed_size"] <= lds, (sub, k)
    # the substrings the existing resource tests count by stay unambiguous
    for sub in ("k_project_bwd", "k_strand_build", "k_sh_grad_from_views", "k_render_fwd", "k_render_bwd_cells", "k_loss_fwd_cached_v",
                "k_loss_bwd_v", "k_adam_v4"):
        assert not [k for k in meta if "k_shared" in k and sub in k], sub
