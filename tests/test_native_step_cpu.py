"""ghr_view_step (include/ghr.h) as far as a host without a GPU can tell: the export, the struct layout the ctypes binding
assumes, and the refusals -- every one of them decided from the arguments before anything is launched."""
import ctypes
import os
import subprocess

import pytest

from gaussianhaircut_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = 0x1000  # stands for a buffer: a refused call touches none


def _filled():
    """A struct that passes every check of the call (P = 257 Gaussians, 33 x 17 pixels, K = 16)."""
    a = _lib.ViewStepArgs()
    m = a.model
    m.P, m.W, m.H, m.sh_degree, m.sh_coeffs = 257, 33, 17, 3, 16
    for n in ("xyz", "log_scales", "rotations", "opacity_logit", "label_logit", "orient_conf_log", "features_dc", "features_rest",
              "viewmatrix", "projmatrix", "campos", "background"):
        setattr(m, n, X)
    m.scale_modifier, m.tan_fovx, m.tan_fovy, m.conic_eps = 1.0, 0.5, 0.5, 1e-12
    a.R = 4096
    for n in ("R_host", "geom_ws", "img_ws", "bin_ws", "radii", "means2D_out", "render", "maps", "sums", "loss_out", "grad_loss",
              "d_pix", "grad_scratch", "d_means2D", "d_xyz", "d_log_scales", "d_rotations", "d_opacity_logit", "d_label_logit",
              "d_orient_conf_log", "d_features_dc", "d_features_rest", "nan_flag"):
        setattr(a, n, X)
    l = a.loss
    l.W, l.H = 33, 17
    l.gt_image = l.gt_mask = l.gt_orient_angle = l.gt_orient_conf = X
    l.w_l1, l.w_ssim, l.w_mask, l.w_orient = 0.8, 0.2, 0.1, 0.1
    a.prezero, a.accumulate = 1, 0
    return a


def _refused(a):
    L = _lib.lib()
    rc = L.ghr_view_step(None, ctypes.byref(a))
    return rc, L.ghr_last_error().decode()


def test_library_exports_the_view_step():
    L = _lib.lib()
    assert "ghr_view_step" in _lib.EXPORTS and hasattr(L, "ghr_view_step")
    # (an added function with no existing struct or signature changed: the header's rule for such additions keeps the ABI number)
    assert int(L.ghr_abi_version()) == _lib.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "ghr.h")).read()
    assert "#define GHR_ABI_VERSION %d\n" % _lib.ABI_VERSION in hdr and "int ghr_view_step(void* stream, const ghr_view_step_args* v);" in hdr
    assert "ghr_strands.h" in _lib.HEADERS  # (a header edit marks the library stale: every header it includes is listed)
    csrc = os.path.join(ROOT, "gaussianhaircut_amd", "csrc")
    assert sorted(f for f in os.listdir(csrc) if f.endswith(".h")) == sorted(_lib.HEADERS)


def test_a_null_struct_is_refused():
    L = _lib.lib()
    assert L.ghr_view_step(None, None) == _lib.GHR_E_INVALID
    assert b"ghr_view_step" in L.ghr_last_error()


@pytest.mark.parametrize("field", ["geom_ws", "img_ws", "bin_ws", "grad_scratch", "R_host", "radii", "render", "maps", "sums",
                                   "loss_out", "d_pix", "d_means2D", "d_xyz", "d_orient_conf_log"])
def test_a_null_buffer_is_refused_by_name(field):
    a = _filled()
    setattr(a, field, None)
    rc, msg = _refused(a)
    assert rc == _lib.GHR_E_INVALID and msg.startswith("ghr_view_step: ") and (field + " is NULL") in msg, msg


@pytest.mark.parametrize("field", ["xyz", "features_rest", "campos", "background"])
def test_a_null_model_pointer_is_refused_by_name(field):
    a = _filled()
    setattr(a.model, field, None)
    rc, msg = _refused(a)
    assert rc == _lib.GHR_E_INVALID and ("model.%s is NULL" % field) in msg, msg


def test_the_binning_workspace_may_be_null_only_at_capacity_zero():
    a = _filled()
    a.bin_ws = None
    assert _refused(a)[0] == _lib.GHR_E_INVALID
    a.R = 0
    a.grad_scratch = None
    a.loss.W = 34  # (the struct is otherwise fine: it is refused for the NEXT reason, not for bin_ws)
    rc, msg = _refused(a)
    assert rc == _lib.GHR_E_INVALID and "bin_ws" not in msg and "loss.W" in msg, msg


@pytest.mark.parametrize("dW,dH", [(1, 0), (0, 1), (-1, 0)])
def test_loss_and_model_must_agree_on_the_image_size(dW, dH):
    a = _filled()
    a.loss.W += dW
    a.loss.H += dH
    rc, msg = _refused(a)
    assert rc == _lib.GHR_E_INVALID and "loss.W / loss.H differ from model.W / model.H" in msg, msg


def _adam_fuse(flag=X):
    f = _lib.AdamFuse()
    f.n = 257 * 61
    for n in ("p_in", "m_in", "v_in", "p_out", "m_out", "v_out", "state", "flag_next"):
        setattr(f, n, X)
    f.flag = flag
    f.n_groups = 8
    ends = (ctypes.c_int64 * 8)(*[257 * e for e in (3, 6, 10, 11, 12, 13, 16, 61)])
    lrs = (ctypes.c_float * 8)(*([1e-3] * 8))
    f.group_end_host, f.lr_host = ctypes.cast(ends, ctypes.c_void_p), ctypes.cast(lrs, ctypes.c_void_p)
    f._keep = (ends, lrs)
    return f


def test_adam_fuse_with_accumulate_needs_the_gradient_buffers_it_adds_from():
    """ghr_adam_fuse: the view that carries the update adds what the earlier views accumulated (accumulate != 0) from the SH
    gradient buffers -- NULL there is only allowed for the step's single view (accumulate == 0)."""
    f = _adam_fuse()
    a = _filled()
    a.model.adam_fuse = ctypes.addressof(f)
    a.model.dens_img_ws, a.model.overflow_raises_flag = a.img_ws, 1
    a.accumulate = 1
    a.d_features_dc = None
    rc, msg = _refused(a)
    assert rc == _lib.GHR_E_INVALID and "d_features_dc" in msg and "adam_fuse" in msg and "accumulate" in msg, msg
    a.d_features_dc, a.d_features_rest = X, None
    rc, msg = _refused(a)
    assert rc == _lib.GHR_E_INVALID and "d_features_rest" in msg and "accumulate" in msg, msg


def test_adam_fuse_contract_is_checked_before_any_launch():
    f = _adam_fuse()
    a = _filled()
    a.model.adam_fuse = ctypes.addressof(f)
    a.model.dens_img_ws, a.model.overflow_raises_flag = a.img_ws, 1
    a.model.d_rgb = X  # the updating view stores no dL/d(rgb) table
    rc, msg = _refused(a)
    assert rc == _lib.GHR_E_INVALID and "model.d_rgb with model.adam_fuse" in msg, msg
    a.model.d_rgb = None
    a.model.dens_img_ws, a.model.overflow_raises_flag = None, 0  # an overflowed view could reach the parameters
    rc, msg = _refused(a)
    assert rc == _lib.GHR_E_INVALID and "model.adam_fuse needs model.dens_img_ws" in msg, msg
    a.model.dens_img_ws, a.model.overflow_raises_flag = a.img_ws, 1
    a.nan_flag = X + 4  # every view of the step raises the step's own word
    rc, msg = _refused(a)
    assert rc == _lib.GHR_E_INVALID and "nan_flag" in msg and "adam_fuse->flag" in msg, msg
    f.group_end_host = None  # (a.nan_flag right again: without a group table the struct is refused as a whole)
    a.nan_flag = X
    rc, msg = _refused(a)
    assert rc == _lib.GHR_E_INVALID and "ghr_adam_fuse" in msg, msg


def test_what_the_call_does_not_cover_is_refused():
    for field, value, word in (("mode", 1, "model.mode"), ("row0", 256, "model.row0"), ("debug", 1, "model.debug"),
                               ("cam_partial", X, "model.cam_partial"), ("fovx_dev", X, "model.fovx_dev"),
                               ("P", 0, "model.P"), ("sh_coeffs", 5, "model.sh_coeffs"), ("sh_degree", 4, "model.sh_degree")):
        a = _filled()
        setattr(a.model, field, value)
        rc, msg = _refused(a)
        assert rc == _lib.GHR_E_INVALID and word in msg, (field, msg)
    a = _filled()
    a.model.dens_grad_accum = X
    rc, msg = _refused(a)
    assert rc == _lib.GHR_E_INVALID and "all three or none" in msg, msg
    a = _filled()
    a.model.dens_img_ws = X + 256
    rc, msg = _refused(a)
    assert rc == _lib.GHR_E_INVALID and "model.dens_img_ws must be img_ws" in msg, msg
    a = _filled()
    a.model.overflow_raises_flag = 1
    rc, msg = _refused(a)
    assert rc == _lib.GHR_E_INVALID and "overflow_raises_flag" in msg, msg


def test_sh_fold_is_checked_against_the_model():
    f = _lib.ShFoldArgs()
    f.P, f.sh_degree, f.sh_coeffs, f.n_views = 257, 3, 16, 2
    f.xyz = f.campos = f.g_views = f.d_features_dc = f.d_features_rest = X
    f.campos_stride = f.view_stride = 776
    a = _filled()
    a.sh_fold = ctypes.addressof(f)
    f.P = 256
    rc, msg = _refused(a)
    assert rc == _lib.GHR_E_INVALID and "sh_fold.P" in msg, msg
    f.P, f.view_stride = 257, 700  # two views' tables would overlap
    rc, msg = _refused(a)
    assert rc == _lib.GHR_E_INVALID and "sh_fold" in msg and "overlapping" in msg, msg
    f.view_stride, f.g_views = 776, None
    rc, msg = _refused(a)
    assert rc == _lib.GHR_E_INVALID and "sh_fold.g_views is NULL" in msg, msg


def test_ctypes_structs_have_the_layout_of_the_header(tmp_path):
    """The binding restates ghr_view_step_args and ghr_sh_fold_args field by field: sizes and offsets from the C compiler."""
    fields = {"ghr_view_step_args": [n for n, _ in _lib.ViewStepArgs._fields_],
              "ghr_sh_fold_args": [n for n, _ in _lib.ShFoldArgs._fields_]}
    lines = ['#include <cstdio>', '#include <cstddef>', '#include "ghr.h"', 'int main() {']
    for s, names in fields.items():
        lines.append('std::printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for n in names:
            lines.append('std::printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, n, s, n))
    lines.append('return 0; }')
    src = tmp_path / "layout.cpp"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([_lib._hipcc(), "-x", "c++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)],
                   check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for s, cls in (("ghr_view_step_args", _lib.ViewStepArgs), ("ghr_sh_fold_args", _lib.ShFoldArgs)):
        assert int(got[s]) == ctypes.sizeof(cls), s
        for n, _ in cls._fields_:
            assert int(got["%s.%s" % (s, n)]) == getattr(cls, n).offset, (s, n)


def test_a_model_on_another_device_than_the_background_is_not_eligible():
    """The native views launch on the background's device with the model's pointers: a mismatch takes the Python path (or
    raises with native=True) before anything else is looked at."""
    from types import SimpleNamespace
    import torch
    from gaussianhaircut_amd import native_step
    plan = SimpleNamespace(fused_sink=True, all_direct=True, defer=True, factored=None)
    model = SimpleNamespace(_xyz=torch.zeros(4, 3))
    why = native_step.ineligible(plan, model, [object()], torch.zeros(10, device="meta"), SimpleNamespace(debug=False), None, [])
    assert why is not None and "different devices" in why
