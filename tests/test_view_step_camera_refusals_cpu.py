"""What ghr_view_step_camera and the two exchange entries of the camera bank refuse (no GPU).

Every call below is refused from its arguments alone, before the HIP runtime is touched: GHR_E_INVALID, and ghr_last_error() names
the field.  The pointers stand for buffers (X); nothing follows them.
"""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gaussianhaircut_amd import _lib  # noqa: E402

X = 0x10000      # stands for a buffer
ROW = 0x20000    # out_row
P, W, H = 257, 33, 17


def _view():
    v = _lib.ViewStepArgs()
    m = v.model
    m.P, m.W, m.H, m.sh_degree, m.sh_coeffs = P, W, H, 3, 16
    for n in ("xyz", "log_scales", "rotations", "opacity_logit", "label_logit", "orient_conf_log", "features_dc", "features_rest",
              "background"):
        setattr(m, n, X)
    m.scale_modifier, m.tan_fovx, m.tan_fovy, m.conic_eps = 1.0, 1.0, 1.0, 1e-12
    m.viewmatrix, m.projmatrix, m.campos = ROW, ROW + 4 * 16, ROW + 4 * 48
    m.fovx_dev, m.fovy_dev = ROW + 4 * 51, ROW + 4 * 52
    m.cam_partial, m.cam_slot0, m.cam_slots = X, 0, int(_lib.lib().ghr_camera_slots(P))
    v.R = 4096
    for n in ("geom_ws", "img_ws", "bin_ws", "radii", "means2D_out", "render", "maps", "sums", "loss_out", "grad_loss",
              "d_pix", "grad_scratch", "d_means2D", "d_xyz", "d_log_scales", "d_rotations", "d_opacity_logit", "d_label_logit",
              "d_orient_conf_log", "d_features_dc", "d_features_rest", "nan_flag", "R_host"):
        setattr(v, n, X)
    l = v.loss
    l.W, l.H = W, H
    l.gt_image = l.gt_mask = l.gt_orient_angle = l.gt_orient_conf = X
    l.w_l1, l.w_ssim, l.w_mask, l.w_orient = 0.8, 0.2, 0.1, 0.1
    v.prezero = 1
    return v


def _camera():
    c = _lib.ViewCameraArgs()
    c.parametrisation, c.rows, c.index = _lib.CAMERA_SE3, 5, 2
    c.consts, c.const_stride, c.params, c.param_stride = X, _lib.CAMERA_CONST, X, 8
    c.grads, c.grad_stride, c.touched = X, 8, X
    c.train_mask = _lib.CAMERA_TRAIN_POSE | _lib.CAMERA_TRAIN_FOV
    c.out_row, c.d_cam = ROW, X
    return c


def _refused(rc, *words):
    assert rc == _lib.GHR_E_INVALID
    msg = _lib.lib().ghr_last_error().decode()
    for w in words:
        assert w in msg, msg
    return msg


def _set(obj, path, value):
    *head, last = path.split(".")
    for h in head:
        obj = getattr(obj, h)
    setattr(obj, last, value)


def test_symbols_and_abi():
    L = _lib.lib()
    for name in ("ghr_view_step_camera", "ghr_camera_pack_row_message", "ghr_camera_merge_ranks"):
        assert hasattr(L, name)
    assert int(L.ghr_abi_version()) == 20 == _lib.ABI_VERSION


def test_null_structs():
    L = _lib.lib()
    _refused(L.ghr_view_step_camera(None, ctypes.byref(_view()), None), "ghr_view_step_camera", "(c) is NULL")
    _refused(L.ghr_view_step_camera(None, None, ctypes.byref(_camera())), "ghr_view_step_camera", "NULL")


CAMERA_CASES = [
    ("index", -1, "index outside rows"),
    ("index", 5, "index outside rows"),
    ("index", 1 << 30, "index outside rows"),
    ("rows", 0, "index outside rows"),
    ("train_mask", 0, "train_mask"),
    ("train_mask", 4, "train_mask"),
    ("out_row", None, "out_row is NULL"),
    ("d_cam", None, "d_cam is NULL"),
    ("grads", None, "grads is NULL"),
    ("touched", None, "touched is NULL"),
    ("consts", None, "NULL base pointer"),
    ("params", None, "NULL base pointer"),
    ("parametrisation", 2, "parametrisation"),
    ("param_stride", 7, "stride"),
    ("grad_stride", 7, "grad_stride"),
    ("const_stride", 20, "stride"),
]


@pytest.mark.parametrize("field,value,word", CAMERA_CASES, ids=["%s=%s" % (f, v) for f, v, _ in CAMERA_CASES])
def test_camera_struct_refusals(field, value, word):
    v, c = _view(), _camera()
    setattr(c, field, value)
    _refused(_lib.lib().ghr_view_step_camera(None, ctypes.byref(v), ctypes.byref(c)), "ghr_view_step_camera", word)


VIEW_CASES = [
    ("model.cam_partial", None, "model.cam_partial"),
    ("model.cam_slots", 4, "model.cam_slots"),
    ("model.cam_slots", 6, "model.cam_slots"),
    ("model.cam_slot0", 1, "model.cam_slot"),
    ("model.fovx_dev", None, "model.fovx_dev"),
    ("model.fovy_dev", None, "fovy_dev"),
    ("model.viewmatrix", ROW + 4, "model.viewmatrix"),
    ("model.projmatrix", ROW, "model.projmatrix"),
    ("model.campos", ROW + 4 * 32, "model.campos"),
    ("model.fovx_dev", ROW + 4 * 52, "model.fovx_dev"),
    ("model.fovy_dev", ROW + 4 * 51, "model.fovy_dev"),
    # ... and what ghr_view_step refuses, in its words
    ("model.P", 0, "model.P"),
    ("model.mode", 1, "model.mode"),
    ("model.debug", 1, "model.debug"),
    ("model.cam_only", 1, "cam_only"),
    ("model.detach_means2D", 1, "detach_means2D"),
    ("model.xyz", None, "model.xyz"),
    ("model.background", None, "model.background"),
    ("render", None, "render"),
    ("d_pix", None, "d_pix"),
    ("d_xyz", None, "d_xyz"),
    ("R_host", None, "R_host"),
    ("loss.W", W + 1, "loss.W"),
    ("loss.gt_image", None, "loss.gt_image"),
    ("model.sh_degree", 4, "model.sh_degree"),
]


@pytest.mark.parametrize("path,value,word", VIEW_CASES, ids=["%s=%s" % (p, v) for p, v, _ in VIEW_CASES])
def test_view_struct_refusals(path, value, word):
    v, c = _view(), _camera()
    _set(v, path, value)
    _refused(_lib.lib().ghr_view_step_camera(None, ctypes.byref(v), ctypes.byref(c)), word)


def test_out_row_moved_under_the_model():
    """the model's five pointers must point into THIS out_row"""
    v, c = _view(), _camera()
    c.out_row = ROW + 4 * _lib.CAMERA_OUT
    _refused(_lib.lib().ghr_view_step_camera(None, ctypes.byref(v), ctypes.byref(c)), "model.viewmatrix must be out_row")


def test_view_step_keeps_refusing_camera_gradients():
    L = _lib.lib()
    _refused(L.ghr_view_step(None, ctypes.byref(_view())), "ghr_view_step", "cam_partial")
    v = _view()
    v.model.cam_partial = None
    _refused(L.ghr_view_step(None, ctypes.byref(v)), "ghr_view_step", "fovx_dev")


PACK = dict(n=5, width=8, grads=X, grad_stride=8, touched=X, message=X)
MERGE = dict(n=5, width=8, G=2, gathered=X, grads=X, grad_stride=8, touched=X)


def _pack(**kw):
    a = dict(PACK, **kw)
    return _lib.lib().ghr_camera_pack_row_message(None, a["n"], a["width"], a["grads"], a["grad_stride"], a["touched"], a["message"])


def _merge(**kw):
    a = dict(MERGE, **kw)
    return _lib.lib().ghr_camera_merge_ranks(None, a["n"], a["width"], a["G"], a["gathered"], a["grads"], a["grad_stride"],
                                             a["touched"])


@pytest.mark.parametrize("field", ["grads", "touched", "message"])
def test_pack_null(field):
    _refused(_pack(**{field: None}), "ghr_camera_pack_row_message", field + " is NULL")


@pytest.mark.parametrize("field", ["gathered", "grads", "touched"])
def test_merge_null(field):
    _refused(_merge(**{field: None}), "ghr_camera_merge_ranks", field + " is NULL")


@pytest.mark.parametrize("G", [0, -1])
def test_merge_ranks_below_one(G):
    _refused(_merge(G=G), "ghr_camera_merge_ranks", "G < 1")


@pytest.mark.parametrize("width", [0, 7, 9, 10, 12, -8])
def test_exchange_width(width):
    _refused(_pack(width=width, grad_stride=16), "ghr_camera_pack_row_message", "width")
    _refused(_merge(width=width, grad_stride=16), "ghr_camera_merge_ranks", "width")


def test_exchange_other_sizes():
    _refused(_pack(n=-1), "n < 0")
    _refused(_merge(n=-1), "n < 0")
    _refused(_pack(width=11, grad_stride=8), "grad_stride")
    _refused(_merge(width=11, grad_stride=8), "grad_stride")
    # an empty bank is no error and launches nothing
    assert _pack(n=0) == _lib.GHR_OK and _merge(n=0) == _lib.GHR_OK
