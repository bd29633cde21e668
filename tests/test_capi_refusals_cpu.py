"""What the C API refuses, and with which words, decided from the arguments alone (no GPU).

tests/golden/capi_refusals.json is a table of calls -- an entry point, a well-formed argument set (BASES below) and the fields
a case changes -- with the (return code, ghr_last_error text) each gave when the table was recorded.  Every call in it ends
before the HIP runtime is touched: a refusal, or one of the empty argument sets (P == 0, rows_total == 0, n_strands == 0) that
return GHR_OK at once.  The replay compares byte for byte, so a host-side change of the library keeps every code and message.

The second half is about ghr_view_step: it asks up front everything the six calls it composes would refuse, so each rule it
shares with one of them must be refused by both -- by ghr_view_step and by the call that owns the rule.

The "expect" column is what the library answered BEFORE its host layer was reworked: it is not re-recorded from a later tree.
"""
import ctypes
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gaussianhaircut_amd import _lib  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "golden", "capi_refusals.json")
X = 0x1000  # stands for a buffer: none of these calls follows a pointer (but "@word", a real uint32, and the group tables)


def _view_args():
    a = _lib.ViewArgs()
    a.P, a.W, a.H, a.C = 257, 33, 17, 10
    for n in ("background", "means3D", "colors", "opacities", "scales", "rotations", "viewmatrix", "projmatrix"):
        setattr(a, n, X)
    a.scale_modifier, a.tan_fovx, a.tan_fovy = 1.0, 0.5, 0.5
    return a


def _model_args():
    m = _lib.ModelArgs()
    m.P, m.W, m.H, m.sh_degree, m.sh_coeffs = 257, 33, 17, 3, 16
    for n in ("xyz", "log_scales", "rotations", "opacity_logit", "label_logit", "orient_conf_log", "features_dc", "features_rest",
              "viewmatrix", "projmatrix", "campos", "background"):
        setattr(m, n, X)
    # the eight raw-parameter arrays as the groups of one flat optimizer buffer at X (_adam_fuse, _ends)
    for n, col in zip(("xyz", "log_scales", "rotations", "opacity_logit", "label_logit", "orient_conf_log", "features_dc",
                       "features_rest"), (0, 3, 6, 10, 11, 12, 13, 16)):
        setattr(m, n, X + 4 * 257 * col)
    m.scale_modifier, m.tan_fovx, m.tan_fovy, m.conic_eps = 1.0, 0.5, 0.5, 1e-12
    return m


def _strand_model_args():
    m = _model_args()
    m.P, m.mode, m.dir3d = 258, 1, X
    return m


def _shared():
    sf = _lib.SharedFeatures()
    sf.n_strands, sf.rows_per_strand = 129, 2
    return sf


def _view_step_args():
    v = _lib.ViewStepArgs()
    v.model = _model_args()
    v.R = 4096
    for n in ("geom_ws", "img_ws", "bin_ws", "radii", "means2D_out", "render", "maps", "sums", "loss_out", "grad_loss",
              "d_pix", "grad_scratch", "d_means2D", "d_xyz", "d_log_scales", "d_rotations", "d_opacity_logit", "d_label_logit",
              "d_orient_conf_log", "d_features_dc", "d_features_rest", "nan_flag", "R_host"):
        setattr(v, n, X)
    l = v.loss
    l.W, l.H = 33, 17
    l.gt_image = l.gt_mask = l.gt_orient_angle = l.gt_orient_conf = X
    l.w_l1, l.w_ssim, l.w_mask, l.w_orient = 0.8, 0.2, 0.1, 0.1
    v.prezero, v.accumulate = 1, 0
    return v


def _adam_fuse():
    """The optimizer state of the 257-row model above: eight groups that tile 61 floats per row; every array at X."""
    f = _lib.AdamFuse()
    f.n = 257 * 61
    for n in ("p_in", "m_in", "v_in", "p_out", "m_out", "v_out", "state", "flag", "flag_next"):
        setattr(f, n, X)
    f.n_groups = 8
    f.beta1, f.beta2, f.eps = 0.9, 0.999, 1e-15
    return f


def _sh_fold():
    f = _lib.ShFoldArgs()
    f.P, f.sh_degree, f.sh_coeffs, f.n_views = 257, 3, 16, 2
    f.xyz = f.campos = f.g_views = f.d_features_dc = f.d_features_rest = X
    f.campos_stride = f.view_stride = 776
    return f


def _ends():
    return (ctypes.c_int64 * 8)(*[257 * e for e in (3, 6, 10, 11, 12, 13, 16, 61)])


def _lrs():
    return (ctypes.c_float * 8)(*([1e-3] * 8))


def _widths():
    return (ctypes.c_int32 * 8)(3, 3, 4, 1, 1, 1, 3, 45)


_BWD_GRADS = ["d_means2D", "d_xyz", "d_log_scales", "d_rotations", "d_opacity_logit", "d_label_logit", "d_orient_conf_log",
              "d_features_dc", "d_features_rest"]
_ADAM_TAIL = [("n_groups", 8), ("group_end_host", _ends), ("lr_host", _lrs), ("beta1", 0.9), ("beta2", 0.999), ("eps", 1e-15)]

# entry point -> its arguments in the order of include/ghr.h, each with a well-formed value (a callable makes a fresh one)
BASES = {
    "ghr_forward_stage1": [("stream", None), ("a", _view_args), ("geom_ws", X), ("img_ws", X), ("radii", X), ("R_host", "@word")],
    "ghr_forward_stage2": [("stream", None), ("a", _view_args), ("R", 4096), ("geom_ws", X), ("img_ws", X), ("bin_ws", X),
                           ("out_color", X), ("grad_scratch", X)],
    "ghr_backward": [("stream", None), ("a", _view_args), ("R", 4096), ("radii", X), ("geom_ws", X), ("img_ws", X), ("bin_ws", X),
                     ("dL_dpix", X), ("grad_scratch", X)] +
                    [(n, X) for n in ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors", "dL_dmeans3D", "dL_dcov3D",
                                      "dL_dscales", "dL_drotations")] + [("prezeroed", 0)],
    "ghr_model_forward_segment": [("stream", None), ("m", _model_args), ("rows_total", 257), ("first", 1), ("geom_ws", X),
                                  ("img_ws", X), ("radii", X), ("means2D_out", X)],
    "ghr_model_forward_segment_shared": [("stream", None), ("m", _strand_model_args), ("sf", _shared), ("rows_total", 258),
                                         ("first", 1), ("geom_ws", X), ("img_ws", X), ("radii", X), ("means2D_out", X)],
    "ghr_model_forward_finish": [("stream", None), ("rows_total", 257), ("W", 33), ("H", 17), ("debug", 0), ("geom_ws", X),
                                 ("img_ws", X), ("R_host", "@word")],
    "ghr_model_forward_stage1": [("stream", None), ("m", _model_args), ("geom_ws", X), ("img_ws", X), ("radii", X),
                                 ("means2D_out", X), ("R_host", "@word")],
    "ghr_render_backward": [("stream", None), ("rows_total", 257), ("W", 33), ("H", 17), ("R", 4096), ("background", X),
                            ("geom_ws", X), ("img_ws", X), ("bin_ws", X), ("dL_dpix", X), ("grad_scratch", X), ("prezeroed", 0)],
    "ghr_model_backward_segment": [("stream", None), ("m", _model_args), ("rows_total", 257), ("radii", X), ("geom_ws", X),
                                   ("grad_scratch", X)] + [(n, X) for n in _BWD_GRADS] +
                                  [("d_dir3d", None), ("accumulate", 0), ("nan_flag", X), ("grad_rows", 4096), ("bin_ws", X),
                                   ("R", 4096)],
    "ghr_model_backward_segment_shared": [("stream", None), ("m", _strand_model_args), ("sf", _shared), ("rows_total", 258),
                                          ("radii", X), ("geom_ws", X), ("grad_scratch", X)] + [(n, X) for n in _BWD_GRADS] +
                                         [("d_dir3d", X), ("nan_flag", X), ("grad_rows", 4096), ("bin_ws", X), ("R", 4096),
                                          ("d_rgb_ws", X)],
    "ghr_model_backward": [("stream", None), ("m", _model_args), ("R", 4096), ("radii", X), ("geom_ws", X), ("img_ws", X),
                           ("bin_ws", X), ("dL_dpix", X), ("grad_scratch", X)] + [(n, X) for n in _BWD_GRADS] +
                          [("accumulate", 0), ("nan_flag", X), ("prezeroed", 0)],
    "ghr_shared_sh_fold": [("stream", None), ("sf", _shared), ("sh_degree", 3), ("sh_coeffs", 16), ("xyz", X), ("campos", X),
                           ("d_rgb", X), ("d_features_dc", X), ("d_features_rest", X), ("nan_flag", X)],
    "ghr_sh_grad_from_views": [("stream", None), ("P", 257), ("sh_degree", 3), ("sh_coeffs", 16), ("xyz", X), ("n_views", 2),
                               ("campos", X), ("campos_stride", 776), ("g_views", X), ("view_stride", 776), ("d_features_dc", X),
                               ("d_features_rest", X), ("accumulate", 0), ("nan_flag", X), ("flag_offset", 771)],
    "ghr_ws_inspect": [("P", 257), ("W", 33), ("H", 17), ("mode_b", 0), ("R", 4096), ("geom_ws", X), ("img_ws", X), ("bin_ws", X),
                       ("out", _lib.WsView)],
    "ghr_adam_step": [("stream", None), ("n", 257 * 61), ("p", X), ("g", X), ("m", X), ("v", X), ("state", X)] + _ADAM_TAIL +
                     [("nan_guard", 0), ("zero_grad", 1), ("skip_mask", 0)],
    "ghr_adam_step_range": [("stream", None), ("n", 257 * 61), ("begin", 0), ("count", 257 * 61), ("p", X), ("g", X), ("m", X),
                            ("v", X), ("state", X)] + _ADAM_TAIL + [("nan_guard", 0), ("zero_grad", 1), ("last", 1), ("skip_mask", 0)],
    "ghr_adam_step_range_to": [("stream", None), ("n", 257 * 61), ("begin", 0), ("count", 257 * 61), ("p_in", X), ("m_in", X),
                               ("v_in", X), ("p_out", X + 256), ("g", X), ("m_out", X + 256), ("v_out", X + 256), ("state", X),
                               ("flag", X), ("nan_mark", 0)] + _ADAM_TAIL + [("zero_grad", 1), ("skip_mask", 0)],
    "ghr_adam_fused_finish": [("stream", None), ("af", _adam_fuse)],
    "ghr_adam_nan_scan": [("stream", None), ("g", X), ("count", 257), ("state", X)],
    "ghr_adam_relay_rows": [("stream", None), ("n_groups", 8), ("width_host", _widths), ("P_old", 257), ("P_new", 300),
                            ("take", X), ("fresh", X), ("child", X), ("override_host", None)] +
                           [(n, X) for n in ("p_in", "m_in", "v_in", "p_out", "m_out", "v_out")],
    "ghr_view_step": [("stream", None), ("v", _view_step_args)],
}
BASES["ghr_backward_ex"] = BASES["ghr_backward"] + [("dL_dconic3", None)]


class Call:
    """One call of the table: BASES[fn] with the case's changes.  Changes are {"path": value} in order; a path is an argument
    or a field below it ("a.P", "v.model.sh_coeffs"), or a field of one of the side structs "af" (ghr_adam_fuse) / "shf"
    (ghr_sh_fold_args).  Values: a number, null, "X" / "X+<n>" (a stand-in pointer), "@word" (a real uint32), "@af" / "@shf"
    (the side struct's address), or a list (an array: of float for lr_host, of int32 for width_host, else of int64)."""

    def __init__(self, fn, changes=None, deterministic=0):
        self.fn, self.deterministic = fn, deterministic
        self.word = ctypes.c_uint32(0xdeadbeef)
        self.side = {"af": _adam_fuse(), "shf": _sh_fold()}
        self.keep = [_ends(), _lrs()]
        self.side["af"].group_end_host = ctypes.cast(self.keep[0], ctypes.c_void_p)
        self.side["af"].lr_host = ctypes.cast(self.keep[1], ctypes.c_void_p)
        self.args = {n: (d() if callable(d) else d) for n, d in BASES[fn]}
        for path, value in (changes or {}).items():
            self.set(path, value)

    def _value(self, path, v):
        if v == "X":
            return X
        if isinstance(v, str) and v.startswith("X+"):
            return X + int(v[2:])
        if v == "@word":
            return ctypes.addressof(self.word)
        if v in ("@af", "@shf"):
            return ctypes.addressof(self.side[v[1:]])
        if isinstance(v, list):
            leaf = path.rpartition(".")[2]
            arr = ({"lr_host": ctypes.c_float, "width_host": ctypes.c_int32}.get(leaf, ctypes.c_int64) * len(v))(*v)
            self.keep.append(arr)
            return arr
        return v

    def set(self, path, v):
        v = self._value(path, v)
        head, _, rest = path.partition(".")
        if not rest:
            assert head in self.args, path
            self.args[head] = v
            return
        obj = self.args[head] if head in self.args else self.side[head]
        *mid, leaf = rest.split(".")
        for n in mid:
            obj = getattr(obj, n)
        assert hasattr(obj, leaf), path
        if isinstance(v, ctypes.Array):
            v = ctypes.cast(v, ctypes.c_void_p)
        setattr(obj, leaf, v)

    def run(self):
        L = _lib.lib()
        argv = []
        for n, _ in BASES[self.fn]:
            a = self.args[n]
            a = self._value(n, a) if isinstance(a, str) else a
            argv.append(ctypes.byref(a) if isinstance(a, ctypes.Structure) else a)
        prev = L.ghr_set_deterministic(self.deterministic)
        try:
            rc = getattr(L, self.fn)(*argv)
        finally:
            L.ghr_set_deterministic(prev)
        return [int(rc), L.ghr_last_error().decode() if rc != _lib.GHR_OK else ""]


def _table():
    with open(TABLE) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("case", _table(), ids=lambda c: c["id"])
def test_the_call_is_answered_as_recorded(case):
    call = Call(case["fn"], case.get("set"), case.get("deterministic", 0))
    got = call.run()
    assert got == case["expect"], (case["id"], got)
    if got[0] == _lib.GHR_OK and "R_host" in call.args and call.args["R_host"] == "@word":
        assert call.word.value == 0  # an empty pass counts no instances


def test_the_table_covers_the_entry_points_it_is_about():
    cases = _table()
    assert len({c["id"] for c in cases}) == len(cases)
    assert {c["fn"] for c in cases} == set(BASES)
    ok = {c["fn"] for c in cases if c["expect"][0] == _lib.GHR_OK}
    assert ok >= {"ghr_forward_stage1", "ghr_backward_ex", "ghr_model_forward_segment", "ghr_model_forward_segment_shared",
                  "ghr_model_forward_finish", "ghr_model_forward_stage1", "ghr_render_backward", "ghr_model_backward_segment",
                  "ghr_model_backward", "ghr_shared_sh_fold", "ghr_sh_grad_from_views"}
    assert "ghr_forward_stage2" not in ok  # (at P == 0 it zero-fills the image: a runtime call)


# ---- ghr_view_step and the six calls it composes: one rule, refused by both ------------------------------------------------
def _owner(fn, v, **over):
    """The composed call `fn` with the fields ghr_view_step would pass it from `v` (arguments not named here keep BASES')."""
    m = v.args["v"].model
    c = Call(fn)
    if "m" in c.args:
        c.args["m"] = m
    for n, _ in BASES[fn]:
        if n in over:
            c.args[n] = over[n]
        elif n not in ("stream", "m", "a") and hasattr(v.args["v"], n):
            c.args[n] = getattr(v.args["v"], n)
    c.deterministic = v.deterministic
    return c


def _drift_cases():
    """(rule, the ghr_view_step call that breaks only it, a word of its message, the owner's call, a word of its message)"""
    big_r = {"v.model.W": 16, "v.model.H": 16, "v.loss.W": 16, "v.loss.H": 16}
    seg = dict(rows_total=257, grad_rows=4096)
    fuse = {"v.model.adam_fuse": "@af", "v.model.dens_img_ws": "X", "v.model.overflow_raises_flag": 1}
    fold = {"nan_flag": None, "flag_offset": 0}
    return [
        # (R >> 6) + T + 1 groups of 128 B reach 2^32 B; T = 1 at 16 x 16 pixels.  Nothing is allocated: refused first
        ("cell-mask offsets", Call("ghr_view_step", dict(big_r, **{"v.R": 2 ** 31})), "cell masks",
         lambda v: Call("ghr_forward_stage2", {"a.W": 16, "a.H": 16, "R": 2 ** 31}), "cell masks"),
        ("ordered walk's offsets", Call("ghr_view_step", dict(big_r, **{"v.R": 2 ** 26}), deterministic=1), "ghr_set_deterministic",
         lambda v: _owner("ghr_render_backward", v, rows_total=257, W=16, H=16, dL_dpix=X), "ghr_set_deterministic"),
        ("sh_coeffs covers sh_degree", Call("ghr_view_step", {"v.model.sh_coeffs": 9}), "model.sh_coeffs",
         lambda v: _owner("ghr_model_forward_stage1", v), "sh_coeffs"),
        ("sh_coeffs is a square", Call("ghr_view_step", {"v.model.sh_degree": 1, "v.model.sh_coeffs": 5}), "model.sh_coeffs",
         lambda v: _owner("ghr_model_forward_stage1", v), "sh_coeffs"),
        ("dens_* all or none", Call("ghr_view_step", {"v.model.dens_denom": "X"}), "all three or none",
         lambda v: _owner("ghr_model_backward_segment", v, **seg), "all three or none"),
        ("SH gradients stored somewhere", Call("ghr_view_step", {"v.d_features_rest": None}), "d_features_rest",
         lambda v: _owner("ghr_model_backward_segment", v, **seg), "NULL buffer"),
        ("sh_fold views do not overlap", Call("ghr_view_step", {"v.sh_fold": "@shf", "shf.view_stride": 700}), "overlapping",
         lambda v: Call("ghr_sh_grad_from_views", dict(fold, view_stride=700)), "overlapping"),
        ("sh_fold degree", Call("ghr_view_step", {"v.sh_fold": "@shf", "shf.sh_degree": 4}), "sh_fold",
         lambda v: Call("ghr_sh_grad_from_views", dict(fold, sh_degree=4)), "bad sizes"),
        ("adam_fuse raises the call's own flag", Call("ghr_view_step", dict(fuse, **{"v.nan_flag": "X+4"})), "adam_fuse->flag",
         lambda v: _owner("ghr_model_backward_segment", v, **seg), "adam_fuse->flag"),
        ("adam_fuse arrays tile p_in", Call("ghr_view_step", dict(fuse, **{"af.n": 257 * 61 + 4})), "tile p_in",
         lambda v: _owner("ghr_model_backward_segment", v, **seg), "tile p_in"),
        ("adam_fuse arrays inside their groups",
         Call("ghr_view_step", dict(fuse, **{"af.group_end_host": [257 * e for e in (3, 6, 9, 11, 12, 13, 16, 61)]})), "straddles",
         lambda v: _owner("ghr_model_backward_segment", v, **seg), "straddles"),
    ]


@pytest.mark.parametrize("rule,step,word,owner,owner_word", [pytest.param(*c, id=c[0]) for c in _drift_cases()])
def test_a_rule_of_a_composed_call_is_refused_by_the_view_step_and_by_its_owner(rule, step, word, owner, owner_word):
    """The struct is _view_step_args() -- well-formed, like the one of test_native_step_cpu.py -- but for the one rule, and
    each side names that rule in its message."""
    rc, msg = step.run()
    assert rc == _lib.GHR_E_INVALID and word in msg, (rule, rc, msg)
    rc, msg = owner(step).run()
    assert rc == _lib.GHR_E_INVALID and owner_word in msg, (rule, rc, msg)

