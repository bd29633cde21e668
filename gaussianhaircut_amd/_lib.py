"""ctypes binding of ``libghr_hip.so`` (C ABI in ``include/ghr.h``) and its in-tree build recipe.

The shared library is the product: there is **no** CPU or eager-PyTorch fallback.  If the library is missing and
cannot be built (no ``hipcc``) importing it raises, and every entry point refuses non-ROCm tensors.
"""
from __future__ import annotations

import ctypes
import os
import shutil
import subprocess
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("GHR_LIB_PATH") or os.path.join(CSRC, "libghr_hip.so")  # override: kernel experiments
SOURCES = ["ghr_capi.hip"]
HEADERS = ["ghr_device.h", "ghr_preprocess.h", "ghr_binning.h", "ghr_render_fwd.h", "ghr_render_bwd.h", "ghr_render_bwd2.h", "ghr_render_bwd3.h",
           "ghr_geom_bwd.h", "ghr_project.h", "ghr_loss.h", "ghr_adam.h", "ghr_strands.h", "ghr_knn.h", "ghr_camera.h", "ghr_eval.h", "ghr_products.h", "ghr_orient.h", "ghr_gt.h", "ghr_latent.h", "ghr_shared.h", "ghr_mesh.h", "ghr_meshdist.h", "ghr_tilelists.h", "ghr_visibility.h", "ghr_strandview.h", "ghr_sds.h", "ghr_nn.h", "ghr_compare.h", "ghr_texstrands.h", "ghr_guides.h", "ghr_haar.h", "ghr_capture.h", "ghr_field.h", "ghr_grow.h", "ghr_shape.h", "ghr_upsample.h"]
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-munsafe-fp-atomics", "-fPIC",
               "-shared"]

NUM_CHANNELS = 10
GRAD_STRIDE = 16
CAM_PARTIALS = 32  # GHR_CAM_PARTIALS: rows of the camera-gradient partial table
CAM_GRADS = 37     # GHR_CAM_GRADS: d view[16] | d proj[16] | d camera_center[3] | d tanfov[2]
STRAND_MAX_SEG = 2048  # GHR_STRAND_MAX_SEG: longest strand ghr_strand_build takes
ADAM_STATE = 18  # GHR_ADAM_STATE
CAMERA_ORTHO6D, CAMERA_SE3 = 0, 1  # GHR_CAMERA_*: parametrisation of a camera bank's rotation residual
CAMERA_CONST, CAMERA_OUT = 21, 53  # GHR_CAMERA_CONST / GHR_CAMERA_OUT: floats per constants / output row
CAMERA_TRAIN_POSE, CAMERA_TRAIN_FOV = 1, 2  # GHR_CAMERA_TRAIN_*
EVAL_TERMS = 8  # GHR_EVAL_TERMS: doubles per view of the evaluation table {l1, ce, or_num, or_den, mse[3], ssim}
ABI_VERSION = 20  # GHR_ABI_VERSION of include/ghr.h this binding was written for

GHR_OK, GHR_E_INVALID, GHR_E_NOCOLORS, GHR_E_HIP = 0, -1, -2, -3


class GhrError(RuntimeError):
    pass


def _hipcc() -> Optional[str]:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def _stale() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    deps = [os.path.join(CSRC, f) for f in SOURCES + HEADERS] + [os.path.join(_HERE, "..", "include", "ghr.h")]
    return any(os.path.exists(d) and os.path.getmtime(d) > t for d in deps)


def build_library(force: bool = False, verbose: bool = False) -> str:
    """Compile every HIP source for gfx950 into ``csrc/libghr_hip.so`` (cross-compiles without a GPU)."""
    if os.environ.get("GHR_LIB_PATH"):
        # an experiment library is used as it is: rebuilding it from the tree's sources (it is always "stale" after the
        # next edit) would silently turn an A/B into a comparison of the product with itself
        if not os.path.exists(LIB_PATH):
            raise GhrError("GHR_LIB_PATH=%s does not exist" % LIB_PATH)
        return LIB_PATH
    if not force and not _stale():
        return LIB_PATH
    hipcc = _hipcc()
    if hipcc is None:
        raise GhrError("libghr_hip.so is missing/stale and hipcc was not found; the HIP extension is required "
                       "(there is no CPU fallback)")
    tmp = LIB_PATH + ".tmp.%d" % os.getpid()
    cmd = [hipcc] + HIPCC_FLAGS + ["-o", tmp] + [os.path.join(CSRC, s) for s in SOURCES]
    if verbose:
        print(" ".join(cmd))
    res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    if res.returncode != 0:
        raise GhrError("hipcc failed:\n" + res.stdout + res.stderr)
    os.replace(tmp, LIB_PATH)
    return LIB_PATH


class ViewArgs(ctypes.Structure):
    """``ghr_view_args`` (include/ghr.h)."""
    _fields_ = [
        ("P", ctypes.c_int32), ("W", ctypes.c_int32), ("H", ctypes.c_int32), ("C", ctypes.c_int32),
        ("background", ctypes.c_void_p), ("means3D", ctypes.c_void_p), ("colors", ctypes.c_void_p),
        ("opacities", ctypes.c_void_p), ("scales", ctypes.c_void_p), ("rotations", ctypes.c_void_p),
        ("cov3D_precomp", ctypes.c_void_p), ("conic_precomp", ctypes.c_void_p), ("viewmatrix", ctypes.c_void_p),
        ("projmatrix", ctypes.c_void_p), ("scale_modifier", ctypes.c_float), ("tan_fovx", ctypes.c_float),
        ("tan_fovy", ctypes.c_float), ("prefiltered", ctypes.c_int32), ("debug", ctypes.c_int32),
        ("img_ws_recycled", ctypes.c_int32),
    ]


class ModelArgs(ctypes.Structure):
    """``ghr_model_args`` (include/ghr.h)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("P", "W", "H", "sh_degree", "sh_coeffs")] + \
               [(n, ctypes.c_void_p) for n in ("xyz", "log_scales", "rotations", "opacity_logit", "label_logit",
                                               "orient_conf_log", "features_dc", "features_rest", "viewmatrix",
                                               "projmatrix", "campos", "background")] + \
               [(n, ctypes.c_float) for n in ("scale_modifier", "tan_fovx", "tan_fovy", "conic_eps")] + \
               [("debug", ctypes.c_int32), ("mode", ctypes.c_int32), ("row0", ctypes.c_int32),
                ("dir3d", ctypes.c_void_p)] + \
               [(n, ctypes.c_float) for n in ("const_opacity", "const_label", "const_conf")] + \
               [("img_ws_recycled", ctypes.c_int32)] + \
               [("fovx_dev", ctypes.c_void_p), ("fovy_dev", ctypes.c_void_p), ("cam_partial", ctypes.c_void_p), ("cam_slot0", ctypes.c_int32),
                ("cam_slots", ctypes.c_int32), ("cam_only", ctypes.c_int32), ("detach_means2D", ctypes.c_int32),
                ("dens_grad_accum", ctypes.c_void_p), ("dens_denom", ctypes.c_void_p), ("dens_max_radii2D", ctypes.c_void_p),
                ("dens_img_ws", ctypes.c_void_p), ("overflow_raises_flag", ctypes.c_int32), ("adam_fuse", ctypes.c_void_p),
                ("d_rgb", ctypes.c_void_p)]


class AdamFuse(ctypes.Structure):
    """``ghr_adam_fuse`` (include/ghr.h): the optimizer update fused into the step's last projection backward."""
    _fields_ = [("n", ctypes.c_int64)] + \
               [(n, ctypes.c_void_p) for n in ("p_in", "m_in", "v_in", "p_out", "m_out", "v_out", "state", "flag", "flag_next")] + \
               [("n_groups", ctypes.c_int32), ("group_end_host", ctypes.c_void_p), ("lr_host", ctypes.c_void_p),
                ("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_float)]


class LossArgs(ctypes.Structure):
    """``ghr_loss_args`` (include/ghr.h)."""
    _fields_ = [("W", ctypes.c_int32), ("H", ctypes.c_int32)] + \
               [(n, ctypes.c_void_p) for n in ("image", "mask", "dir2d", "orient_conf", "gt_image", "gt_mask",
                                               "gt_orient_angle", "gt_orient_conf")] + \
               [(n, ctypes.c_float) for n in ("w_l1", "w_ssim", "w_mask", "w_orient")] + \
               [("unmasked_colours", ctypes.c_int32), ("gt_stats", ctypes.c_void_p)]


class ShFoldArgs(ctypes.Structure):
    """``ghr_sh_fold_args`` (include/ghr.h)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("P", "sh_degree", "sh_coeffs", "n_views")] + \
               [("xyz", ctypes.c_void_p), ("campos", ctypes.c_void_p), ("campos_stride", ctypes.c_int64),
                ("g_views", ctypes.c_void_p), ("view_stride", ctypes.c_int64), ("d_features_dc", ctypes.c_void_p),
                ("d_features_rest", ctypes.c_void_p), ("accumulate", ctypes.c_int32)]


class ViewStepArgs(ctypes.Structure):
    """``ghr_view_step_args`` (include/ghr.h): one training view -- forward, loss, backward -- in one call."""
    _fields_ = [("model", ModelArgs), ("R", ctypes.c_uint32), ("R_host", ctypes.c_void_p)] + \
               [(n, ctypes.c_void_p) for n in ("geom_ws", "img_ws", "bin_ws", "radii", "means2D_out", "render")] + \
               [("loss", LossArgs)] + \
               [(n, ctypes.c_void_p) for n in ("maps", "sums", "loss_out", "grad_loss", "d_pix", "grad_scratch")] + \
               [("prezero", ctypes.c_int32)] + \
               [(n, ctypes.c_void_p) for n in ("d_means2D", "d_xyz", "d_log_scales", "d_rotations", "d_opacity_logit",
                                               "d_label_logit", "d_orient_conf_log", "d_features_dc", "d_features_rest")] + \
               [("accumulate", ctypes.c_int32), ("nan_flag", ctypes.c_void_p), ("sh_fold", ctypes.c_void_p),
                ("count_event", ctypes.c_void_p), ("acc_wait_event", ctypes.c_void_p), ("acc_record_event", ctypes.c_void_p)]


class ViewCameraArgs(ctypes.Structure):
    """``ghr_view_camera_args`` (include/ghr.h): the bank row a ``ghr_view_step_camera`` view composes and back-propagates into."""
    _fields_ = [("parametrisation", ctypes.c_int32), ("rows", ctypes.c_int32), ("index", ctypes.c_int32),
                ("const_stride", ctypes.c_int32), ("consts", ctypes.c_void_p), ("params", ctypes.c_void_p),
                ("param_stride", ctypes.c_int32), ("grad_stride", ctypes.c_int32), ("grads", ctypes.c_void_p),
                ("touched", ctypes.c_void_p), ("train_mask", ctypes.c_int32), ("out_row", ctypes.c_void_p),
                ("d_cam", ctypes.c_void_p)]


class EvalArgs(ctypes.Structure):
    """``ghr_eval_args`` (include/ghr.h)."""
    _fields_ = [("W", ctypes.c_int32), ("H", ctypes.c_int32)] + \
               [(n, ctypes.c_void_p) for n in ("renders", "gt_image", "gt_mask", "gt_orient_angle", "gt_orient_conf")] + \
               [("with_ssim", ctypes.c_int32)]


class LatentLossArgs(ctypes.Structure):
    """``ghr_latent_loss_args`` (include/ghr.h)."""
    _fields_ = [("W", ctypes.c_int32), ("H", ctypes.c_int32)] + \
               [(n, ctypes.c_void_p) for n in ("image", "mask0", "dir2d", "orient_conf", "gt_image", "gt_mask0",
                                               "gt_orient_angle", "gt_orient_conf")] + \
               [(n, ctypes.c_float) for n in ("w_l1", "w_mask", "w_orient")]


class SharedFeatures(ctypes.Structure):
    """``ghr_shared_features`` (include/ghr.h): a segment whose SH coefficients are stored once per strand."""
    _fields_ = [("n_strands", ctypes.c_int32), ("rows_per_strand", ctypes.c_int32)]


class MeshGrid(ctypes.Structure):
    """``ghr_mesh_grid`` (include/ghr.h): the header of a containment grid blob."""
    _fields_ = [("magic", ctypes.c_uint32), ("G", ctypes.c_int32), ("n_faces", ctypes.c_int32), ("n_vertices", ctypes.c_int32),
                ("lo", ctypes.c_float * 3), ("hi", ctypes.c_float * 3), ("scale", ctypes.c_float * 3),
                ("list_total", ctypes.c_uint32 * 3), ("list_max", ctypes.c_uint32 * 3), ("pad_", ctypes.c_uint32),
                ("off_rec", ctypes.c_uint64 * 3), ("off_start", ctypes.c_uint64 * 3), ("off_list", ctypes.c_uint64 * 3),
                ("bytes", ctypes.c_uint64)]


class MeshTris(ctypes.Structure):
    """``ghr_mesh_tris`` (include/ghr.h): the header of a closest-point triangle blob."""
    _fields_ = [("magic", ctypes.c_uint32), ("n_faces", ctypes.c_int32), ("n_blocks", ctypes.c_int32), ("n_super", ctypes.c_int32),
                ("lo", ctypes.c_float * 3), ("hi", ctypes.c_float * 3), ("pad_", ctypes.c_uint32 * 2),
                ("off_rec", ctypes.c_uint64), ("off_bbox", ctypes.c_uint64), ("off_sbox", ctypes.c_uint64),
                ("off_keys", ctypes.c_uint64), ("bytes", ctypes.c_uint64)]


PROBE_REFERENCE, PROBE_AXIS_SCALED = 0, 1  # GHR_PROBE_*
STRANDVIEW_KAJIYA, STRANDVIEW_TANGENT = 0, 1  # GHR_STRANDVIEW_*


class StrandViewShading(ctypes.Structure):
    """``ghr_strandview_shading`` (include/ghr.h)."""
    _fields_ = [("eye", ctypes.c_float * 3), ("light", ctypes.c_float * 3), ("ambient", ctypes.c_float), ("kd", ctypes.c_float),
                ("ks", ctypes.c_float), ("shininess_log2", ctypes.c_int32), ("base_rgb", ctypes.c_float * 3),
                ("head_rgb", ctypes.c_float * 3), ("background_rgb", ctypes.c_float * 3)]


class StrandViewShadow(ctypes.Structure):
    """``ghr_strandview_shadow`` (include/ghr.h)."""
    _fields_ = [("Ml", ctypes.c_float * 12), ("near_w", ctypes.c_float), ("Hl", ctypes.c_int32), ("Wl", ctypes.c_int32),
                ("layer", ctypes.c_float), ("kappa", ctypes.c_float), ("bias", ctypes.c_float), ("q0", ctypes.c_void_p),
                ("layers", ctypes.c_void_p), ("qfl", ctypes.c_void_p)]


def latent_loss_sums_floats(W: int, H: int) -> int:
    """floats of the latent-stage loss kernels' ``sums`` for a W x H image (``ghr_latent_loss_sums_floats``)."""
    return int(lib().ghr_latent_loss_sums_floats(int(W), int(H)))


def loss_sums_floats(W: int, H: int) -> int:
    """floats of the loss kernels' ``sums`` scratch for a W x H image (``ghr_loss_sums_floats``)."""
    return int(lib().ghr_loss_sums_floats(int(W), int(H)))


class WsView(ctypes.Structure):
    """``ghr_ws_view`` (include/ghr.h) -- test introspection."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("rec", "depths", "rects", "cov3D", "final_T", "n_contrib",
                                                "tile_start", "keys", "point_list")]


# Every symbol include/ghr.h declares (the CPU test suite checks the library exports all of them).
EXPORTS = ["ghr_last_error", "ghr_abi_version", "ghr_forward_sizes", "ghr_binning_size", "ghr_forward_stage1",
           "ghr_forward_stage2", "ghr_backward", "ghr_backward_ex", "ghr_mark_visible", "ghr_ws_inspect", "ghr_set_profile_events", "ghr_set_deterministic", "ghr_selftest_wave", "ghr_selftest_math", "ghr_model_forward_stage1",
           "ghr_model_backward", "ghr_model_forward_segment", "ghr_model_forward_finish", "ghr_render_backward",
           "ghr_model_backward_segment", "ghr_camera_slots", "ghr_camera_grad_fold", "ghr_strand_build", "ghr_strand_build_backward", "ghr_strand_build_backward_ex", "ghr_sh_grad_from_views", "ghr_loss_sums_floats", "ghr_loss_forward", "ghr_loss_gt_stats", "ghr_loss_backward", "ghr_view_step", "ghr_adam_step",
           "ghr_adam_step_range", "ghr_adam_step_range_to", "ghr_adam_nan_scan", "ghr_adam_relay_rows", "ghr_adam_fused_finish",
           "ghr_knn_workspace_size", "ghr_knn_keys", "ghr_knn_mean_dist2",
           "ghr_camera_compose", "ghr_camera_compose_backward", "ghr_camera_adam_step",
           "ghr_view_step_camera", "ghr_camera_pack_row_message", "ghr_camera_merge_ranks",
           "ghr_eval_scratch_floats", "ghr_eval_metrics", "ghr_eval_products",
           "ghr_orient_dog_scratch_bytes", "ghr_orient_dog", "ghr_orient_bank_floats", "ghr_orient_gabor",
           "ghr_resample_scratch_bytes", "ghr_resample_u8", "ghr_gt_assemble", "ghr_gt_resize_variance", "ghr_gt_from_render",
           "ghr_strand_points_build", "ghr_strand_points_build_backward", "ghr_strand_rows_expand", "ghr_strand_rows_reduce",
           "ghr_latent_loss_sums_floats", "ghr_latent_loss_forward", "ghr_latent_loss_backward",
           "ghr_model_forward_segment_shared", "ghr_model_backward_segment_shared", "ghr_shared_sh_fold",
           "ghr_mesh_grid_sizes", "ghr_mesh_grid_build", "ghr_mesh_contains", "ghr_gaussian_probe_outside",
           "ghr_mesh_tris_sizes", "ghr_mesh_tris_build", "ghr_mesh_closest", "ghr_mesh_distance_backward",
           "ghr_vis_sizes", "ghr_vis_view", "ghr_vis_head_mask",
           "ghr_strandview_sizes", "ghr_strandview_face_depth", "ghr_strandview_raster", "ghr_strandview_shade",
           "ghr_strandview_resolve", "ghr_strandview_opacity", "ghr_strandview_shade_shadowed", "ghr_strandview_capture",
           "ghr_sds_local", "ghr_sds_local_backward", "ghr_sds_texture", "ghr_sds_texture_backward",
           "ghr_nn_workspace_size", "ghr_nn_search", "ghr_chamfer_point", "ghr_chamfer_point_backward",
           "ghr_cmp_over_white", "ghr_cmp_strip",
           "ghr_ts_fetch", "ghr_ts_fetch_backward", "ghr_ts_world", "ghr_ts_world_backward",
           "ghr_guides_blend", "ghr_guides_blend_backward",
           "ghr_field_workspace_size", "ghr_field_build", "ghr_field_query", "ghr_field_trace", "ghr_strands_resample",
           "ghr_field_trace_guarded",
           "ghr_shape_neighbours", "ghr_shape_forward", "ghr_shape_backward",
           "ghr_upsample_neighbours", "ghr_upsample_blend"]

_lib = None


def lib() -> ctypes.CDLL:
    """Load (building first if needed) the HIP library.  torch must be imported first so that the HIP runtime the
    library binds to (soname libamdhip64.so.7) is the one torch already loaded -- streams and pointers are shared."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (load torch's libamdhip64 first)
    build_library()
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, u32, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_float
    L.ghr_last_error.restype = ctypes.c_char_p
    L.ghr_abi_version.restype = ctypes.c_int
    got = int(L.ghr_abi_version())
    if got != ABI_VERSION:
        # a stale build or a GHR_LIB_PATH experiment library with other argument lists: calling it would read garbage
        raise GhrError("%s reports ABI %d, this binding needs %d (rebuild: gaussianhaircut_amd._lib.build_library(force=True))"
                       % (LIB_PATH, got, ABI_VERSION))
    L.ghr_forward_sizes.argtypes = [i32, i32, i32, i32, ctypes.POINTER(ctypes.c_size_t),
                                    ctypes.POINTER(ctypes.c_size_t)]
    L.ghr_binning_size.argtypes = [u32, i32, i32, ctypes.POINTER(ctypes.c_size_t)]
    L.ghr_forward_stage1.argtypes = [vp, ctypes.POINTER(ViewArgs), vp, vp, vp, vp]
    L.ghr_forward_stage2.argtypes = [vp, ctypes.POINTER(ViewArgs), u32, vp, vp, vp, vp, vp]
    L.ghr_backward.argtypes = [vp, ctypes.POINTER(ViewArgs), u32] + [vp] * 14 + [i32]
    L.ghr_backward_ex.argtypes = [vp, ctypes.POINTER(ViewArgs), u32] + [vp] * 14 + [i32, vp]
    L.ghr_mark_visible.argtypes = [vp, i32, vp, vp, vp, vp]
    L.ghr_set_profile_events.argtypes = [vp, vp, vp, vp]
    L.ghr_set_deterministic.argtypes = [i32]
    L.ghr_selftest_wave.argtypes = [vp, vp, vp]
    L.ghr_selftest_math.argtypes = [vp, i32, vp, vp]
    L.ghr_model_forward_stage1.argtypes = [vp, ctypes.POINTER(ModelArgs), vp, vp, vp, vp, vp]
    L.ghr_loss_sums_floats.argtypes = [i32, i32]
    L.ghr_loss_sums_floats.restype = ctypes.c_size_t
    L.ghr_loss_forward.argtypes = [vp, ctypes.POINTER(LossArgs), vp, vp, vp]
    L.ghr_loss_gt_stats.argtypes = [vp, ctypes.POINTER(LossArgs), vp]
    L.ghr_loss_backward.argtypes = [vp, ctypes.POINTER(LossArgs)] + [vp] * 9
    L.ghr_view_step.argtypes = [vp, ctypes.POINTER(ViewStepArgs)]
    L.ghr_adam_step.argtypes = [vp, ctypes.c_int64, vp, vp, vp, vp, vp, i32, ctypes.POINTER(ctypes.c_int64),
                                ctypes.POINTER(ctypes.c_float), ctypes.c_double, ctypes.c_double, f32, i32, i32, u32]
    L.ghr_adam_step_range.argtypes = [vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, vp, vp, vp, vp, vp, i32,
                                      ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_float), ctypes.c_double,
                                      ctypes.c_double, f32, i32, i32, i32, u32]
    L.ghr_adam_step_range_to.argtypes = [vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64] + [vp] * 9 + [
        i32, i32, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_float), ctypes.c_double, ctypes.c_double, f32, i32, u32]
    L.ghr_model_backward.argtypes = [vp, ctypes.POINTER(ModelArgs), u32] + [vp] * 15 + [i32, vp, i32]
    L.ghr_model_forward_segment.argtypes = [vp, ctypes.POINTER(ModelArgs), i32, i32, vp, vp, vp, vp]
    L.ghr_model_forward_finish.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp]
    L.ghr_render_backward.argtypes = [vp, i32, i32, i32, u32] + [vp] * 6 + [i32]
    L.ghr_model_backward_segment.argtypes = [vp, ctypes.POINTER(ModelArgs), i32] + [vp] * 13 + [i32, vp, u32, vp, u32]
    L.ghr_camera_slots.argtypes = [i32]
    L.ghr_camera_grad_fold.argtypes = [vp, vp, i32, vp, vp, vp]
    L.ghr_sh_grad_from_views.argtypes = [vp, i32, i32, i32, vp, i32, vp, ctypes.c_int64, vp, ctypes.c_int64, vp, vp, i32, vp,
                                         ctypes.c_int64]
    L.ghr_adam_relay_rows.argtypes = [vp, i32, vp, ctypes.c_int64, ctypes.c_int64] + [vp] * 10
    L.ghr_adam_fused_finish.argtypes = [vp, vp]
    L.ghr_adam_nan_scan.argtypes = [vp, vp, ctypes.c_int64, vp]
    L.ghr_strand_build.argtypes = [vp, i32, i32, vp, vp, f32, vp, vp, vp]
    L.ghr_strand_build_backward.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp]
    L.ghr_strand_build_backward_ex.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.ghr_knn_workspace_size.argtypes = [ctypes.c_int64, ctypes.POINTER(ctypes.c_size_t)]
    L.ghr_knn_keys.argtypes = [vp, ctypes.c_int64, vp, vp, vp]
    L.ghr_knn_mean_dist2.argtypes = [vp, ctypes.c_int64, vp, vp, vp, vp]
    L.ghr_camera_compose.argtypes = [vp, i32, i32, i32, i32, vp, i32, vp, i32, vp, i32]
    L.ghr_camera_compose_backward.argtypes = [vp, i32, i32, i32, i32, vp, i32, vp, i32] + [vp] * 6 + [vp, i32, vp, i32]
    L.ghr_camera_adam_step.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, f32, f32, f32, ctypes.c_double, ctypes.c_double,
                                       f32, i32]
    L.ghr_view_step_camera.argtypes = [vp, ctypes.POINTER(ViewStepArgs), ctypes.POINTER(ViewCameraArgs)]
    L.ghr_camera_pack_row_message.argtypes = [vp, i32, i32, vp, i32, vp, vp]
    L.ghr_camera_merge_ranks.argtypes = [vp, i32, i32, i32, vp, vp, i32, vp]
    L.ghr_eval_scratch_floats.argtypes = [i32, i32]
    L.ghr_eval_metrics.argtypes = [vp, ctypes.POINTER(EvalArgs), vp, vp]
    L.ghr_eval_products.argtypes = [vp, i32, i32, vp, vp, vp]
    L.ghr_orient_dog_scratch_bytes.argtypes = [i32, i32]
    L.ghr_orient_dog.argtypes = [vp, i32, i32, i32, i32, vp, i32, vp, i32, vp, vp, vp]
    L.ghr_orient_bank_floats.argtypes = [i32, i32]
    L.ghr_orient_gabor.argtypes = [vp, i32, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, i32]
    L.ghr_resample_scratch_bytes.argtypes = [i32] * 5
    L.ghr_resample_u8.argtypes = [vp, i32, i32, i32, vp, i32, i32, vp, vp, vp, i32, vp, vp, i32, vp]
    L.ghr_gt_assemble.argtypes = [vp, i32, i32] + [vp] * 5 + [i32, i32, vp, vp, i32, i32, i32] + [vp] * 4
    L.ghr_gt_resize_variance.argtypes = [vp, i32, i32, vp, i32, i32, i32, vp]
    L.ghr_gt_from_render.argtypes = [vp, i32, i32, vp, vp, i32, i32, vp, vp, vp, vp]
    L.ghr_strand_points_build.argtypes = [vp, i32, i32, vp, f32, vp, vp, vp, vp]
    L.ghr_strand_points_build_backward.argtypes = [vp, i32, i32] + [vp] * 6
    L.ghr_strand_rows_expand.argtypes = [vp, i32, i32, i32, vp, vp]
    L.ghr_strand_rows_reduce.argtypes = [vp, i32, i32, i32, vp, vp]
    L.ghr_latent_loss_sums_floats.argtypes = [i32, i32]
    L.ghr_latent_loss_forward.argtypes = [vp, ctypes.POINTER(LatentLossArgs), vp, vp]
    L.ghr_latent_loss_backward.argtypes = [vp, ctypes.POINTER(LatentLossArgs), vp, vp, vp]
    L.ghr_model_forward_segment_shared.argtypes = [vp, ctypes.POINTER(ModelArgs), ctypes.POINTER(SharedFeatures), i32, i32,
                                                   vp, vp, vp, vp]
    L.ghr_model_backward_segment_shared.argtypes = [vp, ctypes.POINTER(ModelArgs), ctypes.POINTER(SharedFeatures), i32] + \
        [vp] * 13 + [vp, u32, vp, u32, vp]
    L.ghr_shared_sh_fold.argtypes = [vp, ctypes.POINTER(SharedFeatures), i32, i32] + [vp] * 6
    L.ghr_mesh_grid_sizes.argtypes = [i32, vp, i32, vp, i32, ctypes.POINTER(MeshGrid)]
    L.ghr_mesh_grid_build.argtypes = [i32, vp, i32, vp, i32, vp, ctypes.c_size_t]
    L.ghr_mesh_contains.argtypes = [vp, ctypes.POINTER(MeshGrid), vp, ctypes.c_int64, vp, vp, vp]
    L.ghr_gaussian_probe_outside.argtypes = [vp, ctypes.POINTER(MeshGrid), vp, ctypes.c_int64, vp, vp, vp, i32, vp]
    L.ghr_mesh_tris_sizes.argtypes = [i32, vp, i32, vp, ctypes.POINTER(MeshTris)]
    L.ghr_mesh_tris_build.argtypes = [i32, vp, i32, vp, vp, ctypes.c_size_t]
    L.ghr_mesh_closest.argtypes = [vp, ctypes.POINTER(MeshTris), vp, ctypes.c_int64] + [vp] * 6
    L.ghr_mesh_distance_backward.argtypes = [vp, ctypes.c_int64] + [vp] * 6
    L.ghr_vis_sizes.argtypes = [i32, i32, i32, i32, ctypes.POINTER(ctypes.c_size_t)]
    L.ghr_vis_view.argtypes = [vp, i32, vp, i32, vp, ctypes.POINTER(ctypes.c_float * 12), f32, i32, i32] + [vp] * 7
    L.ghr_vis_head_mask.argtypes = [vp, i32, i32, vp, vp, vp]
    L.ghr_strandview_sizes.argtypes = [i32, i32, i32, i32, ctypes.POINTER(ctypes.c_size_t)]
    L.ghr_strandview_face_depth.argtypes = [vp, i32, vp, i32, vp, ctypes.POINTER(ctypes.c_float * 12), f32, i32, i32, vp, vp]
    L.ghr_strandview_raster.argtypes = [vp, i32, i32, vp, ctypes.POINTER(ctypes.c_float * 12), f32, i32, i32, f32, f32] + [vp] * 7
    L.ghr_strandview_shade.argtypes = [vp, i32, i32, vp, i32, vp, i32, vp, i32, i32, vp, vp, i32,
                                       ctypes.POINTER(StrandViewShading), vp, vp]
    L.ghr_strandview_resolve.argtypes = [vp, i32, i32, i32, vp, vp]
    L.ghr_strandview_opacity.argtypes = [vp, i32, i32, vp, ctypes.POINTER(ctypes.c_float * 12), f32, i32, i32, f32, f32, vp,
                                         ctypes.c_size_t, vp, vp]
    L.ghr_strandview_shade_shadowed.argtypes = [vp, i32, i32, vp, i32, vp, i32, vp, i32, i32, vp, vp, vp, i32,
                                                ctypes.POINTER(StrandViewShading), vp, ctypes.POINTER(StrandViewShadow), vp]
    L.ghr_strandview_capture.argtypes = [vp, i32, i32, vp, ctypes.POINTER(ctypes.c_float * 12), f32, i32, i32, i32, i32, vp, vp, vp, f32,
                                         vp, vp, vp, vp]
    L.ghr_sds_local.argtypes = [vp, i32, i32, i32, vp, vp, i32, vp, f32, vp, vp]
    L.ghr_sds_local_backward.argtypes = [vp, i32, i32, i32, vp, i32, vp, vp, f32, vp, vp, vp]
    L.ghr_sds_texture.argtypes = [vp, i32, i32, i32, i32] + [vp] * 13
    L.ghr_sds_texture_backward.argtypes = [vp, i32, i32, i32, i32] + [vp] * 13
    L.ghr_nn_workspace_size.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_size_t)]
    L.ghr_nn_search.argtypes = [vp, ctypes.c_int64, vp, vp, vp, ctypes.c_int64, vp, vp, vp, i32, vp, vp, vp]
    L.ghr_chamfer_point.argtypes = [vp, ctypes.c_int64, ctypes.c_int64, vp, vp, vp, i32, vp, vp, vp]
    L.ghr_chamfer_point_backward.argtypes = [vp, ctypes.c_int64, ctypes.c_int64, i32] + [vp] * 8 + [i32] + [vp] * 5
    L.ghr_cmp_over_white.argtypes = [vp, ctypes.c_int64, vp, vp]
    L.ghr_cmp_strip.argtypes = [vp, i32, i32, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp]
    L.ghr_ts_fetch.argtypes = [vp, i32, i32, i32, i32] + [vp] * 7
    L.ghr_ts_fetch_backward.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    L.ghr_ts_world.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, f32, vp, vp]
    L.ghr_ts_world_backward.argtypes = [vp, i32, i32, i32, vp, vp, f32, vp, vp, vp]
    L.ghr_guides_blend.argtypes = [vp, i32, i32, i32, i32] + [vp] * 13
    L.ghr_guides_blend_backward.argtypes = [vp, i32, i32, i32, i32] + [vp] * 13
    L.ghr_field_workspace_size.argtypes = [ctypes.c_int64, ctypes.POINTER(ctypes.c_size_t)]
    L.ghr_field_build.argtypes = [vp, ctypes.c_int64] + [vp] * 6
    L.ghr_field_query.argtypes = [vp, ctypes.c_int64, vp, ctypes.c_int64, vp, vp, vp, f32, vp, vp, vp, vp]
    L.ghr_field_trace.argtypes = [vp, ctypes.c_int64, vp, ctypes.c_int64, vp, vp, vp, i32, f32, f32, f32, f32, i32, vp, vp, vp]
    L.ghr_strands_resample.argtypes = [vp, ctypes.c_int64, i32, i32, vp, vp, vp]
    L.ghr_field_trace_guarded.argtypes = [vp, ctypes.c_int64, vp, ctypes.POINTER(MeshTris), vp, ctypes.POINTER(MeshGrid), vp, ctypes.c_int64,
                                          vp, vp, vp, i32, f32, f32, f32, f32, i32, f32, vp, vp, vp, vp, vp]
    L.ghr_shape_neighbours.argtypes = [vp, i32, vp, f32, vp]
    L.ghr_shape_forward.argtypes = [vp, i32, i32, vp, vp, vp, ctypes.c_int64, vp, vp]
    L.ghr_shape_backward.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, ctypes.c_int64, vp, vp]
    L.ghr_upsample_neighbours.argtypes = [vp, i32, vp, i32, vp, f32, vp, vp]
    L.ghr_upsample_blend.argtypes = [vp, i32, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp, f32, f32, i32, vp, vp, vp, vp]
    L.ghr_ws_inspect.argtypes = [i32, i32, i32, i32, u32, vp, vp, vp, ctypes.POINTER(WsView)]
    for name in EXPORTS:
        fn = getattr(L, name)
        if name not in ("ghr_last_error", "ghr_eval_scratch_floats", "ghr_orient_dog_scratch_bytes", "ghr_orient_bank_floats",
                        "ghr_resample_scratch_bytes", "ghr_latent_loss_sums_floats"):
            fn.restype = ctypes.c_int
    for name in ("ghr_eval_scratch_floats", "ghr_orient_dog_scratch_bytes", "ghr_orient_bank_floats", "ghr_resample_scratch_bytes",
                 "ghr_latent_loss_sums_floats"):
        getattr(L, name).restype = ctypes.c_size_t
    _lib = L
    return L


def check(rc: int) -> None:
    if rc != GHR_OK:
        msg = lib().ghr_last_error().decode("utf-8", "replace")
        if rc == GHR_E_NOCOLORS:
            raise RuntimeError(msg)  # same text as the reference's std::runtime_error (rasterizer_impl.cu:246)
        raise GhrError("libghr_hip: %s (code %d)" % (msg, rc))


def forward_sizes(P: int, W: int, H: int, mode_b: bool):
    g, i = ctypes.c_size_t(0), ctypes.c_size_t(0)
    check(lib().ghr_forward_sizes(P, W, H, int(mode_b), ctypes.byref(g), ctypes.byref(i)))
    return int(g.value), int(i.value)


def knn_workspace_size(P: int) -> int:
    b = ctypes.c_size_t(0)
    check(lib().ghr_knn_workspace_size(P, ctypes.byref(b)))
    return int(b.value)


def nn_workspace_size(Px: int, Py: int) -> int:
    b = ctypes.c_size_t(0)
    check(lib().ghr_nn_workspace_size(Px, Py, ctypes.byref(b)))
    return int(b.value)


def field_workspace_size(P: int) -> int:
    b = ctypes.c_size_t(0)
    check(lib().ghr_field_workspace_size(P, ctypes.byref(b)))
    return int(b.value)


def binning_size(R: int, W: int, H: int) -> int:
    b = ctypes.c_size_t(0)
    check(lib().ghr_binning_size(R, W, H, ctypes.byref(b)))
    return int(b.value)
