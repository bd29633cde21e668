/*
 * ghr.h -- C ABI of libghr_hip.so, the MI355X (gfx950) strand-aligned Gaussian tile rasterizer.
 *
 * Drop-in boundary for the reference's native module `diff_gaussian_rasterization._C`
 * (ext/diff_gaussian_rasterization_hair/ext.cpp:15-19; signatures rasterize_points.h:18-69):
 *
 *   _C.rasterize_gaussians           (rasterize_points.cu:35-123)   -> ghr_forward_stage1 + ghr_forward_stage2
 *   _C.rasterize_gaussians_backward  (rasterize_points.cu:125-206)  -> ghr_backward
 *   _C.mark_visible                  (rasterize_points.cu:208-227)  -> ghr_mark_visible
 *   CudaRasterizer::required<State>  (rasterizer_impl.h:67-73)      -> ghr_forward_sizes / ghr_binning_size
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no torch / C++ types.  All pointers are DEVICE pointers unless the
 *    name ends in `_host`.  `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *  - Nullable pointers select the mode exactly like the reference's empty-tensor => nullptr convention
 *    (diff_gaussian_rasterization/__init__.py:210-222; forward.cu:215,228):
 *        conic_precomp != NULL            : "pipeline mode" (A): conic supplied by the caller (what render() does)
 *        conic_precomp == NULL            : "kernel-geometry mode" (B): cov3D_precomp, or scales+rotations, in-kernel
 *  - Matrices are the reference's: 16 floats, element [4*c + r] multiplies component c into output r
 *    (auxiliary.h:58-77), i.e. world_view_transform / full_proj_transform of src/scene/cameras.py:72-80.
 *  - Feature channels: `colors` is [P, C] row-major, C == GHR_NUM_CHANNELS (config.h:15).  Like the reference
 *    (rasterizer_impl.cu:244-247) the library refuses to run without precomputed colors.
 *  - Every function returns 0 on success, a negative GHR_E_* code on failure; ghr_last_error() returns a
 *    thread-local description.  No exceptions cross the ABI.  Kernels never trap: a Gaussian that fails the near
 *    test is culled even when `prefiltered` is set (the reference __trap()s, auxiliary.h:154-162).
 *  - Ownership: the caller owns every buffer (workspaces included) and must keep geom/img/bin workspaces alive
 *    and unmodified between forward and backward of the same view (the reference does this with
 *    ctx.save_for_backward, __init__.py:102).  The library allocates nothing and never synchronises, except that
 *    `debug != 0` makes each call hipStreamSynchronize + check errors before returning (auxiliary.h:166-173).
 */
#ifndef GHR_H
#define GHR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GHR_ABI_VERSION 20
#define GHR_NUM_CHANNELS 10 /* R:cuda_rasterizer/config.h:15 */
#define GHR_TILE 16         /* R:cuda_rasterizer/config.h:16-17 (BLOCK_X, BLOCK_Y) */
#define GHR_ADAM_STATE 18  /* ints of the fused Adam's device state */
#define GHR_GRAD_STRIDE 16  /* floats per Gaussian-tile instance in the gradient scratch of ghr_backward */
#define GHR_CAM_PARTIALS 32 /* rows of the camera-gradient partial table (ghr_model_args.cam_partial) */
#define GHR_CAM_GRADS 37    /* floats ghr_camera_grad_fold writes: d view[16] | d proj[16] | d camera_center[3] | d tanfov[2] */
#define GHR_STRAND_MAX_SEG 2048 /* longest strand (segments) ghr_strand_build takes */

#define GHR_OK 0
#define GHR_E_INVALID (-1)  /* bad argument (NULL where required, C != GHR_NUM_CHANNELS, ...) */
#define GHR_E_NOCOLORS (-2) /* "For non-RGB, provide precomputed Gaussian colors!" */
#define GHR_E_HIP (-3)      /* a HIP runtime call or kernel launch failed */

/* Inputs shared by forward and backward of one view (argument lists of rasterize_points.h:18-69). */
typedef struct ghr_view_args {
    int32_t P;                  /* number of Gaussians handed to the op (after the Python-side mask) */
    int32_t W, H;               /* image_width, image_height */
    int32_t C;                  /* feature channels; must be GHR_NUM_CHANNELS */
    const float* background;    /* [C] */
    const float* means3D;       /* [P,3] */
    const float* colors;        /* [P,C] colors_precomp */
    const float* opacities;     /* [P] (tensor [P,1]) */
    const float* scales;        /* [P,3] or NULL */
    const float* rotations;     /* [P,4] (r,x,y,z), NOT normalised in-kernel (forward.cu:127), or NULL */
    const float* cov3D_precomp; /* [P,6] or NULL */
    const float* conic_precomp; /* [P,3] (a, b, c) or NULL */
    const float* viewmatrix;    /* [16] */
    const float* projmatrix;    /* [16] */
    float scale_modifier;
    float tan_fovx, tan_fovy;
    int32_t prefiltered;        /* accepted for API parity; culling is always silent */
    int32_t debug;              /* != 0: synchronise + check after the call */
    /* ABI 17 (ghr_forward_stage1 only).  != 0: img_ws is the image workspace of an EARLIER forward pass of the same W x H whose
     * stage 1 AND stage 2 ran (P > 0), ordered before this call, untouched since: its per-tile counters are back at zero and
     * stage 1 skips its zero-fill (the promise of ghr_model_args.img_ws_recycled, for the rasterizer op itself).  0: any buffer. */
    int32_t img_ws_recycled;
} ghr_view_args;

const char* ghr_last_error(void);
int ghr_abi_version(void);

/* Workspace sizes (host only).  geom: per-Gaussian state (packed 64-B render records, depths, tile rects,
 * [mode B: cov3D]); img: per-pixel final_T / n_contrib + per-tile counts, list offsets and the largest n_contrib of
 * each 4x4-pixel cell. */
int ghr_forward_sizes(int32_t P, int32_t W, int32_t H, int32_t mode_b, size_t* geom_bytes, size_t* img_bytes);
/* bin: per-instance (Gaussian x tile) sort keys + the sorted point list + (ABI 12) the forward pass's cell masks:
 * per 64 list positions of a tile and per 4x4-pixel cell, which entries can touch the cell (2 B per instance + 128 B
 * per tile, hence W and H). */
int ghr_binning_size(uint32_t R, int32_t W, int32_t H, size_t* bin_bytes);

/* Stage 1 = preprocess (K1) + per-tile instance count + tile offset scan.  Writes radii[P] (int32, 0 = culled)
 * and asynchronously copies num_rendered R to *R_host (pinned host memory; valid once `stream` reaches the
 * point after this call, e.g. after hipStreamSynchronize -- the reference blocks on the same 4 bytes,
 * rasterizer_impl.cu:284-285). */
int ghr_forward_stage1(void* stream, const ghr_view_args* a, void* geom_ws, void* img_ws, int32_t* radii,
                       uint32_t* R_host);

/* Stage 2 = instance scatter + per-tile depth sort (== the reference's global (tile|depth) stable radix sort,
 * rasterizer_impl.cu:293-321) + front-to-back compositing (K7).  out_color is [C,H,W].
 * R is the CAPACITY (in instances) of bin_ws (ghr_binning_size(R)) and fixes its layout: it must be >= the instance
 * count stage 1 reported for the result to be valid, and the same value must be passed to the backward call.  A caller
 * may therefore launch stage 2 speculatively with a capacity guessed from the previous frame BEFORE reading *R_host
 * (no GPU bubble behind the host round trip) and relaunch it only if the true count turned out larger: instances
 * beyond the capacity are dropped without touching memory outside bin_ws.  Stage 2 may be replayed.
 * grad_scratch (ABI 12, may be NULL): the scratch the backward call over this state will be given (>= R lines).  Its
 * lines are then zeroed here, by the render kernel as its last act, so that the backward call can be told `prezeroed` (below). */
int ghr_forward_stage2(void* stream, const ghr_view_args* a, uint32_t R, void* geom_ws, void* img_ws, void* bin_ws,
                       float* out_color, float* grad_scratch);

/* Backward (K8 + K9 + K10).  dL_dpix is [C,H,W].  R: the capacity stage 2 was run with (layout of bin_ws).
 * grad_scratch: GHR_GRAD_STRIDE floats (one 64-B gradient line) per Gaussian-tile instance actually reported by stage 1
 * (may be NULL when that count is 0): every line is zero-filled and accumulated by K8 and the lines of a Gaussian are
 * summed in a fixed order -- no cross-tile float atomics.
 * prezeroed (ABI 13; the library keeps NO record of buffers -- it is stateless between calls): 0 = grad_scratch is
 * uninitialised, K8 zero-fills it.  != 0 = the CALLER guarantees that grad_scratch is exactly as
 * ghr_forward_stage2(..., bin_ws, ..., grad_scratch) of THIS state left it: same scratch, zeroed by that stage 2,
 * and nothing written to it since -- in particular no other backward call (of this or any other state).  Sharing
 * rule: when several states share one scratch buffer, at most the state whose stage 2 was the LAST to be handed the
 * buffer may be backwarded with prezeroed != 0, and only as the first backward that touches the buffer after it; every
 * other backward over the shared buffer passes 0.  A second backward over the same state passes 0.  A caller that launched stage 2
 * speculatively and has not read the count yet passes R lines instead: no line index >= R is ever touched, so a count
 * above the capacity (whose results the caller must discard and recompute) cannot write outside the buffer.
 * Outputs (all fully written, no pre-zeroing needed), shapes of rasterize_points.cu:160-168:
 *   dL_dmeans2D [P,3] (z = 0), dL_dconic [P,2,2] ([0][0], [0][1] = HALF of d/db as in backward.cu:554, [1][1]),
 *   dL_dopacity [P], dL_dcolors [P,C], dL_dmeans3D [P,3], dL_dcov3D [P,6], dL_dscales [P,3], dL_drotations [P,4]. */
int ghr_backward(void* stream, const ghr_view_args* a, uint32_t R, const int32_t* radii, const void* geom_ws,
                 const void* img_ws, const void* bin_ws, const float* dL_dpix, float* grad_scratch,
                 float* dL_dmeans2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolors, float* dL_dmeans3D,
                 float* dL_dcov3D, float* dL_dscales, float* dL_drotations, int32_t prezeroed);
/* ABI 14: ghr_backward with one more (optional) output, dL_dconic3 [P,3] = (dL_dconic[0][0], 2 * dL_dconic[0][1],
 * dL_dconic[1][1]): the gradient w.r.t. conic_precomp as the reference's Python wrapper hands it to autograd
 * (diff_gaussian_rasterization/__init__.py:149-153 restacks dL_dconic with three slices, a doubling and a stack: two more
 * kernels per backward pass of the drop-in op).  NULL: exactly ghr_backward. */
int ghr_backward_ex(void* stream, const ghr_view_args* a, uint32_t R, const int32_t* radii, const void* geom_ws,
                    const void* img_ws, const void* bin_ws, const float* dL_dpix, float* grad_scratch,
                    float* dL_dmeans2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolors, float* dL_dmeans3D,
                    float* dL_dcov3D, float* dL_dscales, float* dL_drotations, int32_t prezeroed, float* dL_dconic3);

/* ---- fused model path ------------------------------------------------------------------------
 * One kernel computes, from the RAW parameters of the reference's GaussianModel, everything render() would build with
 * ~60 PyTorch kernels before calling the rasterizer (src/gaussian_renderer/__init__.py:29-83):
 *   activations (gaussian_model.py:107-141), get_conic (:230-315), get_mean_2d / get_depths (:317-342),
 *   get_direction_2d (:344-393), eval_sh + clamp (sh_utils.py:57-112), the 10-channel feature vector, filter_points
 *   (:143-228) -- and feeds K1's cull / radius / tile rect directly.  ghr_model_backward runs K8 and then maps the
 *   packed per-Gaussian gradients to raw-parameter gradients (what autograd does for that graph), in one pass.
 * Semantics are the PYTHON pipeline's (torch.clamp / normalize / clamp_min gradients, conic eps), tolerance 1e-4. */
struct ghr_adam_fuse;
typedef struct ghr_model_args {
    int32_t P, W, H;
    int32_t sh_degree;            /* active SH degree 0..3 */
    int32_t sh_coeffs;            /* K = (max_sh_degree + 1)^2: 1, 4, 9 or 16 (anything else: GHR_E_INVALID) */
    const float* xyz;             /* [P,3]   _xyz */
    const float* log_scales;      /* [P,3]   _scaling (exp activation) */
    const float* rotations;       /* [P,4]   _rotation, raw (normalised in-kernel like build_rotation) */
    const float* opacity_logit;   /* [P]     _opacity (sigmoid) */
    const float* label_logit;     /* [P]     _label (sigmoid) */
    const float* orient_conf_log; /* [P]     _orient_conf (exp) */
    const float* features_dc;     /* [P,1,3] */
    const float* features_rest;   /* [P,K-1,3] */
    const float* viewmatrix;      /* [16] */
    const float* projmatrix;      /* [16] */
    const float* campos;          /* [3] */
    const float* background;      /* [C] */
    float scale_modifier, tan_fovx, tan_fovy;
    float conic_eps;              /* 1e-12 (gaussian_model.py:312); strand stage 1e-7 (gaussian_model_strands.py:355) */
    int32_t debug;
    /* ---- explicit linear-space Gaussians: what render_hair() feeds the rasterizer in the strand stage
     * (src/gaussian_renderer/__init__.py:116-214).  mode 1: log_scales holds the scaling, opacity_logit / label_logit /
     * orient_conf_log the ACTIVATED values (NULL = the constant below), dir3d the strand direction whose normalised
     * projection normalize(dir) @ T is the 2D direction (NULL = zero direction: frozen head Gaussians).
     * row0: first workspace row of this segment (ghr_model_forward_segment); a multiple of 256. */
    int32_t mode;
    int32_t row0;
    const float* dir3d;           /* [P,3] or NULL */
    float const_opacity, const_label, const_conf;
    /* ABI 16.  != 0: img_ws is the image workspace of an EARLIER forward pass of the same W x H whose stage 1 AND stage 2 were
     * both launched, ordered before this call on the stream (or through events), and which nobody has written since.  Its
     * per-tile counters are then back at zero -- k_tile_scan turns the counts into append cursors starting at 0 and stage 2's
     * tile sort resets every cursor -- so stage 1 does not launch its zero-fill (one ~5-us launch per view).  0: any buffer.
     * A pass with P == 0 does NOT qualify (both stages return before touching the workspace).  With `debug` set the library
     * reads the counters back and fails with GHR_E_INVALID if any is non-zero; otherwise the promise is taken on trust. */
    int32_t img_ws_recycled;
    /* ---- ABI 17: trainable cameras.  The reference's projection graph is differentiable w.r.t. the camera
     * (src/scene/gaussian_model.py:258-266,279-294,332-335; src/gaussian_renderer/__init__.py:59), whose tensors are functions
     * of trainable pose / FoV residuals (src/scene/cameras.py:85-151) stepped by an optimizer of their own
     * (src/train_gaussians.py:45-60,183-196; on by default: src/arguments/__init__.py:61-62).
     * fovx_dev, fovy_dev (both or neither): DEVICE scalars FoVx, FoVy in radians.  Non-NULL: forward and backward kernels take
     * tan(FoV / 2) from there (and derive focal = dim / (2 tan) themselves) instead of tan_fovx / tan_fovy above, so a FoV that
     * changes every step never costs a device-to-host read; ghr_camera_grad_fold can then return dL/dFoV directly.
     * cam_partial (backward calls only; NULL = no camera gradients): table of GHR_CAM_PARTIALS rows of cam_slots floats.  The
     * segment's backward writes one column per 64 Gaussians -- columns cam_slot0 .. cam_slot0 + ghr_camera_slots(P) - 1, every
     * row of them -- and ghr_camera_grad_fold adds the columns up.  Several segments of one view share a table.
     * cam_only != 0: a frozen segment (render_hair()'s head Gaussians): its backward writes NOTHING but its camera columns (the
     * parameter-gradient and d_means2D pointers may be NULL).
     * detach_means2D != 0: the segment's NDC means are constants of the graph (render_hair() detaches the head's,
     * src/gaussian_renderer/__init__.py:136): no gradient flows through projmatrix for it. */
    const float* fovx_dev;
    const float* fovy_dev;
    float* cam_partial;
    int32_t cam_slot0, cam_slots;
    int32_t cam_only;
    int32_t detach_means2D;
    /* Per-iteration densification statistics of the stage-1 loop (src/train_gaussians.py:161-165,
     * src/scene/gaussian_model.py:739-741), folded into the backward call (all three non-NULL, or all NULL): for every Gaussian
     * of the segment the view sees (radii > 0)   xyz_gradient_accum += |d_means2D.xy|,   denom += 1,
     * max_radii2D = max(max_radii2D, radii).  All [P] floats (the reference's [P,1], [P,1], [P]).  Read-modify-write: calls that
     * share the arrays must be ordered (they are wherever they share the flat gradient buffer). */
    float* dens_grad_accum;
    float* dens_denom;
    float* dens_max_radii2D;
    /* optional with the three above: the view's image workspace.  The update then only happens if the instance count stage 1 left
     * there is within the capacity R the backward call is given -- a view rasterized speculatively with too small a capacity
     * (ghr_forward_stage2) has invalid gradients and is recomputed by the caller: its statistics must not be counted twice. */
    const void* dens_img_ws;
    /* != 0 with dens_img_ws (statistics pointers may be NULL): a view whose instance count exceeds the capacity R raises nan_flag
     * -- what every view of a step whose LAST backward carries adam_fuse must do (see ghr_adam_fuse). */
    int32_t overflow_raises_flag;
    /* ---- the optimizer update fused into this backward call (mode 0, the LAST backward of a single-rank gradient step): see
     * ghr_adam_fuse below.  NULL: gradients are stored / accumulated as documented. */
    const struct ghr_adam_fuse* adam_fuse;
    /* ---- ABI 19 (backward calls, mode 0 or 1; NULL = off): d_rgb [P,3], ASSIGNED: dL/d(rgb) of every Gaussian behind the colour
     * clamp (sh_utils.py:57-112 + clamp_min(.. + 0.5, 0), src/gaussian_renderer/__init__.py:58-63).  This view's gradient of the
     * SH coefficients is the outer product basis_k(dir) x d_rgb[c] -- 48 floats determined by 3 and by the view direction, which
     * any holder of xyz and the camera centre can recompute: ghr_sh_grad_from_views.  With d_rgb set, d_features_dc and
     * d_features_rest of the call may be NULL (nothing is stored for them); non-finite d_rgb raises nan_flag. */
    float* d_rgb;
} ghr_model_args;

/* Adam fused into the projection backward (src/scene/gaussian_model.py:431-444 stepped at src/train_gaussians.py:174-181).
 * The last view's backward of a step holds every parameter gradient of the step in registers -- its own terms plus what the
 * earlier views accumulated in the gradient buffers it is given with accumulate != 0 -- and the raw parameters too: with
 * adam_fuse set it applies ghr_adam_step's update there and stores NO gradients (the gradient buffers are left as they were:
 * 244 B per Gaussian neither written nor read back by a separate optimizer pass).
 * Two sets of flat buffers of n floats each: the raw-parameter pointers of ghr_model_args must point into p_in (all eight
 * arrays; together they must tile it: the reference's eight parameter groups), m_in / v_in are the moments at the same offsets;
 * the updated p, m, v go to p_out / m_out / v_out at the same offsets, and the caller swaps the roles of the two sets for the
 * next step.  The skip-on-non-finite rule is global: nan_flag of the backward call must be `flag`; after the projection kernel
 * the call launches a second kernel that, when *flag != 0, copies in -> out (the update is undone: 732 B per Gaussian, a rare
 * event) and otherwise advances state[0]; it clears *flag_next, never *flag -- alternate two words between steps (every view of
 * a step raises the same word).  With dens_img_ws set, a view whose instance count exceeds the capacity R raises the flag as
 * well (a speculative forward pass that overflowed must not reach the parameters).
 * state / n_groups / group_end_host / lr_host / beta1 / beta2 / eps: as ghr_adam_step (no group may be marked to sit out). */
typedef struct ghr_adam_fuse {
    int64_t n;
    const float* p_in;
    const float* m_in;
    const float* v_in;
    float* p_out;
    float* m_out;
    float* v_out;
    int32_t* state;
    int32_t* flag;
    int32_t* flag_next;
    int32_t n_groups;
    const int64_t* group_end_host;
    const float* lr_host;
    double beta1, beta2;
    float eps;
} ghr_adam_fuse;
/* ABI 19: a strand segment (mode 1, render_hair(): src/train_strands.py:98-160) may carry the update too, as the step's single
 * view (accumulate == 0).  Of its raw values only features_dc / features_rest are parameters of the optimizer's flat buffer
 * (the other groups there -- strand directions, confidence: gaussian_model_strands.py:578-589 -- receive their gradients through
 * autograd, after this call): the kernel updates those two arrays into the `out` set, stores every other gradient as usual
 * (d_features_dc / d_features_rest may be NULL) and launches NO finish kernel.  The caller then (1) adds the non-finite mark
 * of the late gradients to *flag (ghr_adam_nan_scan with state = flag - 1), (2) brings the remaining ranges of the `out` set up
 * to date (ghr_adam_step_range_to with flag, ABI 20; or: copy in -> out, ghr_adam_step_range on the `out` buffers with
 * nan_guard = 2 and state[1] = *flag), (3) calls
 * ghr_adam_fused_finish: the same k_adam_fused_finish as above (out := in for everything when the flag is up, step counter). */
int ghr_adam_fused_finish(void* stream, const ghr_adam_fuse* adam_fuse);

/* Stage 1 of the fused path: replaces ghr_forward_stage1 (then call ghr_forward_stage2 with a ghr_view_args that
 * carries P, W, H, C and background; every other field may be NULL).  means2D_out [P,3] (NDC) may be NULL. */
int ghr_model_forward_stage1(void* stream, const ghr_model_args* m, void* geom_ws, void* img_ws, int32_t* radii,
                             float* means2D_out, uint32_t* R_host);

/* Backward of the fused path.  Outputs: d_means2D [P,3] (always assigned), d_xyz [P,3], d_log_scales [P,3],
 * d_rotations [P,4], d_opacity_logit [P], d_label_logit [P], d_orient_conf_log [P], d_features_dc [P,1,3],
 * d_features_rest [P,K-1,3].  accumulate == 0: every parameter-gradient element is assigned; != 0: added to what the
 * buffers hold (they may be the optimizer's own flat gradient buffer: no separate accumulation pass).
 * nan_flag (nullable, device int): set to 1 when any stored parameter-gradient value is NaN (the stage-1 loop's NaN
 * guard, src/train_gaussians.py:174-181, without a scan over the gradients). */
/* ---- segmented form (strand stage): several ghr_model_args segments, each covering rows row0 .. row0+P-1 of ONE
 * rasterizer state of rows_total rows (workspaces sized with ghr_forward_sizes(rows_total, ...); radii / means2D_out
 * [rows_total(,3)]).  Call ghr_model_forward_segment for every segment (first != 0 on the first), then
 * ghr_model_forward_finish (tile scan + *R_host), then ghr_forward_stage2 with P = rows_total as usual.  Rows between
 * the end of a segment and the next multiple of 256 are culled padding.
 * radii / means2D_out (and d_means2D below) are the caller's per-row arrays and are indexed by workspace row, row0 + i: a call
 * touches the rows of ITS segment only (plus, in radii, the zero-fill of the padding rows behind it), so a caller that wants
 * its outputs without the padding -- the reference's [head rows, strand rows] indexing -- may hand a later segment base
 * pointers displaced by the padding in front of it (round 6: the Python side does; the three arrays are then written compact,
 * earlier segments first).  The same displaced `radii` must be passed to that segment's ghr_model_backward_segment. */
int ghr_model_forward_segment(void* stream, const ghr_model_args* m, int32_t rows_total, int32_t first, void* geom_ws,
                              void* img_ws, int32_t* radii, float* means2D_out);
int ghr_model_forward_finish(void* stream, int32_t rows_total, int32_t W, int32_t H, int32_t debug, void* geom_ws,
                             void* img_ws, uint32_t* R_host);
/* Backward in two steps: K8 over the whole state (rows_total rows), then the per-Gaussian chain for the segments that
 * need gradients.  d_means2D is [rows_total,3]; the parameter gradients are per segment ([P,...]); in mode 1
 * d_log_scales / d_opacity_logit / d_label_logit / d_orient_conf_log are the gradients of the linear quantities and,
 * like d_dir3d, may be NULL.  grad_rows: number of lines in grad_scratch (0: R), see ghr_backward.  bin_ws / R: the binning
 * workspace and the capacity ghr_forward_stage2 ran with (ABI 12: the gradient lines lie in tile-list order, the per-Gaussian
 * chain finds a Gaussian's lines through the index the tile sort left in bin_ws). */
int ghr_render_backward(void* stream, int32_t rows_total, int32_t W, int32_t H, uint32_t R, const float* background,
                        const void* geom_ws, const void* img_ws, const void* bin_ws, const float* dL_dpix,
                        float* grad_scratch, int32_t prezeroed /* see ghr_backward */);
int ghr_model_backward_segment(void* stream, const ghr_model_args* m, int32_t rows_total, const int32_t* radii,
                               const void* geom_ws, const float* grad_scratch, float* d_means2D, float* d_xyz,
                               float* d_log_scales, float* d_rotations, float* d_opacity_logit, float* d_label_logit,
                               float* d_orient_conf_log, float* d_features_dc, float* d_features_rest, float* d_dir3d,
                               int32_t accumulate, int32_t* nan_flag, uint32_t grad_rows, const void* bin_ws,
                               uint32_t R);

/* ABI 17.  Columns of ghr_model_args.cam_partial a segment of P Gaussians fills (host only). */
int32_t ghr_camera_slots(int32_t P);
/* Adds the cam_slots columns of a partial table up (fixed order, double accumulation) into d_cam[GHR_CAM_GRADS]:
 * dL/d world_view_transform [4,4] (column 3 zero: never read) | dL/d full_proj_transform [4,4] (column 2 zero: the NDC z carries
 * no gradient) | dL/d camera_center [3] | dL/d {tan(FoVx / 2), tan(FoVy / 2)} -- the gradients autograd hands the camera tensors
 * in the reference's render() (torch.clamp's tensor bounds 1.3 tan included).  fovx_dev / fovy_dev (both or neither; the
 * pointers of ghr_model_args): the last two entries are dL/dFoVx, dL/dFoVy instead (x (1 + tan^2(FoV / 2)) / 2). */
int ghr_camera_grad_fold(void* stream, const float* cam_partial, int32_t cam_slots, float* d_cam, const float* fovx_dev,
                         const float* fovy_dev);

/* ABI 19.  SH-coefficient gradients from per-view factors: the data-parallel step's gradient message (an all-reduce
 * of 244 B per Gaussian over xGMI) is 79 % SH gradients, and those are rank-1 per view.  Ranks all-gather d_rgb (12 B per Gaussian
 * and view, ghr_model_args.d_rgb) and their camera centres instead, and every rank calls this:
 *   d_features_dc[i][c]      = sum_v basis_0 d_rgb[v][i][c]
 *   d_features_rest[i][k][c] = sum_v basis_{k+1}(normalize(xyz_i - campos_v)) d_rgb[v][i][c]
 * (both ASSIGNED, or added to what the arrays hold with accumulate != 0), views in list order, the products and the order of the sum being those of one rank accumulating the same views
 * (ghr_model_backward with accumulate != 0): that run's bits.  campos and g_views are DEVICE arrays: view v's camera centre is
 * the 3 floats at campos + v * campos_stride, its [P,3] table starts at g_views + v * view_stride (strides in floats; both may
 * point into the same gathered rows).  sh_degree = the active degree (bands above it get zeros), sh_coeffs = K.
 * nan_flag (optional) with flag_offset: the float at g_views + v * view_stride + flag_offset of every view is that view's
 * owner's "my gradients are not finite" mark (non-zero = raised); any raised mark raises *nan_flag -- the ranks' skip-the-step
 * flags (ghr_adam_step, nan_guard = 2) travel inside the gathered rows instead of through a collective of their own. */
int ghr_sh_grad_from_views(void* stream, int32_t P, int32_t sh_degree, int32_t sh_coeffs, const float* xyz, int32_t n_views,
                           const float* campos, int64_t campos_stride, const float* g_views, int64_t view_stride,
                           float* d_features_dc, float* d_features_rest, int32_t accumulate, int32_t* nan_flag,
                           int64_t flag_offset);

/* ABI 18.  Strand polylines -> one Gaussian per segment: initialize_gaussians_hair (src/scene/gaussian_model_strands.py:435-452,
 * the same lines in gaussian_model_latent_strands.py), run at the top of every strand-stage iteration
 * (src/train_strands.py:98-104).  origins [S,3] strand roots, dirs [S,n_seg,3] segment vectors (n_seg <= GHR_STRAND_MAX_SEG);
 * outputs, row s n_seg + k = segment k of strand s:
 *   xyz [S n_seg,3]      mid-points of pts = origins + cat(0, cumsum(dirs)) -- the sum taken in list order: bit-identical to torch
 *   rotation [S n_seg,4] parallel_transport((1,0,0), dir) = (1 + b.x, 0, -b.z, b.y), b = dir / max(|dir|, 1e-12)
 *                        (src/utils/general_utils.py:150-160; not normalised)
 *   scaling [S n_seg,3]  (|dir| / 2, scale, scale)
 * The direction rows themselves (self._dir) are a view of dirs and need no kernel. */
int ghr_strand_build(void* stream, int32_t S, int32_t n_seg, const float* origins, const float* dirs, float scale, float* xyz,
                     float* rotation, float* scaling);
/* Its backward: cotangents of the three outputs (each may be NULL = zero; of d_scaling only column 0 is read) -> d_dirs
 * [S,n_seg,3], ASSIGNED.  d xyz_k / d dirs_j = 1 for j < k and 1/2 for j == k (a suffix sum along the strand). */
int ghr_strand_build_backward(void* stream, int32_t S, int32_t n_seg, const float* dirs, const float* d_xyz,
                              const float* d_rotation, const float* d_scaling, float* d_dirs);
/* ABI 20: the same with the cotangent of the direction ROWS (self._dir = dirs.reshape(-1, 3): what render_hair() hands the
 * rasterizer as dir3d, and what ghr_model_backward_segment returns as d_dir3d) as a fourth input, [S n_seg,3] or NULL, added to
 * the result last -- one kernel where autograd otherwise sums the two paths into `_dirs` with a pass of its own. */
int ghr_strand_build_backward_ex(void* stream, int32_t S, int32_t n_seg, const float* dirs, const float* d_xyz,
                                 const float* d_rotation, const float* d_scaling, const float* d_dir_rows, float* d_dirs);

int ghr_model_backward(void* stream, const ghr_model_args* m, uint32_t R, const int32_t* radii, const void* geom_ws,
                       const void* img_ws, const void* bin_ws, const float* dL_dpix, float* grad_scratch,
                       float* d_means2D, float* d_xyz, float* d_log_scales, float* d_rotations,
                       float* d_opacity_logit, float* d_label_logit, float* d_orient_conf_log, float* d_features_dc,
                       float* d_features_rest, int32_t accumulate, int32_t* nan_flag,
                       int32_t prezeroed /* see ghr_backward */);

/* ---- fused stage-1 loss (src/train_gaussians.py:126-140; src/utils/loss_utils.py:19-47,91-121) ----------------
 * loss = w_l1 * mean(|image-gt| * m) + w_ssim * (1 - mean(ssim(image*m, gt*m))) + w_mask * mean(|mask-gt_mask|)
 *        + w_orient * or_loss(orient_angle(dir2d), gt_orient_angle, orient_conf, weight = gt_orient_conf, mask = gt_mask[0]),
 * m = gt_mask[1]; orient_angle as in src/gaussian_renderer/__init__.py:100-105; a NaN orientation term is dropped
 * (train_gaussians.py:134).  All planes are H*W floats: image/gt_image 3, mask/gt_mask 2, dir2d 2 (x, y), the rest 1.
 * The rendered planes may point into one packed [10,H,W] rasterizer output (channels 0-2, 3-4, 5-6, 8).
 * w_orient == 0 disables the orientation term (its pointers may then be NULL). */
typedef struct ghr_loss_args {
    int32_t W, H;
    const float* image;
    const float* mask;
    const float* dir2d;
    const float* orient_conf;
    const float* gt_image;
    const float* gt_mask;
    const float* gt_orient_angle;
    const float* gt_orient_conf;
    float w_l1, w_ssim, w_mask, w_orient;
    int32_t unmasked_colours;     /* != 0: L1 / SSIM on the whole image (train_strands.py:128-129) instead of * gt_mask[1] */
    const float* gt_stats;        /* optional [2,3,H,W]: the SSIM window moments of the (masked) ground truth from
                                     ghr_loss_gt_stats -- constants of a training view; with them ghr_loss_forward
                                     convolves three moments instead of five, with bit-identical results */
} ghr_loss_args;
/* maps: 9*H*W floats of scratch kept for backward.  sums: ghr_loss_sums_floats(W, H) device floats of scratch kept for
 * backward -- {sum of orientation weights, NaN flag, pad} + one slot of five partial sums per workgroup of the forward kernel;
 * needs no initialisation (ABI 16: the 256 shared slots of earlier versions were zero-filled by a launch of their own in front
 * of every forward pass; with a slot per workgroup the fold also has a fixed order).  loss_out: device scalar. */
size_t ghr_loss_sums_floats(int32_t W, int32_t H);
int ghr_loss_forward(void* stream, const ghr_loss_args* a, float* maps, float* sums, float* loss_out);
/* stats_out [2,3,H,W] = {w * y, w * y^2} per colour channel, y = gt_image (* gt_mask[1] unless unmasked_colours), w the
 * 11x11 window of loss_utils.py:91-121.  Reads only W, H, gt_image, gt_mask, unmasked_colours of `a`. */
int ghr_loss_gt_stats(void* stream, const ghr_loss_args* a, float* stats_out);
/* grad_loss: device scalar dL/dloss (NULL = 1).  d_image [3,H,W], d_mask [2,H,W] fully written; d_dir2d [2,H,W] and
 * d_orient_conf [1,H,W] (both or neither; zeros when the orientation term is off or was NaN); zero_plane_a/b: optional
 * H*W planes to zero-fill (the channels of a packed [10,H,W] gradient that no loss term touches). */
int ghr_loss_backward(void* stream, const ghr_loss_args* a, const float* maps, const float* sums,
                      const float* grad_loss, float* d_image, float* d_mask, float* d_dir2d, float* d_orient_conf,
                      float* zero_plane_a, float* zero_plane_b);

/* ---- one call per training view (src/train_gaussians.py:104-147: render, the four loss terms, backward) ------------------------
 * Added without an ABI_VERSION bump: one new function and two new structs, no existing struct or signature changed.
 * ghr_view_step enqueues, on the caller's one stream, what ghr_model_forward_stage1, ghr_forward_stage2 (at capacity R),
 * ghr_loss_forward, ghr_loss_backward, ghr_render_backward and ghr_model_backward_segment enqueue when called in that order with
 * the same values -- it calls those functions: the same kernels, launch shapes and arguments -- so that a binding states the
 * sequence, the hand-over of the workspaces and the flag discipline once, as one struct.  Every buffer is the caller's; the call
 * allocates nothing and never waits for the device.  The instance count lands in *R_host as after stage 1; the caller reads it
 * when it likes (after count_event, or after the stream) and, when it exceeds R, discards and recomputes the view: the kernels
 * stay inside their buffers (ghr_forward_stage2, ghr_backward).
 * The whole struct is validated first: a refused call has launched nothing and ghr_last_error() names the field. */
typedef struct ghr_sh_fold_args {   /* the arguments of ghr_sh_grad_from_views without a flag word */
    int32_t P, sh_degree, sh_coeffs, n_views;
    const float* xyz;
    const float* campos;
    int64_t campos_stride;
    const float* g_views;
    int64_t view_stride;
    float* d_features_dc;
    float* d_features_rest;
    int32_t accumulate;
} ghr_sh_fold_args;
typedef struct ghr_view_step_args {
    /* mode 0, row0 0, P > 0, debug 0, no camera gradients (cam_partial, fovx_dev / fovy_dev NULL) -- ghr_view_step_camera below
     * takes the same struct WITH them, for a camera that is a row of a bank.  Forward fields and backward
     * fields both filled: dens_* / dens_img_ws / overflow_raises_flag / adam_fuse / d_rgb / img_ws_recycled mean what they mean
     * for the single calls (dens_img_ws, when set, must be img_ws below). */
    ghr_model_args model;
    uint32_t R;                /* capacity in instances of bin_ws and of grad_scratch (ghr_forward_stage2) */
    uint32_t* R_host;          /* pinned host word that receives the instance count */
    void* geom_ws;             /* ghr_forward_sizes(P, W, H, 0) */
    void* img_ws;
    void* bin_ws;              /* ghr_binning_size(R, W, H); may be NULL when R == 0 */
    int32_t* radii;            /* [P] */
    float* means2D_out;        /* [P,3] or NULL */
    float* render;             /* [10,H,W]: the packed rasterizer output */
    /* W, H (must equal the model's), the four ground-truth pointers, the weights, unmasked_colours and gt_stats are read; the
     * rendered planes (image, mask, dir2d, orient_conf) are taken from `render` (channels 0, 3, 5, 8) whatever the fields hold */
    ghr_loss_args loss;
    float* maps;               /* 9*H*W floats */
    float* sums;               /* ghr_loss_sums_floats(W, H) floats */
    float* loss_out;           /* device scalar */
    const float* grad_loss;    /* device scalar dL/dloss, NULL = 1 */
    float* d_pix;              /* [10,H,W] scratch: the loss backward fills it, the gradient walk reads it */
    float* grad_scratch;       /* R gradient lines of GHR_GRAD_STRIDE floats; may be NULL when R == 0 */
    int32_t prezero;           /* != 0: stage 2 zeroes the lines and the gradient walk is told so (ghr_backward, prezeroed) */
    /* the outputs and modes of ghr_model_backward; d_features_dc / d_features_rest may be NULL where that call lets them */
    float* d_means2D;
    float* d_xyz;
    float* d_log_scales;
    float* d_rotations;
    float* d_opacity_logit;
    float* d_label_logit;
    float* d_orient_conf_log;
    float* d_features_dc;
    float* d_features_rest;
    int32_t accumulate;
    int32_t* nan_flag;
    /* optional, NULL = not there.  sh_fold: ghr_sh_grad_from_views with these arguments between the gradient walk and the
     * projection backward (the view that carries the update folds the earlier views' d_rgb tables first).
     * The three hipEvent_t: count_event is recorded behind stage 1 (the count has landed once it completes); acc_wait_event is
     * waited for and acc_record_event recorded around {sh_fold, projection backward}, the only kernels of a view that
     * read-modify-write buffers shared with the step's other views -- views on several streams chain exactly those. */
    const ghr_sh_fold_args* sh_fold;
    void* count_event;
    void* acc_wait_event;
    void* acc_record_event;
} ghr_view_step_args;
int ghr_view_step(void* stream, const ghr_view_step_args* v);

/* ---- evaluation pass (src/train_gaussians.py:232-293 training_report; src/metrics.py:71-78; src/render_gaussians.py:31-68) ----
 * Metrics of one view on the packed [10,H,W] rasterizer output `renders` (channels: rgb 0-2, mask 3-4, dir2d 5-6, orientation
 * confidence 8) against gt_image [3,H,W], gt_mask [2,H,W], gt_orient_angle [1,H,W], gt_orient_conf [1,H,W]; all terms on
 * clamp(x, 0, 1) of render, mask, orientation angle and their ground truths, as training_report forms them.  gt_orient_angle
 * and gt_orient_conf both NULL: no orientation terms (their two sums are 0). */
typedef struct ghr_eval_args {
    int32_t W, H;
    const float* renders;
    const float* gt_image;
    const float* gt_mask;
    const float* gt_orient_angle;
    const float* gt_orient_conf;
    int32_t with_ssim;            /* 0: the SSIM kernel is not launched and the row's ssim is 0 */
} ghr_eval_args;
#define GHR_EVAL_TERMS 8
/* Floats of device scratch for one view's partial sums (one slot per workgroup, plain stores: nothing to initialise). */
size_t ghr_eval_scratch_floats(int32_t W, int32_t H);
/* row: GHR_EVAL_TERMS device doubles of a caller-owned table, written by the last of the (at most three) launches:
 *   {l1 = mean |dimage|, ce = mean |dmask|, or_num = sum min(|d|, |d-1|, |d+1|) pi gt_mask[0] w, or_den = sum w (w = gt_orient_conf,
 *    unclamped), mse[3] = mean dimage^2 per channel, ssim = mean of the 11x11 Gaussian-window SSIM map}.
 * The slots are folded in a fixed order in double: the same bits run after run.  Nothing is read back. */
int ghr_eval_metrics(void* stream, const ghr_eval_args* a, float* scratch, double* row);
/* The seven products of render_set in one launch.  bytes: 12*H*W device bytes
 *   [render HWC3 | hair mask HW | head mask HW | orient_angle * hair HW | vis_orient(angle, hair) HWC3 |
 *    vis_orient(angle, 1 - 1 / (orient_conf * hair + 1)) HWC3], quantised as torchvision's save_image does
 *   (floor(clamp(255 v + 0.5, 0, 255))); conf: H*W device floats = orient_conf * hair (the reference's .pth product). */
int ghr_eval_products(void* stream, int32_t W, int32_t H, const float* renders, uint8_t* bytes, float* conf);

/* ---- fused Adam (src/scene/gaussian_model.py:431-444; src/train_gaussians.py:174-181) ---------------------------
 * One pass over flat buffers p/g/m/v of n floats split into n_groups contiguous groups (group_end[i] = exclusive end
 * offset, lr[i] = its learning rate; host arrays).  state: GHR_ADAM_STATE (18) device ints {step, nan_flag, steps each
 * group has sat out [16]}, zero-initialised once.  skip_mask bit g: group g takes no update in this step and its own step
 * number stops advancing for it -- what torch.optim.Adam does for a parameter whose grad is None, i.e. for the
 * nn.Parameters the reference's densification / opacity reset has just replaced (gaussian_model.py:581-658; the
 * optimizer step follows at train_gaussians.py:180).
 * nan_guard != 0: skip the whole update (and do not advance step) when any gradient is NaN, on-device;
 * nan_guard == 1 scans the gradients first, nan_guard == 2 trusts state[1] as maintained by the gradient producer
 * (ghr_model_backward's nan_flag).
 * zero_grad != 0: the gradient buffer is zeroed for the next step. */
/* ABI 19.  One re-lay of the flat parameter / moment buffers for a densification event (src/scene/gaussian_model.py:596-741:
 * densify_and_clone, densify_and_split, prune_points with their cat_tensors_to_optimizer / _prune_optimizer re-creations of
 * every parameter and Adam state tensor).  The buffers are group-major: group g holds P rows of width[g] floats.  For every
 * group and every NEW row r (P_new of them):  p_out[g][r] = override[g] != NULL && child[r] >= 0 ? override[g][child[r]] :
 * p_in[g][take[r]];  m_out / v_out[g][r] = fresh[r] ? 0 : m_in / v_in[g][take[r]]  (clones and split children start with zero
 * moments, gaussian_model.py:634-654).  take, child (nullable; int64) and fresh (uint8) are DEVICE arrays of P_new entries;
 * width_host and override_host (nullable; n_groups device pointers, each NULL or [n_children, width[g]]) are HOST arrays. */
int ghr_adam_relay_rows(void* stream, int32_t n_groups, const int32_t* width_host, int64_t P_old, int64_t P_new,
                        const int64_t* take, const uint8_t* fresh, const int64_t* child, const float* const* override_host,
                        const float* p_in, const float* m_in, const float* v_in, float* p_out, float* m_out, float* v_out);
/* ABI 18.  state[1] |= any(isnan(g[0 .. count))): the scan of nan_guard == 1 over a part of the gradients, for a step whose other
 * gradients came from a producer that keeps the flag itself (the strand stage, src/train_strands.py:151-155: the SH features'
 * gradients are assigned by the fused render_hair backward, those of the strand directions arrive through autograd); follow
 * it with ghr_adam_step(nan_guard = 2). */
int ghr_adam_nan_scan(void* stream, const float* g, int64_t count, int32_t* state);
int ghr_adam_step(void* stream, int64_t n, float* p, float* g, float* m, float* v, int32_t* state, int32_t n_groups,
                  const int64_t* group_end_host, const float* lr_host, double beta1, double beta2, float eps,
                  int32_t nan_guard, int32_t zero_grad, uint32_t skip_mask);
/* The same update restricted to the elements [begin, begin + count) of the n-element buffers (pointers, groups and n
 * as for the whole buffer), so a step can be applied chunk by chunk as the chunks of an all-reduce arrive.  Every
 * chunk of a step sees the same step number; `last` != 0 on the final chunk advances the counter and clears the
 * flag.  nan_guard 1 (scan) is only accepted for the whole buffer. */
int ghr_adam_step_range(void* stream, int64_t n, int64_t begin, int64_t count, float* p, float* g, float* m, float* v,
                        int32_t* state, int32_t n_groups, const int64_t* group_end_host, const float* lr_host,
                        double beta1, double beta2, float eps, int32_t nan_guard, int32_t zero_grad, int32_t last,
                        uint32_t skip_mask);

/* ABI 20.  ghr_adam_step_range OUT OF PLACE: p, m, v of [begin, begin + count) are read from the *_in buffers and written to
 * the *_out buffers (same offsets; an element that takes no update -- flag up, or its group in skip_mask -- is copied), the
 * gradients zeroed when zero_grad != 0.  flag != NULL: the skip-the-step word is *flag instead of state[1].  nan_mark != 0 (needs
 * flag): the pass ORs 1 into *flag itself when a gradient of the range is NaN (the check of src/train_strands.py:151-155) -- some
 * of its elements may then have been updated already, which is harmless here and ONLY here: the `in` set is intact and the
 * caller's finish (ghr_adam_fused_finish) copies it over the `out` set when the flag is up.  No separate ghr_adam_nan_scan of the
 * range is needed in front of the call.  The step counter is not advanced.  For the late groups of a fused step (ghr_adam_fuse, strand segment: the strand directions' and the
 * confidence's gradients arrive through autograd after the kernel that carried the SH features' update): their ranges of the
 * `out` set are produced by ONE pass each instead of three copies and an in-place pass (src/train_strands.py:151-160). */
int ghr_adam_step_range_to(void* stream, int64_t n, int64_t begin, int64_t count, const float* p_in, const float* m_in,
                           const float* v_in, float* p_out, float* g, float* m_out, float* v_out, int32_t* state,
                           int32_t* flag, int32_t nan_mark, int32_t n_groups, const int64_t* group_end_host,
                           const float* lr_host, double beta1, double beta2, float eps, int32_t zero_grad, uint32_t skip_mask);

/* present[i] = view-space z > 0.2 (rasterizer_impl.cu:54-66). */
int ghr_mark_visible(void* stream, int32_t P, const float* means3D, const float* viewmatrix,
                     const float* projmatrix, uint8_t* present);

/* Profiling hook used by bench.py: raw hipEvent_t handles (as void*) that the NEXT calls (from any thread --
 * autograd runs backward on a worker thread) record on the caller's stream immediately before / after the compositing kernel (ghr_forward_stage2: k_render_fwd) and the
 * gradient-walk kernel (ghr_backward: k_render_bwd).  NULL disables a pair.  Sticky until changed. */
int ghr_set_profile_events(void* fwd_start, void* fwd_stop, void* bwd_start, void* bwd_stop);

/* Debug aid (ABI 12; SURVEY.md 5: the reference has none -- its backward sums with float atomics in scheduling
 * order): on != 0 makes the gradient walk bit-reproducible from run to run.  One wave per tile then works the tile's
 * sixteen cells in index order, so the additions into a gradient line happen in one fixed order (the per-Gaussian sum
 * over lines is ordered anyway); about 3x the kernel time.  Process-wide, sticky; returns the previous setting.  While it
 * is on, a backward call at a size the ordered walk cannot address (>= 2^26 rows or instances) FAILS with GHR_E_INVALID
 * instead of running unordered. */
int ghr_set_deterministic(int32_t on);

/* Self test of the wave-level primitives the scan form of the gradient walk is built from (16-lane DPP row scans,
 * row broadcast, v_mfma_f32_16x16x4_f32 operand / result layout): in[8][64] floats -> out[12][64] floats (device
 * pointers); tests/test_gpu_wave_primitives.py states the expected values. */
int ghr_selftest_wave(void* stream, const float* in, float* out);

/* ABI 15.  Self test of the hardware transcendentals the kernels use where the reference calls libm (exp in the alpha of
 * forward.cu:366 / backward.cu:504, 1 / (1 - alpha) in backward.cu:507, sqrt / log / rcp in the conservative culls): the
 * DEVICE twins of csrc/ghr_device.h -- v_exp_f32(x * log2 e), v_rcp_f32, v_sqrt_f32, v_log_f32 * ln 2 -- which the CPU
 * host-sim tests cannot see (they compile the host twins: expf, 1 / x, sqrtf, logf).  in[n][4] -> out[n][4] (device pointers):
 * out = (fast_exp(in.x), fast_rcp(in.y), fast_sqrt(in.z), fast_log(in.w)); tests/test_gpu_wave_primitives.py bounds their
 * error in ulp -- the margin of 2e-5 the parity tests give a discrete decision (tests/helpers.py) rests on those bounds. */
int ghr_selftest_math(void* stream, int32_t n, const float* in, float* out);

/* ---- exact 3-nearest-neighbour mean squared distance (simple_knn's distCUDA2; src/scene/gaussian_model.py:409) ------------
 * Added without an ABI_VERSION bump: three new functions, no existing struct or signature changed.
 * out[i] = ((b0 + b1) + b2) / 3 with b0 <= b1 <= b2 the three smallest d = (dx*dx + dy*dy) + dz*dz (fp32, no contraction;
 * dx = p[j].x - p[i].x) over every j != i (by index), where a slot starts at FLT_MAX and takes d only when d is strictly
 * smaller: +inf for P = 1, 2.  Bit-identical for any schedule and any input permutation.  Sequence: ghr_knn_keys; the caller
 * sorts the keys (ascending, any stable or unstable sort) into `order`, the int64 permutation of 0 .. P-1 that sorts them;
 * ghr_knn_mean_dist2.  P < 2^31; P == 0 does nothing.  Finite coordinates are the caller's check: other bits give
 * unspecified values but no access outside the buffers (an `order` entry outside [0, P) is read as 0). */
/* bytes of the workspace ghr_knn_mean_dist2 needs for P points (256-byte aligned base) */
int ghr_knn_workspace_size(int64_t P, size_t* bytes);
/* points [P,3] f32; bounds_dev [6] f32 = min x, y, z, max x, y, z of the points (device); keys [P] u64 (63-bit Morton codes,
 * sortable as int64).  Keys only steer the search's speed, never its result. */
int ghr_knn_keys(void* stream, int64_t P, const float* points, const float* bounds_dev, uint64_t* keys);
/* order [P] int64 (device); ws: ghr_knn_workspace_size(P) bytes; out [P] f32 (device). */
int ghr_knn_mean_dist2(void* stream, int64_t P, const float* points, const int64_t* order, void* ws, float* out);

/* ---- the camera bank: trainable camera residuals of a whole scene in flat device buffers (src/scene/cameras.py:83-154,
 * src/utils/camera_opt_utils.py:84-141, src/train_gaussians.py:45-66,183-196) -------------------------------------------------
 * Added without an ABI_VERSION bump: three new functions, no existing struct or signature changed.
 * One row per camera in every buffer, rows `stride` floats apart (all fp32):
 *   consts  GHR_CAMERA_CONST floats: W2C[16] (row-major getWorld2View2) | FoVx0 | FoVy0 | znear | P[2][2] | P[2][3] of
 *           getProjectionMatrix (zfar / (zfar - znear), -(zfar znear) / (zfar - znear))
 *   params / grads / moments  rotation_res[6 (ortho-6D) | 3 (se(3))] | translation_res[3] | fov_res[2]
 *   out     GHR_CAMERA_OUT floats: world_view_transform[16] | full_proj_transform[16] | projection_matrix[16] | camera_center[3] |
 *           FoVx | FoVy, the matrices transposed as the reference keeps them
 * `rows`: the number of cameras the bank's buffers hold; `first`, `n`: the calls handle rows [first, first + n) of consts / params /
 * grads / touched and fail when that range reaches past `rows` (nothing is launched); `out` and the cotangents hold the
 * RANGE's rows from 0 (out + r * out_stride; cotangents dense: [n][16], [n][16], [n][16], [n][3], [n], [n]).
 * train_mask: GHR_CAMERA_TRAIN_POSE (rotation + translation) | GHR_CAMERA_TRAIN_FOV; a group outside it composes, gets no
 * gradient and no update. */
#define GHR_CAMERA_ORTHO6D 0
#define GHR_CAMERA_SE3 1
#define GHR_CAMERA_CONST 21
#define GHR_CAMERA_OUT 53
#define GHR_CAMERA_TRAIN_POSE 1
#define GHR_CAMERA_TRAIN_FOV 2
int ghr_camera_compose(void* stream, int32_t parametrisation, int32_t rows, int32_t first, int32_t n, const float* consts,
                       int32_t const_stride, const float* params, int32_t param_stride, float* out, int32_t out_stride);
/* The hand-derived VJP of ghr_camera_compose.  Each cotangent pointer may be NULL (that output took no part in the loss); dFoV
 * receives its direct cotangent and the part through projection_matrix / full_proj_transform.  A row whose touched mark is 0 has
 * its gradient ASSIGNED (whatever it held is gone), a row with the mark up has it ADDED; the mark is set.  One thread owns a row:
 * calls that may run concurrently (two streams) must cover disjoint rows. */
int ghr_camera_compose_backward(void* stream, int32_t parametrisation, int32_t rows, int32_t first, int32_t n, const float* consts,
                                int32_t const_stride, const float* params, int32_t param_stride, const float* d_view,
                                const float* d_full, const float* d_proj, const float* d_center, const float* d_fovx,
                                const float* d_fovy, float* grads, int32_t grad_stride, int32_t* touched, int32_t train_mask);
/* torch.optim.Adam over the rows of all n cameras whose touched mark is up, each with ITS OWN step count (torch counts per parameter
 * and passes a parameter without .grad by), three learning rates as host floats.  If any gradient of a touched row is NaN nothing
 * moves and no count advances (train_gaussians.py:190-196).  Either way the touched rows' gradients and marks are cleared.  One
 * launch, one workgroup; nothing is read back. */
int ghr_camera_adam_step(void* stream, int32_t parametrisation, int32_t n, float* params, float* grads, float* exp_avg,
                         float* exp_avg_sq, int32_t stride, int32_t* steps, int32_t* touched, float lr_rotation,
                         float lr_translation, float lr_fov, double beta1, double beta2, float eps, int32_t train_mask);

/* ---- a training view whose camera is a row of a bank: ghr_view_step with the camera chain around it -----------------------------
 * Added without an ABI_VERSION bump: three new functions and one new struct, no existing struct or signature changed.
 * ghr_view_step_camera enqueues, on the caller's one stream, in this order:
 *   1. ghr_camera_compose(index, 1) into out_row;
 *   2. what ghr_view_step enqueues for `v`, whose model reads the camera from out_row and writes the camera-gradient partial table:
 *      v->model.viewmatrix = out_row, projmatrix = out_row + 16, campos = out_row + 48, fovx_dev = out_row + 51, fovy_dev =
 *      out_row + 52 (the row layout above); cam_partial set, cam_slot0 = 0 ... cam_slots == ghr_camera_slots(P);
 *   3. ghr_camera_grad_fold of that table into d_cam;
 *   4. ghr_camera_compose_backward(index, 1) with d view = d_cam, d full = d_cam + 16, d centre = d_cam + 32, d FoVx = d_cam + 35,
 *      d FoVy = d_cam + 36 and d proj NULL: the row's gradient in `grads`, its touched mark up.
 * It calls those functions -- the same kernels, launch shapes and arguments as the four calls one after the other.  Both structs
 * are validated first: a refused call has launched nothing and ghr_last_error() names the field.  ghr_view_step itself keeps
 * refusing camera gradients.  Views that may run concurrently must be distinct rows of the bank. */
typedef struct ghr_view_camera_args {
    int32_t parametrisation;   /* GHR_CAMERA_ORTHO6D / GHR_CAMERA_SE3 */
    int32_t rows;              /* cameras the bank's buffers hold */
    int32_t index;             /* this view's camera: 0 .. rows - 1 */
    int32_t const_stride;
    const float* consts;
    const float* params;
    int32_t param_stride;
    int32_t grad_stride;
    float* grads;
    int32_t* touched;
    int32_t train_mask;        /* != 0: a bank with both groups frozen is a constant camera (ghr_view_step) */
    float* out_row;            /* caller-owned, GHR_CAMERA_OUT floats: the composed camera the view reads */
    float* d_cam;              /* caller-owned, GHR_CAM_GRADS floats: the folded camera gradients */
} ghr_view_camera_args;
int ghr_view_step_camera(void* stream, const ghr_view_step_args* v, const ghr_view_camera_args* c);

/* The exchange of a replicated bank's gradient rows between G ranks (width: 8 (se(3)) or 11 (ortho-6D) floats of gradient per row).
 * ghr_camera_pack_row_message: message [n][width + 1]: a touched row is its gradient row followed by 1.0f, an untouched row all
 * zeros (whatever `grads` holds there -- a stale NaN included -- does not travel).
 * ghr_camera_merge_ranks: gathered [G][n][width + 1], the ranks' messages in ascending rank order.  Per row and column the first
 * touched rank's value is ASSIGNED to `grads`, later touched ranks' values are added in that order; touched[row] = 1 if any rank
 * touched it; a row no rank touched is neither read nor written.  A row touched by exactly one rank arrives with that rank's bits. */
int ghr_camera_pack_row_message(void* stream, int32_t n, int32_t width, const float* grads, int32_t grad_stride,
                                const int32_t* touched, float* message);
int ghr_camera_merge_ranks(void* stream, int32_t n, int32_t width, int32_t G, const float* gathered, float* grads,
                           int32_t grad_stride, int32_t* touched);

/* ---- ground-truth orientation maps from an image (src/preprocessing/calc_orientation_maps.py; loader: src/utils/camera_utils.py:66-68)
 * Added without an ABI_VERSION bump: five new functions, no existing struct or signature changed.
 * ghr_orient_dog: rgb2gray (0.2989 r + 0.5870 g + 0.1140 b; one channel: the value itself) and the difference of two Gaussians,
 * both in double with indices clamped at the border (scipy.ndimage's mode 'nearest'), axis 0 then axis 1, narrowed to float32.
 *   image [H][W][channels] (channels 1 or 3), uint8 (is_u8) or float32, device; w_low [2 r_low + 1] / w_high [2 r_high + 1]:
 *   symmetric double taps on the DEVICE; scratch: ghr_orient_dog_scratch_bytes(W, H) bytes, 8-B aligned; filtered [H][W] f32.
 * ghr_orient_gabor: cross-correlation of the zero-padded plane with n_filters (1 ... 256) filters of ksize x ksize (odd, <= 25)
 * taps, F_k = |response_k|, deg = the FIRST arg-max, var = sum_k d_k^2 F_k / max(sum_k F_k, 1e-12) with d_k the distance of
 * deg / n_filters * pi and thetas[k] on the circle of circumference pi; angle = deg / 180, conf = 1 / ((v / pi^2)^2 + 1e-7) with
 * v = var, or var rounded through float16 when via_half.  deg (uint8), var, angle, conf [H][W]: each may be NULL.
 *   weights: ghr_orient_bank_floats(n_filters, ksize) floats in the order the matrix unit reads them,
 *   [tile][chunk][lane 0 .. 63] = w[filter 16 tile + (lane & 15)][tap 4 chunk + (lane >> 4)] (tap = row * ksize + column), zero where
 *   the filter or the tap does not exist; tile < 4 ceil(ceil(n_filters / 16) / 4), chunk < ceil(ksize^2 / 4).
 * Finite input is the caller's check.  The same input gives the same bytes on every run.  A refused call launches nothing. */
size_t ghr_orient_dog_scratch_bytes(int32_t W, int32_t H);
int ghr_orient_dog(void* stream, int32_t W, int32_t H, int32_t channels, int32_t is_u8, const void* image, int32_t r_low,
                   const double* w_low, int32_t r_high, const double* w_high, void* scratch, float* filtered);
size_t ghr_orient_bank_floats(int32_t n_filters, int32_t ksize);
int ghr_orient_gabor(void* stream, int32_t W, int32_t H, const float* filtered, int32_t n_filters, int32_t ksize,
                     const float* weights, const float* thetas, uint8_t* deg, float* var, float* angle, float* conf,
                     int32_t via_half);

/* ---- ground-truth loader (src/preprocessing/resize_images.py:101-106; src/utils/camera_utils.py:29-84; src/scene/cameras.py:51-64)
 * Added without an ABI_VERSION bump: four new functions, no existing struct or signature changed.
 * ghr_resample_u8: Pillow's 8-bit resampling (ImagingResample, any filter the coefficients describe; the loader uses bicubic)
 * of in [in_h][in_w][channels] (channels 1 or 3, interleaved) to out [out_h][out_w][channels], bit for bit: the horizontal pass
 * first and only if the widths differ, the vertical pass second and only if the heights differ, the intermediate
 * [in_h][out_w][channels] clipped to uint8 in `scratch` (ghr_resample_scratch_bytes; needed only when both passes run); equal
 * sizes: a device-to-device copy on the stream and no launch.  Per output index i of an axis: bounds[2 i] = the first source
 * index, bounds[2 i + 1] = n taps, coef[i * ksize + 0 .. n) = the weights with 22 fractional bits as Pillow's
 * precompute_coeffs / normalize_coeffs_8bpc give them; out = clip(((1 << 21) + sum in * coef) >> 22, 0, 255) in 32-bit integers.
 * bounds and coef live on the DEVICE; the bounds are read back on the stream (which is synchronised once per pass) and a pair
 * with n > ksize or first + n > the input's size refuses the call.  in and out must not overlap.
 * ghr_gt_assemble: one launch for a view's tensors at W x H from the resized bytes: out_image [3][H][W] = (image / 255) * body +
 * white_background * (1 - body); out_mask [2][H][W] = hair, body as m / 255, or (m >= 128) when binarize; out_angle [1][H][W] =
 * clamp(angle / 180, 0, 1); out_conf [1][H][W] = 1 / ((v / pi^2)^2 + 1e-7), v = the variance map var [var_h][var_w] (rounded
 * through float16 first when via_half) sampled as F.interpolate(mode='bilinear', align_corners=False) samples it, in float32:
 * src = max(scale (dst + 0.5) - 0.5, 0), hy (hx a + lx b) + ly (hx c + lx d); at equal sizes the map's own value.
 * div255_table / div180_table: 256 device floats i / 255 and i / 180 divided on the host.  (angle, out_angle) and (var, out_conf)
 * may be NULL together.  ghr_gt_resize_variance: that bilinear sample alone, out [H][W].
 * The same input gives the same bytes on every run.  A refused call launches nothing. */
size_t ghr_resample_scratch_bytes(int32_t in_w, int32_t in_h, int32_t out_w, int32_t out_h, int32_t channels);
int ghr_resample_u8(void* stream, int32_t in_w, int32_t in_h, int32_t channels, const uint8_t* in, int32_t out_w, int32_t out_h,
                    uint8_t* out, const int32_t* bounds_x, const int32_t* coef_x, int32_t ksize_x, const int32_t* bounds_y,
                    const int32_t* coef_y, int32_t ksize_y, void* scratch);
int ghr_gt_assemble(void* stream, int32_t W, int32_t H, const uint8_t* image, const uint8_t* mask_hair, const uint8_t* mask_body,
                    const uint8_t* angle, const float* var, int32_t var_w, int32_t var_h, const float* div255_table,
                    const float* div180_table, int32_t white_background, int32_t binarize, int32_t via_half, float* out_image,
                    float* out_mask, float* out_angle, float* out_conf);
int ghr_gt_resize_variance(void* stream, int32_t W, int32_t H, const float* var, int32_t var_w, int32_t var_h, int32_t via_half,
                           float* out);

/* ---- synthetic ground truth (src/utils/camera_utils.py:51-64 with load_synthetic_rgba and load_synthetic_geom, at -r 1)
 * Added without an ABI_VERSION bump: one new function, no existing struct or signature changed.
 * ghr_gt_from_render: one launch from the packed render [10][H][W] (channels 0-6 and 8 are read) to the four tensors the
 * reference builds by writing render_set's products to disk and reading them back.  Per pixel, with q(v) = the 8-bit level
 * uint8(clamp(v * 255 + 0.5, 0, 255)) of torchvision's save_image and t = div255_table (256 device floats i / 255 divided on the
 * host): hair = t[q(r3)], body = t[q(r4)], or (level >= 128) when binarize; out_image [3][H][W] = t[q(r_c)] * body +
 * white_background * (1 - body); out_mask [2][H][W] = hair, body; out_angle [1][H][W] = t[q(angle * r3)], angle the orientation
 * angle / pi of (r5, r6) as ghr_eval_products forms it; out_conf [1][H][W] = r8 * r3, not clamped.  The levels are those
 * ghr_eval_products writes; image and masks are what ghr_gt_assemble makes of them.  Renders must be finite.  Four pixels per
 * thread with 16-B accesses when H * W % 4 == 0 and all five buffers are 16-B aligned, single accesses otherwise: the same bits
 * either way, run after run.  A refused call launches nothing. */
int ghr_gt_from_render(void* stream, int32_t W, int32_t H, const float* renders, const float* div255_table, int32_t white_background,
                       int32_t binarize, float* out_image, float* out_mask, float* out_angle, float* out_conf);

/* ---- the latent-strand stage (src/train_latent_strands.py:103-164; src/scene/gaussian_model_latent_strands.py:451-499)
 * Added without an ABI_VERSION bump: seven new functions and one new struct, no existing struct or signature changed.
 * ghr_strand_points_build: strands given as POINTS p [S][L][3], L >= 2 (no upper bound), n_seg = L - 1; row s n_seg + k is
 * segment k of strand s (the layout of ghr_strand_build): xyz = (p[k+1] + p[k]) * 0.5 and dir_rows = p[k+1] - p[k], bit for bit
 * the PyTorch expressions; rotation [.][4] (16-B aligned) and scaling [.][3] as ghr_strand_build makes them from the direction.
 * ghr_strand_points_build_backward: d_p [S][L][3] is ASSIGNED; each cotangent may be NULL, of d_scaling only column 0 is read.
 * Point j gets  d_xyz / 2 + g  of segment j - 1 first, then  d_xyz / 2 - g  of segment j, g = the segment's whole direction
 * cotangent (rotation, scaling[0], d_dir_rows).  No atomics: the same input gives the same bytes on every run.
 * ghr_strand_rows_expand: dst [S n_seg][C] = src [S][C] repeated over a strand's segments (C >= 1);
 * ghr_strand_rows_reduce: out [S][C] = the sum of the strand's n_seg rows of g in index order, one fp32 accumulator each.
 * ghr_latent_loss_*: loss = w_l1 mean_{3HW}|image - gt_image| + w_mask mean_{HW}|mask0 - gt_mask0| + w_orient or_loss(angle(dir2d),
 * gt_orient_angle, orient_conf, weight = gt_orient_conf, mask = gt_mask0) (src/utils/loss_utils.py:31-47); each term is dropped
 * (value 0, gradient 0) exactly when it is NaN.  The rendered planes may point into one packed [10][H][W] output.
 * sums: ghr_latent_loss_sums_floats(W, H) floats, 16-B aligned, nothing to pre-fill: {Ll1, LCE, LOR, their three NaN flags, the
 * sum of the orientation weights, 0} then one slot {l1, ce, or_num, or_den} per 1024 pixels.  The backward recomputes pointwise
 * from the same args and `sums`, and writes ALL ten planes of d_packed [10][H][W] (image 0-2, mask0 3, dir2d 5-6, confidence 8;
 * zeros elsewhere); grad_loss: device scalar or NULL (1).  The whole struct is checked before any launch and ghr_last_error()
 * names the field.  A refused call launches nothing. */
typedef struct ghr_latent_loss_args {
    int32_t W, H;
    const float* image;            /* [3][H][W] rendered */
    const float* mask0;            /* [1][H][W] rendered hair label */
    const float* dir2d;            /* [2][H][W] rendered 2D direction */
    const float* orient_conf;      /* [1][H][W] rendered confidence, or NULL: train_orient_conf = False */
    const float* gt_image;         /* [3][H][W] */
    const float* gt_mask0;         /* [1][H][W] */
    const float* gt_orient_angle;  /* [1][H][W] */
    const float* gt_orient_conf;   /* [1][H][W], or NULL: weight 1 (use_gt_orient_conf = False) */
    float w_l1, w_mask, w_orient;
} ghr_latent_loss_args;
int ghr_strand_points_build(void* stream, int32_t S, int32_t L, const float* p, float scale, float* xyz, float* rotation,
                            float* scaling, float* dir_rows);
int ghr_strand_points_build_backward(void* stream, int32_t S, int32_t L, const float* p, const float* d_xyz,
                                     const float* d_rotation, const float* d_scaling, const float* d_dir_rows, float* d_p);
int ghr_strand_rows_expand(void* stream, int32_t S, int32_t n_seg, int32_t C, const float* src, float* dst);
int ghr_strand_rows_reduce(void* stream, int32_t S, int32_t n_seg, int32_t C, const float* g, float* out);
size_t ghr_latent_loss_sums_floats(int32_t W, int32_t H);
int ghr_latent_loss_forward(void* stream, const ghr_latent_loss_args* l, float* sums, float* loss_out);
int ghr_latent_loss_backward(void* stream, const ghr_latent_loss_args* l, const float* sums, const float* grad_loss,
                             float* d_packed);

/* ---- per-strand SH coefficients in the segmented form (csrc/ghr_shared.h)
 * Added without an ABI_VERSION bump: three new functions and one new struct, no existing struct or signature changed.
 * A mode-1 segment whose features_dc is [S][1][3] and features_rest [S][K-1][3]: row i of the segment (P = S rows_per_strand
 * rows, row s rows_per_strand + k = segment k of strand s) reads the coefficients of strand i / rows_per_strand.  Everything else
 * is as in ghr_model_forward_segment / ghr_model_backward_segment, and such a segment may be mixed freely with ordinary
 * segments of the same rasterizer state: the records, radii, means2D and every per-row gradient have the bits those calls
 * give for the coefficients repeated over the rows.
 * ghr_model_backward_segment_shared runs the projection backward in factored form into d_rgb_ws [P][3] (caller-owned scratch,
 * ASSIGNED: dL/d(rgb) behind the colour clamp) and then folds it: d_features_dc [S][1][3] and d_features_rest [S][K-1][3] are
 * ASSIGNED the sums over the strand's rows j = 0 .. rows_per_strand - 1, in index order, one fp32 accumulator each, of
 * basis_k(normalize(xyz_j - campos)) d_rgb_j[c] -- the products the ordinary call stores per row, summed as
 * ghr_strand_rows_reduce sums them (a row without gradient contributes +0; its direction is not evaluated).  There is no
 * `accumulate`.  nan_flag is raised for a non-finite value in any gradient written, the folded ones included.
 * The whole argument set is checked before any launch and ghr_last_error() names the field.  Refused: mode != 1;
 * P != n_strands * rows_per_strand; rows_per_strand < 1; adam_fuse, cam_only or d_rgb set in `m`; sh_coeffs outside 1, 4, 9, 16;
 * (backward, P > 0) NULL d_rgb_ws, d_features_dc, or d_features_rest with K > 1.  A refused call launches nothing.  P == 0 is
 * GHR_OK and launches nothing -- not even the counter reset of a `first` forward segment: give `first` to a segment with rows
 * or to an ordinary (possibly empty) one.
 * ghr_shared_sh_fold is the second half of that backward on its own, for a caller that holds a d_rgb table already: xyz and
 * d_rgb are [S rows_per_strand][3], campos [3] (device), both outputs ASSIGNED; n_strands == 0 is GHR_OK and launches nothing. */
typedef struct ghr_shared_features {
    int32_t n_strands;        /* S */
    int32_t rows_per_strand;  /* n_seg >= 1; the segment's P must equal S * n_seg */
} ghr_shared_features;
int ghr_model_forward_segment_shared(void* stream, const ghr_model_args* m, const ghr_shared_features* sf, int32_t rows_total,
                                     int32_t first, void* geom_ws, void* img_ws, int32_t* radii, float* means2D_out);
int ghr_model_backward_segment_shared(void* stream, const ghr_model_args* m, const ghr_shared_features* sf, int32_t rows_total,
                                      const int32_t* radii, const void* geom_ws, const float* grad_scratch, float* d_means2D,
                                      float* d_xyz, float* d_log_scales, float* d_rotations, float* d_opacity_logit,
                                      float* d_label_logit, float* d_orient_conf_log, float* d_features_dc,
                                      float* d_features_rest, float* d_dir3d, int32_t* nan_flag, uint32_t grad_rows,
                                      const void* bin_ws, uint32_t R, float* d_rgb_ws);
int ghr_shared_sh_fold(void* stream, const ghr_shared_features* sf, int32_t sh_degree, int32_t sh_coeffs, const float* xyz,
                       const float* campos, const float* d_rgb, float* d_features_dc, float* d_features_rest, int32_t* nan_flag);

/* ---- point-in-mesh containment and the Gaussian probe filter (csrc/ghr_mesh.h)
 * Added without an ABI_VERSION bump: four new functions and one new struct, no existing struct or signature changed.
 * The definition of "inside" is the one at the top of csrc/ghr_mesh.h: three axis rays, exact complementary edge predicates,
 * the majority of the three parities; a query with a non-finite coordinate or outside the mesh's bounding box is outside.
 * ghr_mesh_grid_sizes / ghr_mesh_grid_build run on the HOST (plain C++, deterministic: the same mesh gives the same bytes):
 * vertices [V][3] finite floats, faces [F][3] indices into them, G the cells per side of each axis' grid (0: ceil(sqrt(F)),
 * at most 256).  _sizes validates the mesh and fills *header, whose `bytes` is the size of the blob; _build fills `blob`
 * (host memory, 16-B aligned, `bytes` long), which starts with the finished header (list_max filled in).  The caller copies
 * the blob to the device as it is.
 * ghr_mesh_contains: points [Q][3]; inside [Q] bytes 0 / 1; crossings [Q][3] (the three axes' crossing counts) or NULL.
 * ghr_gaussian_probe_outside: xyz [P][3], scaling [P][3] ACTIVATED, rotation [P][4] raw (normalised in the kernel);
 * outside [P] bytes: 1 iff all twelve probes xyz + (3-sigma image of a level-0 icosphere vertex) are outside.
 * probe: GHR_PROBE_REFERENCE, the points of src/preprocessing/filter_flame_intersections.py:88,109 (R diag(3 s) v + xyz: that
 * script's build_rotation returns the transpose of the rotation matrix R); GHR_PROBE_AXIS_SCALED, diag(3 s) Rt v + xyz.
 * `header` is the HOST copy of the blob's header, `grid_dev` the blob on the device.  Q == 0 / P == 0 is GHR_OK and launches
 * nothing.  A refused call launches nothing and ghr_last_error() says why. */
#define GHR_PROBE_REFERENCE 0
#define GHR_PROBE_AXIS_SCALED 1
typedef struct ghr_mesh_grid {
    uint32_t magic;
    int32_t G, n_faces, n_vertices;
    float lo[3], hi[3];      /* bounding box of the mesh */
    float scale[3];          /* cells per unit along each world coordinate */
    uint32_t list_total[3];  /* entries of each axis' cell lists */
    uint32_t list_max[3];    /* longest cell list of each axis (filled by ghr_mesh_grid_build) */
    uint32_t pad_;
    uint64_t off_rec[3], off_start[3], off_list[3];  /* byte offsets into the blob */
    uint64_t bytes;
} ghr_mesh_grid;
int ghr_mesh_grid_sizes(int32_t n_vertices, const float* vertices, int32_t n_faces, const int32_t* faces, int32_t G,
                        ghr_mesh_grid* header);
int ghr_mesh_grid_build(int32_t n_vertices, const float* vertices, int32_t n_faces, const int32_t* faces, int32_t G,
                        void* blob, size_t bytes);
int ghr_mesh_contains(void* stream, const ghr_mesh_grid* header, const void* grid_dev, int64_t Q, const float* points,
                      uint8_t* inside, uint32_t* crossings);
int ghr_gaussian_probe_outside(void* stream, const ghr_mesh_grid* header, const void* grid_dev, int64_t P, const float* xyz,
                               const float* scaling, const float* rotation, int32_t probe, uint8_t* outside);

/* ---- closest point on and signed distance to a triangle mesh (csrc/ghr_meshdist.h)
 * Added without an ABI_VERSION bump: four new functions and one new struct, no existing struct or signature changed.
 * The definition of the closest point, of dist2 and of the winning face is the one at the top of csrc/ghr_meshdist.h: three
 * clamped edge candidates and a clamped interior candidate per face in float32, the smallest d, the lowest face index among
 * equals.  ghr_mesh_tris_sizes / ghr_mesh_tris_build run on the HOST (plain C++, deterministic): vertices [V][3] with
 * |coordinate| <= 2^30, faces [F][3] indices into them, F >= 1.  _sizes validates the mesh and fills *header, whose `bytes` is
 * the size of the blob; _build fills `blob` (host memory, 16-B aligned, `bytes` long), which starts with the header.  The
 * caller copies the blob to the device as it is.
 * ghr_mesh_closest: points [Q][3], Q < 2^31; order [Q] the permutation that sorts the 63-bit keys of the points
 * (ghr_knn_keys over the bounds header.lo, header.hi), keys_sorted [Q] those keys sorted.  dist2 [Q], face [Q], point [Q][3]
 * are written at the queries' original indices; a query with a non-finite coordinate gets +inf, -1 and itself.
 * ghr_mesh_distance_backward: the gradient of sd = (inside ? -1 : 1) sqrtf(dist2) to the points: closest [Q][3], dist2 [Q],
 * inside [Q] bytes (ghr_mesh_contains'), g [Q] the upstream gradient -> d_points [Q][3] = (g sign) ((q - c) / sqrtf(dist2)),
 * 0 where dist2 == 0 or the query was not finite.
 * `header` is the HOST copy of the blob's header, `tris_dev` the blob on the device.  Q == 0 is GHR_OK and launches nothing.
 * A refused call launches nothing and ghr_last_error() says why. */
typedef struct ghr_mesh_tris {
    uint32_t magic;
    int32_t n_faces, n_blocks, n_super;
    float lo[3], hi[3];      /* box of the vertices that faces use: the bounds of the keys */
    uint32_t pad_[2];
    uint64_t off_rec, off_bbox, off_sbox, off_keys;  /* byte offsets into the blob */
    uint64_t bytes;
} ghr_mesh_tris;
int ghr_mesh_tris_sizes(int32_t n_vertices, const float* vertices, int32_t n_faces, const int32_t* faces, ghr_mesh_tris* header);
int ghr_mesh_tris_build(int32_t n_vertices, const float* vertices, int32_t n_faces, const int32_t* faces, void* blob,
                        size_t bytes);
int ghr_mesh_closest(void* stream, const ghr_mesh_tris* header, const void* tris_dev, int64_t Q, const float* points,
                     const int64_t* order, const uint64_t* keys_sorted, float* dist2, int32_t* face, float* point);
int ghr_mesh_distance_backward(void* stream, int64_t Q, const float* points, const float* closest, const float* dist2,
                               const uint8_t* inside, const float* g, float* d_points);

/* ---- head-mesh visibility: a triangle rasterizer and the per-vertex view counts (csrc/ghr_visibility.h)
 * Added without an ABI_VERSION bump: three new functions, no existing struct or signature changed.
 * The definition of pix_to_face, of the head mask and of "seen" is the one at the top of csrc/ghr_visibility.h: pixel centres
 * at +0.5, ghr_mesh.h's exact complementary edge predicates, the largest inverse depth wins, the lower face index among equals.
 * ghr_vis_sizes: bytes of the workspace of one view of H x W pixels of a mesh of V vertices and F faces (device memory, 16-B
 * aligned; it may be reused for any view of at most these sizes, one view at a time).
 * ghr_vis_view: vertices [V][3], faces [F][3] (a face with an index outside 0 .. V - 1 never covers), M [12] on the HOST: the
 * row-major 3 x 4 matrix to (x w, y w, w) in pixels; near: a vertex is valid iff its w is finite and > near.  body / hair: uint8
 * [H][W] planes or both NULL (head then holds nowhere).  Writes pix_to_face [H][W] int32 (-1: nothing) and, unless NULL,
 * vis [H][W] uint8 (255 where a face wins and head holds); unless both NULL, ADDS to cnt [V] / cnt_head [V] (int32) 1 for every
 * vertex a winning face of this view has / has at a pixel where head holds.  V == 0, F == 0 and H * W == 0 are valid.
 * ghr_vis_head_mask: head [H][W] bytes 0 / 1 = (max5x5(body) >= 128) and not (max5x5(hair) >= 128), windows clipped to the image.
 * A refused call launches nothing and ghr_last_error() says why. */
int ghr_vis_sizes(int32_t V, int32_t F, int32_t H, int32_t W, size_t* bytes);
int ghr_vis_view(void* stream, int32_t V, const float* vertices, int32_t F, const int32_t* faces, const float* M, float near_w,
                 int32_t H, int32_t W, const uint8_t* body, const uint8_t* hair, void* workspace, int32_t* pix_to_face,
                 uint8_t* vis, int32_t* cnt, int32_t* cnt_head);
int ghr_vis_head_mask(void* stream, int32_t H, int32_t W, const uint8_t* body, const uint8_t* hair, uint8_t* head);

/* ---- the strand stage's prior term between its networks (csrc/ghr_sds.h)
 * Added without an ABI_VERSION bump: four new functions, no existing struct or signature changed.
 * ghr_sds_local: N guiding strands idx [N] (int64, drawn with replacement from 0 .. S - 1) of dirs [S][n][3] into their local
 * frames: e [N][n + 1][3] = (M P) scale with P the running sum of the strand's segments from 0, v [N][n][3] = (M dir) scale.
 * frames [S][3][3] row-major: local2world (M is its adjugate inverse, formed per strand) or, frames_are_inverse != 0, M itself.
 * An index outside 0 .. S - 1 reads nothing and leaves NaN rows.
 * ghr_sds_local_backward: d_dirs [S][n][3], ZERO-FILLED BY THE CALLER, += (M^T (d_v[g, i] + sum_{j > i} d_e[g, j])) scale for
 * every guiding strand; sorted_idx / order [N] (int64) are a STABLE ascending sort of idx and its permutation: strands drawn
 * more than once add in ascending g.  d_e or d_v may be NULL (both: nothing is launched).
 * ghr_sds_texture: uvg [N][2] the guiding strands' UVs, centres [G] the texel centres of one axis (texel q = row G + col lies
 * at (centres[col], centres[row])), z [N][C], v [N][n][3].  Writes nbr [G G][4] int32 (the four nearest under (d2, g)
 * ascending), w [G G][4], csim / alpha [N] (of TEXEL q < N: alpha[g] is read by whoever chose guiding strand g), alpha_q [G G],
 * the inverted lists start [N + 1] / list [4 G G] (entries 4 q + k, ascending within a strand; count [N] is their scratch) and
 * texture [C][G][G].  Three kernels and one fill.
 * ghr_sds_texture_backward: from the forward's buffers and d_texture [C][G][G]: d_z [N][C] and, unless NULL, d_v [N][n][3]
 * (every element written); dalpha_q [G G] and d_csim [N] are scratch.  Sums run over the lists in their order: no atomics,
 * the same bits every time.
 * Refused before the runtime is touched: NULL pointers, N < 4, G G < N, C < 1, n < 1, S < 1. */
int ghr_sds_local(void* stream, int32_t S, int32_t N, int32_t n, const float* dirs, const float* frames, int32_t frames_are_inverse,
                  const int64_t* idx, float scale, float* e, float* v);
int ghr_sds_local_backward(void* stream, int32_t S, int32_t N, int32_t n, const float* frames, int32_t frames_are_inverse,
                           const int64_t* sorted_idx, const int64_t* order, float scale, const float* d_e, const float* d_v,
                           float* d_dirs);
int ghr_sds_texture(void* stream, int32_t N, int32_t n, int32_t C, int32_t G, const float* uvg, const float* centres, const float* z,
                    const float* v, int32_t* nbr, float* w, float* csim, float* alpha, float* alpha_q, int32_t* count,
                    int32_t* start, int32_t* list, float* texture);
int ghr_sds_texture_backward(void* stream, int32_t N, int32_t n, int32_t C, int32_t G, const float* z, const float* v,
                             const int32_t* nbr, const float* w, const float* csim, const float* alpha_q, const int32_t* start,
                             const int32_t* list, const float* d_texture, float* dalpha_q, float* d_csim, float* d_z, float* d_v);

/* ---- cross-cloud nearest neighbour and the point terms of a chamfer distance (csrc/ghr_nn.h)
 * Added without an ABI_VERSION bump: four new functions, no existing struct or signature changed.
 * For query x_i and every candidate y_j, j < Py: d = (dx*dx + dy*dy) + dz*dz (norm 2, the SQUARED distance) or
 * d = (|dx| + |dy|) + |dz| (norm 1), dx = y_j.x - x_i.x, fp32 without contraction.  dist[i] is the smallest d and idx[i] the
 * LOWEST original j among those that reach it: the same bits for any schedule and any permutation of either cloud; idx in
 * [0, Py).  Finite coordinates are the caller's check: other bits give unspecified values, never an out-of-range access.
 * Sequence: ghr_knn_keys on each cloud with bounds_dev = the bounds of their UNION; the caller sorts each cloud's keys (stable)
 * and passes the permutations and the sorted keys; ghr_nn_search (two box passes and the search).
 * ghr_chamfer_point: term[i] = 1 - cos or 1 - |cos| (abs_cosine != 0), cos = (a . b) / (max(|a|, 1e-6) max(|b|, 1e-6)),
 * a = x_normals[i], b = y_normals[idx[i]]; weight[i] = y_weights[idx[i]].  Normals (with term) and weights (with weight) are
 * each optional (NULL), not both.
 * ghr_chamfer_point_backward: from g_dist [Px] (optional) d_x [Px][3] and d_y [Py][3], from g_cos [Px] (optional)
 * d_x_normals / d_y_normals; every element written.  start [Py + 1] / members [Px] (int64): the queries that chose candidate j
 * are members[start[j] .. start[j + 1]) in ASCENDING order (a stable sort of idx); d_y[j] adds their products in that order
 * with one fp32 accumulator per component, no atomics: the same bits every time, +0 for a candidate nobody chose.
 * Refused before the runtime is touched: sizes outside [0, 2^31), Py == 0, a norm other than 1 or 2, NULL pointers.
 * Px == 0 does nothing in ghr_nn_search and ghr_chamfer_point. */
int ghr_nn_workspace_size(int64_t Px, int64_t Py, size_t* bytes);
int ghr_nn_search(void* stream, int64_t Px, const float* x, const int64_t* order_x, const uint64_t* keys_x_sorted, int64_t Py,
                  const float* y, const int64_t* order_y, const uint64_t* keys_y_sorted, int32_t norm, void* ws, float* dist,
                  int32_t* idx);
int ghr_chamfer_point(void* stream, int64_t Px, int64_t Py, const int32_t* idx, const float* x_normals, const float* y_normals,
                      int32_t abs_cosine, const float* y_weights, float* term, float* weight);
int ghr_chamfer_point_backward(void* stream, int64_t Px, int64_t Py, int32_t norm, const float* x, const float* y, const int32_t* idx,
                               const int64_t* start, const int64_t* members, const float* g_dist, const float* x_normals,
                               const float* y_normals, int32_t abs_cosine, const float* g_cos, float* d_x, float* d_y,
                               float* d_x_normals, float* d_y_normals);

/* ---- the strand preview: depth-tested polylines over the head mesh, shaded (csrc/ghr_strandview.h)
 * Added without an ABI_VERSION bump: five new functions and one new struct, no existing struct or signature changed.
 * The definition of coverage (a closed capsule of half-width r pixels around every segment of S strands of L points), of the
 * winner (largest inverse depth, lowest segment index among equals), of the head test and of the shading is the one at the top of
 * csrc/ghr_strandview.h.  M [12] is on the HOST, as for ghr_vis_view; every other pointer is device memory.
 * ghr_strandview_sizes: bytes of the workspace of one frame (16-B aligned; reusable for any frame of at most these sizes).
 * ghr_strandview_face_depth: qf [H][W] = 8h's inverse depth of face pix_to_face[pixel] at the pixel's centre, 0 where the entry
 * is outside 0 .. F - 1 or the face does not cover the centre.
 * ghr_strandview_raster: points [S][L][3]; pix_to_face / qf are given or NULL together (NULL: no mesh).  Writes the four planes
 * pix_to_segment (int32, -1: none or hidden by the head), t, pix_to_face_out (int32) and inv_depth.
 * ghr_strandview_shade: rgb [H][W][3] bytes from the two index planes; mode GHR_STRANDVIEW_KAJIYA or GHR_STRANDVIEW_TANGENT;
 * base [S][3] per-strand colours or NULL (shading->base_rgb for every strand).  An index outside its table shades as background.
 * ghr_strandview_resolve: dst [H][W][3] from src [s H][s W][3], s = supersample in {1, 2, 4}: (sum + s s / 2) / (s s).
 * S == 0, F == 0 and H * W == 0 are valid.  Refused: L < 2, a half_width that is not finite and > 0, a negative (or NaN)
 * head_bias, an unknown mode, a shininess_log2 outside 0 .. 16, supersample outside {1, 2, 4}, a NULL required buffer, a
 * workspace that is not 16-B aligned or a plane that is not 4-B aligned.  A refused call launches nothing and ghr_last_error()
 * says why. */
#define GHR_STRANDVIEW_KAJIYA 0
#define GHR_STRANDVIEW_TANGENT 1
typedef struct ghr_strandview_shading {
    float eye[3];             /* the camera centre, world space */
    float light[3];           /* a unit vector towards the light, world space */
    float ambient, kd, ks;
    int32_t shininess_log2;   /* the specular term is squared this many times */
    float base_rgb[3], head_rgb[3], background_rgb[3];
} ghr_strandview_shading;
int ghr_strandview_sizes(int32_t S, int32_t L, int32_t H, int32_t W, size_t* bytes);
int ghr_strandview_face_depth(void* stream, int32_t V, const float* vertices, int32_t F, const int32_t* faces, const float* M,
                              float near_w, int32_t H, int32_t W, const int32_t* pix_to_face, float* qf);
int ghr_strandview_raster(void* stream, int32_t S, int32_t L, const float* points, const float* M, float near_w, int32_t H,
                          int32_t W, float half_width, float head_bias, const int32_t* pix_to_face, const float* qf,
                          void* workspace, int32_t* pix_to_segment, float* t, int32_t* pix_to_face_out, float* inv_depth);
int ghr_strandview_shade(void* stream, int32_t S, int32_t L, const float* points, int32_t V, const float* vertices, int32_t F,
                         const int32_t* faces, int32_t H, int32_t W, const int32_t* pix_to_segment, const int32_t* pix_to_face_out,
                         int32_t mode, const ghr_strandview_shading* shading, const float* base, uint8_t* rgb);
int ghr_strandview_resolve(void* stream, int32_t H, int32_t W, int32_t supersample, const uint8_t* src, uint8_t* dst);

/* ---- self-shadowing of the strand preview: a deep opacity map of a light view (csrc/ghr_strandview.h)
 * Added without an ABI_VERSION bump, as the preview itself was: two new functions and one new struct, nothing existing changed.
 * ghr_strandview_opacity: the light pass.  points [S][L][3] under the light view (Ml [12] on the HOST, Hl, Wl, near_w) with the
 * half-width half_width (texels) and the layer depth `layer` (the light's w units).  Writes q0 [Hl][Wl] float (the front plane:
 * the largest inverse depth that covers the texel's centre, 0: none) and layers [Hl][Wl][4] uint32 (the covering segments counted
 * in four layers behind it).  The workspace is the one ghr_strandview_sizes(S, L, Hl, Wl) sizes; workspace_bytes is checked.
 * ghr_strandview_shade_shadowed: ghr_strandview_shade with the raster's t plane and the light's map: in kajiya mode the diffuse
 * and specular terms of a strand pixel and the diffuse term of a head pixel are multiplied by the transmittance at the pixel's
 * world point; tangent mode and the background are ghr_strandview_shade's.  shadow->qfl (the head's inverse depth in the light
 * view, from ghr_vis_view and ghr_strandview_face_depth) may be NULL: no mesh.
 * S == 0 and Hl * Wl == 0 are valid.  Refused: what ghr_strandview_raster and _shade refuse, a layer or half_width that is not
 * finite and > 0, a kappa or bias that is negative or not finite, a NULL plane, layers not 16-B aligned, a workspace too small. */
typedef struct ghr_strandview_shadow {
    float Ml[12];            /* the light view's pixel matrix */
    float near_w;
    int32_t Hl, Wl;
    float layer, kappa, bias;
    const float* q0;         /* [Hl][Wl] */
    const uint32_t* layers;  /* [Hl][Wl][4], 16-B aligned */
    const float* qfl;        /* [Hl][Wl] or NULL */
} ghr_strandview_shadow;
int ghr_strandview_opacity(void* stream, int32_t S, int32_t L, const float* points, const float* Ml, float near_w, int32_t Hl,
                           int32_t Wl, float half_width, float layer, void* workspace, size_t workspace_bytes, float* q0,
                           uint32_t* layers);
int ghr_strandview_shade_shadowed(void* stream, int32_t S, int32_t L, const float* points, int32_t V, const float* vertices, int32_t F,
                                  const int32_t* faces, int32_t H, int32_t W, const int32_t* pix_to_segment,
                                  const int32_t* pix_to_face_out, const float* t, int32_t mode, const ghr_strandview_shading* shading,
                                  const float* base, const ghr_strandview_shadow* shadow, uint8_t* rgb);

/* ---- synthetic captures: a groom's masks and orientation map from the strand raster (csrc/ghr_capture.h)
 * Added without an ABI_VERSION bump, as the preview's entries were: one new function, nothing existing changed.
 * ghr_strandview_capture: from the planes pix_to_segment and pix_to_face_out [s H][s W] of ghr_strandview_raster on the s-times
 * finer grid (s = supersample in {1, 2, 4}; M [12] on the HOST is that grid's matrix: already supersampled) the four planes
 * [H][W] of one view: mask_hair and mask_body (bytes: the covered share of the pixel's s s subsamples; the body includes the
 * hair), angle (a byte 0 .. 179: the bin of the mean doubled angle of the covering segments' screen directions; byte k is the
 * direction (sin k deg, cos k deg), x right, y down) and var (float: var_floor + half of one minus the mean resultant length,
 * 0.5 where no strand is seen).  table [180][2] = (cos 2 th_k, sin 2 th_k), th_k = k pi / 180, in float64 rounded once, is device
 * memory.  The definition is the one at the top of csrc/ghr_capture.h.  An entry outside its table counts as nothing.
 * H * W == 0, S == 0 and F == 0 are valid.  Refused, launching nothing: L < 2, supersample outside {1, 2, 4}, a var_floor that is
 * negative or not finite, a negative (or NaN) near, a NULL required buffer, an index or float plane that is not 4-B aligned. */
int ghr_strandview_capture(void* stream, int32_t S, int32_t L, const float* points, const float* M, float near_w, int32_t H,
                           int32_t W, int32_t supersample, int32_t F, const int32_t* pix_to_segment, const int32_t* pix_to_face_out,
                           const float* table, float var_floor, uint8_t* mask_hair, uint8_t* mask_body, uint8_t* angle, float* var);

/* ---- the comparison video's frame assembly (src/postprocessing/concat_video.py:26-40; csrc/ghr_compare.h)
 * Added without an ABI_VERSION bump: two new functions, no existing struct or signature changed.
 * ghr_cmp_over_white: rgba [n_pixels][4] -> rgb [n_pixels][3], Pillow's paste of the image over opaque white through its own
 * alpha: per colour byte c of a pixel with alpha a, t = c a + 255 (255 - a) + 128 and out = ((t >> 8) + t) >> 8; alpha is dropped.
 * Four pixels per thread with one 16-B load and three dword stores when rgba is 16-B and rgb 4-B aligned, single bytes otherwise:
 * the same bytes either way.
 * ghr_cmp_strip: out [h][3 w][3] = gt | window | render in one launch.  gt and render are [h][w][3]; preview [ph][pw][3] is the
 * strand render already resized.  Pixel (y, x) of the window is preview pixel (y + crop_top - pad_top, x + crop_left - pad_left),
 * or zero where that lies outside [0, ph) x [0, pw): torchvision's CenterCrop, which pads an axis with black up to the window's
 * length when the image is shorter there (pad_left / pad_top of it before the image) and then cuts at crop_left / crop_top.  The
 * padded image is max(pw, w) x max(ph, h): a padding that reaches past it or a window that does not lie inside it is refused.
 * Dword accesses for the outer panels when w % 4 == 0 and gt, render and out are 4-B aligned, single bytes otherwise: the same
 * bytes either way.
 * Both refuse, with GHR_E_INVALID and a ghr_last_error() text: a NULL pointer, a size < 1, an output that overlaps an input, an
 * image too large for the launch grid.  A refused call launches nothing.  Integer arithmetic alone: the same input gives the same
 * bytes on every run. */
int ghr_cmp_over_white(void* stream, int64_t n_pixels, const uint8_t* rgba, uint8_t* rgb);
int ghr_cmp_strip(void* stream, int32_t w, int32_t h, const uint8_t* gt, const uint8_t* preview, int32_t pw, int32_t ph,
                  int32_t pad_left, int32_t pad_top, int32_t crop_left, int32_t crop_top, const uint8_t* render, uint8_t* out);

/* ---- the textured strand generator between its networks (csrc/ghr_texstrands.h)
 * Smax roots on the scalp with, per root r, the bilinear taps of its UV in a T x T texture made once on the host in float64:
 * x0, y0 [Smax] int32 and fx, fy [Smax] float32.  Tap k = 0..3 is texel (x0 + (k & 1), y0 + (k >> 1)) with weight (1-fx)(1-fy),
 * fx(1-fy), (1-fx)fy, fx fy; a tap outside 0..T-1 is dropped (padding "zeros"), an in-range tap with weight 0 stays a tap.
 * idx [S] int64 is this call's draw of S <= Smax roots, none twice.  float32, no contraction, the operand order written.
 *
 * ghr_ts_fetch: z [S][C], z[s][c] = ((w0 t0 + w1 t1) + w2 t2) + w3 t3 with t_k = texture[c][y_k][x_k] of root idx[s], the dropped
 *   taps skipped (none left: 0).  texture is [C][T][T].  An idx outside 0..Smax-1 reads nothing and makes its row NaN.
 * ghr_ts_fetch_backward: d_texture [C][T][T], EVERY element assigned (no zero fill by the caller):
 *   d_texture[c][q] = sum, in list order, over list[start[q] .. start[q + 1]) of w_k d_z[pos[r]][c], entry = 4 r + k, skipping
 *   roots with pos[r] = -1.  start [T T + 1] and list [list_len <= 4 Smax] are the static inverted lists: for texel q = y T + x the
 *   (root, tap) pairs that touch it, ascending.  pos [Smax] int32 is scratch the call fills: -1, then pos[idx[s]] = s.  No
 *   floating-point atomics: two calls, or a permuted idx with d_z permuted to match, give the same bits.
 * ghr_ts_world: v [S][n][3] decoded local segments -> p [S][n + 1][3] world points and (p_local may be NULL) the local ones:
 *   p_local[s][j] = (sum_{i < j} v[s][i]) inv_scale, p[s][j] = origins[idx[s]] + M p_local[s][j], M = local2world[idx[s]] row-major,
 *   the product bracketed ((M0 x + M1 y) + M2 z); the sum in the chunked scan order of ghr_sds_local.
 * ghr_ts_world_backward: d_v[s][i] = (M^T sum_{j > i} d_p[s][j] + sum_{j > i} d_p_local[s][j]) inv_scale; either cotangent may be
 *   NULL, not both.
 * All refuse, with GHR_E_INVALID and a ghr_last_error() text before the runtime is touched: a NULL pointer, S < 1, S > Smax,
 * T < 1, C < 1, n < 1, list_len outside 0 .. 4 Smax, sizes beyond 32-bit indexing. */
int ghr_ts_fetch(void* stream, int32_t Smax, int32_t S, int32_t T, int32_t C, const float* texture, const int32_t* x0,
                 const int32_t* y0, const float* fx, const float* fy, const int64_t* idx, float* z);
int ghr_ts_fetch_backward(void* stream, int32_t Smax, int32_t S, int32_t T, int32_t C, const float* fx, const float* fy,
                          const int32_t* start, const int32_t* list, int32_t list_len, const int64_t* idx, const float* d_z,
                          int32_t* pos, float* d_texture);
int ghr_ts_world(void* stream, int32_t Smax, int32_t S, int32_t n, const float* v, const float* local2world, const float* origins,
                 const int64_t* idx, float inv_scale, float* p, float* p_local);
int ghr_ts_world_backward(void* stream, int32_t Smax, int32_t S, int32_t n, const float* local2world, const int64_t* idx,
                          float inv_scale, const float* d_p, const float* d_p_local, float* d_v);

/* ---- guiding strands of the textured generator (csrc/ghr_guides.h)
 * uvs [S][2] are the UVs of one draw's roots, the N guides first; z_g [N][C] the guides' fetched latent rows, v_g [N][n][3] their
 * decoded local segments.  float32, no contraction, the operand order of csrc/ghr_sds.h's per-element functions.
 *
 * ghr_guides_blend: for every s < S the four nearest guides g < N in UV under (d2 ascending, g ascending) -> nbr [S][4], and
 *   their normalised inverse-distance weights w [S][4]; for every guide its csim / alpha [N] from its OWN four neighbours'
 *   segment vectors; alpha_s [S] = sum_k w_k alpha[nbr_k]; z [S][C] row-major: z[s] = z_g[s] for s < N, else
 *   z_g[nbr_0] alpha_s + (sum_k w_k z_g[nbr_k]) (1 - alpha_s).  start [N + 1] / list [4 S]: per guide the 4 s + k that chose
 *   it, ASCENDING.  count [N] and unsorted [4 S] are scratch the call fills (count is zero again on return).
 * ghr_guides_blend_backward: from the forward's buffers and d_z [S][C]: d_zg [N][C] (the guide's own row first, then the
 *   interpolated rows of its list in order) and, unless NULL, d_vg [N][n][3] (through alpha_s, alpha and csim).  dalpha_s [S]
 *   and d_csim [N] are scratch.  No floating-point atomics: two calls give the same bits.
 * Both refuse, with GHR_E_INVALID and a ghr_last_error() text before the runtime is touched: N < 4, S < N, n < 1, C < 1, a NULL
 * pointer (d_vg excepted), sizes beyond 32-bit indexing. */
int ghr_guides_blend(void* stream, int32_t S, int32_t N, int32_t n, int32_t C, const float* uvs, const float* z_g, const float* v_g,
                     int32_t* nbr, float* w, float* csim, float* alpha, float* alpha_s, int32_t* count, int32_t* start,
                     int32_t* unsorted, int32_t* list, float* z);
int ghr_guides_blend_backward(void* stream, int32_t S, int32_t N, int32_t n, int32_t C, const float* z_g, const float* v_g,
                              const int32_t* nbr, const float* w, const float* csim, const float* alpha_s, const int32_t* start,
                              const int32_t* list, const float* d_z, float* dalpha_s, float* d_csim, float* d_zg, float* d_vg);

/* ---- growing strands through the orientation field of a hair-point cloud (csrc/ghr_field.h)
 * Added without an ABI_VERSION bump: five new functions, no existing struct or signature changed.
 * The definition of the field (rho, v, c, n at a point under a heading: sequential fp32 sums over the points inside the radius in
 * ascending key-ordered position), of a strand's trace and of the resampling is the one at the top of csrc/ghr_field.h.  A
 * query's and a strand's bits depend on nothing but the cloud, its order and their own arguments.
 * Sequence: ghr_knn_keys on the points over their own bounds; the caller sorts the keys (stable) and passes the permutation;
 * ghr_field_build (block boxes and the payload in sorted order) fills ws, which ghr_field_query / ghr_field_trace then only read.
 * ghr_field_build: points / directions / colors [P][3], weights [P], order [P] int64; ws: ghr_field_workspace_size(P) bytes.
 * ghr_field_query: x / t [Q][3]; r2 the squared radius; rho [Q], v [Q][3], c [Q][3], n [Q] int32: every element written.
 * ghr_field_trace: roots / normals [S][3]; path [S][M + 1][3], steps [S] int32, rgb [S][3]: every element written.
 * query_order [Q] / root_order [S] (int64) may be NULL; otherwise a permutation: lane i of the launch takes row order[i] and
 * writes that row, so rows that are near each other share a wave (speed only; the caller sorts them by their ghr_knn_keys in the
 * cloud's bounds).
 * ghr_strands_resample: path [S][M + 1][3], steps [S] -> out [S][L][3].
 * Refused, with GHR_E_INVALID and a ghr_last_error() text before the runtime is touched: P < 1, Q or S < 0, M < 1, L < 2, r2 <= 0
 * or not finite, h <= 0, rho_min <= 0, beta outside [0, 1], max_coast < 0, a NULL buffer (the two orders excepted), sizes beyond
 * 32-bit indexing.  Q == 0 / S == 0 do nothing. */
int ghr_field_workspace_size(int64_t P, size_t* bytes);
int ghr_field_build(void* stream, int64_t P, const float* points, const int64_t* order, const float* directions, const float* weights,
                    const float* colors, void* ws);
int ghr_field_query(void* stream, int64_t P, const void* ws, int64_t Q, const float* x, const float* t, const int64_t* query_order,
                    float r2, float* rho, float* v, float* c, int32_t* n);
int ghr_field_trace(void* stream, int64_t P, const void* ws, int64_t S, const float* roots, const float* normals,
                    const int64_t* root_order, int32_t M, float r2, float h, float beta, float rho_min, int32_t max_coast, float* path,
                    int32_t* steps, float* rgb);
int ghr_strands_resample(void* stream, int64_t S, int32_t M, int32_t L, const float* path, const int32_t* steps, float* out);

/* ---- the guarded trace: strands grown around the head mesh (csrc/ghr_grow.h)
 * Added without an ABI_VERSION bump: one new function, no existing struct or signature changed.
 * ghr_field_trace with the head mesh asked at every step: where that trace sets x += h t, y = x + h t is given to
 * ghr_mesh_closest's closest point and ghr_mesh_contains' containment; a y whose signed distance is below margin is projected to
 * margin above its closest point and the heading's component into the surface is removed (the definition is at the top of
 * csrc/ghr_grow.h).  A strand's bits depend on nothing but the cloud, the mesh and the strand's own arguments.
 * ws: a field workspace after ghr_field_build; tris_header / tris_dev: the triangle blob of ghr_mesh_tris_build (device copy);
 * grid_header / grid_dev: the grid blob of ghr_mesh_grid_build (device copy); root_order as ghr_field_trace's (may be NULL).
 * path [S][M + 1][3], steps [S] int32, rgb [S][3], contacts [S] int32 (contact steps), stop [S] bytes (0: ran out of M, 1: coasted
 * out of support, 2: met the head head-on): every element written.
 * Refused, with GHR_E_INVALID and a ghr_last_error() text before the runtime is touched: everything ghr_field_trace refuses,
 * margin <= 0 or not finite, a NULL contacts / stop, a NULL header or blob, a header whose magic or sizes are not its kind's.
 * S == 0 does nothing. */
int ghr_field_trace_guarded(void* stream, int64_t P, const void* ws, const ghr_mesh_tris* tris_header, const void* tris_dev,
                            const ghr_mesh_grid* grid_header, const void* grid_dev, int64_t S, const float* roots, const float* normals,
                            const int64_t* root_order, int32_t M, float r2, float h, float beta, float rho_min, int32_t max_coast,
                            float margin, float* path, int32_t* steps, float* rgb, int32_t* contacts, uint8_t* stop);

/* ---- the strand shape term: stretch, bend, neighbour coherence of explicit strands (csrc/ghr_shape.h)
 * Added without an ABI_VERSION bump: three new functions, no existing struct or signature changed.
 * The definition -- the three means, the dead rule, the order of every sum -- is at the top of csrc/ghr_shape.h; a result's bits
 * depend on the inputs alone.
 * ghr_shape_neighbours: roots [S][3] -> nbr [S][4] int32: the 4 nearest OTHER roots by squared distance, ascending, ties to the
 * lower index; -1 where the squared distance exceeds r2 (+inf: no cut) or fewer than 4 other roots exist.  Every element written.
 * ghr_shape_forward: dirs [S][n][3], rest [S] (> 0), nbr [S][4] (another strand or -1), M the number of entries of nbr that are
 * >= 0 -> partial [S][3] (the per-strand sums) and E [3] (the means): every element written.
 * ghr_shape_backward: start [S + 1] / list [M]: per strand the entries 4 t + k with nbr[t][k] == s, ascending; dE [3] on the
 * device -> d_dirs [S][n][3], every element assigned.  An entry of nbr or list outside [0, S) is skipped, and a range of start that
 * does not lie inside the M entries of list is read as empty.
 * Refused, with GHR_E_INVALID and a ghr_last_error() text before the runtime is touched: S < 0, n < 1, M < 0 or > 4 S, r2 <= 0 or
 * NaN, a NULL buffer, sizes beyond 32-bit indexing.  S == 0 does nothing. */
int ghr_shape_neighbours(void* stream, int32_t S, const float* roots, float r2, int32_t* nbr);
int ghr_shape_forward(void* stream, int32_t S, int32_t n, const float* dirs, const float* rest, const int32_t* nbr, int64_t M,
                      float* partial, float* E);
int ghr_shape_backward(void* stream, int32_t S, int32_t n, const float* dirs, const float* rest, const int32_t* nbr, const int32_t* start,
                       const int32_t* list, int64_t M, const float* dE, float* d_dirs);

/* ---- groom upsampling: child strands blended from guide strands (csrc/ghr_upsample.h)
 * Added without an ABI_VERSION bump: two new functions, no existing struct or signature changed.  Forward only.
 * The definition -- the neighbour rule, the similarity gate, the weights, the order of every sum -- is at the top of
 * csrc/ghr_upsample.h; a result's bits depend on the inputs alone.
 * ghr_upsample_neighbours: guide_roots [G][3], child_origins [N][3] -> nbr [N][4] int32: the 4 nearest guides of every child by
 * squared distance, ascending, ties to the lower index, and nd2 [N][4] their squared distances; -1 and +inf where the squared
 * distance exceeds r2 (+inf: no cut) or fewer than 4 guides exist.  Every element written.
 * ghr_upsample_blend: gp [G][L][3] the guides' points, gM [G][3][3] their local2world frames (row-major), gf [G][F] features (NULL
 * when F == 0), co [N][3] / cM [N][3][3] the children's origins and frames, nbr / nd2 as above (the leading entries inside [0, G)
 * are a child's list; any other value ends it and is never dereferenced), eps2, tau and gate (0: every similarity weight is 1)
 * -> out [N][L][3], w [N][4], of [N][F] (NULL when F == 0), valid [N] uint8: every element written.
 * Refused, with GHR_E_INVALID and a ghr_last_error() text before the runtime is touched: G < 1, N < 0, L < 2, F < 0, r2 <= 0 or
 * NaN, eps2 <= 0 or not finite, tau outside [-1, 1) while gate is set, a NULL buffer (gf and of may be NULL when F == 0), sizes
 * beyond 32-bit indexing.  N == 0 does nothing. */
int ghr_upsample_neighbours(void* stream, int32_t G, const float* guide_roots, int32_t N, const float* child_origins, float r2,
                            int32_t* nbr, float* nd2);
int ghr_upsample_blend(void* stream, int32_t G, int32_t L, const float* gp, const float* gM, const float* gf, int32_t F, int32_t N,
                       const float* co, const float* cM, const int32_t* nbr, const float* nd2, float eps2, float tau, int32_t gate,
                       float* out, float* w, float* of, uint8_t* valid);

/* Introspection for tests (device pointers into the workspaces; layout is otherwise private). */
typedef struct ghr_ws_view {
    const float* rec;          /* [P][16]: x, y, conic a, b, c, opacity, features[10] */
    const float* depths;       /* [P] */
    const uint32_t* rects;     /* [P][4]: (xmin | xmax<<16), (ymin | ymax<<16), first gradient slot = [2] + [3] */
    const float* cov3D;        /* [P][6] (mode B) or NULL */
    const float* final_T;      /* [H*W] */
    const uint32_t* n_contrib; /* [H*W] */
    const uint32_t* tile_start;/* [T+1] exclusive scan of per-tile instance counts == ranges */
    const uint64_t* keys;      /* [R] per-tile sorted (depth_bits << 32 | gaussian idx) */
    const uint32_t* point_list;/* [R] */
} ghr_ws_view;
int ghr_ws_inspect(int32_t P, int32_t W, int32_t H, int32_t mode_b, uint32_t R, const void* geom_ws,
                   const void* img_ws, const void* bin_ws, ghr_ws_view* out);

#ifdef __cplusplus
}
#endif
#endif /* GHR_H */
