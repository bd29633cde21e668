// ghr_capi.hip -- C ABI of libghr_hip.so (declared in include/ghr.h).  Host-side orchestration only:
// workspace carving, argument checks, kernel launches on the caller's stream.  Replaces
// R:rasterize_points.cu (torch glue) + R:cuda_rasterizer/rasterizer_impl.cu:155-441 (state carving, forward, backward).
#include "../../include/ghr.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "ghr_binning.h"
#include "ghr_device.h"
#include "ghr_adam.h"
#include "ghr_camera.h"
#include "ghr_geom_bwd.h"
#include "ghr_knn.h"
#include "ghr_nn.h"
#include "ghr_field.h"
#include "ghr_loss.h"
#include "ghr_eval.h"
#include "ghr_orient.h"
#include "ghr_gt.h"
#include "ghr_compare.h"
#include "ghr_preprocess.h"
#include "ghr_project.h"
#include "ghr_render_bwd.h"
#include "ghr_render_bwd2.h"
#include "ghr_render_bwd3.h"
#include "ghr_render_fwd.h"
#include "ghr_strands.h"
#include "ghr_latent.h"
#include "ghr_shared.h"
#include "ghr_mesh.h"
#include "ghr_meshdist.h"
#include "ghr_grow.h"
#include "ghr_shape.h"
#include "ghr_upsample.h"
#include "ghr_visibility.h"
#include "ghr_strandview.h"
#include "ghr_capture.h"
#include "ghr_sds.h"
#include "ghr_texstrands.h"
#include "ghr_guides.h"

namespace {

thread_local char g_err[512] = "";
// Process-wide (NOT thread_local): torch's autograd engine calls ghr_backward from its own worker thread.
hipEvent_t g_ev[4] = {nullptr, nullptr, nullptr, nullptr};  // fwd start/stop, bwd start/stop

// K8 variant (same gradient-line format; GHR_K8=cell selects the fallback, read at every call so that a test can switch):
//   2 = cell-list form (k_render_bwd_cells, default): one wave per 4x4 cell from the forward pass's hit masks, records
//       gathered straight into LDS two chunks ahead;
//   0 = cell-group form (k_render_bwd, round 1): lane = pixel, 16-lane butterflies; the fallback where the cell-list
//       form's 32-bit byte offsets do not reach (b3_fits: >= 2^26 rows / instances).
int g_deterministic = 0;  // ghr_set_deterministic

// Which per-tile kernels take their tiles in k_tile_scan's heaviest-first order instead of the XCD-interleaved raster
// order (xcd_tile): bit 0 tile sort, bit 1 K7, bit 2 K8.  GHR_TILE_ORDER=<mask> overrides (A/B knob, like GHR_K8).
#ifndef GHR_TILE_ORDER_DEFAULT
#define GHR_TILE_ORDER_DEFAULT 3
#endif
const uint32_t* order_ptr(const uint32_t* p, int bit)
{
    const char* e = std::getenv("GHR_TILE_ORDER");
    const int mask = e ? std::atoi(e) : GHR_TILE_ORDER_DEFAULT;
    return (mask >> bit) & 1 ? p : nullptr;
}

int k8_variant()
{
    const char* e = std::getenv("GHR_K8");
    return (e && std::strcmp(e, "cell") == 0) ? 0 : 2;
}

#define GHR_E_DETERMINISTIC_MSG "ghr_set_deterministic(1) cannot be honoured at this size (the ordered walk needs 32-bit byte offsets: < 2^26 rows / instances)"

int fail(int code, const char* fmt, const char* detail = "")
{
    std::snprintf(g_err, sizeof(g_err), fmt, detail);
    return code;
}

#define GHR_HIP(expr)                                                                     \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) return fail(GHR_E_HIP, #expr ": %s", hipGetErrorString(e_)); \
    } while (0)

// Device-visible alias of the host word that receives num_rendered, when that word lives in pinned (hipHostMalloc /
// hipHostRegister) memory; nullptr for pageable memory, which then gets a stream-ordered 4-byte copy instead.
uint32_t* mapped_word(uint32_t* host)
{
    void* dev = nullptr;
    if (hipHostGetDevicePointer(&dev, host, 0) != hipSuccess) {
        (void)hipGetLastError();  // not an error for the caller: fall back to the copy
        return nullptr;
    }
    return (uint32_t*)dev;
}

constexpr size_t ALIGN = 256;
inline size_t up(size_t x) { return (x + ALIGN - 1) / ALIGN * ALIGN; }

// Sub-allocation of the three caller-owned workspaces (cf. obtain()/fromChunk, rasterizer_impl.h:21-73).
struct Geom {
    ghr::f4* rec;
    float* depths;
    ghr::rect4* rects;
    uint32_t* slot_blk;  // [ceil(P/256)]
    uint32_t* pos;       // [P][GHR_BIG_RECT]: place of each small-rect instance in its tile's list (count_tiles)
    float* cov3D;
};
struct Img {
    float* final_T;
    uint32_t* n_contrib;
    uint32_t* tile_count;  // [2][T]: per-tile instance counts of the small / the big rects; [1] then the big rects' append cursors
    uint32_t* tile_start;  // [T+1]
    uint32_t* small_cnt;   // [T]: instances of small rects per tile (k_tile_scan; k_scatter appends the big rects' behind them)
    uint32_t* R_dev;
    uint32_t* cell_last;   // [16 T]: largest n_contrib of each 4x4-pixel cell
    uint32_t* tile_order;  // [xcd_grid(T)]: tile of each workgroup of the per-tile kernels (k_tile_scan: heaviest first)
};
struct Bin {
    uint64_t* keys;
    uint32_t* point_list;
    unsigned long long* cell_mask;  // [mask_groups(R, T)][16]
    uint32_t* inst_line;            // [R]: gradient line (= list position) of every instance (numbered by rect4_slot)
};

size_t carve_geom(char* base, size_t P, bool mode_b, Geom* g)
{
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += up(bytes); return p; };
    ghr::f4* rec = (ghr::f4*)take(P * 64);
    float* depths = (float*)take(P * 4);
    ghr::rect4* rects = (ghr::rect4*)take(P * 16);
    uint32_t* slot_blk = (uint32_t*)take(((P + GHR_BLOCK - 1) / GHR_BLOCK) * 4);
    uint32_t* pos = (uint32_t*)take(P * 4 * GHR_BIG_RECT);
    // cov3D stays last: an entry that is not told the mode (stage 2, the model calls) carves with mode_b = false and finds every
    // other plane where a mode-B stage 1 put it
    float* cov3D = mode_b ? (float*)take(P * 24) : nullptr;
    if (g) *g = Geom{rec, depths, rects, slot_blk, pos, cov3D};
    return off + ALIGN;
}
size_t carve_img(char* base, size_t N, size_t T, Img* im)
{
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += up(bytes); return p; };
    float* final_T = (float*)take(N * 4);
    uint32_t* n_contrib = (uint32_t*)take(N * 4);
    uint32_t* tile_count = (uint32_t*)take(2 * T * 4);
    uint32_t* tile_start = (uint32_t*)take((T + 1) * 4);
    uint32_t* small_cnt = (uint32_t*)take(T * 4);
    uint32_t* R_dev = (uint32_t*)take(4);
    uint32_t* cell_last = (uint32_t*)take(T * 16 * 4);
    uint32_t* tile_order = (uint32_t*)take((size_t)ghr::xcd_grid((uint32_t)T) * 4);
    if (im) *im = Img{final_T, n_contrib, tile_count, tile_start, small_cnt, R_dev, cell_last, tile_order};
    return off + ALIGN;
}
size_t carve_bin(char* base, size_t R, size_t T, Bin* b)
{
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += up(bytes); return p; };
    uint64_t* keys = (uint64_t*)take(R * 8);
    uint32_t* pl = (uint32_t*)take(R * 4);
    unsigned long long* cm = (unsigned long long*)take(ghr::mask_groups(R, T) * 16 * 8);
    uint32_t* il = (uint32_t*)take(R * 4);
    if (b) *b = Bin{keys, pl, cm, il};
    return off + ALIGN;
}
inline char* align_base(const void* p) { return (char*)(((uintptr_t)p + ALIGN - 1) / ALIGN * ALIGN); }

int check_dims(const ghr_view_args* a)
{
    if (!a) return fail(GHR_E_INVALID, "ghr_view_args is NULL");
    if (a->P < 0 || a->W <= 0 || a->H <= 0) return fail(GHR_E_INVALID, "bad P/W/H");
    if (a->C != GHR_NUM_CHANNELS) return fail(GHR_E_INVALID, "C must equal GHR_NUM_CHANNELS (10)");
    if ((a->W + GHR_TILE - 1) / GHR_TILE > 65535 || (a->H + GHR_TILE - 1) / GHR_TILE > 65535)
        return fail(GHR_E_INVALID, "image too large for 16-bit tile coordinates");
    return GHR_OK;
}

int check_view(const ghr_view_args* a)
{
    if (int rc = check_dims(a)) return rc;
    if (a->P == 0) return GHR_OK;
    if (!a->colors) return fail(GHR_E_NOCOLORS, "For non-RGB, provide precomputed Gaussian colors!");
    if (!a->means3D || !a->opacities || !a->background || !a->viewmatrix || !a->projmatrix)
        return fail(GHR_E_INVALID, "means3D/opacities/background/viewmatrix/projmatrix must be non-NULL");
    if (!a->conic_precomp && !a->cov3D_precomp && !(a->scales && a->rotations))
        return fail(GHR_E_INVALID, "kernel-geometry mode needs cov3D_precomp or scales+rotations");
    return GHR_OK;
}

int finish(hipStream_t s, int debug)
{
    GHR_HIP(hipGetLastError());
    if (debug) GHR_HIP(hipStreamSynchronize(s));
    return GHR_OK;
}

inline int grid_x(int W) { return (W + GHR_TILE - 1) / GHR_TILE; }
inline int n_blocks(int rows) { return (rows + GHR_BLOCK - 1) / GHR_BLOCK; }
inline float focal(int extent, float tan_fov) { return extent / (2.0f * tan_fov); }  // rasterizer_impl.cu:224-225

// A view's three workspaces, carved: every entry point that touches them asks here, so there is one layout.  NULL
// workspaces give NULL members.
struct ViewWs {
    Geom g; Img im; Bin b;
    int gx, gy, T;
};
// `mode_b` (ghr_view_args without conic_precomp: stage 1 stores 3D covariances) decides g.cov3D and nothing else (carve_geom).
ViewWs carve_view(size_t rows, int W, int H, bool mode_b, size_t R, const void* geom_ws, const void* img_ws, const void* bin_ws)
{
    ViewWs w;
    w.gx = grid_x(W); w.gy = grid_x(H); w.T = w.gx * w.gy;
    carve_geom(align_base(geom_ws), rows, mode_b, &w.g);
    carve_img(align_base(img_ws), (size_t)W * H, (size_t)w.T, &w.im);
    carve_bin(align_base(bin_ws), R, (size_t)w.T, &w.b);
    return w;
}

// ---- the steps more than one entry point takes -------------------------------------------------------------------------
// The per-tile counters before a pass's first projection: zero-filled, or -- a recycled workspace, whose counters k_tile_sort
// left at zero -- taken on trust; under `debug` the promise is read back.  `not_zero`: the entry's words for a broken one.
int zero_or_verify_counters(const ViewWs& w, int recycled, int debug, const char* not_zero, hipStream_t s)
{
    const size_t n = 2 * (size_t)w.T;
    if (!recycled) GHR_HIP(hipMemsetAsync(w.im.tile_count, 0, sizeof(uint32_t) * n, s));
    else if (debug) {
        std::vector<uint32_t> h(n);
        GHR_HIP(hipMemcpyAsync(h.data(), w.im.tile_count, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, s));
        GHR_HIP(hipStreamSynchronize(s));
        for (uint32_t v : h) if (v != 0) return fail(GHR_E_INVALID, "%s", not_zero);
    }
    return GHR_OK;
}

// k_tile_scan over the counters of `rows` projected rows; the instance count goes to *R_host (mapped_word)
int tile_scan(const ViewWs& w, int rows, uint32_t* R_host, hipStream_t s)
{
    uint32_t* R_mapped = mapped_word(R_host);
    hipLaunchKernelGGL(ghr::k_tile_scan, dim3(1), dim3(GHR_SCAN_BLOCK), 0, s, w.T, w.im.tile_count, w.im.small_cnt, w.im.tile_start,
                       w.im.R_dev, w.g.slot_blk, n_blocks(rows), R_mapped, w.im.tile_order);
    if (!R_mapped) GHR_HIP(hipMemcpyAsync(R_host, w.im.R_dev, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    return GHR_OK;
}

// ghr_set_deterministic(1) is never dropped silently: the ordered walk exists in the cell-list form only (b3_fits)
bool ordered_walk_refused(size_t rows, uint32_t R, int W, int H) { return g_deterministic && !ghr::b3_fits(rows, R, (size_t)W, (size_t)H); }

// The pixel backward (K8) between the two profile events.  Nothing is launched at R == 0: ghr_render_backward does not
// come here then, ghr_backward_ex does and goes on (k_geom_bwd writes the zero gradients).
int pixel_backward(const ViewWs& w, size_t rows, int W, int H, uint32_t R, const float* bg, const float* dL_dpix, float* ginst,
                   int prezeroed, hipStream_t s)
{
    if (g_ev[2]) GHR_HIP(hipEventRecord(g_ev[2], s));
    if (R > 0) {
        if (ordered_walk_refused(rows, R, W, H)) return fail(GHR_E_INVALID, GHR_E_DETERMINISTIC_MSG);
        const dim3 grid(ghr::xcd_grid((uint32_t)w.T));
        const uint32_t* order = order_ptr(w.im.tile_order, 2);
        if ((g_deterministic || k8_variant() == 2) && ghr::b3_fits(rows, R, (size_t)W, (size_t)H))
            hipLaunchKernelGGL(ghr::k_render_bwd_cells, grid, dim3(GHR_B3_THREADS), 0, s, W, H, w.gx, (uint32_t)w.T, w.im.tile_start,
                               w.b.point_list, w.g.rec, bg, w.im.final_T, w.im.n_contrib, dL_dpix, w.g.rects, ginst, R, w.b.cell_mask,
                               w.im.cell_last, g_deterministic, prezeroed ? 1 : 0, order);
        else
            hipLaunchKernelGGL(ghr::k_render_bwd, grid, dim3(GHR_BLOCK), 0, s, W, H, w.gx, (uint32_t)w.T, w.im.tile_start,
                               w.b.point_list, w.g.rec, bg, w.im.final_T, w.im.n_contrib, dL_dpix, w.g.rects, ginst, R);
    }
    if (g_ev[3]) GHR_HIP(hipEventRecord(g_ev[3], s));
    return GHR_OK;
}

void adam_fused_finish(const ghr_adam_fuse* af, hipStream_t s)
{
    hipLaunchKernelGGL(ghr::k_adam_fused_finish, dim3(1024), dim3(256), 0, s, (long long)af->n, af->p_in, af->m_in, af->v_in,
                       af->p_out, af->m_out, af->v_out, af->state, (const int*)af->flag, af->flag_next);
}

// ---- rules more than one entry point states ------------------------------------------------------------------------------
// The shape of SH features: a degree of 0 .. 3, K = sh_coeffs = (max_sh_degree + 1)^2 coefficients per channel (the kernels'
// 16-B staging of features_rest counts on rows of >= 9 floats), and K covers the degree.
inline bool sh_degree_ok(int degree) { return degree >= 0 && degree <= 3; }
inline bool sh_coeffs_ok(int K) { return K == 1 || K == 4 || K == 9 || K == 16; }
inline bool sh_covers(int degree, int K) { return (degree + 1) * (degree + 1) <= K; }

// the cell masks' 32-bit byte offsets (stage 2)
inline bool cell_masks_fit(uint32_t R, int W, int H) { return ghr::mask_groups(R, (size_t)grid_x(W) * grid_x(H)) * 128 < ((size_t)1 << 32); }
// the densification statistics of the projection backward: all three buffers or none
inline int n_dens(const ghr_model_args* m) { return (m->dens_grad_accum != nullptr) + (m->dens_denom != nullptr) + (m->dens_max_radii2D != nullptr); }
inline bool dens_all_or_none(const ghr_model_args* m) { return n_dens(m) == 0 || n_dens(m) == 3; }
// The projection backward stores nothing in d_features_dc / d_features_rest (they may be NULL) in the factored form -- the SH
// gradients leave as d_rgb (ABI 19) -- and when the call carries the update (ghr_adam_fuse) without earlier views' gradients to add.
inline bool sh_grads_unstored(const ghr_model_args* m, bool factored, int accumulate) { return factored || (m->adam_fuse && !accumulate); }
// ghr_sh_grad_from_views: its sizes, and two views' tables [3 P] must not overlap
inline bool sh_views_sizes_ok(int P, int degree, int K, int n_views, int64_t view_stride, int64_t campos_stride)
{
    return P >= 0 && n_views >= 0 && sh_degree_ok(degree) && sh_coeffs_ok(K) && sh_covers(degree, K) && view_stride >= 0 && campos_stride >= 0;
}
inline bool sh_views_overlap(int P, int n_views, int64_t view_stride) { return n_views > 1 && view_stride < 3 * (int64_t)P; }

}  // namespace

extern "C" {

const char* ghr_last_error(void) { return g_err; }
int ghr_abi_version(void) { return GHR_ABI_VERSION; }

int ghr_forward_sizes(int32_t P, int32_t W, int32_t H, int32_t mode_b, size_t* geom_bytes, size_t* img_bytes)
{
    if (P < 0 || W <= 0 || H <= 0 || !geom_bytes || !img_bytes) return fail(GHR_E_INVALID, "ghr_forward_sizes: bad args");
    const size_t T = (size_t)grid_x(W) * grid_x(H);
    *geom_bytes = carve_geom(nullptr, (size_t)P, mode_b != 0, nullptr);
    *img_bytes = carve_img(nullptr, (size_t)W * H, T, nullptr);
    return GHR_OK;
}

int ghr_binning_size(uint32_t R, int32_t W, int32_t H, size_t* bin_bytes)
{
    if (!bin_bytes || W <= 0 || H <= 0) return fail(GHR_E_INVALID, "ghr_binning_size: bad args");
    *bin_bytes = carve_bin(nullptr, (size_t)R, (size_t)grid_x(W) * grid_x(H), nullptr);
    return GHR_OK;
}

int ghr_forward_stage1(void* stream, const ghr_view_args* a, void* geom_ws, void* img_ws, int32_t* radii,
                       uint32_t* R_host)
{
    if (int rc = check_view(a)) return rc;
    if (!R_host) return fail(GHR_E_INVALID, "R_host is NULL");
    hipStream_t s = (hipStream_t)stream;
    if (a->P == 0) { *R_host = 0; return GHR_OK; }
    if (!geom_ws || !img_ws || !radii) return fail(GHR_E_INVALID, "workspace/radii is NULL");
    const ViewWs w = carve_view((size_t)a->P, a->W, a->H, a->conic_precomp == nullptr, 0, geom_ws, img_ws, nullptr);
    if (int rc = zero_or_verify_counters(w, a->img_ws_recycled, a->debug,
                                         "ghr_view_args.img_ws_recycled is set but the workspace's per-tile counters are not zero", s))
        return rc;
    ghr::PreArgs pa;
    pa.P = a->P; pa.W = a->W; pa.H = a->H; pa.gx = w.gx; pa.gy = w.gy;
    pa.means3D = a->means3D; pa.colors = a->colors; pa.opacities = a->opacities;
    pa.scales = a->scales; pa.rotations = a->rotations;
    pa.cov3D_precomp = a->cov3D_precomp; pa.conic_precomp = a->conic_precomp;
    pa.view = a->viewmatrix; pa.proj = a->projmatrix;
    pa.scale_modifier = a->scale_modifier; pa.tan_fovx = a->tan_fovx; pa.tan_fovy = a->tan_fovy;
    pa.focal_y = focal(a->H, a->tan_fovy); pa.focal_x = focal(a->W, a->tan_fovx);
    pa.rec = w.g.rec; pa.depths = w.g.depths; pa.rects = w.g.rects; pa.cov3D = w.g.cov3D; pa.radii = radii;
    pa.tile_count = w.im.tile_count; pa.slot_blk = w.g.slot_blk; pa.pos = w.g.pos;
    hipLaunchKernelGGL(ghr::k_preprocess, dim3(n_blocks(a->P)), dim3(GHR_BLOCK), 0, s, pa);
    if (int rc = tile_scan(w, a->P, R_host, s)) return rc;
    return finish(s, a->debug);
}

// Each call ghr_view_step composes is a check and a run.  The check launches nothing and touches neither device memory nor
// the HIP runtime; it returns what the entry point refuses.  The run takes checked arguments.  ghr_view_step asks all the
// checks before the first run: a struct that only the last call refuses must not leave five calls' kernels in the stream.
static int check_forward_stage2(const ghr_view_args* a, uint32_t R, const void* geom_ws, const void* img_ws, const void* bin_ws,
                                const float* out_color)
{
    if (int rc = check_dims(a)) return rc;  // stage 2 only reads P, W, H, C, background (+ debug)
    if (!out_color) return fail(GHR_E_INVALID, "out_color is NULL");
    if (a->P > 0 && !a->background) return fail(GHR_E_INVALID, "background is NULL");
    if (a->P == 0) return GHR_OK;
    if (!geom_ws || !img_ws || (R > 0 && !bin_ws)) return fail(GHR_E_INVALID, "workspace is NULL");
    if (!cell_masks_fit(R, a->W, a->H)) return fail(GHR_E_INVALID, "too many instances for the 32-bit offsets of the cell masks");
    return GHR_OK;
}

int ghr_forward_stage2(void* stream, const ghr_view_args* a, uint32_t R, void* geom_ws, void* img_ws, void* bin_ws,
                       float* out_color, float* grad_scratch)
{
    if (int rc = check_forward_stage2(a, R, geom_ws, img_ws, bin_ws, out_color)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (a->P == 0) {
        // Nothing to splat: the reference skips the whole forward and returns the zero-filled image
        // (rasterize_points.cu:70,87); keep that.
        GHR_HIP(hipMemsetAsync(out_color, 0, sizeof(float) * (size_t)a->C * a->W * a->H, s));
        return finish(s, a->debug);
    }
    const ViewWs w = carve_view((size_t)a->P, a->W, a->H, false, R, geom_ws, img_ws, bin_ws);
    const Geom& g = w.g; const Img& im = w.im; const Bin& b = w.b;
    const int gx = w.gx, T = w.T;
    if (R > 0) {
        // append cursors are 0 on entry: k_tile_scan leaves them there and k_tile_sort resets them (replay-safe)
        const int scatter_blocks = (a->P + 127) / 128;  // a wave serves 32 Gaussians
        hipLaunchKernelGGL(ghr::k_scatter, dim3(scatter_blocks), dim3(GHR_BLOCK), 0, s, a->P, gx,
                           g.rects, g.slot_blk, g.depths, im.tile_start, im.tile_count, (uint32_t)T, im.small_cnt, g.pos, b.keys, R);
        // dense scenes (long lists on average) first get their dense tiles sorted in big LDS blocks; the regular kernel
        // then passes those by.  R is the capacity here, an upper bound of the count: a guess that is too high only
        // costs an idle 3-us launch.
        const bool dense = (size_t)R >= (size_t)GHR_SORT_BIG_MIN_AVG * (size_t)T;
        if (dense) {
            // (round 6) lists of 1025 .. 4096 keys by 512-thread workgroups with the register-blocked network, longer ones
            // by the 1024-thread kernel; a workgroup looks at up to GHR_SORT_WALK_MAX tiles
            // by up to GHR_SORT_WALK_MAX entries of k_tile_scan's heaviest-first order (the dense tiles sit at its front: dealt
            // out evenly) or, without the order, of the raster order
            const uint32_t* order = order_ptr(im.tile_order, 0);
            const uint32_t order_len = ghr::xcd_grid((uint32_t)T);
            const unsigned walk = ((unsigned)(((order ? order_len : (uint32_t)T) + GHR_SORT_WALK_MAX - 1) / GHR_SORT_WALK_MAX) + 7u) & ~7u;
            uint32_t big_min = GHR_SORT_CAP;
            if (std::getenv("GHR_NO_SORT_MID") == nullptr) {
                // (every workgroup resident: 256 CUs x 8 resp. 4 workgroups)
                uint32_t lo = GHR_SORT_CAP;
                if (GHR_SORT_MID_SPLIT) {
                    hipLaunchKernelGGL(ghr::k_tile_sort_mid<256>, dim3(std::max(2048u, walk)), dim3(256), 0, s, (uint32_t)T,
                                       im.tile_start, b.keys, b.point_list, R, im.tile_count, g.rects, b.inst_line, gx, order,
                                       order_len, lo);
                    lo = 2048u;
                }
                hipLaunchKernelGGL(ghr::k_tile_sort_mid<512>, dim3(std::max(1024u, walk)), dim3(512), 0, s, (uint32_t)T,
                                   im.tile_start, b.keys, b.point_list, R, im.tile_count, g.rects, b.inst_line, gx, order,
                                   order_len, lo);
                big_min = GHR_SORT_MID_CAP;
            }
            hipLaunchKernelGGL(ghr::k_tile_sort_big, dim3(std::max(512u, walk)), dim3(GHR_SORT_BIG_BLOCK), 0, s, (uint32_t)T,
                               im.tile_start, b.keys, b.point_list, R, im.tile_count, g.rects, b.inst_line, gx, big_min, order,
                               order_len);
        }
        hipLaunchKernelGGL(ghr::k_tile_sort<1024>, dim3(ghr::xcd_grid((uint32_t)T)), dim3(GHR_SORT_BLOCK), 0, s, (uint32_t)T,
                           im.tile_start, b.keys, b.point_list, R, im.tile_count, g.rects, b.inst_line, gx,
                           order_ptr(im.tile_order, 0));
    }
    if (g_ev[0]) GHR_HIP(hipEventRecord(g_ev[0], s));
    // GHR_K7_WALK=mask: test / measurement knob (read per call) -- the cells walk their hits bit by bit from the 64-bit masks
    // instead of from hit lists; same outputs bit for bit.  The list walk carries list positions times 16 in 32 bits; a
    // tile's list holds a Gaussian at most once, so below 2^28 Gaussians that cannot wrap (beyond: the mask walk).
    const char* walk = std::getenv("GHR_K7_WALK");
    const bool lists = a->P < (1 << 28) && !(walk != nullptr && std::strcmp(walk, "mask") == 0);
    const auto k7 = lists ? ghr::k_render_fwd<true> : ghr::k_render_fwd<false>;
    hipLaunchKernelGGL(k7, dim3(ghr::xcd_grid((uint32_t)T)), dim3(GHR_BLOCK), 0, s, a->W, a->H, gx,
                       (uint32_t)T, im.tile_start, b.point_list, g.rec, a->background, out_color, im.final_T,
                       im.n_contrib, R, b.cell_mask, im.cell_last, order_ptr(im.tile_order, 1), grad_scratch);
    if (g_ev[1]) GHR_HIP(hipEventRecord(g_ev[1], s));
    return finish(s, a->debug);
}

int ghr_backward(void* stream, const ghr_view_args* a, uint32_t R, const int32_t* radii, const void* geom_ws,
                 const void* img_ws, const void* bin_ws, const float* dL_dpix, float* grad_scratch,
                 float* dL_dmeans2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolors, float* dL_dmeans3D,
                 float* dL_dcov3D, float* dL_dscales, float* dL_drotations, int32_t prezeroed)
{
    return ghr_backward_ex(stream, a, R, radii, geom_ws, img_ws, bin_ws, dL_dpix, grad_scratch, dL_dmeans2D, dL_dconic,
                           dL_dopacity, dL_dcolors, dL_dmeans3D, dL_dcov3D, dL_dscales, dL_drotations, prezeroed, nullptr);
}

int ghr_backward_ex(void* stream, const ghr_view_args* a, uint32_t R, const int32_t* radii, const void* geom_ws,
                    const void* img_ws, const void* bin_ws, const float* dL_dpix, float* grad_scratch,
                    float* dL_dmeans2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolors, float* dL_dmeans3D,
                    float* dL_dcov3D, float* dL_dscales, float* dL_drotations, int32_t prezeroed, float* dL_dconic3)
{
    // backward reads colours / opacity from the packed records in geom_ws, not from `a`
    if (int rc = check_dims(a)) return rc;
    if (a->P > 0 && (!a->means3D || !a->viewmatrix || !a->projmatrix || !a->background))
        return fail(GHR_E_INVALID, "ghr_backward: means3D/viewmatrix/projmatrix/background must be non-NULL");
    if (a->P > 0 && !a->conic_precomp && !a->cov3D_precomp && !(a->scales && a->rotations))
        return fail(GHR_E_INVALID, "kernel-geometry mode needs cov3D_precomp or scales+rotations");
    hipStream_t s = (hipStream_t)stream;
    if (a->P == 0) return GHR_OK;
    if (!radii || !geom_ws || !img_ws || (R > 0 && !bin_ws) || !dL_dpix || (R > 0 && !grad_scratch) || !dL_dmeans2D ||
        !dL_dconic || !dL_dopacity || !dL_dcolors || !dL_dmeans3D || !dL_dcov3D || !dL_dscales || !dL_drotations)
        return fail(GHR_E_INVALID, "ghr_backward: NULL buffer");
    const ViewWs w = carve_view((size_t)a->P, a->W, a->H, a->conic_precomp == nullptr, R, geom_ws, img_ws, bin_ws);
    if (int rc = pixel_backward(w, (size_t)a->P, a->W, a->H, R, a->background, dL_dpix, grad_scratch, prezeroed, s)) return rc;
    ghr::GeomBwdArgs ga;
    ga.P = a->P; ga.means3D = a->means3D; ga.radii = radii; ga.scales = a->scales; ga.rotations = a->rotations;
    ga.cov3D = w.g.cov3D; ga.conic_precomp = a->conic_precomp; ga.view = a->viewmatrix; ga.proj = a->projmatrix;
    ga.scale_modifier = a->scale_modifier; ga.tan_fovx = a->tan_fovx; ga.tan_fovy = a->tan_fovy;
    ga.focal_y = focal(a->H, a->tan_fovy); ga.focal_x = focal(a->W, a->tan_fovx);
    ga.ginst = grad_scratch; ga.inst_line = w.b.inst_line; ga.ginst_rows = R;
    ga.rects = w.g.rects; ga.rec = w.g.rec; ga.half_w = 0.5f * a->W; ga.half_h = 0.5f * a->H;
    ga.dL_dmeans2D = dL_dmeans2D; ga.dL_dconic = dL_dconic; ga.dL_dconic3 = dL_dconic3; ga.dL_dopacity = dL_dopacity; ga.dL_dcolors = dL_dcolors;
    ga.dL_dmeans3D = dL_dmeans3D; ga.dL_dcov3D = dL_dcov3D; ga.dL_dscales = dL_dscales; ga.dL_drots = dL_drotations;
    hipLaunchKernelGGL(ghr::k_geom_bwd, dim3((a->P + GHR_BLOCK - 1) / GHR_BLOCK), dim3(GHR_BLOCK), 0, s, ga);
    return finish(s, a->debug);
}

namespace {
int fill_model(const ghr_model_args* m, ghr::ModelArgs* a)
{
    if (!m) return fail(GHR_E_INVALID, "ghr_model_args is NULL");
    if (m->P < 0 || m->W <= 0 || m->H <= 0) return fail(GHR_E_INVALID, "bad P/W/H");
    if (!sh_degree_ok(m->sh_degree) || !sh_covers(m->sh_degree, m->sh_coeffs) || m->sh_coeffs > GHR_SH_MAX)
        return fail(GHR_E_INVALID, "bad sh_degree / sh_coeffs");
    if (!sh_coeffs_ok(m->sh_coeffs))
        return fail(GHR_E_INVALID, "ghr_model_args: sh_coeffs must be (max_sh_degree + 1)^2, i.e. 1, 4, 9 or 16");
    if (m->mode != 0 && m->mode != 1) return fail(GHR_E_INVALID, "ghr_model_args: mode must be 0 or 1");
    if (m->row0 < 0 || (m->row0 & (GHR_BLOCK - 1))) return fail(GHR_E_INVALID, "ghr_model_args: row0 must be a multiple of 256");
    const bool need_act = m->mode == 0;  // mode 1: opacity / label / confidence pointers are optional
    if (m->P > 0 && (!m->xyz || !m->log_scales || !m->rotations || (need_act && (!m->opacity_logit || !m->label_logit ||
                     !m->orient_conf_log)) || !m->features_dc || (m->sh_coeffs > 1 && !m->features_rest) ||
                     !m->viewmatrix || !m->projmatrix || !m->campos))
        return fail(GHR_E_INVALID, "ghr_model_args: NULL parameter tensor");
    a->P = m->P; a->W = m->W; a->H = m->H; a->gx = grid_x(m->W); a->gy = grid_x(m->H);
    a->sh_degree = m->sh_degree; a->sh_coeffs = m->sh_coeffs;
    a->mode = m->mode; a->row0 = m->row0;
    a->xyz = m->xyz; a->log_scales = m->log_scales; a->rotations = m->rotations;
    a->opacity_logit = m->opacity_logit; a->label_logit = m->label_logit; a->orient_conf_log = m->orient_conf_log;
    a->dir3d = m->mode == 1 ? m->dir3d : nullptr;
    a->const_opacity = m->const_opacity; a->const_label = m->const_label; a->const_conf = m->const_conf;
    a->features_dc = m->features_dc; a->features_rest = m->features_rest;
    a->view = m->viewmatrix; a->proj = m->projmatrix; a->campos = m->campos;
    a->scale_modifier = m->scale_modifier; a->tan_fovx = m->tan_fovx; a->tan_fovy = m->tan_fovy;
    a->focal_y = focal(m->H, m->tan_fovy); a->focal_x = focal(m->W, m->tan_fovx);
    a->conic_eps = m->conic_eps;
    if ((m->fovx_dev != nullptr) != (m->fovy_dev != nullptr)) return fail(GHR_E_INVALID, "ghr_model_args: fovx_dev and fovy_dev: both or neither");
    a->fovx = m->fovx_dev; a->fovy = m->fovy_dev;
    a->rec = nullptr; a->depths = nullptr; a->rects = nullptr; a->radii = nullptr; a->means2D = nullptr;
    a->tile_count = nullptr; a->slot_blk = nullptr; a->pos = nullptr;
    return GHR_OK;
}
// The checks and the host-side table of a backward call that carries the optimizer update (ghr_adam_fuse): which group each
// raw-parameter array of `a` lies in and its learning rate.  Launches nothing (ghr_view_step validates with it up front).
int fill_adam_fuse(const ghr::ModelArgs& a, const ghr_adam_fuse* af, int32_t accumulate, const int32_t* nan_flag,
                   ghr::ModelGrads* mg)
{
    if (a.mode == 1 && accumulate) return fail(GHR_E_INVALID, "ghr_adam_fuse: a strand segment carries the update only as the step's single view");
    if (af->n <= 0 || !af->p_in || !af->m_in || !af->v_in || !af->p_out || !af->m_out || !af->v_out || !af->state || !af->flag ||
        !af->flag_next || af->n_groups <= 0 || af->n_groups > GHR_ADAM_MAX_GROUPS || !af->group_end_host || !af->lr_host)
        return fail(GHR_E_INVALID, "ghr_adam_fuse: NULL buffer / bad group table");
    if (nan_flag != af->flag) return fail(GHR_E_INVALID, "ghr_adam_fuse: nan_flag of the backward call must be adam_fuse->flag");
    const float* arrays[GHR_ADAM_FUSE_ARRAYS] = {a.xyz, a.log_scales, a.rotations, a.opacity_logit, a.label_logit,
                                                 a.orient_conf_log, a.features_dc, a.features_rest};
    // (mode 1, a strand segment: only the SH features are raw parameters of the optimizer; the other groups of its flat
    // buffer -- strand directions, confidence -- get their gradients through autograd and are stepped by the caller)
    const long long w6 = a.mode == 1 ? 0 : 1;
    const long long width[GHR_ADAM_FUSE_ARRAYS] = {3 * w6, 3 * w6, 4 * w6, w6, w6, w6, 3, 3LL * (a.sh_coeffs - 1)};
    long long covered = 0;
    for (int k = 0; k < GHR_ADAM_FUSE_ARRAYS; k++) {
        const long long len = width[k] * a.P;
        if (len == 0) { mg->adam.lr[k] = 0.f; mg->adam.group[k] = 0; continue; }
        const long long off = arrays[k] - af->p_in;
        if (off < 0 || off + len > af->n)
            return fail(GHR_E_INVALID, "ghr_adam_fuse: a raw-parameter array does not lie inside p_in");
        int gi = 0;
        while (gi < af->n_groups - 1 && off >= af->group_end_host[gi]) gi++;
        if (off + len > af->group_end_host[gi])
            return fail(GHR_E_INVALID, "ghr_adam_fuse: a raw-parameter array straddles two parameter groups");
        mg->adam.group[k] = gi;
        mg->adam.lr[k] = af->lr_host[gi];
        covered += len;
    }
    if (a.mode == 0 && covered != af->n)
        return fail(GHR_E_INVALID, "ghr_adam_fuse: the eight raw-parameter arrays must tile p_in (n floats)");
    mg->adam.p_base = af->p_in; mg->adam.m_in = af->m_in; mg->adam.v_in = af->v_in;
    mg->adam.p_out = af->p_out; mg->adam.m_out = af->m_out; mg->adam.v_out = af->v_out;
    mg->adam.state = af->state; mg->adam.beta1 = af->beta1; mg->adam.beta2 = af->beta2; mg->adam.eps = af->eps;
    mg->adam.on = 1;
    return GHR_OK;
}

// Everything a shared-feature segment call refuses, before anything else is looked at (and long before a launch).
// (sh_degree is left to fill_model, which every such call goes through next)
int check_shared(const char* who, const ghr_model_args* m, const ghr_shared_features* sf)
{
    if (!m) return fail(GHR_E_INVALID, "ghr_model_args is NULL");
    if (!sf) return fail(GHR_E_INVALID, "%s: ghr_shared_features is NULL", who);
    if (m->mode != 1) return fail(GHR_E_INVALID, "%s: mode must be 1 (explicit Gaussians)", who);
    if (!sh_coeffs_ok(m->sh_coeffs))
        return fail(GHR_E_INVALID, "%s: sh_coeffs must be 1, 4, 9 or 16", who);
    if (sf->rows_per_strand < 1) return fail(GHR_E_INVALID, "%s: rows_per_strand must be >= 1", who);
    if (sf->n_strands < 0 || (long long)sf->n_strands * sf->rows_per_strand != (long long)m->P)
        return fail(GHR_E_INVALID, "%s: P must equal n_strands * rows_per_strand", who);
    if (m->adam_fuse) return fail(GHR_E_INVALID, "%s: adam_fuse is not available for per-strand features", who);
    if (m->cam_only) return fail(GHR_E_INVALID, "%s: cam_only is not available for per-strand features", who);
    if (m->d_rgb) return fail(GHR_E_INVALID, "%s: d_rgb is set by the call itself (pass d_rgb_ws)", who);
    return GHR_OK;
}

// ---- the projection forward of a segment ---------------------------------------------------------------------------------
int check_forward_segment(const ghr_model_args* m, int32_t rows_total, const void* geom_ws, const void* img_ws,
                          const int32_t* radii, ghr::ModelArgs* a)
{
    if (int rc = fill_model(m, a)) return rc;
    if (rows_total < 0 || (long long)a->row0 + a->P > rows_total) return fail(GHR_E_INVALID, "segment exceeds rows_total");
    if (rows_total == 0) return GHR_OK;
    if (!geom_ws || !img_ws || !radii) return fail(GHR_E_INVALID, "workspace/radii is NULL");
    return GHR_OK;
}

// sf != NULL: features_dc / features_rest of `m` are per strand (checked by check_shared)
int run_forward_segment(ghr::ModelArgs& a, const ghr_model_args* m, const ghr_shared_features* sf, hipStream_t s,
                        int32_t rows_total, int32_t first, void* geom_ws, void* img_ws, int32_t* radii, float* means2D_out)
{
    if (rows_total == 0) return GHR_OK;
    const ViewWs w = carve_view((size_t)rows_total, a.W, a.H, false, 0, geom_ws, img_ws, nullptr);
    if (first)
        if (int rc = zero_or_verify_counters(w, m->img_ws_recycled, m->debug,
                                             "ghr_model_args.img_ws_recycled is set but the workspace's per-tile counters are not zero "
                                             "(was it through stage 1 AND stage 2 of a pass with P > 0 at the same W x H?)", s))
            return rc;
    // rows between the end of this segment and the next multiple of 256 are padding: culled, no gradient slots
    const int end = a.row0 + a.P;
    const int pad_end = (int)std::min<long long>((long long)n_blocks(end) * GHR_BLOCK, rows_total);
    if (pad_end > end) {
        GHR_HIP(hipMemsetAsync(w.g.rects + end, 0, sizeof(ghr::rect4) * (size_t)(pad_end - end), s));
        GHR_HIP(hipMemsetAsync(radii + end, 0, sizeof(int32_t) * (size_t)(pad_end - end), s));
    }
    if (a.P == 0) return finish(s, m->debug);
    a.rec = w.g.rec; a.depths = w.g.depths; a.rects = w.g.rects; a.radii = radii; a.means2D = means2D_out;
    a.tile_count = w.im.tile_count; a.slot_blk = w.g.slot_blk; a.pos = w.g.pos;
    if (sf) {
        const ghr::SharedFeat k{sf->n_strands, sf->rows_per_strand, a.features_dc, a.features_rest};
        a.features_dc = a.xyz;  // load_raw reads 3 floats per ROW there; the kernel replaces them by the strand's
        a.features_rest = nullptr;
        if (a.sh_coeffs > 1) hipLaunchKernelGGL(ghr::k_shared_proj_fwd<true>, dim3(n_blocks(a.P)), dim3(GHR_BLOCK), 0, s, a, k);
        else hipLaunchKernelGGL(ghr::k_shared_proj_fwd<false>, dim3(n_blocks(a.P)), dim3(GHR_BLOCK), 0, s, a, k);
    } else if (a.sh_coeffs > 1) hipLaunchKernelGGL(ghr::k_project<true>, dim3(n_blocks(a.P)), dim3(GHR_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(ghr::k_project<false>, dim3(n_blocks(a.P)), dim3(GHR_BLOCK), 0, s, a);
    return finish(s, m->debug);
}

int forward_segment(const ghr_model_args* m, const ghr_shared_features* sf, void* stream, int32_t rows_total, int32_t first,
                    void* geom_ws, void* img_ws, int32_t* radii, float* means2D_out)
{
    ghr::ModelArgs a;
    if (int rc = check_forward_segment(m, rows_total, geom_ws, img_ws, radii, &a)) return rc;
    return run_forward_segment(a, m, sf, (hipStream_t)stream, rows_total, first, geom_ws, img_ws, radii, means2D_out);
}

int check_model_forward_stage1(const ghr_model_args* m, const void* geom_ws, const void* img_ws, const int32_t* radii,
                               const uint32_t* R_host, ghr::ModelArgs* a)
{
    if (!m) return fail(GHR_E_INVALID, "ghr_model_args is NULL");
    if (m->row0 != 0) return fail(GHR_E_INVALID, "ghr_model_forward_stage1: row0 must be 0 (use the segment calls)");
    if (!R_host) return fail(GHR_E_INVALID, "R_host is NULL");
    // (ghr_model_forward_finish has nothing to add: its sizes, R_host and workspaces are the ones checked here)
    return check_forward_segment(m, m->P, geom_ws, img_ws, radii, a);
}
}  // namespace

int ghr_model_forward_segment(void* stream, const ghr_model_args* m, int32_t rows_total, int32_t first, void* geom_ws,
                              void* img_ws, int32_t* radii, float* means2D_out)
{
    return forward_segment(m, nullptr, stream, rows_total, first, geom_ws, img_ws, radii, means2D_out);
}

int ghr_model_forward_segment_shared(void* stream, const ghr_model_args* m, const ghr_shared_features* sf, int32_t rows_total,
                                     int32_t first, void* geom_ws, void* img_ws, int32_t* radii, float* means2D_out)
{
    if (int rc = check_shared("ghr_model_forward_segment_shared", m, sf)) return rc;
    if (m->P == 0) {  // nothing to project, nothing launched (not even the `first` segment's counter reset)
        ghr::ModelArgs a;
        return fill_model(m, &a);
    }
    return forward_segment(m, sf, stream, rows_total, first, geom_ws, img_ws, radii, means2D_out);
}

int ghr_model_forward_finish(void* stream, int32_t rows_total, int32_t W, int32_t H, int32_t debug, void* geom_ws,
                             void* img_ws, uint32_t* R_host)
{
    if (rows_total < 0 || W <= 0 || H <= 0) return fail(GHR_E_INVALID, "bad rows_total/W/H");
    if (!R_host) return fail(GHR_E_INVALID, "R_host is NULL");
    hipStream_t s = (hipStream_t)stream;
    if (rows_total == 0) { *R_host = 0; return GHR_OK; }
    if (!geom_ws || !img_ws) return fail(GHR_E_INVALID, "workspace is NULL");
    const ViewWs w = carve_view((size_t)rows_total, W, H, false, 0, geom_ws, img_ws, nullptr);
    if (int rc = tile_scan(w, rows_total, R_host, s)) return rc;
    return finish(s, debug);
}

int ghr_model_forward_stage1(void* stream, const ghr_model_args* m, void* geom_ws, void* img_ws, int32_t* radii,
                             float* means2D_out, uint32_t* R_host)
{
    ghr::ModelArgs a;
    if (int rc = check_model_forward_stage1(m, geom_ws, img_ws, radii, R_host, &a)) return rc;
    if (int rc = run_forward_segment(a, m, nullptr, (hipStream_t)stream, m->P, 1, geom_ws, img_ws, radii, means2D_out)) return rc;
    return ghr_model_forward_finish(stream, m->P, m->W, m->H, m->debug, geom_ws, img_ws, R_host);
}

static int check_render_backward(int32_t rows_total, int32_t W, int32_t H, uint32_t R, const float* background, const void* geom_ws,
                                 const void* img_ws, const void* bin_ws, const float* dL_dpix, const float* grad_scratch)
{
    if (rows_total < 0 || W <= 0 || H <= 0) return fail(GHR_E_INVALID, "bad rows_total/W/H");
    if (rows_total == 0 || R == 0) return GHR_OK;
    if (!background || !geom_ws || !img_ws || !bin_ws || !dL_dpix || !grad_scratch)
        return fail(GHR_E_INVALID, "ghr_render_backward: NULL buffer");
    if (ordered_walk_refused((size_t)rows_total, R, W, H)) return fail(GHR_E_INVALID, GHR_E_DETERMINISTIC_MSG);
    return GHR_OK;
}

int ghr_render_backward(void* stream, int32_t rows_total, int32_t W, int32_t H, uint32_t R, const float* background,
                        const void* geom_ws, const void* img_ws, const void* bin_ws, const float* dL_dpix,
                        float* grad_scratch, int32_t prezeroed)
{
    if (int rc = check_render_backward(rows_total, W, H, R, background, geom_ws, img_ws, bin_ws, dL_dpix, grad_scratch)) return rc;
    if (rows_total == 0 || R == 0) return GHR_OK;
    hipStream_t s = (hipStream_t)stream;
    const ViewWs w = carve_view((size_t)rows_total, W, H, false, R, geom_ws, img_ws, bin_ws);
    if (int rc = pixel_backward(w, (size_t)rows_total, W, H, R, background, dL_dpix, grad_scratch, prezeroed, s)) return rc;
    return finish(s, 0);
}

int ghr_shared_sh_fold(void* stream, const ghr_shared_features* sf, int32_t sh_degree, int32_t sh_coeffs, const float* xyz,
                       const float* campos, const float* d_rgb, float* d_features_dc, float* d_features_rest, int32_t* nan_flag)
{
    static const char* who = "ghr_shared_sh_fold";
    if (!sf) return fail(GHR_E_INVALID, "%s: ghr_shared_features is NULL", who);
    if (sf->rows_per_strand < 1 || sf->n_strands < 0 || (long long)sf->n_strands * sf->rows_per_strand > 0x7fffffffLL)
        return fail(GHR_E_INVALID, "%s: bad n_strands / rows_per_strand", who);
    if (!sh_coeffs_ok(sh_coeffs)) return fail(GHR_E_INVALID, "%s: sh_coeffs must be 1, 4, 9 or 16", who);
    // (a degree above 3 is not covered by any such sh_coeffs)
    if (sh_degree < 0 || !sh_covers(sh_degree, sh_coeffs)) return fail(GHR_E_INVALID, "%s: bad sh_degree", who);
    if (sf->n_strands == 0) return GHR_OK;
    if (!xyz || !campos || !d_rgb || !d_features_dc || (sh_coeffs > 1 && !d_features_rest))
        return fail(GHR_E_INVALID, "%s: NULL buffer", who);
    ghr::SharedFoldArgs fa;
    fa.S = sf->n_strands; fa.n_seg = sf->rows_per_strand; fa.sh_degree = sh_degree; fa.sh_coeffs = sh_coeffs;
    fa.xyz = xyz; fa.campos = campos; fa.d_rgb = d_rgb; fa.d_dc = d_features_dc; fa.d_rest = d_features_rest;
    fa.nan_flag = nan_flag;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ghr::k_shared_sh_fold, dim3(fa.S), dim3(GHR_PBW_BLOCK), 0, s, fa);
    return finish(s, 0);
}

namespace {
// where the projection backward of a segment leaves its gradients
struct ProjGrads {
    float *means2D, *xyz, *log_scales, *rotations, *opacity_logit, *label_logit, *orient_conf_log, *features_dc, *features_rest, *dir3d;
};
// Fills `a` and the optimizer table of `mg` (fill_adam_fuse).
int check_backward_segment(const ghr_model_args* m, const ghr_shared_features* sf, int32_t rows_total, const int32_t* radii,
                           const void* geom_ws, const ProjGrads& d, int32_t accumulate, const int32_t* nan_flag, const void* bin_ws,
                           uint32_t R, ghr::ModelArgs* a, ghr::ModelGrads* mg)
{
    if (int rc = fill_model(m, a)) return rc;
    if (rows_total < 0 || (long long)a->row0 + a->P > rows_total) return fail(GHR_E_INVALID, "segment exceeds rows_total");
    if (!bin_ws && R > 0) return fail(GHR_E_INVALID, "ghr_model_backward_segment: bin_ws is NULL");
    mg->adam.on = 0;
    if (a->P == 0) return GHR_OK;
    const bool need_act = a->mode == 0;
    const bool cam_only = m->cam_only != 0;
    if (cam_only && !m->cam_partial) return fail(GHR_E_INVALID, "ghr_model_backward_segment: cam_only without cam_partial");
    if (m->cam_partial && (m->cam_slot0 < 0 || (long long)m->cam_slot0 + ghr_camera_slots(a->P) > m->cam_slots))
        return fail(GHR_E_INVALID, "ghr_model_backward_segment: the segment's camera columns exceed cam_slots");
    if (!radii || !geom_ws) return fail(GHR_E_INVALID, "ghr_model_backward_segment: NULL buffer");
    const bool factored_sh = m->d_rgb != nullptr || sf != nullptr;
    const bool sh_unstored = sh_grads_unstored(m, factored_sh, accumulate);
    if (!cam_only && (!d.means2D || !d.xyz || !d.log_scales || !d.rotations || (!sh_unstored && !d.features_dc) ||
        (need_act && (!d.opacity_logit || !d.label_logit || !d.orient_conf_log)) ||
        (!sh_unstored && a->sh_coeffs > 1 && !d.features_rest)))
        return fail(GHR_E_INVALID, "ghr_model_backward_segment: NULL buffer");
    if (factored_sh && (cam_only || m->adam_fuse))
        return fail(GHR_E_INVALID, "ghr_model_backward_segment: d_rgb with cam_only / adam_fuse");
    if (!dens_all_or_none(m))
        return fail(GHR_E_INVALID, "ghr_model_backward_segment: dens_grad_accum / dens_denom / dens_max_radii2D: all three or none");
    if (m->adam_fuse) {
        if (cam_only) return fail(GHR_E_INVALID, "ghr_adam_fuse: not with a cam_only segment");
        if (int rc = fill_adam_fuse(*a, m->adam_fuse, accumulate, nan_flag, mg)) return rc;
    }
    return GHR_OK;
}

// sf != NULL (checked by check_shared): the projection backward in factored form into d_rgb_ws, then the per-strand fold into
// d.features_dc [S,1,3] / d.features_rest [S,K-1,3]
int run_backward_segment(ghr::ModelArgs& a, ghr::ModelGrads& mg, const ghr_model_args* m, const ghr_shared_features* sf,
                         float* d_rgb_ws, void* stream, int32_t rows_total, const int32_t* radii, const void* geom_ws,
                         const float* grad_scratch, const ProjGrads& d, int32_t accumulate, int32_t* nan_flag, uint32_t grad_rows,
                         const void* bin_ws, uint32_t R)
{
    if (a.P == 0) return GHR_OK;
    hipStream_t s = (hipStream_t)stream;
    const bool cam_only = m->cam_only != 0;
    const ghr_adam_fuse* af = m->adam_fuse;
    // (of the image workspace only the instance count is read, and only where the densification statistics or the step's flag ask)
    const ViewWs w = carve_view((size_t)rows_total, a.W, a.H, false, R, geom_ws, m->dens_img_ws, bin_ws);
    // (rec: the gather unpacks the gradient lines with the pixel mean / conic / opacity k_project stored)
    a.radii = const_cast<int*>(radii); a.rects = w.g.rects; a.rec = w.g.rec;
    mg.inst_line = w.b.inst_line; mg.ginst = grad_scratch; mg.ginst_rows = grad_rows ? (grad_rows < R ? grad_rows : R) : R;
    mg.d_means2D = d.means2D; mg.d_xyz = d.xyz; mg.d_log_scales = d.log_scales; mg.d_rotations = d.rotations;
    mg.d_opacity_logit = d.opacity_logit; mg.d_label_logit = d.label_logit; mg.d_orient_conf_log = d.orient_conf_log;
    mg.d_features_dc = d.features_dc; mg.d_features_rest = d.features_rest; mg.d_rgb = m->d_rgb;
    if (sf) { mg.d_rgb = d_rgb_ws; mg.d_features_dc = mg.d_features_rest = nullptr; }
    mg.d_dir3d = a.mode == 1 ? d.dir3d : nullptr;
    mg.accumulate = accumulate; mg.nan_flag = cam_only ? nullptr : nan_flag;
    mg.cam_partial = m->cam_partial; mg.cam_slot0 = (uint32_t)m->cam_slot0; mg.cam_stride = (uint32_t)m->cam_slots;
    mg.cam_only = cam_only ? 1 : 0; mg.detach_means2D = m->detach_means2D != 0 ? 1 : 0;
    mg.dens_grad_accum = m->dens_grad_accum; mg.dens_denom = m->dens_denom; mg.dens_max_radii = m->dens_max_radii2D;
    // (steps with the fused optimizer update: EVERY view's backward checks its instance count and raises the step's flag)
    const bool overflow_is_bad = m->dens_img_ws && (af || m->overflow_raises_flag);
    mg.dens_count = (n_dens(m) == 3 || overflow_is_bad) ? w.im.R_dev : nullptr;  // (NULL without dens_img_ws)
    mg.dens_cap = R; mg.overflow_is_bad = overflow_is_bad ? 1 : 0;
    const dim3 grid((a.P + GHR_PBW_BLOCK - 1) / GHR_PBW_BLOCK), block(GHR_PBW_BLOCK);
    if (sf) {
        const ghr::SharedFeat k{sf->n_strands, sf->rows_per_strand, a.features_dc, a.features_rest};
        const float *xyz = a.xyz, *campos = a.campos;
        const int deg = a.sh_degree, K = a.sh_coeffs;
        a.features_dc = a.xyz;  // (see forward_segment)
        a.features_rest = nullptr;
        if (mg.cam_partial) hipLaunchKernelGGL(ghr::k_shared_proj_bwd<true>, grid, block, 0, s, a, mg, k);
        else hipLaunchKernelGGL(ghr::k_shared_proj_bwd<false>, grid, block, 0, s, a, mg, k);
        if (int rc = ghr_shared_sh_fold(stream, sf, deg, K, xyz, campos, d_rgb_ws, d.features_dc, d.features_rest, nan_flag)) return rc;
    } else if (af) {
        if (mg.cam_partial) hipLaunchKernelGGL((ghr::k_project_bwd<true, true>), grid, block, 0, s, a, mg);
        else hipLaunchKernelGGL((ghr::k_project_bwd<false, true>), grid, block, 0, s, a, mg);
        // (a strand segment leaves the finish to the caller -- ghr_adam_fused_finish -- who first steps the groups whose
        // gradients are still on their way through autograd and adds their non-finite mark to the step's flag)
        if (a.mode == 0) adam_fused_finish(af, s);
    } else if (mg.cam_partial) hipLaunchKernelGGL((ghr::k_project_bwd<true, false>), grid, block, 0, s, a, mg);
    else hipLaunchKernelGGL((ghr::k_project_bwd<false, false>), grid, block, 0, s, a, mg);
    return finish(s, m->debug);
}

int backward_segment(const ghr_model_args* m, const ghr_shared_features* sf, float* d_rgb_ws, void* stream, int32_t rows_total,
                     const int32_t* radii, const void* geom_ws, const float* grad_scratch, const ProjGrads& d, int32_t accumulate,
                     int32_t* nan_flag, uint32_t grad_rows, const void* bin_ws, uint32_t R)
{
    ghr::ModelArgs a; ghr::ModelGrads mg;
    if (int rc = check_backward_segment(m, sf, rows_total, radii, geom_ws, d, accumulate, nan_flag, bin_ws, R, &a, &mg)) return rc;
    return run_backward_segment(a, mg, m, sf, d_rgb_ws, stream, rows_total, radii, geom_ws, grad_scratch, d, accumulate, nan_flag,
                                grad_rows, bin_ws, R);
}
}  // namespace

int ghr_model_backward_segment(void* stream, const ghr_model_args* m, int32_t rows_total, const int32_t* radii,
                               const void* geom_ws, const float* grad_scratch, float* d_means2D, float* d_xyz,
                               float* d_log_scales, float* d_rotations, float* d_opacity_logit, float* d_label_logit,
                               float* d_orient_conf_log, float* d_features_dc, float* d_features_rest, float* d_dir3d,
                               int32_t accumulate, int32_t* nan_flag, uint32_t grad_rows, const void* bin_ws,
                               uint32_t R)
{
    const ProjGrads d{d_means2D, d_xyz, d_log_scales, d_rotations, d_opacity_logit, d_label_logit, d_orient_conf_log,
                      d_features_dc, d_features_rest, d_dir3d};
    return backward_segment(m, nullptr, nullptr, stream, rows_total, radii, geom_ws, grad_scratch, d, accumulate, nan_flag,
                            grad_rows, bin_ws, R);
}

int ghr_model_backward_segment_shared(void* stream, const ghr_model_args* m, const ghr_shared_features* sf, int32_t rows_total,
                                      const int32_t* radii, const void* geom_ws, const float* grad_scratch, float* d_means2D,
                                      float* d_xyz, float* d_log_scales, float* d_rotations, float* d_opacity_logit,
                                      float* d_label_logit, float* d_orient_conf_log, float* d_features_dc,
                                      float* d_features_rest, float* d_dir3d, int32_t* nan_flag, uint32_t grad_rows,
                                      const void* bin_ws, uint32_t R, float* d_rgb_ws)
{
    static const char* who = "ghr_model_backward_segment_shared";
    if (int rc = check_shared(who, m, sf)) return rc;
    if (m->P > 0 && !d_rgb_ws) return fail(GHR_E_INVALID, "%s: d_rgb_ws is NULL", who);
    if (m->P > 0 && !d_features_dc) return fail(GHR_E_INVALID, "%s: d_features_dc is NULL", who);
    if (m->P > 0 && m->sh_coeffs > 1 && !d_features_rest) return fail(GHR_E_INVALID, "%s: d_features_rest is NULL", who);
    const ProjGrads d{d_means2D, d_xyz, d_log_scales, d_rotations, d_opacity_logit, d_label_logit, d_orient_conf_log,
                      d_features_dc, d_features_rest, d_dir3d};
    return backward_segment(m, sf, d_rgb_ws, stream, rows_total, radii, geom_ws, grad_scratch, d, 0, nan_flag, grad_rows, bin_ws, R);
}

int ghr_adam_fused_finish(void* stream, const ghr_adam_fuse* af)
{
    if (!af || af->n < 0 || !af->p_in || !af->m_in || !af->v_in || !af->p_out || !af->m_out || !af->v_out || !af->state ||
        !af->flag || !af->flag_next)
        return fail(GHR_E_INVALID, "ghr_adam_fused_finish: bad ghr_adam_fuse");
    adam_fused_finish(af, (hipStream_t)stream);
    return finish((hipStream_t)stream, 0);
}

int32_t ghr_camera_slots(int32_t P) { return P > 0 ? (P + GHR_PBW_BLOCK - 1) / GHR_PBW_BLOCK : 0; }

int ghr_camera_grad_fold(void* stream, const float* cam_partial, int32_t cam_slots, float* d_cam, const float* fovx_dev,
                         const float* fovy_dev)
{
    if (!d_cam || cam_slots < 0 || (cam_slots > 0 && !cam_partial) || ((fovx_dev != nullptr) != (fovy_dev != nullptr)))
        return fail(GHR_E_INVALID, "ghr_camera_grad_fold: bad args");
    hipStream_t s = (hipStream_t)stream;
    if (cam_slots == 0) {
        GHR_HIP(hipMemsetAsync(d_cam, 0, sizeof(float) * GHR_CAM_GRADS, s));
        return finish(s, 0);
    }
    hipLaunchKernelGGL(ghr::k_cam_fold, dim3(GHR_CAM_PARTIALS), dim3(GHR_CAM_FOLD_BLOCK), 0, s, cam_partial, (uint32_t)cam_slots,
                       d_cam, fovx_dev, fovy_dev);
    return finish(s, 0);
}

static int check_sh_grad_from_views(int32_t P, int32_t sh_degree, int32_t sh_coeffs, const float* xyz, int32_t n_views,
                                    const float* campos, int64_t campos_stride, const float* g_views, int64_t view_stride,
                                    const float* d_features_dc, const float* d_features_rest, const int32_t* nan_flag, int64_t flag_offset)
{
    if (!sh_views_sizes_ok(P, sh_degree, sh_coeffs, n_views, view_stride, campos_stride) ||
        (nan_flag != nullptr && (flag_offset < 0 || (n_views > 1 && flag_offset >= view_stride))))
        return fail(GHR_E_INVALID, "ghr_sh_grad_from_views: bad sizes");
    if (P == 0) return GHR_OK;
    if (!xyz || !d_features_dc || (sh_coeffs > 1 && !d_features_rest) || (n_views > 0 && (!campos || !g_views)) ||
        sh_views_overlap(P, n_views, view_stride))
        return fail(GHR_E_INVALID, "ghr_sh_grad_from_views: NULL buffer / overlapping views");
    return GHR_OK;
}

int ghr_sh_grad_from_views(void* stream, int32_t P, int32_t sh_degree, int32_t sh_coeffs, const float* xyz, int32_t n_views,
                           const float* campos, int64_t campos_stride, const float* g_views, int64_t view_stride,
                           float* d_features_dc, float* d_features_rest, int32_t accumulate, int32_t* nan_flag,
                           int64_t flag_offset)
{
    if (int rc = check_sh_grad_from_views(P, sh_degree, sh_coeffs, xyz, n_views, campos, campos_stride, g_views, view_stride,
                                          d_features_dc, d_features_rest, nan_flag, flag_offset))
        return rc;
    if (P == 0) return GHR_OK;
    hipStream_t s = (hipStream_t)stream;
    ghr::ShViewsArgs a;
    a.P = P; a.sh_degree = sh_degree; a.sh_coeffs = sh_coeffs; a.n_views = n_views; a.xyz = xyz; a.campos = campos;
    a.campos_stride = (size_t)campos_stride; a.nan_flag = nan_flag; a.flag_offset = flag_offset;
    a.g = g_views; a.view_stride = (size_t)view_stride; a.d_dc = d_features_dc; a.d_rest = d_features_rest;
    a.accumulate = accumulate != 0;
    hipLaunchKernelGGL(ghr::k_sh_grad_from_views, dim3((P + GHR_PBW_BLOCK - 1) / GHR_PBW_BLOCK), dim3(GHR_PBW_BLOCK), 0, s, a);
    return finish(s, 0);
}

static_assert(GHR_STRAND_MAX_SEG * 24 <= 48 * 1024, "one strand's two LDS rows");

int ghr_strand_build(void* stream, int32_t S, int32_t n_seg, const float* origins, const float* dirs, float scale, float* xyz,
                     float* rotation, float* scaling)
{
    if (S < 0 || n_seg < 0 || n_seg > GHR_STRAND_MAX_SEG) return fail(GHR_E_INVALID, "ghr_strand_build: bad strand shape");
    if (S == 0 || n_seg == 0) return GHR_OK;
    if ((int64_t)S * n_seg > (int64_t)INT32_MAX / 4) return fail(GHR_E_INVALID, "ghr_strand_build: too many segments");
    if (!origins || !dirs || !xyz || !rotation || !scaling) return fail(GHR_E_INVALID, "ghr_strand_build: NULL buffer");
    hipStream_t s = (hipStream_t)stream;
    ghr::StrandArgs a;
    a.S = S; a.n_seg = n_seg; a.spb = ghr::strands_per_block(n_seg);
    a.origins = origins; a.dirs = dirs; a.scale = scale; a.xyz = xyz; a.rot = rotation; a.scaling = scaling;
    const size_t lds = (size_t)2 * a.spb * n_seg * 3 * sizeof(float);
    hipLaunchKernelGGL(ghr::k_strand_build, dim3((S + a.spb - 1) / a.spb), dim3(GHR_STRAND_BLOCK), lds, s, a);
    return finish(s, 0);
}

int ghr_strand_build_backward(void* stream, int32_t S, int32_t n_seg, const float* dirs, const float* d_xyz,
                              const float* d_rotation, const float* d_scaling, float* d_dirs)
{
    return ghr_strand_build_backward_ex(stream, S, n_seg, dirs, d_xyz, d_rotation, d_scaling, nullptr, d_dirs);
}

int ghr_strand_build_backward_ex(void* stream, int32_t S, int32_t n_seg, const float* dirs, const float* d_xyz,
                                 const float* d_rotation, const float* d_scaling, const float* d_dir_rows, float* d_dirs)
{
    if (S < 0 || n_seg < 0 || n_seg > GHR_STRAND_MAX_SEG) return fail(GHR_E_INVALID, "ghr_strand_build_backward: bad strand shape");
    if (S == 0 || n_seg == 0) return GHR_OK;
    if ((int64_t)S * n_seg > (int64_t)INT32_MAX / 4) return fail(GHR_E_INVALID, "ghr_strand_build_backward: too many segments");
    if (!dirs || !d_dirs) return fail(GHR_E_INVALID, "ghr_strand_build_backward: NULL buffer");
    hipStream_t s = (hipStream_t)stream;
    ghr::StrandBwdArgs a;
    a.S = S; a.n_seg = n_seg; a.spb = ghr::strands_per_block(n_seg);
    a.dirs = dirs; a.d_xyz = d_xyz; a.d_rot = d_rotation; a.d_scaling = d_scaling; a.d_dir_rows = d_dir_rows; a.d_dirs = d_dirs;
    const size_t lds = (size_t)2 * a.spb * n_seg * 3 * sizeof(float);
    hipLaunchKernelGGL(ghr::k_strand_build_bwd, dim3((S + a.spb - 1) / a.spb), dim3(GHR_STRAND_BLOCK), lds, s, a);
    return finish(s, 0);
}

int ghr_model_backward(void* stream, const ghr_model_args* m, uint32_t R, const int32_t* radii, const void* geom_ws,
                       const void* img_ws, const void* bin_ws, const float* dL_dpix, float* grad_scratch,
                       float* d_means2D, float* d_xyz, float* d_log_scales, float* d_rotations,
                       float* d_opacity_logit, float* d_label_logit, float* d_orient_conf_log, float* d_features_dc,
                       float* d_features_rest, int32_t accumulate, int32_t* nan_flag, int32_t prezeroed)
{
    if (!m) return fail(GHR_E_INVALID, "ghr_model_args is NULL");
    if (m->row0 != 0) return fail(GHR_E_INVALID, "ghr_model_backward: row0 must be 0 (use the segment calls)");
    if (m->P == 0) return GHR_OK;
    if (!dL_dpix || (R > 0 && (!grad_scratch || !bin_ws)) || !img_ws || !m->background)
        return fail(GHR_E_INVALID, "ghr_model_backward: NULL buffer");
    if (int rc = ghr_render_backward(stream, m->P, m->W, m->H, R, m->background, geom_ws, img_ws, bin_ws, dL_dpix,
                                     grad_scratch, prezeroed))
        return rc;
    return ghr_model_backward_segment(stream, m, m->P, radii, geom_ws, grad_scratch, d_means2D, d_xyz, d_log_scales,
                                      d_rotations, d_opacity_logit, d_label_logit, d_orient_conf_log, d_features_dc,
                                      d_features_rest, nullptr, accumulate, nan_flag, R, bin_ws, R);
}

#ifndef GHR_ADAM_BLOCKS
#define GHR_ADAM_BLOCKS 65536
#endif
// The marching form of the loss kernels (ghr_loss.h) needs 16-B aligned image rows
// Rows of a strip per wave.  Measured on 1080p (profiles/r03h): 16 .. 40 rows give the same kernel time, 64 is 6 % slower,
// 128 10 %, 272 60 % -- the kernels live on the number of waves in flight, the ten extra rows a segment filters for its
// first output row are cheap
static int loss_march_seg(const ghr_loss_args* l, bool backward)
{
    const char* e = std::getenv(backward ? "GHR_LOSS_SEG_B" : "GHR_LOSS_SEG_F");  // measurement knob
    int seg = e ? atoi(e) : 0;
    if (seg <= 0) seg = 32;
    (void)l;
    return (seg + GHR_LM_ROWS - 1) / GHR_LM_ROWS * GHR_LM_ROWS;
}
static dim3 loss_march_grid(const ghr_loss_args* l, int seg)
{
    return dim3(8 * (((l->W + GHR_LM_TW - 1) / GHR_LM_TW + 7) / 8), (l->H + seg - 1) / seg, 3);
}
static bool loss_vec_ok(const ghr_loss_args* l, const void* p0 = nullptr, const void* p1 = nullptr)
{
    const bool off = std::getenv("GHR_LOSS_SCALAR") != nullptr;  // test / measurement knob (read per call): the tile kernels
    if (off || (l->W & 3) || (size_t)l->W * (size_t)l->H >= ((size_t)1 << 30)) return false;
    const void* ps[] = {l->image, l->gt_image, l->gt_mask, l->gt_stats, p0, p1};
    for (const void* p : ps)
        if (((uintptr_t)p & 15u) != 0) return false;
    return true;
}

size_t ghr_loss_sums_floats(int32_t W, int32_t H)
{
    if (W <= 0 || H <= 0) return 0;
    // the larger of the two kernel forms' slot counts (marching form at its shortest segment, GHR_LM_ROWS rows)
    const size_t n = std::max(ghr::loss_slots_tile(W, H), ghr::loss_slots_march(W, H, GHR_LM_ROWS));
    return GHR_LOSS_AUX + GHR_LOSS_TERMS * n;
}

static int check_loss_forward(const ghr_loss_args* l, const float* maps, const float* sums, const float* loss_out)
{
    if (!l || l->W <= 0 || l->H <= 0 || !l->image || !l->mask || !l->gt_image || !l->gt_mask || !maps || !sums || !loss_out)
        return fail(GHR_E_INVALID, "ghr_loss_forward: bad args");
    if (l->w_orient != 0.f && (!l->dir2d || !l->orient_conf || !l->gt_orient_angle || !l->gt_orient_conf))
        return fail(GHR_E_INVALID, "ghr_loss_forward: w_orient != 0 needs dir2d / orient_conf / gt_orient_angle / gt_orient_conf");
    return GHR_OK;
}

int ghr_loss_forward(void* stream, const ghr_loss_args* l, float* maps, float* sums, float* loss_out)
{
    if (int rc = check_loss_forward(l, maps, sums, loss_out)) return rc;
    const bool orient = l->w_orient != 0.f;
    hipStream_t s = (hipStream_t)stream;
    // sums = {aux[GHR_LOSS_AUX] | one slot of five partial sums per workgroup of the forward kernel}: nothing to zero
    ghr::LossArgs a{l->W, l->H, l->image, l->mask, orient ? l->dir2d : nullptr, l->orient_conf, l->gt_image, l->gt_mask,
                    l->gt_orient_angle, l->gt_orient_conf, l->unmasked_colours ? 0 : 1, maps, sums + GHR_LOSS_AUX, l->gt_stats,
                    nullptr, loss_march_seg(l, false), 0u};
    const dim3 grid((l->W + GHR_L_TW - 1) / GHR_L_TW, (l->H + GHR_L_TH - 1) / GHR_L_TH, 3);
    const bool vec = loss_vec_ok(l, maps);
    const dim3 grid_v = loss_march_grid(l, a.seg);
    const size_t n_slots = vec ? ghr::loss_slots_march(l->W, l->H, a.seg) : ghr::loss_slots_tile(l->W, l->H);
    a.n_slots = (uint32_t)n_slots;
    if (l->gt_stats) {
        if (vec) hipLaunchKernelGGL(ghr::k_loss_fwd_cached_v, grid_v, dim3(64), 0, s, a);
        else hipLaunchKernelGGL(ghr::k_loss_fwd_cached, grid, dim3(256), 0, s, a);
    } else {
        if (vec) hipLaunchKernelGGL(ghr::k_loss_fwd_v, grid_v, dim3(64), 0, s, a);
        else hipLaunchKernelGGL(ghr::k_loss_fwd, grid, dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(ghr::k_loss_finalize, dim3(1), dim3(1024), 0, s, sums + GHR_LOSS_AUX, (uint32_t)n_slots, l->w_l1,
                       l->w_ssim, l->w_mask, orient ? l->w_orient : 0.f, (float)l->W * (float)l->H, sums, loss_out);
    return finish(s, 0);
}

int ghr_loss_gt_stats(void* stream, const ghr_loss_args* l, float* stats_out)
{
    if (!l || l->W <= 0 || l->H <= 0 || !l->gt_image || !l->gt_mask || !stats_out)
        return fail(GHR_E_INVALID, "ghr_loss_gt_stats: bad args");
    hipStream_t s = (hipStream_t)stream;
    ghr::LossArgs a{l->W, l->H, l->gt_image, nullptr, nullptr, nullptr, l->gt_image, l->gt_mask, nullptr, nullptr,
                    l->unmasked_colours ? 0 : 1, nullptr, nullptr, nullptr, stats_out, loss_march_seg(l, false), 0u};
    const dim3 grid((l->W + GHR_L_TW - 1) / GHR_L_TW, (l->H + GHR_L_TH - 1) / GHR_L_TH, 3);
    if (loss_vec_ok(l, stats_out)) hipLaunchKernelGGL(ghr::k_loss_gt_stats_v, loss_march_grid(l, a.seg), dim3(64), 0, s, a);
    else hipLaunchKernelGGL(ghr::k_loss_gt_stats, grid, dim3(256), 0, s, a);
    return finish(s, 0);
}

static int check_loss_backward(const ghr_loss_args* l, const float* maps, const float* sums, const float* d_image,
                               const float* d_mask, const float* d_dir2d, const float* d_orient_conf)
{
    if (!l || l->W <= 0 || l->H <= 0 || !l->image || !l->mask || !l->gt_image || !l->gt_mask || !maps || !sums ||
        !d_image || !d_mask || ((d_dir2d == nullptr) != (d_orient_conf == nullptr)))
        return fail(GHR_E_INVALID, "ghr_loss_backward: bad args");
    if (l->w_orient != 0.f && (!l->dir2d || !l->orient_conf || !l->gt_orient_angle || !l->gt_orient_conf || !d_dir2d))
        return fail(GHR_E_INVALID, "ghr_loss_backward: w_orient != 0 needs the orientation inputs and d_dir2d / d_orient_conf");
    return GHR_OK;
}

int ghr_loss_backward(void* stream, const ghr_loss_args* l, const float* maps, const float* sums,
                      const float* grad_loss, float* d_image, float* d_mask, float* d_dir2d, float* d_orient_conf,
                      float* zero_plane_a, float* zero_plane_b)
{
    if (int rc = check_loss_backward(l, maps, sums, d_image, d_mask, d_dir2d, d_orient_conf)) return rc;
    const bool orient = l->w_orient != 0.f;
    hipStream_t s = (hipStream_t)stream;
    ghr::LossBwdArgs a{l->W, l->H, l->image, l->mask, orient ? l->dir2d : nullptr, l->orient_conf, l->gt_image,
                       l->gt_mask, l->gt_orient_angle, l->gt_orient_conf, l->unmasked_colours ? 0 : 1, maps,
                       sums,  // aux: {sum of the orientation weights, NaN flag} (k_loss_finalize)
                       grad_loss, l->w_l1, l->w_ssim, l->w_mask, orient ? l->w_orient : 0.f, d_image, d_mask, d_dir2d,
                       d_orient_conf, zero_plane_a, zero_plane_b, loss_march_seg(l, true)};
    const dim3 grid((l->W + GHR_L_TW - 1) / GHR_L_TW, (l->H + GHR_L_TH - 1) / GHR_L_TH, 3);
    if (loss_vec_ok(l, maps)) hipLaunchKernelGGL(ghr::k_loss_bwd_v, loss_march_grid(l, a.seg), dim3(64), 0, s, a);
    else hipLaunchKernelGGL(ghr::k_loss_bwd, grid, dim3(256), 0, s, a);
    return finish(s, 0);
}

// ---- one call per training view (include/ghr.h, ghr_view_step) -------------------------------------------------
namespace {
int vs_bad(const char* what) { return fail(GHR_E_INVALID, "ghr_view_step: %s", what); }
#define GHR_VS_PTR(p, name) \
    do { if (!(p)) return vs_bad(name " is NULL"); } while (0)

// Everything ghr_view_step refuses, asked before the first launch.  First what the call itself does not cover, and the rules
// of the six calls in its own words: a NULL buffer by the name of its field, the others with the predicate their owner asks
// too.  Then the six calls' own checks, in call order: what they refuse is refused here, whether or not it has words above.
// `camera`: the view of ghr_view_step_camera, whose model carries the camera-gradient table and the device FoV (checked there).
int check_view_step(const ghr_view_step_args* v, const ghr_view_args* va, const ghr_loss_args* lr, const ProjGrads& pg, bool camera)
{
    const ghr_model_args* m = &v->model;
    if (m->P <= 0) return vs_bad("model.P must be > 0");
    if (m->W <= 0 || m->H <= 0) return vs_bad("model.W / model.H must be > 0");
    if ((m->W + GHR_TILE - 1) / GHR_TILE > 65535 || (m->H + GHR_TILE - 1) / GHR_TILE > 65535)
        return vs_bad("model.W / model.H: image too large for 16-bit tile coordinates");
    if (m->mode != 0) return vs_bad("model.mode must be 0");
    if (m->row0 != 0) return vs_bad("model.row0 must be 0");
    if (m->debug != 0) return vs_bad("model.debug must be 0 (the call never waits for the device)");
    if ((!camera && m->cam_partial) || m->cam_only || m->detach_means2D)
        return vs_bad("model.cam_partial / cam_only / detach_means2D: camera gradients are not part of the call");
    if (!camera && (m->fovx_dev || m->fovy_dev)) return vs_bad("model.fovx_dev / fovy_dev must be NULL");
    if (!sh_degree_ok(m->sh_degree)) return vs_bad("model.sh_degree must be 0 .. 3");
    if (!sh_coeffs_ok(m->sh_coeffs) || !sh_covers(m->sh_degree, m->sh_coeffs))
        return vs_bad("model.sh_coeffs must be (max_sh_degree + 1)^2 and cover model.sh_degree");
    GHR_VS_PTR(m->xyz, "model.xyz"); GHR_VS_PTR(m->log_scales, "model.log_scales"); GHR_VS_PTR(m->rotations, "model.rotations");
    GHR_VS_PTR(m->opacity_logit, "model.opacity_logit"); GHR_VS_PTR(m->label_logit, "model.label_logit");
    GHR_VS_PTR(m->orient_conf_log, "model.orient_conf_log"); GHR_VS_PTR(m->features_dc, "model.features_dc");
    if (m->sh_coeffs > 1) GHR_VS_PTR(m->features_rest, "model.features_rest");
    GHR_VS_PTR(m->viewmatrix, "model.viewmatrix"); GHR_VS_PTR(m->projmatrix, "model.projmatrix");
    GHR_VS_PTR(m->campos, "model.campos"); GHR_VS_PTR(m->background, "model.background");
    GHR_VS_PTR(v->R_host, "R_host"); GHR_VS_PTR(v->geom_ws, "geom_ws"); GHR_VS_PTR(v->img_ws, "img_ws");
    if (v->R > 0) { GHR_VS_PTR(v->bin_ws, "bin_ws"); GHR_VS_PTR(v->grad_scratch, "grad_scratch"); }
    if (!cell_masks_fit(v->R, m->W, m->H)) return vs_bad("R: too many instances for the 32-bit offsets of the cell masks");
    if (ordered_walk_refused((size_t)m->P, v->R, m->W, m->H)) return vs_bad("model.P / R: " GHR_E_DETERMINISTIC_MSG);
    GHR_VS_PTR(v->radii, "radii"); GHR_VS_PTR(v->render, "render");
    const ghr_loss_args* l = &v->loss;
    if (l->W != m->W || l->H != m->H) return vs_bad("loss.W / loss.H differ from model.W / model.H");
    GHR_VS_PTR(l->gt_image, "loss.gt_image"); GHR_VS_PTR(l->gt_mask, "loss.gt_mask");
    if (l->w_orient != 0.f) { GHR_VS_PTR(l->gt_orient_angle, "loss.gt_orient_angle"); GHR_VS_PTR(l->gt_orient_conf, "loss.gt_orient_conf"); }
    GHR_VS_PTR(v->maps, "maps"); GHR_VS_PTR(v->sums, "sums"); GHR_VS_PTR(v->loss_out, "loss_out"); GHR_VS_PTR(v->d_pix, "d_pix");
    GHR_VS_PTR(v->d_means2D, "d_means2D"); GHR_VS_PTR(v->d_xyz, "d_xyz"); GHR_VS_PTR(v->d_log_scales, "d_log_scales");
    GHR_VS_PTR(v->d_rotations, "d_rotations"); GHR_VS_PTR(v->d_opacity_logit, "d_opacity_logit");
    GHR_VS_PTR(v->d_label_logit, "d_label_logit"); GHR_VS_PTR(v->d_orient_conf_log, "d_orient_conf_log");
    const ghr_adam_fuse* af = m->adam_fuse;
    if (m->d_rgb && af) return vs_bad("model.d_rgb with model.adam_fuse (the view that carries the update stores no table)");
    if (!sh_grads_unstored(m, m->d_rgb != nullptr, v->accumulate) && (!v->d_features_dc || (m->sh_coeffs > 1 && !v->d_features_rest)))
        return vs_bad(af ? "d_features_dc / d_features_rest is NULL: model.adam_fuse with accumulate != 0 adds the earlier views' "
                           "gradients from there"
                         : "d_features_dc / d_features_rest is NULL (without model.d_rgb)");
    if (!dens_all_or_none(m)) return vs_bad("model.dens_grad_accum / dens_denom / dens_max_radii2D: all three or none");
    if (m->dens_img_ws && m->dens_img_ws != v->img_ws) return vs_bad("model.dens_img_ws must be img_ws");
    if (m->overflow_raises_flag && (!m->dens_img_ws || !v->nan_flag))
        return vs_bad("model.overflow_raises_flag needs model.dens_img_ws and nan_flag");
    if (af && !m->dens_img_ws) return vs_bad("model.adam_fuse needs model.dens_img_ws (an overflowed view must not reach the parameters)");
    const ghr_sh_fold_args* f = v->sh_fold;
    if (f) {
        if (f->P != m->P || f->sh_coeffs != m->sh_coeffs) return vs_bad("sh_fold.P / sh_fold.sh_coeffs differ from the model's");
        if (!sh_views_sizes_ok(f->P, f->sh_degree, f->sh_coeffs, f->n_views, f->view_stride, f->campos_stride) ||
            sh_views_overlap(f->P, f->n_views, f->view_stride))
            return vs_bad("sh_fold: bad sizes / overlapping views");
        GHR_VS_PTR(f->xyz, "sh_fold.xyz"); GHR_VS_PTR(f->d_features_dc, "sh_fold.d_features_dc");
        if (f->sh_coeffs > 1) GHR_VS_PTR(f->d_features_rest, "sh_fold.d_features_rest");
        if (f->n_views > 0) { GHR_VS_PTR(f->campos, "sh_fold.campos"); GHR_VS_PTR(f->g_views, "sh_fold.g_views"); }
    }
    const float* d = v->d_pix;
    const size_t n = (size_t)m->W * m->H;
    ghr::ModelArgs a; ghr::ModelGrads mg;
    if (int rc = check_model_forward_stage1(m, v->geom_ws, v->img_ws, v->radii, v->R_host, &a)) return rc;
    if (int rc = check_forward_stage2(va, v->R, v->geom_ws, v->img_ws, v->bin_ws, v->render)) return rc;
    if (int rc = check_loss_forward(lr, v->maps, v->sums, v->loss_out)) return rc;
    if (int rc = check_loss_backward(lr, v->maps, v->sums, d, d + 3 * n, d + 5 * n, d + 8 * n)) return rc;
    if (int rc = check_render_backward(m->P, m->W, m->H, v->R, m->background, v->geom_ws, v->img_ws, v->bin_ws, d, v->grad_scratch))
        return rc;
    if (f)
        if (int rc = check_sh_grad_from_views(f->P, f->sh_degree, f->sh_coeffs, f->xyz, f->n_views, f->campos, f->campos_stride,
                                              f->g_views, f->view_stride, f->d_features_dc, f->d_features_rest, nullptr, 0))
            return rc;
    return check_backward_segment(m, nullptr, m->P, v->radii, v->geom_ws, pg, v->accumulate, v->nan_flag, v->bin_ws, v->R, &a, &mg);
}


// what the six calls take that is no field of `v`: stage 2's view struct, the loss struct over the rendered planes of the
// packed output (include/ghr.h, ghr_loss_args), the gradient pointers
struct ViewStepPlan {
    ghr_view_args va;
    ghr_loss_args l;
    ProjGrads pg;
};

int plan_view_step(const ghr_view_step_args* v, bool camera, ViewStepPlan* p)
{
    if (!v) return vs_bad("the argument struct is NULL");
    const ghr_model_args* m = &v->model;
    const size_t n = (size_t)m->W * m->H;
    std::memset(&p->va, 0, sizeof(p->va));
    p->va.P = m->P; p->va.W = m->W; p->va.H = m->H; p->va.C = GHR_NUM_CHANNELS; p->va.background = m->background;
    p->l = v->loss;
    p->l.image = v->render; p->l.mask = v->render + 3 * n; p->l.dir2d = v->render + 5 * n; p->l.orient_conf = v->render + 8 * n;
    p->pg = ProjGrads{v->d_means2D, v->d_xyz, v->d_log_scales, v->d_rotations, v->d_opacity_logit, v->d_label_logit,
                      v->d_orient_conf_log, v->d_features_dc, v->d_features_rest, nullptr};
    return check_view_step(v, &p->va, &p->l, p->pg, camera);
}

int run_view_step(void* stream, const ghr_view_step_args* v, ViewStepPlan& p)
{
    const ghr_model_args* m = &v->model;
    const size_t n = (size_t)m->W * m->H;
    ghr_loss_args& l = p.l;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = ghr_model_forward_stage1(stream, m, v->geom_ws, v->img_ws, v->radii, v->means2D_out, v->R_host)) return rc;
    if (v->count_event) GHR_HIP(hipEventRecord((hipEvent_t)v->count_event, s));
    if (int rc = ghr_forward_stage2(stream, &p.va, v->R, v->geom_ws, v->img_ws, v->bin_ws, v->render,
                                    v->prezero ? v->grad_scratch : nullptr))
        return rc;
    if (int rc = ghr_loss_forward(stream, &l, v->maps, v->sums, v->loss_out)) return rc;
    l.gt_stats = nullptr;  // (the backward pass reads no window moments)
    float* d = v->d_pix;     // channels 7 and 9 carry no loss term: zero-filled by the loss backward
    if (int rc = ghr_loss_backward(stream, &l, v->maps, v->sums, v->grad_loss, d, d + 3 * n, d + 5 * n, d + 8 * n, d + 7 * n,
                                   d + 9 * n))
        return rc;
    if (int rc = ghr_render_backward(stream, m->P, m->W, m->H, v->R, m->background, v->geom_ws, v->img_ws, v->bin_ws, d,
                                     v->grad_scratch, v->prezero))
        return rc;
    if (v->acc_wait_event) GHR_HIP(hipStreamWaitEvent(s, (hipEvent_t)v->acc_wait_event, 0));
    if (const ghr_sh_fold_args* f = v->sh_fold)
        if (int rc = ghr_sh_grad_from_views(stream, f->P, f->sh_degree, f->sh_coeffs, f->xyz, f->n_views, f->campos, f->campos_stride,
                                            f->g_views, f->view_stride, f->d_features_dc, f->d_features_rest, f->accumulate,
                                            nullptr, 0))
            return rc;
    if (int rc = backward_segment(m, nullptr, nullptr, stream, m->P, v->radii, v->geom_ws, v->grad_scratch, p.pg, v->accumulate,
                                  v->nan_flag, v->R, v->bin_ws, v->R))
        return rc;
    if (v->acc_record_event) GHR_HIP(hipEventRecord((hipEvent_t)v->acc_record_event, s));
    return GHR_OK;
}
}  // namespace

int ghr_view_step(void* stream, const ghr_view_step_args* v)
{
    ViewStepPlan p;
    if (int rc = plan_view_step(v, false, &p)) return rc;
    return run_view_step(stream, v, p);
}

// ---- evaluation pass (ghr_eval.h) ------------------------------------------------------------------------------------
static bool eval_aligned16(std::initializer_list<const void*> ps)
{
    for (const void* p : ps)
        if (((uintptr_t)p & 15u) != 0) return false;
    return true;
}
// the knob of the loss kernels' tests selects the scalar / tile forms here too
static bool eval_vec_off() { return std::getenv("GHR_LOSS_SCALAR") != nullptr; }

size_t ghr_eval_scratch_floats(int32_t W, int32_t H)
{
    if (W <= 0 || H <= 0) return 0;
    const size_t n_ssim = std::max(ghr::loss_slots_tile(W, H), ghr::loss_slots_march(W, H, GHR_LM_ROWS));
    return (size_t)GHR_EVAL_POINT_TERMS * ghr::eval_point_groups(W, H) + n_ssim;
}

int ghr_eval_metrics(void* stream, const ghr_eval_args* e, float* scratch, double* row)
{
    if (!e || e->W <= 0 || e->H <= 0 || !e->renders || !e->gt_image || !e->gt_mask || !scratch || !row)
        return fail(GHR_E_INVALID, "ghr_eval_metrics: bad args");
    if ((e->gt_orient_angle == nullptr) != (e->gt_orient_conf == nullptr))
        return fail(GHR_E_INVALID, "ghr_eval_metrics: gt_orient_angle and gt_orient_conf come together (both NULL: no orientation terms)");
    if (((uintptr_t)row & 7u) != 0) return fail(GHR_E_INVALID, "ghr_eval_metrics: row must be 8-B aligned");
    hipStream_t s = (hipStream_t)stream;
    const size_t N = (size_t)e->W * (size_t)e->H;
    const uint32_t n_point = ghr::eval_point_groups(e->W, e->H);
    ghr::EvalArgs a{e->W, e->H, e->renders, e->gt_image, e->gt_mask, e->gt_orient_angle, e->gt_orient_conf, scratch, n_point};
    const bool vec = !eval_vec_off() && (N & 3) == 0 &&
                     eval_aligned16({e->renders, e->gt_image, e->gt_mask, e->gt_orient_angle, e->gt_orient_conf});
    if (vec) hipLaunchKernelGGL(ghr::k_eval_points_v, dim3(n_point), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(ghr::k_eval_points, dim3(n_point), dim3(256), 0, s, a);
    float* ssim_slots = scratch + (size_t)GHR_EVAL_POINT_TERMS * n_point;
    uint32_t n_ssim = 0;
    if (e->with_ssim) {
        ghr_loss_args l{};
        l.W = e->W; l.H = e->H; l.image = e->renders; l.gt_image = e->gt_image; l.gt_mask = e->gt_mask;
        const int seg = loss_march_seg(&l, false);
        ghr::LossArgs la{e->W, e->H, e->renders, nullptr, nullptr, nullptr, e->gt_image, e->gt_mask, nullptr, nullptr,
                         0, nullptr, ssim_slots, nullptr, nullptr, seg, 0u};
        if (loss_vec_ok(&l)) {
            n_ssim = (uint32_t)ghr::loss_slots_march(e->W, e->H, seg);
            la.n_slots = n_ssim;
            hipLaunchKernelGGL(ghr::k_eval_ssim_v, loss_march_grid(&l, seg), dim3(64), 0, s, la);
        } else {
            n_ssim = (uint32_t)ghr::loss_slots_tile(e->W, e->H);
            la.n_slots = n_ssim;
            hipLaunchKernelGGL(ghr::k_eval_ssim, dim3((e->W + GHR_L_TW - 1) / GHR_L_TW, (e->H + GHR_L_TH - 1) / GHR_L_TH, 3),
                               dim3(256), 0, s, la);
        }
    }
    hipLaunchKernelGGL(ghr::k_eval_finalize, dim3(1), dim3(256), 0, s, scratch, n_point, ssim_slots, n_ssim, (double)N, row);
    return finish(s, 0);
}

int ghr_eval_products(void* stream, int32_t W, int32_t H, const float* renders, uint8_t* bytes, float* conf)
{
    if (W <= 0 || H <= 0 || !renders || !bytes || !conf) return fail(GHR_E_INVALID, "ghr_eval_products: bad args");
    hipStream_t s = (hipStream_t)stream;
    const size_t N = (size_t)W * (size_t)H, quads = (N + 3) / 4;
    ghr::ProductArgs a{W, H, renders, bytes, conf};
    const dim3 grid((unsigned)((quads + 255) / 256));
    const bool vec = !eval_vec_off() && (N & 3) == 0 && eval_aligned16({renders, conf}) && ((uintptr_t)bytes & 3u) == 0;
    if (vec) hipLaunchKernelGGL(ghr::k_eval_products, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(ghr::k_eval_products_s, grid, dim3(256), 0, s, a);
    return finish(s, 0);
}

// ---- orientation maps (ghr_orient.h) ---------------------------------------------------------------------------------
size_t ghr_orient_dog_scratch_bytes(int32_t W, int32_t H)
{
    if (W <= 0 || H <= 0) return 0;
    return 2 * sizeof(double) * (size_t)W * (size_t)H;
}

int ghr_orient_dog(void* stream, int32_t W, int32_t H, int32_t channels, int32_t is_u8, const void* image, int32_t r_low,
                   const double* w_low, int32_t r_high, const double* w_high, void* scratch, float* filtered)
{
    if (W < 1 || H < 1) return fail(GHR_E_INVALID, "ghr_orient_dog: W and H must be >= 1");
    if (channels != 1 && channels != 3) return fail(GHR_E_INVALID, "ghr_orient_dog: channels must be 1 or 3");
    if (r_low < 0 || r_high < 0) return fail(GHR_E_INVALID, "ghr_orient_dog: negative radius");
    if (!image || !w_low || !w_high || !scratch || !filtered) return fail(GHR_E_INVALID, "ghr_orient_dog: NULL buffer");
    if (((uintptr_t)scratch & 7u) != 0) return fail(GHR_E_INVALID, "ghr_orient_dog: scratch must be 8-B aligned");
    hipStream_t s = (hipStream_t)stream;
    ghr::OrientDogArgs a{W, H, channels, is_u8 != 0, image, r_low, r_high, w_low, w_high, (double*)scratch, filtered};
    const dim3 grid((W + 63) / 64, (H + 3) / 4);
    hipLaunchKernelGGL(ghr::k_orient_dog<0>, grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(ghr::k_orient_dog<1>, grid, dim3(256), 0, s, a);
    return finish(s, 0);
}

static int orient_tiles_per_wave(int32_t n_filters) { return ((n_filters + 15) / 16 + GHR_ORIENT_WAVES - 1) / GHR_ORIENT_WAVES; }

size_t ghr_orient_bank_floats(int32_t n_filters, int32_t ksize)
{
    if (n_filters < 1 || n_filters > GHR_ORIENT_MAX_FILTERS || ksize < 1 || ksize > GHR_ORIENT_MAX_KSIZE || !(ksize & 1)) return 0;
    return (size_t)GHR_ORIENT_WAVES * orient_tiles_per_wave(n_filters) * ((ksize * ksize + 3) / 4) * 64;
}

int ghr_orient_gabor(void* stream, int32_t W, int32_t H, const float* filtered, int32_t n_filters, int32_t ksize,
                     const float* weights, const float* thetas, uint8_t* deg, float* var, float* angle, float* conf,
                     int32_t via_half)
{
    if (W < 1 || H < 1) return fail(GHR_E_INVALID, "ghr_orient_gabor: W and H must be >= 1");
    if (n_filters < 1 || n_filters > GHR_ORIENT_MAX_FILTERS) return fail(GHR_E_INVALID, "ghr_orient_gabor: n_filters must be 1 ... 256");
    if (ksize < 1 || ksize > GHR_ORIENT_MAX_KSIZE || !(ksize & 1)) return fail(GHR_E_INVALID, "ghr_orient_gabor: ksize must be odd and <= 25");
    if (!filtered || !weights || !thetas) return fail(GHR_E_INVALID, "ghr_orient_gabor: NULL buffer");
    hipStream_t s = (hipStream_t)stream;
    ghr::OrientGaborArgs a{W, H, filtered, n_filters, ksize, (ksize * ksize + 3) / 4, weights, thetas, deg, var, angle, conf, via_half != 0};
    const dim3 grid((W + GHR_ORIENT_TW - 1) / GHR_ORIENT_TW, (H + GHR_ORIENT_TH - 1) / GHR_ORIENT_TH), block(64 * GHR_ORIENT_WAVES);
    switch (orient_tiles_per_wave(n_filters)) {
    case 1: hipLaunchKernelGGL(ghr::k_orient_gabor<1>, grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL(ghr::k_orient_gabor<2>, grid, block, 0, s, a); break;
    case 3: hipLaunchKernelGGL(ghr::k_orient_gabor<3>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(ghr::k_orient_gabor<4>, grid, block, 0, s, a);
    }
    return finish(s, 0);
}

// ---- ground-truth loader (ghr_gt.h) ------------------------------------------------------------------------------------
size_t ghr_resample_scratch_bytes(int32_t in_w, int32_t in_h, int32_t out_w, int32_t out_h, int32_t channels)
{
    if (in_w < 1 || in_h < 1 || out_w < 1 || out_h < 1 || (channels != 1 && channels != 3)) return 0;
    if (in_w == out_w || in_h == out_h) return 0;   // one pass or none: no intermediate
    return (size_t)in_h * (size_t)out_w * (size_t)channels;
}

namespace {
// The bounds live on the device and decide which bytes a kernel reads: they are read back on the caller's stream (eight bytes
// per output row or column) and checked before anything is launched.
int resample_check_bounds(hipStream_t s, const char* axis, const int32_t* bounds, int32_t n_out, int32_t ksize, int32_t n_in,
                          int32_t channels, bool* staged)
{
    std::vector<int32_t> h((size_t)n_out * 2);
    GHR_HIP(hipMemcpyAsync(h.data(), bounds, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    GHR_HIP(hipStreamSynchronize(s));
    for (int32_t i = 0; i < n_out; i++) {
        const int32_t lo = h[2 * i], n = h[2 * i + 1];
        if (lo < 0 || n < 0 || n > ksize || lo > n_in - n) {
            std::snprintf(g_err, sizeof(g_err), "ghr_resample_u8: bounds_%s[%d] = (%d, %d) does not fit ksize %d and an input of %d",
                          axis, i, lo, n, ksize, n_in);
            return GHR_E_INVALID;
        }
    }
    // k_resample_u8_h_lds stages the bytes between a workgroup's first window's start and its last window's end: every window
    // of the workgroup has to lie in between, and the span and the taps have to fit its LDS
    // Measured at 2160 x 3840 (profiles/ground_truth_loader.txt): with three channels the staged form is twice as fast as the direct
    // one (33 against 64 us at 11 taps); with one channel it wins at 19 taps (17 against 29 us) and loses at 11 (37 against 24 us),
    // where a workgroup's coefficients are more bytes than its pixels.
    *staged = ksize <= GHR_RESAMPLE_HK && (channels == 3 || ksize > 11);
    for (int32_t f = 0; f < n_out && *staged; f += GHR_RESAMPLE_HC) {
        const int32_t l = std::min(f + GHR_RESAMPLE_HC, n_out) - 1;
        const int32_t x0 = h[2 * f], x1 = h[2 * l] + h[2 * l + 1];
        if ((int64_t)(x1 - x0) * channels > GHR_RESAMPLE_SPAN) *staged = false;
        for (int32_t i = f; i <= l && *staged; i++)
            if (h[2 * i] < x0 || h[2 * i] + h[2 * i + 1] > x1) *staged = false;
    }
    return GHR_OK;
}
}  // namespace

int ghr_resample_u8(void* stream, int32_t in_w, int32_t in_h, int32_t channels, const uint8_t* in, int32_t out_w, int32_t out_h,
                    uint8_t* out, const int32_t* bounds_x, const int32_t* coef_x, int32_t ksize_x, const int32_t* bounds_y,
                    const int32_t* coef_y, int32_t ksize_y, void* scratch)
{
    if (in_w < 1 || in_h < 1 || out_w < 1 || out_h < 1) return fail(GHR_E_INVALID, "ghr_resample_u8: sizes must be >= 1");
    if (channels != 1 && channels != 3) return fail(GHR_E_INVALID, "ghr_resample_u8: channels must be 1 or 3 (RGBA is not built)");
    if (!in || !out) return fail(GHR_E_INVALID, "ghr_resample_u8: NULL image");
    if (in_h > 4 * 65535 || ((size_t)out_w * channels + 1023) / 1024 > 65535)
        return fail(GHR_E_INVALID, "ghr_resample_u8: image too large for the launch grid");
    const bool hor = in_w != out_w, ver = in_h != out_h;
    if (hor && (!bounds_x || !coef_x || ksize_x < 1))
        return fail(GHR_E_INVALID, "ghr_resample_u8: the widths differ: bounds_x, coef_x and ksize_x >= 1 are needed");
    if (ver && (!bounds_y || !coef_y || ksize_y < 1))
        return fail(GHR_E_INVALID, "ghr_resample_u8: the heights differ: bounds_y, coef_y and ksize_y >= 1 are needed");
    if (hor && ver && !scratch) return fail(GHR_E_INVALID, "ghr_resample_u8: two passes need ghr_resample_scratch_bytes of scratch");
    if ((hor || ver) && in == out) return fail(GHR_E_INVALID, "ghr_resample_u8: in and out must not be the same buffer");
    hipStream_t s = (hipStream_t)stream;
    if (!hor && !ver) {   // Pillow returns a copy
        if (in != out) GHR_HIP(hipMemcpyAsync(out, in, (size_t)in_w * in_h * channels, hipMemcpyDeviceToDevice, s));
        return GHR_OK;
    }
    bool staged = false, unused = false;
    if (hor)
        if (int rc = resample_check_bounds(s, "x", bounds_x, out_w, ksize_x, in_w, channels, &staged)) return rc;
    if (ver)
        if (int rc = resample_check_bounds(s, "y", bounds_y, out_h, ksize_y, in_h, channels, &unused)) return rc;
    const uint8_t* mid = in;
    if (hor) {
        uint8_t* dst = ver ? (uint8_t*)scratch : out;
        ghr::ResampleArgs a{in_w, in_h, out_w, in_h, channels, in, dst, bounds_x, coef_x, ksize_x};
        if (staged) {
            const dim3 grid((out_w + GHR_RESAMPLE_HC - 1) / GHR_RESAMPLE_HC, (in_h + GHR_RESAMPLE_HR - 1) / GHR_RESAMPLE_HR);
            if (channels == 3) hipLaunchKernelGGL(ghr::k_resample_u8_h_lds<3>, grid, dim3(256), 0, s, a);
            else hipLaunchKernelGGL(ghr::k_resample_u8_h_lds<1>, grid, dim3(256), 0, s, a);
        } else {
            const dim3 grid((out_w + 63) / 64, (in_h + 3) / 4);
            if (channels == 3) hipLaunchKernelGGL(ghr::k_resample_u8_h<3>, grid, dim3(256), 0, s, a);
            else hipLaunchKernelGGL(ghr::k_resample_u8_h<1>, grid, dim3(256), 0, s, a);
        }
        mid = dst;
    }
    if (ver) {
        ghr::ResampleArgs a{out_w, in_h, out_w, out_h, channels, mid, out, bounds_y, coef_y, ksize_y};
        const size_t row = (size_t)out_w * channels;
        const dim3 grid(out_h, (unsigned)((row + 1023) / 1024));
        const bool vec = (row & 3) == 0 && ((uintptr_t)mid & 3u) == 0 && ((uintptr_t)out & 3u) == 0;
        if (vec) hipLaunchKernelGGL(ghr::k_resample_u8_v<true>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(ghr::k_resample_u8_v<false>, grid, dim3(256), 0, s, a);
    }
    return finish(s, 0);
}

int ghr_gt_assemble(void* stream, int32_t W, int32_t H, const uint8_t* image, const uint8_t* mask_hair, const uint8_t* mask_body,
                    const uint8_t* angle, const float* var, int32_t var_w, int32_t var_h, const float* div255_table,
                    const float* div180_table, int32_t white_background, int32_t binarize, int32_t via_half, float* out_image,
                    float* out_mask, float* out_angle, float* out_conf)
{
    if (W < 1 || H < 1) return fail(GHR_E_INVALID, "ghr_gt_assemble: W and H must be >= 1");
    if (!image || !mask_hair || !mask_body || !div255_table || !out_image || !out_mask)
        return fail(GHR_E_INVALID, "ghr_gt_assemble: NULL buffer");
    if ((angle == nullptr) != (out_angle == nullptr)) return fail(GHR_E_INVALID, "ghr_gt_assemble: angle and out_angle come together");
    if ((var == nullptr) != (out_conf == nullptr)) return fail(GHR_E_INVALID, "ghr_gt_assemble: var and out_conf come together");
    if (angle && !div180_table) return fail(GHR_E_INVALID, "ghr_gt_assemble: angle needs div180_table");
    if (var && (var_w < 1 || var_h < 1)) return fail(GHR_E_INVALID, "ghr_gt_assemble: var_w and var_h must be >= 1");
    if (white_background != 0 && white_background != 1) return fail(GHR_E_INVALID, "ghr_gt_assemble: white_background must be 0 or 1");
    hipStream_t s = (hipStream_t)stream;
    ghr::GtAssembleArgs a{W, H, image, mask_hair, mask_body, angle, var, var_w, var_h, div255_table, div180_table, white_background,
                          binarize != 0, via_half != 0, out_image, out_mask, out_angle, out_conf};
    const size_t N = (size_t)W * H;
    hipLaunchKernelGGL(ghr::k_gt_assemble, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, a);
    return finish(s, 0);
}

int ghr_gt_resize_variance(void* stream, int32_t W, int32_t H, const float* var, int32_t var_w, int32_t var_h, int32_t via_half,
                           float* out)
{
    if (W < 1 || H < 1 || var_w < 1 || var_h < 1) return fail(GHR_E_INVALID, "ghr_gt_resize_variance: sizes must be >= 1");
    if (!var || !out) return fail(GHR_E_INVALID, "ghr_gt_resize_variance: NULL buffer");
    hipStream_t s = (hipStream_t)stream;
    const size_t N = (size_t)W * H;
    hipLaunchKernelGGL(ghr::k_gt_resize_var, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, W, H, var, var_w, var_h,
                       (int)(via_half != 0), out);
    return finish(s, 0);
}

int ghr_gt_from_render(void* stream, int32_t W, int32_t H, const float* renders, const float* div255_table, int32_t white_background,
                       int32_t binarize, float* out_image, float* out_mask, float* out_angle, float* out_conf)
{
    if (W < 1 || H < 1) return fail(GHR_E_INVALID, "ghr_gt_from_render: W and H must be >= 1");
    if (!renders || !div255_table || !out_image || !out_mask || !out_angle || !out_conf)
        return fail(GHR_E_INVALID, "ghr_gt_from_render: NULL buffer");
    if (white_background != 0 && white_background != 1) return fail(GHR_E_INVALID, "ghr_gt_from_render: white_background must be 0 or 1");
    const size_t N = (size_t)W * (size_t)H, quads = (N + 3) / 4, groups = (quads + 255) / 256;
    if (groups > 0x7fffffffu) return fail(GHR_E_INVALID, "ghr_gt_from_render: image too large for the launch grid");
    hipStream_t s = (hipStream_t)stream;
    ghr::GtFromRenderArgs a{W, H, renders, div255_table, white_background, binarize != 0, out_image, out_mask, out_angle, out_conf};
    const dim3 grid((unsigned)groups);
    const bool vec = (N & 3) == 0 && eval_aligned16({renders, out_image, out_mask, out_angle, out_conf});
    if (vec) hipLaunchKernelGGL(ghr::k_gt_from_render<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(ghr::k_gt_from_render<false>, grid, dim3(256), 0, s, a);
    return finish(s, 0);
}

// ---- the comparison video's frame assembly (ghr_compare.h) -------------------------------------------------------------------
namespace {
bool cmp_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}
}  // namespace

int ghr_cmp_over_white(void* stream, int64_t n_pixels, const uint8_t* rgba, uint8_t* rgb)
{
    if (n_pixels < 1) return fail(GHR_E_INVALID, "ghr_cmp_over_white: n_pixels must be >= 1");
    if (!rgba || !rgb) return fail(GHR_E_INVALID, "ghr_cmp_over_white: NULL image");
    const uint64_t groups = (((uint64_t)n_pixels + 3) / 4 + 255) / 256;
    if (groups > 0x7fffffffu) return fail(GHR_E_INVALID, "ghr_cmp_over_white: image too large for the launch grid");
    if (cmp_overlap(rgba, 4 * (size_t)n_pixels, rgb, 3 * (size_t)n_pixels))
        return fail(GHR_E_INVALID, "ghr_cmp_over_white: rgba and rgb must not overlap");
    hipStream_t s = (hipStream_t)stream;
    const bool vec = ((uintptr_t)rgba & 15u) == 0 && ((uintptr_t)rgb & 3u) == 0;
    if (vec) hipLaunchKernelGGL(ghr::k_cmp_over_white<true>, dim3((unsigned)groups), dim3(256), 0, s, n_pixels, rgba, rgb);
    else hipLaunchKernelGGL(ghr::k_cmp_over_white<false>, dim3((unsigned)groups), dim3(256), 0, s, n_pixels, rgba, rgb);
    return finish(s, 0);
}

int ghr_cmp_strip(void* stream, int32_t w, int32_t h, const uint8_t* gt, const uint8_t* preview, int32_t pw, int32_t ph,
                  int32_t pad_left, int32_t pad_top, int32_t crop_left, int32_t crop_top, const uint8_t* render, uint8_t* out)
{
    if (w < 1 || h < 1 || pw < 1 || ph < 1) return fail(GHR_E_INVALID, "ghr_cmp_strip: sizes must be >= 1");
    if (!gt || !preview || !render || !out) return fail(GHR_E_INVALID, "ghr_cmp_strip: NULL image");
    if ((int64_t)w * h > ((int64_t)1 << 36) || (int64_t)pw * ph > ((int64_t)1 << 36) || w > (1 << 27))
        return fail(GHR_E_INVALID, "ghr_cmp_strip: image too large for the launch grid");
    // CenterCrop pads an axis only when the image is shorter than the window there, and then to the window's length exactly
    const int32_t padded_w = pw < w ? w : pw, padded_h = ph < h ? h : ph;
    if (pad_left < 0 || pad_top < 0 || pad_left > padded_w - pw || pad_top > padded_h - ph)
        return fail(GHR_E_INVALID, "ghr_cmp_strip: the padding does not fit: an axis is padded up to the panel's size and no further");
    if (crop_left < 0 || crop_top < 0 || crop_left > padded_w - w || crop_top > padded_h - h)
        return fail(GHR_E_INVALID, "ghr_cmp_strip: the window does not lie inside the padded preview");
    const size_t panel = (size_t)3 * w * h, strip = 3 * panel;
    if (cmp_overlap(out, strip, gt, panel) || cmp_overlap(out, strip, render, panel) ||
        cmp_overlap(out, strip, preview, (size_t)3 * pw * ph))
        return fail(GHR_E_INVALID, "ghr_cmp_strip: out must not overlap an input");
    hipStream_t s = (hipStream_t)stream;
    ghr::CmpStripArgs a{w, h, gt, preview, pw, ph, crop_left - pad_left, crop_top - pad_top, render, out};
    const dim3 grid((unsigned)(((strip + 3) / 4 + 255) / 256));
    const bool vec = (w & 3) == 0 && (((uintptr_t)gt | (uintptr_t)render | (uintptr_t)out) & 3u) == 0;
    if (vec) hipLaunchKernelGGL(ghr::k_cmp_strip<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(ghr::k_cmp_strip<false>, grid, dim3(256), 0, s, a);
    return finish(s, 0);
}

namespace {
int adam_step_range(void* stream, int64_t n, int64_t begin, int64_t count, const float* p_in, const float* m_in,
                    const float* v_in, float* p, float* g, float* m, float* v, int32_t* state, int32_t* flag, int32_t nan_mark,
                    int32_t n_groups, const int64_t* group_end_host, const float* lr_host, double beta1, double beta2,
                    float eps, int32_t nan_guard, int32_t zero_grad, int32_t last, uint32_t skip_mask)
{
    if (n < 0 || begin < 0 || count < 0 || begin + count > n || !p || !g || !m || !v || !state || n_groups <= 0 ||
        n_groups > GHR_ADAM_MAX_GROUPS || !group_end_host || !lr_host)
        return fail(GHR_E_INVALID, "ghr_adam_step: bad args");
    if (nan_guard == 1 && (begin != 0 || count != n))
        return fail(GHR_E_INVALID, "ghr_adam_step_range: the scanning NaN guard needs the whole buffer (use 0 or 2)");
    hipStream_t s = (hipStream_t)stream;
    if (count > 0) {
        ghr::AdamArgs a;
        a.begin = begin; a.n = begin + count; a.p = p; a.g = g; a.m = m; a.v = v; a.state = state; a.n_groups = n_groups;
        for (int i = 0; i < n_groups; i++) { a.end[i] = group_end_host[i]; a.lr[i] = lr_host[i]; }
        a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.zero_grad = zero_grad; a.skip_mask = skip_mask;
        a.p_in = p_in; a.m_in = m_in; a.v_in = v_in; a.flag = flag; a.nan_mark = nan_mark ? flag : nullptr;
        const int blocks = (int)((count + 255) / 256 < 4096 ? (count + 255) / 256 : 4096);
        if (nan_guard == 1)
            hipLaunchKernelGGL(ghr::k_adam_nan_flag, dim3(blocks), dim3(256), 0, s, g, (long long)n, state);
        // four elements per thread where the range and the buffers allow 16-B accesses (GHR_ADAM_SCALAR: the scalar kernel)
        const bool v4 = (begin & 3) == 0 && ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v) |
                                              ((uintptr_t)p_in) | ((uintptr_t)m_in) | ((uintptr_t)v_in)) & 15u) == 0 &&
                        std::getenv("GHR_ADAM_SCALAR") == nullptr;
        if (v4) {
            const long long n4 = (count + 3) / 4;
            const long long cap4 = GHR_ADAM_BLOCKS;
            const int blocks4 = (int)((n4 + 255) / 256 < cap4 ? (n4 + 255) / 256 : cap4);
            hipLaunchKernelGGL(ghr::k_adam_v4, dim3(blocks4 > 0 ? blocks4 : 1), dim3(256), 0, s, a);
        } else {
            hipLaunchKernelGGL(ghr::k_adam, dim3(blocks), dim3(256), 0, s, a);
        }
    }
    if (last && n > 0) hipLaunchKernelGGL(ghr::k_adam_finish, dim3(1), dim3(64), 0, s, state, skip_mask, n_groups);
    return finish(s, 0);
}
}  // namespace

int ghr_adam_step_range(void* stream, int64_t n, int64_t begin, int64_t count, float* p, float* g, float* m, float* v,
                        int32_t* state, int32_t n_groups, const int64_t* group_end_host, const float* lr_host,
                        double beta1, double beta2, float eps, int32_t nan_guard, int32_t zero_grad, int32_t last,
                        uint32_t skip_mask)
{
    return adam_step_range(stream, n, begin, count, nullptr, nullptr, nullptr, p, g, m, v, state, nullptr, 0, n_groups,
                           group_end_host, lr_host, beta1, beta2, eps, nan_guard, zero_grad, last, skip_mask);
}

int ghr_adam_step_range_to(void* stream, int64_t n, int64_t begin, int64_t count, const float* p_in, const float* m_in,
                           const float* v_in, float* p_out, float* g, float* m_out, float* v_out, int32_t* state,
                           int32_t* flag, int32_t nan_mark, int32_t n_groups, const int64_t* group_end_host,
                           const float* lr_host, double beta1, double beta2, float eps, int32_t zero_grad, uint32_t skip_mask)
{
    if (!p_in || !m_in || !v_in) return fail(GHR_E_INVALID, "ghr_adam_step_range_to: NULL input buffer");
    if (nan_mark && !flag) return fail(GHR_E_INVALID, "ghr_adam_step_range_to: nan_mark needs the flag word");
    if (p_in == p_out || m_in == m_out || v_in == v_out)
        return fail(GHR_E_INVALID, "ghr_adam_step_range_to: in and out buffers must differ (ghr_adam_step_range updates in place)");
    // (nan_guard 2: whoever produced the gradients keeps the flag; last 0: the caller's own finish advances the counter)
    return adam_step_range(stream, n, begin, count, p_in, m_in, v_in, p_out, g, m_out, v_out, state, flag, nan_mark, n_groups,
                           group_end_host, lr_host, beta1, beta2, eps, 2, zero_grad, 0, skip_mask);
}

int ghr_adam_step(void* stream, int64_t n, float* p, float* g, float* m, float* v, int32_t* state, int32_t n_groups,
                  const int64_t* group_end_host, const float* lr_host, double beta1, double beta2, float eps,
                  int32_t nan_guard, int32_t zero_grad, uint32_t skip_mask)
{
    return ghr_adam_step_range(stream, n, 0, n, p, g, m, v, state, n_groups, group_end_host, lr_host, beta1, beta2,
                               eps, nan_guard, zero_grad, 1, skip_mask);
}

int ghr_adam_relay_rows(void* stream, int32_t n_groups, const int32_t* width_host, int64_t P_old, int64_t P_new,
                        const int64_t* take, const uint8_t* fresh, const int64_t* child, const float* const* override_host,
                        const float* p_in, const float* m_in, const float* v_in, float* p_out, float* m_out, float* v_out)
{
    if (n_groups <= 0 || n_groups > GHR_ADAM_MAX_GROUPS || !width_host || P_old < 0 || P_new < 0)
        return fail(GHR_E_INVALID, "ghr_adam_relay_rows: bad sizes");
    if (P_new == 0) return GHR_OK;
    if (!take || !fresh || !p_in || !m_in || !v_in || !p_out || !m_out || !v_out)
        return fail(GHR_E_INVALID, "ghr_adam_relay_rows: NULL buffer");
    ghr::RelayArgs a;
    a.P_old = P_old; a.P_new = P_new; a.n_groups = n_groups;
    long long off_old = 0, end_new = 0;
    for (int g = 0; g < n_groups; g++) {
        if (width_host[g] <= 0) return fail(GHR_E_INVALID, "ghr_adam_relay_rows: a group without columns");
        a.width[g] = width_host[g];
        a.off_old[g] = off_old;
        off_old += (long long)width_host[g] * P_old;
        end_new += (long long)width_host[g] * P_new;
        a.end_new[g] = end_new;
        a.override_[g] = override_host ? override_host[g] : nullptr;
        if (a.override_[g] && !child) return fail(GHR_E_INVALID, "ghr_adam_relay_rows: override rows without child indices");
    }
    for (int g = n_groups; g < GHR_ADAM_MAX_GROUPS; g++) { a.width[g] = 1; a.off_old[g] = 0; a.end_new[g] = end_new; a.override_[g] = nullptr; }
    a.take = (const long long*)take; a.fresh = fresh; a.child = (const long long*)child;
    a.p_in = p_in; a.m_in = m_in; a.v_in = v_in; a.p_out = p_out; a.m_out = m_out; a.v_out = v_out;
    hipStream_t s = (hipStream_t)stream;
    const long long blocks_ll = (end_new + 255) / 256;
    const int blocks = (int)(blocks_ll < 16384 ? blocks_ll : 16384);
    hipLaunchKernelGGL(ghr::k_relay_rows, dim3(blocks), dim3(256), 0, s, a);
    return finish(s, 0);
}

int ghr_adam_nan_scan(void* stream, const float* g, int64_t count, int32_t* state)
{
    if (count < 0 || !state || (count > 0 && !g)) return fail(GHR_E_INVALID, "ghr_adam_nan_scan: bad args");
    if (count == 0) return GHR_OK;
    hipStream_t s = (hipStream_t)stream;
    const int blocks = (int)((count + 255) / 256 < 4096 ? (count + 255) / 256 : 4096);
    hipLaunchKernelGGL(ghr::k_adam_nan_flag, dim3(blocks), dim3(256), 0, s, g, (long long)count, state);
    return finish(s, 0);
}

int ghr_mark_visible(void* stream, int32_t P, const float* means3D, const float* viewmatrix,
                     const float* projmatrix, uint8_t* present)
{
    (void)projmatrix;
    if (P < 0) return fail(GHR_E_INVALID, "P < 0");
    if (P == 0) return GHR_OK;
    if (!means3D || !viewmatrix || !present) return fail(GHR_E_INVALID, "ghr_mark_visible: NULL buffer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ghr::k_mark_visible, dim3((P + GHR_BLOCK - 1) / GHR_BLOCK), dim3(GHR_BLOCK), 0, s, P, means3D,
                       viewmatrix, present);
    return finish(s, 0);
}

static_assert(GHR_KNN_ALIGN == ALIGN, "a cloud's regions are aligned like every workspace");

static void knn_boxes(hipStream_t s, const ghr::KnnCloud& c, const float* points, const int64_t* order)
{
    hipLaunchKernelGGL(ghr::k_knn_boxes, dim3((unsigned)c.nsuper), dim3(64 * GHR_KNN_WAVES), 0, s, c, points, (const long long*)order);
}

int ghr_knn_workspace_size(int64_t P, size_t* bytes)
{
    if (!bytes || P < 0 || P >= ((int64_t)1 << 31)) return fail(GHR_E_INVALID, "ghr_knn_workspace_size: bad args");
    *bytes = ghr::knn_layout((uint64_t)P).bytes + ALIGN;
    return GHR_OK;
}

int ghr_knn_keys(void* stream, int64_t P, const float* points, const float* bounds_dev, uint64_t* keys)
{
    if (P < 0 || P >= ((int64_t)1 << 31)) return fail(GHR_E_INVALID, "ghr_knn_keys: P must be in [0, 2^31)");
    if (P == 0) return GHR_OK;
    if (!points || !bounds_dev || !keys) return fail(GHR_E_INVALID, "ghr_knn_keys: NULL buffer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ghr::k_knn_keys, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, (int)P, points, bounds_dev,
                       (unsigned long long*)keys);
    return finish(s, 0);
}

int ghr_knn_mean_dist2(void* stream, int64_t P, const float* points, const int64_t* order, void* ws, float* out)
{
    if (P < 0 || P >= ((int64_t)1 << 31)) return fail(GHR_E_INVALID, "ghr_knn_mean_dist2: P must be in [0, 2^31)");
    if (P == 0) return GHR_OK;
    if (!points || !order || !ws || !out) return fail(GHR_E_INVALID, "ghr_knn_mean_dist2: NULL buffer");
    const ghr::KnnCloud c = ghr::knn_cloud(align_base(ws), (uint64_t)P);
    hipStream_t s = (hipStream_t)stream;
    knn_boxes(s, c, points, order);
    hipLaunchKernelGGL(ghr::k_knn_search, dim3((unsigned)((c.nblocks + GHR_KNN_WAVES - 1) / GHR_KNN_WAVES)),
                       dim3(64 * GHR_KNN_WAVES), 0, s, c, out);
    return finish(s, 0);
}

// ---- cross-cloud nearest neighbour and the chamfer point terms (ghr_nn.h) ------------------------------------------------------
static int nn_sizes(const char* fn, int64_t Px, int64_t Py)
{
    if (Px < 0 || Px >= ((int64_t)1 << 31)) return fail(GHR_E_INVALID, fn, "Px must be in [0, 2^31)");
    if (Py < 0 || Py >= ((int64_t)1 << 31)) return fail(GHR_E_INVALID, fn, "Py must be in [0, 2^31)");
    if (Py == 0) return fail(GHR_E_INVALID, fn, "Py == 0: there is no nearest neighbour in an empty cloud");
    return GHR_OK;
}

int ghr_nn_workspace_size(int64_t Px, int64_t Py, size_t* bytes)
{
    static const char* fn = "ghr_nn_workspace_size: %s";
    if (!bytes) return fail(GHR_E_INVALID, fn, "bytes is NULL");
    if (int rc = nn_sizes(fn, Px, Py)) return rc;
    *bytes = ghr::knn_layout((uint64_t)Px).bytes + ghr::knn_layout((uint64_t)Py).bytes + ALIGN;
    return GHR_OK;
}

int ghr_nn_search(void* stream, int64_t Px, const float* x, const int64_t* order_x, const uint64_t* keys_x_sorted, int64_t Py,
                  const float* y, const int64_t* order_y, const uint64_t* keys_y_sorted, int32_t norm, void* ws, float* dist,
                  int32_t* idx)
{
    static const char* fn = "ghr_nn_search: %s";
    if (int rc = nn_sizes(fn, Px, Py)) return rc;
    if (norm != 1 && norm != 2) return fail(GHR_E_INVALID, fn, "norm must be 1 or 2");
    if (Px == 0) return GHR_OK;
    if (!x || !order_x || !keys_x_sorted) return fail(GHR_E_INVALID, fn, "x, order_x or keys_x_sorted is NULL");
    if (!y || !order_y || !keys_y_sorted) return fail(GHR_E_INVALID, fn, "y, order_y or keys_y_sorted is NULL");
    if (!ws || !dist || !idx) return fail(GHR_E_INVALID, fn, "ws, dist or idx is NULL");
    char* base = align_base(ws);
    const ghr::KnnCloud cx = ghr::knn_cloud(base, (uint64_t)Px);
    const ghr::KnnCloud cy = ghr::knn_cloud(base + ghr::knn_layout((uint64_t)Px).bytes, (uint64_t)Py);
    hipStream_t s = (hipStream_t)stream;
    knn_boxes(s, cx, x, order_x);
    knn_boxes(s, cy, y, order_y);
    const dim3 grid((unsigned)((cx.nblocks + GHR_NN_WAVES - 1) / GHR_NN_WAVES)), block(64 * GHR_NN_WAVES);
    const auto kx = (const unsigned long long*)keys_x_sorted, ky = (const unsigned long long*)keys_y_sorted;
    if (norm == 2) hipLaunchKernelGGL(ghr::k_nn_search<2>, grid, block, 0, s, cx, kx, cy, ky, dist, idx);
    else hipLaunchKernelGGL(ghr::k_nn_search<1>, grid, block, 0, s, cx, kx, cy, ky, dist, idx);
    return finish(s, 0);
}

#ifdef GHR_NN_COUNT_BLOCKS
// measurement build only: reads {candidate blocks scanned, waves} since the last call and zeroes them (synchronises)
int ghr_nn_read_counters(uint64_t* out2)
{
    unsigned long long h[2] = {0, 0}, z[2] = {0, 0};
    GHR_HIP(hipDeviceSynchronize());
    GHR_HIP(hipMemcpyFromSymbol(h, HIP_SYMBOL(ghr::g_nn_count), sizeof(h)));
    GHR_HIP(hipMemcpyToSymbol(HIP_SYMBOL(ghr::g_nn_count), z, sizeof(z)));
    out2[0] = h[0]; out2[1] = h[1];
    return GHR_OK;
}
#endif

int ghr_chamfer_point(void* stream, int64_t Px, int64_t Py, const int32_t* idx, const float* x_normals, const float* y_normals,
                      int32_t abs_cosine, const float* y_weights, float* term, float* weight)
{
    static const char* fn = "ghr_chamfer_point: %s";
    if (int rc = nn_sizes(fn, Px, Py)) return rc;
    if (Px == 0) return GHR_OK;
    if (!idx) return fail(GHR_E_INVALID, fn, "idx is NULL");
    if ((x_normals != nullptr) != (y_normals != nullptr) || (x_normals != nullptr) != (term != nullptr))
        return fail(GHR_E_INVALID, fn, "x_normals, y_normals and term: all three or none");
    if ((y_weights != nullptr) != (weight != nullptr)) return fail(GHR_E_INVALID, fn, "y_weights and weight: both or neither");
    if (!term && !weight) return fail(GHR_E_INVALID, fn, "neither normals nor weights: nothing to compute");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ghr::k_chamfer_point, dim3((unsigned)((Px + GHR_NN_BLOCK - 1) / GHR_NN_BLOCK)), dim3(GHR_NN_BLOCK), 0, s,
                       (int)Px, (int)Py, idx, x_normals, y_normals, abs_cosine, y_weights, term, weight);
    return finish(s, 0);
}

int ghr_chamfer_point_backward(void* stream, int64_t Px, int64_t Py, int32_t norm, const float* x, const float* y, const int32_t* idx,
                               const int64_t* start, const int64_t* members, const float* g_dist, const float* x_normals,
                               const float* y_normals, int32_t abs_cosine, const float* g_cos, float* d_x, float* d_y,
                               float* d_x_normals, float* d_y_normals)
{
    static const char* fn = "ghr_chamfer_point_backward: %s";
    if (int rc = nn_sizes(fn, Px, Py)) return rc;
    if (norm != 1 && norm != 2) return fail(GHR_E_INVALID, fn, "norm must be 1 or 2");
    if (!idx || !start || !members) return fail(GHR_E_INVALID, fn, "idx, start or members is NULL");
    const bool pts = g_dist != nullptr, nrm = g_cos != nullptr;
    if (!pts && !nrm) return fail(GHR_E_INVALID, fn, "neither g_dist nor g_cos: nothing to compute");
    if (pts && (!x || !y || !d_x || !d_y)) return fail(GHR_E_INVALID, fn, "g_dist needs x, y, d_x and d_y");
    if (!pts && (d_x || d_y)) return fail(GHR_E_INVALID, fn, "d_x / d_y without g_dist");
    if (nrm && (!x_normals || !y_normals || !d_x_normals || !d_y_normals))
        return fail(GHR_E_INVALID, fn, "g_cos needs x_normals, y_normals, d_x_normals and d_y_normals");
    if (!nrm && (d_x_normals || d_y_normals)) return fail(GHR_E_INVALID, fn, "d_x_normals / d_y_normals without g_cos");
    hipStream_t s = (hipStream_t)stream;
    const dim3 gx((unsigned)((Px + GHR_NN_BLOCK - 1) / GHR_NN_BLOCK)), gy((unsigned)((Py + GHR_NN_BLOCK - 1) / GHR_NN_BLOCK));
    if (norm == 2) {
        if (Px > 0)
            hipLaunchKernelGGL(ghr::k_chamfer_bwd_x<2>, gx, dim3(GHR_NN_BLOCK), 0, s, (int)Px, (int)Py, x, y, idx, g_dist, x_normals,
                               y_normals, abs_cosine, g_cos, d_x, d_x_normals);
        hipLaunchKernelGGL(ghr::k_chamfer_bwd_y<2>, gy, dim3(GHR_NN_BLOCK), 0, s, (int)Px, (int)Py, x, y, (const long long*)start,
                           (const long long*)members, g_dist, x_normals, y_normals, abs_cosine, g_cos, d_y, d_y_normals);
    } else {
        if (Px > 0)
            hipLaunchKernelGGL(ghr::k_chamfer_bwd_x<1>, gx, dim3(GHR_NN_BLOCK), 0, s, (int)Px, (int)Py, x, y, idx, g_dist, x_normals,
                               y_normals, abs_cosine, g_cos, d_x, d_x_normals);
        hipLaunchKernelGGL(ghr::k_chamfer_bwd_y<1>, gy, dim3(GHR_NN_BLOCK), 0, s, (int)Px, (int)Py, x, y, (const long long*)start,
                           (const long long*)members, g_dist, x_normals, y_normals, abs_cosine, g_cos, d_y, d_y_normals);
    }
    return finish(s, 0);
}

static int check_camera_rows(const char* who, int32_t parametrisation, int32_t rows, int32_t first, int32_t n, const void* consts,
                             int32_t const_stride, const void* params, int32_t param_stride)
{
    if (parametrisation != GHR_CAM_ORTHO6D && parametrisation != GHR_CAM_SE3)
        return fail(GHR_E_INVALID, "%s: unknown parametrisation (GHR_CAMERA_ORTHO6D or GHR_CAMERA_SE3)", who);
    if (first < 0 || n < 0 || rows < 0) return fail(GHR_E_INVALID, "%s: rows / first / n < 0", who);
    if ((int64_t)first + n > rows) return fail(GHR_E_INVALID, "%s: rows [first, first + n) reach past the bank's rows", who);
    if (!consts || !params) return fail(GHR_E_INVALID, "%s: NULL base pointer", who);
    if (const_stride < GHR_CAM_CONST || param_stride < ghr::cam_row(parametrisation))
        return fail(GHR_E_INVALID, "%s: a row stride is smaller than the row", who);
    return GHR_OK;
}

int ghr_camera_compose(void* stream, int32_t parametrisation, int32_t rows, int32_t first, int32_t n, const float* consts,
                       int32_t const_stride, const float* params, int32_t param_stride, float* out, int32_t out_stride)
{
    if (int rc = check_camera_rows("ghr_camera_compose", parametrisation, rows, first, n, consts, const_stride, params, param_stride))
        return rc;
    if (!out) return fail(GHR_E_INVALID, "ghr_camera_compose: NULL base pointer");
    if (out_stride < GHR_CAM_OUT) return fail(GHR_E_INVALID, "ghr_camera_compose: a row stride is smaller than the row");
    if (n == 0) return GHR_OK;
    const ghr::CamArgs a{parametrisation, first, n, consts, const_stride, params, param_stride};
    hipLaunchKernelGGL(ghr::k_cam_compose, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, a, out, out_stride);
    return finish((hipStream_t)stream, 0);
}

int ghr_camera_compose_backward(void* stream, int32_t parametrisation, int32_t rows, int32_t first, int32_t n, const float* consts,
                                int32_t const_stride, const float* params, int32_t param_stride, const float* d_view,
                                const float* d_full, const float* d_proj, const float* d_center, const float* d_fovx,
                                const float* d_fovy, float* grads, int32_t grad_stride, int32_t* touched, int32_t train_mask)
{
    if (int rc = check_camera_rows("ghr_camera_compose_backward", parametrisation, rows, first, n, consts, const_stride, params,
                                   param_stride))
        return rc;
    if (!grads || !touched) return fail(GHR_E_INVALID, "ghr_camera_compose_backward: NULL base pointer");
    if (grad_stride < ghr::cam_row(parametrisation))
        return fail(GHR_E_INVALID, "ghr_camera_compose_backward: a row stride is smaller than the row");
    if (train_mask & ~(GHR_CAM_TRAIN_POSE | GHR_CAM_TRAIN_FOV)) return fail(GHR_E_INVALID, "ghr_camera_compose_backward: bad train_mask");
    if (n == 0 || train_mask == 0) return GHR_OK;
    const ghr::CamArgs a{parametrisation, first, n, consts, const_stride, params, param_stride};
    const ghr::CamCotangents d{d_view, d_full, d_proj, d_center, d_fovx, d_fovy};
    hipLaunchKernelGGL(ghr::k_cam_compose_bwd, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, a, d, grads, grad_stride,
                       touched, train_mask);
    return finish((hipStream_t)stream, 0);
}

int ghr_camera_adam_step(void* stream, int32_t parametrisation, int32_t n, float* params, float* grads, float* exp_avg,
                         float* exp_avg_sq, int32_t stride, int32_t* steps, int32_t* touched, float lr_rotation,
                         float lr_translation, float lr_fov, double beta1, double beta2, float eps, int32_t train_mask)
{
    if (parametrisation != GHR_CAM_ORTHO6D && parametrisation != GHR_CAM_SE3)
        return fail(GHR_E_INVALID, "ghr_camera_adam_step: unknown parametrisation (GHR_CAMERA_ORTHO6D or GHR_CAMERA_SE3)");
    if (n < 0) return fail(GHR_E_INVALID, "ghr_camera_adam_step: n < 0");
    if (!params || !grads || !exp_avg || !exp_avg_sq || !steps || !touched)
        return fail(GHR_E_INVALID, "ghr_camera_adam_step: NULL base pointer");
    if (stride < ghr::cam_row(parametrisation)) return fail(GHR_E_INVALID, "ghr_camera_adam_step: the row stride is smaller than the row");
    if (train_mask & ~(GHR_CAM_TRAIN_POSE | GHR_CAM_TRAIN_FOV)) return fail(GHR_E_INVALID, "ghr_camera_adam_step: bad train_mask");
    if (n == 0) return GHR_OK;
    hipLaunchKernelGGL(ghr::k_cam_adam, dim3(1), dim3(GHR_CAM_ADAM_THREADS), 0, (hipStream_t)stream, parametrisation, n, params,
                       grads, exp_avg, exp_avg_sq, stride, steps, touched, lr_rotation, lr_translation, lr_fov, beta1, beta2, eps,
                       train_mask);
    return finish((hipStream_t)stream, 0);
}

// ---- a training view with a bank camera (include/ghr.h, ghr_view_step_camera) and the exchange of a replicated bank's rows ---------
namespace {
int vc_bad(const char* what) { return fail(GHR_E_INVALID, "ghr_view_step_camera: %s", what); }
}  // namespace

int ghr_view_step_camera(void* stream, const ghr_view_step_args* v, const ghr_view_camera_args* c)
{
    if (!v) return vc_bad("the view's argument struct is NULL");
    if (!c) return vc_bad("the camera's argument struct (c) is NULL");
    // the camera's side first, in its own words; then everything ghr_view_step refuses; nothing is launched before both passed
    if (c->rows < 0 || c->index < 0 || c->index >= c->rows) return vc_bad("index outside rows");
    if (int rc = check_camera_rows("ghr_view_step_camera", c->parametrisation, c->rows, c->index, 1, c->consts, c->const_stride,
                                   c->params, c->param_stride))
        return rc;
    if (c->train_mask == 0) return vc_bad("train_mask is 0: a bank with both groups frozen is a constant camera (ghr_view_step)");
    if (c->train_mask & ~(GHR_CAM_TRAIN_POSE | GHR_CAM_TRAIN_FOV)) return vc_bad("bad train_mask");
    if (!c->grads) return vc_bad("grads is NULL");
    if (!c->touched) return vc_bad("touched is NULL");
    if (c->grad_stride < ghr::cam_row(c->parametrisation)) return vc_bad("grad_stride is smaller than the row");
    if (!c->out_row) return vc_bad("out_row is NULL");
    if (!c->d_cam) return vc_bad("d_cam is NULL");
    const ghr_model_args* m = &v->model;
    if (!m->cam_partial) return vc_bad("model.cam_partial is NULL");
    if (m->cam_slot0 != 0 || m->cam_slots != ghr_camera_slots(m->P))
        return vc_bad("model.cam_slots must be ghr_camera_slots(model.P) (and model.cam_slot0 0): the view has one segment");
    if (!m->fovx_dev || !m->fovy_dev) return vc_bad("model.fovx_dev / fovy_dev is NULL");
    if (m->viewmatrix != c->out_row) return vc_bad("model.viewmatrix must be out_row");
    if (m->projmatrix != c->out_row + 16) return vc_bad("model.projmatrix must be out_row + 16");
    if (m->campos != c->out_row + 48) return vc_bad("model.campos must be out_row + 48");
    if (m->fovx_dev != c->out_row + 51) return vc_bad("model.fovx_dev must be out_row + 51");
    if (m->fovy_dev != c->out_row + 52) return vc_bad("model.fovy_dev must be out_row + 52");
    ViewStepPlan p;
    if (int rc = plan_view_step(v, true, &p)) return rc;
    if (int rc = ghr_camera_compose(stream, c->parametrisation, c->rows, c->index, 1, c->consts, c->const_stride, c->params,
                                    c->param_stride, c->out_row, GHR_CAM_OUT))
        return rc;
    if (int rc = run_view_step(stream, v, p)) return rc;
    if (int rc = ghr_camera_grad_fold(stream, m->cam_partial, m->cam_slots, c->d_cam, m->fovx_dev, m->fovy_dev)) return rc;
    const float* d = c->d_cam;
    return ghr_camera_compose_backward(stream, c->parametrisation, c->rows, c->index, 1, c->consts, c->const_stride, c->params,
                                       c->param_stride, d, d + 16, nullptr, d + 32, d + 35, d + 36, c->grads, c->grad_stride,
                                       c->touched, c->train_mask);
}

static int check_camera_exchange(const char* who, int32_t n, int32_t width, int32_t grad_stride)
{
    if (n < 0) return fail(GHR_E_INVALID, "%s: n < 0", who);
    if (width != ghr::cam_row(GHR_CAM_SE3) && width != ghr::cam_row(GHR_CAM_ORTHO6D))
        return fail(GHR_E_INVALID, "%s: width must be 8 (se(3)) or 11 (ortho-6D)", who);
    if (grad_stride < width) return fail(GHR_E_INVALID, "%s: grad_stride is smaller than the row", who);
    return GHR_OK;
}

int ghr_camera_pack_row_message(void* stream, int32_t n, int32_t width, const float* grads, int32_t grad_stride,
                                const int32_t* touched, float* message)
{
    if (int rc = check_camera_exchange("ghr_camera_pack_row_message", n, width, grad_stride)) return rc;
    if (!grads) return fail(GHR_E_INVALID, "ghr_camera_pack_row_message: grads is NULL");
    if (!touched) return fail(GHR_E_INVALID, "ghr_camera_pack_row_message: touched is NULL");
    if (!message) return fail(GHR_E_INVALID, "ghr_camera_pack_row_message: message is NULL");
    if (n == 0) return GHR_OK;
    const size_t total = (size_t)n * (size_t)(width + 1);
    hipLaunchKernelGGL(ghr::k_cam_pack, dim3((unsigned)((total + GHR_CAM_XCHG_THREADS - 1) / GHR_CAM_XCHG_THREADS)),
                       dim3(GHR_CAM_XCHG_THREADS), 0, (hipStream_t)stream, n, width, grads, grad_stride, touched, message);
    return finish((hipStream_t)stream, 0);
}

int ghr_camera_merge_ranks(void* stream, int32_t n, int32_t width, int32_t G, const float* gathered, float* grads,
                           int32_t grad_stride, int32_t* touched)
{
    if (int rc = check_camera_exchange("ghr_camera_merge_ranks", n, width, grad_stride)) return rc;
    if (G < 1) return fail(GHR_E_INVALID, "ghr_camera_merge_ranks: G < 1");
    if (!gathered) return fail(GHR_E_INVALID, "ghr_camera_merge_ranks: gathered is NULL");
    if (!grads) return fail(GHR_E_INVALID, "ghr_camera_merge_ranks: grads is NULL");
    if (!touched) return fail(GHR_E_INVALID, "ghr_camera_merge_ranks: touched is NULL");
    if (n == 0) return GHR_OK;
    const size_t total = (size_t)n * (size_t)width;
    hipLaunchKernelGGL(ghr::k_cam_merge, dim3((unsigned)((total + GHR_CAM_XCHG_THREADS - 1) / GHR_CAM_XCHG_THREADS)),
                       dim3(GHR_CAM_XCHG_THREADS), 0, (hipStream_t)stream, n, width, G, gathered, grads, grad_stride, touched);
    return finish((hipStream_t)stream, 0);
}

int ghr_selftest_wave(void* stream, const float* in, float* out)
{
    if (!in || !out) return fail(GHR_E_INVALID, "ghr_selftest_wave: NULL buffer");
    hipLaunchKernelGGL(ghr::k_wave_selftest, dim3(1), dim3(64), 0, (hipStream_t)stream, in, out);
    return finish((hipStream_t)stream, 1);
}

int ghr_selftest_math(void* stream, int32_t n, const float* in, float* out)
{
    if (n < 0 || (n > 0 && (!in || !out))) return fail(GHR_E_INVALID, "ghr_selftest_math: bad arguments");
    if (n == 0) return GHR_OK;
    hipLaunchKernelGGL(ghr::k_math_selftest, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, in, out);
    return finish((hipStream_t)stream, 1);
}

int ghr_set_deterministic(int32_t on)
{
    const int prev = g_deterministic;
    g_deterministic = on != 0;
    return prev;
}

int ghr_set_profile_events(void* fwd_start, void* fwd_stop, void* bwd_start, void* bwd_stop)
{
    g_ev[0] = (hipEvent_t)fwd_start; g_ev[1] = (hipEvent_t)fwd_stop;
    g_ev[2] = (hipEvent_t)bwd_start; g_ev[3] = (hipEvent_t)bwd_stop;
    return GHR_OK;
}

#ifdef GHR_K8_PROF
// kernel-experiment builds only (not declared in include/ghr.h): per-wave phase cycles of the instrumented K8
int ghr_debug_prof(unsigned long long* out, int n_slots, int reset)
{
    if (n_slots < 0 || n_slots > GHR_PROF_SLOTS) return GHR_E_INVALID;
    if (hipDeviceSynchronize() != hipSuccess) return GHR_E_HIP;
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(ghr::g_k8_prof), 64 * (size_t)n_slots) != hipSuccess) return GHR_E_HIP;
    if (reset) {
        void* p = nullptr;
        if (hipGetSymbolAddress(&p, HIP_SYMBOL(ghr::g_k8_prof)) != hipSuccess) return GHR_E_HIP;
        if (hipMemset(p, 0, 64 * (size_t)GHR_PROF_SLOTS) != hipSuccess) return GHR_E_HIP;
    }
    return GHR_OK;
}
int ghr_debug_timeline(unsigned long long* out, int n_slots)
{
    if (!out || n_slots < 0 || n_slots > GHR_PROF_SLOTS) return GHR_E_INVALID;
    if (hipDeviceSynchronize() != hipSuccess) return GHR_E_HIP;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(ghr::g_k8_tl), 16 * (size_t)n_slots) != hipSuccess) return GHR_E_HIP;
    return GHR_OK;
}
#endif

int ghr_ws_inspect(int32_t P, int32_t W, int32_t H, int32_t mode_b, uint32_t R, const void* geom_ws,
                   const void* img_ws, const void* bin_ws, ghr_ws_view* out)
{
    if (!out || P < 0 || W <= 0 || H <= 0) return fail(GHR_E_INVALID, "ghr_ws_inspect: bad args");
    const ViewWs w = carve_view((size_t)P, W, H, mode_b != 0, R, geom_ws, img_ws, bin_ws);
    out->rec = (const float*)w.g.rec;
    out->depths = w.g.depths;
    out->rects = (const uint32_t*)w.g.rects;
    out->cov3D = w.g.cov3D;
    out->final_T = w.im.final_T;
    out->n_contrib = w.im.n_contrib;
    out->tile_start = w.im.tile_start;
    out->keys = w.b.keys;
    out->point_list = w.b.point_list;
    return GHR_OK;
}

// ---- the latent-strand stage (include/ghr.h; csrc/ghr_latent.h) -----------------------------------------------------------
namespace {
int lt_bad(const char* fn, const char* what) { return fail(GHR_E_INVALID, fn, what); }
inline bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline unsigned lt_blocks(size_t n) { return (unsigned)((n + GHR_LATENT_BLOCK - 1) / GHR_LATENT_BLOCK); }

int lt_points_shape(const char* fn, int32_t S, int32_t L)
{
    if (S < 0) return lt_bad(fn, "S < 0");
    if (L < 2) return lt_bad(fn, "L < 2");
    if ((int64_t)S * L > (int64_t)INT32_MAX / 4) return lt_bad(fn, "S * L too large");
    return GHR_OK;
}
int lt_rows_shape(const char* fn, int32_t S, int32_t n_seg, int32_t C)
{
    if (S < 0) return lt_bad(fn, "S < 0");
    if (n_seg < 1) return lt_bad(fn, "n_seg < 1");
    if (C < 1) return lt_bad(fn, "C < 1");
    if ((int64_t)S * n_seg > (int64_t)INT32_MAX / 4) return lt_bad(fn, "S * n_seg too large");
    return GHR_OK;
}
// the whole struct, before any launch
int lt_loss_check(const char* fn, const ghr_latent_loss_args* l)
{
    if (!l) return lt_bad(fn, "args is NULL");
    if (l->W <= 0 || l->H <= 0) return lt_bad(fn, "W * H == 0");
    if ((int64_t)l->W * l->H > ((int64_t)1 << 30)) return lt_bad(fn, "W * H too large");
    if (!l->image) return lt_bad(fn, "image is NULL");
    if (!l->mask0) return lt_bad(fn, "mask0 is NULL");
    if (!l->dir2d) return lt_bad(fn, "dir2d is NULL");
    if (!l->gt_image) return lt_bad(fn, "gt_image is NULL");
    if (!l->gt_mask0) return lt_bad(fn, "gt_mask0 is NULL");
    if (!l->gt_orient_angle) return lt_bad(fn, "gt_orient_angle is NULL");
    return GHR_OK;
}
ghr::LatentLossArgs lt_loss_args(const ghr_latent_loss_args* l, float* sums, const float* grad_loss, float* d_packed)
{
    return ghr::LatentLossArgs{l->W, l->H, l->image, l->mask0, l->dir2d, l->orient_conf, l->gt_image, l->gt_mask0,
                               l->gt_orient_angle, l->gt_orient_conf, l->w_l1, l->w_mask, l->w_orient, sums, grad_loss, d_packed};
}
// the float4 form: 16-B aligned planes of H W % 4 == 0 pixels (GHR_LATENT_SCALAR: test / measurement knob, read per call)
bool lt_loss_vec(const ghr_latent_loss_args* l, const void* extra)
{
    if (std::getenv("GHR_LATENT_SCALAR") != nullptr || (((size_t)l->W * (size_t)l->H) & 3u) != 0) return false;
    const void* ps[] = {l->image, l->mask0, l->dir2d, l->orient_conf, l->gt_image, l->gt_mask0, l->gt_orient_angle,
                        l->gt_orient_conf, extra};
    for (const void* p : ps)
        if (!al16(p)) return false;
    return true;
}
inline size_t lt_loss_wgs(int32_t W, int32_t H)
{
    const size_t per = (size_t)GHR_LATENT_BLOCK * GHR_LATENT_QUAD;
    return ((size_t)W * (size_t)H + per - 1) / per;
}
}  // namespace

int ghr_strand_points_build(void* stream, int32_t S, int32_t L, const float* p, float scale, float* xyz, float* rotation,
                            float* scaling, float* dir_rows)
{
    static const char* fn = "ghr_strand_points_build: %s";
    if (int rc = lt_points_shape(fn, S, L)) return rc;
    if (S == 0) return GHR_OK;
    if (!p) return lt_bad(fn, "p is NULL");
    if (!xyz) return lt_bad(fn, "xyz is NULL");
    if (!rotation) return lt_bad(fn, "rotation is NULL");
    if (!al16(rotation)) return lt_bad(fn, "rotation is not 16-B aligned");
    if (!scaling) return lt_bad(fn, "scaling is NULL");
    if (!dir_rows) return lt_bad(fn, "dir_rows is NULL");
    hipStream_t s = (hipStream_t)stream;
    ghr::PointsArgs a{S, L, p, scale, xyz, rotation, scaling, dir_rows};
    hipLaunchKernelGGL(ghr::k_points_build, dim3(lt_blocks((size_t)S * (L - 1))), dim3(GHR_LATENT_BLOCK), 0, s, a);
    return finish(s, 0);
}

int ghr_strand_points_build_backward(void* stream, int32_t S, int32_t L, const float* p, const float* d_xyz,
                                     const float* d_rotation, const float* d_scaling, const float* d_dir_rows, float* d_p)
{
    static const char* fn = "ghr_strand_points_build_backward: %s";
    if (int rc = lt_points_shape(fn, S, L)) return rc;
    if (S == 0) return GHR_OK;
    if (!p) return lt_bad(fn, "p is NULL");
    if (!d_p) return lt_bad(fn, "d_p is NULL");
    hipStream_t s = (hipStream_t)stream;
    ghr::PointsBwdArgs a{S, L, p, d_xyz, d_rotation, d_scaling, d_dir_rows, d_p};
    hipLaunchKernelGGL(ghr::k_points_build_bwd, dim3(lt_blocks((size_t)S * L)), dim3(GHR_LATENT_BLOCK), 0, s, a);
    return finish(s, 0);
}

int ghr_strand_rows_expand(void* stream, int32_t S, int32_t n_seg, int32_t C, const float* src, float* dst)
{
    static const char* fn = "ghr_strand_rows_expand: %s";
    if (int rc = lt_rows_shape(fn, S, n_seg, C)) return rc;
    if (S == 0) return GHR_OK;
    if (!src) return lt_bad(fn, "src is NULL");
    if (!dst) return lt_bad(fn, "dst is NULL");
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)S * n_seg * C;
    if ((C & 3) == 0 && al16(src) && al16(dst))
        hipLaunchKernelGGL(ghr::k_rows_expand<4>, dim3(lt_blocks(n / 4)), dim3(GHR_LATENT_BLOCK), 0, s, n / 4, n_seg, C, src, dst);
    else
        hipLaunchKernelGGL(ghr::k_rows_expand<1>, dim3(lt_blocks(n)), dim3(GHR_LATENT_BLOCK), 0, s, n, n_seg, C, src, dst);
    return finish(s, 0);
}

int ghr_strand_rows_reduce(void* stream, int32_t S, int32_t n_seg, int32_t C, const float* g, float* out)
{
    static const char* fn = "ghr_strand_rows_reduce: %s";
    if (int rc = lt_rows_shape(fn, S, n_seg, C)) return rc;
    if (S == 0) return GHR_OK;
    if (!g) return lt_bad(fn, "g is NULL");
    if (!out) return lt_bad(fn, "out is NULL");
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)S * C;
    if ((C & 3) == 0 && al16(g) && al16(out))
        hipLaunchKernelGGL(ghr::k_rows_reduce<4>, dim3(lt_blocks(n / 4)), dim3(GHR_LATENT_BLOCK), 0, s, n / 4, n_seg, C, g, out);
    else
        hipLaunchKernelGGL(ghr::k_rows_reduce<1>, dim3(lt_blocks(n)), dim3(GHR_LATENT_BLOCK), 0, s, n, n_seg, C, g, out);
    return finish(s, 0);
}

size_t ghr_latent_loss_sums_floats(int32_t W, int32_t H)
{
    if (W <= 0 || H <= 0) return 0;
    return GHR_LATENT_AUX + GHR_LATENT_TERMS * lt_loss_wgs(W, H);
}

int ghr_latent_loss_forward(void* stream, const ghr_latent_loss_args* l, float* sums, float* loss_out)
{
    static const char* fn = "ghr_latent_loss_forward: %s";
    if (int rc = lt_loss_check(fn, l)) return rc;
    if (!sums) return lt_bad(fn, "sums is NULL");
    if (!al16(sums)) return lt_bad(fn, "sums is not 16-B aligned");
    if (!loss_out) return lt_bad(fn, "loss_out is NULL");
    hipStream_t s = (hipStream_t)stream;
    const ghr::LatentLossArgs a = lt_loss_args(l, sums, nullptr, nullptr);
    const unsigned wgs = (unsigned)lt_loss_wgs(l->W, l->H);
    if (lt_loss_vec(l, nullptr)) hipLaunchKernelGGL(ghr::k_latent_loss_fwd<1>, dim3(wgs), dim3(GHR_LATENT_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(ghr::k_latent_loss_fwd<0>, dim3(wgs), dim3(GHR_LATENT_BLOCK), 0, s, a);
    hipLaunchKernelGGL(ghr::k_latent_loss_fold, dim3(1), dim3(GHR_LATENT_BLOCK), 0, s, a, (uint32_t)wgs, loss_out);
    return finish(s, 0);
}

int ghr_latent_loss_backward(void* stream, const ghr_latent_loss_args* l, const float* sums, const float* grad_loss,
                             float* d_packed)
{
    static const char* fn = "ghr_latent_loss_backward: %s";
    if (int rc = lt_loss_check(fn, l)) return rc;
    if (!sums) return lt_bad(fn, "sums is NULL");
    if (!d_packed) return lt_bad(fn, "d_packed is NULL");
    hipStream_t s = (hipStream_t)stream;
    const ghr::LatentLossArgs a = lt_loss_args(l, const_cast<float*>(sums), grad_loss, d_packed);
    const unsigned wgs = (unsigned)lt_loss_wgs(l->W, l->H);
    if (lt_loss_vec(l, d_packed)) hipLaunchKernelGGL(ghr::k_latent_loss_bwd<1>, dim3(wgs), dim3(GHR_LATENT_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(ghr::k_latent_loss_bwd<0>, dim3(wgs), dim3(GHR_LATENT_BLOCK), 0, s, a);
    return finish(s, 0);
}

}  // extern "C"

// ---- containment in a triangle mesh (include/ghr.h; csrc/ghr_mesh.h) ---------------------------------------------------------
namespace {
static_assert(sizeof(ghr_mesh_grid) == sizeof(ghr::MeshGrid), "ghr_mesh_grid is ghr::MeshGrid");

int mesh_header_check(const char* fn, const ghr_mesh_grid* h, const void* grid_dev)
{
    if (!h) return lt_bad(fn, "header is NULL");
    if (h->magic != GHR_MESH_MAGIC) return lt_bad(fn, "header is not a grid header (magic)");
    if (h->G < 1 || h->G > GHR_MESH_G_MAX) return lt_bad(fn, "header.G outside 1 .. 256");
    if (h->n_faces < 0) return lt_bad(fn, "header.n_faces < 0");
    if (!grid_dev) return lt_bad(fn, "grid_dev is NULL");
    if (!al16(grid_dev)) return lt_bad(fn, "grid_dev is not 16-B aligned");
    const uint64_t cells = (uint64_t)h->G * h->G;
    for (int a = 0; a < 3; a++) {
        if ((h->off_rec[a] | h->off_start[a] | h->off_list[a]) & 15u) return lt_bad(fn, "header offsets are not 16-B aligned");
        if (h->off_rec[a] + 4ull * GHR_MESH_REC_WORDS * (uint64_t)h->n_faces > h->bytes ||
            h->off_start[a] + 4ull * (cells + 1) > h->bytes || h->off_list[a] + 4ull * h->list_total[a] > h->bytes)
            return lt_bad(fn, "header offsets reach past header.bytes");
    }
    return GHR_OK;
}
}  // namespace

extern "C" {

int ghr_mesh_grid_sizes(int32_t n_vertices, const float* vertices, int32_t n_faces, const int32_t* faces, int32_t G,
                        ghr_mesh_grid* header)
{
    static const char* fn = "ghr_mesh_grid_sizes: %s";
    if (!header) return lt_bad(fn, "header is NULL");
    if (const char* why = ghr::mesh_grid_plan(n_vertices, vertices, n_faces, faces, G, reinterpret_cast<ghr::MeshGrid*>(header)))
        return lt_bad(fn, why);
    return GHR_OK;
}

int ghr_mesh_grid_build(int32_t n_vertices, const float* vertices, int32_t n_faces, const int32_t* faces, int32_t G,
                        void* blob, size_t bytes)
{
    static const char* fn = "ghr_mesh_grid_build: %s";
    ghr::MeshGrid plan;
    if (const char* why = ghr::mesh_grid_plan(n_vertices, vertices, n_faces, faces, G, &plan)) return lt_bad(fn, why);
    if (!blob) return lt_bad(fn, "blob is NULL");
    if (!al16(blob)) return lt_bad(fn, "blob is not 16-B aligned");
    if ((uint64_t)bytes != plan.bytes) return lt_bad(fn, "bytes is not what ghr_mesh_grid_sizes reports for this mesh and G");
    if (const char* why = ghr::mesh_grid_fill(vertices, faces, plan, blob)) return lt_bad(fn, why);
    return GHR_OK;
}

int ghr_mesh_contains(void* stream, const ghr_mesh_grid* header, const void* grid_dev, int64_t Q, const float* points,
                      uint8_t* inside, uint32_t* crossings)
{
    static const char* fn = "ghr_mesh_contains: %s";
    if (int rc = mesh_header_check(fn, header, grid_dev)) return rc;
    if (Q < 0) return lt_bad(fn, "Q < 0");
    if (Q > ((int64_t)1 << 40)) return lt_bad(fn, "Q too large");
    if (Q == 0) return GHR_OK;
    if (!points) return lt_bad(fn, "points is NULL");
    if (!inside) return lt_bad(fn, "inside is NULL");
    const uint64_t blocks = ((uint64_t)Q + GHR_MESH_BLOCK - 1) / GHR_MESH_BLOCK;
    if (blocks > 0x7fffffffull) return lt_bad(fn, "Q too large");
    hipStream_t s = (hipStream_t)stream;
    ghr::MeshQueryArgs a{ghr::mesh_view(*reinterpret_cast<const ghr::MeshGrid*>(header), grid_dev), Q, points, inside, crossings};
    hipLaunchKernelGGL(ghr::k_mesh_contains, dim3((unsigned)blocks), dim3(GHR_MESH_BLOCK), 0, s, a);
    return finish(s, 0);
}

int ghr_gaussian_probe_outside(void* stream, const ghr_mesh_grid* header, const void* grid_dev, int64_t P, const float* xyz,
                               const float* scaling, const float* rotation, int32_t probe, uint8_t* outside)
{
    static const char* fn = "ghr_gaussian_probe_outside: %s";
    if (int rc = mesh_header_check(fn, header, grid_dev)) return rc;
    if (probe != GHR_PROBE_REFERENCE && probe != GHR_PROBE_AXIS_SCALED) return lt_bad(fn, "probe is neither GHR_PROBE_REFERENCE nor GHR_PROBE_AXIS_SCALED");
    if (P < 0) return lt_bad(fn, "P < 0");
    if (P == 0) return GHR_OK;
    if (!xyz) return lt_bad(fn, "xyz is NULL");
    if (!scaling) return lt_bad(fn, "scaling is NULL");
    if (!rotation) return lt_bad(fn, "rotation is NULL");
    if (!outside) return lt_bad(fn, "outside is NULL");
    const uint64_t blocks = ((uint64_t)P * 16 + GHR_MESH_BLOCK - 1) / GHR_MESH_BLOCK;  // a 16-lane row per Gaussian
    if (P > ((int64_t)1 << 36) || blocks > 0x7fffffffull) return lt_bad(fn, "P too large");
    hipStream_t s = (hipStream_t)stream;
    ghr::MeshProbeArgs a{ghr::mesh_view(*reinterpret_cast<const ghr::MeshGrid*>(header), grid_dev), P, probe, xyz, scaling, rotation,
                         outside};
    hipLaunchKernelGGL(ghr::k_gaussian_probe_outside, dim3((unsigned)blocks), dim3(GHR_MESH_BLOCK), 0, s, a);
    return finish(s, 0);
}

}  // extern "C"

// ---- closest point on a triangle mesh (include/ghr.h; csrc/ghr_meshdist.h) ----------------------------------------------------
namespace {
static_assert(sizeof(ghr_mesh_tris) == sizeof(ghr::MeshTris), "ghr_mesh_tris is ghr::MeshTris");

int tris_header_check(const char* fn, const ghr_mesh_tris* h, const void* tris_dev)
{
    if (!h) return lt_bad(fn, "header is NULL");
    if (h->magic != GHR_MD_MAGIC) return lt_bad(fn, "header is not a triangle-blob header (magic)");
    if (h->n_faces < 1) return lt_bad(fn, "header.n_faces < 1");
    if (h->n_blocks != (h->n_faces + GHR_KNN_BLOCK - 1) / GHR_KNN_BLOCK || h->n_super != (h->n_blocks + GHR_KNN_SUPER - 1) / GHR_KNN_SUPER)
        return lt_bad(fn, "header.n_blocks / n_super do not belong to header.n_faces");
    if (!tris_dev) return lt_bad(fn, "tris_dev is NULL");
    if (!al16(tris_dev)) return lt_bad(fn, "tris_dev is not 16-B aligned");
    if ((h->off_rec | h->off_bbox | h->off_sbox | h->off_keys) & 15u) return lt_bad(fn, "header offsets are not 16-B aligned");
    if (h->off_rec + 4ull * GHR_MD_REC_WORDS * (uint64_t)h->n_faces > h->bytes || h->off_bbox + 32ull * (uint64_t)h->n_blocks > h->bytes ||
        h->off_sbox + 32ull * (uint64_t)h->n_super > h->bytes || h->off_keys + 8ull * (uint64_t)h->n_blocks > h->bytes)
        return lt_bad(fn, "header offsets reach past header.bytes");
    return GHR_OK;
}
}  // namespace

extern "C" {

int ghr_mesh_tris_sizes(int32_t n_vertices, const float* vertices, int32_t n_faces, const int32_t* faces, ghr_mesh_tris* header)
{
    static const char* fn = "ghr_mesh_tris_sizes: %s";
    if (!header) return lt_bad(fn, "header is NULL");
    if (const char* why = ghr::mesh_tris_plan(n_vertices, vertices, n_faces, faces, reinterpret_cast<ghr::MeshTris*>(header)))
        return lt_bad(fn, why);
    return GHR_OK;
}

int ghr_mesh_tris_build(int32_t n_vertices, const float* vertices, int32_t n_faces, const int32_t* faces, void* blob, size_t bytes)
{
    static const char* fn = "ghr_mesh_tris_build: %s";
    ghr::MeshTris plan;
    if (const char* why = ghr::mesh_tris_plan(n_vertices, vertices, n_faces, faces, &plan)) return lt_bad(fn, why);
    if (!blob) return lt_bad(fn, "blob is NULL");
    if (!al16(blob)) return lt_bad(fn, "blob is not 16-B aligned");
    if ((uint64_t)bytes != plan.bytes) return lt_bad(fn, "bytes is not what ghr_mesh_tris_sizes reports for this mesh");
    if (const char* why = ghr::mesh_tris_fill(vertices, faces, plan, blob)) return lt_bad(fn, why);
    return GHR_OK;
}

int ghr_mesh_closest(void* stream, const ghr_mesh_tris* header, const void* tris_dev, int64_t Q, const float* points,
                     const int64_t* order, const uint64_t* keys_sorted, float* dist2, int32_t* face, float* point)
{
    static const char* fn = "ghr_mesh_closest: %s";
    if (int rc = tris_header_check(fn, header, tris_dev)) return rc;
    if (Q < 0 || Q >= ((int64_t)1 << 31)) return lt_bad(fn, "Q must be in [0, 2^31)");
    if (Q == 0) return GHR_OK;
    if (!points || !order || !keys_sorted) return lt_bad(fn, "points, order or keys_sorted is NULL");
    if (!dist2 || !face || !point) return lt_bad(fn, "dist2, face or point is NULL");
    const int64_t waves = (Q + GHR_KNN_BLOCK - 1) / GHR_KNN_BLOCK;
    hipStream_t s = (hipStream_t)stream;
    ghr::MdSearchArgs a{ghr::md_view(*reinterpret_cast<const ghr::MeshTris*>(header), tris_dev), (int)Q, points, (const long long*)order,
                        (const unsigned long long*)keys_sorted, dist2, face, point};
    hipLaunchKernelGGL(ghr::k_meshdist_search, dim3((unsigned)((waves + GHR_MD_WAVES - 1) / GHR_MD_WAVES)), dim3(64 * GHR_MD_WAVES), 0, s, a);
    return finish(s, 0);
}

#ifdef GHR_MD_COUNT_BLOCKS
// measurement build only: reads {face blocks scanned, waves, faces evaluated} since the last call and zeroes them (synchronises)
int ghr_meshdist_read_counters(uint64_t* out3)
{
    unsigned long long h[3] = {0, 0, 0}, z[3] = {0, 0, 0};
    GHR_HIP(hipDeviceSynchronize());
    GHR_HIP(hipMemcpyFromSymbol(h, HIP_SYMBOL(ghr::g_md_count), sizeof(h)));
    GHR_HIP(hipMemcpyToSymbol(HIP_SYMBOL(ghr::g_md_count), z, sizeof(z)));
    out3[0] = h[0]; out3[1] = h[1]; out3[2] = h[2];
    return GHR_OK;
}
#endif

int ghr_mesh_distance_backward(void* stream, int64_t Q, const float* points, const float* closest, const float* dist2,
                               const uint8_t* inside, const float* g, float* d_points)
{
    static const char* fn = "ghr_mesh_distance_backward: %s";
    if (Q < 0 || Q >= ((int64_t)1 << 31)) return lt_bad(fn, "Q must be in [0, 2^31)");
    if (Q == 0) return GHR_OK;
    if (!points || !closest || !dist2 || !inside) return lt_bad(fn, "points, closest, dist2 or inside is NULL");
    if (!g || !d_points) return lt_bad(fn, "g or d_points is NULL");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ghr::k_meshdist_bwd, dim3((unsigned)((Q + GHR_MD_BLOCK - 1) / GHR_MD_BLOCK)), dim3(GHR_MD_BLOCK), 0, s,
                       (long long)Q, points, closest, dist2, inside, g, d_points);
    return finish(s, 0);
}

}  // extern "C"

// ---- head-mesh visibility (include/ghr.h; csrc/ghr_visibility.h) --------------------------------------------------------------
namespace {
// -- the tile lists (csrc/ghr_tilelists.h) that this raster and the two of the strand preview below are built on
inline unsigned tl_blocks(uint64_t n) { return (unsigned)((n + GHR_TL_BLOCK - 1) / GHR_TL_BLOCK); }

// the lists' share of a raster's arguments, from the layout and the workspace
ghr::TileLists tl_bind(const ghr::TileListLayout& L, char* ws, uint32_t n_points, uint32_t n_prims, const float* points, const float* M,
                       float near_w)
{
    ghr::TileLists tl{};
    tl.n_points = n_points; tl.n_prims = n_prims; tl.tiles_x = L.tiles_x; tl.tiles_y = L.tiles_y;
    tl.near = near_w;
    for (int k = 0; k < 12; k++) tl.M[k] = M[k];
    tl.points = points;
    tl.proj = reinterpret_cast<float*>(ws + L.off_proj);
    tl.rec = reinterpret_cast<float*>(ws + L.off_rec);
    tl.start = reinterpret_cast<uint32_t*>(ws + L.off_start);
    tl.count = reinterpret_cast<uint32_t*>(ws + L.off_count);
    tl.nbig = reinterpret_cast<uint32_t*>(ws + L.off_nbig);
    tl.list = reinterpret_cast<uint32_t*>(ws + L.off_list);
    tl.big = reinterpret_cast<uint32_t*>(ws + L.off_big);
    tl.list_cap = (uint32_t)L.list_cap;
    return tl;
}

// One view's lists.  The tile counts and the big list's length (and what their owner put behind them: `fill_bytes`) start every
// view at 0: one fill, so that a workspace needs no preparation by its owner and may change image size between views.  Then the
// projection, the owner's setup kernel (launch_setup), the scan and the scatter; an image without pixels has no lists to build.
template <int UNITS, class Setup>
int tl_build(hipStream_t s, const ghr::TileLists& tl, void* fill, size_t fill_bytes, Setup launch_setup)
{
    GHR_HIP(hipMemsetAsync(fill, 0, fill_bytes, s));
    if (tl.tiles_x == 0 || tl.tiles_y == 0) return GHR_OK;
    if (tl.n_prims) {
        if (tl.n_points) hipLaunchKernelGGL(ghr::k_tl_project, dim3(tl_blocks(tl.n_points)), dim3(GHR_TL_BLOCK), 0, s, tl);
        launch_setup();
    }
    hipLaunchKernelGGL(ghr::k_tl_scan, dim3(1), dim3(GHR_TL_BLOCK), 0, s, tl);
    if (tl.n_prims) hipLaunchKernelGGL((ghr::k_tl_scatter<UNITS>), dim3(tl_blocks(tl.n_prims)), dim3(GHR_TL_BLOCK), 0, s, tl);
    return GHR_OK;
}
}  // namespace

extern "C" {

int ghr_vis_sizes(int32_t V, int32_t F, int32_t H, int32_t W, size_t* bytes)
{
    static const char* fn = "ghr_vis_sizes: %s";
    if (!bytes) return lt_bad(fn, "bytes is NULL");
    ghr::VisLayout L;
    if (const char* why = ghr::vis_layout(V, F, H, W, &L)) return lt_bad(fn, why);
    *bytes = (size_t)L.bytes;
    return GHR_OK;
}

int ghr_vis_head_mask(void* stream, int32_t H, int32_t W, const uint8_t* body, const uint8_t* hair, uint8_t* head)
{
    static const char* fn = "ghr_vis_head_mask: %s";
    ghr::VisLayout L;
    if (const char* why = ghr::vis_layout(0, 0, H, W, &L)) return lt_bad(fn, why);
    if ((int64_t)H * W == 0) return GHR_OK;
    if (!body || !hair) return lt_bad(fn, "body or hair is NULL");
    if (!head) return lt_bad(fn, "head is NULL");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ghr::k_vis_head_mask, dim3((unsigned)L.tiles_x, (unsigned)L.tiles_y), dim3(GHR_VIS_BLOCK), 0, s,
                       ghr::VisHeadArgs{H, W, body, hair, head});
    return finish(s, 0);
}

int ghr_vis_view(void* stream, int32_t V, const float* vertices, int32_t F, const int32_t* faces, const float* M, float near_w,
                 int32_t H, int32_t W, const uint8_t* body, const uint8_t* hair, void* workspace, int32_t* pix_to_face,
                 uint8_t* vis, int32_t* cnt, int32_t* cnt_head)
{
    static const char* fn = "ghr_vis_view: %s";
    ghr::VisLayout L;
    if (const char* why = ghr::vis_layout(V, F, H, W, &L)) return lt_bad(fn, why);
    if (V && !vertices) return lt_bad(fn, "vertices is NULL");
    if (F && !faces) return lt_bad(fn, "faces is NULL");
    if (!M) return lt_bad(fn, "M is NULL");
    if (!(near_w >= 0.f)) return lt_bad(fn, "near is negative or NaN");
    if ((body == nullptr) != (hair == nullptr)) return lt_bad(fn, "body and hair must be given or NULL together");
    if (!workspace) return lt_bad(fn, "workspace is NULL");
    if (!al16(workspace)) return lt_bad(fn, "workspace is not 16-B aligned (the face records are read 16 B at a time)");
    if ((cnt == nullptr) != (cnt_head == nullptr)) return lt_bad(fn, "cnt and cnt_head must be given or NULL together");
    const bool pixels = (int64_t)H * W > 0;
    if (pixels && !pix_to_face) return lt_bad(fn, "pix_to_face is NULL");
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    ghr::VisArgs a{};
    a.tl = tl_bind(L, ws, (uint32_t)V, (uint32_t)F, vertices, M, near_w);
    a.V = V; a.F = F; a.H = H; a.W = W;
    a.faces = faces;
    a.seen = reinterpret_cast<uint8_t*>(ws + L.off_seen);
    a.seen_head = reinterpret_cast<uint8_t*>(ws + L.off_seen_head);
    a.pix_to_face = pix_to_face; a.vis = vis; a.cnt = cnt; a.cnt_head = cnt_head;
    // (the fill covers the vertex flags too)
    if (int rc = tl_build<GHR_VIS_REC_UNITS>(s, a.tl, ws + L.off_fill, (size_t)L.fill_bytes, [&] {
            hipLaunchKernelGGL(ghr::k_vis_setup, dim3(tl_blocks(F)), dim3(GHR_VIS_BLOCK), 0, s, a);
        }))
        return rc;
    if (pixels) {
        if (body) {
            uint8_t* head = reinterpret_cast<uint8_t*>(ws + L.off_head);
            hipLaunchKernelGGL(ghr::k_vis_head_mask, dim3((unsigned)L.tiles_x, (unsigned)L.tiles_y), dim3(GHR_VIS_BLOCK), 0, s,
                               ghr::VisHeadArgs{H, W, body, hair, head});
            a.head = head;
        }
        hipLaunchKernelGGL(ghr::k_vis_raster, dim3((unsigned)L.tiles_x, (unsigned)L.tiles_y), dim3(GHR_VIS_BLOCK), 0, s, a);
        if (V && F && cnt) hipLaunchKernelGGL(ghr::k_vis_accumulate, dim3(tl_blocks(V)), dim3(GHR_VIS_BLOCK), 0, s, a);
    }
    return finish(s, 0);
}

}  // extern "C"

// ---- the strand preview (include/ghr.h; csrc/ghr_strandview.h) ---------------------------------------------------------------
namespace {
inline unsigned sv_blocks(uint64_t n) { return (unsigned)((n + GHR_SV_BLOCK - 1) / GHR_SV_BLOCK); }
inline bool al4(const void* p) { return ((uintptr_t)p & 3u) == 0; }
static_assert(sizeof(ghr_strandview_shading) == sizeof(ghr::SvShading), "ghr_strandview_shading is ghr::SvShading");
static_assert(GHR_STRANDVIEW_KAJIYA == GHR_SV_KAJIYA && GHR_STRANDVIEW_TANGENT == GHR_SV_TANGENT, "the modes of include/ghr.h");
}  // namespace

extern "C" {

int ghr_strandview_sizes(int32_t S, int32_t L, int32_t H, int32_t W, size_t* bytes)
{
    static const char* fn = "ghr_strandview_sizes: %s";
    if (!bytes) return lt_bad(fn, "bytes is NULL");
    ghr::SvLayout Y;
    if (const char* why = ghr::sv_layout(S, L, H, W, &Y)) return lt_bad(fn, why);
    *bytes = (size_t)Y.bytes;
    return GHR_OK;
}

int ghr_strandview_face_depth(void* stream, int32_t V, const float* vertices, int32_t F, const int32_t* faces, const float* M,
                              float near_w, int32_t H, int32_t W, const int32_t* pix_to_face, float* qf)
{
    static const char* fn = "ghr_strandview_face_depth: %s";
    ghr::VisLayout L;
    if (const char* why = ghr::vis_layout(V, F, H, W, &L)) return lt_bad(fn, why);
    if (V && !vertices) return lt_bad(fn, "vertices is NULL");
    if (F && !faces) return lt_bad(fn, "faces is NULL");
    if (!M) return lt_bad(fn, "M is NULL");
    if (!(near_w >= 0.f)) return lt_bad(fn, "near is negative or NaN");
    const uint64_t N = (uint64_t)H * (uint64_t)W;
    if (N == 0) return GHR_OK;
    if (!pix_to_face) return lt_bad(fn, "pix_to_face is NULL");
    if (!qf) return lt_bad(fn, "qf is NULL");
    if (!al4(vertices) || !al4(faces) || !al4(pix_to_face) || !al4(qf)) return lt_bad(fn, "a buffer is not 4-B aligned");
    hipStream_t s = (hipStream_t)stream;
    ghr::SvFaceDepthArgs a{};
    a.V = V; a.F = F; a.H = H; a.W = W; a.near = near_w;
    for (int k = 0; k < 12; k++) a.M[k] = M[k];
    a.vertices = vertices; a.faces = faces; a.pix_to_face = pix_to_face; a.qf = qf;
    hipLaunchKernelGGL(ghr::k_sv_face_depth, dim3(sv_blocks(N)), dim3(GHR_SV_BLOCK), 0, s, a);
    return finish(s, 0);
}

int ghr_strandview_raster(void* stream, int32_t S, int32_t L, const float* points, const float* M, float near_w, int32_t H,
                          int32_t W, float half_width, float head_bias, const int32_t* pix_to_face, const float* qf,
                          void* workspace, int32_t* pix_to_segment, float* t, int32_t* pix_to_face_out, float* inv_depth)
{
    static const char* fn = "ghr_strandview_raster: %s";
    ghr::SvLayout Y;
    if (const char* why = ghr::sv_layout(S, L, H, W, &Y)) return lt_bad(fn, why);
    if (S && !points) return lt_bad(fn, "points is NULL");
    if (!M) return lt_bad(fn, "M is NULL");
    if (!(near_w >= 0.f)) return lt_bad(fn, "near is negative or NaN");
    if (!(ghr::vis_finite(half_width) && half_width > 0.f)) return lt_bad(fn, "half_width is not finite and > 0");
    if (!(ghr::vis_finite(head_bias) && head_bias >= 0.f)) return lt_bad(fn, "head_bias is negative or not finite");
    if ((pix_to_face == nullptr) != (qf == nullptr)) return lt_bad(fn, "pix_to_face and qf must be given or NULL together");
    if (!workspace) return lt_bad(fn, "workspace is NULL");
    if (!al16(workspace)) return lt_bad(fn, "workspace is not 16-B aligned (the segment records are read 16 B at a time)");
    const bool pixels = (int64_t)H * W > 0;
    if (pixels && (!pix_to_segment || !t || !pix_to_face_out || !inv_depth)) return lt_bad(fn, "an output plane is NULL");
    if (!al4(points) || !al4(pix_to_face) || !al4(qf) || !al4(pix_to_segment) || !al4(t) || !al4(pix_to_face_out) || !al4(inv_depth))
        return lt_bad(fn, "a buffer is not 4-B aligned");
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    ghr::SvArgs a{};
    a.tl = tl_bind(Y, ws, (uint32_t)Y.n_points, (uint32_t)Y.n_segments, points, M, near_w);
    a.L = L; a.H = H; a.W = W;
    a.r = half_width; a.head_bias = head_bias;
    a.pix_to_face = pix_to_face; a.qf = qf;
    a.pix_to_segment = pix_to_segment; a.t = t; a.pix_to_face_out = pix_to_face_out; a.inv_depth = inv_depth;
    if (!pixels) return GHR_OK;
    if (int rc = tl_build<GHR_SV_REC_UNITS>(s, a.tl, ws + Y.off_fill, (size_t)Y.fill_bytes, [&] {
            hipLaunchKernelGGL(ghr::k_sv_setup, dim3(tl_blocks(Y.n_segments)), dim3(GHR_SV_BLOCK), 0, s, a);
        }))
        return rc;
    hipLaunchKernelGGL(ghr::k_sv_raster, dim3((unsigned)Y.tiles_x, (unsigned)Y.tiles_y), dim3(GHR_SV_BLOCK), 0, s, a);
    return finish(s, 0);
}

int ghr_strandview_shade(void* stream, int32_t S, int32_t L, const float* points, int32_t V, const float* vertices, int32_t F,
                         const int32_t* faces, int32_t H, int32_t W, const int32_t* pix_to_segment, const int32_t* pix_to_face_out,
                         int32_t mode, const ghr_strandview_shading* shading, const float* base, uint8_t* rgb)
{
    static const char* fn = "ghr_strandview_shade: %s";
    ghr::SvLayout Y;
    if (const char* why = ghr::sv_layout(S, L, H, W, &Y)) return lt_bad(fn, why);
    ghr::VisLayout VL;
    if (const char* why = ghr::vis_layout(V, F, H, W, &VL)) return lt_bad(fn, why);
    if (mode != GHR_SV_KAJIYA && mode != GHR_SV_TANGENT) return lt_bad(fn, "mode is neither GHR_STRANDVIEW_KAJIYA nor GHR_STRANDVIEW_TANGENT");
    if (!shading) return lt_bad(fn, "shading is NULL");
    if (shading->shininess_log2 < 0 || shading->shininess_log2 > GHR_SV_MAX_SHININESS_LOG2) return lt_bad(fn, "shininess_log2 is outside 0 .. 16");
    if (S && !points) return lt_bad(fn, "points is NULL");
    if (V && !vertices) return lt_bad(fn, "vertices is NULL");
    if (F && !faces) return lt_bad(fn, "faces is NULL");
    const uint64_t N = (uint64_t)H * (uint64_t)W;
    if (N == 0) return GHR_OK;
    if (!pix_to_segment || !pix_to_face_out) return lt_bad(fn, "pix_to_segment or pix_to_face_out is NULL");
    if (!rgb) return lt_bad(fn, "rgb is NULL");
    if (!al4(points) || !al4(vertices) || !al4(faces) || !al4(pix_to_segment) || !al4(pix_to_face_out) || !al4(base))
        return lt_bad(fn, "a buffer is not 4-B aligned");
    hipStream_t s = (hipStream_t)stream;
    ghr::SvShadeArgs a{};
    a.S = S; a.L = L; a.V = V; a.F = F; a.H = H; a.W = W; a.mode = mode;
    memcpy(&a.sh, shading, sizeof(a.sh));
    a.points = points; a.vertices = vertices; a.faces = faces; a.base = base;
    a.pix_to_segment = pix_to_segment; a.pix_to_face_out = pix_to_face_out; a.rgb = rgb;
    hipLaunchKernelGGL(ghr::k_sv_shade, dim3(sv_blocks(N)), dim3(GHR_SV_BLOCK), 0, s, a);
    return finish(s, 0);
}

int ghr_strandview_resolve(void* stream, int32_t H, int32_t W, int32_t supersample, const uint8_t* src, uint8_t* dst)
{
    static const char* fn = "ghr_strandview_resolve: %s";
    if (supersample != 1 && supersample != 2 && supersample != 4) return lt_bad(fn, "supersample is not 1, 2 or 4");
    if (H < 0 || W < 0) return lt_bad(fn, "negative size");
    if ((uint64_t)H * supersample * (uint64_t)W * supersample > 0x7fffffffull) return lt_bad(fn, "H * W exceeds 32-bit offsets");
    const uint64_t N = (uint64_t)H * (uint64_t)W;
    if (N == 0) return GHR_OK;
    if (!src) return lt_bad(fn, "src is NULL");
    if (!dst) return lt_bad(fn, "dst is NULL");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ghr::k_sv_resolve, dim3(sv_blocks(N)), dim3(GHR_SV_BLOCK), 0, s, ghr::SvResolveArgs{H, W, supersample, src, dst});
    return finish(s, 0);
}

// -- self-shadowing: the light pass and the shadowed shade
static_assert(sizeof(ghr_strandview_shadow) == sizeof(ghr::SvShadow), "ghr_strandview_shadow is ghr::SvShadow");

int ghr_strandview_opacity(void* stream, int32_t S, int32_t L, const float* points, const float* Ml, float near_w, int32_t Hl,
                           int32_t Wl, float half_width, float layer, void* workspace, size_t workspace_bytes, float* q0,
                           uint32_t* layers)
{
    static const char* fn = "ghr_strandview_opacity: %s";
    ghr::SvLayout Y;
    if (const char* why = ghr::sv_layout(S, L, Hl, Wl, &Y)) return lt_bad(fn, why);
    if (S && !points) return lt_bad(fn, "points is NULL");
    if (!Ml) return lt_bad(fn, "Ml is NULL");
    if (!(near_w >= 0.f)) return lt_bad(fn, "near is negative or NaN");
    if (!(ghr::vis_finite(half_width) && half_width > 0.f)) return lt_bad(fn, "half_width is not finite and > 0");
    if (!(ghr::vis_finite(layer) && layer > 0.f)) return lt_bad(fn, "layer is not finite and > 0");
    if (!workspace) return lt_bad(fn, "workspace is NULL");
    if (!al16(workspace)) return lt_bad(fn, "workspace is not 16-B aligned (the segment records are read 16 B at a time)");
    if ((uint64_t)workspace_bytes < Y.bytes) return lt_bad(fn, "workspace is too small: ghr_strandview_sizes(S, L, Hl, Wl) sizes it");
    const bool texels = (int64_t)Hl * Wl > 0;
    if (texels && (!q0 || !layers)) return lt_bad(fn, "an output plane is NULL");
    if (!al4(points) || !al4(q0)) return lt_bad(fn, "a buffer is not 4-B aligned");
    if (!al16(layers)) return lt_bad(fn, "layers is not 16-B aligned (a texel's four counts are one store)");
    if (!texels) return GHR_OK;
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    ghr::SvLayersArgs la{};
    ghr::SvArgs& a = la.a;
    a.tl = tl_bind(Y, ws, (uint32_t)Y.n_points, (uint32_t)Y.n_segments, points, Ml, near_w);
    a.L = L; a.H = Hl; a.W = Wl;
    a.r = half_width;
    la.layer = layer; la.q0 = q0; la.layers = layers;
    if (int rc = tl_build<GHR_SV_REC_UNITS>(s, a.tl, ws + Y.off_fill, (size_t)Y.fill_bytes, [&] {
            hipLaunchKernelGGL(ghr::k_sv_setup, dim3(tl_blocks(Y.n_segments)), dim3(GHR_SV_BLOCK), 0, s, a);
        }))
        return rc;
    hipLaunchKernelGGL(ghr::k_sv_layers, dim3((unsigned)Y.tiles_x, (unsigned)Y.tiles_y), dim3(GHR_SV_BLOCK), 0, s, la);
    return finish(s, 0);
}

int ghr_strandview_shade_shadowed(void* stream, int32_t S, int32_t L, const float* points, int32_t V, const float* vertices, int32_t F,
                                  const int32_t* faces, int32_t H, int32_t W, const int32_t* pix_to_segment,
                                  const int32_t* pix_to_face_out, const float* t, int32_t mode, const ghr_strandview_shading* shading,
                                  const float* base, const ghr_strandview_shadow* shadow, uint8_t* rgb)
{
    static const char* fn = "ghr_strandview_shade_shadowed: %s";
    ghr::SvLayout Y;
    if (const char* why = ghr::sv_layout(S, L, H, W, &Y)) return lt_bad(fn, why);
    ghr::VisLayout VL;
    if (const char* why = ghr::vis_layout(V, F, H, W, &VL)) return lt_bad(fn, why);
    if (mode != GHR_SV_KAJIYA && mode != GHR_SV_TANGENT) return lt_bad(fn, "mode is neither GHR_STRANDVIEW_KAJIYA nor GHR_STRANDVIEW_TANGENT");
    if (!shading) return lt_bad(fn, "shading is NULL");
    if (shading->shininess_log2 < 0 || shading->shininess_log2 > GHR_SV_MAX_SHININESS_LOG2) return lt_bad(fn, "shininess_log2 is outside 0 .. 16");
    if (!shadow) return lt_bad(fn, "shadow is NULL");
    if (shadow->Hl < 0 || shadow->Wl < 0) return lt_bad(fn, "negative size of the light map");
    if ((uint64_t)shadow->Hl * (uint64_t)shadow->Wl > 0x7fffffffull) return lt_bad(fn, "Hl * Wl exceeds 32-bit offsets");
    if (!(shadow->near_w >= 0.f)) return lt_bad(fn, "near of the light view is negative or NaN");
    if (!(ghr::vis_finite(shadow->layer) && shadow->layer > 0.f)) return lt_bad(fn, "layer is not finite and > 0");
    if (!(ghr::vis_finite(shadow->kappa) && shadow->kappa >= 0.f)) return lt_bad(fn, "kappa is negative or not finite");
    if (!(ghr::vis_finite(shadow->bias) && shadow->bias >= 0.f)) return lt_bad(fn, "shadow bias is negative or not finite");
    const bool texels = (int64_t)shadow->Hl * shadow->Wl > 0;
    if (texels && (!shadow->q0 || !shadow->layers)) return lt_bad(fn, "q0 or layers of the light map is NULL");
    if (!al4(shadow->q0) || !al4(shadow->qfl)) return lt_bad(fn, "a buffer is not 4-B aligned");
    if (!al16(shadow->layers)) return lt_bad(fn, "layers is not 16-B aligned");
    if (S && !points) return lt_bad(fn, "points is NULL");
    if (V && !vertices) return lt_bad(fn, "vertices is NULL");
    if (F && !faces) return lt_bad(fn, "faces is NULL");
    const uint64_t N = (uint64_t)H * (uint64_t)W;
    if (N == 0) return GHR_OK;
    if (!pix_to_segment || !pix_to_face_out) return lt_bad(fn, "pix_to_segment or pix_to_face_out is NULL");
    if (!t) return lt_bad(fn, "t is NULL");
    if (!rgb) return lt_bad(fn, "rgb is NULL");
    if (!al4(points) || !al4(vertices) || !al4(faces) || !al4(pix_to_segment) || !al4(pix_to_face_out) || !al4(t) || !al4(base))
        return lt_bad(fn, "a buffer is not 4-B aligned");
    hipStream_t s = (hipStream_t)stream;
    ghr::SvShadeShadowedArgs sa{};
    ghr::SvShadeArgs& a = sa.a;
    a.S = S; a.L = L; a.V = V; a.F = F; a.H = H; a.W = W; a.mode = mode;
    memcpy(&a.sh, shading, sizeof(a.sh));
    a.points = points; a.vertices = vertices; a.faces = faces; a.base = base;
    a.pix_to_segment = pix_to_segment; a.pix_to_face_out = pix_to_face_out; a.rgb = rgb;
    sa.t = t;
    memcpy(&sa.sd, shadow, sizeof(sa.sd));
    hipLaunchKernelGGL(ghr::k_sv_shade_shadowed, dim3(sv_blocks(N)), dim3(GHR_SV_BLOCK), 0, s, sa);
    return finish(s, 0);
}

// -- synthetic captures: the masks and the orientation map of a view from its supersampled raster
int ghr_strandview_capture(void* stream, int32_t S, int32_t L, const float* points, const float* M, float near_w, int32_t H,
                           int32_t W, int32_t supersample, int32_t F, const int32_t* pix_to_segment, const int32_t* pix_to_face_out,
                           const float* table, float var_floor, uint8_t* mask_hair, uint8_t* mask_body, uint8_t* angle, float* var)
{
    static const char* fn = "ghr_strandview_capture: %s";
    if (S < 0 || H < 0 || W < 0 || F < 0) return lt_bad(fn, "negative size");
    if (L < 2) return lt_bad(fn, "L < 2: a strand needs two points");
    if (S > 0 && L > (0x7fffffffll / 3) / S) return lt_bad(fn, "S * L * 3 exceeds 32-bit offsets");
    if (supersample != 1 && supersample != 2 && supersample != 4) return lt_bad(fn, "supersample is not 1, 2 or 4");
    if ((uint64_t)H * supersample * (uint64_t)W * supersample > 0x7fffffffull) return lt_bad(fn, "H * W exceeds 32-bit offsets");
    if (!(ghr::vis_finite(var_floor) && var_floor >= 0.f)) return lt_bad(fn, "var_floor is negative or not finite");
    if (!(near_w >= 0.f)) return lt_bad(fn, "near is negative or NaN");
    if (S && !points) return lt_bad(fn, "points is NULL");
    if (!M) return lt_bad(fn, "M is NULL");
    if (!table) return lt_bad(fn, "table is NULL");
    const uint64_t N = (uint64_t)H * (uint64_t)W;
    if (N && (!pix_to_segment || !pix_to_face_out)) return lt_bad(fn, "pix_to_segment or pix_to_face_out is NULL");
    if (N && (!mask_hair || !mask_body || !angle || !var)) return lt_bad(fn, "an output plane is NULL");
    if (!al4(points) || !al4(pix_to_segment) || !al4(pix_to_face_out) || !al4(table) || !al4(var))
        return lt_bad(fn, "a buffer is not 4-B aligned");
    if (N == 0) return GHR_OK;
    hipStream_t s = (hipStream_t)stream;
    ghr::CapArgs a{};
    a.S = S; a.L = L; a.H = H; a.W = W; a.F = F;
    a.near = near_w; a.var_floor = var_floor;
    for (int k = 0; k < 12; k++) a.Ms[k] = M[k];
    a.out_dword = al4(mask_hair) && al4(mask_body) && al4(angle);
    a.out_f4 = al16(var);
    a.points = points; a.pix_to_segment = pix_to_segment; a.pix_to_face_out = pix_to_face_out; a.table = table;
    a.mask_hair = mask_hair; a.mask_body = mask_body; a.angle = angle; a.var = var;
    // a row of a pixel's subsamples is one load when both planes are aligned to it (a plane's rows are 4 s W bytes apart)
    const uintptr_t both = (uintptr_t)pix_to_segment | (uintptr_t)pix_to_face_out;
    const bool vec = (both & (uintptr_t)(4 * supersample - 1)) == 0;
    const dim3 grid(sv_blocks((N + GHR_CAP_QUAD - 1) / GHR_CAP_QUAD)), block(GHR_CAP_BLOCK);
    if (supersample == 4) {
        if (vec) hipLaunchKernelGGL((ghr::k_sv_capture<4, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((ghr::k_sv_capture<4, false>), grid, block, 0, s, a);
    } else if (supersample == 2) {
        if (vec) hipLaunchKernelGGL((ghr::k_sv_capture<2, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((ghr::k_sv_capture<2, false>), grid, block, 0, s, a);
    } else {
        hipLaunchKernelGGL((ghr::k_sv_capture<1, false>), grid, block, 0, s, a);
    }
    return finish(s, 0);
}

}  // extern "C"

// ---- the strand stage's prior term: guiding strands' local frames and the latent texture (include/ghr.h; csrc/ghr_sds.h) ------
namespace {
// one wave per item, here and for the guiding strands of the generator below (both launch csrc/ghr_haar.h's kernels)
inline unsigned sds_blocks(int64_t waves) { return (unsigned)((waves + GHR_SDS_BLOCK / GHR_SDS_WAVE - 1) / (GHR_SDS_BLOCK / GHR_SDS_WAVE)); }

// the sizes every entry shares, before anything touches the runtime; S < 0: not checked (the texture has no S)
const char* sds_sizes(int64_t S, int64_t N, int64_t n, int64_t C, int64_t G)
{
    if (N < GHR_SDS_K) return "N < 4: a texel needs four guiding strands";
    if (n < 1) return "n < 1";
    if (S == 0) return "S < 1";
    if (C < 1) return "C < 1";
    if (G >= 0 && G * G < N) return "G * G < N: guiding strand g takes its coefficient from texel g";
    if (G > 16384 || N > (1 << 24) || N * (n + 1) * 3 >= (1ll << 31) || N * C >= (1ll << 31) || (G >= 0 && C * G * G >= (1ll << 31)) ||
        (S > 0 && S * n * 3 >= (1ll << 40)))
        return "sizes exceed the kernels' 32-bit indexing";
    return nullptr;
}
}  // namespace

extern "C" {

int ghr_sds_local(void* stream, int32_t S, int32_t N, int32_t n, const float* dirs, const float* frames, int32_t frames_are_inverse,
                  const int64_t* idx, float scale, float* e, float* v)
{
    static const char* fn = "ghr_sds_local: %s";
    if (S < 0) return lt_bad(fn, "S is negative");
    if (const char* why = sds_sizes(S, N, n, 1, -1)) return lt_bad(fn, why);
    if (!dirs || !frames || !idx) return lt_bad(fn, "dirs, frames or idx is NULL");
    if (!e || !v) return lt_bad(fn, "e or v is NULL");
    hipStream_t s = (hipStream_t)stream;
    ghr::SdsLocalArgs a{};
    a.S = S; a.N = N; a.n = n; a.frames_are_inverse = frames_are_inverse; a.scale = scale;
    a.dirs = dirs; a.frames = frames; a.idx = idx; a.e = e; a.v = v;
    hipLaunchKernelGGL(ghr::k_sds_local, dim3(sds_blocks(N)), dim3(GHR_SDS_BLOCK), 0, s, a);
    return finish(s, 0);
}

int ghr_sds_local_backward(void* stream, int32_t S, int32_t N, int32_t n, const float* frames, int32_t frames_are_inverse,
                           const int64_t* sorted_idx, const int64_t* order, float scale, const float* d_e, const float* d_v,
                           float* d_dirs)
{
    static const char* fn = "ghr_sds_local_backward: %s";
    if (S < 0) return lt_bad(fn, "S is negative");
    if (const char* why = sds_sizes(S, N, n, 1, -1)) return lt_bad(fn, why);
    if (!frames || !sorted_idx || !order) return lt_bad(fn, "frames, sorted_idx or order is NULL");
    if (!d_dirs) return lt_bad(fn, "d_dirs is NULL");
    if (!d_e && !d_v) return GHR_OK;  // nothing arrives: the zero-filled d_dirs is the answer
    hipStream_t s = (hipStream_t)stream;
    ghr::SdsLocalArgs a{};
    a.S = S; a.N = N; a.n = n; a.frames_are_inverse = frames_are_inverse; a.scale = scale;
    a.frames = frames; a.idx = sorted_idx; a.order = order; a.d_e = d_e; a.d_v = d_v; a.d_dirs = d_dirs;
    hipLaunchKernelGGL(ghr::k_sds_local_bwd, dim3(sds_blocks(N)), dim3(GHR_SDS_BLOCK), 0, s, a);
    return finish(s, 0);
}

int ghr_sds_texture(void* stream, int32_t N, int32_t n, int32_t C, int32_t G, const float* uvg, const float* centres, const float* z,
                    const float* v, int32_t* nbr, float* w, float* csim, float* alpha, float* alpha_q, int32_t* count,
                    int32_t* start, int32_t* list, float* texture)
{
    static const char* fn = "ghr_sds_texture: %s";
    if (G < 0) return lt_bad(fn, "G is negative");
    if (const char* why = sds_sizes(-1, N, n, C, G)) return lt_bad(fn, why);
    if (!uvg || !centres || !z || !v) return lt_bad(fn, "uvg, centres, z or v is NULL");
    if (!nbr || !w || !csim || !alpha || !alpha_q || !count || !start || !list) return lt_bad(fn, "a saved-state buffer is NULL");
    if (!texture) return lt_bad(fn, "texture is NULL");
    hipStream_t s = (hipStream_t)stream;
    ghr::HaarArgs a{};
    a.Q = G * G; a.N = N; a.n = n; a.C = C; a.G = G; a.uvg = uvg; a.centres = centres; a.z = z; a.v = v;
    a.nbr = nbr; a.w = w; a.csim = csim; a.alpha = alpha; a.alpha_q = alpha_q; a.count = count; a.start = start; a.list = list;
    a.out = texture;
    GHR_HIP(hipMemsetAsync(count, 0, sizeof(int32_t) * (size_t)N, s));
    hipLaunchKernelGGL(ghr::k_haar_knn<ghr::HaarTexels>, dim3(sds_blocks(a.Q)), dim3(GHR_SDS_BLOCK), 0, s, a);
    hipLaunchKernelGGL(ghr::k_sds_lists, dim3(sds_blocks(N)), dim3(GHR_SDS_BLOCK), 0, s, a);
    hipLaunchKernelGGL(ghr::k_haar_blend<ghr::HaarTexels>, dim3(sds_blocks(a.Q)), dim3(GHR_SDS_BLOCK), 0, s, a);
    return finish(s, 0);
}

int ghr_sds_texture_backward(void* stream, int32_t N, int32_t n, int32_t C, int32_t G, const float* z, const float* v,
                             const int32_t* nbr, const float* w, const float* csim, const float* alpha_q, const int32_t* start,
                             const int32_t* list, const float* d_texture, float* dalpha_q, float* d_csim, float* d_z, float* d_v)
{
    static const char* fn = "ghr_sds_texture_backward: %s";
    if (G < 0) return lt_bad(fn, "G is negative");
    if (const char* why = sds_sizes(-1, N, n, C, G)) return lt_bad(fn, why);
    if (!z || !v) return lt_bad(fn, "z or v is NULL");
    if (!nbr || !w || !csim || !alpha_q || !start || !list) return lt_bad(fn, "a saved-state buffer is NULL");
    if (!d_texture) return lt_bad(fn, "d_texture is NULL");
    if (!dalpha_q || !d_csim) return lt_bad(fn, "dalpha_q or d_csim is NULL");
    if (!d_z) return lt_bad(fn, "d_z is NULL");
    hipStream_t s = (hipStream_t)stream;
    ghr::HaarArgs a{};
    a.Q = G * G; a.N = N; a.n = n; a.C = C; a.G = G; a.z = z; a.v = v;
    a.nbr = const_cast<int32_t*>(nbr); a.w = const_cast<float*>(w); a.csim = const_cast<float*>(csim);
    a.alpha_q = const_cast<float*>(alpha_q); a.start = const_cast<int32_t*>(start); a.list = const_cast<int32_t*>(list);
    a.d_out = d_texture; a.dalpha_q = dalpha_q; a.d_csim = d_csim; a.d_z = d_z; a.d_v = d_v;
    hipLaunchKernelGGL(ghr::k_haar_dalpha<ghr::HaarTexels>, dim3(sds_blocks(a.Q)), dim3(GHR_SDS_BLOCK), 0, s, a);
    hipLaunchKernelGGL(ghr::k_haar_gather<ghr::HaarTexels>, dim3(sds_blocks(N)), dim3(GHR_SDS_BLOCK), 0, s, a);
    if (d_v) hipLaunchKernelGGL(ghr::k_haar_bwd_v<ghr::HaarTexels>, dim3(sds_blocks(N)), dim3(GHR_SDS_BLOCK), 0, s, a);
    return finish(s, 0);
}

}  // extern "C"

// ---- the textured strand generator between its networks: texture fetch, local frames (include/ghr.h; csrc/ghr_texstrands.h) ----
namespace {
inline unsigned ts_blocks(int64_t waves) { return (unsigned)((waves + GHR_TS_BLOCK / GHR_TS_WAVE - 1) / (GHR_TS_BLOCK / GHR_TS_WAVE)); }

// the sizes every entry shares, before anything touches the runtime; a size of -1 is not checked by that entry
const char* ts_sizes(int64_t Smax, int64_t S, int64_t T, int64_t C, int64_t n)
{
    if (S < 1) return "S < 1";
    if (S > Smax) return "S > Smax";
    if (T != -1 && T < 1) return "T < 1";
    if (C != -1 && C < 1) return "C < 1";
    if (n != -1 && n < 1) return "n < 1";
    if (Smax > (1 << 28) || T > 16384 || (T > 0 && C * T * T >= (1ll << 31)) || (C > 0 && S * C >= (1ll << 31)) ||
        (n > 0 && S * (n + 1) * 3 >= (1ll << 31)))
        return "sizes exceed the kernels' 32-bit indexing";
    return nullptr;
}
}  // namespace

extern "C" {

int ghr_ts_fetch(void* stream, int32_t Smax, int32_t S, int32_t T, int32_t C, const float* texture, const int32_t* x0,
                 const int32_t* y0, const float* fx, const float* fy, const int64_t* idx, float* z)
{
    static const char* fn = "ghr_ts_fetch: %s";
    if (const char* why = ts_sizes(Smax, S, T, C, -1)) return lt_bad(fn, why);
    if (!texture) return lt_bad(fn, "texture is NULL");
    if (!x0 || !y0 || !fx || !fy) return lt_bad(fn, "a tap buffer is NULL");
    if (!idx) return lt_bad(fn, "idx is NULL");
    if (!z) return lt_bad(fn, "z is NULL");
    hipStream_t s = (hipStream_t)stream;
    ghr::TsFetchArgs a{};
    a.Smax = Smax; a.S = S; a.T = T; a.C = C; a.texture = texture; a.x0 = x0; a.y0 = y0; a.fx = fx; a.fy = fy; a.idx = idx; a.z = z;
    hipLaunchKernelGGL(ghr::k_ts_fetch, dim3(ts_blocks(S)), dim3(GHR_TS_BLOCK), 0, s, a);
    return finish(s, 0);
}

int ghr_ts_fetch_backward(void* stream, int32_t Smax, int32_t S, int32_t T, int32_t C, const float* fx, const float* fy,
                          const int32_t* start, const int32_t* list, int32_t list_len, const int64_t* idx, const float* d_z,
                          int32_t* pos, float* d_texture)
{
    static const char* fn = "ghr_ts_fetch_backward: %s";
    if (const char* why = ts_sizes(Smax, S, T, C, -1)) return lt_bad(fn, why);
    if (list_len < 0 || (int64_t)list_len > 4ll * Smax) return lt_bad(fn, "list_len outside 0 .. 4 Smax");
    if (!fx || !fy) return lt_bad(fn, "a tap buffer is NULL");
    if (!start || (!list && list_len > 0)) return lt_bad(fn, "start or list is NULL");
    if (!idx) return lt_bad(fn, "idx is NULL");
    if (!d_z) return lt_bad(fn, "d_z is NULL");
    if (!pos) return lt_bad(fn, "pos is NULL");
    if (!d_texture) return lt_bad(fn, "d_texture is NULL");
    hipStream_t s = (hipStream_t)stream;
    ghr::TsFetchArgs a{};
    a.Smax = Smax; a.S = S; a.T = T; a.C = C; a.list_len = list_len; a.fx = fx; a.fy = fy; a.start = start; a.list = list;
    a.idx = idx; a.d_z = d_z; a.pos = pos; a.d_texture = d_texture;
    const int64_t TT = (int64_t)T * T;
    GHR_HIP(hipMemsetAsync(pos, 0xff, sizeof(int32_t) * (size_t)Smax, s));  // -1: not in this draw
    hipLaunchKernelGGL(ghr::k_ts_positions, dim3((unsigned)((S + GHR_TS_BLOCK - 1) / GHR_TS_BLOCK)), dim3(GHR_TS_BLOCK), 0, s, a);
    hipLaunchKernelGGL(ghr::k_ts_texgrad, dim3((unsigned)((TT + GHR_TS_TEXELS - 1) / GHR_TS_TEXELS)), dim3(GHR_TS_GRAD_BLOCK), 0, s, a);
    return finish(s, 0);
}

int ghr_ts_world(void* stream, int32_t Smax, int32_t S, int32_t n, const float* v, const float* local2world, const float* origins,
                 const int64_t* idx, float inv_scale, float* p, float* p_local)
{
    static const char* fn = "ghr_ts_world: %s";
    if (const char* why = ts_sizes(Smax, S, -1, -1, n)) return lt_bad(fn, why);
    if (!v) return lt_bad(fn, "v is NULL");
    if (!local2world || !origins) return lt_bad(fn, "local2world or origins is NULL");
    if (!idx) return lt_bad(fn, "idx is NULL");
    if (!p) return lt_bad(fn, "p is NULL");
    hipStream_t s = (hipStream_t)stream;
    ghr::TsWorldArgs a{};
    a.Smax = Smax; a.S = S; a.n = n; a.inv_scale = inv_scale; a.v = v; a.frames = local2world; a.origins = origins; a.idx = idx;
    a.p = p; a.p_local = p_local;
    hipLaunchKernelGGL(ghr::k_ts_world, dim3(ts_blocks(S)), dim3(GHR_TS_BLOCK), 0, s, a);
    return finish(s, 0);
}

int ghr_ts_world_backward(void* stream, int32_t Smax, int32_t S, int32_t n, const float* local2world, const int64_t* idx,
                          float inv_scale, const float* d_p, const float* d_p_local, float* d_v)
{
    static const char* fn = "ghr_ts_world_backward: %s";
    if (const char* why = ts_sizes(Smax, S, -1, -1, n)) return lt_bad(fn, why);
    if (!local2world) return lt_bad(fn, "local2world is NULL");
    if (!idx) return lt_bad(fn, "idx is NULL");
    if (!d_p && !d_p_local) return lt_bad(fn, "d_p and d_p_local are both NULL");
    if (!d_v) return lt_bad(fn, "d_v is NULL");
    hipStream_t s = (hipStream_t)stream;
    ghr::TsWorldArgs a{};
    a.Smax = Smax; a.S = S; a.n = n; a.inv_scale = inv_scale; a.frames = local2world; a.idx = idx; a.d_p = d_p; a.d_pl = d_p_local;
    a.d_v = d_v;
    hipLaunchKernelGGL(ghr::k_ts_world_bwd, dim3(ts_blocks(S)), dim3(GHR_TS_BLOCK), 0, s, a);
    return finish(s, 0);
}

}  // extern "C"

// ---- guiding strands of the textured generator: neighbours, lists, the HAAR blend (include/ghr.h; csrc/ghr_guides.h) ----------
namespace {
// the sizes both entries share, before anything touches the runtime
const char* gd_sizes(int64_t S, int64_t N, int64_t n, int64_t C)
{
    if (N < GHR_SDS_K) return "N < 4: a strand needs four guides";
    if (S < N) return "S < N: the guides are the first N of the S drawn roots";
    if (n < 1) return "n < 1";
    if (C < 1) return "C < 1";
    if (S > (1 << 28) || S * C >= (1ll << 31) || N * n * 3 >= (1ll << 31)) return "sizes exceed the kernels' 32-bit indexing";
    return nullptr;
}
}  // namespace

extern "C" {

int ghr_guides_blend(void* stream, int32_t S, int32_t N, int32_t n, int32_t C, const float* uvs, const float* z_g, const float* v_g,
                     int32_t* nbr, float* w, float* csim, float* alpha, float* alpha_s, int32_t* count, int32_t* start,
                     int32_t* unsorted, int32_t* list, float* z)
{
    static const char* fn = "ghr_guides_blend: %s";
    if (const char* why = gd_sizes(S, N, n, C)) return lt_bad(fn, why);
    if (!uvs || !z_g || !v_g) return lt_bad(fn, "uvs, z_g or v_g is NULL");
    if (!nbr || !w || !csim || !alpha || !alpha_s || !count || !start || !unsorted || !list) return lt_bad(fn, "a saved-state buffer is NULL");
    if (!z) return lt_bad(fn, "z is NULL");
    hipStream_t s = (hipStream_t)stream;
    ghr::HaarArgs a{};
    a.Q = S; a.N = N; a.n = n; a.C = C; a.uvg = uvs; a.z = z_g; a.v = v_g;
    a.nbr = nbr; a.w = w; a.csim = csim; a.alpha = alpha; a.alpha_q = alpha_s; a.count = count; a.start = start;
    a.unsorted = unsorted; a.list = list; a.out = z;
    GHR_HIP(hipMemsetAsync(count, 0, sizeof(int32_t) * (size_t)N, s));
    hipLaunchKernelGGL(ghr::k_haar_knn<ghr::HaarRoots>, dim3(sds_blocks(S)), dim3(GHR_SDS_BLOCK), 0, s, a);
    hipLaunchKernelGGL(ghr::k_haar_blend<ghr::HaarRoots>, dim3(sds_blocks(S)), dim3(GHR_SDS_BLOCK), 0, s, a);
    hipLaunchKernelGGL(ghr::k_gd_start, dim3(1), dim3(GHR_SDS_WAVE), 0, s, a);
    hipLaunchKernelGGL(ghr::k_gd_fill, dim3((unsigned)((4ll * S + GHR_SDS_BLOCK - 1) / GHR_SDS_BLOCK)), dim3(GHR_SDS_BLOCK), 0, s, a);
    hipLaunchKernelGGL(ghr::k_gd_lists, dim3(sds_blocks(N)), dim3(GHR_SDS_BLOCK), 0, s, a);
    return finish(s, 0);
}

int ghr_guides_blend_backward(void* stream, int32_t S, int32_t N, int32_t n, int32_t C, const float* z_g, const float* v_g,
                              const int32_t* nbr, const float* w, const float* csim, const float* alpha_s, const int32_t* start,
                              const int32_t* list, const float* d_z, float* dalpha_s, float* d_csim, float* d_zg, float* d_vg)
{
    static const char* fn = "ghr_guides_blend_backward: %s";
    if (const char* why = gd_sizes(S, N, n, C)) return lt_bad(fn, why);
    if (!z_g || !v_g) return lt_bad(fn, "z_g or v_g is NULL");
    if (!nbr || !w || !csim || !alpha_s || !start || !list) return lt_bad(fn, "a saved-state buffer is NULL");
    if (!d_z) return lt_bad(fn, "d_z is NULL");
    if (!dalpha_s || !d_csim) return lt_bad(fn, "dalpha_s or d_csim is NULL");
    if (!d_zg) return lt_bad(fn, "d_zg is NULL");
    hipStream_t s = (hipStream_t)stream;
    ghr::HaarArgs a{};
    a.Q = S; a.N = N; a.n = n; a.C = C; a.z = z_g; a.v = v_g;
    a.nbr = const_cast<int32_t*>(nbr); a.w = const_cast<float*>(w); a.csim = const_cast<float*>(csim);
    a.alpha_q = const_cast<float*>(alpha_s); a.start = const_cast<int32_t*>(start); a.list = const_cast<int32_t*>(list);
    a.d_out = d_z; a.dalpha_q = dalpha_s; a.d_csim = d_csim; a.d_z = d_zg; a.d_v = d_vg;
    hipLaunchKernelGGL(ghr::k_haar_dalpha<ghr::HaarRoots>, dim3(sds_blocks(S)), dim3(GHR_SDS_BLOCK), 0, s, a);
    hipLaunchKernelGGL(ghr::k_haar_gather<ghr::HaarRoots>, dim3(sds_blocks(N)), dim3(GHR_SDS_BLOCK), 0, s, a);
    if (d_vg) hipLaunchKernelGGL(ghr::k_haar_bwd_v<ghr::HaarRoots>, dim3(sds_blocks(N)), dim3(GHR_SDS_BLOCK), 0, s, a);
    return finish(s, 0);
}

// ---- the hair field, strands traced through it, their resampling (ghr_field.h) ---------------------------------------------------
static const int64_t FIELD_2_31 = (int64_t)1 << 31;

static const char* field_cloud_bad(int64_t P)
{
    if (P < 1) return "P < 1: the field needs a point";
    if (P >= FIELD_2_31) return "sizes exceed the kernels' 32-bit indexing";
    return nullptr;
}

static const char* field_radius_bad(float r2)
{
    return (r2 > 0.f && r2 <= FLT_MAX) ? nullptr : "r2 must be positive and finite";
}

struct FieldWs { ghr::KnnCloud cloud; ghr::FieldPayload pay; };
static FieldWs field_carve(const void* ws, int64_t P)
{
    char* base = align_base(ws);
    return FieldWs{ghr::knn_cloud(base, (uint64_t)P), ghr::field_payload(base + ghr::knn_layout((uint64_t)P).bytes, (uint64_t)P)};
}

int ghr_field_workspace_size(int64_t P, size_t* bytes)
{
    static const char* fn = "ghr_field_workspace_size: %s";
    if (const char* why = field_cloud_bad(P)) return lt_bad(fn, why);
    if (!bytes) return lt_bad(fn, "bytes is NULL");
    *bytes = ghr::knn_layout((uint64_t)P).bytes + ghr::field_payload_bytes((uint64_t)P) + ALIGN;
    return GHR_OK;
}

int ghr_field_build(void* stream, int64_t P, const float* points, const int64_t* order, const float* directions, const float* weights,
                    const float* colors, void* ws)
{
    static const char* fn = "ghr_field_build: %s";
    if (const char* why = field_cloud_bad(P)) return lt_bad(fn, why);
    if (!points || !order) return lt_bad(fn, "points or order is NULL");
    if (!directions || !weights || !colors) return lt_bad(fn, "directions, weights or colors is NULL");
    if (!ws) return lt_bad(fn, "ws is NULL");
    const FieldWs w = field_carve(ws, P);
    hipStream_t s = (hipStream_t)stream;
    knn_boxes(s, w.cloud, points, order);
    hipLaunchKernelGGL(ghr::k_field_pack, dim3((unsigned)((P + GHR_FIELD_BLOCK - 1) / GHR_FIELD_BLOCK)), dim3(GHR_FIELD_BLOCK), 0, s,
                       w.cloud, directions, weights, colors, const_cast<float4*>(w.pay.dm), const_cast<float4*>(w.pay.f));
    return finish(s, 0);
}

static unsigned field_wave_blocks(int64_t rows)
{
    const int64_t waves = (rows + GHR_KNN_BLOCK - 1) / GHR_KNN_BLOCK;
    return (unsigned)((waves + GHR_FIELD_WAVES - 1) / GHR_FIELD_WAVES);
}

int ghr_field_query(void* stream, int64_t P, const void* ws, int64_t Q, const float* x, const float* t, const int64_t* query_order,
                    float r2, float* rho, float* v, float* c, int32_t* n)
{
    static const char* fn = "ghr_field_query: %s";
    if (const char* why = field_cloud_bad(P)) return lt_bad(fn, why);
    if (Q < 0) return lt_bad(fn, "Q < 0");
    if (Q >= FIELD_2_31 / 3) return lt_bad(fn, "sizes exceed the kernels' 32-bit indexing");
    if (const char* why = field_radius_bad(r2)) return lt_bad(fn, why);
    if (!ws) return lt_bad(fn, "ws is NULL");
    if (!x || !t) return lt_bad(fn, "x or t is NULL");
    if (!rho || !v || !c || !n) return lt_bad(fn, "rho, v, c or n is NULL");
    if (Q == 0) return GHR_OK;
    const FieldWs w = field_carve(ws, P);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ghr::k_field_query, dim3(field_wave_blocks(Q)), dim3(64 * GHR_FIELD_WAVES), 0, s, w.cloud, w.pay, (int)Q, x, t,
                       (const long long*)query_order, r2, rho, v, c, n);
    return finish(s, 0);
}

// what ghr_field_trace and ghr_field_trace_guarded refuse alike, in one order
static const char* field_trace_bad(int64_t P, const void* ws, int64_t S, const float* roots, const float* normals, int32_t M, float r2,
                                   float h, float beta, float rho_min, int32_t max_coast, const float* path, const int32_t* steps,
                                   const float* rgb)
{
    if (const char* why = field_cloud_bad(P)) return why;
    if (S < 0) return "S < 0";
    if (M < 1) return "M < 1";
    if (S >= FIELD_2_31 || S * ((int64_t)M + 1) * 3 >= FIELD_2_31) return "sizes exceed the kernels' 32-bit indexing";
    if (const char* why = field_radius_bad(r2)) return why;
    if (!(h > 0.f) || !(h <= FLT_MAX)) return "h must be positive and finite";
    if (!(beta >= 0.f && beta <= 1.f)) return "beta must be in [0, 1]";
    if (!(rho_min > 0.f)) return "rho_min must be positive";
    if (max_coast < 0) return "max_coast < 0";
    if (!ws) return "ws is NULL";
    if (!roots || !normals) return "roots or normals is NULL";
    if (!path || !steps || !rgb) return "path, steps or rgb is NULL";
    return nullptr;
}

int ghr_field_trace(void* stream, int64_t P, const void* ws, int64_t S, const float* roots, const float* normals,
                    const int64_t* root_order, int32_t M, float r2, float h, float beta, float rho_min, int32_t max_coast, float* path,
                    int32_t* steps, float* rgb)
{
    static const char* fn = "ghr_field_trace: %s";
    if (const char* why = field_trace_bad(P, ws, S, roots, normals, M, r2, h, beta, rho_min, max_coast, path, steps, rgb)) return lt_bad(fn, why);
    if (S == 0) return GHR_OK;
    const FieldWs w = field_carve(ws, P);
    const ghr::FieldTraceArgs a{r2, h, beta, 1.f - beta, rho_min, M, max_coast};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ghr::k_field_trace, dim3(field_wave_blocks(S)), dim3(64 * GHR_FIELD_WAVES), 0, s, w.cloud, w.pay, (int)S, roots,
                       normals, (const long long*)root_order, a, path, steps, rgb);
    return finish(s, 0);
}

// ---- the guarded trace: strands grown around the head mesh (ghr_grow.h) -----------------------------------------------------------
int ghr_field_trace_guarded(void* stream, int64_t P, const void* ws, const ghr_mesh_tris* tris_header, const void* tris_dev,
                            const ghr_mesh_grid* grid_header, const void* grid_dev, int64_t S, const float* roots, const float* normals,
                            const int64_t* root_order, int32_t M, float r2, float h, float beta, float rho_min, int32_t max_coast,
                            float margin, float* path, int32_t* steps, float* rgb, int32_t* contacts, uint8_t* stop)
{
    static const char* fn = "ghr_field_trace_guarded: %s";
    if (const char* why = field_trace_bad(P, ws, S, roots, normals, M, r2, h, beta, rho_min, max_coast, path, steps, rgb)) return lt_bad(fn, why);
    if (!(margin > 0.f) || !(margin <= FLT_MAX)) return lt_bad(fn, "margin must be positive and finite");
    if (!contacts || !stop) return lt_bad(fn, "contacts or stop is NULL");
    if (!tris_header || !tris_dev) return lt_bad(fn, "tris_header or tris_dev is NULL");
    if (!grid_header || !grid_dev) return lt_bad(fn, "grid_header or grid_dev is NULL");
    if (int rc = tris_header_check("ghr_field_trace_guarded: tris_header: %s", tris_header, tris_dev)) return rc;
    if (int rc = mesh_header_check("ghr_field_trace_guarded: grid_header: %s", grid_header, grid_dev)) return rc;
    if (S == 0) return GHR_OK;
    const FieldWs w = field_carve(ws, P);
    const ghr::MeshTris& th = *reinterpret_cast<const ghr::MeshTris*>(tris_header);
    ghr::GrowArgs g{};
    g.c = w.cloud; g.pay = w.pay;
    g.md = ghr::md_view(th, tris_dev);
    for (int k = 0; k < 3; k++) g.md_bounds[k] = th.lo[k], g.md_bounds[3 + k] = th.hi[k];
    g.mesh = ghr::mesh_view(*reinterpret_cast<const ghr::MeshGrid*>(grid_header), grid_dev);
    g.a = ghr::FieldTraceArgs{r2, h, beta, 1.f - beta, rho_min, M, max_coast};
    g.margin = margin; g.S = (int)S;
    g.roots = roots; g.normals = normals; g.order = (const long long*)root_order;
    g.path = path; g.steps = steps; g.rgb = rgb; g.contacts = contacts; g.stop = stop;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ghr::k_grow_guarded, dim3(field_wave_blocks(S)), dim3(64 * GHR_FIELD_WAVES), 0, s, g);
    return finish(s, 0);
}

int ghr_strands_resample(void* stream, int64_t S, int32_t M, int32_t L, const float* path, const int32_t* steps, float* out)
{
    static const char* fn = "ghr_strands_resample: %s";
    if (S < 0) return lt_bad(fn, "S < 0");
    if (M < 1) return lt_bad(fn, "M < 1");
    if (L < 2) return lt_bad(fn, "L < 2");
    if (S >= FIELD_2_31 || S * ((int64_t)M + 1) * 3 >= FIELD_2_31 || S * (int64_t)L * 3 >= FIELD_2_31)
        return lt_bad(fn, "sizes exceed the kernels' 32-bit indexing");
    if (!path || !steps) return lt_bad(fn, "path or steps is NULL");
    if (!out) return lt_bad(fn, "out is NULL");
    if (S == 0) return GHR_OK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ghr::k_strands_resample, dim3((unsigned)((S * L + GHR_FIELD_BLOCK - 1) / GHR_FIELD_BLOCK)), dim3(GHR_FIELD_BLOCK),
                       0, s, (int)S, (int)M, (int)L, path, steps, out);
    return finish(s, 0);
}

}  // extern "C"

// ---- the strand shape term: neighbours over the roots, forward, backward (ghr_shape.h) --------------------------------------------
namespace {
// the sizes the three entries share, before anything touches the runtime
const char* shape_sizes(int64_t S, int64_t n)
{
    if (S < 0) return "S < 0";
    if (n < 1) return "n < 1";
    if (GHR_SHAPE_K * S >= ((int64_t)1 << 31) || S * n * 3 >= ((int64_t)1 << 31)) return "sizes exceed the kernels' 32-bit indexing";
    return nullptr;
}
unsigned shape_blocks(int64_t S) { return (unsigned)((S + GHR_SHAPE_BLOCK / GHR_SHAPE_WAVE - 1) / (GHR_SHAPE_BLOCK / GHR_SHAPE_WAVE)); }
}  // namespace

extern "C" {

int ghr_shape_neighbours(void* stream, int32_t S, const float* roots, float r2, int32_t* nbr)
{
    static const char* fn = "ghr_shape_neighbours: %s";
    if (const char* why = shape_sizes(S, 1)) return lt_bad(fn, why);
    if (!(r2 > 0.f)) return lt_bad(fn, "r2 must be positive (+inf: no cut)");
    if (!roots) return lt_bad(fn, "roots is NULL");
    if (!nbr) return lt_bad(fn, "nbr is NULL");
    if (S == 0) return GHR_OK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ghr::k_shape_nbr, dim3((unsigned)((S + GHR_SHAPE_WAVE - 1) / GHR_SHAPE_WAVE)), dim3(GHR_SHAPE_WAVE), 0, s, (int)S, roots,
                       r2, nbr);
    return finish(s, 0);
}

int ghr_shape_forward(void* stream, int32_t S, int32_t n, const float* dirs, const float* rest, const int32_t* nbr, int64_t M,
                      float* partial, float* E)
{
    static const char* fn = "ghr_shape_forward: %s";
    if (const char* why = shape_sizes(S, n)) return lt_bad(fn, why);
    if (M < 0) return lt_bad(fn, "M < 0");
    if (M > (int64_t)GHR_SHAPE_K * S) return lt_bad(fn, "M > 4 S: more pairs than choices");
    if (!dirs || !rest || !nbr) return lt_bad(fn, "dirs, rest or nbr is NULL");
    if (!partial || !E) return lt_bad(fn, "partial or E is NULL");
    if (S == 0) return GHR_OK;
    hipStream_t s = (hipStream_t)stream;
    ghr::ShapeArgs a{};
    a.S = S; a.n = n; a.dirs = dirs; a.rest = rest; a.nbr = nbr; a.partial = partial;
    ghr::shape_divisors(S, n, M, a.div);
    hipLaunchKernelGGL(ghr::k_shape_fwd, dim3(shape_blocks(S)), dim3(GHR_SHAPE_BLOCK), 0, s, a);
    hipLaunchKernelGGL(ghr::k_shape_fold, dim3(1), dim3(GHR_SHAPE_FOLD), 0, s, (int)S, (const float*)partial, a.div[0], a.div[1], a.div[2], E);
    return finish(s, 0);
}

int ghr_shape_backward(void* stream, int32_t S, int32_t n, const float* dirs, const float* rest, const int32_t* nbr, const int32_t* start,
                       const int32_t* list, int64_t M, const float* dE, float* d_dirs)
{
    static const char* fn = "ghr_shape_backward: %s";
    if (const char* why = shape_sizes(S, n)) return lt_bad(fn, why);
    if (M < 0) return lt_bad(fn, "M < 0");
    if (M > (int64_t)GHR_SHAPE_K * S) return lt_bad(fn, "M > 4 S: more pairs than choices");
    if (!dirs || !rest || !nbr) return lt_bad(fn, "dirs, rest or nbr is NULL");
    if (!start || !list) return lt_bad(fn, "start or list is NULL");
    if (!dE) return lt_bad(fn, "dE is NULL");
    if (!d_dirs) return lt_bad(fn, "d_dirs is NULL");
    if (S == 0) return GHR_OK;
    hipStream_t s = (hipStream_t)stream;
    ghr::ShapeArgs a{};
    a.S = S; a.n = n; a.dirs = dirs; a.rest = rest; a.nbr = nbr; a.start = start; a.list = list; a.M = (int)M; a.dE = dE; a.d_dirs = d_dirs;
    ghr::shape_divisors(S, n, M, a.div);
    hipLaunchKernelGGL(ghr::k_shape_bwd, dim3(shape_blocks(S)), dim3(GHR_SHAPE_BLOCK), 0, s, a);
    return finish(s, 0);
}

}  // extern "C"

// ---- groom upsampling: the guides nearest to every child root, the gated blend (ghr_upsample.h) -----------------------------------
namespace {
const int64_t UPS_LIMIT = (int64_t)1 << 31;
}  // namespace

extern "C" {

int ghr_upsample_neighbours(void* stream, int32_t G, const float* guide_roots, int32_t N, const float* child_origins, float r2,
                            int32_t* nbr, float* nd2)
{
    static const char* fn = "ghr_upsample_neighbours: %s";
    if (G < 1) return lt_bad(fn, "G < 1");
    if (N < 0) return lt_bad(fn, "N < 0");
    if (!(r2 > 0.f)) return lt_bad(fn, "r2 must be positive (+inf: no cut)");
    if (3 * (int64_t)G >= UPS_LIMIT || GHR_UPS_K * (int64_t)N >= UPS_LIMIT) return lt_bad(fn, "sizes exceed the kernels' 32-bit indexing");
    if (!guide_roots || !child_origins) return lt_bad(fn, "guide_roots or child_origins is NULL");
    if (!nbr || !nd2) return lt_bad(fn, "nbr or nd2 is NULL");
    if (N == 0) return GHR_OK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ghr::k_ups_near, dim3((unsigned)(((int64_t)N + GHR_UPS_BLOCK - 1) / GHR_UPS_BLOCK)), dim3(GHR_UPS_BLOCK), 0, s, (int)G,
                       guide_roots, (int)N, child_origins, r2, nbr, nd2);
    return finish(s, 0);
}

int ghr_upsample_blend(void* stream, int32_t G, int32_t L, const float* gp, const float* gM, const float* gf, int32_t F, int32_t N,
                       const float* co, const float* cM, const int32_t* nbr, const float* nd2, float eps2, float tau, int32_t gate,
                       float* out, float* w, float* of, uint8_t* valid)
{
    static const char* fn = "ghr_upsample_blend: %s";
    if (G < 1) return lt_bad(fn, "G < 1");
    if (N < 0) return lt_bad(fn, "N < 0");
    if (L < 2) return lt_bad(fn, "L < 2");
    if (F < 0) return lt_bad(fn, "F < 0");
    if (!(eps2 > 0.f) || !(eps2 < INFINITY)) return lt_bad(fn, "eps2 must be positive and finite");
    if (gate && !(tau >= -1.f && tau < 1.f)) return lt_bad(fn, "tau must lie in [-1, 1) while the gate is set");
    const int64_t big = (int64_t)(G > N ? G : N);
    if (big * L * 3 >= UPS_LIMIT || big * 9 >= UPS_LIMIT || big * F >= UPS_LIMIT || GHR_UPS_K * (int64_t)N >= UPS_LIMIT)
        return lt_bad(fn, "sizes exceed the kernels' 32-bit indexing");
    if (!gp || !gM) return lt_bad(fn, "gp or gM is NULL");
    if (!co || !cM) return lt_bad(fn, "co or cM is NULL");
    if (!nbr || !nd2) return lt_bad(fn, "nbr or nd2 is NULL");
    if (F > 0 && (!gf || !of)) return lt_bad(fn, "gf or of is NULL while F > 0");
    if (!out || !w || !valid) return lt_bad(fn, "out, w or valid is NULL");
    if (N == 0) return GHR_OK;
    hipStream_t s = (hipStream_t)stream;
    ghr::UpsArgs a{};
    a.G = G; a.L = L; a.F = F; a.N = N; a.gp = gp; a.gM = gM; a.gf = gf; a.co = co; a.cM = cM; a.nbr = nbr; a.nd2 = nd2;
    a.eps2 = eps2; a.tau = tau; a.gate = gate ? 1 : 0; a.out = out; a.w = w; a.of = of; a.valid = valid;
    const int per = GHR_UPS_BLOCK / GHR_UPS_WAVE;
    hipLaunchKernelGGL(ghr::k_ups_blend, dim3((unsigned)(((int64_t)N + per - 1) / per)), dim3(GHR_UPS_BLOCK), 0, s, a);
    return finish(s, 0);
}

}  // extern "C"
