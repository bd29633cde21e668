// ghr_strandview.h -- a preview of the groom: S strands of L points drawn as depth-tested polylines over the head mesh
// (DESIGN.md 8l).  It stands where the reference's run.sh ends, src/postprocessing/render_video.py: that script hands the strands,
// the head mesh and a camera path to Blender's Cycles hair (render_color.py on main.blend, a file the reference does not ship).
// Blender is not a dependency, so the picture is DEFINED here, exactly and independently of any traversal order, and every form
// (these kernels, the host simulator, the PyTorch comparator, the numpy model of the tests) is held to it bit for bit.
// Everything is float32 without contraction, in the operand order written; only + - x /, sqrtf, fminf / fmaxf, comparisons and
// integer arithmetic are used (no powf / expf / rsqrt), so that no bit depends on a math library.
//
//   View: M[12], H, W, near exactly as in 8h (ghr_visibility.h).  A point is projected by ghr::vis_project_one to
//       (sx, sy, q = 1 / w, valid).  Pixel (row i, column j) is sampled at its centre c = (j + 0.5, i + 0.5).
//   Segments: segment k = s (L - 1) + i joins points i and i + 1 of strand s.  It EXISTS iff both end points are valid.  Nothing is
//       clipped: a segment with an end behind `near`, or with a NaN coordinate, is dropped whole.
//   Coverage: half-width r (pixels, finite, > 0), screen ends a, b.  d = b - a, len2 = dx dx + dy dy, and for a centre c
//       t = ((cx - ax) dx + (cy - ay) dy) / len2, clamped to [0, 1] as fminf(fmaxf(t, 0), 1);  t = 0 when len2 == 0 or t is NaN;
//       e = c - (a + t d), i.e. ex = cx - (ax + t dx);
//       the segment COVERS the pixel iff  ex ex + ey ey <= r r  (a closed capsule; a disc when the ends coincide)
//       and c lies in the closed box [fminf(ax, bx) - r, fmaxf(ax, bx) + r] x [fminf(ay, by) - r, fmaxf(ay, by) + r].
//       The box is implied by the capsule in exact arithmetic (as the box rule of 8g and 8h is implied by their side rule);
//       stating it with the very floats the binning uses makes the tile lists and the wave skip EXACT instead of nearly safe.
//   Inverse depth: qs = qa + t (qb - qa) -- inverse depth is linear along the screen segment.
//   Strand WINNER of a pixel: the covering segment with the largest qs, the lowest k among equals; a qs that is NaN or not > 0
//       never wins.  A maximum under a total order: binning, chunking and traversal order cannot change a bit of it.
//   Head: pix_to_face [H][W] is 8h's winner plane, an input (or none: no mesh).  qf is 8h's inverse-depth expression of that
//       face at the centre (sv_face_depth_one: vis_covers of the face's own record).  An entry outside 0 .. F - 1, or a face
//       that does not cover the centre with an inverse depth > 0, counts as no face (qf = 0).
//       The strand winner is KEPT iff there is no face, or  qs (1 + head_bias) >= qf  (head_bias >= 0, default 0: roots sit on
//       the scalp, a caller may lift them).  Otherwise the head owns the pixel.
//   Outputs, all [H][W]:  pix_to_segment int32 (-1: none, or hidden by the head), t float (0 where -1), pix_to_face_out int32
//       (-1 where a strand is kept or nothing is there), inv_depth float (qs, qf or 0).
//   Shading, uint8 [H][W][3], modes GHR_SV_KAJIYA (0, default) and GHR_SV_TANGENT (1).  A, B: the winner's two WORLD points.
//       T = (B - A) / |B - A|, |x| = sqrtf((x0 x0 + x1 x1) + x2 x2); T = (0, 0, 0) when the length is 0.
//       Dot products are (a0 b0 + a1 b1) + a2 b2.
//       tangent:  colour = 0.5 + 0.5 T.
//       kajiya:   V = eye - 0.5 (A + B), normalised the same way; Lw a world-space unit vector towards the light;
//                 cl = T.Lw, cv = T.V, sl = sqrtf(fmaxf(0, 1 - cl cl)), sv likewise; diffuse = sl;
//                 spec = fmaxf(0, cl cv + sl sv), then squared shininess_log2 times (default 5: the power 32);
//                 colour = base[s] (ambient + kd diffuse) + ks spec.
//       head pixel: n = (v1 - v0) x (v2 - v0) of the face, normalised the same way; colour = head_rgb (ambient + kd |n.Lw|),
//                 |x| = fmaxf(x, -x).
//       elsewhere: background_rgb.
//       byte = quant8(clamp01(colour)) -- torchvision's save_image rule, ghr_products.h.
//       Defaults (this header's and the README's): ambient 0.25, kd 0.65, ks 0.35, shininess_log2 5, hair (0.45, 0.30, 0.18)
//       (a warm brown), head (0.62, 0.62, 0.62), background (1, 1, 1); the light (0.45, -0.60, -0.66) in camera axes (x right,
//       y down, z forward: above and to the right of the camera, on its side of the head), normalised and rotated to world;
//       eye and Lw are formed on the host in double and rounded once.
//   Supersampling s in {1, 2, 4}: rows 0 and 1 of M and r are multiplied by s (exact: a power of two), 8h's raster, this raster
//       and the shade run at sH x sW, and sv_resolve_one writes (sum of the s x s bytes + s s / 2) / (s s) per channel, in integers.
//   Self-shadowing: a deep opacity map (Yuksel & Keyser 2008) -- per texel of a LIGHT view, the strands in front of a
//       point counted in four layers behind the first one.  Integer counts and float32 + - x / only; 1 / x is the IEEE division.
//       Light view: (Ml[12], Hl, Wl, near), a view as above (perspective: q = 1 / w orders depth), texel centres at + 0.5.
//       Front plane q0 [Hl][Wl]: the largest qs over the segments that COVER the texel's centre (the coverage rule above with the
//           light half-width rl, in texels); a qs that is NaN or not > 0 never counts; 0 where there is none.
//       Layer counts, layers [Hl][Wl][4] uint32: every segment that covers the centre with a counted qs has
//           u = 1 / qs - 1 / q0  (>= 0: division is monotone)  and adds 1 to layer 0 if u < d, else to layer 1 if u < 3 d, else to
//           layer 2 if u < 7 d, else to layer 3 (sv_layer_of); d = `layer`, a depth in the light's w units, finite and > 0; 3 d and
//           7 d are 3.f * d and 7.f * d.  Integer sums of a set: chunking, binning and traversal order cannot change a bit;
//           duplicated segments each count.
//       Lookup of a world point P (the occluders in front of it, sv_occluders): P is projected by Ml to (lx, ly, ql, valid).
//           n = 0 when P is not valid, when  lx >= 0 && lx < (float)Wl && ly >= 0 && ly < (float)Hl  is false, when q0 == 0 at
//           texel (i, j) = ((int)ly, (int)lx), or when  u = 1 / ql - 1 / q0  is not > 0.  Otherwise, with c0 = n0, c1 = c0 + n1,
//           c2 = c1 + n2 as integers, every count clamped to 2^24 and converted to float:
//               u < d:    n = c0 (u / d)
//               u < 3 d:  n = c0 + n1 ((u - d) / (2.f d))
//               u < 7 d:  n = c1 + n2 ((u - 3.f d) / (4.f d))
//               else:     n = c2 + n3 fminf((u - 7.f d) / (8.f d), 1.f)
//           A point's own segment is in the counts; at u ~ 0 its share is ~ 0: the method's answer to self-shadowing acne.
//       Head as an occluder: qfl [Hl][Wl] is 8h's pix_to_face of the mesh in the light view put through the face depth above (or
//           absent: no mesh).  P is BEHIND THE HEAD iff qfl > 0 at its texel and  ql (1.f + shadow_bias) < qfl.
//       Transmittance: Tr = 0 behind the head, else Tr = 1.f / (1.f + kappa n); Tr == 1 exactly where n == 0.
//       Shading with shadows (kajiya only; tangent mode and the background are untouched):
//           strand pixel (winner k, t from the t plane): P = A + t (B - A) per component;
//               colour = base (ambient + kd (Tr diffuse)) + ks (Tr spec);
//           head pixel: P = ((v0 + v1) + v2) / 3.f per component (flat shading: the shadow is per face);
//               colour = head_rgb (ambient + kd (Tr |n.Lw|)).
//           With Tr == 1 these are the unshadowed bytes: 1.f x == x.
//       Look constants (defaults of the keywords, CHOSEN here like ambient and kd, not measured): light map 1024 x 1024, rl 1.0 texel,
//           kappa 0.2, shadow_bias 0.02, d = rho / 32 with rho the radius of the bounding sphere the light camera is fitted to.
//
// Per frame (ghr_strandview_raster): the fill, projection, scan and scatter of ghr_tilelists.h (which also owns the tile rectangle
// and the staged walk of a tile's list), and this header's own kernels:
//   k_sv_setup     one thread per segment: a 32-B record  ax ay bx by | qa qb xy bits  from its two projected points, then tl_count.
//                  The rectangle is tl_pixel_range of the box widened by r -- the same four floats the coverage rule compares the
//                  centre with -- so it can never be too small: a centre inside the closed box satisfies j + 0.5 >= lo, and
//                  tl_pixel_range's floor of the rounded lo - 0.5 is never above such a j (monotone rounding, j exact), likewise
//                  at the upper end.  A segment of more than GHR_SV_BIG_RECT tiles goes to the big list.
//   k_sv_raster    the tile's walk with GHR_SV_CHUNK records per round (tl_walk's loop written out here: it measured faster so) and
//                  the winner's total order; pix_to_face / qf are read once.
// and, on their own entries: k_sv_face_depth (one thread per pixel: qf), k_sv_shade (one thread per pixel: it gathers the winner's
// two world points or the face's three vertices), k_sv_resolve (one thread per output pixel).  Integer atomics only.
// The light pass (ghr_strandview_opacity) is the same lists in the light view, then
//   k_sv_layers    k_sv_raster's shape, but TWO tl_walks in one launch: walk 1 keeps the largest qs in a register, walk 2 re-tests
//                  coverage and classifies every covering segment against that register into four counters in registers; the
//                  epilogue writes q0 (4 B) and the four counts as one 16-B store.  No atomics, no pix_to_face, no segment ids.
// and k_sv_shade_shadowed (one thread per camera pixel, behind ghr_strandview_shade_shadowed) is k_sv_shade with the lookup.
// Everything per element is GHR_HD so that tests/hostsim/ghr_hostsim_strandview.cpp runs the product's own arithmetic on the CPU.
#pragma once
#include "ghr_visibility.h"
#if defined(__HIPCC__)
#include "ghr_products.h"
#endif

#define GHR_SV_TILE GHR_TL_TILE
#define GHR_SV_BLOCK GHR_TL_BLOCK
#define GHR_SV_CHUNK 128     // records staged in LDS per round of k_sv_raster (two 16-B units each: one per thread)
#define GHR_SV_REC_WORDS 8   // two 16-B units per segment
#define GHR_SV_REC_UNITS (GHR_SV_REC_WORDS / 4)
#define GHR_SV_BIG_RECT 16   // a segment of more tiles than this goes to the big list
#define GHR_SV_NEVER GHR_TL_NEVER  // the list builder's flags in a record's last word, under the names a walk of segments reads them by
#define GHR_SV_EMPTY GHR_TL_EMPTY
#define GHR_SV_BIG GHR_TL_BIG
#define GHR_SV_KAJIYA 0
#define GHR_SV_TANGENT 1
#define GHR_SV_MAX_SHININESS_LOG2 16

namespace ghr {

// == ghr_strandview_shading of include/ghr.h
struct SvShading {
    float eye[3], light[3];
    float ambient, kd, ks;
    int32_t shininess_log2;
    float base_rgb[3], head_rgb[3], background_rgb[3];
};

// One segment: its record from the projected end points pa, pb = {sx, sy, q, valid}.
GHR_HD void sv_setup_one(const float* pa, const float* pb, float r, int H, int W, float* rec)
{
    const bool never = pa[3] == 0.f || pb[3] == 0.f;
    rec[0] = pa[0]; rec[1] = pa[1]; rec[2] = pb[0]; rec[3] = pb[1]; rec[4] = pa[2]; rec[5] = pb[2];
    const float ulo = fminf(pa[0], pb[0]) - r, uhi = fmaxf(pa[0], pb[0]) + r;
    const float vlo = fminf(pa[1], pb[1]) - r, vhi = fmaxf(pa[1], pb[1]) + r;
    tl_rect(never ? GHR_SV_NEVER : 0u, ulo, uhi, vlo, vhi, H, W, GHR_SV_BIG_RECT, rec + 6);
}

GHR_HD bool sv_in_box(const float* rec, float r, float px, float py)
{
    const float ulo = fminf(rec[0], rec[2]) - r, uhi = fmaxf(rec[0], rec[2]) + r;
    const float vlo = fminf(rec[1], rec[3]) - r, vhi = fmaxf(rec[1], rec[3]) + r;
    return px >= ulo && px <= uhi && py >= vlo && py <= vhi;
}

// One record against one pixel centre: does the segment cover it, where along itself and with which inverse depth?
GHR_HD bool sv_covers(const float* rec, float r, float px, float py, float* t_out, float* qs)
{
    uint32_t bits;
    memcpy(&bits, rec + 7, 4);
    if ((bits & GHR_SV_NEVER) || !sv_in_box(rec, r, px, py)) return false;
    const float ax = rec[0], ay = rec[1], bx = rec[2], by = rec[3], qa = rec[4], qb = rec[5];
    const float dx = bx - ax, dy = by - ay;
    const float len2 = dx * dx + dy * dy;
    float t = ((px - ax) * dx + (py - ay) * dy) / len2;
    t = fminf(fmaxf(t, 0.f), 1.f);
    if (len2 == 0.f || t != t) t = 0.f;
    const float ex = px - (ax + t * dx), ey = py - (ay + t * dy);
    if (!(ex * ex + ey * ey <= r * r)) return false;
    *t_out = t;
    *qs = qa + t * (qb - qa);
    return true;
}

// The total order of the winner: (inverse depth, lower index).  best starts at (0, -1): only a qs > 0 gets in, a NaN never.
GHR_HD void sv_take(float q, float t, int32_t k, float* best_q, float* best_t, int32_t* best_k)
{
    if (q > *best_q || (q == *best_q && k < *best_k)) { *best_q = q; *best_t = t; *best_k = k; }
}

// 8h's inverse depth of face f at a pixel centre, from the mesh itself; 0: no face there.
GHR_HD float sv_face_depth_one(const float* M, float near, const float* vertices, int V, const int32_t* faces, int F, int32_t f,
                               float px, float py)
{
    if (f < 0 || f >= F) return 0.f;
    const int32_t t[3] = {faces[3 * (size_t)f], faces[3 * (size_t)f + 1], faces[3 * (size_t)f + 2]};
    if (t[0] < 0 || t[0] >= V || t[1] < 0 || t[1] >= V || t[2] < 0 || t[2] >= V) return 0.f;
    float p[3][4];
    for (int k = 0; k < 3; k++) vis_project_one(M, vertices + 3 * (size_t)t[k], near, p[k]);
    float r[GHR_VIS_REC_WORDS], d;
    const uint32_t bits = vis_face_record(p[0], p[1], p[2], t, r);  // (a NEVER face fails vis_covers)
    r[10] = 0.f;
    memcpy(r + 11, &bits, 4);
    if (!vis_covers(r, px, py, &d)) return 0.f;
    return d > 0.f ? d : 0.f;  // (a NaN fails the comparison)
}

// Strand winner (best_k, best_t, best_q; best_k < 0: none) against the head (face, qf): the four planes' values at one pixel.
GHR_HD void sv_resolve_head(int32_t best_k, float best_t, float best_q, int32_t face, float qf, float head_bias, int32_t* seg,
                            float* t, int32_t* face_out, float* inv_depth)
{
    const bool has_face = qf > 0.f;
    if (best_k >= 0 && (!has_face || best_q * (1.f + head_bias) >= qf)) {
        *seg = best_k; *t = best_t; *face_out = -1; *inv_depth = best_q;
    } else if (has_face) {
        *seg = -1; *t = 0.f; *face_out = face; *inv_depth = qf;
    } else {
        *seg = -1; *t = 0.f; *face_out = -1; *inv_depth = 0.f;
    }
}

GHR_HD float sv_dot(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// x / |x|, (0, 0, 0) when the length is 0
GHR_HD void sv_normalise(const float* x, float* out)
{
    const float len = sqrtf(sv_dot(x, x));
    for (int c = 0; c < 3; c++) out[c] = len == 0.f ? 0.f : x[c] / len;
}

GHR_HD uint32_t sv_quant8(float v)
{
#if defined(__HIPCC__)
    return quant8(clamp01(v));
#else  // (ghr_products.h needs the HIP runtime; its two expressions, for the host simulator)
    return (uint32_t)fminf(fmaxf(fminf(fmaxf(v, 0.f), 1.f) * 255.f + 0.5f, 0.f), 255.f);
#endif
}

// Tr: the transmittance on the two light terms; 1.f (1.f x == x) where there is no shadow map.  Tangent mode has no light.
GHR_HD void sv_shade_strand(const float* A, const float* B, const float* base, int mode, const SvShading& sh, float Tr, uint8_t* rgb)
{
    const float d[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]};
    float T[3];
    sv_normalise(d, T);
    if (mode == GHR_SV_TANGENT) {
        for (int c = 0; c < 3; c++) rgb[c] = (uint8_t)sv_quant8(0.5f + 0.5f * T[c]);
        return;
    }
    const float v[3] = {sh.eye[0] - 0.5f * (A[0] + B[0]), sh.eye[1] - 0.5f * (A[1] + B[1]), sh.eye[2] - 0.5f * (A[2] + B[2])};
    float Vn[3];
    sv_normalise(v, Vn);
    const float cl = sv_dot(T, sh.light), cv = sv_dot(T, Vn);
    const float sl = sqrtf(fmaxf(0.f, 1.f - cl * cl)), sv = sqrtf(fmaxf(0.f, 1.f - cv * cv));
    float spec = fmaxf(0.f, cl * cv + sl * sv);
    for (int k = 0; k < sh.shininess_log2; k++) spec = spec * spec;
    for (int c = 0; c < 3; c++) rgb[c] = (uint8_t)sv_quant8(base[c] * (sh.ambient + sh.kd * (Tr * sl)) + sh.ks * (Tr * spec));
}

GHR_HD void sv_shade_head(const float* v0, const float* v1, const float* v2, const SvShading& sh, float Tr, uint8_t* rgb)
{
    const float e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]}, e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
    const float n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    float nn[3];
    sv_normalise(n, nn);
    const float c = sv_dot(nn, sh.light);
    const float lit = sh.ambient + sh.kd * (Tr * fmaxf(c, -c));
    for (int k = 0; k < 3; k++) rgb[k] = (uint8_t)sv_quant8(sh.head_rgb[k] * lit);
}

// One pixel of the picture.  An index that points outside its table shades as background (the planes are a caller's).
GHR_HD void sv_shade_one(int32_t seg, int32_t face, int S, int L, const float* points, int V, const float* vertices, int F,
                         const int32_t* faces, const float* base, int mode, const SvShading& sh, uint8_t* rgb)
{
    if (seg >= 0 && L >= 2 && (int64_t)seg < (int64_t)S * (L - 1)) {
        const int s = seg / (L - 1), i = seg % (L - 1);
        const float* A = points + 3 * ((size_t)s * L + i);
        sv_shade_strand(A, A + 3, base ? base + 3 * (size_t)s : sh.base_rgb, mode, sh, 1.f, rgb);
        return;
    }
    if (face >= 0 && face < F) {
        const int32_t* t = faces + 3 * (size_t)face;
        if (t[0] >= 0 && t[0] < V && t[1] >= 0 && t[1] < V && t[2] >= 0 && t[2] < V) {
            sv_shade_head(vertices + 3 * (size_t)t[0], vertices + 3 * (size_t)t[1], vertices + 3 * (size_t)t[2], sh, 1.f, rgb);
            return;
        }
    }
    for (int c = 0; c < 3; c++) rgb[c] = (uint8_t)sv_quant8(sh.background_rgb[c]);
}

// ---- self-shadowing: the deep opacity map of the light view -------------------------------------------------------------------
// == ghr_strandview_shadow of include/ghr.h
struct SvShadow {
    float Ml[12];
    float near_w;
    int32_t Hl, Wl;
    float layer, kappa, bias;
    const float* q0;         // [Hl][Wl]
    const uint32_t* layers;  // [Hl][Wl][4]
    const float* qfl;        // [Hl][Wl] or NULL: no mesh
};

// The layer of a covering segment u = 1 / qs - 1 / q0 behind the front plane.
GHR_HD int sv_layer_of(float u, float d)
{
    if (u < d) return 0;
    if (u < 3.f * d) return 1;
    if (u < 7.f * d) return 2;
    return 3;
}

GHR_HD float sv_count_float(uint32_t c) { return (float)(c < (1u << 24) ? c : (1u << 24)); }

// The occluders in front of a point of inverse depth ql at a texel with front plane q0 and the four counts n4.
GHR_HD float sv_occluders(float ql, float q0, const uint32_t* n4, float d)
{
    if (q0 == 0.f) return 0.f;
    const float u = 1.f / ql - 1.f / q0;
    if (!(u > 0.f)) return 0.f;
    const uint32_t i0 = n4[0], i1 = i0 + n4[1], i2 = i1 + n4[2];
    const float c0 = sv_count_float(i0), c1 = sv_count_float(i1), c2 = sv_count_float(i2);
    if (u < d) return c0 * (u / d);
    if (u < 3.f * d) return c0 + sv_count_float(n4[1]) * ((u - d) / (2.f * d));
    if (u < 7.f * d) return c1 + sv_count_float(n4[2]) * ((u - 3.f * d) / (4.f * d));
    return c2 + sv_count_float(n4[3]) * fminf((u - 7.f * d) / (8.f * d), 1.f);
}

GHR_HD float sv_transmittance(float n, float kappa, bool behind_head) { return behind_head ? 0.f : 1.f / (1.f + kappa * n); }

// Tr of a world point P; *n_out (may be NULL) gets the occluders in front of it (0 where the point has no texel).
GHR_HD float sv_shadow_at(const SvShadow& sd, const float* P, float* n_out)
{
    float o[4], n = 0.f;
    bool behind = false;
    vis_project_one(sd.Ml, P, sd.near_w, o);
    if (o[3] != 0.f && o[0] >= 0.f && o[0] < (float)sd.Wl && o[1] >= 0.f && o[1] < (float)sd.Hl) {
        const size_t e = (size_t)(int)o[1] * (size_t)sd.Wl + (size_t)(int)o[0];  // (0 <= (int)x < the size: x is in [0, size))
        const float qfl = sd.qfl ? sd.qfl[e] : 0.f;
        behind = qfl > 0.f && o[2] * (1.f + sd.bias) < qfl;
        const float q0 = sd.q0[e];
        if (q0 != 0.f) n = sv_occluders(o[2], q0, sd.layers + 4 * e, sd.layer);
    }
    if (n_out) *n_out = n;
    return sv_transmittance(n, sd.kappa, behind);
}

// One pixel of the shadowed picture: sv_shade_one with the lookup at the strand point A + t (B - A) or at the face's centroid.
GHR_HD void sv_shade_one_shadowed(int32_t seg, int32_t face, float t, int S, int L, const float* points, int V, const float* vertices,
                                  int F, const int32_t* faces, const float* base, int mode, const SvShading& sh, const SvShadow& sd,
                                  uint8_t* rgb)
{
    if (mode == GHR_SV_KAJIYA && seg >= 0 && L >= 2 && (int64_t)seg < (int64_t)S * (L - 1)) {
        const int s = seg / (L - 1), i = seg % (L - 1);
        const float* A = points + 3 * ((size_t)s * L + i);
        const float* B = A + 3;
        const float P[3] = {A[0] + t * (B[0] - A[0]), A[1] + t * (B[1] - A[1]), A[2] + t * (B[2] - A[2])};
        sv_shade_strand(A, B, base ? base + 3 * (size_t)s : sh.base_rgb, mode, sh, sv_shadow_at(sd, P, nullptr), rgb);
        return;
    }
    if (mode == GHR_SV_KAJIYA && face >= 0 && face < F) {  // (no strand here: the branch above returned)
        const int32_t* tr = faces + 3 * (size_t)face;
        if (tr[0] >= 0 && tr[0] < V && tr[1] >= 0 && tr[1] < V && tr[2] >= 0 && tr[2] < V) {
            const float *v0 = vertices + 3 * (size_t)tr[0], *v1 = vertices + 3 * (size_t)tr[1], *v2 = vertices + 3 * (size_t)tr[2];
            const float P[3] = {((v0[0] + v1[0]) + v2[0]) / 3.f, ((v0[1] + v1[1]) + v2[1]) / 3.f, ((v0[2] + v1[2]) + v2[2]) / 3.f};
            sv_shade_head(v0, v1, v2, sh, sv_shadow_at(sd, P, nullptr), rgb);
            return;
        }
    }
    sv_shade_one(seg, face, S, L, points, V, vertices, F, faces, base, mode, sh, rgb);  // tangent mode, the background
}

// One output pixel of the resolve: src is [s H][s W][3], dst [H][W][3].
GHR_HD void sv_resolve_one(const uint8_t* src, int W, int s, int i, int j, uint8_t* dst)
{
    for (int c = 0; c < 3; c++) {
        uint32_t sum = 0u;
        for (int di = 0; di < s; di++)
            for (int dj = 0; dj < s; dj++) sum += src[3 * (((size_t)i * s + di) * ((size_t)W * s) + (size_t)j * s + dj) + c];
        dst[3 * ((size_t)i * W + j) + c] = (uint8_t)((sum + (uint32_t)(s * s) / 2u) / (uint32_t)(s * s));
    }
}

// ---- the workspace ---------------------------------------------------------------------------------------------------------
// The tile lists of ghr_tilelists.h over the S L points and the S (L - 1) segments, and nothing else.
struct SvLayout : TileListLayout {
    uint64_t bytes, n_points, n_segments;
};

inline const char* sv_layout(int64_t S, int64_t L, int64_t H, int64_t W, SvLayout* Y)
{
    if (L < 2) return "L < 2: a strand needs two points";
    if (S > 0 && L > (0x7fffffffll / 3) / S) return "S * L * 3 exceeds 32-bit offsets";
    // (S * L fits from here on; a negative S is passed on as it is, for the refusal)
    const int64_t N = S < 0 ? S : S * L, K = S < 0 ? S : S * (L - 1);
    if (const char* why = tl_layout(N, K, H, W, GHR_SV_REC_UNITS, GHR_SV_BIG_RECT, Y)) return why;
    Y->n_points = (uint64_t)N; Y->n_segments = (uint64_t)K;
    Y->bytes = Y->off_fill + Y->fill_bytes + 16;  // (never 0: a caller's allocation of `bytes` has an address)
    return nullptr;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
struct SvArgs {
    TileLists tl;                // points [S][L][3]; n_prims = S (L - 1)
    int32_t L, H, W;
    float r, head_bias;
    const int32_t* pix_to_face;  // [H][W] or NULL: no mesh
    const float* qf;             // [H][W] or NULL with it
    int32_t* pix_to_segment;     // [H][W]
    float* t;                    // [H][W]
    int32_t* pix_to_face_out;    // [H][W]
    float* inv_depth;            // [H][W]
};

__global__ void __launch_bounds__(GHR_SV_BLOCK) k_sv_setup(SvArgs a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t k = blockIdx.x * GHR_SV_BLOCK + threadIdx.x;
    if (k >= a.tl.n_prims) return;
    const uint32_t s = k / (uint32_t)(a.L - 1), i = k % (uint32_t)(a.L - 1);
    const size_t p = (size_t)s * (uint32_t)a.L + i;  // (p + 1 < S L)
    const f4 pa = reinterpret_cast<const f4*>(a.tl.proj)[p], pb = reinterpret_cast<const f4*>(a.tl.proj)[p + 1];
    const float fa[4] = {pa.x, pa.y, pa.z, pa.w}, fb[4] = {pb.x, pb.y, pb.z, pb.w};
    float r[GHR_SV_REC_WORDS];
    sv_setup_one(fa, fb, a.r, a.H, a.W, r);
    f4* out = reinterpret_cast<f4*>(a.tl.rec) + 2 * (size_t)k;
    out[0] = f4{r[0], r[1], r[2], r[3]};
    out[1] = f4{r[4], r[5], r[6], r[7]};
    tl_count(a.tl, r + 6, k);
#endif
}

// One tile per workgroup, one pixel per thread (a wave holds 4 rows of 16 pixels).
__global__ void __launch_bounds__(GHR_SV_BLOCK) k_sv_raster(SvArgs a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ f4 s_rec[GHR_SV_REC_UNITS * GHR_SV_CHUNK];
    __shared__ uint32_t s_id[GHR_SV_CHUNK];
    const int i = (int)blockIdx.y * GHR_SV_TILE + (int)threadIdx.x / GHR_SV_TILE;
    const int j = (int)blockIdx.x * GHR_SV_TILE + (int)threadIdx.x % GHR_SV_TILE;
    const bool in_image = i < a.H && j < a.W;
    const float px = (float)j + 0.5f, py = (float)i + 0.5f;
    float best_q = 0.f, best_t = 0.f;
    int32_t best_k = -1;
    // tl_walk's loop, written out: through the shared walk this kernel measured 0.6 - 1 % slower per frame (profiles/strand_preview.txt)
    const TileLists& tl = a.tl;
    const uint32_t tile = blockIdx.y * (uint32_t)tl.tiles_x + blockIdx.x;
    const uint32_t beg = tl.start[tile], n_own = tl.start[tile + 1] - beg;
    const uint32_t n_big = tl.n_prims > 0u ? min(*tl.nbig, tl.n_prims) : 0u;
    const uint32_t n = n_own + n_big;  // (workgroup-uniform)
    for (uint32_t c0 = 0u; c0 < n; c0 += GHR_SV_CHUNK) {
        const uint32_t m = min((uint32_t)GHR_SV_CHUNK, n - c0);
        if (threadIdx.x < 2u * m) {
            const uint32_t k = threadIdx.x / 2u, part = threadIdx.x % 2u, e = c0 + k;
            uint32_t id = e < n_own ? tl.list[min(beg + e, tl.list_cap - 1u)] : tl.big[e - n_own];  // (tl_walk's clamps)
            id = min(id, tl.n_prims - 1u);
            s_rec[2u * k + part] = reinterpret_cast<const f4*>(tl.rec)[2 * (size_t)id + part];
            if (part == 0u) s_id[k] = id;
        }
        __syncthreads();
        for (uint32_t k = 0u; k < m; k++) {
            const f4 r0 = s_rec[2u * k], r1 = s_rec[2u * k + 1u];  // (one address per wave: broadcast)
            const float r[GHR_SV_REC_WORDS] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
            const bool box = in_image && sv_in_box(r, a.r, px, py);
            if (__builtin_amdgcn_ballot_w64(box) == 0ull) continue;  // nobody in this wave is inside the widened box
            float t, q;
            if (box && sv_covers(r, a.r, px, py, &t, &q)) sv_take(q, t, (int32_t)s_id[k], &best_q, &best_t, &best_k);
        }
        __syncthreads();
    }
    if (!in_image) return;
    const size_t o = (size_t)i * a.W + j;
    const int32_t face = a.pix_to_face ? a.pix_to_face[o] : -1;
    const float qf = a.pix_to_face ? a.qf[o] : 0.f;
    int32_t seg, face_out;
    float t, d;
    sv_resolve_head(best_k, best_t, best_q, face, qf, a.head_bias, &seg, &t, &face_out, &d);
    a.pix_to_segment[o] = seg;
    a.t[o] = t;
    a.pix_to_face_out[o] = face_out;
    a.inv_depth[o] = d;
#endif
}

// The light pass's raster: a (H, W, r, the tables) is the light view's; pix_to_face, qf and the four planes of a are not used.
struct SvLayersArgs {
    SvArgs a;
    float layer;
    float* q0;         // [H][W]
    uint32_t* layers;  // [H][W][4], 16-B aligned
};
typedef uint32_t sv_u4 __attribute__((ext_vector_type(4)));

// One tile per workgroup, one texel per thread; the tile's lists are walked twice: the front plane, then the counts behind it.
__global__ void __launch_bounds__(GHR_SV_BLOCK) k_sv_layers(SvLayersArgs la)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ f4 s_rec[GHR_SV_REC_UNITS * GHR_SV_CHUNK];
    const SvArgs& a = la.a;
    const uint32_t tile = blockIdx.y * (uint32_t)a.tl.tiles_x + blockIdx.x;
    const int i = (int)blockIdx.y * GHR_SV_TILE + (int)threadIdx.x / GHR_SV_TILE;
    const int j = (int)blockIdx.x * GHR_SV_TILE + (int)threadIdx.x % GHR_SV_TILE;
    const bool in_image = i < a.H && j < a.W;
    const float px = (float)j + 0.5f, py = (float)i + 0.5f;
    const auto in_box = [&](const float* r) { return in_image && sv_in_box(r, a.r, px, py); };
    float best_q = 0.f;
    tl_walk<GHR_SV_REC_UNITS, GHR_SV_CHUNK, false>(a.tl, tile, s_rec, nullptr, in_box, [&](const float* r, uint32_t) {
        float t, q;
        if (sv_covers(r, a.r, px, py, &t, &q) && q > best_q) best_q = q;  // (a NaN or a q that is not > 0 never gets in)
    });
    const float inv_q0 = 1.f / best_q;  // (read only behind a covering segment with qs > 0: then best_q > 0)
    uint32_t n0 = 0u, n1 = 0u, n2 = 0u, n3 = 0u;
    tl_walk<GHR_SV_REC_UNITS, GHR_SV_CHUNK, false>(a.tl, tile, s_rec, nullptr, in_box, [&](const float* r, uint32_t) {
        float t, q;
        if (!(sv_covers(r, a.r, px, py, &t, &q) && q > 0.f)) return;
        const int layer = sv_layer_of(1.f / q - inv_q0, la.layer);
        n0 += layer == 0 ? 1u : 0u; n1 += layer == 1 ? 1u : 0u; n2 += layer == 2 ? 1u : 0u; n3 += layer == 3 ? 1u : 0u;
    });
    if (!in_image) return;
    const size_t o = (size_t)i * a.W + j;
    la.q0[o] = best_q;
    reinterpret_cast<sv_u4*>(la.layers)[o] = sv_u4{n0, n1, n2, n3};
#endif
}

struct SvFaceDepthArgs {
    int32_t V, F, H, W;
    float near;
    float M[12];
    const float* vertices;
    const int32_t* faces;
    const int32_t* pix_to_face;
    float* qf;
};

__global__ void __launch_bounds__(GHR_SV_BLOCK) k_sv_face_depth(SvFaceDepthArgs a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t o = blockIdx.x * GHR_SV_BLOCK + threadIdx.x;
    if (o >= (uint32_t)a.H * (uint32_t)a.W) return;
    const int i = (int)(o / (uint32_t)a.W), j = (int)(o % (uint32_t)a.W);
    a.qf[o] = sv_face_depth_one(a.M, a.near, a.vertices, a.V, a.faces, a.F, a.pix_to_face[o], (float)j + 0.5f, (float)i + 0.5f);
#endif
}

struct SvShadeArgs {
    int32_t S, L, V, F, H, W, mode;
    SvShading sh;
    const float* points;
    const float* vertices;
    const int32_t* faces;
    const float* base;  // [S][3] or NULL: sh.base_rgb
    const int32_t* pix_to_segment;
    const int32_t* pix_to_face_out;
    uint8_t* rgb;       // [H][W][3]
};

__global__ void __launch_bounds__(GHR_SV_BLOCK) k_sv_shade(SvShadeArgs a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t o = blockIdx.x * GHR_SV_BLOCK + threadIdx.x;
    if (o >= (uint32_t)a.H * (uint32_t)a.W) return;
    uint8_t rgb[3];
    sv_shade_one(a.pix_to_segment[o], a.pix_to_face_out[o], a.S, a.L, a.points, a.V, a.vertices, a.F, a.faces, a.base, a.mode, a.sh,
                 rgb);
    a.rgb[3 * (size_t)o] = rgb[0]; a.rgb[3 * (size_t)o + 1] = rgb[1]; a.rgb[3 * (size_t)o + 2] = rgb[2];
#endif
}

struct SvShadeShadowedArgs {
    SvShadeArgs a;
    const float* t;  // [H][W]: the raster's t plane
    SvShadow sd;
};

__global__ void __launch_bounds__(GHR_SV_BLOCK) k_sv_shade_shadowed(SvShadeShadowedArgs sa)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const SvShadeArgs& a = sa.a;
    const uint32_t o = blockIdx.x * GHR_SV_BLOCK + threadIdx.x;
    if (o >= (uint32_t)a.H * (uint32_t)a.W) return;
    uint8_t rgb[3];
    sv_shade_one_shadowed(a.pix_to_segment[o], a.pix_to_face_out[o], sa.t[o], a.S, a.L, a.points, a.V, a.vertices, a.F, a.faces, a.base,
                          a.mode, a.sh, sa.sd, rgb);
    a.rgb[3 * (size_t)o] = rgb[0]; a.rgb[3 * (size_t)o + 1] = rgb[1]; a.rgb[3 * (size_t)o + 2] = rgb[2];
#endif
}

struct SvResolveArgs {
    int32_t H, W, s;
    const uint8_t* src;
    uint8_t* dst;
};

__global__ void __launch_bounds__(GHR_SV_BLOCK) k_sv_resolve(SvResolveArgs a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t o = blockIdx.x * GHR_SV_BLOCK + threadIdx.x;
    if (o >= (uint32_t)a.H * (uint32_t)a.W) return;
    sv_resolve_one(a.src, a.W, a.s, (int)(o / (uint32_t)a.W), (int)(o % (uint32_t)a.W), a.dst);
#endif
}
#endif  // __HIPCC__

}  // namespace ghr
