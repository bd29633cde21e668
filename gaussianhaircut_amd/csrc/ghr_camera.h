// ghr_camera.h -- the camera bank: every trainable camera of a scene as one row of flat device buffers.
//
// Reference: src/scene/cameras.py:83-154 (a camera's five tensors as functions of per-camera residuals, rebuilt by ~40 PyTorch
// launches per view with autograd), src/utils/camera_opt_utils.py:84-141 (BARF's se(3) exponential, the default), src/train_gaussians.py:
// 45-66,183-196 (a torch.optim.Adam of their own, stepped after the Gaussians').  That is ~100 floats of arithmetic per camera:
// here one thread composes a camera (k_cam_compose), one thread back-propagates the six cotangents to its residuals by a hand-
// derived VJP (k_cam_compose_bwd), and one workgroup steps every camera that was viewed (k_cam_adam).
//
// Rows (floats):
//   constants  GHR_CAM_CONST = 21: W2C[16] row-major (getWorld2View2, cameras.py:72) | FoVx0 | FoVy0 | znear | P[2][2] | P[2][3]
//              (the two constant entries of getProjectionMatrix, graphics_utils.py:69-70, rounded to fp32 by the host as torch does)
//   parameters rot[6 | 3] | translation[3] | fov[2]          (ortho-6D: 11 floats; se(3): 8)
//   output     GHR_CAM_OUT = 53: view[16] | full[16] | proj[16] | centre[3] | FoVx | FoVy     (view, full, proj as the reference's
//              TRANSPOSED row-vector matrices: view = (W2C @ residual)^T, proj = getProjectionMatrix^T, full = view @ proj)
// Everything is fp32 in the reference's operation order where that order is stated; the 3x3 / 4x4 work is fully unrolled over
// constant indices (no private segment: tests/test_kernel_resources.py).
#pragma once
#include "ghr_adam.h"
#include "ghr_device.h"

namespace ghr {

#define GHR_CAM_ORTHO6D 0
#define GHR_CAM_SE3 1
#define GHR_CAM_CONST 21
#define GHR_CAM_OUT 53
#define GHR_CAM_TRAIN_POSE 1  // train_mask bits: rotation + translation (trainable_cameras), FoV (trainable_intrinsics)
#define GHR_CAM_TRAIN_FOV 2
#ifdef GHR_CAMERA_CONST  // include/ghr.h states the same numbers for the callers
static_assert(GHR_CAMERA_CONST == GHR_CAM_CONST && GHR_CAMERA_OUT == GHR_CAM_OUT && GHR_CAMERA_SE3 == GHR_CAM_SE3 &&
              GHR_CAMERA_ORTHO6D == GHR_CAM_ORTHO6D && GHR_CAMERA_TRAIN_POSE == GHR_CAM_TRAIN_POSE &&
              GHR_CAMERA_TRAIN_FOV == GHR_CAM_TRAIN_FOV, "camera bank constants of include/ghr.h");
#endif

GHR_HD int cam_rot_dim(int param) { return param == GHR_CAM_SE3 ? 3 : 6; }
GHR_HD int cam_row(int param) { return cam_rot_dim(param) + 5; }

struct CamV3 { float x, y, z; };
GHR_HD float cam_dot(const CamV3& a, const CamV3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
GHR_HD CamV3 cam_cross(const CamV3& a, const CamV3& b) { return CamV3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
GHR_HD CamV3 cam_scale(const CamV3& a, float s) { return CamV3{a.x * s, a.y * s, a.z * s}; }
GHR_HD CamV3 cam_add(const CamV3& a, const CamV3& b) { return CamV3{a.x + b.x, a.y + b.y, a.z + b.z}; }
GHR_HD CamV3 cam_sub(const CamV3& a, const CamV3& b) { return CamV3{a.x - b.x, a.y - b.y, a.z - b.z}; }

// The residual transform's 3x4 top: rotation r[3][3] (row-major) and translation t.
struct CamResidual { float r[9]; CamV3 t; };

// ---- ortho-6D (cameras.py:116-120,170-196): Gram-Schmidt of two raw 3-vectors, z = x cross y, COLUMNS (x, y, z) -------------
struct CamOrtho {
    CamV3 x, y, yraw;   // the orthonormal pair and the raw second vector
    float nx, nu;       // max(|x_raw|, 1e-12), max(|u|, 1e-12): the two normalisations' divisors
    bool ux, uu;        // ... and whether the norm itself was the divisor (F.normalize clamps it from below)
    float a, d, xx;     // <x, y_raw>, clamp(<x, x>, 1e-8) + 1e-10, <x, x>
};

GHR_HD CamOrtho cam_ortho_fwd(const float* rot, CamResidual& R)
{
    CamOrtho o;
    const CamV3 xr{rot[0], rot[1], rot[2]};
    o.yraw = CamV3{rot[3], rot[4], rot[5]};
    const float n0 = sqrtf(cam_dot(xr, xr));
    o.ux = n0 > 1e-12f;
    o.nx = o.ux ? n0 : 1e-12f;
    o.x = CamV3{xr.x / o.nx, xr.y / o.nx, xr.z / o.nx};
    o.a = cam_dot(o.x, o.yraw);
    o.xx = cam_dot(o.x, o.x);
    o.d = (o.xx < 1e-8f ? 1e-8f : o.xx) + 1e-10f;
    const float f = o.a / o.d;
    const CamV3 u = cam_sub(o.yraw, cam_scale(o.x, f));
    const float n1 = sqrtf(cam_dot(u, u));
    o.uu = n1 > 1e-12f;
    o.nu = o.uu ? n1 : 1e-12f;
    o.y = CamV3{u.x / o.nu, u.y / o.nu, u.z / o.nu};
    const CamV3 z = cam_cross(o.x, o.y);
    R.r[0] = o.x.x; R.r[1] = o.y.x; R.r[2] = z.x;
    R.r[3] = o.x.y; R.r[4] = o.y.y; R.r[5] = z.y;
    R.r[6] = o.x.z; R.r[7] = o.y.z; R.r[8] = z.z;
    return o;
}

// gR: cotangent of the rotation (row-major) -> cotangent of the six raw floats
GHR_HD void cam_ortho_bwd(const CamOrtho& o, const float* gR, float* g_rot)
{
    CamV3 gx{gR[0], gR[3], gR[6]}, gy{gR[1], gR[4], gR[7]};
    const CamV3 gz{gR[2], gR[5], gR[8]};
    gx = cam_add(gx, cam_cross(o.y, gz));   // z = x cross y
    gy = cam_add(gy, cam_cross(gz, o.x));
    // y = u / max(|u|, eps)
    CamV3 gu = o.uu ? cam_sub(gy, cam_scale(o.y, cam_dot(o.y, gy))) : gy;
    gu = CamV3{gu.x / o.nu, gu.y / o.nu, gu.z / o.nu};
    // u = y_raw - f x,  f = a / d
    const float f = o.a / o.d;
    CamV3 gyr = gu;
    gx = cam_sub(gx, cam_scale(gu, f));
    const float gf = -cam_dot(o.x, gu);
    const float ga = gf / o.d, gd = -gf * o.a / (o.d * o.d);
    gyr = cam_add(gyr, cam_scale(o.x, ga));
    gx = cam_add(gx, cam_scale(o.yraw, ga));
    if (o.xx >= 1e-8f) gx = cam_add(gx, cam_scale(o.x, 2.f * gd));   // (clamp passes its gradient where it does not bind)
    // x = x_raw / max(|x_raw|, eps)
    CamV3 gxr = o.ux ? cam_sub(gx, cam_scale(o.x, cam_dot(o.x, gx))) : gx;
    gxr = CamV3{gxr.x / o.nx, gxr.y / o.nx, gxr.z / o.nx};
    g_rot[0] = gxr.x; g_rot[1] = gxr.y; g_rot[2] = gxr.z;
    g_rot[3] = gyr.x; g_rot[4] = gyr.y; g_rot[5] = gyr.z;
}

// ---- se(3) (cameras.py:110-114, camera_opt_utils.py:84-141) ------------------------------------------------------------------
// A = sin(t) / t, B = (1 - cos t) / t^2, C = (t - sin t) / t^3 as the reference's 11-term series (nth = 10), which are polynomials
// in s = t^2 = w . w: evaluated in s, no square root, so value and gradient are finite at w = 0 -- where every camera starts.
// K = 1, 2, 3 selects A, B, C: term i is (-1)^i s^i / denom_i with denom_i the running product of camera_opt_utils.py:118-141
// (the loop unrolls and the denominators fold to constants).  Returns the value, *ds = d/ds.
template <int K>
GHR_HD float cam_series(float s, float* ds)
{
    float ans = 0.f, der = 0.f, pw = 1.f, pw1 = 0.f;   // s^i and s^(i-1)
    double denom = 1.0;
#pragma unroll
    for (int i = 0; i <= 10; i++) {
        if (K == 1) { if (i > 0) denom *= (double)((2 * i) * (2 * i + 1)); }
        else if (K == 2) denom *= (double)((2 * i + 1) * (2 * i + 2));
        else denom *= (double)((2 * i + 2) * (2 * i + 3));
        const float sign = (i & 1) ? -1.f : 1.f, dn = (float)denom;
        ans = ans + sign * pw / dn;
        der = der + sign * ((float)i * pw1) / dn;
        pw1 = pw;
        pw = pw * s;
    }
    *ds = der;
    return ans;
}

struct CamSe3 {
    float wx[9], w2[9];   // [w]x and its square
    float A, B, C, dA, dB, dC;
    CamV3 w, u;
    float V[9];
};

GHR_HD void cam_mul3(const float* a, const float* b, float* c)
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

GHR_HD CamSe3 cam_se3_fwd(const float* rot, const float* trans, CamResidual& R)
{
    CamSe3 e;
    e.w = CamV3{rot[0], rot[1], rot[2]};
    e.u = CamV3{trans[0], trans[1], trans[2]};
    e.wx[0] = 0.f;    e.wx[1] = -e.w.z; e.wx[2] = e.w.y;
    e.wx[3] = e.w.z;  e.wx[4] = 0.f;    e.wx[5] = -e.w.x;
    e.wx[6] = -e.w.y; e.wx[7] = e.w.x;  e.wx[8] = 0.f;
    cam_mul3(e.wx, e.wx, e.w2);
    const float s = cam_dot(e.w, e.w);
    e.A = cam_series<1>(s, &e.dA);
    e.B = cam_series<2>(s, &e.dB);
    e.C = cam_series<3>(s, &e.dC);
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const float I = (k == 0 || k == 4 || k == 8) ? 1.f : 0.f;
        R.r[k] = I + e.A * e.wx[k] + e.B * e.w2[k];
        e.V[k] = I + e.B * e.wx[k] + e.C * e.w2[k];
    }
    R.t = CamV3{e.V[0] * e.u.x + e.V[1] * e.u.y + e.V[2] * e.u.z, e.V[3] * e.u.x + e.V[4] * e.u.y + e.V[5] * e.u.z,
                e.V[6] * e.u.x + e.V[7] * e.u.y + e.V[8] * e.u.z};
    return e;
}

// gR, gt: cotangents of the residual's rotation and translation column -> cotangents of w and u
GHR_HD void cam_se3_bwd(const CamSe3& e, const float* gR, const CamV3& gt, float* g_w, float* g_u)
{
    // t = V u
    g_u[0] = e.V[0] * gt.x + e.V[3] * gt.y + e.V[6] * gt.z;
    g_u[1] = e.V[1] * gt.x + e.V[4] * gt.y + e.V[7] * gt.z;
    g_u[2] = e.V[2] * gt.x + e.V[5] * gt.y + e.V[8] * gt.z;
    const float gV[9] = {gt.x * e.u.x, gt.x * e.u.y, gt.x * e.u.z, gt.y * e.u.x, gt.y * e.u.y, gt.y * e.u.z,
                         gt.z * e.u.x, gt.z * e.u.y, gt.z * e.u.z};
    float gA = 0.f, gB = 0.f, gC = 0.f, gwx[9], gw2[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
        gA += gR[k] * e.wx[k];
        gB += gR[k] * e.w2[k] + gV[k] * e.wx[k];
        gC += gV[k] * e.w2[k];
        gwx[k] = e.A * gR[k] + e.B * gV[k];
        gw2[k] = e.B * gR[k] + e.C * gV[k];
    }
    // w2 = wx wx:  g wx += g w2 wx^T + wx^T g w2
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 3; k++) acc += gw2[3 * i + k] * e.wx[3 * j + k] + e.wx[3 * k + i] * gw2[3 * k + j];
            gwx[3 * i + j] += acc;
        }
    const float gs = gA * e.dA + gB * e.dB + gC * e.dC;   // s = w . w
    g_w[0] = (gwx[7] - gwx[5]) + 2.f * e.w.x * gs;
    g_w[1] = (gwx[2] - gwx[6]) + 2.f * e.w.y * gs;
    g_w[2] = (gwx[3] - gwx[1]) + 2.f * e.w.z * gs;
}

// ---- the camera's matrices from the residual transform -------------------------------------------------------------------------
// view[j][i] = M[i][j], M = W2C @ [[r, t], [0 0 0 1]]
GHR_HD void cam_view(const float* c, const CamResidual& R, float* view)
{
    const float tt[3] = {R.t.x, R.t.y, R.t.z};
#pragma unroll
    for (int i = 0; i < 4; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) view[4 * j + i] = c[4 * i] * R.r[j] + c[4 * i + 1] * R.r[3 + j] + c[4 * i + 2] * R.r[6 + j];
        view[12 + i] = c[4 * i] * tt[0] + c[4 * i + 1] * tt[1] + c[4 * i + 2] * tt[2] + c[4 * i + 3];
    }
}

// 1 / tan(FoV / 2) the way getProjectionMatrix spells it (graphics_utils.py:52-65): 2 n / (right - left), right = tan * n
GHR_HD float cam_inv_tan(float fov, float znear, float* tan_half)
{
    const float t = tanf(fov / 2.f);
    const float right = t * znear;
    *tan_half = t;
    return 2.0f * znear / (right - (-right));
}

// One camera, forward.  cst: its constants row, par: its parameter row, out: its output row (GHR_CAM_OUT floats).
GHR_HD void cam_compose_row(int param, const float* cst, const float* par, float* out)
{
    const int rd = cam_rot_dim(param);
    CamResidual R;
    if (param == GHR_CAM_SE3) {
        cam_se3_fwd(par, par + rd, R);
    } else {
        cam_ortho_fwd(par, R);
        R.t = CamV3{par[rd], par[rd + 1], par[rd + 2]};
    }
    float c[16], view[16];
#pragma unroll
    for (int k = 0; k < 16; k++) c[k] = cst[k];
    cam_view(c, R, view);
    const float fovx = cst[16] + par[rd + 3], fovy = cst[17] + par[rd + 4];
    const float znear = cst[18], p22 = cst[19], p32 = cst[20];
    float tx, ty;
    const float p00 = cam_inv_tan(fovx, znear, &tx), p11 = cam_inv_tan(fovy, znear, &ty);
#pragma unroll
    for (int k = 0; k < 16; k++) out[k] = view[k];
#pragma unroll
    for (int r = 0; r < 4; r++) {   // full = view @ proj
        out[16 + 4 * r] = view[4 * r] * p00;
        out[16 + 4 * r + 1] = view[4 * r + 1] * p11;
        out[16 + 4 * r + 2] = view[4 * r + 2] * p22 + view[4 * r + 3] * p32;
        out[16 + 4 * r + 3] = view[4 * r + 2];
    }
#pragma unroll
    for (int k = 0; k < 16; k++) out[32 + k] = 0.f;
    out[32] = p00; out[32 + 5] = p11; out[32 + 10] = p22; out[32 + 11] = 1.f; out[32 + 14] = p32;
    // camera centre: inverse(view)[3, :3] of a rigid transform = -t R^T (cameras.py:150 inverts the 4x4)
#pragma unroll
    for (int i = 0; i < 3; i++)
        out[48 + i] = -(view[12] * view[4 * i] + view[13] * view[4 * i + 1] + view[14] * view[4 * i + 2]);
    out[51] = fovx;
    out[52] = fovy;
}

// One camera, backward.  d_*: the cotangents of its six outputs (each may be NULL), g: GHR row of cam_row(param) floats that
// RECEIVES dL/d(rotation_res | translation_res | fov_res) (assigned, every entry).
GHR_HD void cam_compose_bwd_row(int param, const float* cst, const float* par, const float* d_view, const float* d_full,
                                const float* d_proj, const float* d_center, const float* d_fovx, const float* d_fovy, float* g)
{
    const int rd = cam_rot_dim(param);
    CamResidual R;
    CamOrtho o;
    CamSe3 e;
    if (param == GHR_CAM_SE3) {
        e = cam_se3_fwd(par, par + rd, R);
    } else {
        o = cam_ortho_fwd(par, R);
        R.t = CamV3{par[rd], par[rd + 1], par[rd + 2]};
    }
    float c[16], view[16], gv[16];
#pragma unroll
    for (int k = 0; k < 16; k++) c[k] = cst[k];
    cam_view(c, R, view);
    const float fovx = cst[16] + par[rd + 3], fovy = cst[17] + par[rd + 4];
    const float znear = cst[18], p22 = cst[19], p32 = cst[20];
    float tx, ty;
    const float p00 = cam_inv_tan(fovx, znear, &tx), p11 = cam_inv_tan(fovy, znear, &ty);
    float gp00 = 0.f, gp11 = 0.f;
#pragma unroll
    for (int k = 0; k < 16; k++) gv[k] = d_view ? d_view[k] : 0.f;
    if (d_proj) { gp00 = d_proj[0]; gp11 = d_proj[5]; }
    if (d_full) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float f0 = d_full[4 * r], f1 = d_full[4 * r + 1], f2 = d_full[4 * r + 2], f3 = d_full[4 * r + 3];
            gp00 += view[4 * r] * f0;
            gp11 += view[4 * r + 1] * f1;
            gv[4 * r] += f0 * p00;
            gv[4 * r + 1] += f1 * p11;
            gv[4 * r + 2] += f2 * p22 + f3;
            gv[4 * r + 3] += f2 * p32;
        }
    }
    if (d_center) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const float dc = d_center[i];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                gv[12 + j] -= dc * view[4 * i + j];
                gv[4 * i + j] -= dc * view[12 + j];
            }
        }
    }
    // P[0][0] = 1 / tan(FoVx / 2):  d / dFoVx = -(1 + tan^2) / (2 tan^2)
    g[rd + 3] = (d_fovx ? d_fovx[0] : 0.f) - gp00 * (0.5f * (1.f + tx * tx) / (tx * tx));
    g[rd + 4] = (d_fovy ? d_fovy[0] : 0.f) - gp11 * (0.5f * (1.f + ty * ty) / (ty * ty));
    // view = M^T, M = W2C @ residual:  g residual = W2C^T gM, gM[i][j] = gv[j][i]
    float gR[9], gt[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int j = 0; j < 3; j++)
            gR[3 * k + j] = c[k] * gv[4 * j] + c[4 + k] * gv[4 * j + 1] + c[8 + k] * gv[4 * j + 2] + c[12 + k] * gv[4 * j + 3];
        gt[k] = c[k] * gv[12] + c[4 + k] * gv[13] + c[8 + k] * gv[14] + c[12 + k] * gv[15];
    }
    if (param == GHR_CAM_SE3) {
        cam_se3_bwd(e, gR, CamV3{gt[0], gt[1], gt[2]}, g, g + rd);
    } else {
        cam_ortho_bwd(o, gR, g);
        g[rd] = gt[0]; g[rd + 1] = gt[1]; g[rd + 2] = gt[2];
    }
}

// One camera's Adam update (torch.optim.Adam, eps 1e-15, this camera's own step number `step` >= 1: torch counts steps per
// parameter and passes a parameter without .grad by).  lr: rotation, translation, fov.  Groups outside train_mask stay.
GHR_HD void cam_adam_row(int param, float* p, const float* g, float* m, float* v, int step, float lr_rot, float lr_trans,
                         float lr_fov, double beta1, double beta2, float eps, int train_mask)
{
    const int rd = cam_rot_dim(param);
    const double bias1 = 1.0 - pow(beta1, (double)step);
    const float b2s = (float)sqrt(1.0 - pow(beta2, (double)step));
    const float w1 = (float)(1.0 - beta1), w2 = (float)(1.0 - beta2), b2 = (float)beta2;
    const float ss_rot = (float)((double)lr_rot / bias1), ss_trans = (float)((double)lr_trans / bias1),
                ss_fov = (float)((double)lr_fov / bias1);
    const int W = rd + 5;
    for (int k = 0; k < W; k++) {
        const bool fov = k >= rd + 3;
        if (!(train_mask & (fov ? GHR_CAM_TRAIN_FOV : GHR_CAM_TRAIN_POSE))) continue;
        float pp = p[k], mm = m[k], vv = v[k];
        adam_update(pp, g[k], mm, vv, fov ? ss_fov : (k < rd ? ss_rot : ss_trans), w1, b2, w2, eps, b2s);
        p[k] = pp; m[k] = mm; v[k] = vv;
    }
}

// ---- kernels -------------------------------------------------------------------------------------------------------------------
struct CamArgs {
    int param, first, n;      // parametrisation; rows [first, first + n) of the bank
    const float* cst; int cst_stride;
    const float* par; int par_stride;
};

// One thread per camera of the range; out row r of the RANGE (r = 0 .. n-1) at out + r * out_stride.
__global__ void __launch_bounds__(64) k_cam_compose(CamArgs a, float* __restrict__ out, int out_stride)
{
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= a.n) return;
    const size_t row = (size_t)(a.first + r);
    if (a.param == GHR_CAM_SE3) cam_compose_row(GHR_CAM_SE3, a.cst + row * a.cst_stride, a.par + row * a.par_stride, out + (size_t)r * out_stride);
    else cam_compose_row(GHR_CAM_ORTHO6D, a.cst + row * a.cst_stride, a.par + row * a.par_stride, out + (size_t)r * out_stride);
}

struct CamCotangents {   // dense per row of the range: [n][16], [n][16], [n][16], [n][3], [n], [n]; each may be NULL
    const float* d_view; const float* d_full; const float* d_proj; const float* d_center; const float* d_fovx; const float* d_fovy;
};

// One thread per camera of the range: the residual gradients are ASSIGNED to a row whose touched mark is down (whatever it held --
// a stale NaN included -- is gone) and ADDED to a row that was touched since the last k_cam_adam; the mark goes up.  Groups outside
// train_mask are left alone.  Rows are owned by one thread: concurrent launches must cover disjoint rows.
template <int PARAM>
__device__ __forceinline__ void cam_bwd_thread(const CamArgs& a, const CamCotangents& d, float* grads, int grad_stride, int* touched,
                                   int train_mask, int r)
{
    const size_t row = (size_t)(a.first + r);
    constexpr int RD = PARAM == GHR_CAM_SE3 ? 3 : 6, W = RD + 5;
    float g[W];
    cam_compose_bwd_row(PARAM, a.cst + row * a.cst_stride, a.par + row * a.par_stride, d.d_view ? d.d_view + 16 * (size_t)r : nullptr,
                        d.d_full ? d.d_full + 16 * (size_t)r : nullptr, d.d_proj ? d.d_proj + 16 * (size_t)r : nullptr,
                        d.d_center ? d.d_center + 3 * (size_t)r : nullptr, d.d_fovx ? d.d_fovx + r : nullptr,
                        d.d_fovy ? d.d_fovy + r : nullptr, g);
    float* dst = grads + row * grad_stride;
    const bool add = touched[row] != 0;
#pragma unroll
    for (int k = 0; k < W; k++) {
        const bool on = (train_mask & (k >= RD + 3 ? GHR_CAM_TRAIN_FOV : GHR_CAM_TRAIN_POSE)) != 0;
        if (on) dst[k] = add ? dst[k] + g[k] : g[k];
        else if (!add) dst[k] = 0.f;
    }
    touched[row] = 1;
}

__global__ void __launch_bounds__(64) k_cam_compose_bwd(CamArgs a, CamCotangents d, float* __restrict__ grads, int grad_stride,
                                                        int* __restrict__ touched, int train_mask)
{
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= a.n) return;
    if (a.param == GHR_CAM_SE3) cam_bwd_thread<GHR_CAM_SE3>(a, d, grads, grad_stride, touched, train_mask, r);
    else cam_bwd_thread<GHR_CAM_ORTHO6D>(a, d, grads, grad_stride, touched, train_mask, r);
}

// ONE workgroup over all N rows (a scene has tens to a few hundred cameras), a thread per row in turns.  The reference's rule
// (train_gaussians.py:190-196) is all or nothing: a NaN (isnan, not isinf) in any gradient of a camera that was viewed skips the
// whole step -- nothing moves, no step count advances.  With one workgroup that decision is a barrier, not a grid-wide flag.
// Either way the touched rows' gradients and marks are cleared; untouched rows are neither read nor written.
#define GHR_CAM_ADAM_THREADS 256
__global__ void __launch_bounds__(GHR_CAM_ADAM_THREADS) k_cam_adam(int param, int n, float* __restrict__ p, float* __restrict__ g,
                                                                   float* __restrict__ m, float* __restrict__ v, int stride,
                                                                   int* __restrict__ steps, int* __restrict__ touched, float lr_rot,
                                                                   float lr_trans, float lr_fov, double beta1, double beta2, float eps,
                                                                   int train_mask)
{
    const int W = cam_row(param), rd = cam_rot_dim(param);
    int bad = 0;
    for (int r = threadIdx.x; r < n; r += GHR_CAM_ADAM_THREADS) {
        if (!touched[r]) continue;
        const float* gr = g + (size_t)r * stride;
        for (int k = 0; k < W; k++) {
            const bool on = (train_mask & (k >= rd + 3 ? GHR_CAM_TRAIN_FOV : GHR_CAM_TRAIN_POSE)) != 0;
            const float x = gr[k];
            bad |= (on && x != x) ? 1 : 0;
        }
    }
    bad = __syncthreads_or(bad);
    for (int r = threadIdx.x; r < n; r += GHR_CAM_ADAM_THREADS) {
        if (!touched[r]) continue;
        const size_t o = (size_t)r * stride;
        if (!bad) {
            const int step = steps[r] + 1;
            steps[r] = step;
            cam_adam_row(param, p + o, g + o, m + o, v + o, step, lr_rot, lr_trans, lr_fov, beta1, beta2, eps, train_mask);
        }
        for (int k = 0; k < W; k++) g[o + k] = 0.f;
        touched[r] = 0;
    }
}

// ---- a replicated bank: the gradient rows of G ranks (scene.cameras.CameraBank.exchange_gradients) ---------------------------------
// One thread per (row, column) of the message [n][W + 1]: a touched row travels as its W gradient floats and 1.0f, an untouched one
// as zeros -- what its gradient row holds (a stale NaN: the backward kernel ASSIGNS to an untouched row, nobody clears it before)
// is not read.
#define GHR_CAM_XCHG_THREADS 256
__global__ void __launch_bounds__(GHR_CAM_XCHG_THREADS) k_cam_pack(int n, int W, const float* __restrict__ g, int stride,
                                                                   const int* __restrict__ touched, float* __restrict__ msg)
{
    const size_t i = (size_t)blockIdx.x * GHR_CAM_XCHG_THREADS + threadIdx.x;
    if (i >= (size_t)n * (size_t)(W + 1)) return;
    const int r = (int)(i / (size_t)(W + 1)), k = (int)(i % (size_t)(W + 1));
    float x = 0.f;
    if (touched[r]) x = k < W ? g[(size_t)r * stride + k] : 1.f;
    msg[i] = x;
}

// One thread per (row, column) of the gradient rows; `all` [G][n][W + 1] holds the ranks' messages in rank order.  The first rank
// that touched the row assigns, the later ones add, in ascending rank order: every rank computes the same bits, and a row that one
// rank alone touched keeps that rank's.  A row nobody touched is left exactly as it is (gradient row and mark).
__global__ void __launch_bounds__(GHR_CAM_XCHG_THREADS) k_cam_merge(int n, int W, int G, const float* __restrict__ all,
                                                                    float* __restrict__ g, int stride, int* __restrict__ touched)
{
    const size_t i = (size_t)blockIdx.x * GHR_CAM_XCHG_THREADS + threadIdx.x;
    if (i >= (size_t)n * (size_t)W) return;
    const int r = (int)(i / (size_t)W), k = (int)(i % (size_t)W);
    const size_t row = (size_t)r * (size_t)(W + 1), rank = (size_t)n * (size_t)(W + 1);
    bool any = false;
    float acc = 0.f;
    for (int q = 0; q < G; q++) {
        const float* m = all + (size_t)q * rank + row;
        if (m[W] == 0.f) continue;
        acc = any ? acc + m[k] : m[k];
        any = true;
    }
    if (!any) return;
    g[(size_t)r * stride + k] = acc;
    if (k == 0) touched[r] = 1;
}

}  // namespace ghr
