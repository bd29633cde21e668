// ghr_compare.h -- the comparison video's frame assembly: the strand render over white and the three-panel strip.
//
// Reference: src/postprocessing/concat_video.py:26-40 -- Image.new("RGBA", size, "WHITE").paste(im, (0, 0), im).convert("RGB") for
// the strand render, torchvision's Resize / CenterCrop for the panels and np.concatenate for the strip.  The two resizes before
// the strip and the one after it are ghr_resample_u8 (ghr_gt.h); what is left is here.
//
//   k_cmp_over_white  Pillow's paste of an RGBA image over opaque white through its own alpha, per colour byte c with alpha a:
//                     t = c a + 255 (255 - a) + 128, out = ((t >> 8) + t) >> 8 (Pillow's MULDIV255 of both terms, added before the
//                     division).  Four pixels per thread: one 16-B load, three dwords stored.
//   k_cmp_strip       the strip [h][3 w][3] = photograph | preview | render in one launch: the outer panels are copies, the middle
//                     one is the h x w window of the resized preview [ph][pw][3] after CenterCrop's padding with black
// Integer arithmetic alone: no floating point, no atomics, no LDS; the same bytes run after run.  Each per-pixel rule is one
// __host__ __device__ function, read beside gaussianhaircut_amd/comparison.py's torch expression of it.
#pragma once
#include "ghr_device.h"

namespace ghr {

// ---- over white ------------------------------------------------------------------------------------------------------------------

// one colour byte over white: 0 <= t <= 255 * 255 + 128, so ((t >> 8) + t) >> 8 is the rounded t / 255
GHR_HD uint8_t cmp_over_white(uint32_t c, uint32_t a)
{
    const uint32_t t = c * a + 255u * (255u - a) + 128u;
    return (uint8_t)(((t >> 8) + t) >> 8);
}

// the three colour bytes of the pixel packed as r | g << 8 | b << 16 | a << 24 (its bytes in memory order), in the low 24 bits
GHR_HD uint32_t cmp_over_white_pixel(uint32_t rgba)
{
    const uint32_t a = rgba >> 24;
    return (uint32_t)cmp_over_white(rgba & 255u, a) | (uint32_t)cmp_over_white((rgba >> 8) & 255u, a) << 8 |
           (uint32_t)cmp_over_white((rgba >> 16) & 255u, a) << 16;
}

// grid ceil(ceil(n / 4) / 256), block 256; a thread makes pixels 4 q .. 4 q + 3.  VEC (rgba 16-B aligned, rgb 4-B aligned): a
// whole quad is one uint4 load and three dword stores (byte 12 q of rgb is then 4-B aligned); the last, partial quad and every
// quad of the other form go pixel by pixel through bytes.  The same function makes the bytes either way.
template <bool VEC>
__global__ __launch_bounds__(256) void k_cmp_over_white(int64_t n, const uint8_t* __restrict__ rgba, uint8_t* __restrict__ rgb)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x, p0 = 4 * q;
    if (p0 >= n) return;
    if (VEC && p0 + 4 <= n) {
        const uint4 v = *reinterpret_cast<const uint4*>(rgba + 4 * p0);
        const uint32_t o0 = cmp_over_white_pixel(v.x), o1 = cmp_over_white_pixel(v.y), o2 = cmp_over_white_pixel(v.z),
                       o3 = cmp_over_white_pixel(v.w);
        uint32_t* dst = reinterpret_cast<uint32_t*>(rgb + 3 * p0);
        dst[0] = o0 | o1 << 24;
        dst[1] = o1 >> 8 | o2 << 16;
        dst[2] = o2 >> 16 | o3 << 8;
        return;
    }
    for (int j = 0; j < 4 && p0 + j < n; j++) {
        const uint8_t* s = rgba + 4 * (p0 + j);
        const uint32_t o = cmp_over_white_pixel((uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24);
        uint8_t* d = rgb + 3 * (p0 + j);
        d[0] = (uint8_t)o;
        d[1] = (uint8_t)(o >> 8);
        d[2] = (uint8_t)(o >> 16);
    }
}

// ---- the strip -----------------------------------------------------------------------------------------------------------------------

struct CmpStripArgs {
    int w, h;                // a panel's size: the render's
    const uint8_t* gt;       // [h][w][3]: the photograph, resized
    const uint8_t* preview;  // [ph][pw][3]: the strand render, resized
    int pw, ph;
    int dx, dy;              // crop_left - pad_left, crop_top - pad_top: window pixel (y, x) is preview pixel (y + dy, x + dx)
    const uint8_t* render;   // [h][w][3]
    uint8_t* out;            // [h][3 w][3]
};

// Byte xb of row y of the strip, 0 <= xb < 9 w: bytes [0, 3 w) are the photograph's row, [3 w, 6 w) the window's, [6 w, 9 w) the
// render's.  A window pixel whose source lies outside the resized preview is CenterCrop's padding: zero.
GHR_HD uint8_t cmp_strip_byte(const CmpStripArgs& a, int y, int xb)
{
    const int row = 3 * a.w;
    if (xb < row) return a.gt[(size_t)y * row + xb];
    if (xb >= 2 * row) return a.render[(size_t)y * row + (xb - 2 * row)];
    const int b = xb - row, x = b / 3, c = b - 3 * x;
    const int sy = y + a.dy, sx = x + a.dx;
    if (sy < 0 || sy >= a.ph || sx < 0 || sx >= a.pw) return 0;
    return a.preview[((size_t)sy * a.pw + sx) * 3 + c];
}

// grid ceil(ceil(9 w h / 4) / 256), block 256; a thread makes four consecutive bytes of the strip.  A row of the strip is 9 w
// bytes and a panel's row 3 w: with w % 4 == 0 and gt, render and out 4-B aligned (VEC) a thread's bytes are one aligned dword of
// one panel's row, at the same alignment in the outer panels' sources -- a dword load and a dword store there; the middle panel's
// source starts at any byte (dx is any number), so its four bytes are loaded singly and stored as one dword.  Otherwise (w = 33:
// 297 bytes a row) every byte is loaded and stored singly.  cmp_strip_byte decides every byte of both forms.
template <bool VEC>
__global__ __launch_bounds__(256) void k_cmp_strip(CmpStripArgs a)
{
    const size_t row = (size_t)9 * a.w, total = row * a.h;
    const size_t b0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (b0 >= total) return;
    if (VEC) {   // total % 4 == 0 and row % 4 == 0: the four bytes are in one row and one panel
        const int y = (int)(b0 / row), xb = (int)(b0 - (size_t)y * row), prow = 3 * a.w;
        uint32_t v;
        if (xb < prow) {
            v = *reinterpret_cast<const uint32_t*>(a.gt + (size_t)y * prow + xb);
        } else if (xb >= 2 * prow) {
            v = *reinterpret_cast<const uint32_t*>(a.render + (size_t)y * prow + (xb - 2 * prow));
        } else {
            v = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) v |= (uint32_t)cmp_strip_byte(a, y, xb + j) << (8 * j);
        }
        *reinterpret_cast<uint32_t*>(a.out + b0) = v;
        return;
    }
    for (int j = 0; j < 4 && b0 + j < total; j++) {
        const size_t b = b0 + j;
        const int y = (int)(b / row);
        a.out[b] = cmp_strip_byte(a, y, (int)(b - (size_t)y * row));
    }
}

}  // namespace ghr
