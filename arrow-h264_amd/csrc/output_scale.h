// output_scale.h -- the window and pixel code of the scaled RGB kernels, shared by the k_output_rgb_scaled
// kernels (k_output_scale.hip: one region and output size per job, kernel arguments) and the
// k_output_boxes kernels (k_output_boxes.hip: one per box, read from a plan record).  Both filters of
// include/h264r_output.h as one weighted window of source samples: the quotients by divisors whose
// reciprocals the ScaleAxis carries (scale_div), an axis' window and weights (scale_window, scale_weight),
// the fetch of a 16-pixel source unit at any column of the crop (scale_fetch), and the three channel
// sums of one output pixel (scale_pixel).  k_output_scale.hip's comment says how they fit together.
// Everything is inlined; neither kernel family's registers depend on the other.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "output_rgb.h"

namespace h264r {

// n / den for a quotient below 2^16: inv = 1 / den in binary32 guesses it to within one
__device__ __forceinline__ uint32_t scale_div(uint32_t n, uint32_t den, float inv)
{
    uint32_t q = (uint32_t)((float)n * inv);
    const int32_t rem = (int32_t)(n - q * den);
    if (rem < 0) --q;
    else if (rem >= (int32_t)den) ++q;
    return q;
}

// One axis of one output index d: the window [lo, hi) of source samples and what their weights need.
struct ScaleWin {
    int lo, hi;
    int a, b;                  // AREA: the interval [a, b) = [d S, (d + 1) S) in units of 1 / D; BILINEAR: w0, w1
};

__device__ __forceinline__ ScaleWin scale_window(const ScaleAxis& X, int d, int filter)
{
    ScaleWin w;
    if (filter == H264R_SCALE_AREA) {
        w.a = d * X.s;
        w.b = w.a + X.s;
        w.lo = (int)scale_div((uint32_t)w.a, (uint32_t)X.d, X.inv_d);
        w.hi = (int)scale_div((uint32_t)(w.b + X.d - 1), (uint32_t)X.d, X.inv_d);
    } else {
        const int p = min(max((2 * d + 1) * X.S - X.D, 0), 2 * X.D * (X.S - 1));
        w.lo = (int)scale_div((uint32_t)p, (uint32_t)(2 * X.D), X.inv_2D);
        const int f = p - 2 * X.D * w.lo;
        w.b = (int)scale_div((uint32_t)(256 * f + X.D), (uint32_t)(2 * X.D), X.inv_2D);
        w.a = 256 - w.b;
        w.hi = w.lo + (w.b ? 2 : 1);                      // w1 == 0 wherever i1 == i0
    }
    return w;
}

// the weight of source sample i (any integer; outside the window: 0)
__device__ __forceinline__ int scale_weight(const ScaleWin& w, int i, int D, int filter)
{
    if (filter == H264R_SCALE_AREA) return max(min(w.b, (i + 1) * D) - max(w.a, i * D), 0);
    return i == w.lo ? w.a : i == w.lo + 1 ? w.b : 0;
}

// v's 16 bytes moved down by sh (0..15); the bytes that come in at the top repeat its last
__device__ __forceinline__ uint4 scale_shr(uint4 v, int sh)
{
    const uint32_t rep = (v.w >> 24) * 0x01010101u;
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
    if (sh & 8) { w[0] = w[2]; w[1] = w[3]; w[2] = w[3] = rep; }
    if (sh & 4) { w[0] = w[1]; w[1] = w[2]; w[2] = w[3]; w[3] = rep; }
    const uint32_t bs = (uint32_t)sh & 3u;
    return make_uint4(__builtin_amdgcn_alignbyte(w[1], w[0], bs), __builtin_amdgcn_alignbyte(w[2], w[1], bs),
                      __builtin_amdgcn_alignbyte(w[3], w[2], bs), __builtin_amdgcn_alignbyte(rep, w[3], bs));
}

// eight chroma samples and the clamped ninth (SubWidthC 2) moved down by sh samples: those behind the
// crop's last repeat it, which is the clamp of the bilinear taps
__device__ __forceinline__ uint4 scale_shr8(uint4 v, int sh)
{
    const uint32_t rep = (v.y >> 24) * 0x01010101u;
    return scale_shr(make_uint4(v.x, v.y, rep, rep), sh);
}

// rgb_fetch_at (output_rgb.h) for a unit at any column.  A unit that reaches past the crop's last column is, where
// the crop is 16 wide at least, the crop's LAST whole unit moved down in registers: wide loads of
// samples inside the crop and a byte shift, instead of the bytewise fetch (one round trip per sample).
template <int MODE>
__device__ __forceinline__ void scale_fetch(const RgbJob& J, ScaleSrc src, const uint8_t* const (&yp)[2], const uint8_t* const (&up)[2],
                                            const uint8_t* const (&vp)[2], RgbUnit& t)
{
    if (t.n == RGB_UNIT || J.lw < RGB_UNIT) {
        rgb_fetch_at<MODE>(J, src, yp, up, vp, t);
        return;
    }
    RgbUnit b;
    b.r = t.r;
    b.x = J.lw - RGB_UNIT;
    b.n = RGB_UNIT;
    rgb_fetch_at<MODE>(J, src, yp, up, vp, b);
    const int sh = t.x - b.x;                               // 1..15; even where SubWidthC is 2
    t.y = scale_shr(b.y, sh);
    if (MODE == RGB_MONO) return;
    if (MODE < RGB_REP) {
        t.ua = scale_shr(b.ua, sh);
        t.va = scale_shr(b.va, sh);
    } else {
        t.ua = scale_shr8(b.ua, sh >> 1);
        t.va = scale_shr8(b.va, sh >> 1);
        if (MODE == RGB_BIL2) {
            t.ub = scale_shr8(b.ub, sh >> 1);
            t.vb = scale_shr8(b.vb, sh >> 1);
        }
    }
}

// The three channel sums of output pixel (dy, dx) of one frame.
template <int MODE, int FILTER>
__device__ __forceinline__ void scale_pixel(const ScaleJob& S, ScaleSrc src, const uint8_t* const (&yp)[2], const uint8_t* const (&up)[2],
                                            const uint8_t* const (&vp)[2], int dy, int dx, uint32_t (&acc)[3])
{
    const RgbJob& J = S.rgb;
    const ScaleWin wx = scale_window(S.ax, dx, FILTER), wy = scale_window(S.ay, dy, FILTER);
    const int xend = S.roi_x + wx.hi;                       // columns and rows of the cropped rectangle from here on
    int xc = S.roi_x + wx.lo;
    if (MODE >= RGB_REP) xc &= ~1;
    do {                                                    // no window is empty
        int wh[RGB_UNIT];
#pragma unroll
        for (int q = 0; q < RGB_UNIT / 4; ++q) {
            const bool weighed = 4 * q < S.taps;            // job-wide: a branch, not a lane mask
#pragma unroll
            for (int k = 4 * q; k < 4 * q + 4; ++k) wh[k] = 0;
            if (weighed) {
#pragma unroll
                for (int k = 4 * q; k < 4 * q + 4; ++k) wh[k] = scale_weight(wx, xc + k - S.roi_x, S.ax.d, FILTER);
            }
        }
        RgbUnit t;
        t.x = xc;
        t.n = min(RGB_UNIT, J.lw - xc);
        int iy = wy.lo;
        do {
            t.r = S.roi_y + iy;
            scale_fetch<MODE>(J, src, yp, up, vp, t);
            uint32_t row[3] = {0, 0, 0};
#pragma unroll
            for (int q = 0; q < RGB_UNIT / 4; ++q) {
                if (4 * q < S.taps) {                       // job-wide: four pixels at a time
#pragma unroll
                    for (int k = 4 * q; k < 4 * q + 4; ++k) {
                        int r, g, b;
                        rgb_pixel<MODE>(J, t, k, r, g, b);
                        row[0] += (uint32_t)__mul24(wh[k], r);
                        row[1] += (uint32_t)__mul24(wh[k], g);
                        row[2] += (uint32_t)__mul24(wh[k], b);
                    }
                }
            }
            const uint32_t wv = (uint32_t)scale_weight(wy, iy, S.ay.d, FILTER);
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += wv * row[c];
        } while (++iy < wy.hi);
    } while ((xc += RGB_UNIT) < xend);
}

}  // namespace h264r
