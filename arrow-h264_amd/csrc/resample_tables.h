// resample_tables.h -- the coefficient table of one axis of h264r_output_rgb_resampled, exactly as
// include/h264r_output.h states it ("Resampled RGB frames"): Pillow's 8-bit resampler, whose coefficients
// are binary64 values rounded to 22-bit integers.  Device-free and header-only: host_output.hip builds a
// plan's two axes with it, h264r_resample_axis exports it, and tools/resample_tables_check.cc compiles it
// on its own under the sanitizers.
//
// Every floating-point operation below is one binary64 operation in the header's order.  Contraction is
// off: an a * b + c fused by the host compiler rounds once where the definition rounds twice, and the
// 22-bit integer can come out one apart.
#pragma once

#include <math.h>
#include <stdint.h>

#include "h264r_output.h"

// (a compiler that does not know the pragma is given -ffp-contract=off instead)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace h264r {

// support of the filter's kernel, 0: no such filter
inline double resample_support(int filter)
{
    return filter == H264R_RESAMPLE_TRIANGLE ? 1.0 : filter == H264R_RESAMPLE_BICUBIC ? 2.0 : filter == H264R_RESAMPLE_LANCZOS ? 3.0 : 0.0;
}

inline double resample_sinc(double x)
{
    if (x == 0.0) return 1.0;
    x = x * 3.14159265358979323846;
    return sin(x) / x;
}

// f of the header, per filter
inline double resample_kernel(int filter, double x)
{
    if (filter == H264R_RESAMPLE_LANCZOS) {
        if (-3.0 <= x && x < 3.0) return resample_sinc(x) * resample_sinc(x / 3);
        return 0.0;
    }
    if (x < 0.0) x = -x;
    if (filter == H264R_RESAMPLE_TRIANGLE) return x < 1.0 ? 1.0 - x : 0.0;
    const double a = -0.5;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// ksize of an axis whose arguments resample_axis accepts
inline int64_t resample_ksize(int filter, int in0, int in1, int out_size)
{
    const double scale = (double)(in1 - in0) / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = resample_support(filter) * filterscale;
    return 2 * (int64_t)ceil(support) + 1;
}

// The table of one axis: for every output index d the first source sample xmin[d], the number of taps
// count[d] (1 .. ksize) and the taps kk[d * ksize + j], zero from count[d] on.  With the three arrays
// NULL only *ksize is written.  xmin and count hold out_size entries, kk out_size * *ksize.
// H264R_EINVAL: no such filter, in_size < 1, a region [in0, in1) that is empty or not inside
// [0, in_size), out_size outside 1..H264R_SCALE_MAX_OUT, a NULL ksize, some but not all arrays NULL.
inline int resample_axis(int filter, int in_size, int in0, int in1, int out_size, int32_t* xmin, int32_t* count, int32_t* kk,
                         int32_t* ksize)
{
    const double fs = resample_support(filter);
    if (fs == 0.0 || !ksize || in_size < 1 || in0 < 0 || in1 <= in0 || in1 > in_size || out_size < 1 || out_size > H264R_SCALE_MAX_OUT)
        return H264R_EINVAL;
    if ((xmin == nullptr) != (count == nullptr) || (xmin == nullptr) != (kk == nullptr)) return H264R_EINVAL;
    const double scale = (double)(in1 - in0) / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = fs * filterscale;
    const double ss = 1.0 / filterscale;
    const int64_t ks = 2 * (int64_t)ceil(support) + 1;
    *ksize = (int32_t)ks;
    if (!xmin) return H264R_OK;
    for (int d = 0; d < out_size; ++d) {
        const double center = in0 + (d + 0.5) * scale;
        int lo = (int)(center - support + 0.5);
        if (lo < 0) lo = 0;
        int hi = (int)(center + support + 0.5);
        if (hi > in_size) hi = in_size;
        const int n = hi - lo;                              // 1 .. ksize: the centre lies inside [0, in_size]
        int32_t* const k = kk + (int64_t)d * ks;
        double ww = 0.0;
        // the real taps are computed twice, once for ww and once for the quotient, so that no binary64 row
        // is kept: the same operations on the same operands give the same bits
        for (int j = 0; j < n; ++j) ww += resample_kernel(filter, (j + lo - center + 0.5) * ss);
        for (int j = 0; j < n; ++j) {
            double w = resample_kernel(filter, (j + lo - center + 0.5) * ss);
            if (ww != 0.0) w /= ww;
            k[j] = w < 0 ? (int32_t)(-0.5 + w * (double)(1 << 22)) : (int32_t)(0.5 + w * (double)(1 << 22));
        }
        for (int64_t j = n; j < ks; ++j) k[j] = 0;
        xmin[d] = lo;
        count[d] = n;
    }
    return H264R_OK;
}

}  // namespace h264r
