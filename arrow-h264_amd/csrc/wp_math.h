// wp_math.h -- the implicit bi-prediction weight (weighted_bipred_idc 2), shared by the host helper
// h264r_implicit_w1 (h264r_host.hip) and the MBAFF path's field MBs (k_mbaff.hip):
//
//   InterPrediction::bi_prediction (inter_prediction.cc:120-137), the arithmetic of the reference as
//   it stands: C's truncating division in tx, tb and td clipped to -128 .. 127, the default weights
//   for td == 0, a long-term reference and a weight outside -64 .. 128.
//
// Host and device; needs nothing from the including file.
#pragma once

namespace h264r {

// weight1 of the pair (ref0, ref1) for a current picture of POC cur; weight0 = 64 - weight1
__host__ __device__ inline int wp_implicit_w1(int cur, int poc0, int poc1, int lt0, int lt1)
{
    const int d = poc1 - poc0, td = d < -128 ? -128 : (d > 127 ? 127 : d);             // :120
    if (td == 0 || lt0 || lt1) return 32;                                              // :121-123
    const int e = cur - poc0, tb = e < -128 ? -128 : (e > 127 ? 127 : e);              // :127
    const int h = td / 2, tx = (16384 + (h < 0 ? -h : h)) / td;                        // :128
    const int s = (tx * tb + 32) >> 6, dsf = s < -1024 ? -1024 : (s > 1023 ? 1023 : s); // :129
    const int w1 = dsf >> 2;                                                           // :131
    return w1 < -64 || w1 > 128 ? 32 : w1;                                             // :133-136
}

}  // namespace h264r
