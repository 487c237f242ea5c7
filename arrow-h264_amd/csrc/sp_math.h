// sp_math.h -- the scalar arithmetic of SP-slice inter macroblocks, shared by the frame / field
// path (mb_inter_sp.h, k_inter_sp) and the MBAFF path (k_mbaff.hip):
//
//   Transform::itrans_sp / itrans_sp_cr (transform.cc:1098-1265, forward_4x4 :556-595), the
//   arithmetic of the reference as it stands (see oracle/h264r_oracle.c sp_mb for its quirks).
//
// Needs DEV and iabs (device_common.h) from the including file.
#pragma once
#include <stdint.h>

namespace h264r {

__device__ static const uint8_t SP_A[16] = {16, 20, 16, 20, 20, 25, 20, 25, 16, 20, 16, 20, 20, 25, 20, 25};
DEV int sp_sgn(int x) { return (x >= 0) - (x < 0); }                                   // defines.h:73-77
DEV int sp_ls2(int m, int j, int i)                                                     // LevelScale2 :1105-1130
{
    const int cls = (j & 1) + (i & 1);
    constexpr int v0[6] = {13107, 11916, 10082, 9362, 8192, 7282};
    constexpr int v1[6] = {8066, 7490, 6554, 5825, 5243, 4559};
    constexpr int v2[6] = {5243, 4660, 4194, 3647, 3355, 2893};
    return cls == 0 ? v0[m] : (cls == 1 ? v1[m] : v2[m]);
}
DEV int sp_dq(int m, int j, int i)                                                      // dequant_coef :93-100
{
    constexpr int v0[6] = {10, 11, 13, 14, 16, 18};
    constexpr int v1[6] = {13, 14, 16, 18, 20, 23};
    constexpr int v2[6] = {16, 18, 20, 23, 25, 29};
    const int cls = (j & 1) + (i & 1);
    return cls == 0 ? v0[m] : (cls == 1 ? v1[m] : v2[m]);
}
// One coefficient of itrans_sp (luma, :1158-1178): cr the dequantised level, cp the
// transformed prediction; returns the re-dequantised coefficient.
DEV int sp_luma_coef(int cr, int cp, int j, int i, int qp, int qs, int sw)
{
    const int ls = sp_ls2(qs % 6, j, i);
    int cij;
    if (sw) {
        cij = cr + sp_sgn(cp) * ((iabs(cp) * ls + (1 << (14 + qs / 6))) >> (15 + qs / 6));
    } else {
        const int cs = cp + ((int)((unsigned)(cr * sp_dq(qp % 6, j, i) * SP_A[j * 4 + i]) << (qp / 6)) >> 10);
        cij = sp_sgn(cs) * ((iabs(cs) * ls + (1 << (14 + qs / 6))) >> (15 + qs / 6));
    }
    const int dq = sp_dq(qs % 6, j, i);
    return qs >= 24 ? (int)((unsigned)(cij * dq) << (qs / 6 - 4)) : (cij * dq + (1 << (3 - qs / 6))) >> (4 - qs / 6);
}
// One chroma DC coefficient of itrans_sp_cr (:1209-1244): cr the raw DC level (transform_chroma_dc
// skips SP inter MBs, :865-875), cp the 2x2 transform of the four blocks' transformed-prediction
// DCs; qs = QsC < 6.  Returns the coefficient before the closing 2x2 transform.
DEV int sp_chroma_dc(int cr, int cp, int qp, int qs, int sw)
{
    const int ls = sp_ls2(qs % 6, 0, 0);
    int cij;
    if (sw) {
        cij = ((sp_sgn(cp) * (iabs(cp) * ls + (1 << (15 + qs / 6)))) >> (16 + qs / 6)) + cp;
    } else {
        const int cs = cp + ((int)((unsigned)(cr * sp_dq(qp % 6, 0, 0) * 16) << (qp / 6)) >> 9);
        cij = (sp_sgn(cs) * (iabs(cs) * ls + (1 << (15 + qs / 6)))) >> (16 + qs / 6);
    }
    return (int)((unsigned)(cij * sp_dq(qs % 6, 0, 0)) << (qp / 6));
}
// One chroma AC coefficient of itrans_sp_cr (:1246-1260): cr the dequantised level, cp the
// PREDICTION SAMPLE at the coefficient's position (not its transform, :1246)
DEV int sp_chroma_ac(int cr, int cp, int j, int i, int qp, int qs, int sw)
{
    const int ls = sp_ls2(qs % 6, j, i);
    int cij;
    if (sw) {
        cij = cr + ((sp_sgn(cp) * (iabs(cp) * ls + (1 << (14 + qs / 6)))) >> (15 + qs / 6));
    } else {
        const int cs = cp + ((int)((unsigned)(cr * sp_dq(qp % 6, j, i) * SP_A[j * 4 + i]) << (qp / 6)) >> 9);
        cij = (sp_sgn(cs) * (iabs(cs) * ls + (1 << (14 + qs / 6)))) >> (15 + qs / 6);
    }
    return (int)((unsigned)(cij * sp_dq(qs % 6, j, i)) << (qp / 6));
}
// 4-point forward core transform (forward_4x4 rows / columns, :560-594)
DEV void fwd4(int p0, int p1, int p2, int p3, int& c0, int& c1, int& c2, int& c3)
{
    const int e0 = p0 + p3, e1 = p1 + p2, e2 = p1 - p2, e3 = p0 - p3;
    c0 = e0 + e1; c1 = e2 + (e3 << 1); c2 = e0 - e1; c3 = e3 - (e2 << 1);
}
DEV void fwd4_inplace(int& a, int& b, int& c, int& d) { fwd4(a, b, c, d, a, b, c, d); }

}  // namespace h264r
