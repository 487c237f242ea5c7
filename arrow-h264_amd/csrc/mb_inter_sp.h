// mb_inter_sp.h -- the inter macroblocks of SP slices (k_inter_sp), on the lane layout and the
// stages of mb_inter4.h: the prediction is transformed, combined with the levels and re-quantised
// at QS; the reconstruction is the clipped inverse transform alone.
//
//   Decoder::mb_pred_inter decoder.cc:256-257 (inverse_transform_sp), Transform::itrans_sp /
//   itrans_sp_cr (transform.cc:1098-1265, forward_4x4 :556-595), the arithmetic of the reference
//   as it stands (see oracle/h264r_oracle.c sp_mb for its quirks).
#pragma once
#include "mb_inter4.h"
#include "sp_math.h"

namespace h264r {

// itrans_sp of my 4x4 luma block (:1132-1187), all in-lane, and its store
DEV void inter4_sp_luma(uint8_t* rmb, const h264r_mb& q, const h264r_slice* __restrict__ qs, const Inter4Lane& L, const Inter4Res& R,
                        const uint32_t (&predY)[4])
{
    const int qp = q.qp_y, qsy = qs->qs_y, sw = qs->sp_switch;
    const int per = q.qp_scaled[0] / 6;
    int cf[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p0 = predY[i] & 255, p1 = (predY[i] >> 8) & 255, p2 = (predY[i] >> 16) & 255, p3 = predY[i] >> 24;
        fwd4(p0, p1, p2, p3, cf[i][0], cf[i][1], cf[i][2], cf[i][3]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) fwd4(cf[0][c], cf[1][c], cf[2][c], cf[3][c], cf[0][c], cf[1][c], cf[2][c], cf[3][c]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int cr = dq4(level_at(R, i, c), scale_at(R, i, c), per);   // inverse_quantize :409-413
            cf[i][c] = sp_luma_coef(cr, cf[i][c], i, c, qp, qsy, sw);
        }
    idct4x4_inplace(cf);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t wv = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            int v = (cf[i][c] + 32) >> 6;
            // opaque: shift + clamp + byte packing otherwise becomes v_ashr_pk_u8_i32, whose
            // upper result half the compiler takes as zero -- on MI355X it kept the old
            // register's upper bits (bytes 2-3 = 0xFF after a negative input), measured
            asm volatile("" : "+v"(v));
            wv |= (uint32_t)clip255(v) << (8 * c);
        }
        *reinterpret_cast<uint32_t*>(rmb + L.yoff + i * 16) = wv;
    }
}

// itrans_sp_cr (:1190-1265) then inverse_transform_chroma (:1033-1049) of my 2x2 quadrant of both
// planes, and its store: chroma block cb is spread over lanes {blk, ^1, ^4, ^5}; my quadrant rows
// cr.., cols cc..  The DC pass takes the raw DC levels (transform_chroma_dc skips SP inter MBs,
// :865-875), the AC pass the PREDICTION SAMPLES (:1246)
DEV void inter4_sp_chroma(uint8_t* rmb, const h264r_mb& q, const h264r_slice* __restrict__ qs, const Inter4Lane& L, const Inter4Res& R,
                          const uint32_t (&predC)[2], int lane)
{
    const int cb = L.cb, cr = L.cr, cc = L.cc;
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
        const int qpc = q.qp_c[pl], qsc = qs->qs_c[pl];
        int pr[2][2], f[2][2];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 2; ++c) pr[r][c] = (predC[pl] >> (16 * r + 8 * c)) & 255;
        // forward transform of the prediction: rows, then columns
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            f[r][0] = pr[r][0];
            f[r][1] = pr[r][1];
            quad_rows<fwd4_inplace>(f[r][0], f[r][1], cc);
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) quad_cols<fwd4_inplace, true>(f[0][c], f[1][c], cr);
        // the four blocks' DC coefficients (lanes 0, 2, 8, 10 of the MB's 16)
        const int gb = lane & ~15;
        const int d00 = __shfl(f[0][0], gb + 0), d01 = __shfl(f[0][0], gb + 2);
        const int d10 = __shfl(f[0][0], gb + 8), d11 = __shfl(f[0][0], gb + 10);
        int mp[4] = {d00 + d10 + d01 + d11, d00 - d10 + d01 - d11, d00 + d10 - d01 - d11, d00 - d10 - d01 + d11};
        const int c00 = (int16_t)(R.cdc[pl].x & 0xFFFF), c01 = (int16_t)(R.cdc[pl].x >> 16);
        const int c10 = (int16_t)(R.cdc[pl].y & 0xFFFF), c11 = (int16_t)(R.cdc[pl].y >> 16);
        const int crd[4] = {c00, c01, c10, c11};
        const int ls0 = sp_ls2(qsc % 6, 0, 0);
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int cp = mp[n];
            int cij;
            if (qs->sp_switch) {
                cij = ((sp_sgn(cp) * (iabs(cp) * ls0 + (1 << (15 + qsc / 6)))) >> (16 + qsc / 6)) + cp;
            } else {
                const int cs = cp + ((int)((unsigned)(crd[n] * sp_dq(qpc % 6, 0, 0) * 16) << (qpc / 6)) >> 9);
                cij = (sp_sgn(cs) * (iabs(cs) * ls0 + (1 << (15 + qsc / 6)))) >> (16 + qsc / 6);
            }
            mp[n] = (int)((unsigned)(cij * sp_dq(qsc % 6, 0, 0)) << (qpc / 6));
        }
        // AC (every position; (0,0) is replaced by the DC result below)
        int k[2][2];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int j = cr + r, i = cc + c;
                const int crv = dq4((int16_t)(R.clev[pl][r] >> (16 * c)), (int16_t)(R.csc[pl][r] >> (16 * c)), qpc / 6);
                const int cp = pr[r][c], ls = sp_ls2(qsc % 6, j, i);
                int cij;
                if (qs->sp_switch) {
                    cij = crv + ((sp_sgn(cp) * (iabs(cp) * ls + (1 << (14 + qsc / 6)))) >> (15 + qsc / 6));
                } else {
                    const int cs = cp + ((int)((unsigned)(crv * sp_dq(qpc % 6, j, i) * SP_A[j * 4 + i]) << (qpc / 6)) >> 9);
                    cij = (sp_sgn(cs) * (iabs(cs) * ls + (1 << (14 + qsc / 6)))) >> (15 + qsc / 6);
                }
                k[r][c] = (int)((unsigned)(cij * sp_dq(qsc % 6, j, i)) << (qpc / 6));
            }
        if (cr == 0 && cc == 0) {
            const int dcv = cb == 0 ? (mp[0] + mp[1] + mp[2] + mp[3]) >> 1
                          : cb == 1 ? (mp[0] + mp[1] - mp[2] - mp[3]) >> 1
                          : cb == 2 ? (mp[0] - mp[1] + mp[2] - mp[3]) >> 1
                                    : (mp[0] - mp[1] - mp[2] + mp[3]) >> 1;
            k[0][0] = dcv;
        }
        // inverse transform (inter4_chroma_residual's 32-bit path) and construction with the prediction
#pragma unroll
        for (int r = 0; r < 2; ++r) quad_rows<idct4_inplace>(k[r][0], k[r][1], cc);
#pragma unroll
        for (int c = 0; c < 2; ++c) quad_cols<idct4_inplace, true>(k[0][c], k[1][c], cr);
        uint8_t* cdst = rmb + L.coff + pl * 64;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const uint32_t wv = (uint32_t)clip255(pr[r][0] + ((k[r][0] + 32) >> 6)) | ((uint32_t)clip255(pr[r][1] + ((k[r][1] + 32) >> 6)) << 8);
            *reinterpret_cast<uint16_t*>(cdst + r * 8) = (uint16_t)wv;
        }
    }
}

// The inter macroblocks of SP slices among a0 .. a0+3 of picture `pic` (k_inter_sp): the ones
// inter4_mbs flagged and left out.
DEV void inter4_sp_mbs(const h264r_batch& b, const Geom& g, int pic, int a0, int aend, int lane, const Inter4Lds& S,
                       uint8_t* __restrict__ recon)
{
    const Inter4Lane L = inter4_lane(g, a0, aend, lane);
    const h264r_slice* slices = b.slices + (size_t)pic * b.slice_stride;
    const Inter4Pre pre = inter4_pre(b, g, pic, a0, aend, lane);
    const h264r_mb q = pre.q;
    const h264r_slice* qs = &slices[q.slice];
    const uint2 qsh = slice_hdr(slices, S, q.slice);
    const uint2 m0 = motion_word(pre.mv[0], pre.ri[0], slices, S, q.slice, 0);
    const uint2 m1 = motion_word(pre.mv[1], pre.ri[1], slices, S, q.slice, 1);
    if (!L.valid || mb_is_intra(q) || (qsh.x & 255) != H264R_SLICE_SP) return;

    uint32_t predY[4], predC[2];
    inter4_predict(b, g, pic, L, S, qs, qsh.y & 255, m0, m1, predY, predC);
    const Inter4Res R = inter4_res_load(q, L, b.levels + q.coef_off, &b.quant[pic]);
    uint8_t* const rmb = recon_mb(recon, g, pic, L.aa);
    inter4_sp_luma(rmb, q, qs, L, R, predY);
    inter4_sp_chroma(rmb, q, qs, L, R, predC, lane);
}

}  // namespace h264r
