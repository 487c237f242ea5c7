// mb_inter4.h -- inter (and I_PCM) macroblocks, FOUR per 64-lane wave, one lane per
// 4x4 luma block (+ its 2x2 chroma sub-blocks in both planes), and the deblocking
// record of every MB.
//
//   Decoder::mb_pred_inter decoder.cc:212-262 (partition walk = per-4x4 motion),
//   InterPrediction::get_block_luma inter_prediction.cc:158-340 (6-tap qpel),
//   get_block_chroma :342-406 (bilinear), mc_prediction :53-86 and bi_prediction
//   :88-156 (weighted prediction), Transform::inverse_transform_inter
//   transform.cc:1051-1095 (inverse_4x4 :597-641, inverse_8x8 :643-733, chroma DC
//   :875-889, construction :913-984), mb_pred_ipcm decoder.cc:149-168,
//   Deblock::strength deblock.cc:78-289 (boundary strengths, DbInfo).
//
// Why this shape: a wave per MB with a lane per sample row keeps one MB in flight
// per wave, recomputes the 6-tap intermediates of every row in every lane, and
// leaves the kernel latency-bound (a handful of dependent global round trips per MB,
// at 5 waves per SIMD).  With a lane per 4x4 block a wave carries four MBs, each
// lane filters its 9x9 reference window once (the horizontal intermediates of a row
// feed both the half-sample b and the centre j of all four output rows), the 4x4
// inverse transform runs entirely in-lane, and a 4x4 block's motion is exactly what
// the boundary strengths of its left and top edges need.
//
// Lane roles: g = lane >> 4 picks the MB (a0 + g), blk = lane & 15 the 4x4 block in
// raster order (bx = blk & 3, by = blk >> 2).  Chroma: the lane owns the 2x2 chroma
// samples (2bx.., 2by..) of each plane (4:2:0: the chroma of a luma 4x4 block, with
// the same motion vector).  A chroma 4x4 transform block is spread over the lanes
// {blk, blk^1, blk^4, blk^5}; an 8x8 luma transform block likewise.
//
// inter4_mbs (k_inter4r, at the end of the file) is a sequence of stages, each a function whose
// parameters are what it reads and writes: inter4_lane (Inter4Lane, the roles above) -> the gate
// (invalid / intra / SP / inter4_pcm) -> inter4_predict -> inter4_res_load (Inter4Res) ->
// inter4_luma_residual (luma_res_bypass / luma_res_4x4 / luma_res_8x8) -> inter4_store_luma ->
// inter4_chroma_residual -> inter4_store_chroma.  The generic instantiation parks state in LDS between
// the stages (Inter4Park), the PLAIN one does not.  The inter MBs of SP slices are k_inter_sp's:
// inter4_sp_mbs (mb_inter_sp.h), on the same lane roles, prediction and residual inputs.
#pragma once
#include "mb_deblock.h"
#include "launch_cfg.h"

// H264R_INTER_DIAG: diagnostic builds only (wrong output; make EXTRA=-DH264R_INTER_DIAG=<bits>) that
// take one part of k_inter4r away to time the rest: 1 one 16-byte store per lane, 2 no luma
// filter (window loads kept), 4 neither, 8 no chroma MC, 16 no residual (nor its loads), 32 no
// deblocking records, 64 no luma residual transform (its loads kept), 128 the same for chroma
#ifndef H264R_INTER_DIAG
#define H264R_INTER_DIAG 0
#endif
// H264R_INTER_FAST: the two shortcuts of k_inter4r, each wave-uniform with today's code as the other
// branch, so either can be A/B'd alone (make EXTRA=-DH264R_INTER_FAST=<bits>): 1 the residual and
// the construction on packed 16-bit pairs (the PK parameter of luma_res_4x4 and
// inter4_chroma_residual), 2 one-list deblocking records (k_recon.hip)
#ifndef H264R_INTER_FAST
#define H264R_INTER_FAST 3
#endif
// H264R_INTER_MC: shorter forms around the motion compensation, each with the form before it as the other
// side of an `if constexpr`, so that either builds from one tree for an A/B (make EXTRA=-DH264R_INTER_MC=<bits>):
// 1 the luma and chroma window fetches clamp rows and columns by one v_med3_i32 (clip0), 2 inter4_lane divides
// in 24 bits, 4 a luma window across the left or right edge is fixed up once, in a block that a wave without such a
// lane skips (luma_window_edge), and the row loop of luma_block_pred has no branch (the PLAIN stages only: the
// generic ones spill with it).  What else was tried in
// luma_block_pred and why it is not here: profiles/r12_a_inter_mc_wg_ab.txt.
#ifndef H264R_INTER_MC
#define H264R_INTER_MC 7
#endif

namespace h264r {

constexpr int INTER4_WG_WAVES = H264R_INTER_WG_WAVES;   // waves of a k_inter4r workgroup (launch_cfg.h)
constexpr int INTER4_WG_THREADS = 64 * INTER4_WG_WAVES;
constexpr int INTER4_MBS = 4 * INTER4_WG_WAVES;          // MBs per k_inter4r workgroup (4 per wave)
constexpr int INTER4_LDS_SLICES = 64;   // slices whose ref tables the workgroup keeps in LDS
constexpr int INTER4_PLAIN_SLICES = 8;  // slices of a plain picture at most (inter4_plain_picture)
static_assert(INTER4_PLAIN_SLICES <= INTER4_LDS_SLICES, "a plain picture's slices are all in the LDS copy");

struct Inter4Lds {
    const uint8_t* planes[3 * H264R_MAX_SLOTS];
    uint2 hdr[INTER4_LDS_SLICES];                            // dwords 0..1 of the picture's slices (type, idc, offsets, wp)
    int8_t ref_slot[INTER4_LDS_SLICES][2][H264R_MAX_REFS];   // h264r_slice::ref_slot of the picture's slices
    uint8_t slice_type[INTER4_LDS_SLICES];                   // h264r_slice::slice_type of the same slices
    uint8_t not_plain[INTER4_PLAIN_SLICES];                  // slice i keeps the picture from being plain (inter4_plain_picture)
};

// k_inter4r's parking space for the GENERIC stages: INTER4_PARK_SLOTS dwords per lane that hold state
// over a motion compensation which does not read it, so that the generic side fits the kernel's
// register budget (k_recon.hip H264R_INTER_WAVES) without scratch.  Lane-major ([slot][thread]): a
// wave's 64 lanes touch 64 consecutive dwords, no bank conflict.  A slot is its lane's own, written
// and read back by the same lane under the same exec mask: no barrier.  The accesses are volatile, so
// the compiler neither forwards the stored value to the read (that would keep it in a register) nor
// moves them across each other.
constexpr int PARK_PRED = 0;     // 2 x 6: each list's prediction (4 luma rows, 2 chroma planes) until the combine
constexpr int PARK_M1 = 12;      // 2: list 1's motion word while list 0 is compensated
constexpr int PARK_Q = 14;       // 4: the MB record's dwords 0, 3, 2, 4 (park_put_mb)
constexpr int INTER4_PARK_SLOTS = 18;
struct Inter4Park {
    uint32_t w[INTER4_PARK_SLOTS][INTER4_WG_THREADS];
};
// (address space 3 by name: a volatile access through a generic pointer stays a flat one, 64-bit address and all)
typedef __attribute__((address_space(3))) volatile uint32_t lds_vdword;
DEV void park_put(Inter4Park& P, int slot, uint32_t v) { *(lds_vdword*)&P.w[slot][threadIdx.x] = v; }
DEV uint32_t park_get(Inter4Park& P, int slot) { return *(lds_vdword*)&P.w[slot][threadIdx.x]; }
// The MB record's dwords that the stages after the motion compensation read (the residual and the
// slice's weights: mb_type, flags, cbp, slice, qp_scaled, coef_off); the others come back zero (the
// lossless path reads its prediction modes from the batch, luma_res_bypass).
constexpr int PARK_Q_N = 4;
constexpr int PARK_Q_WORD[PARK_Q_N] = {0, 3, 2, 4};            // the chroma residual's first: cbp, flags, qp_scaled
DEV void park_put_mb(Inter4Park& P, const h264r_mb& q)
{
    const uint32_t* w = reinterpret_cast<const uint32_t*>(&q);
#pragma unroll
    for (int k = 0; k < PARK_Q_N; ++k) park_put(P, PARK_Q + k, w[PARK_Q_WORD[k]]);
}
// FIRST: the first FIRST of those dwords only
template <int FIRST = PARK_Q_N>
DEV h264r_mb park_get_mb(Inter4Park& P)
{
    h264r_mb q = {};
    uint32_t* w = reinterpret_cast<uint32_t*>(&q);
#pragma unroll
    for (int k = 0; k < FIRST; ++k) w[PARK_Q_WORD[k]] = park_get(P, PARK_Q + k);
    return q;
}

// A lane's roles ("Lane roles" above) for the MBs a0 .. a0+3 of a picture.
struct Inter4Lane {
    int blk, bx, by;   // my 4x4 block of the MB, raster
    int aa;            // my MB's address (the range's last MB for the lanes past its end)
    bool valid;        // my MB is one of the range's
    int mbx, mby;      // my MB in the picture
    int X4, Y4;        // my block in the picture, in 4x4 units
    int b8;            // my 8x8 block: its levels, and its transform in a T8x8 MB
    int cb, cr, cc;    // my chroma 4x4 block of each plane (= b8) and my 2x2 quadrant of it: rows cr.., cols cc..
    int yoff, coff;    // my block's first luma row and my Cb quadrant (Cr 64 bytes on) in the MB's 384 bytes of the
                       // MB-tiled reconstruction (device_common.h recon_mb): rows of 16 / 8 bytes
};
DEV Inter4Lane inter4_lane(const Geom& g, int a0, int aend, int lane)
{
    Inter4Lane L;
    const int blk = lane & 15, bx = blk & 3, by = blk >> 2, a = a0 + (lane >> 4);
    L.blk = blk; L.bx = bx; L.by = by;
    L.valid = a < aend;
    L.aa = L.valid ? a : aend - 1;
    if constexpr (H264R_INTER_MC & 2) {
        // an MB address is below 2^24 and a picture's width in MBs below 2^16 (level 6.2 allows 139,264 MBs):
        // said to the compiler, the division is its 24-bit form, a third of the signed 32-bit one's instructions
        const uint32_t ua = (uint32_t)L.aa & 0xFFFFFFu, uw = (uint32_t)g.wmb & 0xFFFFu;
        L.mby = (int)(ua / uw); L.mbx = (int)(ua - (uint32_t)L.mby * uw);
    } else {
        L.mbx = L.aa % g.wmb; L.mby = L.aa / g.wmb;
    }
    L.X4 = L.mbx * 4 + bx; L.Y4 = L.mby * 4 + by;
    L.b8 = L.cb = (by >> 1) * 2 + (bx >> 1);
    L.cr = (by & 1) * 2; L.cc = (bx & 1) * 2;
    L.yoff = (by * 4) * 16 + bx * 4;
    L.coff = RECON_CB + (by * 2) * 8 + bx * 2;
    return L;
}

// Byte `off` of slice `slice`'s h264r_slice, for the slices past the LDS copy: a buffer
// load (a select between an LDS and a global byte became one flat load, whose wait covers
// every outstanding load of both kinds).
DEV int slice_byte(const h264r_slice* slices, int slice, int off)
{
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<h264r_slice*>(slices + slice), 0,
                                                                        (int)sizeof(h264r_slice), 0x00020000);
    return __builtin_amdgcn_raw_buffer_load_b8(rs, off, 0, 0);
}
// NEAR (a template parameter of the three readers below and of the stages that call them): every
// slice index the caller passes is below INTER4_LDS_SLICES, so the LDS copy answers alone and the
// slice-table path is not compiled (the PLAIN stages: a plain picture has at most INTER4_PLAIN_SLICES).
// slice_type of a slice: the LDS copy, else the slice table
template <bool NEAR = false>
DEV int slice_type_of(const h264r_slice* slices, const Inter4Lds& S, int slice)
{
    int t = S.slice_type[min(slice, INTER4_LDS_SLICES - 1)];
    if constexpr (!NEAR)
        if (slice >= INTER4_LDS_SLICES) t = slice_byte(slices, slice, (int)offsetof(h264r_slice, slice_type));
    return t;
}

// Dwords 0..1 of slice `slice` (type, idc, filter offsets, wp mode, log2 wd): the LDS copy,
// else the slice table
template <bool NEAR = false>
DEV uint2 slice_hdr(const h264r_slice* slices, const Inter4Lds& S, int slice)
{
    if (NEAR || slice < INTER4_LDS_SLICES) return S.hdr[NEAR ? min(slice, INTER4_LDS_SLICES - 1) : slice];
    return *reinterpret_cast<const uint2*>(&slices[slice]);
}

// Motion of one 4x4 block as {mv, ref_idx | slot << 8} per list: RefPicList[l][ref_idx]
// of the block's slice resolved to its DPB slot (get_ref_pic dpb.cc:1046-1054;
// pic_motion_params::ref_pic interpret_mb.cc:611-623), slot -1 when the list is unused.
template <bool NEAR = false>
DEV uint2 motion_word(uint32_t mv, int ri, const h264r_slice* slices, const Inter4Lds& S, int slice, int l)
{
    // the table read at a clamped index and the "no list" case selected afterwards: an LDS
    // read under the lane's `has` compiled to a lane-divergent branch
    const bool has = ri >= 0 && ri < H264R_MAX_REFS;
    const int ric = has ? ri : 0;
    int slot = S.ref_slot[min(slice, INTER4_LDS_SLICES - 1)][l][ric];
    if constexpr (!NEAR)
        if (slice >= INTER4_LDS_SLICES)
            slot = (int8_t)slice_byte(slices, slice, (int)offsetof(h264r_slice, ref_slot) + l * H264R_MAX_REFS + ric);
    slot = has ? slot : -1;
    return make_uint2(mv, (uint32_t)(uint8_t)ri | ((uint32_t)(uint8_t)slot << 8));
}
DEV uint2 block_motion(const h264r_batch& b, const h264r_slice* slices, const Inter4Lds& S, size_t at, int slice, int l)
{
    return motion_word(b.mv[at], b.ref_idx[at], slices, S, slice, l);
}

DEV h264r_mb mb_lane(const h264r_mb* p)          // per-lane 32-byte record, two 16-byte loads
{
    const uint4* q = reinterpret_cast<const uint4*>(p);
    const uint4 w0 = q[0], w1 = q[1];
    h264r_mb m;
    uint32_t* w = reinterpret_cast<uint32_t*>(&m);
    w[0] = w0.x; w[1] = w0.y; w[2] = w0.z; w[3] = w0.w; w[4] = w1.x; w[5] = w1.y; w[6] = w1.z; w[7] = w1.w;
    return m;
}

// A lane's MB record, its block's motion ({mv, ref_idx} per list) and the slice header:
// none depends on the workgroup's LDS tables, so the kernels issue them before filling
// those tables (one global round trip less in front of the motion compensation).
struct Inter4Pre {
    h264r_mb q;
    uint32_t mv[2];
    int ri[2];
};
DEV Inter4Pre inter4_pre(const h264r_batch& b, const Geom& g, int pic, int a0, int aend, int lane)
{
    const Inter4Lane L = inter4_lane(g, a0, aend, lane);
    const int mi = L.Y4 * g.W4 + L.X4;
    const size_t mbase = (size_t)pic * 2 * g.motion_plane;
    Inter4Pre p;
    p.q = mb_lane(&b.mbs[(size_t)pic * g.nmb + L.aa]);
#pragma unroll
    for (int l = 0; l < 2; ++l) {
        p.mv[l] = b.mv[mbase + l * g.motion_plane + mi];
        p.ri[l] = b.ref_idx[mbase + l * g.motion_plane + mi];
    }
    return p;
}

// What the deblocking record of a lane's block reads besides its own MB: the left and upper
// MB records and the motion of the blocks left of and above it (the MB's own blocks or the
// neighbours'), loaded unconditionally and with no dependence on the MB record, so k_inter4r
// issues them together with inter4_pre's loads (one global round trip per group).
struct DbNb {
    h264r_mb L, U;
    uint32_t lmv[2], umv[2];
    int lri[2], uri[2];
};
DEV DbNb dbinfo_pre(const h264r_batch& b, const Geom& g, int pic, int a0, int aend, int lane)
{
    const Inter4Lane L = inter4_lane(g, a0, aend, lane);
    const int aa = L.aa, mi = L.Y4 * g.W4 + L.X4;
    const int li = L.X4 > 0 ? mi - 1 : mi, ui = L.Y4 > 0 ? mi - g.W4 : mi;
    const size_t mbase = (size_t)pic * 2 * g.motion_plane;
    const h264r_mb* mbs = b.mbs + (size_t)pic * g.nmb;
    DbNb n;
    n.L = mb_lane(&mbs[L.mbx > 0 ? aa - 1 : aa]);
    n.U = mb_lane(&mbs[L.mby > 0 ? aa - g.wmb : aa]);
#pragma unroll
    for (int l = 0; l < 2; ++l) {
        n.lmv[l] = b.mv[mbase + l * g.motion_plane + li];
        n.lri[l] = b.ref_idx[mbase + l * g.motion_plane + li];
        n.umv[l] = b.mv[mbase + l * g.motion_plane + ui];
        n.uri[l] = b.ref_idx[mbase + l * g.motion_plane + ui];
    }
    return n;
}

DEV int sel16(uint32_t lo, uint32_t hi, int c) { return (int16_t)(((c & 2) ? hi : lo) >> (16 * (c & 1))); }

// ---------------------------------------------------------------- packed 16-bit helpers
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
DEV s16x2 as_s16x2(uint32_t v) { return __builtin_bit_cast(s16x2, v); }
DEV uint32_t as_u32(s16x2 v) { return __builtin_bit_cast(uint32_t, v); }
DEV s16x2 splat16(short v) { return (s16x2){v, v}; }
DEV s16x2 pk_max(s16x2 a, s16x2 b) { return __builtin_elementwise_max(a, b); }
DEV s16x2 pk_min(s16x2 a, s16x2 b) { return __builtin_elementwise_min(a, b); }
DEV s16x2 pk_clip255(s16x2 a) { return pk_min(pk_max(a, splat16(0)), splat16(255)); }
// {a's low half, b's low half} / {a's high half, b's high half}
DEV s16x2 pk_lo(uint32_t a, uint32_t b) { return as_s16x2(__builtin_amdgcn_perm(b, a, 0x05040100u)); }
DEV s16x2 pk_hi(uint32_t a, uint32_t b) { return as_s16x2(__builtin_amdgcn_perm(b, a, 0x07060302u)); }
// {a, b} saturated to 16 bits each
DEV s16x2 pk_sat(int a, int b) { return __builtin_bit_cast(s16x2, __builtin_amdgcn_cvt_pk_i16(a, b)); }
// idct4 (device_common.h) on both halves
DEV void idct4_pk(s16x2& a, s16x2& b, s16x2& c, s16x2& d)
{
    const s16x2 e0 = a + c, e1 = a - c, e2 = (b >> splat16(1)) - d, e3 = b + (d >> splat16(1));
    a = e0 + e3; b = e1 + e2; c = e1 - e2; d = e0 - e3;
}
// dq4 (device_common.h) + 2^27 as an unsigned value, for every 32-bit product: the sign bit flipped
// is + 2^31 before a logical shift.  The low 16 bits are dq4's, and |dq4| = |u - 2^27| is one
// v_sad_u32 (no wrap: |dq4| <= 2^27, so 16 of them sum below 2^32).
constexpr uint32_t DQ4_BIAS = 1u << 27;
DEV uint32_t dq4_biased(int lev, int scale, int per) { return ((uint32_t)(lev * scale) * (1u << per) + 0x80000008u) >> 4; }
DEV uint32_t abs_acc_biased(uint32_t u, uint32_t acc)
{
    uint32_t r;
    asm("v_sad_u32 %0, %1, %2, %3" : "=v"(r) : "v"(u), "s"(DQ4_BIAS), "v"(acc));
    return r;
}
// The packed 16-bit inverse transforms below are exact when the block's 16 dequantised coefficients
// have sum |d| <= PK_RES_MAX.  Each 1-D pass (idct4) forms its intermediates and outputs from its
// four inputs with weights of magnitude <= 1 (|x >> 1| <= |x|), so after the first pass an entry is
// at most its line's sum |d|, and every intermediate and output of the second pass at most the sum
// of those, the block's sum |d|.  The rounding is folded in as +32 on d[0][0] before the first pass:
// the DC takes only the unshifted e0 / e1 = d0 +- d2 paths, so every output gains exactly 32, as
// (x + 32) >> 6 asks.  With it no value leaves [-32732, 32732], inside int16.  The sum is taken on
// the 32-bit values (a coefficient past int16 fails it like a large sum does).
constexpr uint32_t PK_RES_MAX = 32700;
// Construction of one row of four samples: prediction bytes + residual pairs {0, 1}, {2, 3}
// (saturated to 16 bits, pk_sat: the clip to 0..255 decides the same), clipped.
DEV uint32_t construct4(uint32_t pred, s16x2 r01, s16x2 r23)
{
    const s16x2 p01 = as_s16x2(__builtin_amdgcn_perm(0, pred, 0x0c010c00u)), p23 = as_s16x2(__builtin_amdgcn_perm(0, pred, 0x0c030c02u));
    const s16x2 s01 = pk_clip255(__builtin_elementwise_add_sat(p01, r01)), s23 = pk_clip255(__builtin_elementwise_add_sat(p23, r23));
    return __builtin_amdgcn_perm(as_u32(s23), as_u32(s01), 0x06040200u);
}
// (p[k], p[k+1]) of the 9 row samples held as bytes in r0 = p0..p3, r1 = p4..p7, r2 = p8
template <int K>
DEV s16x2 pair_at(uint32_t r0, uint32_t r1, uint32_t r2)
{
    constexpr uint32_t sel = K < 3 ? (0x0c000c00u | ((K + 1) << 16) | K)
                           : K == 3 ? 0x0c040c03u
                           : K < 7 ? (0x0c000c00u | ((K - 3) << 16) | (K - 4))
                           : 0x0c040c03u;
    return as_s16x2(K < 4 ? __builtin_amdgcn_perm(r1, r0, sel) : __builtin_amdgcn_perm(r2, r1, sel));
}

// clip3(0, hi, x) for a wave-uniform hi >= 0 as one v_med3_i32 (H264R_INTER_MC bit 0).  clip3's
// ternaries compile to a minimum, a compare and a select: the compiler may not assume 0 <= hi.
DEV int clip0(int hi, int x)
{
    if constexpr (!(H264R_INTER_MC & 1)) return clip3(0, hi, x);
    int r;
    asm("v_med3_i32 %0, %1, 0, %2" : "=v"(r) : "v"(x), "s"(hi));
    return r;
}

// The 16 luma prediction samples of one 4x4 block at integer position (x, y) and
// quarter phase (xf, yf): spec 8.4.2.2.1 / reference get_block_luma
// (inter_prediction.cc:158-340).  The 9 window rows y-2..y+6 are loaded at once and
// streamed; per row the unrounded horizontal 6-tap b1 of columns 0..3 is computed
// once (packed 16-bit pairs, exact: |b1| <= 10710) and feeds both b (rows 2..6) and
// the centre j of every output row it is a tap of (32-bit); the vertical 6-tap h of
// column c + 2 (+1 for xf == 3: m) accumulates in packed 16-bit.  Every output is
// (X + Y + 1) >> 1 of two of {G, b, h, j}, chosen per lane from the phase.
// out[i] packs row i's four samples as bytes.
// The 9 window rows of one lane straight from the reference plane (three aligned dwords
// per row from clip(x - 2) & ~3, row index clamped).
DEV void luma_window_global(const uint8_t* __restrict__ img, int W, int pitch, int H, int x, int y, uint32_t (&w)[9][3])
{
    const int a = clip0(W - 1, x - 2) & ~3;             // (row_dwords, device_common.h, with clip0)
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const gdword* q = as_global(img + (size_t)clip0(H - 1, y - 2 + r) * pitch + a);
        w[r][0] = q[0]; w[r][1] = q[1]; w[r][2] = q[2];
    }
}

// (The LDS reference-tile variant of round 3 -- one 13-row tile per 8x8 quadrant by LDS-DMA,
// measured slower, profiles/r03_e_ab.txt -- is gone, and since round 5 so is its never-taken
// branch, which had steered k_inter4r's register allocation: each output row is finished as
// soon as its last tap row is in, so its accumulators are free for the rest of the window and
// the kernel fits 128 VGPRs without it.)
// A window that crosses the picture's left or right edge, rewritten in place (H264R_INTER_MC bit 2): row r's
// dwords become the clamped samples 0..3, 4..7 and 8 (byte 0), which is what the interior extraction of
// luma_block_pred gives at shift 0.  The clamped column k sits at byte idx[k] = clip(x - 2 + k) - a of the row's
// 12 bytes; idx never steps by more than one, so samples 0..3 lie in one pair of neighbouring dwords and samples
// 4..8 in one: a byte permute each, the selectors and the pairs chosen once per lane (chroma_block_pred2's way).
// The caller runs it under its lane's !inside: a wave with no such lane skips it whole, column clamps included.
DEV void luma_window_edge(uint32_t (&w)[9][3], int W, int x)
{
    // opaque to the compiler, so that the column arithmetic is not moved out in front of the caller's branch,
    // where every wave would execute it
    asm volatile("" : "+v"(x));
    const int a = clip0(W - 1, x - 2) & ~3;
    int idx[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) idx[k] = clip0(W - 1, x - 2 + k) - a;      // 0 .. 11
    const bool hi0 = idx[0] >= 4, hi1 = idx[4] >= 4;                       // the pair is dwords {1, 2}, not {0, 1}
    const int o0 = hi0 ? 4 : 0, o1 = hi1 ? 4 : 0;
    uint32_t sel0 = 0, sel1 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        sel0 |= (uint32_t)(idx[k] - o0) << (8 * k);
        sel1 |= (uint32_t)(idx[4 + k] - o1) << (8 * k);
    }
    const uint32_t sel2 = 0x0c0c0c00u | (uint32_t)(idx[8] - o1);
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const uint32_t lo0 = hi0 ? w[r][1] : w[r][0], up0 = hi0 ? w[r][2] : w[r][1];
        const uint32_t lo1 = hi1 ? w[r][1] : w[r][0], up1 = hi1 ? w[r][2] : w[r][1];
        w[r][0] = __builtin_amdgcn_perm(up0, lo0, sel0);
        w[r][1] = __builtin_amdgcn_perm(up1, lo1, sel1);
        w[r][2] = __builtin_amdgcn_perm(up1, lo1, sel2);
    }
}

// w: not const -- an edge lane's window is rewritten in place (luma_window_edge).
// ONCE: bit 2 of H264R_INTER_MC applies (the PLAIN stages).  The generic stages keep the per-row form: without the
// per-row branches their nine rows are one basic block, which the scheduler interleaves past k_inter4r's 96 VGPRs
// (6 spilled; 1 with a scheduling barrier per row: profiles/r13_a_inter_edge_isa.txt).
template <bool ONCE>
DEV void luma_block_pred(uint32_t (&w)[9][3], int W, int x, int xf, int yf, uint32_t (&out)[4])
{
    constexpr int MC = ONCE ? H264R_INTER_MC : (H264R_INTER_MC & ~4);
    const int hs = xf == 3 ? 1 : 0;                  // G / h column c + 2 + hs
    const int brow = yf == 3 ? 1 : 0;                // b / G row i + 2 + brow
    const bool inside = x - 2 >= 0 && x + 6 < W;
    int sh = (x - 2) & 3;
    if constexpr (MC & 4) {
        // the edge lanes fix their window up once, here; the row loop below is then the interior extraction
        // for every lane, with no branch in it
        if (!inside) {
            luma_window_edge(w, W, x);
            sh = 0;
        }
    }
    // output = (X + Y + 1) >> 1, X, Y in {0 G, 1 b, 2 h, 3 j}: (xs, ys) of the 16 phases as a
    // 64-bit table (an if-chain on the lane's phase compiled to lane-divergent branches)
    // XSYS nibble 4 xf + yf = xs | ys << 2:  xf 0: (0,0) (0,2) (2,2) (0,2); yf 0: (0,1) (1,1)
    // (0,1); xf 2: (1,3) (3,3) (1,3); yf 2: (2,3); else (1,2)
    constexpr uint64_t XSYS = 0x9e94dfd59e948a80ull;
    const int xsys = (int)(XSYS >> (4 * (xf * 4 + yf))) & 15, xs = xsys & 3, ys = xsys >> 2;
    // one of four by masks (a ternary chain became a branch tree)
    const uint32_t mx1 = 0u - (uint32_t)(xs & 1), mx2 = 0u - (uint32_t)(xs >> 1);
    const uint32_t my1 = 0u - (uint32_t)(ys & 1), my2 = 0u - (uint32_t)(ys >> 1);
    auto pick = [](uint32_t m1, uint32_t m2, uint32_t a, uint32_t b, uint32_t c, uint32_t d) -> uint32_t {
        const uint32_t lo = a ^ ((a ^ b) & m1), hi = c ^ ((c ^ d) & m1);
        return lo ^ ((lo ^ hi) & m2);
    };
    s16x2 hacc[4][2], bsv[4][2], gsv[4][2];
    // the centre j's vertical 6-tap over b1 (|sum| < 2^20) in packed fp32, exact below 2^24:
    // two columns per v_pk_fma_f32 instead of one 32-bit multiply-add each
    f32x2 jacc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
            hacc[i][h2] = bsv[i][h2] = gsv[i][h2] = splat16(0);
            jacc[i][h2] = (f32x2){0.f, 0.f};
        }
    }
    constexpr short C6[6] = {1, -5, 20, 20, -5, 1};
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        uint32_t r0, r1, r2;
        if ((MC & 4) || inside) {
            r0 = __builtin_amdgcn_alignbyte(w[r][1], w[r][0], sh);
            r1 = __builtin_amdgcn_alignbyte(w[r][2], w[r][1], sh);
            r2 = w[r][2] >> (8 * sh);
        } else {                                       // window crosses the picture edge: clamp per sample
            int p[9];
            row9(w[r][0], w[r][1], w[r][2], x, W, p);
            r0 = p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24);
            r1 = p[4] | (p[5] << 8) | (p[6] << 16) | ((uint32_t)p[7] << 24);
            r2 = p[8];
        }
        const s16x2 q0 = pair_at<0>(r0, r1, r2), q1 = pair_at<1>(r0, r1, r2), q2 = pair_at<2>(r0, r1, r2);
        const s16x2 q3 = pair_at<3>(r0, r1, r2), q4 = pair_at<4>(r0, r1, r2), q5 = pair_at<5>(r0, r1, r2);
        const s16x2 q6 = pair_at<6>(r0, r1, r2), q7 = pair_at<7>(r0, r1, r2);
        const s16x2 b01 = (q0 + q5) + splat16(20) * (q2 + q3) - splat16(5) * (q1 + q4);   // b1 cols 0,1
        const s16x2 b23 = (q2 + q7) + splat16(20) * (q4 + q5) - splat16(5) * (q3 + q6);   // b1 cols 2,3
        const s16x2 g01 = hs ? q3 : q2, g23 = hs ? q5 : q4;                                // G column pairs
        const f32x2 bf[2] = {(f32x2){(float)b01.x, (float)b01.y}, (f32x2){(float)b23.x, (float)b23.y}};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = r - i;                       // tap index of row r for output row i
            if (k < 0 || k > 5) continue;
            hacc[i][0] += splat16(C6[k]) * g01;
            hacc[i][1] += splat16(C6[k]) * g23;
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2)
                jacc[i][h2] = __builtin_elementwise_fma((f32x2){(float)C6[k], (float)C6[k]}, bf[h2], jacc[i][h2]);
            if (k == 2 || k == 3) {                    // b / G of output row i: row i + 2 + brow
                const bool take = k == 2 + brow;
                bsv[i][0] = take ? b01 : bsv[i][0];
                bsv[i][1] = take ? b23 : bsv[i][1];
                gsv[i][0] = take ? g01 : gsv[i][0];
                gsv[i][1] = take ? g23 : gsv[i][1];
            }
        }
        // output row i has all its taps after row i + 5: finished here, its accumulators free
        if (r >= 5) {
            const int i = r - 5;
            uint32_t o2[2];
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
                const s16x2 G = gsv[i][h2];
                const s16x2 hh = pk_clip255((hacc[i][h2] + splat16(16)) >> splat16(5));
                const s16x2 bb = pk_clip255((bsv[i][h2] + splat16(16)) >> splat16(5));
                // (j1 + 512) >> 10 clipped: j1 / 1024 + 0.5 is exact, and truncation equals the
                // floor wherever the clip does not send the value to 0 anyway
                const f32x2 jf = __builtin_elementwise_fma(jacc[i][h2], (f32x2){1.f / 1024.f, 1.f / 1024.f}, (f32x2){0.5f, 0.5f});
                const int j0 = (int)__builtin_amdgcn_fmed3f(jf.x, 0.f, 255.f), j1 = (int)__builtin_amdgcn_fmed3f(jf.y, 0.f, 255.f);
                // all four computed, then picked per lane (the phase differs between lanes)
                const uint32_t g32 = as_u32(G), b32 = as_u32(bb), h32 = as_u32(hh), j32 = (uint32_t)j0 | ((uint32_t)j1 << 16);
                const s16x2 X = as_s16x2(pick(mx1, mx2, g32, b32, h32, j32));
                const s16x2 Y = as_s16x2(pick(my1, my2, g32, b32, h32, j32));
                o2[h2] = as_u32((X + Y + splat16(1)) >> splat16(1));
            }
            out[i] = __builtin_amdgcn_perm(o2[1], o2[0], 0x06040200u);
        }
    }
}

// 2x2 chroma prediction samples at chroma integer position (xi, yi), eighth phase
// (xf, yf): get_block_chroma inter_prediction.cc:380-404 with clamped coordinates.
// Both planes; each plane's four samples as bytes (row 0 in bits 0..15, row 1 in 16..31).
// A row's three clamped samples come out of its two dwords by one byte permute (the
// selector computed once per lane), and the two samples of an output row are one packed
// 16-bit sum: (8-xf)(8-yf) + xf(8-yf) + (8-xf)yf + xf yf = 64, so 255 * 64 + 32 fits.
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
DEV u16x2 as_u16x2(uint32_t v) { return __builtin_bit_cast(u16x2, v); }
DEV void chroma_block_pred2(const uint8_t* __restrict__ cb, const uint8_t* __restrict__ cr, int W, int pitch, int H, int xi,
                            int yi, int xf, int yf, uint32_t (&out)[2])
{
    const int a = clip0(W - 1, xi) & ~3;
    // both planes' three rows first (12 dwords in flight): a lane-divergent interior / edge
    // split made every row's load wait for the previous row's use, and one plane at a time
    // left the second plane's last row behind a full vmcnt wait
    uint32_t w[2][3][2];
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const gdword* q = as_global((pl ? cr : cb) + (size_t)clip0(H - 1, yi + k) * pitch + a);
            w[pl][k][0] = q[0];
            w[pl][k][1] = q[1];
        }
    // byte c (c = 0..2) of the selector: the clamped column's byte in {dword 0 (0..3), dword 1
    // (4..7)}; byte 3 reads zero
    uint32_t sel = 0x0c000000u;
#pragma unroll
    for (int c = 0; c < 3; ++c) sel |= (uint32_t)(clip0(W - 1, xi + c) - a) << (8 * c);
    const u16x2 wa = (u16x2)(unsigned short)((8 - xf) * (8 - yf)), wb = (u16x2)(unsigned short)(xf * (8 - yf));
    const u16x2 wc = (u16x2)(unsigned short)((8 - xf) * yf), wd = (u16x2)(unsigned short)(xf * yf);
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
        u16x2 A[3], B[3];                       // row k: {p[k][0], p[k][1]} and {p[k][1], p[k][2]}
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint32_t r = __builtin_amdgcn_perm(w[pl][k][1], w[pl][k][0], sel);
            A[k] = as_u16x2(__builtin_amdgcn_perm(r, r, 0x0c010c00u));
            B[k] = as_u16x2(__builtin_amdgcn_perm(r, r, 0x0c020c01u));
        }
        uint32_t o[2];
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const u16x2 v = (wa * A[rr] + wb * B[rr] + wc * A[rr + 1] + wd * B[rr + 1] + (u16x2)(unsigned short)32) >> (u16x2)(unsigned short)6;
            o[rr] = __builtin_bit_cast(uint32_t, v);
        }
        out[pl] = __builtin_amdgcn_perm(o[1], o[0], 0x06040200u);
    }
}

// mc_prediction / bi_prediction combine (inter_prediction.cc:53-156) of one lane and
// plane as w0 * v0 + w1 * v1, rounded right shift by d (rshift_rnd :35-38), + o, with the
// reference's case split resolved once per plane instead of per sample: one list unweighted
// {1, 0 | 0, 1; d 0}, one list explicit {w, 0 | 0, w; logWD; o}, both lists unweighted
// {1, 1; 1}, explicit {w0, w1; logWD + 1; (o0 + o1 + 1) >> 1}, implicit {64 - w1, w1;
// logWD + 1 = 6}.  The slice's weights are loaded together, not per sample behind branches.
struct WpPar {
    int w0, w1, o, d, rnd;
};
// The slice's weights and offsets of both lists' references, all three planes, loaded
// together (per-plane loads behind the case split below waited for each other: three round
// trips per MB in weighted slices)
struct WpRaw {
    int lwd[2];
    int wa[3], wb[3], oa[3], ob[3];
    int iw;
};
DEV WpRaw wp_raw(const h264r_slice* __restrict__ sl, int r0, int r1)
{
    const int ra = clip3(0, H264R_MAX_REFS - 1, r0), rb = clip3(0, H264R_MAX_REFS - 1, r1);   // unused list: any entry
    WpRaw w;
    w.lwd[0] = sl->luma_log2_wd;
    w.lwd[1] = sl->chroma_log2_wd;
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
        w.wa[pl] = sl->wp_weight[0][ra][pl];
        w.wb[pl] = sl->wp_weight[1][rb][pl];
        w.oa[pl] = sl->wp_offset[0][ra][pl];
        w.ob[pl] = sl->wp_offset[1][rb][pl];
    }
    w.iw = sl->implicit_w1[ra][rb];
    return w;
}
DEV WpPar wp_params(const WpRaw& w, int wp_mode, int dir, int pl)
{
    const int lwd = w.lwd[pl ? 1 : 0];
    const int wa = w.wa[pl], wb = w.wb[pl], oa = w.oa[pl], ob = w.ob[pl], iw = w.iw;
    // selects, not branches (dir and the slice's mode differ between a wave's lanes): one
    // list (explicit weights or plain), both lists averaged, explicit or implicit
    WpPar p;
    const bool ex = wp_mode == 1, im = wp_mode == 2, bi = dir == 2;
    p.w0 = bi ? (ex ? wa : (im ? 64 - iw : 1)) : (dir == 0 ? (ex ? wa : 1) : 0);
    p.w1 = bi ? (ex ? wb : (im ? iw : 1)) : (dir == 1 ? (ex ? wb : 1) : 0);
    p.o = bi ? (ex ? (oa + ob + 1) >> 1 : 0) : (ex ? (dir == 0 ? oa : ob) : 0);
    p.d = bi ? (wp_mode == 0 ? 1 : lwd + 1) : (ex ? lwd : 0);
    p.rnd = p.d > 0 ? 1 << (p.d - 1) : 0;
    return p;
}
// 4 packed samples of each list
DEV uint32_t wp_apply4(const WpPar& p, uint32_t v0, uint32_t v1)
{
    uint32_t o = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int x = p.w0 * (int)((v0 >> (8 * c)) & 255) + p.w1 * (int)((v1 >> (8 * c)) & 255);
        o |= (uint32_t)clip255(((x + p.rnd) >> p.d) + p.o) << (8 * c);
    }
    return o;
}
// The combine of 4 packed samples: weighted prediction off is byte-wise SWAR.
DEV uint32_t wp_combine4(const WpPar& p, int wp_mode, int dir, uint32_t v0, uint32_t v1)
{
    if (wp_mode == 0) {
        // one list or (a + b + 1) >> 1 per byte, selected (dir differs between a wave's lanes)
        const uint32_t avg = (v0 | v1) - (((v0 ^ v1) >> 1) & 0x7F7F7F7Fu);
        return dir == 0 ? v0 : (dir == 1 ? v1 : avg);
    }
    return wp_apply4(p, v0, v1);
}

// 4-point inverse transform of one column / row held in registers, (x + 32) >> 6 at
// the end of the second pass (inverse_4x4 transform.cc:597-641).
DEV void idct4_inplace(int& a, int& b, int& c, int& d)
{
    int o0, o1, o2, o3;
    idct4(a, b, c, d, o0, o1, o2, o3);
    a = o0; b = o1; c = o2; d = o3;
}
// rows then columns of a 4x4 block in registers
DEV void idct4x4_inplace(int (&d)[4][4])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) idct4_inplace(d[i][0], d[i][1], d[i][2], d[i][3]);
#pragma unroll
    for (int c = 0; c < 4; ++c) idct4_inplace(d[0][c], d[1][c], d[2][c], d[3][c]);
}

// QpY (pl 0) / QpC[pl - 1] of a record, from its dwords 0 and 1
DEV int mb_qp(const h264r_mb& m, int pl)
{
    const uint32_t w0 = reinterpret_cast<const uint32_t*>(&m)[0], w1 = reinterpret_cast<const uint32_t*>(&m)[1];
    return pl == 0 ? (int)(int8_t)(w0 >> 24) : (int)(int8_t)(w1 >> (8 * (pl - 1)));
}

// A list without motion as motion_word would give it (ref_idx -1, no slot, zero mv), without the
// table read.
DEV uint2 inter4_no_list() { return make_uint2(0, 0xFFFFu); }
// True when no lane's block, left block or upper block has list-1 motion: every ref_idx of list 1 is
// negative and every mv word of it zero (P pictures, and the waves of a B picture that predict from
// list 0 alone).  The list-1 motion words of those blocks are then all inter4_no_list().
DEV bool inter4_one_list(const Inter4Pre& pre, const DbNb& nb)
{
    const bool used = (pre.ri[1] & nb.lri[1] & nb.uri[1]) >= 0 || (pre.mv[1] | nb.lmv[1] | nb.umv[1]) != 0;
    return !__any(used);
}

// A picture is PLAIN when it has at most INTER4_PLAIN_SLICES slices, each of them P or I with
// default weights (wp_mode 0): its waves may take the PLAIN stages.  The workgroup works it out
// beside its LDS fill, whose first threads hold the slice headers anyway: thread t < 8 marks slice t
// (inter4_plain_mark, before the barrier), every wave reads the 8 marks back after it.
// n: the picture's num_slices.
static_assert(offsetof(Inter4Lds, not_plain) % 8 == 0 && INTER4_PLAIN_SLICES == 8, "the marks are read as one uint2");
DEV void inter4_plain_mark(Inter4Lds& S, int t, uint2 hdr, int n)
{
    const uint32_t type = hdr.x & 255, wp = hdr.y & 255;                            // slice_type, wp_mode
    if (t < INTER4_PLAIN_SLICES) S.not_plain[t] = t < n && ((type != H264R_SLICE_P && type != H264R_SLICE_I) || wp != 0);
}
DEV bool inter4_plain_picture(const h264r_batch& b, const Inter4Lds& S, int n)
{
    const uint2 m = *reinterpret_cast<const uint2*>(S.not_plain);
    return n >= 1 && n <= min(b.slice_stride, INTER4_PLAIN_SLICES) && __builtin_amdgcn_readfirstlane(m.x | m.y) == 0;
}
// What a wave of a plain picture must find before it takes the PLAIN stages; a wave that does not
// takes the generic stages instead (k_recon.hip k_inter4r).  No conforming stream fails it:
//   - inter4_one_list: the one-list records, and list 0 alone in the prediction;
//   - every slice index in reach (mine, my left and upper MB's) is one of the picture's ns slices,
//     which inter4_plain_picture vouches for (and so in the LDS copy);
//   - every block of an inter MB has a list-0 ref_idx (the generic path predicts a block without
//     one from list 1: zeros).
DEV bool inter4_plain_wave(const Inter4Pre& pre, const DbNb& nb, int ns)
{
    const bool far = (int)pre.q.slice >= ns || (int)nb.L.slice >= ns || (int)nb.U.slice >= ns;
    const bool noref = !mb_is_intra(pre.q) && pre.ri[0] < 0;
    return inter4_one_list(pre, nb) && !__any(far || noref);
}

// The record of dbinfo_block once the motion of the block (mq), of its left (ml) and of its upper
// neighbour (mu) is resolved.  ONE: the wave compares one list (bs_compare_one).
template <bool ONE>
DEV void dbinfo_records(const h264r_mb& q, const h264r_mb& L, const h264r_mb& U, const MotionRef& mq, const MotionRef& ml,
                        const MotionRef& mu, int blk, int hasL, int hasU, uint32_t qsh0, int l_type, int u_type, int fld,
                        const DbTables& T, DbInfo* __restrict__ out)
{
    const int bx = blk & 3, by = blk >> 2;
    const int q_type = qsh0 & 255, idc = (qsh0 >> 8) & 255;
    const int offa = (int8_t)((qsh0 >> 16) & 255), offb = (int8_t)(qsh0 >> 24);
    const int mvlim = fld ? 2 : 4;
    const int q_intra = mb_is_intra(q);
    const int fl = idc == 0 ? hasL : (idc == 2 && hasL && L.slice == q.slice);
    const int ft = idc == 0 ? hasU : (idc == 2 && hasU && U.slice == q.slice);
    const int t8 = (q.flags & H264R_MBF_T8x8) != 0;
    const int pskip = q_type == H264R_SLICE_P && q.mb_type == H264R_P_SKIP;
    const int special_q = special_slice(q_type);
#pragma unroll
    for (int hor = 0; hor < 2; ++hor) {
        const int e = hor ? by : bx, s = hor ? bx : by;
        const int en = idc != 1 && (e == 0 ? (hor ? ft : fl) : ((e & 1) ? !t8 : 1));
        int v = 0;
        if (en) {
            // MB P of the edge: the left / upper MB for edge 0, else this MB
            const int p_flags = e == 0 ? (hor ? U.flags : L.flags) : q.flags;
            const int p_cbp = e == 0 ? (hor ? U.cbp_blks : L.cbp_blks) : q.cbp_blks;
            const int special = special_q || (e == 0 && special_slice(hor ? u_type : l_type));
            const int intra = q_intra || (p_flags & H264R_MBF_INTRA) != 0;
            const int blkQ = 4 * by + bx;
            const int blkP = hor ? (e == 0 ? 12 + bx : blkQ - 4) : (e == 0 ? blkQ + 3 : blkQ - 1);
            const int coded = ((q.cbp_blks >> blkQ) & 1) || ((p_cbp >> blkP) & 1);
            const int same_part = e > 0 && (q.mb_type == H264R_P_16x16 ||
                                            q.mb_type == (hor ? H264R_P_8x16 : H264R_P_16x8));
            if (!hor) {
                if (special) v = e == 0 ? 4 : 3;
                else if (e > 0 && pskip) v = 0;
                else if (e == 0 && intra) v = 4;
                else if (intra) v = 3;
                else if (coded) v = 2;
                else if (same_part) v = 0;
                else v = ONE ? bs_compare_one(mq, ml, mvlim) : bs_compare(mq, ml, mvlim);
            } else {
                if (e == 0 && !fld && (special || intra)) v = 4;
                else if (special || intra) v = 3;
                else if (e > 0 && pskip) v = 0;
                else if (coded) v = 2;
                else if (same_part) v = 0;
                else v = ONE ? bs_compare_one(mq, mu, mvlim) : bs_compare(mq, mu, mvlim);
            }
        }
        out->bs[hor * 16 + e * 4 + s] = (uint8_t)v;
    }
    if (blk < 9) {                                              // edge parameters
        const int pl = blk / 3, which = blk - pl * 3;
        // QP of plane pl from the record's dwords 0 / 1 (a select between the byte fields
        // became a select of their addresses: the record went to memory, promoted to LDS)
        const h264r_mb& P = which == 0 ? L : (which == 1 ? U : q);
        const int qp = mb_qp(P, pl), qq = mb_qp(q, pl);
        out->par[blk] = edge_word(qp, qq, offa, offb, T.ab, T.tc0);
    }
}

// The deblocking record of one MB's 4x4 block (Deblock::strength deblock.cc:78-289,
// edge parameters :469-480): the block's left edge (vertical edge bx, segment by) and top
// edge (horizontal edge by, segment bx), and for blk < 9 one alpha/beta/tc0 word.  Inside
// k_inter4r, before the group's reconstruction.
// `one` (wave-uniform, inter4_one_list): no list-1 motion in reach of any lane; m1 is then
// inter4_no_list().
// PLAIN (a plain wave of k_inter4r): `one` holds and every slice is in the LDS copy, so only the one-list records are
// compiled.  Returns false, with nothing written, when the wave needs bs_compare after all: the
// caller runs the generic instantiation instead.  The generic instantiation always returns true.
template <bool PLAIN = false>
DEV bool dbinfo_block(const h264r_batch& b, int pic, const Inter4Lane& ln, const Inter4Lds& S, const DbTables& T,
                      const h264r_mb& q, uint2 m0, uint2 m1, uint2 qsh, const DbNb& nb, DbInfo* __restrict__ dbout, bool one)
{
    const int bx = ln.bx, by = ln.by;
    const h264r_slice* slices = b.slices + (size_t)pic * b.slice_stride;
    const int hasL = ln.mbx > 0, hasU = ln.mby > 0;
    const h264r_mb& L = nb.L;
    const h264r_mb& U = nb.U;
    // the neighbour block belongs to this MB or to the left / upper one (its slice resolves it)
    const int lsl = bx > 0 ? q.slice : L.slice, usl = by > 0 ? q.slice : U.slice;
    const uint2 l0 = motion_word<PLAIN>(nb.lmv[0], nb.lri[0], slices, S, lsl, 0);
    const uint2 u0 = motion_word<PLAIN>(nb.umv[0], nb.uri[0], slices, S, usl, 0);
    uint2 l1 = inter4_no_list(), u1 = l1;
    if constexpr (!PLAIN) {
        if (!one) {
            l1 = motion_word(nb.lmv[1], nb.lri[1], slices, S, lsl, 1);
            u1 = motion_word(nb.umv[1], nb.uri[1], slices, S, usl, 1);
        }
    }
    const int l_type = slice_type_of<PLAIN>(slices, S, L.slice), u_type = slice_type_of<PLAIN>(slices, S, U.slice);
    // field pictures: mvlimit 2 (deblock.cc:86,164) and no bS 4 across horizontal MB edges
    // (cond_bS4 = !field || vertical, deblock.cc:103-107,184-189)
    const int fld = (int)__builtin_amdgcn_readfirstlane(ld_const(&b.pics[pic].structure)) != H264R_FRAME;
    // ---- deblocking record (Deblock::strength deblock.cc:78-289): this lane's
    // left edge (vertical edge bx, segment by) and top edge (horizontal edge by,
    // segment bx)
    const MotionRef mq = motion_of(m0, m1), ml = motion_of(l0, l1), mu = motion_of(u0, u1);
    // bs_compare_one also needs a list-0 reference on one side of every edge it is asked about.
    // Only edges between two inter MBs reach the comparison, so an inter MB's block without one
    // (no conforming stream has it: ref_idx out of range, or an empty RefPicList entry) sends
    // the wave to bs_compare.
    const bool both_missing = !mb_is_intra(q) && mq.ref[0] < 0 && (ml.ref[0] < 0 || mu.ref[0] < 0);
    if constexpr (PLAIN) {
        if (__any(ln.valid && both_missing)) return false;
    }
    if (ln.valid) {
        DbInfo* out = dbout + ln.aa;
        if constexpr (PLAIN) {
            dbinfo_records<true>(q, L, U, mq, ml, mu, ln.blk, hasL, hasU, qsh.x, l_type, u_type, fld, T, out);
        } else {
            if (one) one = !__any(both_missing);
            if (one) dbinfo_records<true>(q, L, U, mq, ml, mu, ln.blk, hasL, hasU, qsh.x, l_type, u_type, fld, T, out);
            else dbinfo_records<false>(q, L, U, mq, ml, mu, ln.blk, hasL, hasU, qsh.x, l_type, u_type, fld, T, out);
        }
    }
    return true;
}

// ------------------------------------------------------------------ the stages of inter4_mbs
// I_PCM: the samples as the level buffer holds them (mb_pred_ipcm decoder.cc:149-168)
DEV void inter4_pcm(uint8_t* rmb, const Inter4Lane& L, const int16_t* lv)
{
    const uint8_t* raw = reinterpret_cast<const uint8_t*>(lv);
#pragma unroll
    for (int r = 0; r < 4; ++r)
        *reinterpret_cast<uint32_t*>(rmb + L.yoff + r * 16) = *reinterpret_cast<const uint32_t*>(raw + (L.by * 4 + r) * 16 + L.bx * 4);
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
#pragma unroll
        for (int r = 0; r < 2; ++r)
            *reinterpret_cast<uint16_t*>(rmb + L.coff + pl * 64 + r * 8) =
                *reinterpret_cast<const uint16_t*>(raw + 256 + pl * 64 + (L.by * 2 + r) * 8 + L.bx * 2);
}

// The motion compensation of my block from one list (mw: its motion_word; rr: its ref_idx): tY[i] luma
// row i's four samples as bytes, tC[pl] my 2x2 chroma samples of plane pl (chroma_block_pred2); 128
// (no_ref, inter_prediction.cc:164-167,366-369) where the list's entry names no picture.  `use`: the
// lane predicts from this list at all.  structure / fld: the picture's, wave-uniform.
template <bool PLAIN>
DEV void inter4_mc(const Geom& g, const Inter4Lane& L, const Inter4Lds& S, int structure, int fld, uint2 mw, int rr, bool use,
                   uint32_t (&tY)[4], uint32_t (&tC)[2])
{
    tY[0] = tY[1] = tY[2] = tY[3] = 0x80808080u;
    tC[0] = tC[1] = 0x80808080u;
    const int ref = (int8_t)((mw.y >> 8) & 255);                // slot | H264R_REF_BOTTOM
    const int slot = ref & 31, bot = fld & (ref >> 6);
    const bool ok = use && ref >= 0 && (ref & ~H264R_REF_BOTTOM) < H264R_MAX_SLOTS && rr < H264R_MAX_REFS &&
                    S.planes[slot * 3];
    const int mvx = (int16_t)(mw.x & 0xFFFF), mvy = (int16_t)(mw.x >> 16);
    const int vx = L.X4 * 16 + mvx, vy = L.Y4 * 16 + mvy;       // quarter luma / eighth chroma units
    const int x = vx >> 2, y = vy >> 2;
    {
        // the 9 window rows of the lane's own block, straight from the plane
        uint32_t w[9][3];
        if constexpr (H264R_INTER_DIAG & 4) {
            // diagnostic build (wrong output): no window loads, no luma filter
            tY[0] = tY[1] = tY[2] = tY[3] = (uint32_t)(vx ^ vy);
        } else {
            if (ok) luma_window_global(S.planes[slot * 3] + bot * g.W, g.W, g.W << fld, g.H, x, y, w);
            if constexpr (H264R_INTER_DIAG & 2) {
                // diagnostic build (wrong output): the window loads without the luma filter
                if (ok) {
                    uint32_t acc = 0;
#pragma unroll
                    for (int r = 0; r < 9; ++r) acc ^= w[r][0] ^ w[r][1] ^ w[r][2];
                    tY[0] = tY[1] = tY[2] = tY[3] = acc;
                }
            } else {
                if (ok) luma_block_pred<PLAIN>(w, g.W, x, vx & 3, vy & 3, tY);
            }
        }
    }
    // a reference field of the other parity: the chroma sample grid sits a quarter
    // chroma row off (get_block_chroma inter_prediction.cc:352-355)
    const int vyc = vy + (fld && bot != (structure == H264R_BOTTOM_FIELD) ? (bot ? -2 : 2) : 0);
    if constexpr (H264R_INTER_DIAG & 8) {
        tC[0] = tC[1] = (uint32_t)vyc;        // diagnostic build (wrong output): no chroma MC
    } else {
        if (ok) chroma_block_pred2(S.planes[slot * 3 + 1] + bot * g.Wc, S.planes[slot * 3 + 2] + bot * g.Wc, g.Wc,
                                   g.Wc << fld, g.Hc, vx >> 3, vyc >> 3, vx & 7, vyc & 7, tC);
    }
}

// The prediction of my block: the motion compensation of each list it uses (m0 / m1: motion_word),
// combined by the slice's weighted prediction (qs, wp_mode).  predY[i]: luma row i's four samples as
// bytes; predC[pl]: my 2x2 chroma samples of plane pl (chroma_block_pred2).
// PLAIN (a plain wave of k_inter4r): the caller's lanes all predict from list 0 alone with default weights, so the
// prediction is list 0's motion compensation: no list loop, no per-list copies, no combine.
template <bool PLAIN = false, bool PARK = false>
DEV void inter4_predict(const h264r_batch& b, const Geom& g, int pic, const Inter4Lane& L, const Inter4Lds& S,
                        const h264r_slice* __restrict__ qs, int wp_mode, uint2 m0, uint2 m1, uint32_t (&predY)[4],
                        uint32_t (&predC)[2], Inter4Park* park = nullptr)
{
    // a field picture (include/h264r.h H264R_TOP_FIELD) reads fields of the DPB frames:
    // every second row from the field's first row, clamped to the field's own rows
    const int structure = (int)__builtin_amdgcn_readfirstlane(ld_const(&b.pics[pic].structure));
    // an MBAFF picture of a mixed batch counts as a field picture here and in dbinfo_block
    const int fld = structure != H264R_FRAME;
    const int r0 = (int8_t)(m0.y & 255);
    if constexpr (PLAIN) {
        inter4_mc<true>(g, L, S, structure, fld, m0, r0, true, predY, predC);
        return;
    }
    const int r1 = (int8_t)(m1.y & 255);
    const int dir = (r0 >= 0 && r1 >= 0) ? 2 : (r0 >= 0 ? 0 : 1);
    if constexpr (PARK) {
        park_put(*park, PARK_M1, m1.x);
        park_put(*park, PARK_M1 + 1, m1.y);
    }
    // the prediction of each list in named registers: an array indexed by the (not
    // unrolled) list loop was promoted to LDS by the compiler (48 B per lane)
    uint32_t pY[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, pC[2][2] = {{0, 0}, {0, 0}};
    bool parked[2] = {false, false};                                // wave-uniform: list l's prediction is in `park`
#pragma unroll 1
    for (int l = 0; l < 2; ++l) {
        const int rr = l ? r1 : r0;
        const bool use = rr >= 0;
        if (!__any(use)) continue;                                  // P pictures: list 1 never
        uint2 mw = l ? m1 : m0;
        if constexpr (PARK)
            if (l) mw = make_uint2(park_get(*park, PARK_M1), park_get(*park, PARK_M1 + 1));
        uint32_t tY[4], tC[2];
        inter4_mc<false>(g, L, S, structure, fld, mw, rr, use, tY, tC);
        const bool l1 = l != 0;
        if constexpr (PARK) {
            // each list's prediction goes to LDS as it is finished and both come back after the loop:
            // nothing of either is live across a motion compensation, and the loop carries no
            // prediction registers (Inter4Park)
#pragma unroll
            for (int i = 0; i < 4; ++i) park_put(*park, PARK_PRED + 6 * l + i, use ? tY[i] : 0);
#pragma unroll
            for (int k = 0; k < 2; ++k) park_put(*park, PARK_PRED + 6 * l + 4 + k, use ? tC[k] : 0);
            parked[0] |= !l1;
            parked[1] |= l1;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                pY[0][i] = (use && !l1) ? tY[i] : pY[0][i];
                pY[1][i] = (use && l1) ? tY[i] : pY[1][i];
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                pC[0][k] = (use && !l1) ? tC[k] : pC[0][k];
                pC[1][k] = (use && l1) ? tC[k] : pC[1][k];
            }
        }
    }
    if constexpr (PARK) {
#pragma unroll
        for (int l = 0; l < 2; ++l)
            if (parked[l]) {                                        // the lanes that wrote, and no others
#pragma unroll
                for (int i = 0; i < 4; ++i) pY[l][i] = park_get(*park, PARK_PRED + 6 * l + i);
#pragma unroll
                for (int k = 0; k < 2; ++k) pC[l][k] = park_get(*park, PARK_PRED + 6 * l + 4 + k);
            }
    }
    WpPar wpp[3] = {};
    if (wp_mode != 0) {
        // PARK: qs is the picture's slice table, and the slice index comes back with the parked record
        if constexpr (PARK) qs += park_get(*park, PARK_Q + 2) >> 16;
        const WpRaw wr = wp_raw(qs, r0, r1);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) wpp[pl] = wp_params(wr, wp_mode, dir, pl);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) predY[i] = wp_combine4(wpp[0], wp_mode, dir, pY[0][i], pY[1][i]);
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) predC[pl] = wp_combine4(wpp[1 + pl], wp_mode, dir, pC[0][pl], pC[1][pl]);
}

// The residual inputs of my block.  Luma: the 16 levels and scales of my 4x4 block, or of my 4x4
// quadrant of a T8x8 MB's 8x8 block, raster, four 16-bit values per dword pair.  Chroma, per plane: rows
// cr, cr + 1 of my quadrant (two 16-bit values per dword), the plane's four DC levels and the DC scale.
// Zero where the MB codes nothing.
struct Inter4Res {
    uint4 lev[2], lsc[2];
    uint32_t clev[2][2], csc[2][2];
    uint2 cdc[2];
    int cdcs[2];
};
DEV Inter4Res inter4_res_load(const h264r_mb& q, const Inter4Lane& L, const int16_t* lv, const h264r_quant* __restrict__ qt)
{
    Inter4Res R = {};
    const int cbpc = q.cbp >> 4, qpl = q.qp_scaled[0];
    const int by = L.by, bx = L.bx;
    const int loff = b8_offset(q.cbp, L.b8);
    if (loff >= 0) {
        if (!(q.flags & H264R_MBF_T8x8)) {      // 4x4 block: 16 raster levels
            const uint4* p = reinterpret_cast<const uint4*>(lv + loff + ((by & 1) * 2 + (bx & 1)) * 16);
            R.lev[0] = p[0]; R.lev[1] = p[1];
            const uint4* s = reinterpret_cast<const uint4*>(&qt->scale4x4[1][0][qpl % 6][0]);
            R.lsc[0] = s[0]; R.lsc[1] = s[1];
        } else {                                // my 4x4 quadrant of the 8x8 block: rows (by&1)*4.., cols (bx&1)*4..
            const int16_t* p = lv + loff + (by & 1) * 32 + (bx & 1) * 4;
            const int16_t* s = &qt->scale8x8[1][0][qpl % 6][(by & 1) * 32 + (bx & 1) * 4];
            const uint2 r0 = ld8(p), r1 = ld8(p + 8), r2 = ld8(p + 16), r3 = ld8(p + 24);
            R.lev[0] = make_uint4(r0.x, r0.y, r1.x, r1.y); R.lev[1] = make_uint4(r2.x, r2.y, r3.x, r3.y);
            const uint2 s0 = ld8(s), s1 = ld8(s + 8), s2 = ld8(s + 16), s3 = ld8(s + 24);
            R.lsc[0] = make_uint4(s0.x, s0.y, s1.x, s1.y); R.lsc[1] = make_uint4(s2.x, s2.y, s3.x, s3.y);
        }
    }
    if (cbpc) {
        const LevelOffs lo = level_offsets(q);
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            const int qpc = q.qp_scaled[1 + pl];
            R.cdc[pl] = ld8(lv + lo.cdc + pl * 4);
            R.cdcs[pl] = qt->scale4x4[1][1 + pl][qpc % 6][0];
            if (cbpc == 2) {
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    R.clev[pl][r] = *reinterpret_cast<const uint32_t*>(lv + lo.cac + pl * 64 + L.cb * 16 + (L.cr + r) * 4 + L.cc);
                    R.csc[pl][r] = *reinterpret_cast<const uint32_t*>(&qt->scale4x4[1][1 + pl][qpc % 6][(L.cr + r) * 4 + L.cc]);
                }
            }
        }
    }
    return R;
}
// Luma level / scale (i, c) of my block
DEV int res_at(const uint4 (&w)[2], int i, int c) { return sel16((i & 1) ? w[i >> 1].z : w[i >> 1].x, (i & 1) ? w[i >> 1].w : w[i >> 1].y, c); }
DEV int level_at(const Inter4Res& R, int i, int c) { return res_at(R.lev, i, c); }
DEV int scale_at(const Inter4Res& R, int i, int c) { return res_at(R.lsc, i, c); }
// dq4 / dq8 (transform.cc:394-419) as one form, rounding and shift per lane: the lanes of a wave
// mix 4x4 and 8x8 MBs, and a select per value (not a branch) keeps the 16 values free of
// exec-mask work
DEV void luma_dequant(const Inter4Res& R, int per, int t8, int (&d)[4][4])
{
    const int drnd = t8 ? 32 : 8, dsh = t8 ? 6 : 4;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) d[i][c] = ((level_at(R, i, c) * scale_at(R, i, c)) * (1 << per) + drnd) >> dsh;
}
// the 32-bit paths' result, saturated (pk_sat)
DEV void pack_res(const int (&res)[4][4], s16x2 (&rp)[4][2])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        rp[i][0] = pk_sat(res[i][0], res[i][1]);
        rp[i][1] = pk_sat(res[i][2], res[i][3]);
    }
}

// Lossless MBs (TransformBypassModeFlag): the levels are the residual, DPCM'd in place down
// the columns / along the rows when the block's Intra4x4PredMode / Intra8x8PredMode is vertical /
// horizontal (bypass_4x4 / bypass_8x8 transform.cc:736-778; inverse_transform_4x4 / _8x8 :986-1016
// read those modes for inter MBs too: whatever the parser's mb_t slot holds).  The flag is
// uniform over an MB's 16 lanes, so the cross-lane carries stay inside the caller's branch.
// qg: the MB's record in the batch -- its prediction modes are read from there, inside this (rare)
// branch, and not kept in two registers across the motion compensation of every MB.
DEV void luma_res_bypass(const h264r_mb* __restrict__ qg, const Inter4Lane& L, const Inter4Res& R, int t8, s16x2 (&rp)[4][2])
{
    const int bx = L.bx, by = L.by;
    int d[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) d[i][c] = level_at(R, i, c);
    const uint32_t* qw = reinterpret_cast<const uint32_t*>(qg);
    static_assert(offsetof(h264r_mb, ipred) == 20, "dwords 5 and 6 of the record");
    const uint64_t ipw = (uint64_t)qw[5] | ((uint64_t)qw[6] << 32);
    const int bk = t8 ? L.b8 : (by >> 1) * 8 + (bx >> 1) * 4 + (by & 1) * 2 + (bx & 1);
    const int mode = (int)((ipw >> (4 * bk)) & 15);
    const bool vert = mode == 0, horz = mode == 1;
#pragma unroll
    for (int i = 1; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) d[i][c] += vert ? d[i - 1][c] : 0;
#pragma unroll
    for (int c = 1; c < 4; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i][c] += horz ? d[i][c - 1] : 0;
    // 8x8: the quadrant above (lane ^ 4) / to the left (lane ^ 1) carries in
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int up = lane_xor4(d[3][c]);
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i][c] += (t8 && vert && (by & 1)) ? up : 0;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int left = lane_xor1(d[i][3]);
#pragma unroll
        for (int c = 0; c < 4; ++c) d[i][c] += (t8 && horz && (bx & 1)) ? left : 0;
    }
    pack_res(d, rp);
}

// 4x4 blocks in every lane of the wave: all in-lane.  PK: on 16-bit pairs when every lane's block
// passes PK_RES_MAX (real content does): rows 0, 1 and rows 2, 3 as the halves of two transforms, a
// 2x2 transpose of the pairs, then columns {0, 1} and {2, 3}
template <bool PK>
DEV void luma_res_4x4(const Inter4Res& R, int per, int t8, s16x2 (&rp)[4][2])
{
    bool pk = PK;
    uint32_t u[4][4];
    if (pk) {
        uint32_t gs = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                u[i][c] = dq4_biased(level_at(R, i, c), scale_at(R, i, c), per);
                gs = abs_acc_biased(u[i][c], gs);
            }
        pk = !__any(gs > PK_RES_MAX);
    }
    if (pk) {
        s16x2 A[4], B[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            A[c] = pk_lo(u[0][c], u[1][c]);
            B[c] = pk_lo(u[2][c], u[3][c]);
        }
        A[0] += (s16x2){32, 0};
        idct4_pk(A[0], A[1], A[2], A[3]);
        idct4_pk(B[0], B[1], B[2], B[3]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            s16x2 x0 = pk_lo(as_u32(A[2 * h]), as_u32(A[2 * h + 1])), x1 = pk_hi(as_u32(A[2 * h]), as_u32(A[2 * h + 1]));
            s16x2 x2 = pk_lo(as_u32(B[2 * h]), as_u32(B[2 * h + 1])), x3 = pk_hi(as_u32(B[2 * h]), as_u32(B[2 * h + 1]));
            idct4_pk(x0, x1, x2, x3);
            rp[0][h] = x0 >> splat16(6); rp[1][h] = x1 >> splat16(6);
            rp[2][h] = x2 >> splat16(6); rp[3][h] = x3 >> splat16(6);
        }
    } else {
        // rows then columns, 32-bit (the biased values are the dequantised ones + 2^27,
        // exactly: taken back, not computed again, so that the range test keeps its
        // own shift-and-add)
        int d[4][4], res[4][4];
        if constexpr (PK) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 4; ++c) d[i][c] = (int)(u[i][c] - DQ4_BIAS);
        } else {
            luma_dequant(R, per, t8, d);
        }
        idct4x4_inplace(d);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) res[i][c] = (d[i][c] + 32) >> 6;
        pack_res(res, rp);
    }
}

// A wave with T8x8 MBs: their 8x8 transform across the four lanes of an 8x8 block; the 4x4 MBs of
// the same wave transform in-lane, 32-bit.  Rows: my 4 + the 4 of lane ^ 1.
DEV void luma_res_8x8(const Inter4Lane& L, const Inter4Res& R, int per, int t8, s16x2 (&rp)[4][2])
{
    const int bx = L.bx, by = L.by;
    int d[4][4], e4[4][4], res[4][4];
    luma_dequant(R, per, t8, d);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int in[8], outv[8];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int ov = lane_xor1(d[i][c]);
            in[c] = (bx & 1) ? ov : d[i][c];
            in[4 + c] = (bx & 1) ? d[i][c] : ov;
        }
        idct8(in, outv);
        // mask select: a ternary over the two halves became a lane-indexed array
        // read, which the compiler placed in LDS (32 B per lane)
        const int mx = -(bx & 1);
#pragma unroll
        for (int c = 0; c < 4; ++c) e4[i][c] = (outv[c] & ~mx) | (outv[4 + c] & mx);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        int in[8], outv[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            in[i] = lane_lo4(e4[i][c]);         // rows 0..3: the lane with by even
            in[4 + i] = lane_hi4(e4[i][c]);
        }
        idct8(in, outv);
        const int my = -(by & 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) res[i][c] = t8 ? ((outv[i] & ~my) | (outv[4 + i] & my)) : 0;
    }
    if (!t8) idct4x4_inplace(d);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) res[i][c] = ((t8 ? res[i][c] : d[i][c]) + 32) >> 6;
    pack_res(res, rp);
}

// Luma residual of my block (transform.cc:1058-1073): rp[i][h] = {row i's columns 2h, 2h + 1} as a
// 16-bit pair, what the construction takes (construct4).  (Each path dequantises for itself: the
// lossless one takes the levels, the 4x4 one a biased form its range test reads.)
// PARK (the generic stages of k_inter4r): the luma prediction predY waits in LDS while a wave with
// T8x8 MBs runs its 8x8 transform, the widest stage after the motion compensation (Inter4Park).
template <bool PK, bool PARK = false>
DEV void inter4_luma_residual(const h264r_mb& q, const h264r_mb* __restrict__ qg, const Inter4Lane& L, const Inter4Res& R,
                              s16x2 (&rp)[4][2], uint32_t (&predY)[4], Inter4Park* park = nullptr)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) rp[i][0] = rp[i][1] = splat16(0);
    if (!__any((q.cbp & 15) != 0)) return;
    const int t8 = (q.flags & H264R_MBF_T8x8) != 0, per = q.qp_scaled[0] / 6;
    if (q.flags & H264R_MBF_BYPASS) luma_res_bypass(qg, L, R, t8, rp);
    else if (!__any(t8 != 0)) luma_res_4x4<PK>(R, per, t8, rp);
    else {
        if constexpr (PARK) {
#pragma unroll
            for (int i = 0; i < 4; ++i) park_put(*park, PARK_PRED + i, predY[i]);
        }
        luma_res_8x8(L, R, per, t8, rp);
        if constexpr (PARK) {
#pragma unroll
            for (int i = 0; i < 4; ++i) predY[i] = park_get(*park, PARK_PRED + i);
        }
    }
}
// H264R_INTER_DIAG 64 (wrong output): the luma levels loaded, not transformed (16: R is empty)
DEV void luma_res_stub(const Inter4Res& R, s16x2 (&rp)[4][2])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) rp[i][0] = rp[i][1] = splat16(0);
    rp[0][0].x = (short)((R.lev[0].x ^ R.lev[0].y ^ R.lev[0].z ^ R.lev[0].w ^ R.lev[1].x ^ R.lev[1].y ^ R.lev[1].z ^ R.lev[1].w ^
                          R.lsc[0].x ^ R.lsc[1].y) & 3);
}

// Construction + store of my 4x4 luma block
DEV void inter4_store_luma(uint8_t* rmb, const Inter4Lane& L, const uint32_t (&predY)[4], const s16x2 (&rp)[4][2])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<uint32_t*>(rmb + L.yoff + i * 16) = construct4(predY[i], rp[i][0], rp[i][1]);
}
// H264R_INTER_DIAG 1 (wrong output): one 16-byte store per lane, an MB's 16 lanes contiguous
DEV void inter4_store_luma_16b(uint8_t* rmb, const Inter4Lane& L, const uint32_t (&predY)[4], const s16x2 (&rp)[4][2])
{
    uint32_t wv4[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) wv4[i] = construct4(predY[i], rp[i][0], rp[i][1]);
    *reinterpret_cast<uint4*>(rmb + L.blk * 16) = make_uint4(wv4[0], wv4[1], wv4[2], wv4[3]);
}

// A 4x4 block spread over the lanes {blk, ^1, ^4, ^5}, a 2x2 quadrant each (rows cr.., cols cc..):
// one 1-D pass Op (in place on four values: idct4_inplace, idct4_pk, fwd4_inplace) over the block's
// rows / columns.  a, b: my two values of the row / column, in and out.
DEV s16x2 lane_xor1(s16x2 v) { return as_s16x2((uint32_t)lane_xor1((int)as_u32(v))); }
DEV s16x2 lane_lo4(s16x2 v) { return as_s16x2((uint32_t)lane_lo4((int)as_u32(v))); }
DEV s16x2 lane_hi4(s16x2 v) { return as_s16x2((uint32_t)lane_hi4((int)as_u32(v))); }
// rows: my 2 columns + the 2 of lane ^ 1
template <auto Op, typename T>
DEV void quad_rows(T& a, T& b, int cc)
{
    const T o0 = lane_xor1(a), o1 = lane_xor1(b);
    T d0 = cc ? o0 : a, d1 = cc ? o1 : b, d2 = cc ? a : o0, d3 = cc ? b : o1;
    Op(d0, d1, d2, d3);
    a = cc ? d2 : d0;
    b = cc ? d3 : d1;
}
// columns: my 2 rows + the 2 of lane ^ 4 (rows 0..1 from the lane with by even, 2..3 from the other).
// XOR4: by lane_xor4 and a select (k_inter_sp's form) instead of lane_lo4 / lane_hi4 -- each kernel
// keeps the DPP forms the parity suite verified in it (tests/test_isa.py)
template <auto Op, bool XOR4 = false, typename T>
DEV void quad_cols(T& a, T& b, int cr)
{
    T d0, d1, d2, d3;
    if constexpr (XOR4) {
        const T o0 = lane_xor4(a), o1 = lane_xor4(b);
        d0 = cr ? o0 : a; d1 = cr ? o1 : b; d2 = cr ? a : o0; d3 = cr ? b : o1;
    } else {
        d0 = lane_lo4(a); d1 = lane_lo4(b); d2 = lane_hi4(a); d3 = lane_hi4(b);
    }
    Op(d0, d1, d2, d3);
    a = cr ? d2 : d0;
    b = cr ? d3 : d1;
}

// Chroma residual of my quadrant (transform.cc:1081-1091, DC :875-889): chroma block cb is spread
// over lanes {blk, ^1, ^4, ^5}; my quadrant rows cr.., cols cc..
// rcp[pl][r] = {row r's two samples of plane pl} as a 16-bit pair
template <bool PK>
DEV void inter4_chroma_residual(const h264r_mb& q, const Inter4Lane& L, const Inter4Res& R, s16x2 (&rcp)[2][2])
{
    const int cb = L.cb, cr = L.cr, cc = L.cc;
    const int cbpc = q.cbp >> 4;
    const bool byp = (q.flags & H264R_MBF_BYPASS) != 0;
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) rcp[pl][0] = rcp[pl][1] = splat16(0);
    if (!__any(cbpc != 0)) return;
    const bool dcl_lane = cr == 0 && cc == 0;
    // k: the dequantised coefficients + DQ4_BIAS (dq4_biased), the scaled DC among them
    uint32_t k[2][2][2];
    int dcl[2];
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
        const int qpc = q.qp_scaled[1 + pl], per = qpc / 6;
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 2; ++c)
                k[pl][r][c] = dq4_biased((int16_t)(R.clev[pl][r] >> (16 * c)), (int16_t)(R.csc[pl][r] >> (16 * c)), per);
        const int c00 = (int16_t)(R.cdc[pl].x & 0xFFFF), c01 = (int16_t)(R.cdc[pl].x >> 16);
        const int c10 = (int16_t)(R.cdc[pl].y & 0xFFFF), c11 = (int16_t)(R.cdc[pl].y >> 16);
        const int e00 = c00 + c01, e01 = c00 - c01, e10 = c10 + c11, e11 = c10 - c11;
        // f = (e00 or e01) +/- (e10 or e11) by cb's bits: arithmetic, not a branch tree
        const int ea = (cb & 1) ? e01 : e00, eb = (cb & 1) ? e11 : e10;
        const int f = ea + (eb ^ -(cb >> 1)) + (cb >> 1);
        if (dcl_lane) k[pl][0][0] = (uint32_t)(cbpc ? ((f * R.cdcs[pl]) * (1 << per)) >> 5 : 0) + DQ4_BIAS;
        dcl[pl] = cb == 0 ? c00 : cb == 1 ? c01 : cb == 2 ? c10 : c11;
    }
    // Both planes at once as {Cb, Cr} pairs when every block of the wave passes PK_RES_MAX
    // in both planes (the scaled DC included; lossless MBs do not use the transform).  A
    // block's sum is over its four lanes, of the larger of the lane's two plane sums: never
    // below either plane's own.  (|k| <= 2^27: no wrap.)
    bool pk = PK;
    if (pk) {
        uint32_t gs[2];
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
            gs[pl] = abs_acc_biased(k[pl][0][0], abs_acc_biased(k[pl][0][1], abs_acc_biased(k[pl][1][0], abs_acc_biased(k[pl][1][1], 0))));
        int m = byp ? 0 : (int)max(gs[0], gs[1]);
        int o = lane_xor1(m);
        asm volatile("" : "+v"(o));              // a move, not a fold into the add (tests/test_isa.py)
        m = (int)((uint32_t)m + (uint32_t)o);
        int lo = lane_lo4(m), hi = lane_hi4(m);
        asm volatile("" : "+v"(lo), "+v"(hi));
        pk = !__any((uint32_t)lo + (uint32_t)hi > PK_RES_MAX);
    }
    if (pk) {
        s16x2 K[2][2];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 2; ++c) K[r][c] = pk_lo(k[0][r][c], k[1][r][c]);
        K[0][0] += splat16(dcl_lane ? 32 : 0);   // the rounding, on both planes' DC
#pragma unroll
        for (int r = 0; r < 2; ++r) quad_rows<idct4_pk>(K[r][0], K[r][1], cc);
#pragma unroll
        for (int c = 0; c < 2; ++c) quad_cols<idct4_pk>(K[0][c], K[1][c], cr);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const uint32_t r0 = as_u32(K[r][0] >> splat16(6)), r1 = as_u32(K[r][1] >> splat16(6));
            rcp[0][r] = pk_lo(r0, r1);
            rcp[1][r] = pk_hi(r0, r1);
        }
    } else {
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            int t[2][2];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                t[r][0] = (int)(k[pl][r][0] - DQ4_BIAS);
                t[r][1] = (int)(k[pl][r][1] - DQ4_BIAS);
                quad_rows<idct4_inplace>(t[r][0], t[r][1], cc);
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) quad_cols<idct4_inplace>(t[0][c], t[1][c], cr);
#pragma unroll
            for (int r = 0; r < 2; ++r) rcp[pl][r] = pk_sat((t[r][0] + 32) >> 6, (t[r][1] + 32) >> 6);
        }
    }
    // lossless: the raw levels, DC at (0,0) (transform.cc:453-455,860); an inter MB's
    // intra_chroma_pred_mode is DC (macroblock_t::init slice_data.cc:482), so
    // bypass_chroma (:802-822) copies.  A row's two levels are its loaded word.
    if (byp) {
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            rcp[pl][0] = dcl_lane ? pk_hi((uint32_t)dcl[pl] << 16, R.clev[pl][0]) : as_s16x2(R.clev[pl][0]);
            rcp[pl][1] = as_s16x2(R.clev[pl][1]);
        }
    }
}
// H264R_INTER_DIAG 128 (wrong output): the chroma levels loaded, not transformed (16: R is empty)
DEV void chroma_res_stub(const Inter4Res& R, s16x2 (&rcp)[2][2])
{
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
        rcp[pl][0] = rcp[pl][1] = splat16(0);
        rcp[pl][0].x = (short)((R.clev[pl][0] ^ R.clev[pl][1] ^ R.csc[pl][0] ^ R.csc[pl][1] ^ R.cdc[pl].x ^ R.cdc[pl].y ^ (uint32_t)R.cdcs[pl]) & 3);
    }
}

// Construction + store of my 2x2 chroma samples of both planes
DEV void inter4_store_chroma(uint8_t* rmb, const Inter4Lane& L, const uint32_t (&predC)[2], const s16x2 (&rcp)[2][2])
{
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
        uint8_t* cdst = rmb + L.coff + pl * 64;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const s16x2 pr = as_s16x2(__builtin_amdgcn_perm(0, predC[pl], r ? 0x0c030c02u : 0x0c010c00u));
            const s16x2 sv = pk_clip255(__builtin_elementwise_add_sat(pr, rcp[pl][r]));
            *reinterpret_cast<uint16_t*>(cdst + r * 8) = (uint16_t)__builtin_amdgcn_perm(0, as_u32(sv), 0x0c0c0200u);
        }
    }
}

// The inter / I_PCM macroblocks a0 .. a0+3 of picture `pic` (k_inter4r; their deblocking records come
// first, dbinfo_block).  Inter MBs of SP slices are left out and flagged in *sp_flag (the launch
// tag): k_inter_sp's (mb_inter_sp.h).
// PLAIN: a wave of a plain picture (inter4_plain_picture) that passed inter4_plain_wave --
// P and I slices in the LDS copy, default weights, list 0 alone: no SP test, no list-1 motion word,
// and inter4_predict's one-list form; m0_plain is its list-0 motion word (the kernel's, for its records).
// park: the workgroup's Inter4Park, which the generic instantiation needs and the PLAIN one never touches.
template <bool PLAIN = false>
DEV void inter4_mbs(const h264r_batch& b, const Geom& g, int pic, int a0, int aend, int lane,
                    const Inter4Lds& S, int* sp_flag, const Inter4Pre& pre, uint8_t* __restrict__ recon, int tag,
                    Inter4Park* park = nullptr, uint2 m0_plain = make_uint2(0, 0))
{
    constexpr int DIAG = H264R_INTER_DIAG;
    constexpr bool PK = (H264R_INTER_FAST & 1) != 0;
    const Inter4Lane L = inter4_lane(g, a0, aend, lane);
    const h264r_slice* slices = b.slices + (size_t)pic * b.slice_stride;
    // MB record (inter4_pre: two 16-byte loads -- a struct copy becomes one byte load per field,
    // each waited on its own), its slice header and the motion of this block
    const h264r_mb q0 = pre.q;
    const uint2 qsh = slice_hdr<PLAIN>(slices, S, q0.slice);
    // (PLAIN: the caller's list-0 motion word, which its records needed anyway; formed here again it
    // was one with the caller's, and what both derive from it was kept across the records in scratch)
    const uint2 m0 = PLAIN ? m0_plain : motion_word<PLAIN>(pre.mv[0], pre.ri[0], slices, S, q0.slice, 0);
    uint2 m1 = inter4_no_list();
    if constexpr (!PLAIN) m1 = motion_word(pre.mv[1], pre.ri[1], slices, S, q0.slice, 1);

    const bool pcm = q0.mb_type == H264R_I_PCM;
    if (!L.valid || (mb_is_intra(q0) && !pcm)) return;                // intra: k_intra_* (lanes idle here)
    if constexpr (!PLAIN)
        if ((qsh.x & 255) == H264R_SLICE_SP && !mb_is_intra(q0)) { *sp_flag = tag; return; }   // k_inter_sp's
    if (pcm) { inter4_pcm(recon_mb(recon, g, pic, L.aa), L, b.levels + q0.coef_off); return; }

    uint32_t predY[4], predC[2];
    if constexpr (PLAIN) {
        inter4_predict<true>(b, g, pic, L, S, &slices[q0.slice], qsh.y & 255, m0, m1, predY, predC);
    } else {
        // the generic stages: the record waits in LDS (Inter4Park) and comes back as q below
        park_put_mb(*park, q0);
        inter4_predict<false, true>(b, g, pic, L, S, slices, qsh.y & 255, m0, m1, predY, predC, park);
    }
    h264r_mb q = q0;
    Inter4Lane Lr = L;
    if constexpr (!PLAIN) {
        // ... and the lane's roles are formed again from the lane (a few VALU instructions; kept, they
        // were spilled around the motion compensation)
        q = park_get_mb(*park);
        int ln = lane;
        asm volatile("" : "+v"(ln));
        Lr = inter4_lane(g, a0, aend, ln);
        // the chroma prediction waits out the luma residual (its 8x8 transform is the widest stage)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) park_put(*park, PARK_PRED + 4 + pl, predC[pl]);
    }
    // What only the residual and the stores read comes after the motion compensation, so that it is
    // not live across it: the residual inputs (30 VGPRs: with them k_inter4r first fitted 128 VGPRs;
    // config 3 475 -> 493 M MB/s, profiles/r03_h_inter_ab.txt) and the two 64-bit addresses (formed
    // before it, the kernel took 127 VGPRs instead of 125).  The generic stages go further to fit 96
    // (5 waves/SIMD): what they need after the compensation comes back from LDS or is formed again.
    Inter4Res R = {};
    if constexpr (!(DIAG & 16)) R = inter4_res_load(q, Lr, b.levels + q.coef_off, &b.quant[pic]);
    uint8_t* const rmb = recon_mb(recon, g, pic, Lr.aa);

    s16x2 rp[4][2];
    if constexpr (DIAG & (16 | 64)) luma_res_stub(R, rp);
    else inter4_luma_residual<PK, !PLAIN>(q, &b.mbs[(size_t)pic * g.nmb + Lr.aa], Lr, R, rp, predY, park);
    if constexpr (DIAG & 1) inter4_store_luma_16b(rmb, Lr, predY, rp);
    else inter4_store_luma(rmb, Lr, predY, rp);

    if constexpr (!PLAIN) {
        // ... and so does what the chroma residual reads of the record, which is still parked
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) predC[pl] = park_get(*park, PARK_PRED + 4 + pl);
        q = park_get_mb<2>(*park);
    }
    s16x2 rcp[2][2];
    if constexpr (DIAG & (16 | 128)) chroma_res_stub(R, rcp);
    else inter4_chroma_residual<PK>(q, Lr, R, rcp);
    inter4_store_chroma(rmb, Lr, predC, rcp);
}

}  // namespace h264r

