// device_common.h -- shared device helpers of the gfx950 reconstruction kernels.
//
// Canonical formats are those of include/h264r.h.  Every helper cites the
// reference lines whose arithmetic it reproduces (H/ = R/src/codec/h264/).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "h264r.h"
#include "kernels.h"

#define DEV __device__ __forceinline__

namespace h264r {

// --------------------------------------------------------------------- geometry
struct Geom {
    int wmb, hmb;          // picture size in MBs
    int W, H, Wc, Hc;      // plane sizes in samples
    int W4, H4;            // 4x4-block grid
    int nmb;               // W*H MBs
    size_t ysz, csz;       // plane sizes in bytes
    int motion_plane;      // 4x4 entries per list
};

DEV Geom make_geom(int wmb, int hmb)
{
    Geom g;
    g.wmb = wmb; g.hmb = hmb;
    g.W = wmb * 16; g.H = hmb * 16; g.Wc = wmb * 8; g.Hc = hmb * 8;
    g.W4 = wmb * 4; g.H4 = hmb * 4;
    g.nmb = wmb * hmb;
    g.ysz = (size_t)g.W * g.H; g.csz = (size_t)g.Wc * g.Hc;
    g.motion_plane = g.W4 * g.H4;
    return g;
}

DEV int clip3(int lo, int hi, int x) { return x < lo ? lo : (x > hi ? hi : x); }   // defines.h:48-52
DEV int clip255(int x) { return clip3(0, 255, x); }                                 // clip1, defines.h:54-58
DEV int iabs(int x) { return x < 0 ? -x : x; }

// Scalar (constant address space) load of data that no kernel of the batch writes
// (MB records, slice headers): a wave-uniform address becomes an s_load, issued back
// to back with the others and waited on lgkmcnt, not interleaved with vmcnt waits.
DEV uint32_t ld_const(const void* p) { return *(const __attribute__((address_space(4))) uint32_t*)p; }
DEV h264r_mb load_mb_const(const h264r_mb* p)
{
    h264r_mb m;
    uint32_t* w = reinterpret_cast<uint32_t*>(&m);
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = ld_const(reinterpret_cast<const uint32_t*>(p) + i);
    return m;
}

// Wave-level barrier for LDS scratch owned by one wave: orders this wave's LDS
// accesses across lanes without a workgroup barrier (other waves of the
// workgroup run independent work).  H264R_SYNC_NODRAIN drops the lgkmcnt(0)
// drain: a wave's LDS instructions execute in issue order, so only the compiler
// has to be kept from moving accesses across the barrier (measurement variant).
DEV void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#ifndef H264R_SYNC_NODRAIN
    __builtin_amdgcn_s_waitcnt(0xc07f);          // lgkmcnt(0): LDS ops of this wave done
#endif
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// XCD-local schedules (k_deblock, k_deblock2): a wave takes tickets only from its own
// XCD's counter tickets[k], so an XCD that no wave of the launch reached (a CU-masked
// stream, XCC ids that are not contiguous modulo nx) would leave its pictures unfiltered.
// Every wave passes here once, when its XCD's tickets have run out; the last one checks
// that every XCD's tickets were all taken (a counter that was reached ends past its item
// count) and flags err[0] = DEV_ERR_SCHEDULE otherwise -- a failure is never silent.  One-wave workgroups.
template <typename ItemsOf>
DEV void xcd_drain_check(const int* tickets, int* done, int nx, ItemsOf items_of, int* err)
{
    if (nx <= 1 || threadIdx.x != 0) return;
    const int prev = __hip_atomic_fetch_add(done, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (prev != (int)gridDim.x - 1) return;
    for (int k = 0; k < nx; ++k)
        if (__hip_atomic_load(&tickets[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < items_of(k))
            __hip_atomic_store(err, DEV_ERR_SCHEDULE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

DEV int mb_is_intra(const h264r_mb& m) { return (m.flags & H264R_MBF_INTRA) != 0; }

// ---------------------------------------------------------------- bounded waits
// Every cross-wave wait of the kernels (row hand-offs, the level barrier) is bounded in
// WALL time, not in polls: err[0] is the context's error word (h264r_check), err[1] the
// bound in s_memrealtime ticks (100 MHz), written by the host.  A wait gives up when its
// own bound has passed (it then flags err[0] = DEV_ERR_WAIT) or as soon as another wave has flagged
// an error, so one expired wait drains the whole grid within a few polls instead of
// every waiter behind it serving its own full bound (the round-2 hang: chained
// poll-count bounds of ~17 s each).  Checked every 64 polls (one scalar clock read).
struct WaitClock {
    uint64_t t0 = 0;
    uint32_t n = 0;
};
// true: stop waiting (the error is flagged)
DEV bool wait_give_up(int* err, WaitClock& c)
{
    if ((++c.n & 63u) != 1u) return false;
    const uint64_t now = __builtin_amdgcn_s_memrealtime();
    if (c.n == 1u) { c.t0 = now; return false; }
    if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return true;
    const uint32_t lim = (uint32_t)__hip_atomic_load(err + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (now - c.t0 <= (uint64_t)lim) return false;
    __hip_atomic_store(err, DEV_ERR_WAIT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}

// ----------------------------------------------------------- level block layout
// Section offsets of the compacted level block (include/h264r.h), int16 units.
struct LevelOffs {
    int b8[4];      // -1 if not coded
    int cac, ldc, cdc;
};

// Offset of coded 8x8 luma block k inside the level block, or -1 (register-only form
// of LevelOffs::b8 for a per-lane k).
DEV int b8_offset(int cbp, int k)
{
    const int cbpl = cbp & 15;
    return (cbpl >> k) & 1 ? 64 * __builtin_popcount(cbpl & ((1 << k) - 1)) : -1;
}

DEV LevelOffs level_offsets(const h264r_mb& m)
{
    LevelOffs o;
    int p = 0, cbpl = m.cbp & 15, cbpc = m.cbp >> 4;
    for (int k = 0; k < 4; ++k) { o.b8[k] = (cbpl >> k) & 1 ? p : -1; p += ((cbpl >> k) & 1) * 64; }
    o.cac = cbpc == 2 ? p : -1; p += cbpc == 2 ? 128 : 0;
    o.ldc = m.mb_type == H264R_I_16x16 ? p : -1; p += m.mb_type == H264R_I_16x16 ? 16 : 0;
    o.cdc = cbpc ? p : -1;
    return o;
}

// ----------------------------------------------------------- residual (transform.cc)
// Dequantise one 4x4 AC/luma level, inverse_quantize transform.cc:394-413.
DEV int dq4(int lev, int scale, int per) { return ((lev * scale) * (1 << per) + 8) >> 4; }
// 8x8: transform.cc:414-419.
DEV int dq8(int lev, int scale, int per) { return ((lev * scale) * (1 << per) + 32) >> 6; }

// 1-D 4-point inverse core transform, rows of inverse_4x4 (transform.cc:602-617).
DEV void idct4(int d0, int d1, int d2, int d3, int& o0, int& o1, int& o2, int& o3)
{
    int e0 = d0 + d2, e1 = d0 - d2, e2 = (d1 >> 1) - d3, e3 = d1 + (d3 >> 1);
    o0 = e0 + e3; o1 = e1 + e2; o2 = e1 - e2; o3 = e0 - e3;
}

// 1-D 8-point inverse transform (transform.cc:658-683).
DEV void idct8(const int* in, int* out)
{
    int e0 = in[0] + in[4];
    int e1 = -in[3] + in[5] - in[7] - (in[7] >> 1);
    int e2 = in[0] - in[4];
    int e3 = in[1] + in[7] - in[3] - (in[3] >> 1);
    int e4 = (in[2] >> 1) - in[6];
    int e5 = -in[1] + in[7] + in[5] + (in[5] >> 1);
    int e6 = in[2] + (in[6] >> 1);
    int e7 = in[3] + in[5] + in[1] + (in[1] >> 1);
    int f0 = e0 + e6, f1 = e1 + (e7 >> 2), f2 = e2 + e4, f3 = e3 + (e5 >> 2);
    int f4 = e2 - e4, f5 = (e3 >> 2) - e5, f6 = e0 - e6, f7 = e7 - (e1 >> 2);
    out[0] = f0 + f7; out[1] = f2 + f5; out[2] = f4 + f3; out[3] = f6 + f1;
    out[4] = f6 - f1; out[5] = f4 - f3; out[6] = f2 - f5; out[7] = f0 - f7;
}

// ---------------------------------------------------------------- motion comp.

// ------------------------------------------------------------ row-window MC
// The per-sample forms above fetch one byte per tap.  The MC path proper loads
// each reference row as three aligned dwords and extracts the samples it needs;
// clamping (the padded-plane equivalence of inter_prediction.cc:185-186) is
// applied to the row index always and to the column only for windows that
// cross the picture edge.  Reads may run up to 11 bytes past the last sample
// of a row: reference planes carry H264R_PLANE_SLACK bytes of slack.

// Samples ref(x-2+k, y), k = 0..8, of the row whose dwords w0..w2 start at
// a = clip(x-2) & ~3.
DEV void row9(uint32_t w0, uint32_t w1, uint32_t w2, int x, int W, int (&p)[9])
{
    if (x - 2 >= 0 && x + 6 < W) {
        const int s = (x - 2) & 3;
        const uint32_t r0 = __builtin_amdgcn_alignbyte(w1, w0, s);
        const uint32_t r1 = __builtin_amdgcn_alignbyte(w2, w1, s);
#pragma unroll
        for (int k = 0; k < 4; ++k) { p[k] = (r0 >> (8 * k)) & 255; p[4 + k] = (r1 >> (8 * k)) & 255; }
        p[8] = (w2 >> (8 * s)) & 255;
    } else {
        const int a = clip3(0, W - 1, x - 2) & ~3;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int idx = clip3(0, W - 1, x - 2 + k) - a;
            const uint32_t d = idx < 4 ? w0 : (idx < 8 ? w1 : w2);
            p[k] = (d >> (8 * (idx & 3))) & 255;
        }
    }
}

// Global-address-space view of a pointer whose address space the compiler cannot
// infer (a plane pointer read from LDS or picked per lane): loads through it are
// `global_load`, not `flat_load`.  A flat load counts on lgkmcnt as well as vmcnt and
// may return out of order, so every later LDS wait -- and every use of any load --
// would also wait for it (a prefetch would stop overlapping anything).
typedef const uint32_t __attribute__((address_space(1))) gdword;
DEV const gdword* as_global(const void* p) { return (const gdword*)p; }
template <typename T>
DEV T load_global(const void* p) { return *(const __attribute__((address_space(1))) T*)p; }

// pitch: W for a frame, 2 W for a field of a DPB frame (its rows are every second row,
// include/h264r.h H264R_REF_BOTTOM; the field's pointer starts at its first row)
DEV const gdword* row_dwords(const uint8_t* __restrict__ img, int W, int pitch, int H, int x, int y)
{
    const int a = clip3(0, W - 1, x - 2) & ~3;
    return as_global(img + (size_t)clip3(0, H - 1, y) * pitch + a);
}

// ---------------------------------------------------------------- deblocking
// Tables 8-16 / 8-17 (deblock.cc:294-324), packed alpha | beta<<8 | tc0[3]<<16.. in one word.
__device__ static const uint32_t DB_AB[52] = {
#define AB(a, b) ((uint32_t)(a) | ((uint32_t)(b) << 8))
    AB(0, 0), AB(0, 0), AB(0, 0), AB(0, 0), AB(0, 0), AB(0, 0), AB(0, 0), AB(0, 0), AB(0, 0), AB(0, 0),
    AB(0, 0), AB(0, 0), AB(0, 0), AB(0, 0), AB(0, 0), AB(0, 0), AB(4, 2), AB(4, 2), AB(5, 2), AB(6, 3),
    AB(7, 3), AB(8, 3), AB(9, 3), AB(10, 4), AB(12, 4), AB(13, 4), AB(15, 6), AB(17, 6), AB(20, 7), AB(22, 7),
    AB(25, 8), AB(28, 8), AB(32, 9), AB(36, 9), AB(40, 10), AB(45, 10), AB(50, 11), AB(56, 11), AB(63, 12), AB(71, 12),
    AB(80, 13), AB(90, 13), AB(101, 14), AB(113, 14), AB(127, 15), AB(144, 15), AB(162, 16), AB(182, 16), AB(203, 17), AB(226, 17),
    AB(255, 18), AB(255, 18)
#undef AB
};
__device__ static const uint32_t DB_TC0[52] = {
#define T(a, b, c) ((uint32_t)(a) | ((uint32_t)(b) << 8) | ((uint32_t)(c) << 16))
    T(0, 0, 0), T(0, 0, 0), T(0, 0, 0), T(0, 0, 0), T(0, 0, 0), T(0, 0, 0), T(0, 0, 0), T(0, 0, 0),
    T(0, 0, 0), T(0, 0, 0), T(0, 0, 0), T(0, 0, 0), T(0, 0, 0), T(0, 0, 0), T(0, 0, 0), T(0, 0, 0),
    T(0, 0, 0), T(0, 0, 1), T(0, 0, 1), T(0, 0, 1), T(0, 0, 1), T(0, 1, 1), T(0, 1, 1), T(1, 1, 1),
    T(1, 1, 1), T(1, 1, 1), T(1, 1, 1), T(1, 1, 2), T(1, 1, 2), T(1, 1, 2), T(1, 1, 2), T(1, 2, 3),
    T(1, 2, 3), T(2, 2, 3), T(2, 2, 4), T(2, 3, 4), T(2, 3, 4), T(3, 3, 5), T(3, 4, 6), T(3, 4, 6),
    T(4, 5, 7), T(4, 5, 8), T(4, 6, 9), T(5, 7, 10), T(6, 8, 11), T(6, 8, 13), T(7, 10, 14), T(8, 11, 16),
    T(9, 12, 18), T(10, 13, 20), T(11, 15, 23), T(13, 17, 25)
#undef T
};

// ------------------------------------------------------------- shared helpers
template <int K>
DEV int quad_bcast(int v)       // value of lane K of this lane's quad
{
    return __builtin_amdgcn_update_dpp(0, v, K * 0x55, 0xF, 0xF, false);
}

// The value of lane ^ 1 / lane ^ 4 (inside the lane's 16-lane row) by DPP moves: a VALU op or
// two instead of a ds_bpermute round trip through the LDS crossbar.  lane ^ 4: banks 1, 3 take
// row_shr:4 (lane - 4), banks 0, 2 row_shl:4 (lane + 4).
DEV int lane_xor1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false); }   // quad_perm [1,0,3,2]
DEV int lane_xor4(int v)
{
    const int t = __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xA, false);
    return __builtin_amdgcn_update_dpp(t, v, 0x104, 0xF, 0x5, false);
}

// The value of the lane of this lane's quad pair (lane, lane ^ 4) whose bit 2 is clear (lo) or
// set (hi): one banked DPP row shift each, keeping the own value in the other banks, where the
// exchange needed two moves plus a select per output.  (The pair (lane, lane ^ 1) form by
// quad_perm [0,0,2,2] / [1,1,3,3] gave wrong residuals inside k_inter4r once the compiler folded
// the moves into v_subrev_u32_dpp, a reversed opcode, to which MI355X applies the lane select on
// src1 instead of src0 (tools/dpp/dpp_fold_test.hip); not used.  tests/test_isa.py refuses any
// reversed opcode with DPP in the built library and holds the other forms -- these two's folds
// included -- to the set the GPU parity suite verified.)
DEV int lane_lo4(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x114, 0xF, 0xA, false); }   // banks 1, 3: lane - 4
DEV int lane_hi4(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x104, 0xF, 0x5, false); }   // banks 0, 2: lane + 4

// Column pass of inverse_4x4 (transform.cc:619-640) for the lane holding row r of
// the block: t[k] = row k's value in this column.  Returns ((o_r + 32) >> 6).
DEV int idct4_col_row(int t0, int t1, int t2, int t3, int r)
{
    const int e0 = t0 + t2, e1 = t0 - t2, e2 = (t1 >> 1) - t3, e3 = t1 + (t3 >> 1);
    const bool outer = r == 0 || r == 3;
    const int x = outer ? e0 : e1, y = outer ? e3 : e2;
    return ((r < 2 ? x + y : x - y) + 32) >> 6;
}

DEV uint2 ld8(const void* p) { return *reinterpret_cast<const uint2*>(p); }

// The reconstructed (pre-deblocking) samples of a launch, MB-tiled: per (picture, MB
// address) 384 contiguous bytes -- luma rows 0..15 x 16 B, then Cb and Cr rows 0..7 x 8 B.
// The reconstruction kernels write it and read their intra neighbours from it, the
// deblocking kernels read it and write the output planes (raster, the API's layout) --
// so the deblocking walk fetches whole 128-byte lines (a raster MB row piece is 16 B of a
// line the walk only comes back to after L2 has evicted it: 4x over-fetch, VERDICT r02
// weak 3) and k_inter4's stores of an MB fill its lines.
constexpr int RECON_MB = 384, RECON_CB = 256, RECON_CR = 320;

DEV uint8_t* recon_mb(uint8_t* R, const Geom& g, int pic, int addr)
{
    return R + ((size_t)pic * g.nmb + addr) * RECON_MB;
}
// luma sample (X, Y) / chroma sample (Xc, Yc) of plane pl: rows of 16 / 8 bytes
DEV uint8_t* recon_y(uint8_t* R, const Geom& g, int pic, int X, int Y)
{
    return recon_mb(R, g, pic, (Y >> 4) * g.wmb + (X >> 4)) + (Y & 15) * 16 + (X & 15);
}
DEV uint8_t* recon_c(uint8_t* R, const Geom& g, int pic, int pl, int Xc, int Yc)
{
    return recon_mb(R, g, pic, (Yc >> 3) * g.wmb + (Xc >> 3)) + RECON_CB + pl * 64 + (Yc & 7) * 8 + (Xc & 7);
}

}  // namespace h264r
