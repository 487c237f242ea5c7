// output_rgb.h -- the device code the RGB kernels share: k_output_rgb (k_output.hip), the
// k_output_rgb_scaled kernels (k_output_scale.hip) and the k_output_boxes kernels (k_output_boxes.hip).  The unaligned global loads, the 16-pixel source
// unit and its fetch (rgb_fetch_at), the matrix for one pixel (rgb_pixel), and the unit's way out: the
// format's bytes, interleaved in registers and stored as widely as the destination allows.  There is one
// fetch and one conversion; what differs between the kernels is how a row's address and a partial
// unit's samples are obtained, and that is a policy type each kernel hands to the fetch (RgbSrc,
// ScaleSrc).  Everything is inlined; neither kernel's registers depend on the other.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace h264r {

// The planes are global memory, but their pointers come out of the frame table, where the compiler
// cannot see that: the loads name the address space (global_load_*, not flat_load_*), and the
// alignment of 1.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef u32x4 __attribute__((aligned(1))) u32x4_u;
typedef u32x2 __attribute__((aligned(1))) u32x2_u;
#define H264R_GLOBAL __attribute__((address_space(1)))

__device__ __forceinline__ uint4 ld16u(const uint8_t* p)
{
    const u32x4 v = *(const H264R_GLOBAL u32x4_u*)p;
    return make_uint4(v.x, v.y, v.z, v.w);
}

__device__ __forceinline__ uint2 ld8u(const uint8_t* p)
{
    const u32x2 v = *(const H264R_GLOBAL u32x2_u*)p;
    return make_uint2(v.x, v.y);
}

__device__ __forceinline__ uint8_t ld1(const uint8_t* p)
{
    return *(const H264R_GLOBAL uint8_t*)p;
}

struct RgbUnit {
    int r, x, n;               // output row, first pixel, pixels (0: no unit)
    uint4 y;                   // 16 luma samples
    uint4 ua, va, ub, vb;      // chroma rows A (j0) and B (j1, RGB_BIL2 only): SubWidthC 1: 16 samples;
                               // SubWidthC 2: samples 0..7 in .x .y, the clamped sample 8 in .z
};

constexpr uint32_t RGB_GREY = 0x80808080u;

// The row R of a plane of the woven frame: nullptr = a row of 128 (the missing parity of an unpaired field).
__device__ __forceinline__ const uint8_t* rgb_row(const uint8_t* p0, const uint8_t* p1, int R, int pitch, int kind)
{
    const int fill_parity = kind == H264R_OUT_UNPAIRED_TOP ? 1 : kind == H264R_OUT_UNPAIRED_BOT ? 0 : -1;
    if ((R & 1) == fill_parity) return nullptr;
    const uint8_t* const p = (kind == H264R_OUT_FIELD_PAIR && (R & 1)) ? p1 : p0;
    return p + (int64_t)(kind != H264R_OUT_FRAME ? R >> 1 : R) * pitch;
}

// cnt samples from s[first], indices clamped to last, bytewise: the partial unit's fetch
__device__ __forceinline__ uint4 rgb_ld_clamped(const uint8_t* s, int first, int last, int cnt)
{
    // the nv samples that exist, off one address; the clamped ones behind them repeat the last
    const uint8_t* const p = s + first;
    const int nv = min(cnt, last - first + 1);
    const uint32_t rep = (uint32_t)ld1(p + nv - 1) * 0x01010101u;
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int m = 0; m < 16; ++m)
        if (m < nv) w[m >> 2] |= (uint32_t)ld1(p + m) << (8 * (m & 3));
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int have = nv - 4 * q;                        // bytes of w[q] that exist
        if (have < 4) w[q] |= have <= 0 ? rep : rep & (0xffffffffu << (8 * have));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// rgb_ld_clamped's sixteen bytes, by a loop instead of sixteen predicated loads whose lane masks would
// be kept in SGPRs across the rows: from the last sample that exists down to the first, each pushed in
// at the bottom of 128 bits that start as the repeated last sample.  Narrow crops only.
__device__ __forceinline__ uint4 scale_ld_clamped(const uint8_t* s, int first, int last, int cnt)
{
    const uint8_t* const p = s + first;
    const int nv = min(cnt, last - first + 1);
    const uint32_t rep = (uint32_t)ld1(p + nv - 1) * 0x01010101u;
    uint32_t w0 = rep, w1 = rep, w2 = rep, w3 = rep;
#pragma unroll 1
    for (int m = nv - 1; m >= 0; --m) {
        w3 = (w3 << 8) | (w2 >> 24);
        w2 = (w2 << 8) | (w1 >> 24);
        w1 = (w1 << 8) | (w0 >> 24);
        w0 = (w0 << 8) | (uint32_t)ld1(p + m);
    }
    return make_uint4(w0, w1, w2, w3);
}

// rgb_row with the frame's kind as two integers instead of three lane masks: the parity of the rows of
// 128 (-1: none) and whether a plane holds every second row.  p1 is p0 unless the frame is a field
// pair, so the row's parity alone picks the plane.
struct ScaleKind {
    int fill_parity, half;
};

__device__ __forceinline__ ScaleKind scale_kind(int kind)
{
    ScaleKind k;
    k.fill_parity = kind == H264R_OUT_UNPAIRED_TOP ? 1 : kind == H264R_OUT_UNPAIRED_BOT ? 0 : -1;
    k.half = kind != H264R_OUT_FRAME ? 1 : 0;
    return k;
}

__device__ __forceinline__ const uint8_t* scale_row(const uint8_t* p0, const uint8_t* p1, int R, int pitch, ScaleKind kind)
{
    if ((R & 1) == kind.fill_parity) return nullptr;
    return ((R & 1) ? p1 : p0) + (int64_t)(R >> kind.half) * pitch;
}

// Where a unit's samples come from, for rgb_fetch_at: row() is the address of row R of a plane of the
// woven frame, ld_clamped() a partial unit's samples.  RgbSrc is k_output_rgb's; ScaleSrc the scaled
// kernels', which have no SGPRs to spare for RgbSrc's lane masks.
struct RgbSrc {
    int kind;
    __device__ __forceinline__ const uint8_t* row(const uint8_t* const (&p)[2], int R, int pitch) const { return rgb_row(p[0], p[1], R, pitch, kind); }
    static __device__ __forceinline__ uint4 ld_clamped(const uint8_t* s, int first, int last, int cnt) { return rgb_ld_clamped(s, first, last, cnt); }
};

struct ScaleSrc {
    ScaleKind kind;
    __device__ __forceinline__ const uint8_t* row(const uint8_t* const (&p)[2], int R, int pitch) const { return scale_row(p[0], p[1], R, pitch, kind); }
    static __device__ __forceinline__ uint4 ld_clamped(const uint8_t* s, int first, int last, int cnt) { return scale_ld_clamped(s, first, last, cnt); }
};

// One chroma row's samples for the unit at chroma column i0: s = the row at the crop's first column.
template <class SRC>
__device__ __forceinline__ uint4 rgb_ld_chroma(const uint8_t* s, int i0, int cw, int mode, bool whole)
{
    if (!s) return make_uint4(RGB_GREY, RGB_GREY, RGB_GREY, RGB_GREY);
    const bool wide = mode < RGB_REP;
    if (!whole) return SRC::ld_clamped(s, i0, cw - 1, wide ? 16 : 9);
    if (wide) return ld16u(s + i0);
    const uint2 a = ld8u(s + i0);
    const uint32_t next = mode >= RGB_BIL1 ? ld1(s + min(i0 + 8, cw - 1)) : 0u;
    return make_uint4(a.x, a.y, next, 0u);
}

// The unit of RGB_UNIT source pixels of row r of the cropped rectangle from column x on (even where
// SubWidthC is 2): every load it needs.  The caller has set t.r, t.x and t.n = min(RGB_UNIT, lw - x).
template <int MODE, class SRC>
__device__ __forceinline__ void rgb_fetch_at(const RgbJob& J, SRC src, const uint8_t* const (&yp)[2], const uint8_t* const (&up)[2],
                                             const uint8_t* const (&vp)[2], RgbUnit& t)
{
    const bool whole = t.n == RGB_UNIT;
    const uint8_t* const ys = src.row(yp, J.y0 + t.r, J.lpitch);
    if (!ys) t.y = make_uint4(RGB_GREY, RGB_GREY, RGB_GREY, RGB_GREY);
    else if (whole) t.y = ld16u(ys + J.x0 + t.x);
    else t.y = SRC::ld_clamped(ys + J.x0, t.x, J.lw - 1, RGB_UNIT);
    if (MODE == RGB_MONO) return;
    // the chroma rows j0 (and j1) of the cropped rectangle, and the unit's first chroma column
    const int i0 = MODE < RGB_REP ? t.x : t.x >> 1;
    int ja = t.r, jb = t.r;
    if (MODE >= RGB_REP && J.sub_h == 2) {
        ja = t.r >> 1;
        jb = (t.r & 1) ? min(ja + 1, J.ch - 1) : max(ja - 1, 0);
    }
    const uint8_t* const ur = src.row(up, J.cy0 + ja, J.cpitch);
    const uint8_t* const vr = src.row(vp, J.cy0 + ja, J.cpitch);
    t.ua = rgb_ld_chroma<SRC>(ur ? ur + J.cx0 : nullptr, i0, J.cw, MODE, whole);
    t.va = rgb_ld_chroma<SRC>(vr ? vr + J.cx0 : nullptr, i0, J.cw, MODE, whole);
    if (MODE == RGB_BIL2) {
        const uint8_t* const ub = src.row(up, J.cy0 + jb, J.cpitch);
        const uint8_t* const vb = src.row(vp, J.cy0 + jb, J.cpitch);
        t.ub = rgb_ld_chroma<SRC>(ub ? ub + J.cx0 : nullptr, i0, J.cw, MODE, whole);
        t.vb = rgb_ld_chroma<SRC>(vb ? vb + J.cx0 : nullptr, i0, J.cw, MODE, whole);
    }
}

__device__ __forceinline__ int rgb_byte(const uint4& v, int k)
{
    const uint32_t w = (k >> 2) == 0 ? v.x : (k >> 2) == 1 ? v.y : (k >> 2) == 2 ? v.z : v.w;
    return (int)((w >> (8 * (k & 3))) & 0xffu);
}

// clip255(v >> 17), clamped BEFORE the shift: min(max(v, 0), 2^25 - 1) >> 17 is the same number, and it
// keeps the compiler from fusing shift and clamp of two pixels into gfx950's v_ashr_pk_u8_i32
__device__ __forceinline__ int rgb_clip255_sh17(int v) { return (int)((uint32_t)min(max(v, 0), (256 << 17) - 1) >> 17); }

// Pixel k of the unit: R, G, B by the header's matrix (RGB_GBR: the three samples as they are).
template <int MODE>
__device__ __forceinline__ void rgb_pixel(const RgbJob& J, const RgbUnit& t, int k, int& r, int& g, int& b)
{
    if (MODE == RGB_GBR) {
        r = rgb_byte(t.va, k); g = rgb_byte(t.y, k); b = rgb_byte(t.ua, k);
        return;
    }
    // every factor fits 24 bits and every sum 27: v_mad_i32_i24
    const int yt = __mul24(8 * J.cy, rgb_byte(t.y, k) - J.yo) + 65536;
    if (MODE == RGB_MONO) {
        r = g = b = rgb_clip255_sh17(yt);
        return;
    }
    int cb8, cr8;
    if (MODE == RGB_FULL) {
        cb8 = 8 * rgb_byte(t.ua, k);
        cr8 = 8 * rgb_byte(t.va, k);
    } else {
        const int m = k >> 1, m1 = (MODE != RGB_REP && (k & 1)) ? m + 1 : m;    // wh 2, or 1 and 1
        const int hu = rgb_byte(t.ua, m) + rgb_byte(t.ua, m1), hv = rgb_byte(t.va, m) + rgb_byte(t.va, m1);
        if (MODE == RGB_BIL2) {
            cb8 = 3 * hu + rgb_byte(t.ub, m) + rgb_byte(t.ub, m1);              // wv 3 and 1
            cr8 = 3 * hv + rgb_byte(t.vb, m) + rgb_byte(t.vb, m1);
        } else {
            cb8 = 4 * hu;
            cr8 = 4 * hv;
        }
    }
    const int cbd = cb8 - 1024, crd = cr8 - 1024;
    r = rgb_clip255_sh17(yt + __mul24(J.crv, crd));
    g = rgb_clip255_sh17(yt + __mul24(J.cgu, cbd) + __mul24(J.cgv, crd));
    b = rgb_clip255_sh17(yt + __mul24(J.cbu, cbd));
}

// bytes s of the eight bytes hi:lo (selector byte values 0..3 = lo's bytes, 4..7 = hi's): v_perm_b32
__device__ __forceinline__ uint32_t rgb_perm(uint32_t hi, uint32_t lo, uint32_t s) { return __builtin_amdgcn_perm(hi, lo, s); }

// NDW dwords to d, of which the first nbytes are the row's: 16-byte stores where all of them are and d
// allows it, else dwords, else bytes
template <int NDW>
__device__ __forceinline__ void rgb_store(uint8_t* d, const uint32_t (&w)[NDW], int nbytes)
{
    const unsigned mis = (unsigned)reinterpret_cast<uintptr_t>(d);
    if (nbytes == 4 * NDW && !(mis & 15)) {
#pragma unroll
        for (int q = 0; q < NDW / 4; ++q)
            reinterpret_cast<uint4*>(d)[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
    } else if (nbytes == 4 * NDW && !(mis & 3)) {
#pragma unroll
        for (int q = 0; q < NDW; ++q) reinterpret_cast<uint32_t*>(d)[q] = w[q];
    } else {
#pragma unroll
        for (int b = 0; b < 4 * NDW; ++b)
            if (b < nbytes) d[b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
    }
}

// channel bytes v (4 pixels) -> binary16 of float(v) * scale + bias: a multiplication, an addition, a
// conversion, each rounded to nearest even on its own (no fused multiply-add: contraction is off here)
__device__ __forceinline__ void rgb_half4(uint32_t v, float scale, float bias, uint32_t& lo, uint32_t& hi)
{
#pragma clang fp contract(off)
    uint32_t h[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float f = (float)((v >> (8 * k)) & 0xffu) * scale + bias;
        h[k] = (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)f);
    }
    lo = h[0] | (h[1] << 16);
    hi = h[2] | (h[3] << 16);
}

// The unit's bytes, in the job's format, to its place in the frame at `frame`.
__device__ __forceinline__ void rgb_write(const RgbJob& J, const RgbUnit& t, uint32_t (&c)[3][4], uint8_t* frame)
{
    if (J.bgr) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { const uint32_t s = c[0][q]; c[0][q] = c[2][q]; c[2][q] = s; }
    }
    uint8_t* const row = frame + (int64_t)t.r * J.pitch;
    if (J.format == H264R_RGB_PACKED_U8) {
        uint32_t w[12];
#pragma unroll
        for (int q = 0; q < 4; ++q) {                       // 4 pixels: c0 c1 c2 c0 | c1 c2 c0 c1 | c2 c0 c1 c2
            const uint32_t a = c[0][q], b = c[1][q], d = c[2][q];
            w[3 * q + 0] = rgb_perm(d, rgb_perm(b, a, 0x01000400u), 0x03040100u);   // a0 b0 d0 a1
            w[3 * q + 1] = rgb_perm(a, rgb_perm(d, b, 0x02000501u), 0x03060100u);   // b1 d1 a2 b2
            w[3 * q + 2] = rgb_perm(b, rgb_perm(d, a, 0x07000306u), 0x03070100u);   // d2 a3 b3 d3
        }
        rgb_store<12>(row + 3 * t.x, w, 3 * t.n);
    } else if (J.format == H264R_RGB_PACKED_U8X4) {
        uint32_t w[16];
        const uint32_t al = (uint32_t)J.alpha * 0x01010101u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t ab_lo = rgb_perm(c[1][q], c[0][q], 0x05010400u);   // a0 b0 a1 b1
            const uint32_t ab_hi = rgb_perm(c[1][q], c[0][q], 0x07030602u);   // a2 b2 a3 b3
            const uint32_t dx_lo = rgb_perm(al, c[2][q], 0x04010400u);        // d0 al d1 al
            const uint32_t dx_hi = rgb_perm(al, c[2][q], 0x04030402u);        // d2 al d3 al
            w[4 * q + 0] = rgb_perm(dx_lo, ab_lo, 0x05040100u);
            w[4 * q + 1] = rgb_perm(dx_lo, ab_lo, 0x07060302u);
            w[4 * q + 2] = rgb_perm(dx_hi, ab_hi, 0x05040100u);
            w[4 * q + 3] = rgb_perm(dx_hi, ab_hi, 0x07060302u);
        }
        rgb_store<16>(row + 4 * t.x, w, 4 * t.n);
    } else if (J.format == H264R_RGB_PLANAR_U8) {
#pragma unroll
        for (int p = 0; p < 3; ++p) rgb_store<4>(row + J.plane_off[p] + t.x, c[p], t.n);
    } else {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            uint32_t w[8];
#pragma unroll
            for (int q = 0; q < 4; ++q) rgb_half4(c[p][q], J.scale[p], J.bias[p], w[2 * q], w[2 * q + 1]);
            rgb_store<8>(row + J.plane_off[p] + 2 * t.x, w, 2 * t.n);
        }
    }
}

}  // namespace h264r
