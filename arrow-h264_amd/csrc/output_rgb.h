// output_rgb.h -- the device code the two RGB kernels share: k_output_rgb (k_output.hip) and
// the k_output_rgb_scaled kernels (k_output_scale.hip).  The unaligned global loads, the 16-pixel source
// unit with its row addresses and clamped loads, the clamp of the matrix, and the unit's way out: the
// format's bytes, interleaved in registers and stored as widely as the destination allows.  Only what
// both use: each kernel's fetch and convert are in its own file and name their twins there.
// Everything is inlined; neither kernel's registers depend on the other.
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

// One chroma row's samples for the unit at chroma column i0: s = the row at the crop's first column.
__device__ __forceinline__ uint4 rgb_ld_chroma(const uint8_t* s, int i0, int cw, int mode, bool whole)
{
    if (!s) return make_uint4(RGB_GREY, RGB_GREY, RGB_GREY, RGB_GREY);
    const bool wide = mode < RGB_REP;
    if (!whole) return rgb_ld_clamped(s, i0, cw - 1, wide ? 16 : 9);
    if (wide) return ld16u(s + i0);
    const uint2 a = ld8u(s + i0);
    const uint32_t next = mode >= RGB_BIL1 ? ld1(s + min(i0 + 8, cw - 1)) : 0u;
    return make_uint4(a.x, a.y, next, 0u);
}

__device__ __forceinline__ int rgb_byte(const uint4& v, int k)
{
    const uint32_t w = (k >> 2) == 0 ? v.x : (k >> 2) == 1 ? v.y : (k >> 2) == 2 ? v.z : v.w;
    return (int)((w >> (8 * (k & 3))) & 0xffu);
}

// clip255(v >> 17), clamped BEFORE the shift: min(max(v, 0), 2^25 - 1) >> 17 is the same number, and it
// keeps the compiler from fusing shift and clamp of two pixels into gfx950's v_ashr_pk_u8_i32
__device__ __forceinline__ int rgb_clip255_sh17(int v) { return (int)((uint32_t)min(max(v, 0), (256 << 17) - 1) >> 17); }

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
