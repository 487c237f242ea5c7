// k_output.hip -- the output stage of include/h264r_output.h: cropped, woven, packed frames from
// the coded-size planes (write_out_picture / write_unpaired_field output.cc:109-263,
// dpb_combine_field_yuv picture.cc:578-622), one launch for every frame and plane of a job.
//
// A pure copy.  The unit of work is one 16-byte ALIGNED window of the destination: row r of a plane
// starts at an arbitrary address (contiguous rows of an odd width, any dst), so the row is cut at the
// 16-byte boundaries of the destination into out_chunks_per_row(w) windows at most.  A window that lies
// wholly inside the row is written with one 16-byte store; the windows holding the row's head and tail
// are written bytewise, so no byte outside the row is written (pitch padding, the next frame).  The
// source is misaligned against the destination in general (crop_left, the parity of the row, the
// destination's own offset): the 16 source bytes of a window are fetched with ONE unaligned 16-byte
// load (gfx950 global loads have no alignment requirement; the compiler emits global_load_dwordx4 for
// the align-1 copy below), which reads exactly the bytes the window needs and so nothing outside the
// source plane -- the batch's out planes have no slack behind them.  Semi-planar chroma fetches 8 bytes
// of Cb and 8 of Cr and interleaves them in registers.  A thread fetches OUT_ITEMS windows before it
// stores the first, OUT_THREADS apart so that a wave's loads and stores are contiguous.
//
// Grid: x = groups of OUT_THREADS * OUT_ITEMS windows of one plane, y = frames (strided), z = plane.
//
// Below it k_output_rgb, which writes the same frames as RGB; it has a comment of its own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "output_rgb.h"   // the unaligned loads; what k_output_rgb shares with k_output_rgb_scaled

namespace h264r {

// bytes p0 q0 p1 q1 of the 16-bit pairs p, q
__device__ __forceinline__ uint32_t il2(uint32_t p, uint32_t q)
{
    return (p & 0xffu) | ((q & 0xffu) << 8) | ((p & 0xff00u) << 8) | ((q & 0xff00u) << 16);
}

// a0 b0 a1 b1 ... a7 b7
__device__ __forceinline__ uint4 interleave8(uint2 a, uint2 b)
{
    return make_uint4(il2(a.x, b.x), il2(a.x >> 16, b.x >> 16), il2(a.y, b.y), il2(a.y >> 16, b.y >> 16));
}

// One 16-byte window of the destination.
struct OutItem {
    uint8_t* d;            // the window (16-byte aligned); row byte b is d[b - b0]
    const uint8_t* sa;     // the source row: byte b of the row is sa[b] (interleaved: Cb sample sa[b >> 1])
    const uint8_t* sb;     // interleaved: the Cr row
    int b0;                // the window's first byte, relative to the row (< 0: it starts before the row)
    int lo, hi;            // the row's bytes inside the window, [lo, hi); lo >= hi: none
    bool fill;             // no source: 128
};

}  // namespace h264r

using namespace h264r;

extern "C" __global__ void __launch_bounds__(OUT_THREADS)
k_output(OutJob job, const h264r_out_frame* __restrict__ frames, uint8_t* dst, int* err)
{
    const OutPlane P = job.pl[blockIdx.z];
    const int cpr = out_chunks_per_row(P.w);
    const int total = P.h * cpr;
    const int base = (int)blockIdx.x * (OUT_THREADS * OUT_ITEMS) + (int)threadIdx.x;
    if ((int)blockIdx.x * (OUT_THREADS * OUT_ITEMS) >= total) return;

    for (int f = blockIdx.y; f < job.num_frames; f += gridDim.y) {
        // the refusals: before any pointer of the frame is used
        const int kind = frames[f].kind;
        const bool pair = kind == H264R_OUT_FIELD_PAIR;
        const uint8_t* const y0p = frames[f].y[0];
        const uint8_t* const y1p = frames[f].y[1];
        bool ok = (unsigned)kind <= (unsigned)H264R_OUT_UNPAIRED_BOT && y0p && (!pair || y1p);
        const uint8_t *u0p = nullptr, *u1p = nullptr, *v0p = nullptr, *v1p = nullptr;
        if (job.need_chroma) {
            u0p = frames[f].u[0]; u1p = frames[f].u[1];
            v0p = frames[f].v[0]; v1p = frames[f].v[1];
            ok = ok && u0p && v0p && (!pair || (u1p && v1p));
        }
        if (!ok) {
            if (blockIdx.x == 0 && blockIdx.z == 0 && threadIdx.x == 0) atomicOr(err, DEV_ERR_OUTPUT);
            continue;
        }
        // the rows of the missing parity of an unpaired field: 128 (storable_picture::clear)
        const int fill_parity = kind == H264R_OUT_UNPAIRED_TOP ? 1 : kind == H264R_OUT_UNPAIRED_BOT ? 0 : -1;
        const bool field = kind != H264R_OUT_FRAME;
        uint8_t* const fdst = dst + (int64_t)f * job.frame_stride + P.off;

        OutItem it[OUT_ITEMS];
        uint4 val[OUT_ITEMS];
#pragma unroll
        for (int j = 0; j < OUT_ITEMS; ++j) {
            OutItem& t = it[j];
            const int i = base + j * OUT_THREADS;
            t.lo = t.hi = 0;
            if (i >= total) continue;
            const int r = i / cpr, c = i - r * cpr;
            uint8_t* const drow = fdst + (int64_t)r * P.pitch;
            t.b0 = c * 16 - (int)(reinterpret_cast<uintptr_t>(drow) & 15);
            t.d = drow + t.b0;
            t.lo = max(t.b0, 0);
            t.hi = min(t.b0 + 16, P.w);
            if (t.lo >= t.hi) continue;
            // the source row: row R of the woven frame is row R >> 1 of the field of parity R & 1
            const int R = P.y0 + r;
            const int src = pair ? (R & 1) : 0;
            const int64_t so = (int64_t)(field ? R >> 1 : R) * P.src_pitch + P.x0;
            t.fill = P.mode == OUT_FILL || (R & 1) == fill_parity;
            t.sa = t.sb = nullptr;
            if (!t.fill) {
                if (P.mode == OUT_COPY_Y) t.sa = (src ? y1p : y0p) + so;
                else if (P.mode == OUT_COPY_V) t.sa = (src ? v1p : v0p) + so;
                else t.sa = (src ? u1p : u0p) + so;
                if (P.mode == OUT_INTERLEAVE) t.sb = (src ? v1p : v0p) + so;
            }
            if (t.hi - t.lo < 16) continue;                 // head / tail: bytewise below
            if (t.fill) val[j] = make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);
            else if (P.mode != OUT_INTERLEAVE) val[j] = ld16u(t.sa + t.b0);
            else {
                // row bytes b0 .. b0 + 15 are samples k .. of the plane byte b0 belongs to and the 8
                // samples of the other plane that follow it: from k when b0 is even (Cb first), from
                // k + 1 when it is odd (Cr k first, then Cb k + 1)
                const int k = t.b0 >> 1, odd = t.b0 & 1;
                const uint2 a = ld8u((odd ? t.sb : t.sa) + k);
                const uint2 b = ld8u((odd ? t.sa + 1 : t.sb) + k);
                val[j] = interleave8(a, b);
            }
        }
#pragma unroll
        for (int j = 0; j < OUT_ITEMS; ++j) {
            const OutItem& t = it[j];
            if (t.lo >= t.hi) continue;
            if (t.hi - t.lo == 16) {
                *reinterpret_cast<uint4*>(t.d) = val[j];
                continue;
            }
            for (int b = t.lo; b < t.hi; ++b) {
                uint8_t x = 128;
                if (!t.fill) x = P.mode == OUT_INTERLEAVE ? ld1(((b & 1) ? t.sb : t.sa) + (b >> 1)) : ld1(t.sa + b);
                t.d[b - t.b0] = x;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_output_rgb -- the RGB frames of include/h264r_output.h (its comment is the definition; the names
// below are the header's).  One launch for every frame of a job, nothing but registers.
//
// The unit of work is RGB_UNIT = 16 horizontally consecutive pixels of one output row, counted from
// the row's first pixel.  A whole unit costs one unaligned 16-byte luma load and, per chroma plane and
// chroma row it needs, one 8-byte load (16 in 4:4:4) plus, under bilinear, the one sample that follows
// (clamped to the crop's last column): exactly the bytes the definition names, so nothing outside the
// crop -- let alone the plane -- is read.  The row's last unit, when the width is no multiple of 16,
// fetches its samples bytewise with the same clamp.  Either way the unit then holds the same registers,
// is converted by the same code to 16 bytes per channel, and those are interleaved in registers
// (v_perm_b32) into the format's bytes: 48 (RGB24), 64 (RGBX), 16 per plane (planar u8) or 32 per
// plane (binary16).  Where the unit is whole and its destination 16-byte aligned they leave as 16-byte
// stores; elsewhere as dwords or bytes, never one outside the row.  A thread fetches RGB_ITEMS units
// before it stores the first, RGB_THREADS apart, so that a wave's loads are contiguous.
//
// Grid: x = groups of RGB_THREADS * RGB_ITEMS units, y = frames (strided).
namespace h264r {

// The unit's 16 pixels as 16 bytes per channel: c[0] = R, c[1] = G, c[2] = B.
template <int MODE>
__device__ __forceinline__ void rgb_convert(const RgbJob& J, const RgbUnit& t, uint32_t (&c)[3][4])
{
#pragma unroll
    for (int q = 0; q < 4; ++q) c[0][q] = c[1][q] = c[2][q] = 0;
#pragma unroll
    for (int k = 0; k < RGB_UNIT; ++k) {
        int r, g, b;
        rgb_pixel<MODE>(J, t, k, r, g, b);
        c[0][k >> 2] |= (uint32_t)r << (8 * (k & 3));
        c[1][k >> 2] |= (uint32_t)g << (8 * (k & 3));
        c[2][k >> 2] |= (uint32_t)b << (8 * (k & 3));
    }
}

// Unit i of a frame: every load it needs (t.n = 0: there is no such unit).
template <int MODE>
__device__ __forceinline__ void rgb_fetch(const RgbJob& J, int kind, const uint8_t* const (&yp)[2], const uint8_t* const (&up)[2],
                                          const uint8_t* const (&vp)[2], int i, int total, int upr, RgbUnit& t)
{
    t.n = 0;
    if (i >= total) return;
    t.r = i / upr;
    t.x = (i - t.r * upr) * RGB_UNIT;
    t.n = min(RGB_UNIT, J.lw - t.x);
    rgb_fetch_at<MODE>(J, RgbSrc{kind}, yp, up, vp, t);
}

template <int MODE>
__device__ __forceinline__ void rgb_finish(const RgbJob& J, const RgbUnit& t, uint8_t* fdst)
{
    if (t.n == 0) return;
    uint32_t c[3][4];
    rgb_convert<MODE>(J, t, c);
    rgb_write(J, t, c, fdst);
}

// The units of one frame that fall to this thread, RGB_THREADS apart: every load, then convert and store.
template <int MODE>
__device__ __forceinline__ void rgb_units(const RgbJob& J, int kind, const uint8_t* const (&yp)[2], const uint8_t* const (&up)[2],
                                          const uint8_t* const (&vp)[2], int base, int total, int upr, uint8_t* fdst)
{
    static_assert(RGB_ITEMS == 2, "rgb_units names its units");
    RgbUnit t0, t1;
    rgb_fetch<MODE>(J, kind, yp, up, vp, base, total, upr, t0);
    rgb_fetch<MODE>(J, kind, yp, up, vp, base + RGB_THREADS, total, upr, t1);
    rgb_finish<MODE>(J, t0, fdst);
    rgb_finish<MODE>(J, t1, fdst);
}

}  // namespace h264r

extern "C" __global__ void __launch_bounds__(RGB_THREADS)
k_output_rgb(RgbJob job, const h264r_out_frame* __restrict__ frames, uint8_t* dst, int* err)
{
    const RgbJob& J = job;
    const int upr = rgb_units_per_row(J.lw);
    const int total = J.lh * upr;
    const int base = (int)blockIdx.x * (RGB_THREADS * RGB_ITEMS) + (int)threadIdx.x;
    if ((int)blockIdx.x * (RGB_THREADS * RGB_ITEMS) >= total) return;
    const int mode = J.mode;

    for (int f = blockIdx.y; f < J.num_frames; f += gridDim.y) {
        // the refusals: before any pointer of the frame is used
        const int kind = frames[f].kind;
        const bool pair = kind == H264R_OUT_FIELD_PAIR;
        const uint8_t* const yp[2] = {frames[f].y[0], frames[f].y[1]};
        bool ok = (unsigned)kind <= (unsigned)H264R_OUT_UNPAIRED_BOT && yp[0] && (!pair || yp[1]);
        const uint8_t* const none[2] = {nullptr, nullptr};
        if (mode == RGB_MONO) {
            if (ok) rgb_units<RGB_MONO>(J, kind, yp, none, none, base, total, upr, dst + (int64_t)f * J.frame_stride);
        } else {
            const uint8_t* const up[2] = {frames[f].u[0], frames[f].u[1]};
            const uint8_t* const vp[2] = {frames[f].v[0], frames[f].v[1]};
            ok = ok && up[0] && vp[0] && (!pair || (up[1] && vp[1]));
            if (ok) {
                uint8_t* const fdst = dst + (int64_t)f * J.frame_stride;
                switch (mode) {
                case RGB_FULL: rgb_units<RGB_FULL>(J, kind, yp, up, vp, base, total, upr, fdst); break;
                case RGB_GBR:  rgb_units<RGB_GBR>(J, kind, yp, up, vp, base, total, upr, fdst); break;
                case RGB_REP:  rgb_units<RGB_REP>(J, kind, yp, up, vp, base, total, upr, fdst); break;
                case RGB_BIL1: rgb_units<RGB_BIL1>(J, kind, yp, up, vp, base, total, upr, fdst); break;
                default:       rgb_units<RGB_BIL2>(J, kind, yp, up, vp, base, total, upr, fdst); break;
                }
            }
        }
        if (!ok && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(err, DEV_ERR_OUTPUT);
    }
}
