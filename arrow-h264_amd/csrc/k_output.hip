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
// TWIN: rgb_pixel (k_output_scale.hip) is this arithmetic for one pixel; a change goes into both.
template <int MODE>
__device__ __forceinline__ void rgb_convert(const RgbJob& J, const RgbUnit& t, uint32_t (&c)[3][4])
{
    if (MODE == RGB_GBR) {
        c[0][0] = t.va.x; c[0][1] = t.va.y; c[0][2] = t.va.z; c[0][3] = t.va.w;
        c[1][0] = t.y.x;  c[1][1] = t.y.y;  c[1][2] = t.y.z;  c[1][3] = t.y.w;
        c[2][0] = t.ua.x; c[2][1] = t.ua.y; c[2][2] = t.ua.z; c[2][3] = t.ua.w;
        return;
    }
    const int ky = 8 * J.cy;
#pragma unroll
    for (int q = 0; q < 4; ++q) c[0][q] = c[1][q] = c[2][q] = 0;
#pragma unroll
    for (int k = 0; k < RGB_UNIT; ++k) {
        // every factor fits 24 bits and every sum 27: v_mad_i32_i24
        const int yt = __mul24(ky, rgb_byte(t.y, k) - J.yo) + 65536;
        int r, g, b;
        if (MODE == RGB_MONO) {
            r = g = b = rgb_clip255_sh17(yt);
        } else {
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
        c[0][k >> 2] |= (uint32_t)r << (8 * (k & 3));
        c[1][k >> 2] |= (uint32_t)g << (8 * (k & 3));
        c[2][k >> 2] |= (uint32_t)b << (8 * (k & 3));
    }
}

// Unit i of a frame: every load it needs (t.n = 0: there is no such unit).
// TWIN: rgb_fetch_at (k_output_scale.hip) loads the same for a unit at any column; a change goes into both.
template <int MODE>
__device__ __forceinline__ void rgb_fetch(const RgbJob& J, int kind, const uint8_t* const (&yp)[2], const uint8_t* const (&up)[2],
                                          const uint8_t* const (&vp)[2], int i, int total, int upr, RgbUnit& t)
{
    t.n = 0;
    if (i >= total) return;
    t.r = i / upr;
    t.x = (i - t.r * upr) * RGB_UNIT;
    t.n = min(RGB_UNIT, J.lw - t.x);
    const bool whole = t.n == RGB_UNIT;
    const uint8_t* const ys = rgb_row(yp[0], yp[1], J.y0 + t.r, J.lpitch, kind);
    if (!ys) t.y = make_uint4(RGB_GREY, RGB_GREY, RGB_GREY, RGB_GREY);
    else if (whole) t.y = ld16u(ys + J.x0 + t.x);
    else t.y = rgb_ld_clamped(ys + J.x0, t.x, J.lw - 1, RGB_UNIT);
    if (MODE == RGB_MONO) return;
    // the chroma rows j0 (and j1) of the cropped rectangle, and the unit's first chroma column
    const int i0 = MODE < RGB_REP ? t.x : t.x >> 1;
    int ja = t.r, jb = t.r;
    if (MODE >= RGB_REP && J.sub_h == 2) {
        ja = t.r >> 1;
        jb = (t.r & 1) ? min(ja + 1, J.ch - 1) : max(ja - 1, 0);
    }
    const uint8_t* const ur = rgb_row(up[0], up[1], J.cy0 + ja, J.cpitch, kind);
    const uint8_t* const vr = rgb_row(vp[0], vp[1], J.cy0 + ja, J.cpitch, kind);
    t.ua = rgb_ld_chroma(ur ? ur + J.cx0 : nullptr, i0, J.cw, MODE, whole);
    t.va = rgb_ld_chroma(vr ? vr + J.cx0 : nullptr, i0, J.cw, MODE, whole);
    if (MODE == RGB_BIL2) {
        const uint8_t* const ub = rgb_row(up[0], up[1], J.cy0 + jb, J.cpitch, kind);
        const uint8_t* const vb = rgb_row(vp[0], vp[1], J.cy0 + jb, J.cpitch, kind);
        t.ub = rgb_ld_chroma(ub ? ub + J.cx0 : nullptr, i0, J.cw, MODE, whole);
        t.vb = rgb_ld_chroma(vb ? vb + J.cx0 : nullptr, i0, J.cw, MODE, whole);
    }
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
