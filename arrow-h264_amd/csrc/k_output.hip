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
