// k_output_resample.hip -- the k_output_rgb_resampled kernels: the Pillow-exact resampled RGB frames of
// include/h264r_output.h (its comment is the definition; the names below are the header's).  One launch
// for every frame of a job, of the kernel for the job's RgbMode: k_output_rgb_resampled_<mode>, six in all
// (kernels.h).  The filter is not in the kernel: it is in the two tables of the plan (resample_tables.h).
//
// A workgroup owns a tile of RS_TH x RS_TW = 16 x 16 output pixels of one frame, all three channels, and
// makes both passes inside its LDS; the only global traffic is the source planes, the tables and the
// destination.  No converted and no half-resampled frame exists in device memory.
//
//   1. The tile's rows of the two tables come into LDS: xmin and count of its 16 columns and 16 rows, and
//      their taps kkx [16][ksx], kky [16][ksy].  An output behind the frame's last column or row repeats
//      the last one, and none of its bytes is written.  xmin and xmin + count do not decrease with the
//      output index, so the tile's windows span the source columns [xmin[first], xmin[last] + count[last])
//      and the rows likewise.
//   2. It steps over those source rows, step_rows at a time.  Per step every 16-pixel unit of the column
//      span is fetched and converted once -- scale_fetch and rgb_pixel of output_scale.h / output_rgb.h,
//      the functions the scaled kernels use, so the source planes are the RGB definition's by construction,
//      a unit that reaches past the crop's last column included -- into the strip, one pixel a word
//      (c0 | c1 << 8 | c2 << 16 in R G B order: bgr swaps at the store, the passes treat the channels
//      alike).  Then a thread per (row, output column) sums its window from the strip, three channels
//      off one word and one tap, and stores the clipped bytes in t [row][channel][16].
//   3. After the last step a thread per output pixel sums its vertical window from t, and 16 threads write
//      one row of the tile each with k_output_rgb's rgb_write: 16-byte stores where the row is whole and
//      its destination aligned, dwords or bytes elsewhere, nothing outside the row.
//
// A tap is at most 2^23 in magnitude and a sample 8 bits: one v_mad_i32_i24.  clip8(acc >> 22) clamps
// BEFORE the shift (rs_clip8_sh22), as rgb_clip255_sh17 does, so that hipcc cannot fuse shift and clamp of
// two pixels into gfx950's v_ashr_pk_u8_i32.
//
// Window clamping is in the tables: no index leaves [0, lw) x [0, lh) of the cropped rectangle, so no
// byte outside the crop is read.
//
// LDS (rs_lds_bytes, output_job.h), dynamic, sized by the plan: for 1920 x 1080 -> 224 x 224 BICUBIC
// 3,712 bytes of taps, 4,416 of t (92 rows), 11,264 of strip (16 rows of 176 columns): 20,496 in all
// (TRIANGLE 17,200, LANCZOS 23,664: seven or six workgroups a CU); LANCZOS at scale 16 on both axes 52 KB;
// 64 KiB at the most (TRIANGLE at scale 48, two rows a step), so two workgroups fit a CU's 160 KB always.
// Registers: 55 or 56 VGPRs, 78 to 91 SGPRs, no spills: the registers allow 8 waves per SIMD, the launch
// bounds ask for 4 at the least (a cap of 128 VGPRs), and the LDS decides.
//
// Grid: x = tiles of one frame, row by row; y and z = frames, frame z * gridDim.y + y.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "output_scale.h"

namespace h264r {

static_assert(RS_THREADS == RS_TW * RS_TH, "the vertical pass: a thread per output pixel");

// What only the threads that write a row need of the job -- the output side: offsets, pitch, format, scale
// and bias -- as words of LDS (RS_OUT_WORDS, output_job.h), so that it holds no SGPR during the passes.
enum ResampleOut : int {
    RO_PLANE_OFF = 0,          // 3 x 2 words
    RO_PITCH = 6,              // 2 words
    RO_FORMAT = 8, RO_BGR, RO_ALPHA,
    RO_SCALE = 11, RO_BIAS = 14,
    RO_FRAME = 17,             // 2 words: where the frame starts, from dst on
    RO_WORDS = 19,
};
static_assert(RO_WORDS <= RS_OUT_WORDS, "rs_lds_bytes has room for them");

// clip8(v >> 22), clamped before the shift: min(max(v, 0), 2^30 - 1) >> 22 is the same number
__device__ __forceinline__ int rs_clip8_sh22(int v) { return (int)((uint32_t)min(max(v, 0), (256 << 22) - 1) >> 22); }

template <int MODE>
__device__ __forceinline__ void resample_job(const ResampleJob& S, const h264r_out_frame* __restrict__ frames, uint8_t* dst, int* err)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t rs_lds[];
    const RgbJob& J = S.rgb;
    const int f = (int)(blockIdx.z * gridDim.y + blockIdx.y);
    if (f >= J.num_frames) return;
    // the refusals: before any pointer of the frame is used
    const int kind = frames[f].kind;
    const bool pair = kind == H264R_OUT_FIELD_PAIR;
    const uint8_t* const y0 = frames[f].y[0];
    const uint8_t* const u0 = MODE == RGB_MONO ? nullptr : frames[f].u[0];
    const uint8_t* const v0 = MODE == RGB_MONO ? nullptr : frames[f].v[0];
    const uint8_t* const yp[2] = {y0, pair ? frames[f].y[1] : y0};                  // see scale_row (output_rgb.h)
    const uint8_t* const up[2] = {u0, pair && MODE != RGB_MONO ? frames[f].u[1] : u0};
    const uint8_t* const vp[2] = {v0, pair && MODE != RGB_MONO ? frames[f].v[1] : v0};
    bool ok = (unsigned)kind <= (unsigned)H264R_OUT_UNPAIRED_BOT && yp[0] && yp[1];
    if (MODE != RGB_MONO) ok = ok && up[0] && vp[0] && up[1] && vp[1];
    if (!ok) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(err, DEV_ERR_OUTPUT);
        return;
    }

    // the workgroup's LDS (rs_lds_bytes)
    const int ksx = S.ax.ksize, ksy = S.ay.ksize;
    int32_t* const kkx = reinterpret_cast<int32_t*>(rs_lds);               // [RS_TW][ksx]
    int32_t* const kky = kkx + RS_TW * ksx;                                // [RS_TH][ksy]
    int32_t* const bx = kky + RS_TH * ksy;                                 // xmin and count of the tile's columns
    int32_t* const cx = bx + RS_TW;
    int32_t* const by = cx + RS_TW;                                        // and of its rows
    int32_t* const cy = by + RS_TH;
    uint8_t* const t = reinterpret_cast<uint8_t*>(cy + RS_TH);             // [span_rows][3][RS_TW]
    uint32_t* const strip = reinterpret_cast<uint32_t*>(t + rs_t_bytes(S.span_rows));   // [step_rows][strip_cols]
    uint32_t* const tile = strip + S.step_rows * S.strip_cols;             // [3][RS_TH][RS_TW] bytes
    uint32_t* const out = tile + 3 * RS_TH * RS_TW / 4;                    // [RS_OUT_WORDS]

    const int tid = (int)threadIdx.x;
    const int ty = (int)blockIdx.x / S.tiles_x;
    const int d0 = ((int)blockIdx.x - ty * S.tiles_x) * RS_TW, e0 = ty * RS_TH;
    // 1. the tile's part of the tables; an output behind the last repeats it
    if (tid == RS_THREADS - 1) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            out[RO_PLANE_OFF + 2 * p] = (uint32_t)J.plane_off[p];
            out[RO_PLANE_OFF + 2 * p + 1] = (uint32_t)(J.plane_off[p] >> 32);
            out[RO_SCALE + p] = __float_as_uint(J.scale[p]);
            out[RO_BIAS + p] = __float_as_uint(J.bias[p]);
        }
        out[RO_PITCH] = (uint32_t)J.pitch;
        out[RO_PITCH + 1] = (uint32_t)(J.pitch >> 32);
        out[RO_FORMAT] = (uint32_t)J.format;
        out[RO_BGR] = (uint32_t)J.bgr;
        out[RO_ALPHA] = (uint32_t)J.alpha;
        const uint64_t frame = (uint64_t)((int64_t)f * J.frame_stride);
        out[RO_FRAME] = (uint32_t)frame;
        out[RO_FRAME + 1] = (uint32_t)(frame >> 32);
    }
    if (tid < RS_TW) {
        const int d = min(d0 + tid, S.ax.D - 1);
        bx[tid] = S.ax.xmin[d];
        cx[tid] = S.ax.count[d];
    } else if (tid < RS_TW + RS_TH) {
        const int e = min(e0 + tid - RS_TW, S.ay.D - 1);
        by[tid - RS_TW] = S.ay.xmin[e];
        cy[tid - RS_TW] = S.ay.count[e];
    }
    for (int i = tid; i < RS_TW * ksx; i += RS_THREADS) {
        const int d = i / ksx;
        kkx[i] = S.ax.kk[min(d0 + d, S.ax.D - 1) * ksx + (i - d * ksx)];
    }
    for (int i = tid; i < RS_TH * ksy; i += RS_THREADS) {
        const int e = i / ksy;
        kky[i] = S.ay.kk[min(e0 + e, S.ay.D - 1) * ksy + (i - e * ksy)];
    }
    __syncthreads();

    const int nx = min(RS_TW, S.ax.D - d0), ny = min(RS_TH, S.ay.D - e0);
    const int x_lo = bx[0], x_hi = bx[nx - 1] + cx[nx - 1];               // columns and rows of the cropped rectangle
    const int y_lo = by[0], y_hi = by[ny - 1] + cy[ny - 1];
    const int xs = MODE >= RGB_REP ? x_lo & ~1 : x_lo;                     // a unit starts on a chroma sample
    const int units = (x_hi - xs + RGB_UNIT - 1) / RGB_UNIT;              // units * 16 <= strip_cols, y_hi - y_lo <= span_rows
    const ScaleSrc src{scale_kind(kind)};

    // 2. the source rows, step_rows at a time: convert into the strip, then the horizontal pass into t
    for (int y = y_lo; y < y_hi; y += S.step_rows) {
        const int rows = min(S.step_rows, y_hi - y);
        for (int item = tid; item < rows * units; item += RS_THREADS) {
            const int ri = item / units, u = item - ri * units;
            RgbUnit un;
            un.r = y + ri;
            un.x = xs + RGB_UNIT * u;
            un.n = min(RGB_UNIT, J.lw - un.x);
            scale_fetch<MODE>(J, src, yp, up, vp, un);
            uint32_t* const sp = strip + ri * S.strip_cols + RGB_UNIT * u;
#pragma unroll
            for (int q = 0; q < RGB_UNIT / 4; ++q) {
                uint32_t w[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    int r, g, b;
                    rgb_pixel<MODE>(J, un, 4 * q + k, r, g, b);
                    w[k] = (uint32_t)r | (uint32_t)g << 8 | (uint32_t)b << 16;
                }
                reinterpret_cast<uint4*>(sp)[q] = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
        __syncthreads();
        for (int item = tid; item < rows * RS_TW; item += RS_THREADS) {
            const int ri = item / RS_TW, d = item % RS_TW;
            const uint32_t* const sp = strip + ri * S.strip_cols + (bx[d] - xs);
            const int32_t* const kp = kkx + d * ksx;
            const int n = cx[d];
            int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
            for (int j = 0; j < n; ++j) {
                const uint32_t px = sp[j];
                const int k = kp[j];
                a0 += __mul24(k, (int)(px & 0xffu));
                a1 += __mul24(k, (int)((px >> 8) & 0xffu));
                a2 += __mul24(k, (int)((px >> 16) & 0xffu));
            }
            uint8_t* const tp = t + (y - y_lo + ri) * (3 * RS_TW) + d;
            tp[0] = (uint8_t)rs_clip8_sh22(a0);
            tp[RS_TW] = (uint8_t)rs_clip8_sh22(a1);
            tp[2 * RS_TW] = (uint8_t)rs_clip8_sh22(a2);
        }
        __syncthreads();
    }

    // 3. the vertical pass, a thread per output pixel, then a thread per row of the tile
    {
        const int d = tid % RS_TW, e = tid / RS_TW;
        const int32_t* const kp = kky + e * ksy;
        const uint8_t* tp = t + (by[e] - y_lo) * (3 * RS_TW) + d;
        const int n = cy[e];
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
        for (int j = 0; j < n; ++j) {
            const int k = kp[j];
            a0 += __mul24(k, (int)tp[0]);
            a1 += __mul24(k, (int)tp[RS_TW]);
            a2 += __mul24(k, (int)tp[2 * RS_TW]);
            tp += 3 * RS_TW;
        }
        uint8_t* const o = reinterpret_cast<uint8_t*>(tile) + e * RS_TW + d;
        o[0] = (uint8_t)rs_clip8_sh22(a0);
        o[RS_TH * RS_TW] = (uint8_t)rs_clip8_sh22(a1);
        o[2 * RS_TH * RS_TW] = (uint8_t)rs_clip8_sh22(a2);
    }
    __syncthreads();
    if (tid < ny) {
        RgbJob W;                                           // the output side alone: all rgb_write reads
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            W.plane_off[p] = (int64_t)(out[RO_PLANE_OFF + 2 * p] | (uint64_t)out[RO_PLANE_OFF + 2 * p + 1] << 32);
            W.scale[p] = __uint_as_float(out[RO_SCALE + p]);
            W.bias[p] = __uint_as_float(out[RO_BIAS + p]);
        }
        W.pitch = (int64_t)(out[RO_PITCH] | (uint64_t)out[RO_PITCH + 1] << 32);
        // job-wide, and known to be: the format's branches stay branches of the wave
        W.format = __builtin_amdgcn_readfirstlane((int)out[RO_FORMAT]);
        W.bgr = __builtin_amdgcn_readfirstlane((int)out[RO_BGR]);
        W.alpha = (int)out[RO_ALPHA];
        RgbUnit un;
        un.r = e0 + tid;
        un.x = d0;
        un.n = nx;
        uint32_t c[3][4];
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) c[p][q] = tile[(p * RS_TH + tid) * (RS_TW / 4) + q];
        rgb_write(W, un, c, dst + (int64_t)(out[RO_FRAME] | (uint64_t)out[RO_FRAME + 1] << 32));
    }
}

}  // namespace h264r

using namespace h264r;

// four waves per SIMD at the least: a cap of 128 VGPRs
#define RESAMPLE_KERNEL(NAME, MODE)                                                                                 \
    extern "C" __global__ void __launch_bounds__(RS_THREADS, 4)                                                     \
    k_output_rgb_resampled_##NAME(ResampleJob job, const h264r_out_frame* __restrict__ frames, uint8_t* dst, int* err) \
    {                                                                                                               \
        resample_job<MODE>(job, frames, dst, err);                                                                  \
    }
H264R_RESAMPLE_KERNELS(RESAMPLE_KERNEL)
