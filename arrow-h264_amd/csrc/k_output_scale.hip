// k_output_scale.hip -- the k_output_rgb_scaled kernels: the scaled RGB frames of include/h264r_output.h
// (its comment is the definition; the names below are the header's).  One launch for every frame of a
// job, of the kernel for the job's RgbMode and filter: k_output_rgb_scaled_<mode>_<filter>, twelve in
// all (kernels.h).  One kernel for every mode and filter kept more scalars alive than there are SGPRs.
//
// A thread owns one OUTPUT pixel; adjacent lanes own adjacent pixels of an output row, so the source
// windows of a wave line up along the source rows and its loads cover one contiguous stretch of each.
// The window and the pixel (scale_div .. scale_pixel) are in output_scale.h, which the k_output_boxes
// kernels include as well.  Both filters are one weighted window: columns [xlo, xhi) and rows [ylo, yhi) of the region of
// interest, a weight per column and a weight per row, and
//     acc[c] = sum over rows of wv * (sum over columns of wh * c[row][column])
// H264R_SCALE_AREA takes the box coverages in the axis' reduced unit and ends in (2 acc + T) / (2 T);
// H264R_SCALE_BILINEAR has one or two columns and rows with the 8-bit weights and ends in
// (acc + 32768) >> 16.  The source is fetched exactly as k_output_rgb fetches it (output_rgb.h): a unit
// of 16 consecutive pixels of one source row is one unaligned 16-byte luma load and 8 (4:4:4: 16) bytes
// per chroma plane and chroma row it needs, from the window's first column on -- rounded down to an
// even column where SubWidthC is 2, so that the unit starts on a chroma sample.  A unit that would
// reach past the crop's last column is the crop's LAST whole unit, fetched with the same wide loads and
// moved down in registers (scale_fetch; the samples that come in behind the last column repeat it, and
// weigh nothing) -- every output row ends in such units, and k_output_rgb's bytewise fetch, one round
// trip per sample, made the waves that hold them ten times as slow as the others.  Only a crop narrower
// than 16 is still fetched bytewise (scale_ld_clamped, output_rgb.h).  So nothing outside the crop is read.  Of the unit's 16 pixels the
// first `taps`, rounded up to a multiple of 4, are converted (job-wide: the widest window any output
// has, at most 16) and weighed: a pixel outside the lane's own window has weight 0, so the bounds that
// differ between lanes are predicates, not branches.
// A window wider than 16 columns (ratios above 14 : 1) walks several units; a whole frame to 1 x 1 is
// a serial loop in one lane.  The quotients (window bounds, the final mean) are by job-wide divisors:
// a binary32 product guesses them and one multiplication corrects the guess (scale_div).
//
// The 8-bit results of a workgroup -- SCALE_UNITS = 16 units of 16 output pixels, consecutive in the
// frame's unit order -- meet in 768 bytes of LDS; 16 threads then take one unit each and write it with
// k_output_rgb's rgb_write: the format's bytes interleaved in registers, 16-byte stores where the unit is
// whole and its destination aligned, dwords or bytes elsewhere, nothing outside the row.  What only
// these 16 threads need of the job -- the output side: offsets, pitch, format, scale and bias -- waits
// in LDS too (ScaleOut), so that it holds no SGPR while the windows are summed.
//
// Grid: x = groups of SCALE_UNITS units of one frame; y and z = frames, frame z * gridDim.y + y: no
// loop over frames, whose invariants the compiler would hoist and keep in SGPRs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "output_scale.h"

namespace h264r {

// What a thread needs of the job once its window is summed, as words of LDS: the mean's divisor, and
// what the threads that write a unit read.
enum ScaleOut : int {
    SO_PLANE_OFF = 0,          // 3 x 2 words
    SO_PITCH = 6,              // 2 words
    SO_FORMAT = 8, SO_BGR, SO_ALPHA,
    SO_SCALE = 11, SO_BIAS = 14,
    SO_FRAME = 17,             // 2 words: where the frame starts, from dst on
    SO_UNITS = 19, SO_UPR, SO_WIDTH,
    SO_T = 22, SO_INV_2T,
    SO_WORDS = 24,
};

// One frame of a job: this thread's output pixel as its 8-bit values into the workgroup's tile, then
// the tile's units to the frame.
template <int MODE, int FILTER>
__device__ __forceinline__ void scale_job(const ScaleJob& S, const h264r_out_frame* __restrict__ frames, uint8_t* dst, int* err)
{
    __shared__ uint32_t tile[3][SCALE_THREADS / 4];
    __shared__ uint32_t out[SO_WORDS];
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
    // this thread's output pixel: pixel threadIdx.x % 16 of unit blockIdx.x * 16 + threadIdx.x / 16
    const int upr = rgb_units_per_row(S.ax.D);
    const int units = S.ay.D * upr;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            out[SO_PLANE_OFF + 2 * p] = (uint32_t)J.plane_off[p];
            out[SO_PLANE_OFF + 2 * p + 1] = (uint32_t)(J.plane_off[p] >> 32);
            out[SO_SCALE + p] = __float_as_uint(J.scale[p]);
            out[SO_BIAS + p] = __float_as_uint(J.bias[p]);
        }
        out[SO_PITCH] = (uint32_t)J.pitch;
        out[SO_PITCH + 1] = (uint32_t)(J.pitch >> 32);
        out[SO_FORMAT] = (uint32_t)J.format;
        out[SO_BGR] = (uint32_t)J.bgr;
        out[SO_ALPHA] = (uint32_t)J.alpha;
        const uint64_t frame = (uint64_t)((int64_t)f * J.frame_stride);
        out[SO_FRAME] = (uint32_t)frame;
        out[SO_FRAME + 1] = (uint32_t)(frame >> 32);
        out[SO_UNITS] = (uint32_t)units;
        out[SO_UPR] = (uint32_t)upr;
        out[SO_WIDTH] = (uint32_t)S.ax.D;
        out[SO_T] = S.T;
        out[SO_INV_2T] = __float_as_uint(S.inv_2T);
    }
    __syncthreads();

    const int pu = (int)blockIdx.x * SCALE_UNITS + (int)(threadIdx.x / RGB_UNIT);
    // A thread behind the end of a row or of the frame sums the last pixel's window again: no lane mask
    // to keep, and none of its bytes is written.
    const int py = pu / upr;
    const int dy = min(py, S.ay.D - 1);
    const int dx = min((pu - py * upr) * RGB_UNIT + (int)(threadIdx.x % RGB_UNIT), S.ax.D - 1);
    uint32_t v[3];
    {
        uint32_t acc[3] = {0, 0, 0};
        scale_pixel<MODE, FILTER>(S, ScaleSrc{scale_kind(kind)}, yp, up, vp, dy, dx, acc);
        const uint32_t T = out[SO_T];
        const float inv_2T = __uint_as_float(out[SO_INV_2T]);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = FILTER == H264R_SCALE_AREA ? scale_div(2 * acc[c] + T, 2 * T, inv_2T) : (acc[c] + 32768u) >> 16;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) reinterpret_cast<uint8_t*>(tile[c])[threadIdx.x] = (uint8_t)v[c];
    __syncthreads();

    // the unit this thread writes, if it is one of the first 16
    const int unit = (int)blockIdx.x * SCALE_UNITS + (int)threadIdx.x;
    if (threadIdx.x < SCALE_UNITS && unit < (int)out[SO_UNITS]) {
        RgbJob W;                                           // the output side alone: all rgb_write reads
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            W.plane_off[p] = (int64_t)(out[SO_PLANE_OFF + 2 * p] | (uint64_t)out[SO_PLANE_OFF + 2 * p + 1] << 32);
            W.scale[p] = __uint_as_float(out[SO_SCALE + p]);
            W.bias[p] = __uint_as_float(out[SO_BIAS + p]);
        }
        W.pitch = (int64_t)(out[SO_PITCH] | (uint64_t)out[SO_PITCH + 1] << 32);
        // job-wide, and known to be: the format's branches stay branches of the wave
        W.format = __builtin_amdgcn_readfirstlane((int)out[SO_FORMAT]);
        W.bgr = __builtin_amdgcn_readfirstlane((int)out[SO_BGR]);
        W.alpha = (int)out[SO_ALPHA];
        RgbUnit t;
        t.r = unit / (int)out[SO_UPR];
        t.x = (unit - t.r * (int)out[SO_UPR]) * RGB_UNIT;
        t.n = min(RGB_UNIT, (int)out[SO_WIDTH] - t.x);
        uint32_t c[3][4];
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) c[p][q] = tile[p][4 * threadIdx.x + q];
        rgb_write(W, t, c, dst + (int64_t)(out[SO_FRAME] | (uint64_t)out[SO_FRAME + 1] << 32));
    }
}

}  // namespace h264r

using namespace h264r;

// four waves per SIMD at the least: a cap of 128 VGPRs, of which the kernels take 49 to 91
#define SCALE_KERNEL(NAME, MODE, FILTER)                                                                      \
    extern "C" __global__ void __launch_bounds__(SCALE_THREADS, 4)                                               \
    k_output_rgb_scaled_##NAME(ScaleJob job, const h264r_out_frame* __restrict__ frames, uint8_t* dst, int* err) \
    {                                                                                                         \
        scale_job<MODE, FILTER>(job, frames, dst, err);                                                       \
    }
H264R_SCALE_KERNELS(SCALE_KERNEL)
