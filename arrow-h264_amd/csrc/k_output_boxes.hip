// k_output_boxes.hip -- the k_output_boxes kernels: boxes of scaled RGB from a device table,
// h264r_output_rgb_boxes of include/h264r_output.h (its comment is the definition).  The window and the
// pixel are the scaled kernels' own code (output_scale.h, see k_output_scale.hip's comment); what that
// kernel family takes job-wide as kernel arguments -- the axes with their divisors, the region, taps, T --
// differs from box to box here and comes out of memory.  Two launches per job:
//
// k_output_boxes_plan, one thread per box: the refusal rule (out_box_status, output_boxes.h: the function
// the host runs), then the box's frame-table entry -- kind and the planes the kind needs, tested before
// anything is dereferenced, as k_output_rgb_scaled tests them -- and a BoxPlan: per axis S, D, their
// reduced s, d (Euclid) and the reciprocals scale_div starts from, taps, T, the units of the box and
// where it goes.  A refused box gets a plan of 0 units and ORs DEV_ERR_OUTPUT into the error word.
//
// k_output_boxes_<mode>_<filter>, twelve as H264R_SCALE_KERNELS names them.  Grid: x = groups of
// SCALE_UNITS units of the LARGEST box the job admits (max_out_h rows of max_out_w pixels); y and z =
// boxes, box z * gridDim.y + y, so one launch holds more than 65,535.  A workgroup reads its box's plan
// -- one address for the whole workgroup -- and leaves, before any barrier, when its first unit is past
// the box's own count: a box smaller than the bound costs the workgroups it does not fill a load and a
// branch.  From there on it is k_output_rgb_scaled's workgroup: a thread per output pixel, the 8-bit
// results in 768 bytes of LDS, 16 threads that write a unit each with rgb_write -- at row dst_y + r,
// column dst_x + x of the box's image, so the 16-byte store path is chosen from the destination's
// address as in every other RGB kernel.  taps and the frame's kind go through readfirstlane: they are the
// same for the whole workgroup, and their branches stay branches of the wave.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "output_boxes.h"
#include "output_scale.h"

namespace h264r {

// What the threads that write a unit need, as words of LDS: k_output_rgb_scaled's ScaleOut and where the
// box goes.
enum BoxOut : int {
    BO_PLANE_OFF = 0,          // 3 x 2 words
    BO_PITCH = 6,              // 2 words
    BO_FORMAT = 8, BO_BGR, BO_ALPHA,
    BO_SCALE = 11, BO_BIAS = 14,
    BO_IMAGE = 17,             // 2 words: where the box's image starts, from dst on
    BO_UNITS = 19, BO_UPR, BO_WIDTH,
    BO_T = 22, BO_INV_2T,
    BO_DST_X = 24, BO_DST_Y,
    BO_WORDS = 26,
};

// The plan of box i, or the plan of no units.
__device__ __forceinline__ void boxes_plan(const BoxesJob& B, const h264r_out_frame* __restrict__ frames,
                                           const h264r_out_box* __restrict__ boxes, BoxPlan* __restrict__ plans, int* err, int i)
{
    const h264r_out_box b = boxes[i];
    BoxPlan P{};
    bool ok = out_box_status(b, B) == H264R_OK;
    if (ok) {                                               // b.frame is an entry of the table
        const h264r_out_frame& f = frames[b.frame];
        const int kind = f.kind;
        const bool pair = kind == H264R_OUT_FIELD_PAIR;
        ok = (unsigned)kind <= (unsigned)H264R_OUT_UNPAIRED_BOT && f.y[0] && (!pair || f.y[1]);
        if (B.rgb.mode != RGB_MONO) ok = ok && f.u[0] && f.v[0] && (!pair || (f.u[1] && f.v[1]));
        P.kind = kind;
    }
    if (!ok) {
        atomicOr(err, DEV_ERR_OUTPUT);
        plans[i] = BoxPlan{};
        return;
    }
    const int32_t sw = b.roi_w ? b.roi_w : B.rgb.lw, sh = b.roi_h ? b.roi_h : B.rgb.lh;
    const int32_t gw = box_gcd(sw, b.out_w), gh = box_gcd(sh, b.out_h);
    P.ax.S = sw; P.ax.D = b.out_w; P.ax.s = sw / gw; P.ax.d = b.out_w / gw;
    P.ay.S = sh; P.ay.D = b.out_h; P.ay.s = sh / gh; P.ay.d = b.out_h / gh;
    P.ax.inv_d = 1.0f / (float)P.ax.d; P.ax.inv_2D = 1.0f / (float)(2 * P.ax.D);
    P.ay.inv_d = 1.0f / (float)P.ay.d; P.ay.inv_2D = 1.0f / (float)(2 * P.ay.D);
    P.roi_x = b.roi_x; P.roi_y = b.roi_y;
    // the widest window of columns, as scale_plan (host_output.hip) has it
    const int span = (B.filter == H264R_SCALE_AREA ? (P.ax.s + P.ax.d - 1) / P.ax.d + 1 : 2) + (B.rgb.mode >= RGB_REP ? 1 : 0);
    P.taps = min(span, RGB_UNIT);
    P.T = B.filter == H264R_SCALE_AREA ? (uint32_t)P.ax.s * (uint32_t)P.ay.s : 1u;     // <= 2^23: not refused
    P.inv_2T = 1.0f / (2.0f * (float)P.T);
    P.upr = rgb_units_per_row(b.out_w);
    P.units = b.out_h * P.upr;
    P.frame = b.frame; P.image = b.image;
    P.dst_x = b.dst_x; P.dst_y = b.dst_y;
    plans[i] = P;
}

// One box of a job: this thread's output pixel as its 8-bit values into the workgroup's tile, then the
// tile's units to the box's place in its image.
template <int MODE, int FILTER>
__device__ __forceinline__ void boxes_job(const BoxesJob& B, const h264r_out_frame* __restrict__ frames,
                                          const BoxPlan* __restrict__ plans, uint8_t* dst)
{
    __shared__ uint32_t tile[3][SCALE_THREADS / 4];
    __shared__ uint32_t out[BO_WORDS];
    const int box = (int)(blockIdx.z * gridDim.y + blockIdx.y);
    if (box >= B.num_boxes) return;
    const BoxPlan& P = plans[box];
    const int units = P.units;
    if ((int)blockIdx.x * SCALE_UNITS >= units) return;     // a refused box has none
    ScaleJob S;
    S.rgb = B.rgb;
    S.ax = P.ax;
    S.ay = P.ay;
    S.roi_x = P.roi_x; S.roi_y = P.roi_y;
    S.filter = FILTER;
    S.taps = __builtin_amdgcn_readfirstlane(P.taps);
    S.T = P.T;
    S.inv_2T = P.inv_2T;
    const RgbJob& J = S.rgb;
    // the plan kernel has tested the kind and the planes it needs
    const int f = P.frame;
    const int kind = __builtin_amdgcn_readfirstlane(P.kind);
    const bool pair = kind == H264R_OUT_FIELD_PAIR;
    const uint8_t* const y0 = frames[f].y[0];
    const uint8_t* const u0 = MODE == RGB_MONO ? nullptr : frames[f].u[0];
    const uint8_t* const v0 = MODE == RGB_MONO ? nullptr : frames[f].v[0];
    const uint8_t* const yp[2] = {y0, pair ? frames[f].y[1] : y0};                  // see scale_row (output_rgb.h)
    const uint8_t* const up[2] = {u0, pair && MODE != RGB_MONO ? frames[f].u[1] : u0};
    const uint8_t* const vp[2] = {v0, pair && MODE != RGB_MONO ? frames[f].v[1] : v0};
    const int upr = P.upr;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            out[BO_PLANE_OFF + 2 * p] = (uint32_t)J.plane_off[p];
            out[BO_PLANE_OFF + 2 * p + 1] = (uint32_t)(J.plane_off[p] >> 32);
            out[BO_SCALE + p] = __float_as_uint(J.scale[p]);
            out[BO_BIAS + p] = __float_as_uint(J.bias[p]);
        }
        out[BO_PITCH] = (uint32_t)J.pitch;
        out[BO_PITCH + 1] = (uint32_t)(J.pitch >> 32);
        out[BO_FORMAT] = (uint32_t)J.format;
        out[BO_BGR] = (uint32_t)J.bgr;
        out[BO_ALPHA] = (uint32_t)J.alpha;
        const uint64_t image = (uint64_t)((int64_t)P.image * J.frame_stride);
        out[BO_IMAGE] = (uint32_t)image;
        out[BO_IMAGE + 1] = (uint32_t)(image >> 32);
        out[BO_UNITS] = (uint32_t)units;
        out[BO_UPR] = (uint32_t)upr;
        out[BO_WIDTH] = (uint32_t)S.ax.D;
        out[BO_T] = S.T;
        out[BO_INV_2T] = __float_as_uint(S.inv_2T);
        out[BO_DST_X] = (uint32_t)P.dst_x;
        out[BO_DST_Y] = (uint32_t)P.dst_y;
    }
    __syncthreads();

    // this thread's output pixel: pixel threadIdx.x % 16 of unit blockIdx.x * 16 + threadIdx.x / 16 of the box.
    // A thread behind the end of a row or of the box sums the last pixel's window again: no lane mask
    // to keep, and none of its bytes is written.
    const int pu = (int)blockIdx.x * SCALE_UNITS + (int)(threadIdx.x / RGB_UNIT);
    const int py = pu / upr;
    const int dy = min(py, S.ay.D - 1);
    const int dx = min((pu - py * upr) * RGB_UNIT + (int)(threadIdx.x % RGB_UNIT), S.ax.D - 1);
    uint32_t v[3];
    {
        uint32_t acc[3] = {0, 0, 0};
        scale_pixel<MODE, FILTER>(S, ScaleSrc{scale_kind(kind)}, yp, up, vp, dy, dx, acc);
        const uint32_t T = out[BO_T];
        const float inv_2T = __uint_as_float(out[BO_INV_2T]);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = FILTER == H264R_SCALE_AREA ? scale_div(2 * acc[c] + T, 2 * T, inv_2T) : (acc[c] + 32768u) >> 16;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) reinterpret_cast<uint8_t*>(tile[c])[threadIdx.x] = (uint8_t)v[c];
    __syncthreads();

    // the unit this thread writes, if it is one of the first 16
    const int unit = (int)blockIdx.x * SCALE_UNITS + (int)threadIdx.x;
    if (threadIdx.x < SCALE_UNITS && unit < (int)out[BO_UNITS]) {
        RgbJob W;                                           // the output side alone: all rgb_write reads
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            W.plane_off[p] = (int64_t)(out[BO_PLANE_OFF + 2 * p] | (uint64_t)out[BO_PLANE_OFF + 2 * p + 1] << 32);
            W.scale[p] = __uint_as_float(out[BO_SCALE + p]);
            W.bias[p] = __uint_as_float(out[BO_BIAS + p]);
        }
        W.pitch = (int64_t)(out[BO_PITCH] | (uint64_t)out[BO_PITCH + 1] << 32);
        // job-wide, and known to be: the format's branches stay branches of the wave
        W.format = __builtin_amdgcn_readfirstlane((int)out[BO_FORMAT]);
        W.bgr = __builtin_amdgcn_readfirstlane((int)out[BO_BGR]);
        W.alpha = (int)out[BO_ALPHA];
        const int r = unit / (int)out[BO_UPR];
        const int x = (unit - r * (int)out[BO_UPR]) * RGB_UNIT;
        RgbUnit t;                                          // the unit's place in the IMAGE
        t.r = (int)out[BO_DST_Y] + r;
        t.x = (int)out[BO_DST_X] + x;
        t.n = min(RGB_UNIT, (int)out[BO_WIDTH] - x);
        uint32_t c[3][4];
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) c[p][q] = tile[p][4 * threadIdx.x + q];
        rgb_write(W, t, c, dst + (int64_t)(out[BO_IMAGE] | (uint64_t)out[BO_IMAGE + 1] << 32));
    }
}

}  // namespace h264r

using namespace h264r;

extern "C" __global__ void __launch_bounds__(BOXES_PLAN_THREADS)
k_output_boxes_plan(BoxesJob job, const h264r_out_frame* __restrict__ frames, const h264r_out_box* __restrict__ boxes,
                    BoxPlan* __restrict__ plans, int* err)
{
    const int i = (int)(blockIdx.x * BOXES_PLAN_THREADS + threadIdx.x);
    if (i < job.num_boxes) boxes_plan(job, frames, boxes, plans, err, i);
}

// the scaled kernels' bounds: four waves per SIMD at the least, a cap of 128 VGPRs
#define BOXES_KERNEL(NAME, MODE, FILTER)                                                                             \
    extern "C" __global__ void __launch_bounds__(SCALE_THREADS, 4)                                                      \
    k_output_boxes_##NAME(BoxesJob job, const h264r_out_frame* __restrict__ frames, const BoxPlan* __restrict__ plans, uint8_t* dst) \
    {                                                                                                                \
        boxes_job<MODE, FILTER>(job, frames, plans, dst);                                                            \
    }
H264R_SCALE_KERNELS(BOXES_KERNEL)
