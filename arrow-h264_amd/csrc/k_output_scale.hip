// k_output_scale.hip -- the k_output_rgb_scaled kernels: the scaled RGB frames of include/h264r_output.h
// (its comment is the definition; the names below are the header's).  One launch for every frame of a
// job, of the kernel for the job's RgbMode and filter: k_output_rgb_scaled_<mode>_<filter>, twelve in
// all (kernels.h).  One kernel for every mode and filter kept more scalars alive than there are SGPRs.
//
// A thread owns one OUTPUT pixel; adjacent lanes own adjacent pixels of an output row, so the source
// windows of a wave line up along the source rows and its loads cover one contiguous stretch of each.
// Both filters are one weighted window: columns [xlo, xhi) and rows [ylo, yhi) of the region of
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
// than 16 is still fetched bytewise (scale_ld_clamped).  So nothing outside the crop is read.  Of the unit's 16 pixels the
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
#include "output_rgb.h"

namespace h264r {

// rgb_ld_clamped's sixteen bytes (output_rgb.h), by a loop instead of sixteen predicated loads whose
// lane masks would be kept in SGPRs across the rows: from the last sample that exists down to the
// first, each pushed in at the bottom of 128 bits that start as the repeated last sample.  Narrow crops only.
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

// rgb_row (output_rgb.h) with the frame's kind as two integers instead of three lane masks: the parity
// of the rows of 128 (-1: none) and whether a plane holds every second row.  p1 is p0 unless the frame
// is a field pair, so the row's parity alone picks the plane.
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

// rgb_ld_chroma (output_rgb.h) over scale_ld_clamped
__device__ __forceinline__ uint4 scale_ld_chroma(const uint8_t* s, int i0, int cw, int mode, bool whole)
{
    if (!s) return make_uint4(RGB_GREY, RGB_GREY, RGB_GREY, RGB_GREY);
    const bool wide = mode < RGB_REP;
    if (!whole) return scale_ld_clamped(s, i0, cw - 1, wide ? 16 : 9);
    if (wide) return ld16u(s + i0);
    const uint2 a = ld8u(s + i0);
    const uint32_t next = mode >= RGB_BIL1 ? ld1(s + min(i0 + 8, cw - 1)) : 0u;
    return make_uint4(a.x, a.y, next, 0u);
}

// Pixel k of the unit: R, G, B by the header's matrix (RGB_GBR: the three samples as they are).  TWIN of
// rgb_convert (k_output.hip), which does the same for a unit's 16 pixels at once and stays as it was
// measured: a change to the matrix goes into both.  tests/test_gpu_output_scale.py holds the two
// together (a scaled frame at D = S is byte for byte the frame of h264r_output_rgb).
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

// The unit of RGB_UNIT source pixels of row r of the cropped rectangle from column x on (even where
// SubWidthC is 2): every load it needs.  The caller has set t.r, t.x and t.n = min(RGB_UNIT, lw - x).
// TWIN of rgb_fetch (k_output.hip), which finds row and column from a unit index and fetches a narrow
// crop's samples with predicated loads; a change to what a unit loads goes into both (see rgb_pixel).
template <int MODE>
__device__ __forceinline__ void rgb_fetch_at(const RgbJob& J, ScaleKind kind, const uint8_t* const (&yp)[2], const uint8_t* const (&up)[2],
                                             const uint8_t* const (&vp)[2], RgbUnit& t)
{
    const bool whole = t.n == RGB_UNIT;
    const uint8_t* const ys = scale_row(yp[0], yp[1], J.y0 + t.r, J.lpitch, kind);
    if (!ys) t.y = make_uint4(RGB_GREY, RGB_GREY, RGB_GREY, RGB_GREY);
    else if (whole) t.y = ld16u(ys + J.x0 + t.x);
    else t.y = scale_ld_clamped(ys + J.x0, t.x, J.lw - 1, RGB_UNIT);
    if (MODE == RGB_MONO) return;
    // the chroma rows j0 (and j1) of the cropped rectangle, and the unit's first chroma column
    const int i0 = MODE < RGB_REP ? t.x : t.x >> 1;
    int ja = t.r, jb = t.r;
    if (MODE >= RGB_REP && J.sub_h == 2) {
        ja = t.r >> 1;
        jb = (t.r & 1) ? min(ja + 1, J.ch - 1) : max(ja - 1, 0);
    }
    const uint8_t* const ur = scale_row(up[0], up[1], J.cy0 + ja, J.cpitch, kind);
    const uint8_t* const vr = scale_row(vp[0], vp[1], J.cy0 + ja, J.cpitch, kind);
    t.ua = scale_ld_chroma(ur ? ur + J.cx0 : nullptr, i0, J.cw, MODE, whole);
    t.va = scale_ld_chroma(vr ? vr + J.cx0 : nullptr, i0, J.cw, MODE, whole);
    if (MODE == RGB_BIL2) {
        const uint8_t* const ub = scale_row(up[0], up[1], J.cy0 + jb, J.cpitch, kind);
        const uint8_t* const vb = scale_row(vp[0], vp[1], J.cy0 + jb, J.cpitch, kind);
        t.ub = scale_ld_chroma(ub ? ub + J.cx0 : nullptr, i0, J.cw, MODE, whole);
        t.vb = scale_ld_chroma(vb ? vb + J.cx0 : nullptr, i0, J.cw, MODE, whole);
    }
}

// n / den for a quotient below 2^16: inv = 1 / den in binary32 guesses it to within one
__device__ __forceinline__ uint32_t scale_div(uint32_t n, uint32_t den, float inv)
{
    uint32_t q = (uint32_t)((float)n * inv);
    const int32_t rem = (int32_t)(n - q * den);
    if (rem < 0) --q;
    else if (rem >= (int32_t)den) ++q;
    return q;
}

// One axis of one output index d: the window [lo, hi) of source samples and what their weights need.
struct ScaleWin {
    int lo, hi;
    int a, b;                  // AREA: the interval [a, b) = [d S, (d + 1) S) in units of 1 / D; BILINEAR: w0, w1
};

__device__ __forceinline__ ScaleWin scale_window(const ScaleAxis& X, int d, int filter)
{
    ScaleWin w;
    if (filter == H264R_SCALE_AREA) {
        w.a = d * X.s;
        w.b = w.a + X.s;
        w.lo = (int)scale_div((uint32_t)w.a, (uint32_t)X.d, X.inv_d);
        w.hi = (int)scale_div((uint32_t)(w.b + X.d - 1), (uint32_t)X.d, X.inv_d);
    } else {
        const int p = min(max((2 * d + 1) * X.S - X.D, 0), 2 * X.D * (X.S - 1));
        w.lo = (int)scale_div((uint32_t)p, (uint32_t)(2 * X.D), X.inv_2D);
        const int f = p - 2 * X.D * w.lo;
        w.b = (int)scale_div((uint32_t)(256 * f + X.D), (uint32_t)(2 * X.D), X.inv_2D);
        w.a = 256 - w.b;
        w.hi = w.lo + (w.b ? 2 : 1);                      // w1 == 0 wherever i1 == i0
    }
    return w;
}

// the weight of source sample i (any integer; outside the window: 0)
__device__ __forceinline__ int scale_weight(const ScaleWin& w, int i, int D, int filter)
{
    if (filter == H264R_SCALE_AREA) return max(min(w.b, (i + 1) * D) - max(w.a, i * D), 0);
    return i == w.lo ? w.a : i == w.lo + 1 ? w.b : 0;
}

// v's 16 bytes moved down by sh (0..15); the bytes that come in at the top repeat its last
__device__ __forceinline__ uint4 scale_shr(uint4 v, int sh)
{
    const uint32_t rep = (v.w >> 24) * 0x01010101u;
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
    if (sh & 8) { w[0] = w[2]; w[1] = w[3]; w[2] = w[3] = rep; }
    if (sh & 4) { w[0] = w[1]; w[1] = w[2]; w[2] = w[3]; w[3] = rep; }
    const uint32_t bs = (uint32_t)sh & 3u;
    return make_uint4(__builtin_amdgcn_alignbyte(w[1], w[0], bs), __builtin_amdgcn_alignbyte(w[2], w[1], bs),
                      __builtin_amdgcn_alignbyte(w[3], w[2], bs), __builtin_amdgcn_alignbyte(rep, w[3], bs));
}

// eight chroma samples and the clamped ninth (SubWidthC 2) moved down by sh samples: those behind the
// crop's last repeat it, which is the clamp of the bilinear taps
__device__ __forceinline__ uint4 scale_shr8(uint4 v, int sh)
{
    const uint32_t rep = (v.y >> 24) * 0x01010101u;
    return scale_shr(make_uint4(v.x, v.y, rep, rep), sh);
}

// rgb_fetch_at for a unit at any column.  A unit that reaches past the crop's last column is, where
// the crop is 16 wide at least, the crop's LAST whole unit moved down in registers: wide loads of
// samples inside the crop and a byte shift, instead of the bytewise fetch (one round trip per sample).
template <int MODE>
__device__ __forceinline__ void scale_fetch(const RgbJob& J, ScaleKind kind, const uint8_t* const (&yp)[2], const uint8_t* const (&up)[2],
                                            const uint8_t* const (&vp)[2], RgbUnit& t)
{
    if (t.n == RGB_UNIT || J.lw < RGB_UNIT) {
        rgb_fetch_at<MODE>(J, kind, yp, up, vp, t);
        return;
    }
    RgbUnit b;
    b.r = t.r;
    b.x = J.lw - RGB_UNIT;
    b.n = RGB_UNIT;
    rgb_fetch_at<MODE>(J, kind, yp, up, vp, b);
    const int sh = t.x - b.x;                               // 1..15; even where SubWidthC is 2
    t.y = scale_shr(b.y, sh);
    if (MODE == RGB_MONO) return;
    if (MODE < RGB_REP) {
        t.ua = scale_shr(b.ua, sh);
        t.va = scale_shr(b.va, sh);
    } else {
        t.ua = scale_shr8(b.ua, sh >> 1);
        t.va = scale_shr8(b.va, sh >> 1);
        if (MODE == RGB_BIL2) {
            t.ub = scale_shr8(b.ub, sh >> 1);
            t.vb = scale_shr8(b.vb, sh >> 1);
        }
    }
}

// The three channel sums of output pixel (dy, dx) of one frame.
template <int MODE, int FILTER>
__device__ __forceinline__ void scale_pixel(const ScaleJob& S, ScaleKind kind, const uint8_t* const (&yp)[2], const uint8_t* const (&up)[2],
                                            const uint8_t* const (&vp)[2], int dy, int dx, uint32_t (&acc)[3])
{
    const RgbJob& J = S.rgb;
    const ScaleWin wx = scale_window(S.ax, dx, FILTER), wy = scale_window(S.ay, dy, FILTER);
    const int xend = S.roi_x + wx.hi;                       // columns and rows of the cropped rectangle from here on
    int xc = S.roi_x + wx.lo;
    if (MODE >= RGB_REP) xc &= ~1;
    do {                                                    // no window is empty
        int wh[RGB_UNIT];
#pragma unroll
        for (int q = 0; q < RGB_UNIT / 4; ++q) {
            const bool weighed = 4 * q < S.taps;            // job-wide: a branch, not a lane mask
#pragma unroll
            for (int k = 4 * q; k < 4 * q + 4; ++k) wh[k] = 0;
            if (weighed) {
#pragma unroll
                for (int k = 4 * q; k < 4 * q + 4; ++k) wh[k] = scale_weight(wx, xc + k - S.roi_x, S.ax.d, FILTER);
            }
        }
        RgbUnit t;
        t.x = xc;
        t.n = min(RGB_UNIT, J.lw - xc);
        int iy = wy.lo;
        do {
            t.r = S.roi_y + iy;
            scale_fetch<MODE>(J, kind, yp, up, vp, t);
            uint32_t row[3] = {0, 0, 0};
#pragma unroll
            for (int q = 0; q < RGB_UNIT / 4; ++q) {
                if (4 * q < S.taps) {                       // job-wide: four pixels at a time
#pragma unroll
                    for (int k = 4 * q; k < 4 * q + 4; ++k) {
                        int r, g, b;
                        rgb_pixel<MODE>(J, t, k, r, g, b);
                        row[0] += (uint32_t)__mul24(wh[k], r);
                        row[1] += (uint32_t)__mul24(wh[k], g);
                        row[2] += (uint32_t)__mul24(wh[k], b);
                    }
                }
            }
            const uint32_t wv = (uint32_t)scale_weight(wy, iy, S.ay.d, FILTER);
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += wv * row[c];
        } while (++iy < wy.hi);
    } while ((xc += RGB_UNIT) < xend);
}

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
    const uint8_t* const yp[2] = {y0, pair ? frames[f].y[1] : y0};                  // see scale_row
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
        scale_pixel<MODE, FILTER>(S, scale_kind(kind), yp, up, vp, dy, dx, acc);
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
