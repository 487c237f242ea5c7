// host_output.hip -- the output stage of include/h264r_output.h on the host: the geometry and layout
// of cropped, RGB, scaled and resampled RGB frames and of the images of a boxes job, the plans of the
// resampler (its tables come from resample_tables.h), the planes of a deinterlaced frame
// (include/h264r_deinterlace.h), and the launches of k_output.hip / k_output_scale.hip / k_output_boxes.hip /
// k_output_resample.hip / k_deinterlace.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "h264r.h"
#include "h264r_output.h"
#include "host_ctx.h"
#include "kernels.h"
#include "output_boxes.h"
#include "resample_tables.h"

// ------------------------------------------------------------- output stage (h264r_output.h)
// The planes of one output frame: the geometry (output.cc:135-165) and the layout, as the job k_output
// takes and, for the caller, as an h264r_out_geom.
static int output_plan(int fmt, const h264r_out_desc* d, h264r_out_geom* g, h264r::OutJob* job)
{
    if (!d || fmt < 0 || fmt > 3 || d->width_mbs <= 0 || d->frame_height_mbs <= 0 ||
        d->width_mbs > H264R_OUT_MAX_MBS || d->frame_height_mbs > H264R_OUT_MAX_MBS ||
        (d->frame_mbs_only != 0 && d->frame_mbs_only != 1) ||
        (d->layout != H264R_OUT_PLANAR && d->layout != H264R_OUT_SEMIPLANAR))
        return H264R_EINVAL;
    const int pa = d->pitch_align;
    if (pa < 0 || pa > H264R_OUT_MAX_PITCH_ALIGN || (pa & (pa - 1))) return H264R_EINVAL;
    if (d->crop_left < 0 || d->crop_right < 0 || d->crop_top < 0 || d->crop_bottom < 0) return H264R_EINVAL;
    if (d->fake_chroma && fmt != 0) return H264R_EUNSUPPORTED;
    const int sub_w = (fmt == 1 || fmt == 2) ? 2 : 1, sub_h = fmt == 1 ? 2 : 1;    // 4:0:0: CropUnitX 1
    const int mb_cw = fmt ? 16 / sub_w : 0, mb_ch = fmt ? 16 / sub_h : 0;
    const int64_t uy = 2 - d->frame_mbs_only;
    const int64_t lc = d->crop_left, rc = d->crop_right, tc = d->crop_top * uy, bc = d->crop_bottom * uy;
    const int64_t lw = 16 * (int64_t)d->width_mbs - sub_w * (lc + rc);
    const int64_t lh = 16 * (int64_t)d->frame_height_mbs - sub_h * (tc + bc);
    const int64_t cw = fmt ? mb_cw * (int64_t)d->width_mbs - (lc + rc) : 0;
    const int64_t ch = fmt ? mb_ch * (int64_t)d->frame_height_mbs - (tc + bc) : 0;
    if (lw <= 0 || lh <= 0 || (fmt && (cw <= 0 || ch <= 0))) return H264R_EINVAL;

    h264r::OutJob J{};
    auto plane = [&](int mode, int64_t w, int64_t h, int64_t x0, int64_t y0, int src_pitch) {
        h264r::OutPlane& p = J.pl[J.nplanes];
        p.off = J.nplanes ? J.pl[J.nplanes - 1].off + J.pl[J.nplanes - 1].pitch * J.pl[J.nplanes - 1].h : 0;
        p.pitch = pa > 1 ? (w + pa - 1) / pa * pa : w;
        p.w = (int32_t)w; p.h = (int32_t)h; p.x0 = (int32_t)x0; p.y0 = (int32_t)y0;
        p.src_pitch = src_pitch; p.mode = mode;
        ++J.nplanes;
    };
    plane(h264r::OUT_COPY_Y, lw, lh, sub_w * lc, sub_h * tc, 16 * d->width_mbs);
    const bool semi = d->layout == H264R_OUT_SEMIPLANAR;
    if (fmt) {
        const int cp = mb_cw * d->width_mbs;
        if (semi) plane(h264r::OUT_INTERLEAVE, 2 * cw, ch, lc, tc, cp);
        else { plane(h264r::OUT_COPY_U, cw, ch, lc, tc, cp); plane(h264r::OUT_COPY_V, cw, ch, lc, tc, cp); }
    } else if (d->fake_chroma) {
        const int64_t fu = lw * lh / 4;                          // WriteUV (output.cc:205-224): one run per plane
        if (fu > 0) {
            if (semi) plane(h264r::OUT_FILL, 2 * fu, 1, 0, 0, 0);
            else { plane(h264r::OUT_FILL, fu, 1, 0, 0, 0); plane(h264r::OUT_FILL, fu, 1, 0, 0, 0); }
        }
    }
    J.need_chroma = fmt != 0;
    const h264r::OutPlane& last = J.pl[J.nplanes - 1];
    const int64_t frame_bytes = last.off + last.pitch * last.h;
    if (g) {
        *g = h264r_out_geom{};
        const int32_t l[4] = {(int32_t)(sub_w * lc), (int32_t)(sub_h * tc), (int32_t)lw, (int32_t)lh};
        const int32_t cr[4] = {(int32_t)lc, (int32_t)tc, (int32_t)cw, (int32_t)ch};
        for (int k = 0; k < 4; ++k) { g->luma[k] = l[k]; g->chroma[k] = fmt ? cr[k] : 0; }
        for (int k = 0; k < J.nplanes; ++k) { g->plane_off[k] = J.pl[k].off; g->plane_pitch[k] = J.pl[k].pitch; }
        g->frame_bytes = frame_bytes;
    }
    if (job) { *job = J; job->frame_stride = frame_bytes; }
    return H264R_OK;
}

// The stream an output launch goes to: the caller's, or the context's.  The sources are, as a rule, what
// the context's last launch wrote: ordered as run_batch orders launches.
static int output_stream(h264r_ctx* c, void* stream, hipStream_t* s)
{
    (void)hipSetDevice(c->device);
    *s = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
    return h264r::order_after_last(c, *s);
}

int h264r_output_geometry(int chroma_format_idc, const h264r_out_desc* desc, h264r_out_geom* geom)
{
    if (!geom) return H264R_EINVAL;
    return output_plan(chroma_format_idc, desc, geom, nullptr);
}

int h264r_output_frames(h264r_ctx* c, const h264r_out_desc* desc, const h264r_out_frame* frames, int num_frames,
                        uint8_t* dst, int64_t dst_frame_stride, void* stream)
{
    if (!c || !frames || !dst || num_frames < 0) return H264R_EINVAL;
    h264r::OutJob job;
    const int st = output_plan(c->fmt, desc, nullptr, &job);
    if (st != H264R_OK) return st;
    if (dst_frame_stride < job.frame_stride) return H264R_EINVAL;
    if (num_frames == 0) return H264R_OK;
    job.frame_stride = dst_frame_stride;
    job.num_frames = num_frames;
    hipStream_t s;
    if (const int e = output_stream(c, stream, &s)) return e;
    int items = 0;
    for (int k = 0; k < job.nplanes; ++k)
        items = std::max(items, job.pl[k].h * h264r::out_chunks_per_row(job.pl[k].w));
    const int per = h264r::OUT_THREADS * h264r::OUT_ITEMS;
    const dim3 grid((unsigned)((items + per - 1) / per), (unsigned)std::min(num_frames, 65535), (unsigned)job.nplanes);
    hipLaunchKernelGGL(k_output, grid, dim3(h264r::OUT_THREADS), 0, s, job, frames, dst, c->d_err.p);
    HIP_OK(hipGetLastError());
    return H264R_OK;
}

// ------------------------------------------------------------- deinterlaced frames (h264r_deinterlace.h)
// The coded-size planes of one deinterlaced frame and the cropped rectangle inside each: for the caller as
// an h264r_deint_geom, and as the job k_deinterlace takes.  Argument errors come before what is merely
// unsupported.
static int deint_plan(int fmt, const h264r_out_desc* d, h264r_deint_geom* g, h264r::DeintJob* job)
{
    if (!d || d->layout != H264R_OUT_PLANAR || d->pitch_align > 1 || d->fake_chroma != 0) return H264R_EINVAL;
    h264r_out_geom og;
    const int st = output_plan(fmt, d, &og, nullptr);
    if (st != H264R_OK) return st;
    const int nplanes = fmt ? 3 : 1;
    const int32_t* const rect[3] = {og.luma, og.chroma, og.chroma};
    for (int k = 0; k < nplanes; ++k)
        if ((rect[k][1] | rect[k][3]) & 1) return H264R_EUNSUPPORTED;
    const int sub_w = (fmt == 1 || fmt == 2) ? 2 : 1, sub_h = fmt == 1 ? 2 : 1;
    const int64_t pitch[3] = {16 * (int64_t)d->width_mbs, 16 / sub_w * (int64_t)d->width_mbs, 16 / sub_w * (int64_t)d->width_mbs};
    const int64_t rows[3] = {16 * (int64_t)d->frame_height_mbs, 16 / sub_h * (int64_t)d->frame_height_mbs,
                             16 / sub_h * (int64_t)d->frame_height_mbs};
    int64_t off[3] = {0, 0, 0}, frame_bytes = 0;
    for (int k = 0; k < nplanes; ++k) { off[k] = frame_bytes; frame_bytes += pitch[k] * rows[k]; }
    if (g) {
        *g = h264r_deint_geom{};
        for (int k = 0; k < nplanes; ++k) {
            for (int i = 0; i < 4; ++i) g->rect[k][i] = rect[k][i];
            g->plane_off[k] = off[k];
            g->plane_pitch[k] = pitch[k];
        }
        g->frame_bytes = frame_bytes;
    }
    if (job) {
        h264r::DeintJob J{};
        for (int k = 0; k < nplanes; ++k) {
            h264r::DeintPlane& p = J.pl[k];
            p.off = off[k];
            p.pitch = (int32_t)pitch[k];
            p.x0 = rect[k][0]; p.y0 = rect[k][1]; p.w = rect[k][2]; p.h = rect[k][3];
            p.tiles_x = (p.w + h264r::DEINT_TW - 1) / h264r::DEINT_TW;
            p.tiles = p.tiles_x * ((p.h + h264r::DEINT_TH - 1) / h264r::DEINT_TH);
            p.which = k;
        }
        J.nplanes = nplanes;
        J.need_chroma = fmt != 0;
        J.frame_stride = frame_bytes;
        *job = J;
    }
    return H264R_OK;
}

int h264r_deinterlace_geometry(int chroma_format_idc, const h264r_out_desc* desc, h264r_deint_geom* geom)
{
    if (!geom) return H264R_EINVAL;
    return deint_plan(chroma_format_idc, desc, geom, nullptr);
}

int h264r_deint_job_status(const h264r_deint_job* job, int num_frames)
{
    if (!job || num_frames < 0) return H264R_EINVAL;
    const bool ok = job->cur >= 0 && job->cur < num_frames && job->prev >= -1 && job->prev < num_frames && job->next >= -1 &&
                    job->next < num_frames && (job->keep == 0 || job->keep == 1) && (job->second == 0 || job->second == 1) &&
                    (job->mode == H264R_DEINT_BOB || job->mode == H264R_DEINT_ADAPTIVE);
    return ok ? H264R_OK : H264R_EINVAL;
}

int h264r_deinterlace(h264r_ctx* c, const h264r_out_desc* desc, const h264r_out_frame* frames, int num_frames,
                      const h264r_deint_job* jobs, int num_jobs, uint8_t* dst, int64_t dst_frame_stride, void* stream)
{
    if (!c || !desc || !frames || !jobs || !dst || num_frames < 0 || num_jobs < 0) return H264R_EINVAL;
    h264r::DeintJob job;
    const int st = deint_plan(c->fmt, desc, nullptr, &job);
    if (st != H264R_OK) return st;
    if (dst_frame_stride < job.frame_stride) return H264R_EINVAL;
    if (num_jobs == 0) return H264R_OK;
    job.frame_stride = dst_frame_stride;
    job.num_frames = num_frames;
    job.num_jobs = num_jobs;
    hipStream_t s;
    if (const int e = output_stream(c, stream, &s)) return e;
    int tiles = 0;
    for (int k = 0; k < job.nplanes; ++k) tiles = std::max(tiles, job.pl[k].tiles);
    const int gx = (tiles + h264r::DEINT_GROUP - 1) / h264r::DEINT_GROUP * h264r::DEINT_GROUP;
    // job z / nplanes * grid.y + y, plane z % nplanes: one launch holds any number of jobs
    const int gy = std::min(num_jobs, 16384);
    const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)(job.nplanes * ((num_jobs + gy - 1) / gy)));
    hipLaunchKernelGGL(k_deinterlace, grid, dim3(h264r::DEINT_THREADS), 0, s, job, frames, jobs, dst, c->d_err.p);
    HIP_OK(hipGetLastError());
    return H264R_OK;
}

// ------------------------------------------------------------- RGB frames (h264r_output.h)
int h264r_rgb_coefficients(int matrix, int full_range, int32_t out[6])
{
    // floor(real * 2^14 + 1/2) of the header's reals: cy, crv, cgu, cgv, cbu, yo
    static const int32_t rows[3][2][6] = {
        {{19077, 26149, -6419, -13320, 33050, 16}, {16384, 22970, -5638, -11700, 29032, 0}},   // BT.601
        {{19077, 29372, -3494, -8731, 34610, 16}, {16384, 25802, -3069, -7670, 30402, 0}},     // BT.709
        {{19077, 27503, -3069, -10657, 35091, 16}, {16384, 24160, -2696, -9361, 30825, 0}},    // BT.2020
    };
    if (!out || matrix < H264R_CSC_BT601 || matrix > H264R_CSC_BT2020 || (full_range != 0 && full_range != 1))
        return H264R_EINVAL;
    for (int k = 0; k < 6; ++k) out[k] = rows[matrix][full_range][k];
    return H264R_OK;
}

// The layout of one RGB frame of w x h pixels: for the caller as an h264r_rgb_geom, and as the output
// side of the job the RGB kernels take.
static void rgb_layout(int format, int64_t pa, int64_t w, int64_t h, h264r_rgb_geom* g, h264r::RgbJob* job)
{
    const bool planar = format == H264R_RGB_PLANAR_U8 || format == H264R_RGB_PLANAR_F16;
    const int64_t bpp = format == H264R_RGB_PACKED_U8 ? 3 : format == H264R_RGB_PACKED_U8X4 ? 4 :
                        format == H264R_RGB_PLANAR_F16 ? 2 : 1;
    const int64_t pitch = pa > 1 ? (bpp * w + pa - 1) / pa * pa : bpp * w;
    const int64_t frame_bytes = (planar ? 3 : 1) * pitch * h;
    if (g) {
        *g = h264r_rgb_geom{};
        g->width = (int32_t)w; g->height = (int32_t)h;
        for (int k = 0; k < (planar ? 3 : 1); ++k) { g->plane_off[k] = k * pitch * h; g->plane_pitch[k] = pitch; }
        g->frame_bytes = frame_bytes;
    }
    if (job) {
        for (int k = 0; k < 3; ++k) job->plane_off[k] = planar ? k * pitch * h : 0;
        job->pitch = pitch;
        job->frame_stride = frame_bytes;
    }
}

// what both RGB entry points require of dst: room for every frame, and binary16 at even addresses
static bool rgb_dst_ok(const h264r::RgbJob& job, const void* dst, int64_t dst_frame_stride)
{
    if (dst_frame_stride < job.frame_stride) return false;
    return job.format != H264R_RGB_PLANAR_F16 || !((reinterpret_cast<uintptr_t>(dst) | (uint64_t)dst_frame_stride) & 1);
}

// What RGB frames are made from: the descriptor checked, the size of the cropped rectangle of desc->src
// (known wherever the status is H264R_OK or H264R_EUNSUPPORTED) and the source side of the job: all of
// it but the layout.
static int rgb_source(int fmt, const h264r_rgb_desc* d, int32_t size[2], h264r::RgbJob* job)
{
    if (!d || d->src.layout != H264R_OUT_PLANAR || d->src.fake_chroma != 0) return H264R_EINVAL;
    h264r_out_geom og;
    const int st = output_plan(fmt, &d->src, &og, nullptr);
    if (st != H264R_OK) return st;
    size[0] = og.luma[2]; size[1] = og.luma[3];
    if (d->matrix < H264R_CSC_BT601 || d->matrix > H264R_CSC_GBR ||
        (d->chroma_up != H264R_UP_REPLICATE && d->chroma_up != H264R_UP_BILINEAR) ||
        d->format < H264R_RGB_PACKED_U8 || d->format > H264R_RGB_PLANAR_F16 ||
        (d->full_range != 0 && d->full_range != 1) || (d->bgr != 0 && d->bgr != 1) || d->alpha < 0 || d->alpha > 255)
        return H264R_EINVAL;
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(d->scale[k]) || !std::isfinite(d->bias[k])) return H264R_EINVAL;
    if (d->matrix == H264R_CSC_GBR && fmt != 3) return H264R_EUNSUPPORTED;

    if (job) {
        h264r::RgbJob J{};
        J.lw = og.luma[2]; J.lh = og.luma[3]; J.x0 = og.luma[0]; J.y0 = og.luma[1];
        J.cx0 = og.chroma[0]; J.cy0 = og.chroma[1]; J.cw = og.chroma[2]; J.ch = og.chroma[3];
        J.lpitch = 16 * d->src.width_mbs;
        J.cpitch = fmt == 3 ? J.lpitch : fmt ? J.lpitch / 2 : 0;
        J.sub_h = fmt == 1 ? 2 : 1;
        const bool bil = d->chroma_up == H264R_UP_BILINEAR;
        J.mode = fmt == 0 ? h264r::RGB_MONO : fmt == 3 ? (d->matrix == H264R_CSC_GBR ? h264r::RGB_GBR : h264r::RGB_FULL) :
                 !bil ? h264r::RGB_REP : fmt == 2 ? h264r::RGB_BIL1 : h264r::RGB_BIL2;
        J.format = d->format; J.bgr = d->bgr; J.alpha = d->alpha;
        if (d->matrix != H264R_CSC_GBR) {
            int32_t k[6];
            h264r_rgb_coefficients(d->matrix, d->full_range, k);
            J.cy = k[0]; J.crv = k[1]; J.cgu = k[2]; J.cgv = k[3]; J.cbu = k[4]; J.yo = k[5];
        }
        for (int k = 0; k < 3; ++k) { J.scale[k] = d->scale[k]; J.bias[k] = d->bias[k]; }
        *job = J;
    }
    return H264R_OK;
}

// The layout of one RGB frame and the job k_output_rgb takes, from the geometry of desc->src.
static int rgb_plan(int fmt, const h264r_rgb_desc* d, h264r_rgb_geom* g, h264r::RgbJob* job)
{
    int32_t size[2];
    const int st = rgb_source(fmt, d, size, job);
    if (st == H264R_OK) rgb_layout(d->format, d->src.pitch_align, size[0], size[1], g, job);
    return st;
}

int h264r_output_rgb_geometry(int chroma_format_idc, const h264r_rgb_desc* desc, h264r_rgb_geom* geom)
{
    if (!geom) return H264R_EINVAL;
    return rgb_plan(chroma_format_idc, desc, geom, nullptr);
}

int h264r_output_rgb(h264r_ctx* c, const h264r_rgb_desc* desc, const h264r_out_frame* frames, int num_frames,
                     void* dst, int64_t dst_frame_stride, void* stream)
{
    if (!c || !frames || !dst || num_frames < 0) return H264R_EINVAL;
    h264r::RgbJob job;
    const int st = rgb_plan(c->fmt, desc, nullptr, &job);
    if (st != H264R_OK) return st;
    if (!rgb_dst_ok(job, dst, dst_frame_stride)) return H264R_EINVAL;
    if (num_frames == 0) return H264R_OK;
    job.frame_stride = dst_frame_stride;
    job.num_frames = num_frames;
    hipStream_t s;
    if (const int e = output_stream(c, stream, &s)) return e;
    const int units = job.lh * h264r::rgb_units_per_row(job.lw);
    const int per = h264r::RGB_THREADS * h264r::RGB_ITEMS;
    const dim3 grid((unsigned)((units + per - 1) / per), (unsigned)std::min(num_frames, 65535));
    hipLaunchKernelGGL(k_output_rgb, grid, dim3(h264r::RGB_THREADS), 0, s, job, frames, static_cast<uint8_t*>(dst),
                       c->d_err.p);
    HIP_OK(hipGetLastError());
    return H264R_OK;
}

// ------------------------------------------------------------- scaled RGB frames (h264r_output.h)
static int64_t gcd64(int64_t a, int64_t b)
{
    while (b) { const int64_t t = a % b; a = b; b = t; }
    return a;
}

// The layout of one scaled frame and the job the k_output_rgb_scaled kernels take.  Argument errors come before
// what is merely unsupported, as in rgb_source.
static int scale_plan(int fmt, const h264r_scale_desc* d, h264r_rgb_geom* g, h264r::ScaleJob* job)
{
    if (!d) return H264R_EINVAL;
    int32_t full[2];                                         // rgb_source knows the size before it finds GBR off 4:4:4
    h264r::RgbJob R;
    const int st = rgb_source(fmt, &d->rgb, full, &R);
    if (st != H264R_OK && st != H264R_EUNSUPPORTED) return st;
    if (d->roi_x < 0 || d->roi_y < 0 || d->roi_w < 0 || d->roi_h < 0 || (d->roi_w == 0) != (d->roi_h == 0) ||
        d->out_w < 1 || d->out_w > H264R_SCALE_MAX_OUT || d->out_h < 1 || d->out_h > H264R_SCALE_MAX_OUT ||
        (d->filter != H264R_SCALE_BILINEAR && d->filter != H264R_SCALE_AREA) || d->pad != 0)
        return H264R_EINVAL;
    const int64_t sw = d->roi_w ? d->roi_w : full[0], sh = d->roi_h ? d->roi_h : full[1];
    if (d->roi_x + sw > full[0] || d->roi_y + sh > full[1]) return H264R_EINVAL;
    if (st != H264R_OK) return st;
    const int64_t gw = gcd64(sw, d->out_w), gh = gcd64(sh, d->out_h);
    const int64_t rw = sw / gw, rh = sh / gh;
    if (d->filter == H264R_SCALE_AREA && rw * rh > h264r::SCALE_AREA_MAX_T) return H264R_EUNSUPPORTED;

    rgb_layout(d->rgb.format, d->rgb.src.pitch_align, d->out_w, d->out_h, g, &R);
    if (job) {
        h264r::ScaleJob J{};
        J.rgb = R;
        auto axis = [](int64_t S, int64_t D, int64_t gc) {
            h264r::ScaleAxis a;
            a.S = (int32_t)S; a.D = (int32_t)D; a.s = (int32_t)(S / gc); a.d = (int32_t)(D / gc);
            a.inv_d = 1.0f / (float)a.d; a.inv_2D = 1.0f / (float)(2 * a.D);
            return a;
        };
        J.ax = axis(sw, d->out_w, gw);
        J.ay = axis(sh, d->out_h, gh);
        J.roi_x = d->roi_x; J.roi_y = d->roi_y;
        J.filter = d->filter;
        // the widest window of columns: floor(d s / D) .. ceil((d + 1) s / D) holds ceil(s / D) + 1 at most
        // (bilinear: 2), and one more in front where the unit starts on the even column before it
        const int64_t span = (d->filter == H264R_SCALE_AREA ? (J.ax.s + J.ax.d - 1) / J.ax.d + 1 : 2) + (R.mode >= h264r::RGB_REP ? 1 : 0);
        J.taps = (int32_t)std::min<int64_t>(span, h264r::RGB_UNIT);
        J.T = (uint32_t)(rw * rh);
        J.inv_2T = 1.0f / (2.0f * (float)J.T);
        *job = J;
    }
    return H264R_OK;
}

int h264r_output_rgb_scaled_geometry(int chroma_format_idc, const h264r_scale_desc* desc, h264r_rgb_geom* geom)
{
    if (!geom) return H264R_EINVAL;
    return scale_plan(chroma_format_idc, desc, geom, nullptr);
}

int h264r_output_rgb_scaled(h264r_ctx* c, const h264r_scale_desc* desc, const h264r_out_frame* frames, int num_frames,
                            void* dst, int64_t dst_frame_stride, void* stream)
{
    if (!c || !frames || !dst || num_frames < 0) return H264R_EINVAL;
    h264r::ScaleJob job;
    const int st = scale_plan(c->fmt, desc, nullptr, &job);
    if (st != H264R_OK) return st;
    if (!rgb_dst_ok(job.rgb, dst, dst_frame_stride)) return H264R_EINVAL;
    if (num_frames == 0) return H264R_OK;
    job.rgb.frame_stride = dst_frame_stride;
    job.rgb.num_frames = num_frames;
    hipStream_t s;
    if (const int e = output_stream(c, stream, &s)) return e;
    // the kernel of the job's mode and filter; frame z * grid.y + y, so that one launch holds any number
    using ScaleKernel = void (*)(h264r::ScaleJob, const h264r_out_frame*, uint8_t*, int*);
    ScaleKernel kernel[h264r::RGB_BIL2 + 1][2] = {};
#define H264R_SCALE_KERNEL_ENTRY(NAME, MODE, FILTER) kernel[MODE][FILTER] = k_output_rgb_scaled_##NAME;
    H264R_SCALE_KERNELS(H264R_SCALE_KERNEL_ENTRY)
#undef H264R_SCALE_KERNEL_ENTRY
    const int units = job.ay.D * h264r::rgb_units_per_row(job.ax.D);
    const int gy = std::min(num_frames, 65535);
    const dim3 grid((unsigned)((units + h264r::SCALE_UNITS - 1) / h264r::SCALE_UNITS), (unsigned)gy, (unsigned)((num_frames + gy - 1) / gy));
    hipLaunchKernelGGL(kernel[job.rgb.mode][job.filter], grid, dim3(h264r::SCALE_THREADS), 0, s, job, frames,
                       static_cast<uint8_t*>(dst), c->d_err.p);
    HIP_OK(hipGetLastError());
    return H264R_OK;
}

// ------------------------------------------------------------- resampled RGB frames (h264r_output.h)
// A plan: the job the k_output_rgb_resampled kernels take, whose table pointers are into `tab`.
struct h264r_resample_plan {
    h264r_ctx* ctx = nullptr;         // compared, never dereferenced: a plan may outlive its context
    int device = 0;
    h264r::ResampleJob job{};
    h264r::DevBuf<int32_t> tab;       // xmin, count, kk of the columns, then of the rows
    int lds_bytes = 0;
};

// The region and the layout of one resampled frame, and the job's RGB side.  Argument errors come before
// what is merely unsupported, as in scale_plan.  in[] = in0, in1 of the columns, then of the rows.
static int resample_plan(int fmt, const h264r_resample_desc* d, h264r_rgb_geom* g, h264r::RgbJob* job, int32_t in[4])
{
    if (!d) return H264R_EINVAL;
    int32_t full[2];
    h264r::RgbJob R;
    const int st = rgb_source(fmt, &d->rgb, full, &R);
    if (st != H264R_OK && st != H264R_EUNSUPPORTED) return st;
    if (d->roi_x < 0 || d->roi_y < 0 || d->roi_w < 0 || d->roi_h < 0 || (d->roi_w == 0) != (d->roi_h == 0) ||
        d->out_w < 1 || d->out_w > H264R_SCALE_MAX_OUT || d->out_h < 1 || d->out_h > H264R_SCALE_MAX_OUT ||
        d->filter < H264R_RESAMPLE_TRIANGLE || d->filter > H264R_RESAMPLE_LANCZOS || d->pad != 0)
        return H264R_EINVAL;
    const int64_t sw = d->roi_w ? d->roi_w : full[0], sh = d->roi_h ? d->roi_h : full[1];
    if (d->roi_x + sw > full[0] || d->roi_y + sh > full[1]) return H264R_EINVAL;
    if (st != H264R_OK) return st;
    const int32_t r[4] = {d->roi_x, (int32_t)(d->roi_x + sw), d->roi_y, (int32_t)(d->roi_y + sh)};
    if (h264r::resample_ksize(d->filter, r[0], r[1], d->out_w) > H264R_RESAMPLE_MAX_TAPS ||
        h264r::resample_ksize(d->filter, r[2], r[3], d->out_h) > H264R_RESAMPLE_MAX_TAPS)
        return H264R_EUNSUPPORTED;
    rgb_layout(d->rgb.format, d->rgb.src.pitch_align, d->out_w, d->out_h, g, &R);
    if (job) *job = R;
    if (in) for (int k = 0; k < 4; ++k) in[k] = r[k];
    return H264R_OK;
}

int h264r_output_rgb_resampled_geometry(int chroma_format_idc, const h264r_resample_desc* desc, h264r_rgb_geom* geom)
{
    if (!geom) return H264R_EINVAL;
    return resample_plan(chroma_format_idc, desc, geom, nullptr, nullptr);
}

int h264r_resample_axis(int filter, int in_size, int in0, int in1, int out_size, int32_t* xmin, int32_t* count, int32_t* kk,
                        int32_t* ksize)
{
    return h264r::resample_axis(filter, in_size, in0, in1, out_size, xmin, count, kk, ksize);
}

int h264r_resample_plan_create(h264r_ctx* c, const h264r_resample_desc* desc, h264r_resample_plan** plan)
{
    if (!c || !desc || !plan) return H264R_EINVAL;
    *plan = nullptr;
    h264r::ResampleJob J{};
    int32_t in[4];
    const int st = resample_plan(c->fmt, desc, nullptr, &J.rgb, in);
    if (st != H264R_OK) return st;
    // both axes on the host: xmin [D], count [D], kk [D][ksize] each, one after the other
    const int32_t size[2] = {J.rgb.lw, J.rgb.lh}, D[2] = {desc->out_w, desc->out_h};
    int32_t ks[2];
    size_t off[2], words = 0;
    for (int a = 0; a < 2; ++a) {
        if (h264r::resample_axis(desc->filter, size[a], in[2 * a], in[2 * a + 1], D[a], nullptr, nullptr, nullptr, &ks[a])) return H264R_EINVAL;
        off[a] = words;
        words += (size_t)D[a] * (2 + (size_t)ks[a]);
    }
    std::vector<int32_t> host(words);
    for (int a = 0; a < 2; ++a) {
        int32_t* const p = host.data() + off[a];
        if (h264r::resample_axis(desc->filter, size[a], in[2 * a], in[2 * a + 1], D[a], p, p + D[a], p + 2 * (size_t)D[a], &ks[a])) return H264R_EINVAL;
    }
    // the tiling: the widest tile's columns (from an even column where SubWidthC is 2, in whole units), the
    // highest tile's rows, and as many rows a step as the LDS holds
    const bool even = J.rgb.mode >= h264r::RGB_REP;
    auto span = [&](int a, int tile, bool units) {
        const int32_t* const lo = host.data() + off[a];
        const int32_t* const n = lo + D[a];
        int most = 0;
        for (int first = 0; first < D[a]; first += tile) {
            const int last = std::min(first + tile, D[a]) - 1;
            const int from = units && even ? lo[first] & ~1 : lo[first];
            const int len = lo[last] + n[last] - from;
            most = std::max(most, units ? (len + h264r::RGB_UNIT - 1) / h264r::RGB_UNIT * h264r::RGB_UNIT : len);
        }
        return most;
    };
    J.strip_cols = span(0, h264r::RS_TW, true);
    J.span_rows = span(1, h264r::RS_TH, false);
    J.tiles_x = (D[0] + h264r::RS_TW - 1) / h264r::RS_TW;
    J.tiles_y = (D[1] + h264r::RS_TH - 1) / h264r::RS_TH;
    J.step_rows = std::min(16, J.span_rows);
    while (J.step_rows > 1 && h264r::rs_lds_bytes(ks[0], ks[1], J.strip_cols, J.span_rows, J.step_rows) > h264r::RS_LDS_MAX) J.step_rows /= 2;
    const int lds = h264r::rs_lds_bytes(ks[0], ks[1], J.strip_cols, J.span_rows, J.step_rows);
    if (lds > h264r::RS_LDS_MAX || (int64_t)J.tiles_x * J.tiles_y > 0x7fffffff) return H264R_EUNSUPPORTED;   // H264R_RESAMPLE_MAX_TAPS rules it out

    h264r_resample_plan* const p = new (std::nothrow) h264r_resample_plan;
    if (!p) return H264R_ENOMEM;
    (void)hipSetDevice(c->device);
    if (const int e = p->tab.reserve(words)) { delete p; return e; }
    if (hipMemcpy(p->tab.p, host.data(), words * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) { delete p; return H264R_EDEVICE; }
    h264r::ResampleAxis* const ax[2] = {&J.ax, &J.ay};
    for (int a = 0; a < 2; ++a) {
        ax[a]->xmin = p->tab.p + off[a];
        ax[a]->count = ax[a]->xmin + D[a];
        ax[a]->kk = ax[a]->count + D[a];
        ax[a]->D = D[a];
        ax[a]->ksize = ks[a];
    }
    p->ctx = c;
    p->device = c->device;
    p->job = J;
    p->lds_bytes = lds;
    *plan = p;
    return H264R_OK;
}

void h264r_resample_plan_destroy(h264r_resample_plan* plan)
{
    if (!plan) return;
    (void)hipSetDevice(plan->device);
    delete plan;
}

int h264r_output_rgb_resampled(h264r_ctx* c, const h264r_resample_plan* plan, const h264r_out_frame* frames, int num_frames,
                               void* dst, int64_t dst_frame_stride, void* stream)
{
    if (!c || !plan || plan->ctx != c || !frames || !dst || num_frames < 0) return H264R_EINVAL;
    if (!rgb_dst_ok(plan->job.rgb, dst, dst_frame_stride)) return H264R_EINVAL;
    if (num_frames == 0) return H264R_OK;
    h264r::ResampleJob job = plan->job;
    job.rgb.frame_stride = dst_frame_stride;
    job.rgb.num_frames = num_frames;
    hipStream_t s;
    if (const int e = output_stream(c, stream, &s)) return e;
    // the kernel of the job's mode; frame z * grid.y + y, so that one launch holds any number
    using ResampleKernel = void (*)(h264r::ResampleJob, const h264r_out_frame*, uint8_t*, int*);
    ResampleKernel kernel[h264r::RGB_BIL2 + 1] = {};
#define H264R_RESAMPLE_KERNEL_ENTRY(NAME, MODE) kernel[MODE] = k_output_rgb_resampled_##NAME;
    H264R_RESAMPLE_KERNELS(H264R_RESAMPLE_KERNEL_ENTRY)
#undef H264R_RESAMPLE_KERNEL_ENTRY
    const int gy = std::min(num_frames, 65535);
    const dim3 grid((unsigned)(job.tiles_x * job.tiles_y), (unsigned)gy, (unsigned)((num_frames + gy - 1) / gy));
    hipLaunchKernelGGL(kernel[job.rgb.mode], grid, dim3(h264r::RS_THREADS), (size_t)plan->lds_bytes, s, job, frames,
                       static_cast<uint8_t*>(dst), c->d_err.p);
    HIP_OK(hipGetLastError());
    return H264R_OK;
}

// ------------------------------------------------------------- boxes of scaled RGB (h264r_output.h)
// The layout of one image and the job the k_output_boxes kernels take: all of it but the tables' sizes.
// Argument errors come before what is merely unsupported, as in scale_plan; with H264R_EUNSUPPORTED the
// job holds what bounds a box (the cropped rectangle, the image, max_out, the filter) and nothing else.
static int boxes_plan(int fmt, const h264r_boxes_desc* d, h264r_rgb_geom* g, h264r::BoxesJob* job)
{
    if (!d) return H264R_EINVAL;
    int32_t full[2];
    h264r::RgbJob R;
    const int st = rgb_source(fmt, &d->rgb, full, &R);
    if (st != H264R_OK && st != H264R_EUNSUPPORTED) return st;
    if (d->image_w < 1 || d->image_w > H264R_SCALE_MAX_OUT || d->image_h < 1 || d->image_h > H264R_SCALE_MAX_OUT ||
        d->max_out_w < 1 || d->max_out_w > d->image_w || d->max_out_h < 1 || d->max_out_h > d->image_h ||
        (d->filter != H264R_SCALE_BILINEAR && d->filter != H264R_SCALE_AREA) || d->pad != 0)
        return H264R_EINVAL;
    if (st != H264R_OK) {                                   // the bounds of a box are known all the same
        if (job) {
            *job = h264r::BoxesJob{};
            job->rgb.lw = full[0]; job->rgb.lh = full[1];
            job->image_w = d->image_w; job->image_h = d->image_h;
            job->max_out_w = d->max_out_w; job->max_out_h = d->max_out_h;
            job->filter = d->filter;
        }
        return st;
    }
    rgb_layout(d->rgb.format, d->rgb.src.pitch_align, d->image_w, d->image_h, g, &R);
    if (job) {
        h264r::BoxesJob J{};
        J.rgb = R;
        J.image_w = d->image_w; J.image_h = d->image_h;
        J.max_out_w = d->max_out_w; J.max_out_h = d->max_out_h;
        J.filter = d->filter;
        *job = J;
    }
    return H264R_OK;
}

int h264r_output_rgb_boxes_geometry(int chroma_format_idc, const h264r_boxes_desc* desc, h264r_rgb_geom* geom)
{
    if (!geom) return H264R_EINVAL;
    return boxes_plan(chroma_format_idc, desc, geom, nullptr);
}

int h264r_out_box_status(int chroma_format_idc, const h264r_boxes_desc* desc, const h264r_out_box* box, int num_frames,
                         int num_images)
{
    if (!box || num_frames < 0 || num_images < 0) return H264R_EINVAL;
    h264r::BoxesJob job;
    const int st = boxes_plan(chroma_format_idc, desc, nullptr, &job);
    if (st != H264R_OK && st != H264R_EUNSUPPORTED) return st;
    job.rgb.num_frames = num_frames;
    job.num_images = num_images;
    const int bs = h264r::out_box_status(*box, job);
    // every argument error before anything unsupported: the descriptor's, then the box's
    return bs == H264R_EINVAL || st == H264R_OK ? bs : st;
}

int h264r_output_rgb_boxes(h264r_ctx* c, const h264r_boxes_desc* desc, const h264r_out_frame* frames, int num_frames,
                           const h264r_out_box* boxes, int num_boxes, void* dst, int64_t dst_image_stride, int num_images,
                           void* stream)
{
    if (!c || !frames || !boxes || !dst || num_frames < 0 || num_boxes < 0 || num_images < 0) return H264R_EINVAL;
    h264r::BoxesJob job;
    const int st = boxes_plan(c->fmt, desc, nullptr, &job);
    if (st != H264R_OK) return st;
    if (!rgb_dst_ok(job.rgb, dst, dst_image_stride)) return H264R_EINVAL;
    if (num_boxes == 0) return H264R_OK;
    job.rgb.frame_stride = dst_image_stride;
    job.rgb.num_frames = num_frames;
    job.num_boxes = num_boxes;
    job.num_images = num_images;
    hipStream_t s;
    if (const int e = output_stream(c, stream, &s)) return e;
    // the plans: the buffer grows only when a job has more boxes than any before it
    if (const int e = c->d_box_plans.reserve((size_t)num_boxes)) return e;
    hipLaunchKernelGGL(k_output_boxes_plan, dim3((unsigned)((num_boxes + h264r::BOXES_PLAN_THREADS - 1) / h264r::BOXES_PLAN_THREADS)),
                       dim3(h264r::BOXES_PLAN_THREADS), 0, s, job, frames, boxes, c->d_box_plans.p, c->d_err.p);
    HIP_OK(hipGetLastError());
    // the kernel of the job's mode and filter; box z * grid.y + y, so that one launch holds any number
    using BoxesKernel = void (*)(h264r::BoxesJob, const h264r_out_frame*, const h264r::BoxPlan*, uint8_t*);
    BoxesKernel kernel[h264r::RGB_BIL2 + 1][2] = {};
#define H264R_BOXES_KERNEL_ENTRY(NAME, MODE, FILTER) kernel[MODE][FILTER] = k_output_boxes_##NAME;
    H264R_SCALE_KERNELS(H264R_BOXES_KERNEL_ENTRY)
#undef H264R_BOXES_KERNEL_ENTRY
    const int units = job.max_out_h * h264r::rgb_units_per_row(job.max_out_w);
    const int gy = std::min(num_boxes, 65535);
    const dim3 grid((unsigned)((units + h264r::SCALE_UNITS - 1) / h264r::SCALE_UNITS), (unsigned)gy, (unsigned)((num_boxes + gy - 1) / gy));
    hipLaunchKernelGGL(kernel[job.rgb.mode][job.filter], grid, dim3(h264r::SCALE_THREADS), 0, s, job, frames,
                       static_cast<const h264r::BoxPlan*>(c->d_box_plans.p), static_cast<uint8_t*>(dst));
    HIP_OK(hipGetLastError());
    return H264R_OK;
}
