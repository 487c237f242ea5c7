/* h264r_deinterlace.h -- motion-adaptive deinterlacing of field pairs in the device-side output stage.
 *
 * h264r_output.h weaves: H264R_OUT_FIELD_PAIR interleaves the two fields of a frame, and every RGB call
 * treats the woven frame as progressive.  Wherever something moves between the two fields the woven frame
 * is combed.  h264r_deinterlace writes, from the same frame table, whole progressive pictures: the rows
 * of one field kept, the rows of the other parity interpolated -- from the kept field alone
 * (H264R_DEINT_BOB) or from the kept field and the fields around it in time (H264R_DEINT_ADAPTIVE).
 * The reference has no deinterlacer; what follows is the definition, complete: every output byte is an
 * exact integer function of the source bytes.  Its structure is that of the well-known "yadif" filter
 * with every border resolved by clamping, so there is no special case; no other tool's bytes are claimed.
 *
 * Sources.  The frame table is the h264r_out_frame array of h264r_output.h; each entry is one interlaced
 * frame, either woven already (H264R_OUT_FRAME: a frame picture, an MBAFF frame, a DPB slot) or a pair
 * of field pictures (H264R_OUT_FIELD_PAIR).  "Field p of a source" (p = 0 top, 1 bottom) is rows
 * 2 m + p of the first kind and plane [p] of the second; the result does not depend on which kind names
 * the same bytes.  A job (h264r_deint_job) names the frame `cur` whose field `keep` is kept, and the
 * frames before and after it in time, `prev` and `next` (-1: none).
 *
 * Output.  Output frame j, at dst + j * dst_frame_stride, is three CODED-SIZE planes Y, Cb, Cr (a 4:0:0
 * context: luma alone): plane_pitch[k] is the coded width of plane k, plane_off[k + 1] = plane_off[k] +
 * plane_pitch[k] * coded rows of plane k (planes a 4:0:0 frame does not have: 0 and 0), frame_bytes their
 * sum.  Only the bytes inside each plane's cropped rectangle -- the one h264r_output_geometry computes,
 * returned as rect[k] = x0, y0, w, h -- are written, and nothing outside it is read: no sample outside the
 * crop has any influence.  The result is named to the other output calls, with the same `desc`, as an
 * H264R_OUT_FRAME source: y[0] = dst + j * dst_frame_stride + plane_off[0], u[0] with plane_off[1], v[0]
 * with plane_off[2].  dst may have any alignment; rows whose destination allows it leave as 16-byte
 * stores.  dst MUST NOT overlap any source plane of the job: that is the caller's rule, nothing tests it.
 *
 * The definition, per plane, w x h its cropped rectangle (h is even, below).  All values 32-bit signed.
 *   Hf = h / 2, q = 1 - keep.
 *   X_p[m][x]: field p of source X inside the crop, m in 0 .. Hf - 1, x in 0 .. w - 1 (field parity is
 *   counted inside the crop; y0 is even, so it is the coded parity).
 *   C, P, N: the sources cur, prev, next; P = C if prev == -1, N = C if next == -1.
 *   cl(a) = min(max(a, 0), Hf - 1), cx(a) = min(max(a, 0), w - 1).
 * Kept rows:  out[2 m + keep][x] = C_keep[m][x].
 * Interpolated rows out[2 m + q][x]:
 *   K = C_keep, Pb = P_keep, Pa = N_keep.
 *   (Qb, Qa) = (P_q, C_q) if second == 0, else (C_q, N_q): the fields of the other parity just before
 *   and just after the kept field in time.
 *   ia = cl(m + q - 1), ib = cl(m + q); c = K[ia][x], e = K[ib][x].
 *   H264R_DEINT_BOB:       out = (c + e + 1) >> 1.
 *   H264R_DEINT_ADAPTIVE:
 *     d  = (Qb[m][x] + Qa[m][x]) >> 1
 *     t0 = |Qb[m][x] - Qa[m][x]|
 *     t1 = (|Pb[ia][x] - c| + |Pb[ib][x] - e|) >> 1;  t2 the same with Pa
 *     diff = max(t0 >> 1, t1, t2)
 *     S(j)  = sum over k = -1 .. 1 of |K[ia][cx(x + k + j)] - K[ib][cx(x + k - j)]|
 *     pr(j) = (K[ia][cx(x + j)] + K[ib][cx(x - j)]) >> 1
 *     sp = (c + e) >> 1, score = S(0) - 1
 *     for s = -1, then s = +1:
 *         if S(s) < score:  score = S(s), sp = pr(s);
 *             and only then, if S(2 s) < score:  score = S(2 s), sp = pr(2 s)
 *     mu = cl(m - 1), md = cl(m + 1)
 *     b = (Qb[mu][x] + Qa[mu][x]) >> 1;  f the same with md
 *     mx = max(d - e, d - c, min(b - c, f - e))
 *     mn = min(d - e, d - c, max(b - c, f - e))
 *     diff = max(diff, mn, -mx)
 *     out = min(max(sp, d - diff), d + diff)
 * No shift is ever applied to a negative number, and the result is always in 0 .. 255.
 * Why these pieces: d is the temporal guess (the missing sample as it was just before and after), sp the
 * spatial one (the kept field's neighbours, along the edge direction of the smallest difference), and
 * diff how far the spatial guess may pull away from the temporal one: as far as anything moved -- between
 * the two fields of the missing parity (t0), or between the kept field and its own parity before (t1) and
 * after (t2) -- widened where the vertical neighbourhood says the temporal guess overshoots (mn, -mx).
 * Where nothing moves diff is 0 and out = d: the woven sample.  Where everything moves out = sp: a bob
 * along edges.
 *
 * Additive, as h264r_group.h: no structure of h264r.h or h264r_output.h changes, H264R_ABI_VERSION stays.
 */
#ifndef H264R_DEINTERLACE_H_
#define H264R_DEINTERLACE_H_

#include <stdint.h>

#include "h264r_output.h"

#ifdef __cplusplus
extern "C" {
#endif

#define H264R_DEINT_BOB       0   /* spatial only, from the kept field */
#define H264R_DEINT_ADAPTIVE  1   /* the spatio-temporal filter defined above */

/* What one workgroup of the kernel owns, in samples of a plane's cropped rectangle (columns, frame rows):
 * for tests around its edges. */
#define H264R_DEINT_TILE_W    32
#define H264R_DEINT_TILE_H    64

typedef struct h264r_deint_job {      /* 24 bytes; the job table is a DEVICE array, one record per OUTPUT frame */
    int32_t cur, prev, next;          /* indices into the frame table; prev / next: -1 = none (P = C, N = C) */
    int32_t keep;                     /* 0: keep the top field's rows, interpolate the bottom's; 1: the reverse */
    int32_t second;                   /* 1: the kept field is the later in time of its frame's two fields */
    int32_t mode;                     /* H264R_DEINT_* */
} h264r_deint_job;

typedef struct h264r_deint_geom {     /* filled by h264r_deinterlace_geometry */
    int32_t rect[3][4];               /* x0, y0, w, h of the cropped rectangle inside plane k (4:0:0: [1], [2] zero) */
    int64_t plane_off[3], plane_pitch[3];
    int64_t frame_bytes;
} h264r_deint_geom;

/* Host only, no GPU needed.  H264R_EINVAL: whatever h264r_output_geometry refuses, and layout !=
 * H264R_OUT_PLANAR, pitch_align > 1 or fake_chroma != 0.  H264R_EUNSUPPORTED, after those: a plane whose
 * rectangle has an odd y0 or an odd height (never with frame_mbs_only == 0; with frame_mbs_only == 1 an
 * odd crop does it). */
int h264r_deinterlace_geometry(int chroma_format_idc, const h264r_out_desc* desc, h264r_deint_geom* geom);

/* Host only.  H264R_EINVAL: job NULL, num_frames < 0, cur outside 0 .. num_frames - 1, prev or next
 * outside -1 .. num_frames - 1, keep or second not 0 / 1, mode not an H264R_DEINT_*; else H264R_OK.  The
 * rule the device applies to every record of the job table. */
int h264r_deint_job_status(const h264r_deint_job* job, int num_frames);

/* Write num_jobs output frames, frame j at dst + j * dst_frame_stride from jobs[j], by the geometry of
 * `desc` for the context's chroma format.  One kernel launch for every job and plane; asynchronous on
 * `stream` with the stream rule of h264r_output_frames: planes a decode of this context has just written
 * on another stream are read without a host synchronisation.
 * Statuses: H264R_EINVAL for a NULL ctx, desc, frames, jobs or dst and for a negative count; then those of
 * h264r_deinterlace_geometry; then H264R_EINVAL for dst_frame_stride < frame_bytes.  num_jobs == 0 is
 * H264R_OK and does nothing.
 * The tables are read on the device, and their mistakes are found there, each tested before anything is
 * dereferenced, as h264r_output_frames treats a bad frame: the rule of h264r_deint_job_status, then the
 * sources.  H264R_DEINT_ADAPTIVE needs cur, prev and next (where not -1) each of kind H264R_OUT_FRAME or
 * H264R_OUT_FIELD_PAIR with the non-NULL planes that kind needs (y[0], y[1] of a pair, the same of u and
 * v except on a 4:0:0 context).  H264R_DEINT_BOB reads cur only -- its prev and next are range-checked and
 * never dereferenced -- and its cur may also be H264R_OUT_UNPAIRED_TOP with keep == 0 or
 * H264R_OUT_UNPAIRED_BOT with keep == 1: a whole picture from an unpaired field instead of rows of 128.
 * A refused job writes no byte and ORs the output stage's bit into the context's error word, so
 * h264r_check returns H264R_EDEVICE; every other job of the call is written. */
int h264r_deinterlace(h264r_ctx* ctx, const h264r_out_desc* desc, const h264r_out_frame* frames /*device*/,
                      int num_frames, const h264r_deint_job* jobs /*device*/, int num_jobs, uint8_t* dst /*device*/,
                      int64_t dst_frame_stride, void* stream);

#ifdef __cplusplus
}
#endif

#endif  /* H264R_DEINTERLACE_H_ */
