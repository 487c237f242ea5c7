/* h264r_output.h -- the device-side output stage behind the C ABI.
 *
 * The library reconstructs coded-size planar planes: a frame picture as (16 H) x (16 W) luma rows,
 * a field picture as a picture of half the frame's rows, a 4:0:0 picture as luma alone (h264r.h).
 * The reference turns those into the frames it writes with three host functions:
 *
 *   reference                                            here
 *   ---------------------------------------------------  -----------------------------------------
 *   write_out_picture        output.cc:109-227            h264r_output_frames, kind H264R_OUT_FRAME
 *     SPS cropping           output.cc:135-165            h264r_output_geometry
 *     img2buf, Y / Cb / Cr   output.cc:61-106, 186-203    layout H264R_OUT_PLANAR
 *     4:0:0: U = V = 128     output.cc:205-224            fake_chroma
 *   dpb_combine_field_yuv    picture.cc:578-622           kind H264R_OUT_FIELD_PAIR
 *   write_unpaired_field     output.cc:229-263            kinds H264R_OUT_UNPAIRED_TOP / _BOT
 *     storable_picture::clear picture.cc:129-143            (the missing parity's rows are 128)
 *
 * h264r_output_frames does this on the GPU, from planes that are already there (the out planes of
 * an h264r_batch, the DPB slots of h264r_ref_planes, any device buffer of the right size) into one
 * device buffer of display-size frames, in the order of the caller's frame table: output order is
 * the caller's (the reference's is its DPB's, dpb.cc).  Nothing is copied to the host.
 *
 * Geometry.  SubWidthC / SubHeightC are 2 / 2 (4:2:0), 2 / 1 (4:2:2), 1 / 1 (4:4:4, 4:0:0).  The
 * crop offsets count chroma samples horizontally and chroma rows x (2 - frame_mbs_only) vertically
 * (7.4.2.1.1; output.cc:147-157), so the cropped luma rectangle is
 *     x0 = SubWidthC  * crop_left,  width  = 16 * width_mbs        - SubWidthC  * (crop_left + crop_right)
 *     y0 = SubHeightC * top,        height = 16 * frame_height_mbs - SubHeightC * (top + bottom)
 * with top / bottom = crop_top / crop_bottom x (2 - frame_mbs_only), and the chroma rectangle is
 * (crop_left, top, MbWidthC * width_mbs - (crop_left + crop_right), MbHeightC * frame_height_mbs -
 * (top + bottom)).  A 4:0:0 context has no chroma rectangle (all zero).
 *
 * Layout of one output frame.  H264R_OUT_PLANAR: the luma rows, the Cb rows, the Cr rows.
 * H264R_OUT_SEMIPLANAR: the luma rows, then the chroma rows of 2 x width bytes Cb Cr Cb Cr ...
 * (NV12 for 4:2:0, NV16 for 4:2:2, NV24 for 4:4:4).  plane_pitch[k] is the distance in bytes between
 * the rows of plane k: the row's bytes for pitch_align 0 or 1 (the frame is then the reference's bytes),
 * else those rounded up to a multiple of pitch_align; plane_off[k + 1] = plane_off[k] + plane_pitch[k] x
 * rows of plane k, and frame_bytes is that sum over all planes (the padding of the last row included).
 * Planes a layout does not have get plane_off = plane_pitch = 0.
 * A 4:0:0 context with fake_chroma writes, after the luma, what the reference's WriteUV writes: two runs
 * (planar) of (lw * lh) / 4 bytes of 128, or one run (semi-planar) of twice that; each run counts as ONE
 * row of its plane (plane_pitch = its bytes, rounded up as above), because (lw * lh) / 4 is not a
 * rectangle when lw or lh is odd.  Without fake_chroma the frame is the luma plane alone.
 *
 * Additive: no structure of h264r.h changes and H264R_ABI_VERSION stays what it is, as for
 * h264r_group.h.
 */
#ifndef H264R_OUTPUT_H_
#define H264R_OUTPUT_H_

#include <stdint.h>

#include "h264r.h"

#ifdef __cplusplus
extern "C" {
#endif

#define H264R_OUT_PLANAR      0   /* Y, Cb, Cr: the reference's file layout (output.cc:186-203) */
#define H264R_OUT_SEMIPLANAR  1   /* Y, then rows of interleaved Cb Cr (NV12 / NV16 / NV24)    */

#define H264R_OUT_MAX_MBS     1024   /* width_mbs, frame_height_mbs of a descriptor             */
#define H264R_OUT_MAX_PITCH_ALIGN 4096

typedef struct h264r_out_desc {
    int32_t width_mbs, frame_height_mbs;      /* the FRAME (a field picture has half its rows)   */
    int32_t crop_left, crop_right, crop_top, crop_bottom;   /* SPS syntax units                  */
    int32_t frame_mbs_only;                   /* 0 or 1: vertical crop unit x (2 - frame_mbs_only) */
    int32_t layout;                           /* H264R_OUT_*                                     */
    int32_t pitch_align;                      /* 0 or 1: rows contiguous (the reference's bytes);
                                                 else a power of two <= 4096: every row of every
                                                 plane starts at a multiple of it inside the frame */
    int32_t fake_chroma;                      /* 4:0:0 context only: 1 = the reference's U = V = 128
                                                 planes (output.cc:205-224), 0 = luma alone       */
} h264r_out_desc;

typedef struct h264r_out_geom {               /* filled by h264r_output_geometry */
    int32_t luma[4], chroma[4];               /* x0, y0, width, height inside the coded planes    */
    int64_t plane_off[3], plane_pitch[3];     /* inside one output frame (semi-planar: [2] unused) */
    int64_t frame_bytes;
} h264r_out_geom;

#define H264R_OUT_FRAME         0   /* src 0: a frame (a frame picture, an MBAFF frame, or a DPB slot) */
#define H264R_OUT_FIELD_PAIR    1   /* src 0: the top field picture, src 1: the bottom field picture   */
#define H264R_OUT_UNPAIRED_TOP  2   /* src 0: a top field; the other parity's rows are 128             */
#define H264R_OUT_UNPAIRED_BOT  3   /* src 0: a bottom field; the other parity's rows are 128          */
/* One output frame; the frame table is a DEVICE array of these (56 bytes each).  A frame source is
 * three planes of the frame's coded size; a field source three planes of half its rows (frame row 2 r
 * is the top field's row r, frame row 2 r + 1 the bottom field's, in every plane; the crop applies to
 * the woven frame).  Planes are unpadded, pitch == coded width, and nothing outside them is read (they
 * need no H264R_PLANE_SLACK).  On a 4:0:0 context u and v are never read. */
typedef struct h264r_out_frame {
    int32_t kind, pad;
    const uint8_t* y[2]; const uint8_t* u[2]; const uint8_t* v[2];   /* [1]: H264R_OUT_FIELD_PAIR only */
} h264r_out_frame;

/* Host only, no GPU needed.  H264R_EINVAL: a NULL argument, chroma_format_idc outside 0..3, sizes
 * outside 1..H264R_OUT_MAX_MBS, frame_mbs_only not 0 / 1, a negative crop, a crop that leaves nothing,
 * a bad layout, a pitch_align that is neither 0, 1 nor a power of two <= 4096.  H264R_EUNSUPPORTED:
 * fake_chroma with chroma_format_idc != 0. */
int h264r_output_geometry(int chroma_format_idc, const h264r_out_desc* desc, h264r_out_geom* geom);

/* Write num_frames output frames, frame i at dst + i * dst_frame_stride, from the sources frames[i]
 * names, by the geometry of `desc` for the context's chroma format.  One kernel launch for the whole
 * job; asynchronous on `stream` (a hipStream_t, NULL = the context's stream), with the stream rules of
 * h264r_decode_batch: after a launch of this context on another stream it first waits for that launch,
 * so the planes a decode has just written can be read without a host synchronisation.
 * Only the bytes of the frames are written: not the padding a pitch_align leaves behind a row, nor
 * the bytes between frame_bytes and dst_frame_stride.  dst may have any alignment; rows whose
 * destination allows it are written with 16-byte stores.
 * H264R_EINVAL as h264r_output_geometry, and for NULL frames / dst, num_frames < 0 or
 * dst_frame_stride < frame_bytes (num_frames == 0 is H264R_OK and does nothing).
 * The frame table is read on the device, so its mistakes are found there: a kind outside 0..3 or a
 * NULL plane pointer that the kind needs (y[0], y[1] of a field pair, and the same of u and v except on
 * a 4:0:0 context) is tested before anything is dereferenced; that frame is skipped -- none of its
 * bytes is written -- the context's error word is set and h264r_check returns H264R_EDEVICE.  The other
 * frames of the job are written. */
int h264r_output_frames(h264r_ctx* ctx, const h264r_out_desc* desc, const h264r_out_frame* frames /*device*/,
                        int num_frames, uint8_t* dst /*device*/, int64_t dst_frame_stride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * RGB frames: h264r_output_rgb writes, from the same frame table, the colour-converted frames a tensor
 * consumer reads -- packed or planar 8-bit R'G'B', or planar binary16 scaled and biased per channel.
 * The reference has no RGB output; what follows is the definition, complete: every byte is an exact
 * function of the source planes, in integers (and, for binary16, three IEEE operations).
 *
 * The source frame.  Exactly the planar frame h264r_output_frames writes for the same `src` with
 * layout H264R_OUT_PLANAR, pitch_align 0 and, on a 4:0:0 context, fake_chroma 1: luma Y[r][x] over the
 * cropped luma rectangle lw x lh, chroma Cb[j][i], Cr[j][i] over the cropped chroma rectangle cw x ch
 * (lw = SubWidthC * cw, lh = SubHeightC * ch); field pairs woven (frame row 2 r is the top field's row
 * r, row 2 r + 1 the bottom field's, in every plane), the missing rows of an unpaired field 128 in every
 * plane, 4:0:0 chroma 128 everywhere.  r, x, j, i count from the cropped origin.
 *
 * Chroma at luma sample (r, x), in units of 1 / 8: C8, for Cb (Cb8) and for Cr (Cr8) alike.
 *   H264R_UP_REPLICATE:  C8 = 8 * C[r / SubHeightC][x / SubWidthC]  (integer division).
 *   H264R_UP_BILINEAR:   C8 = sum over the taps below of wv * wh * C[j][i]; the weights sum to 8.
 *     This is chroma_sample_loc_type 0: chroma co-sited with the even luma columns, midway between two
 *     luma rows.  The cropped origin keeps that parity (x0 = SubWidthC * crop_left, y0 = SubHeightC * top).
 *       horizontal, SubWidthC 2:  x even: i = x / 2, wh = 2.
 *                                 x odd:  i0 = (x - 1) / 2, i1 = min(i0 + 1, cw - 1), wh = 1 and 1.
 *       horizontal, SubWidthC 1:  i = x, wh = 2.
 *       vertical, SubHeightC 2:   r even: j0 = r / 2, wv = 3;  j1 = max(j0 - 1, 0), wv = 1.
 *                                 r odd:  j0 = (r - 1) / 2, wv = 3;  j1 = min(j0 + 1, ch - 1), wv = 1.
 *       vertical, SubHeightC 1:   j = r, wv = 4.
 *     Indices clamp to the CROPPED chroma rectangle: no sample outside the crop has any influence.  The
 *     interpolation runs over the woven frame and treats it as progressive: the vertical taps of a
 *     field pair come from the two fields, those of an unpaired field mix the field with the 128 rows.
 *     (Where the fields differ in time, h264r_deinterlace of h264r_deinterlace.h makes progressive
 *     frames of them first; its result is named here as an H264R_OUT_FRAME source.)
 *   4:0:0 context:       C8 = 1024.
 *
 * The matrix.  All arithmetic 32-bit signed, >> an arithmetic shift, clip255(v) = min(max(v, 0), 255):
 *     R = clip255((8 * cy * (Y - yo) + crv * (Cr8 - 1024)                        + 65536) >> 17)
 *     G = clip255((8 * cy * (Y - yo) + cgu * (Cb8 - 1024) + cgv * (Cr8 - 1024) + 65536) >> 17)
 *     B = clip255((8 * cy * (Y - yo) + cbu * (Cb8 - 1024)                        + 65536) >> 17)
 * with (cy, crv, cgu, cgv, cbu) = floor(real * 2^14 + 1/2) of the reals
 *     255 / ys,  255 * 2 (1 - Kr) / cs,  -255 * 2 Kb (1 - Kb) / (Kg * cs),  -255 * 2 Kr (1 - Kr) / (Kg * cs),
 *     255 * 2 (1 - Kb) / cs,        Kg = 1 - Kr - Kb,
 * (ys, cs, yo) = (219, 224, 16) for full_range 0 and (255, 255, 0) for full_range 1 -- the six values
 * h264r_rgb_coefficients returns, in the order cy, crv, cgu, cgv, cbu, yo:
 *     BT.601  limited  19077  26149  -6419  -13320  33050  16      full  16384  22970  -5638  -11700  29032  0
 *     BT.709  limited  19077  29372  -3494   -8731  34610  16      full  16384  25802  -3069   -7670  30402  0
 *     BT.2020 limited  19077  27503  -3069  -10657  35091  16      full  16384  24160  -2696   -9361  30825  0
 * Against clip255(floor(x + 1/2)) of the same expression in real numbers the result differs by at most
 * 1, in fewer than 0.2 % of all (Y, Cb8, Cr8); every accumulator stays below 2^27.
 * H264R_CSC_GBR (4:4:4 contexts only): G = Y, B = Cb, R = Cr, copied; full_range and chroma_up are ignored.
 *
 * Output channels (c0, c1, c2) = (R, G, B), or (B, G, R) with bgr = 1.
 *
 * Formats; one output row holds
 *     H264R_RGB_PACKED_U8    3 lw bytes   c0 c1 c2 of pixel 0, of pixel 1, ...
 *     H264R_RGB_PACKED_U8X4  4 lw bytes   c0 c1 c2 alpha
 *     H264R_RGB_PLANAR_U8      lw bytes   in each of the planes c0, c1, c2
 *     H264R_RGB_PLANAR_F16   2 lw bytes   in each of the planes c0, c1, c2: channel c of a pixel is
 *                                         half_rn(float(v) * scale[c] + bias[c]) of its 8-bit value v:
 *                                         one binary32 multiplication, then one binary32 addition (each
 *                                         rounded to nearest even, NOT fused), then one conversion to
 *                                         binary16 (to nearest even), stored little-endian
 * and src.pitch_align applies to every row as in h264r_output_geometry: plane_pitch is the row's bytes
 * for pitch_align 0 or 1, else those rounded up to a multiple of it.  A packed frame is one plane of lh
 * rows (plane_off[0] = 0; [1], [2] and their pitches 0); a planar frame three planes of lh rows each,
 * plane_off[k] = k * plane_pitch[0] * lh; frame_bytes is the sum over the planes of pitch * lh.
 */
#define H264R_CSC_BT601   0   /* matrix_coefficients 5 / 6: Kr 0.299,  Kb 0.114  */
#define H264R_CSC_BT709   1   /* matrix_coefficients 1:     Kr 0.2126, Kb 0.0722 */
#define H264R_CSC_BT2020  2   /* matrix_coefficients 9:     Kr 0.2627, Kb 0.0593 */
#define H264R_CSC_GBR     3   /* matrix_coefficients 0: G = Y, B = Cb, R = Cr; 4:4:4 contexts only */

#define H264R_UP_REPLICATE 0  /* the chroma sample of the luma sample's chroma cell */
#define H264R_UP_BILINEAR  1  /* chroma_sample_loc_type 0 siting, above */

#define H264R_RGB_PACKED_U8    0   /* c0 c1 c2 per pixel, 3 bytes */
#define H264R_RGB_PACKED_U8X4  1   /* c0 c1 c2 alpha per pixel, 4 bytes */
#define H264R_RGB_PLANAR_U8    2   /* plane c0, plane c1, plane c2 */
#define H264R_RGB_PLANAR_F16   3   /* the same planes as IEEE binary16, normalised */

typedef struct h264r_rgb_desc {
    h264r_out_desc src;        /* size, crop, frame_mbs_only, pitch_align as for h264r_output_frames;
                                  src.layout and src.fake_chroma must be 0 */
    int32_t matrix, full_range, chroma_up, format;   /* H264R_CSC_*, 0 / 1, H264R_UP_*, H264R_RGB_* */
    int32_t bgr;               /* 0: (c0, c1, c2) = (R, G, B); 1: (B, G, R) */
    int32_t alpha;             /* 0..255, H264R_RGB_PACKED_U8X4 only */
    float   scale[3], bias[3]; /* H264R_RGB_PLANAR_F16 only, indexed by output channel c0..c2 */
} h264r_rgb_desc;

typedef struct h264r_rgb_geom {               /* filled by h264r_output_rgb_geometry */
    int32_t width, height;                    /* the cropped luma rectangle */
    int64_t plane_off[3], plane_pitch[3];     /* packed formats: [0] only */
    int64_t frame_bytes;
} h264r_rgb_geom;

/* Host only.  out = cy, crv, cgu, cgv, cbu, yo of the table above.  H264R_EINVAL: NULL out, a matrix
 * other than BT601 / BT709 / BT2020 (GBR has no coefficients), full_range not 0 / 1. */
int h264r_rgb_coefficients(int matrix, int full_range, int32_t out[6]);

/* Host only, no GPU needed.  H264R_EINVAL: what h264r_output_geometry refuses for desc->src, a
 * src.layout or src.fake_chroma other than 0, matrix / chroma_up / format out of range, full_range or
 * bgr not 0 / 1, alpha outside 0..255, a scale or bias that is not finite, a NULL argument.
 * H264R_EUNSUPPORTED: H264R_CSC_GBR with chroma_format_idc != 3. */
int h264r_output_rgb_geometry(int chroma_format_idc, const h264r_rgb_desc* desc, h264r_rgb_geom* geom);

/* h264r_output_frames for RGB: the same frame table and kinds, one launch per job, asynchronous on
 * `stream` under the same stream rules, num_frames == 0 is H264R_OK.  Frame i goes to dst + i *
 * dst_frame_stride (bytes).  Only the bytes of the frames are written (no pitch padding, nothing between
 * frame_bytes and dst_frame_stride), and no byte outside a source plane is read.  dst may have any
 * alignment (PLANAR_F16: a multiple of 2, and so dst_frame_stride); a run of 16 pixels whose destination
 * is 16-byte aligned is written with 16-byte stores.
 * H264R_EINVAL / H264R_EUNSUPPORTED as h264r_output_rgb_geometry for the context's chroma format, and
 * H264R_EINVAL for NULL ctx / frames / dst, num_frames < 0, dst_frame_stride < frame_bytes.
 * The frame table's mistakes are found on the device exactly as for h264r_output_frames: a kind outside
 * 0..3 or a NULL plane the kind needs is tested before anything is dereferenced, that frame is skipped,
 * the error word is set (h264r_check: H264R_EDEVICE) and the other frames are written. */
int h264r_output_rgb(h264r_ctx* ctx, const h264r_rgb_desc* desc, const h264r_out_frame* frames /*device*/,
                     int num_frames, void* dst /*device*/, int64_t dst_frame_stride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Scaled RGB frames: h264r_output_rgb_scaled writes a region of interest of the RGB frame above,
 * resampled to out_w x out_h, without the full-size frame ever existing.  The reference has no scaler;
 * what follows is the definition, complete and in integers, by composition with the RGB definition.
 *
 * The source.  The three channel planes c0, c1, c2 (8 bits, lh x lw) that h264r_output_rgb defines for
 * the same h264r_rgb_desc `rgb` and frame-table entry: crop and weave, the 128 rows of an unpaired field,
 * 4:0:0 chroma, chroma_up (its taps clamp to the CROP, never to the region of interest), matrix, range,
 * bgr, and H264R_CSC_GBR on 4:4:4.  Every source sample is converted and clipped to 8 bits first; the
 * resampling below sees nothing but those planes.
 *
 * The region of interest.  roi_x, roi_y, roi_w, roi_h in luma samples of the cropped rectangle:
 * columns roi_x .. roi_x + roi_w - 1, rows roi_y .. roi_y + roi_h - 1.  roi_w == roi_h == 0 stands for
 * roi_w = lw, roi_h = lh (roi_x and roi_y are then 0, or the region reaches outside).  Call it S_h rows
 * by S_w columns; sample [i] below counts from its origin.
 *
 * The result.  Each channel on its own is resampled to D_h = out_h rows by D_w = out_w columns of
 * 8-bit values v, and the four formats of h264r_output_rgb apply to v: PACKED_U8, PACKED_U8X4 and
 * PLANAR_U8 store v (alpha as there), PLANAR_F16 stores half_rn(float(v) * scale[c] + bias[c]) -- the
 * same three operations, not fused.  rgb.src.pitch_align pads the OUTPUT rows; plane_off, plane_pitch
 * and frame_bytes are those of h264r_output_rgb_geometry with (out_w, out_h) in place of (lw, lh).
 *
 * Per axis, for the output index d, the source size S and the output size D (all divisions are integer
 * divisions of non-negative numbers):
 *
 *   H264R_SCALE_BILINEAR, half-sample centres:
 *       p  = clamp((2 d + 1) * S - D, 0, 2 D * (S - 1)),   i0 = p / (2 D),   f = p - 2 D * i0,
 *       w1 = (256 * f + D) / (2 D)   (0..256),   w0 = 256 - w1,   i1 = min(i0 + 1, S - 1).
 *     With (i0, i1, w0, w1) of the row index as (r0, r1, wv0, wv1) and of the column index as
 *     (x0, x1, wh0, wh1):
 *       v = (wv0 * (wh0 * c[r0][x0] + wh1 * c[r0][x1]) + wv1 * (wh0 * c[r1][x0] + wh1 * c[r1][x1]) + 32768) >> 16.
 *     The sum stays below 2^24 and every intermediate fits 32 bits for S, D <= 16384.  D == S is the
 *     identity (f = 0 everywhere).
 *
 *   H264R_SCALE_AREA, exact box coverage: source sample i weighs
 *       o_i = max(0, min((d + 1) * S, (i + 1) * D) - max(d * S, i * D)),   sum over i of o_i = S.
 *     With ov of the row index and oh of the column index:
 *       A = sum over r, x of ov_r * oh_x * c[r][x],   T = S_h * S_w,   v = (2 A + T) / (2 T):
 *     round-half-up of the exact coverage-weighted mean.  The value does not depend on the unit: S and D
 *     of an axis may both be divided by their greatest common divisor.  With rw = S_w / gcd(S_w, D_w) and
 *     rh = S_h / gcd(S_h, D_h), rw * rh <= 2^23 keeps 2 A + T below 2^32 in that unit; a job beyond that is
 *     refused with H264R_EUNSUPPORTED.  D == S is the identity; D > S on an axis is allowed and means
 *     what the formula says (each output takes the one or two samples its interval touches).
 */
#define H264R_SCALE_BILINEAR 0
#define H264R_SCALE_AREA     1

#define H264R_SCALE_MAX_OUT  16384   /* out_w, out_h */

typedef struct h264r_scale_desc {
    h264r_rgb_desc rgb;                 /* everything of h264r_output_rgb; rgb.src.pitch_align pads the OUTPUT rows */
    int32_t roi_x, roi_y, roi_w, roi_h; /* luma samples inside the cropped rectangle; w == h == 0: all of it */
    int32_t out_w, out_h;               /* 1..16384 */
    int32_t filter;                     /* H264R_SCALE_* */
    int32_t pad;                        /* 0 */
} h264r_scale_desc;

/* Host only, no GPU needed.  geom->width, height = out_w, out_h; the layout as above.
 * H264R_EINVAL: whatever h264r_output_rgb_geometry refuses for desc->rgb; a negative roi_x / roi_y /
 * roi_w / roi_h, exactly one of roi_w and roi_h zero, a region that reaches outside the cropped
 * rectangle; out_w or out_h outside 1..16384; a filter other than the two above; a non-zero pad; a NULL
 * argument.  H264R_EUNSUPPORTED (when nothing above applies): H264R_CSC_GBR with chroma_format_idc != 3,
 * H264R_SCALE_AREA with rw * rh > 2^23. */
int h264r_output_rgb_scaled_geometry(int chroma_format_idc, const h264r_scale_desc* desc, h264r_rgb_geom* geom);

/* h264r_output_rgb, scaled: the same frame table and the same four kinds, one launch per job,
 * asynchronous on `stream` under the same stream rules, num_frames == 0 is H264R_OK.  Frame i goes to
 * dst + i * dst_frame_stride.  Only the bytes of the frames are written, no byte outside a source plane
 * is read -- and none outside the crop: the region's samples and the chroma taps they name are all.
 * dst may have any alignment (PLANAR_F16: a multiple of 2, and so dst_frame_stride).
 * H264R_EINVAL / H264R_EUNSUPPORTED as h264r_output_rgb_scaled_geometry for the context's chroma format,
 * and H264R_EINVAL for NULL ctx / frames / dst, num_frames < 0, dst_frame_stride < frame_bytes.
 * A bad kind or a NULL plane is refused on the device as for h264r_output_rgb: that frame is skipped,
 * the error word is set (h264r_check: H264R_EDEVICE) and the other frames are written. */
int h264r_output_rgb_scaled(h264r_ctx* ctx, const h264r_scale_desc* desc, const h264r_out_frame* frames /*device*/,
                            int num_frames, void* dst /*device*/, int64_t dst_frame_stride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Boxes: h264r_output_rgb_boxes takes the region, the output size and the placement from a DEVICE table,
 * one h264r_out_box per box, and writes every box of the table in one job: a detector's boxes each to a
 * classifier's input size, a letterbox (the whole frame, aspect kept, centred in a canvas whose border the
 * caller has filled), several frames into one mosaic.  The meaning is by composition with the two
 * definitions above; nothing is resampled differently.
 *
 * An image.  The job writes into num_images destination images of image_w x image_h pixels, image k at
 * dst + k * dst_image_stride.  The layout of one image is that of h264r_output_rgb_geometry with
 * (image_w, image_h) in place of (lw, lh) -- the same four formats, rgb.src.pitch_align pads the IMAGE
 * rows -- and it is what h264r_output_rgb_boxes_geometry returns (width, height = image_w, image_h).
 *
 * A box b names out_h rows of out_w pixels, each three 8-bit values v (one per channel c0, c1, c2):
 * exactly the values h264r_output_rgb_scaled defines for the same `rgb`, the frame-table entry b.frame,
 * the region (roi_x, roi_y, roi_w, roi_h) -- w == h == 0 stands for the whole cropped rectangle -- the
 * output size (out_w, out_h) and `filter`.
 *
 * Placement.  Pixel (r, x) of the box, r = 0 .. out_h - 1, x = 0 .. out_w - 1, is pixel
 * (dst_y + r, dst_x + x) of image b.image, written in the image's format: PACKED_U8, PACKED_U8X4 (alpha as
 * in h264r_output_rgb) and PLANAR_U8 store v, PLANAR_F16 stores half_rn(float(v) * scale[c] + bias[c]) by
 * the same three operations, not fused.
 *
 * What is written.  Only the bytes of the boxes' pixels.  Every other byte of dst keeps what it held: the
 * pixels of an image no box covers (a letterbox border is the caller's prefill), the padding a pitch_align
 * leaves behind a row, the bytes between frame_bytes and dst_image_stride, whole images that no box names.
 * Where two boxes overlap in one image, each channel of each pixel they share holds the value of one of
 * them; which one is not defined.  Frames may be named by any number of boxes, in any order, or by none.
 *
 * Reads.  As for h264r_output_rgb_scaled: no byte outside a source plane and none outside the crop.
 *
 * The refusal of a box: ONE rule, the same function on the host (h264r_out_box_status) and on the device,
 * every field tested before it indexes anything.  In this order,
 *   H264R_EINVAL       frame outside 0 .. num_frames - 1, image outside 0 .. num_images - 1;
 *                      a region h264r_output_rgb_scaled_geometry refuses: a negative roi_x / roi_y / roi_w /
 *                      roi_h, exactly one of roi_w and roi_h zero, a region that reaches outside the cropped
 *                      rectangle;
 *                      out_w outside 1 .. max_out_w, out_h outside 1 .. max_out_h;
 *                      a placement that reaches outside the image: dst_x or dst_y negative,
 *                      dst_x + out_w > image_w, dst_y + out_h > image_h;
 *                      a non-zero pad;
 *   H264R_EUNSUPPORTED (when nothing above applies) H264R_SCALE_AREA with rw * rh > 2^23, rw and rh as in
 *                      the scaled definition.
 * On the device a refused box is skipped -- none of its bytes is written -- the context's error word is
 * set (h264r_check: H264R_EDEVICE) and the other boxes are written.  A box whose frame-table entry has a
 * kind outside 0..3 or a NULL plane the kind needs is skipped in the same way.
 */
typedef struct h264r_out_box {          /* 48 bytes; the box table is a DEVICE array of these */
    int32_t frame;                      /* entry of the frame table */
    int32_t image;                      /* destination image, 0 .. num_images - 1 */
    int32_t roi_x, roi_y, roi_w, roi_h; /* as h264r_scale_desc: luma samples of the cropped rectangle; w == h == 0: all */
    int32_t dst_x, dst_y;               /* where the box's pixel (0, 0) goes in the image, in pixels */
    int32_t out_w, out_h;               /* 1 .. desc.max_out_w / max_out_h */
    int32_t pad[2];                     /* 0 */
} h264r_out_box;

typedef struct h264r_boxes_desc {
    h264r_rgb_desc rgb;                 /* everything of h264r_output_rgb; rgb.src.pitch_align pads the IMAGE rows */
    int32_t image_w, image_h;           /* 1 .. H264R_SCALE_MAX_OUT */
    int32_t max_out_w, max_out_h;       /* 1 .. image_w / image_h: bound of every box's out_w / out_h (sizes the grid) */
    int32_t filter, pad;                /* H264R_SCALE_*, 0 */
} h264r_boxes_desc;

/* Host only, no GPU needed.  geom->width, height = image_w, image_h; the layout of one image as above.
 * H264R_EINVAL: whatever h264r_output_rgb_geometry refuses for desc->rgb; image_w or image_h outside
 * 1..16384; max_out_w outside 1..image_w, max_out_h outside 1..image_h; a filter other than the two; a
 * non-zero pad; a NULL argument.  H264R_EUNSUPPORTED (when nothing above applies): H264R_CSC_GBR with
 * chroma_format_idc != 3. */
int h264r_output_rgb_boxes_geometry(int chroma_format_idc, const h264r_boxes_desc* desc, h264r_rgb_geom* geom);

/* Host only, no GPU needed: the rule above for one box (host memory) of a job of num_frames frame-table
 * entries and num_images images.  H264R_EINVAL also for a NULL box, negative counts and a descriptor
 * h264r_output_rgb_boxes_geometry refuses with H264R_EINVAL; every H264R_EINVAL comes before any
 * H264R_EUNSUPPORTED (the descriptor's, then the box's). */
int h264r_out_box_status(int chroma_format_idc, const h264r_boxes_desc* desc, const h264r_out_box* box, int num_frames,
                         int num_images);

/* Write the num_boxes boxes of the device table `boxes` into the num_images images at dst.  Two kernel
 * launches per job whatever the number of boxes (a plan per box, then the pixels of all of them);
 * asynchronous on `stream` under the stream rules of the other three entry points; num_boxes == 0 is
 * H264R_OK and does nothing.  dst may have any alignment (PLANAR_F16: a multiple of 2, and so
 * dst_image_stride); a run of 16 pixels of a box whose destination is 16-byte aligned is written with
 * 16-byte stores.  The context keeps the plans in a buffer of its own that grows only when num_boxes
 * exceeds what it has held before.
 * H264R_EINVAL / H264R_EUNSUPPORTED as h264r_output_rgb_boxes_geometry for the context's chroma format,
 * and H264R_EINVAL for NULL ctx / frames / boxes / dst, num_frames < 0, num_boxes < 0, num_images < 0,
 * dst_image_stride < frame_bytes.  Both tables are read on the device, so their mistakes are found there,
 * as described above. */
int h264r_output_rgb_boxes(h264r_ctx* ctx, const h264r_boxes_desc* desc, const h264r_out_frame* frames /*device*/, int num_frames,
                           const h264r_out_box* boxes /*device*/, int num_boxes,
                           void* dst /*device*/, int64_t dst_image_stride, int num_images, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Resampled RGB frames: h264r_output_rgb_resampled writes a region of the RGB frame resampled to
 * out_w x out_h by the 8-bit resampler of Pillow (Image.resize with BILINEAR, BICUBIC or LANCZOS, which
 * is what most vision models were trained behind), byte for byte, without the full-size frame ever
 * existing.  The definition is Pillow's Resample.c restated; it is complete here.
 *
 * The source.  The three 8-bit channel planes c0, c1, c2 (lh x lw) that h264r_output_rgb defines for the
 * same h264r_rgb_desc `rgb` and frame-table entry, as for h264r_output_rgb_scaled: the same four kinds,
 * crop and weave, the 128 rows of an unpaired field, 4:0:0 chroma, chroma_up (its taps clamp to the CROP),
 * matrix, range, bgr, H264R_CSC_GBR on 4:4:4.  The resampling sees nothing but those planes.
 *
 * The region.  roi_x, roi_y, roi_w, roi_h as in h264r_scale_desc (w == h == 0: the whole cropped
 * rectangle), with the meaning of Pillow's box=:
 *     resize((out_w, out_h), filter, box=(roi_x, roi_y, roi_x + roi_w, roi_y + roi_h))
 * applied to the cropped frame.  The region sets where the sample centres fall; a window that reaches past
 * the region reads the REAL samples of the cropped rectangle there, and clamps only at the crop's edges.
 * This is not crop(box).resize(...), whose windows clamp at the region's edges.
 *
 * The filters f, each with its support; x is binary64 and every operation is written out:
 *   H264R_RESAMPLE_TRIANGLE (Pillow BILINEAR), support 1:
 *       x = |x|;  f = 1.0 - x for x < 1.0, else 0.0.
 *   H264R_RESAMPLE_BICUBIC, support 2, a = -0.5 (torch and OpenCV take a = -0.75: their output is not this):
 *       x = |x|;  f = ((a + 2.0) * x - (a + 3.0)) * x * x + 1 for x < 1.0,
 *                 f = (((x - 5) * x + 8) * x - 4) * a for x < 2.0, else 0.0.
 *   H264R_RESAMPLE_LANCZOS, support 3:
 *       f = sinc(x) * sinc(x / 3) for -3.0 <= x < 3.0, else 0.0;
 *       sinc(0.0) = 1.0, else with y = x * 3.14159265358979323846: sinc = sin(y) / y, the C library's sin.
 *
 * Per axis, with inSize the crop's size along the axis (lw or lh), in0 the region's origin, in1 = in0 +
 * the region's size, and outSize; every operation binary64, in this order, none fused:
 *     scale = (in1 - in0) / outSize        filterscale = max(scale, 1.0)
 *     support = filter_support * filterscale        ss = 1.0 / filterscale
 *     ksize = 2 * ceil(support) + 1
 * and for the output index d:
 *     center = in0 + (d + 0.5) * scale
 *     xmin = max(0, (int)(center - support + 0.5))        xmax = min(inSize, (int)(center + support + 0.5))
 *     k[j] = f((j + xmin - center + 0.5) * ss)   for j = 0 .. xmax - xmin - 1
 *     ww = sum of k[j] in index order;   k[j] = k[j] / ww when ww != 0
 *     kk[j] = (int)(k[j] * 2^22 + 0.5) for k[j] >= 0, (int)(k[j] * 2^22 - 0.5) otherwise
 * where (int) truncates toward zero.  count = xmax - xmin lies in 1 .. ksize.  h264r_resample_axis returns
 * exactly this table.
 *
 * The passes.  With (xminx, kkx) of the columns and (yminy, kky) of the rows, per channel c, >> the
 * arithmetic shift and clip8(v) = min(max(v, 0), 255):
 *     t[r][d] = clip8((2^21 + sum over j of kkx[d][j] * c[r][xminx[d] + j]) >> 22)      horizontal, first
 *     v[e][d] = clip8((2^21 + sum over j of kky[e][j] * t[yminy[e] + j][d]) >> 22)      vertical, over t
 * The clip between the passes is part of the definition: the negative lobes of BICUBIC and LANCZOS
 * overshoot, and that is where the overshoot is cut.  At scale 1 on an axis its pass is the identity.
 * Every accumulator fits 32 bits: 255 * (sum over j of |kk[j]|) + 2^21 < 2^31 for every table (the
 * normalised taps sum to 2^22; the sum of their magnitudes is largest under LANCZOS, about 1.55 * 2^22 when
 * upscaling, where 2.005 * 2^22 would be needed to overflow), and every tap lies inside 24 bits.
 *
 * The result.  The four formats of h264r_output_rgb apply to v, with bgr, alpha and rgb.src.pitch_align
 * (which pads the OUTPUT rows) exactly as for h264r_output_rgb_scaled: PLANAR_F16 stores
 * half_rn(float(v) * scale[c] + bias[c]), the same three operations, not fused.  The layout is that of
 * h264r_output_rgb_geometry with (out_w, out_h) in place of (lw, lh).
 *
 * Bounds.  out_w and out_h lie in 1 .. 16384.  A job whose ksize on either axis exceeds
 * H264R_RESAMPLE_MAX_TAPS is refused with H264R_EUNSUPPORTED: the constant is what the kernel's LDS holds,
 * and it admits every job whose scale is at most 16 on both axes under all three filters (LANCZOS at scale
 * 16: 2 * 48 + 1), TRIANGLE up to scale 48 and BICUBIC up to scale 24.
 */
#define H264R_RESAMPLE_TRIANGLE 0   /* Pillow BILINEAR (antialiased) */
#define H264R_RESAMPLE_BICUBIC  1   /* Pillow BICUBIC */
#define H264R_RESAMPLE_LANCZOS  2   /* Pillow LANCZOS */

#define H264R_RESAMPLE_MAX_TAPS 97  /* ksize of either axis */
#define H264R_RESAMPLE_TILE_W   16  /* output pixels a workgroup of the kernel owns: for tests around its edges */
#define H264R_RESAMPLE_TILE_H   16

typedef struct h264r_resample_desc {
    h264r_rgb_desc rgb;                 /* everything of h264r_output_rgb; rgb.src.pitch_align pads the OUTPUT rows */
    int32_t roi_x, roi_y, roi_w, roi_h; /* luma samples inside the cropped rectangle; w == h == 0: all of it */
    int32_t out_w, out_h;               /* 1..16384 */
    int32_t filter;                     /* H264R_RESAMPLE_* */
    int32_t pad;                        /* 0 */
} h264r_resample_desc;

/* Host only, no GPU needed.  geom->width, height = out_w, out_h; the layout as above.
 * H264R_EINVAL: what h264r_output_rgb_scaled_geometry refuses with it, with the three filters above in
 * place of its two.  H264R_EUNSUPPORTED (when nothing above applies): H264R_CSC_GBR with chroma_format_idc
 * != 3; ksize of either axis above H264R_RESAMPLE_MAX_TAPS. */
int h264r_output_rgb_resampled_geometry(int chroma_format_idc, const h264r_resample_desc* desc, h264r_rgb_geom* geom);

/* Host only, no GPU needed: the table of one axis, as defined above -- the function a plan builds its
 * own tables with.  xmin and count hold out_size entries, kk out_size * *ksize (row d: the taps of output
 * d, zero from count[d] on).  With xmin, count and kk all NULL only *ksize is written; the caller sizes
 * its arrays by it.  No bound on ksize applies here.
 * H264R_EINVAL: a filter other than the three, in_size < 1, in0 < 0, in1 <= in0, in1 > in_size, out_size
 * outside 1..16384, a NULL ksize, some but not all of the three arrays NULL. */
int h264r_resample_axis(int filter, int in_size, int in0, int in1, int out_size, int32_t* xmin, int32_t* count,
                        int32_t* kk, int32_t* ksize);

/* A plan: the two tables of one descriptor in device memory the plan owns (tens of kilobytes: more than
 * kernel arguments carry), with the RGB mode, the layout and the tiling resolved.  Creation is synchronous:
 * it builds both axes on the host and uploads them with blocking copies.  A plan belongs to the context it
 * was made on -- its device and its chroma format -- and serves any number of jobs, on any streams, at
 * once.  The caller destroys it only after the launches that use it are done (h264r_check, or a
 * synchronisation of their streams); destroying NULL does nothing.
 * H264R_EINVAL / H264R_EUNSUPPORTED as h264r_output_rgb_resampled_geometry for the context's chroma
 * format, H264R_EINVAL for a NULL ctx / desc / plan, H264R_ENOMEM. */
typedef struct h264r_resample_plan h264r_resample_plan;
int h264r_resample_plan_create(h264r_ctx* ctx, const h264r_resample_desc* desc, h264r_resample_plan** plan);
void h264r_resample_plan_destroy(h264r_resample_plan* plan);

/* h264r_output_rgb_scaled, resampled by a plan: the same frame table and the same four kinds, ONE launch
 * per job, asynchronous on `stream` under the same stream rules, num_frames == 0 is H264R_OK.  Frame i
 * goes to dst + i * dst_frame_stride.  No host arithmetic beyond the argument checks, no allocation, no
 * copy.  Both passes run inside a workgroup's LDS: no converted and no half-resampled frame exists in
 * device memory.  Only the bytes of the frames are written; no byte outside a source plane is read, and
 * none outside the crop.  dst may have any alignment (PLANAR_F16: a multiple of 2, and so dst_frame_stride).
 * H264R_EINVAL for NULL ctx / plan / frames / dst, a plan of another context, num_frames < 0,
 * dst_frame_stride < frame_bytes.  A bad kind or a NULL plane is refused on the device as for
 * h264r_output_rgb: that frame is skipped, the error word is set (h264r_check: H264R_EDEVICE) and the other
 * frames are written. */
int h264r_output_rgb_resampled(h264r_ctx* ctx, const h264r_resample_plan* plan, const h264r_out_frame* frames /*device*/,
                               int num_frames, void* dst /*device*/, int64_t dst_frame_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* H264R_OUTPUT_H_ */
