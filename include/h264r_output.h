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

#ifdef __cplusplus
}
#endif
#endif /* H264R_OUTPUT_H_ */
