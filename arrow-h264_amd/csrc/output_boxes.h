// output_boxes.h -- the refusal of one box of h264r_output_rgb_boxes (include/h264r_output.h, "The refusal
// of a box"): ONE function, which h264r_out_box_status runs on the host (host_output.hip) and
// k_output_boxes_plan on the device (k_output_boxes.hip), so that the two cannot disagree.  It reads the
// box and the job's bounds and nothing else: every field is tested before anything is indexed by it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "h264r.h"
#include "h264r_output.h"
#include "output_job.h"

namespace h264r {

// Euclid, of positive numbers
inline __host__ __device__ int32_t box_gcd(int32_t a, int32_t b)
{
    while (b) { const int32_t t = a % b; a = b; b = t; }
    return a;
}

// H264R_OK, or why box b is no box of job J: H264R_EINVAL ahead of H264R_EUNSUPPORTED.  J.rgb.lw / lh are
// the cropped rectangle; every sum is taken in 64 bits, so no field can wrap past a bound.
inline __host__ __device__ int out_box_status(const h264r_out_box& b, const BoxesJob& J)
{
    if (b.frame < 0 || b.frame >= J.rgb.num_frames || b.image < 0 || b.image >= J.num_images) return H264R_EINVAL;
    if (b.roi_x < 0 || b.roi_y < 0 || b.roi_w < 0 || b.roi_h < 0 || (b.roi_w == 0) != (b.roi_h == 0)) return H264R_EINVAL;
    const int64_t sw = b.roi_w ? b.roi_w : J.rgb.lw, sh = b.roi_h ? b.roi_h : J.rgb.lh;
    if (b.roi_x + sw > J.rgb.lw || b.roi_y + sh > J.rgb.lh) return H264R_EINVAL;
    if (b.out_w < 1 || b.out_w > J.max_out_w || b.out_h < 1 || b.out_h > J.max_out_h) return H264R_EINVAL;
    if (b.dst_x < 0 || b.dst_y < 0 || (int64_t)b.dst_x + b.out_w > J.image_w || (int64_t)b.dst_y + b.out_h > J.image_h)
        return H264R_EINVAL;
    if (b.pad[0] != 0 || b.pad[1] != 0) return H264R_EINVAL;
    if (J.filter == H264R_SCALE_AREA) {
        const int64_t rw = sw / box_gcd((int32_t)sw, b.out_w), rh = sh / box_gcd((int32_t)sh, b.out_h);
        if (rw * rh > SCALE_AREA_MAX_T) return H264R_EUNSUPPORTED;
    }
    return H264R_OK;
}

}  // namespace h264r
