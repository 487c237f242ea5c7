// output_job.h -- what h264r_output_frames (h264r_host.hip) hands k_output (k_output.hip): the planes
// of one output frame, resolved from an h264r_out_desc by the geometry of include/h264r_output.h.
#pragma once

#include <stdint.h>

namespace h264r {

enum OutMode : int32_t {
    OUT_COPY_Y = 0, OUT_COPY_U = 1, OUT_COPY_V = 2,   // rows of one source plane
    OUT_INTERLEAVE = 3,                               // rows of Cb Cr Cb Cr ... from the u and v planes
    OUT_FILL = 4,                                     // bytes of 128 (4:0:0 fake chroma): no source
};

struct OutPlane {
    int64_t off, pitch;        // inside the output frame, bytes
    int32_t w, h;              // bytes per output row, output rows
    int32_t x0, y0;            // crop origin inside the (woven) source plane, samples / rows
    int32_t src_pitch;         // coded width of the source plane
    int32_t mode;              // OutMode
};

struct OutJob {
    OutPlane pl[3];
    int32_t nplanes;
    int32_t need_chroma;       // 0 on a 4:0:0 context: u / v are neither tested nor read
    int32_t num_frames;
    int32_t pad;
    int64_t frame_stride;
};

constexpr int OUT_THREADS = 256;   // k_output: threads per workgroup
constexpr int OUT_ITEMS = 4;       // 16-byte chunks per thread

// 16-byte chunks a row of w bytes is cut into at most: its destination may start anywhere inside one
inline __host__ __device__ int out_chunks_per_row(int w) { return (w + 15) / 16 + 1; }

}  // namespace h264r
