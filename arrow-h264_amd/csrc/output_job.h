// output_job.h -- what h264r_output_frames (h264r_host.hip) hands k_output (k_output.hip): the planes
// of one output frame, resolved from an h264r_out_desc by the geometry of include/h264r_output.h;
// what h264r_output_rgb hands k_output_rgb (the same file); what h264r_output_rgb_scaled hands
// k_output_rgb_scaled (k_output_scale.hip); what h264r_output_rgb_boxes hands the k_output_boxes
// kernels (k_output_boxes.hip); and what h264r_output_rgb_resampled hands the k_output_rgb_resampled
// kernels (k_output_resample.hip).
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

// What h264r_output_rgb hands k_output_rgb: the geometry of an h264r_rgb_desc resolved for the
// context's chroma format, and the coefficient row of its matrix (h264r_rgb_coefficients).
// what a unit of k_output_rgb loads and how it forms C8
enum RgbMode : int32_t {
    RGB_MONO = 0,     // 4:0:0: u / v are neither tested nor read, C8 = 1024
    RGB_FULL = 1,     // SubWidthC 1 (4:4:4): 16 samples of one chroma row, C8 = 8 C under either chroma_up
    RGB_GBR = 2,      // 4:4:4, H264R_CSC_GBR: the three planes copied
    RGB_REP = 3,      // SubWidthC 2, replicate: 8 samples of one chroma row
    RGB_BIL1 = 4,     // 4:2:2 bilinear: 8 + 1 samples of one chroma row
    RGB_BIL2 = 5,     // 4:2:0 bilinear: 8 + 1 samples of two chroma rows, weights 3 and 1
};

struct RgbJob {
    int64_t plane_off[3], pitch;   // inside the output frame, bytes (packed formats: plane_off[0] alone)
    int64_t frame_stride;
    int32_t lw, lh, x0, y0;        // the cropped luma rectangle inside the (woven) luma plane
    int32_t cw, ch, cx0, cy0;      // the cropped chroma rectangle (all zero on 4:0:0)
    int32_t lpitch, cpitch;        // coded widths of the source planes
    int32_t sub_h;                 // SubHeightC: 1 or 2
    int32_t mode;                  // RgbMode
    int32_t format, bgr, alpha;
    int32_t cy, crv, cgu, cgv, cbu, yo;
    float scale[3], bias[3];
    int32_t num_frames;
};

constexpr int RGB_THREADS = 256;   // k_output_rgb: threads per workgroup
constexpr int RGB_ITEMS = 2;       // units per thread
constexpr int RGB_UNIT = 16;       // pixels per unit: horizontally consecutive, of one output row

inline __host__ __device__ int rgb_units_per_row(int lw) { return (lw + RGB_UNIT - 1) / RGB_UNIT; }

// What h264r_output_rgb_scaled hands k_output_rgb_scaled (k_output_scale.hip): the RgbJob of its
// h264r_rgb_desc, whose source side (lw .. mode, the coefficients) is that of the full-size RGB frame
// and whose output side (plane_off, pitch, frame_stride) is the SCALED frame's; the region of interest
// and, per axis, the sizes the header's formulas take.
struct ScaleAxis {
    int32_t S, D;              // source (region of interest) and output size
    int32_t s, d;              // the same divided by their greatest common divisor (H264R_SCALE_AREA's unit)
    float inv_d, inv_2D;       // 1 / d and 1 / (2 D): first guesses of scale_div's quotients
};

struct ScaleJob {
    RgbJob rgb;
    ScaleAxis ax, ay;          // columns, rows
    int32_t roi_x, roi_y;      // the region's origin inside the cropped rectangle
    int32_t filter;            // H264R_SCALE_*
    int32_t taps;              // columns of a 16-pixel source unit any output can weigh: 1..16
    uint32_t T;                // AREA: ax.s * ay.s <= 2^23
    float inv_2T;
};

constexpr int SCALE_THREADS = 256; // k_output_rgb_scaled: threads per workgroup = output pixels = 16 units of RGB_UNIT
constexpr int SCALE_UNITS = SCALE_THREADS / RGB_UNIT;
constexpr int64_t SCALE_AREA_MAX_T = 1 << 23;

// What h264r_output_rgb_boxes hands the k_output_boxes kernels (k_output_boxes.hip): the RgbJob of its
// h264r_rgb_desc, whose source side is that of the full-size RGB frame and whose output side (plane_off,
// pitch, frame_stride) is the IMAGE's, and what bounds every box.  What k_output_rgb_scaled takes as
// kernel arguments -- the axes, the region, taps, T -- is per box here: k_output_boxes_plan writes one
// BoxPlan per box, and the workgroups of k_output_boxes_<mode>_<filter> read theirs.
struct BoxesJob {
    RgbJob rgb;                // rgb.num_frames: entries of the frame table
    int32_t image_w, image_h;
    int32_t max_out_w, max_out_h;
    int32_t filter;            // H264R_SCALE_*
    int32_t num_boxes, num_images;
};

struct BoxPlan {
    ScaleAxis ax, ay;          // columns, rows: as ScaleJob's
    int32_t roi_x, roi_y;
    int32_t taps;
    uint32_t T;
    float inv_2T;
    int32_t units, upr;        // units of RGB_UNIT output pixels: out_h * upr in all, 0: a refused box, nothing to do
    int32_t kind;              // of the frame-table entry, tested
    int32_t frame, image;
    int32_t dst_x, dst_y;
};
static_assert(sizeof(BoxPlan) == 96, "BoxPlan layout");

constexpr int BOXES_PLAN_THREADS = 256;   // k_output_boxes_plan: threads per workgroup = boxes

// What h264r_output_rgb_resampled hands the k_output_rgb_resampled kernels (k_output_resample.hip): the
// RgbJob of its h264r_rgb_desc (source side the full-size RGB frame's, output side the RESAMPLED frame's),
// the two axis tables of a plan in device memory, and how a workgroup's LDS is cut up for this job.
constexpr int RS_THREADS = 256;           // threads per workgroup
constexpr int RS_TW = 16, RS_TH = 16;     // output pixels a workgroup owns: H264R_RESAMPLE_TILE_W / _H
constexpr int RS_MAX_TAPS = 97;           // H264R_RESAMPLE_MAX_TAPS
constexpr int RS_LDS_MAX = 65536;         // bytes of LDS a workgroup takes at most
constexpr int RS_OUT_WORDS = 20;          // words of the job's output side that wait in LDS for the threads that write
static_assert(RS_TW == RGB_UNIT, "a tile row leaves as one unit of rgb_write");

struct ResampleAxis {
    const int32_t* xmin;       // [D]
    const int32_t* count;      // [D]
    const int32_t* kk;         // [D][ksize]
    int32_t D, ksize;
};

struct ResampleJob {
    RgbJob rgb;
    ResampleAxis ax, ay;       // columns, rows; xmin counts from the CROPPED rectangle's origin
    int32_t tiles_x, tiles_y;
    int32_t strip_cols;        // source columns of the widest tile, from an even column, in whole units: a multiple of 16
    int32_t span_rows;         // source rows of the highest tile
    int32_t step_rows;         // source rows converted and passed horizontally at a time
    int32_t pad;
};

// LDS of one workgroup, in bytes: kkx [RS_TW][ksx] and kky [RS_TH][ksy] words, xmin and count of the tile's
// columns and rows, t [span_rows][3][RS_TW] bytes, the strip [step_rows][strip_cols] words (one pixel a
// word), the tile's 8-bit results [3][RS_TH][RS_TW], and RS_OUT_WORDS words of the job's output side.
inline __host__ __device__ int rs_t_bytes(int span_rows) { return (span_rows * 3 * RS_TW + 15) & ~15; }
inline __host__ __device__ int rs_lds_bytes(int ksx, int ksy, int strip_cols, int span_rows, int step_rows)
{
    return 4 * (RS_TW * ksx + RS_TH * ksy) + 4 * 2 * (RS_TW + RS_TH) + rs_t_bytes(span_rows) + 4 * step_rows * strip_cols +
           3 * RS_TH * RS_TW + 4 * RS_OUT_WORDS;
}
// The widest job H264R_RESAMPLE_MAX_TAPS admits: ceil(support) <= 48, so support <= 48 and scale <= 48
// (TRIANGLE).  A tile's windows span (T - 1) * scale + 2 * support + 1 samples at most (xmin is at least
// center - support + 0.5 - 1, xmax at most center + support + 0.5): 15 * 48 + 97 = 817; the strip starts
// on an even column (+ 1) and ends on a whole unit (+ 15): 848 columns.
constexpr int RS_SPAN_MAX = (RS_TH - 1) * 48 + 97;
constexpr int RS_STRIP_MAX = ((RS_TW - 1) * 48 + 97 + 1 + 15) / 16 * 16;
static_assert(4 * (RS_TW + RS_TH) * RS_MAX_TAPS + 4 * 2 * (RS_TW + RS_TH) + ((RS_SPAN_MAX * 3 * RS_TW + 15) & ~15) + 4 * RS_STRIP_MAX +
              3 * RS_TH * RS_TW + 4 * RS_OUT_WORDS <= RS_LDS_MAX, "the widest job fits with one row a step");

// What h264r_deinterlace hands k_deinterlace (k_deinterlace.hip): per plane, the cropped rectangle inside
// the coded plane (the same in every source and in the output frame, whose planes are coded-size too) and
// how it is cut into tiles; the sizes of the two device tables.
constexpr int DEINT_THREADS = 64;         // threads per workgroup: one wave
constexpr int DEINT_UNIT = 16;            // columns a lane owns: one 16-byte store per output row
constexpr int DEINT_TW = 32;              // H264R_DEINT_TILE_W: DEINT_TW / DEINT_UNIT lanes side by side
constexpr int DEINT_TH = 64;              // H264R_DEINT_TILE_H: DEINT_TH / 2 field rows, one per lane
constexpr int DEINT_GROUP = 32;           // the grid's x is a multiple of it: deint_tile()'s permutation
static_assert(DEINT_TW / DEINT_UNIT * (DEINT_TH / 2) == DEINT_THREADS, "a lane per unit and field row of a tile");

struct DeintPlane {
    int64_t off;               // inside the output frame, bytes
    int32_t pitch;             // coded width: of the sources' planes and of the output's
    int32_t x0, y0, w, h;      // the cropped rectangle; y0 and h are even
    int32_t tiles_x, tiles;    // tiles in a row of tiles, and in all
    int32_t which;             // 0 y, 1 u, 2 v of an h264r_out_frame
};

struct DeintJob {
    DeintPlane pl[3];
    int32_t nplanes;
    int32_t need_chroma;       // 0 on a 4:0:0 context: u / v are neither tested nor read
    int32_t num_frames, num_jobs;
    int64_t frame_stride;
};

// The tile block b of a launch takes.  Blocks b and b + 8 are observed to share an XCD and its L2; a tile
// is a quarter of a 128-byte line wide, so the four tiles of a line go to blocks 8 apart.  A permutation
// of every aligned group of DEINT_GROUP blocks, and only a matter of speed.
inline __host__ __device__ int deint_tile(int b) { return (b & ~31) | ((b & 7) << 2) | ((b >> 3) & 3); }

}  // namespace h264r
