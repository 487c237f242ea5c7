// kernels.h -- the contract between the host (h264r_host.hip) and the kernels: the prototype of
// every kernel the host launches, the constants both sides size things with, the deblocking
// record the launches pass along, and the values of the device error word.  Every k_*.hip and
// the host include it, so a definition that drifts from its prototype does not compile
// ("conflicting types"): extern "C" names are not mangled, and a mismatch would otherwise link
// and launch with a wrong argument block.  The definitions carry the __launch_bounds__.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "h264r.h"
#include "h264r_deinterlace.h"
#include "h264r_output.h"
#include "launch_cfg.h"
#include "output_job.h"
#include "sync_words.h"

#ifndef H264R_WALK_ROWS
#define H264R_WALK_ROWS 8                   // k_intra_pic: MB rows per band = waves per workgroup
#endif

namespace h264r {

// ------------------------------------------------------------------ shared sizes
// the level schedule (k_picture.hip)
constexpr int LEVEL_MAX_MBS = 65536;        // k_level keeps a picture's intra bitmap in LDS
constexpr int LEVEL_LDS = 40960;            // k_level's LDS level bytes: (W + 2) x (rows + 1)
constexpr int LEVEL_LISTS = 64;             // levels 1 .. this many get per-level MB lists
// Two lists per level: id 2 L = its pairable MBs (intra_pairable: I_4x4, not lossless), id
// 2 L + 1 the others, laid out in id order; count / base / cursor arrays of LEVEL_IDS ints.
constexpr int LEVEL_IDS = 2 * (LEVEL_LISTS + 1);

// the deblocking hand-off records, bytes per MB (k_deblock) / per MB column (k_deblock2)
constexpr size_t HANDOFF_BYTES = 256;       // one tagged record: 32 x {dword, epoch}
constexpr size_t HANDOFF2_BYTES = 384;      // 2 row slots x 24 x {dword, tag}
constexpr int DEBLOCK2_UNITS = 64 / H264R_DB2_LPU;              // k_deblock2: (picture, MB row) units per wave
constexpr int DEBLOCK2_PICS = DEBLOCK2_UNITS / H264R_DB2_BAND;  // pictures per wave

// Per-MB deblocking record, produced by k_inter4r for every MB (fully parallel) so
// that the order-dependent walk only loads 48 bytes per MB.  bs[] folds the edge
// enables of Deblock::strength (deblock.cc:236-278) into the strengths: a
// disabled edge has bS 0.  bs[hor * 16 + edge * 4 + segment]; chroma edge 0 uses
// luma edge 0, chroma edge 1 (sample 4) luma edge 2 (deblock.cc:430-433).
struct DbInfo {
    uint8_t  bs[32];
    uint32_t par[9];       // [Y, Cb, Cr][left edge, top edge, internal edges]: edge_word()
    uint32_t pad[3];
};
static_assert(sizeof(DbInfo) == 80, "DbInfo layout");
constexpr int DBINFO_DWORDS = 20;

// ------------------------------------------------------------------ the device error word
// err[0] of the context (h264r_check, h264r_picture_wait: any non-zero word is H264R_EDEVICE; err[1]
// is the wait bound, device_common.h).  The conditions that end a launch early store their value
// (the first error drains the grid, wait_give_up); the refusals of an input OR their bit.
enum DevErr : int {
    // a bounded wait expired (stored by wait_give_up: k_intra_pic, k_intra_levels, k_deblock,
    // k_deblock2 / 2y / 2c, k_c422_intra, k_c422_db)
    DEV_ERR_WAIT = 1,
    // a picture that is no frame on a 4:4:4 / 4:2:2 / 4:0:0 context (OR-ed by k_derive444): the
    // same bit as DEV_ERR_WAIT
    DEV_ERR_NOT_FRAME = 1,
    // a band that starts below row 0 has a top edge to filter (stored by k_deblock,
    // k_deblock2 / 2y / 2c, k_mbaff_deblock)
    DEV_ERR_BAND_EDGE = 2,
    // a broken schedule: an XCD's tickets left untaken (stored by xcd_drain_check: k_deblock,
    // k_deblock2 / 2y / 2c), a level-list pair that is not pairable (stored by k_intra_levels)
    DEV_ERR_SCHEDULE = 3,
    // not decoded off 4:2:0: an SP slice (OR-ed by k_derive444, stored by k_c422_inter), a
    // reference without its chroma plane (stored by k_c422_inter / k_c422_intra)
    DEV_ERR_FORMAT = 4,
    // MBAFF: a reference slot without a plane (stored by k_mbaff_inter)
    DEV_ERR_MBAFF_REF = 5,
    // MBAFF: what that launch sequence does not decode, k_mbaff.hip (OR-ed by k_mbaff_inter)
    DEV_ERR_MBAFF_REFUSED = 8,
    // a refused output frame (OR-ed by k_output, k_output_rgb, k_output_rgb_scaled, k_output_rgb_resampled), a refused box
    // (OR-ed by k_output_boxes_plan), a refused deinterlacing job (OR-ed by k_deinterlace)
    DEV_ERR_OUTPUT = 16,
};

}  // namespace h264r

// ------------------------------------------------------------------ prototypes
// k_recon.hip
extern "C" __global__ void k_inter4r(h264r_batch b, h264r::DbInfo* dbinfo, int2 rows, int* sp_flag, uint8_t* recon, int tag,
                                     int* zero, int nz, int* zero2, int nz2);
extern "C" __global__ void k_inter_sp(h264r_batch b, int2 rows, const int* sp_flag, uint8_t* recon, int tag);
extern "C" __global__ void k_untile(h264r_batch b, int2 rows, const uint8_t* recon);
extern "C" __global__ void k_derive444(h264r_batch b, int pl, int qpl, h264r_mb* mbs, h264r_slice* slices, h264r_quant* quant,
                                       const uint8_t** refs, int ntab, int* err);
// k_picture.hip
extern "C" __global__ void k_intra_pic(h264r_batch b, int* sync, int* err, const uint16_t* lvl, int lmax, int2 rows,
                                       int gstep, uint8_t* recon, const int* pband);
extern "C" __global__ void k_level(h264r_batch b, uint16_t* lvl, int* lvsync, int* lcount, int2 rows, int deep_cut,
                                   int lmax, int* pband);
extern "C" __global__ void k_level_scatter(h264r_batch b, const uint16_t* lvl, const int* lcount, int* lbase, int* lcursor,
                                           uint32_t* list, int2 rows);
extern "C" __global__ void k_intra_levels(h264r_batch b, const int* lcount, const int* lbase, const uint32_t* list,
                                          int lmax, int* lvsync, int* err, uint8_t* recon, int* bar);
#ifdef H264R_TRACE_INTRA
extern "C" __global__ void k_intra_trace_dump(unsigned long long* out, unsigned* n);
#endif
// k_deblock.hip, and k_deblock2.hip under its three kernel names (Makefile)
extern "C" __global__ void k_deblock(h264r_batch b, const h264r::DbInfo* dbinfo, uint64_t* hb,
                                     int* sync, int* err, uint32_t epoch, int2 rows, int nx, uint8_t* recon);
extern "C" __global__ void k_deblock2(h264r_batch b, const h264r::DbInfo* dbinfo, uint64_t* hb,
                                      int* sync, int* err, uint32_t epoch, int2 rows, int nx, const uint8_t* recon);
extern "C" __global__ void k_deblock2y(h264r_batch b, const h264r::DbInfo* dbinfo, uint64_t* hb,
                                       int* sync, int* err, uint32_t epoch, int2 rows, int nx, const uint8_t* recon);
extern "C" __global__ void k_deblock2c(h264r_batch b, const h264r::DbInfo* dbinfo, uint64_t* hb,
                                       int* sync, int* err, uint32_t epoch, int2 rows, int nx, const uint8_t* recon);
// k_chroma422.hip
extern "C" __global__ void k_c422_inter(h264r_batch b, int2 rows, int* err);
extern "C" __global__ void k_c422_intra(h264r_batch b, int2 rows, int* err);
extern "C" __global__ void k_c422_db(h264r_batch b, const h264r::DbInfo* dbinfo, int2 rows, int* err);
// k_mbaff.hip
extern "C" __global__ void k_mbaff_inter(h264r_batch b, int2 rows, int* err);
extern "C" __global__ void k_mbaff_intra(h264r_batch b, int diag, int2 rows, int* err);
extern "C" __global__ void k_mbaff_deblock(h264r_batch b, int diag, int2 rows, int* err);
// k_output.hip
extern "C" __global__ void k_output(h264r::OutJob job, const h264r_out_frame* frames, uint8_t* dst, int* err);
// k_output.hip: RGB frames
extern "C" __global__ void k_output_rgb(h264r::RgbJob job, const h264r_out_frame* frames, uint8_t* dst, int* err);
// k_output_scale.hip: scaled RGB frames, one kernel k_output_rgb_scaled_<name> per RgbMode and filter
#define H264R_SCALE_KERNELS(X)                                 \
    X(mono_bilinear, h264r::RGB_MONO, H264R_SCALE_BILINEAR)    \
    X(full_bilinear, h264r::RGB_FULL, H264R_SCALE_BILINEAR)    \
    X(gbr_bilinear, h264r::RGB_GBR, H264R_SCALE_BILINEAR)      \
    X(rep_bilinear, h264r::RGB_REP, H264R_SCALE_BILINEAR)      \
    X(bil1_bilinear, h264r::RGB_BIL1, H264R_SCALE_BILINEAR)    \
    X(bil2_bilinear, h264r::RGB_BIL2, H264R_SCALE_BILINEAR)    \
    X(mono_area, h264r::RGB_MONO, H264R_SCALE_AREA)            \
    X(full_area, h264r::RGB_FULL, H264R_SCALE_AREA)            \
    X(gbr_area, h264r::RGB_GBR, H264R_SCALE_AREA)              \
    X(rep_area, h264r::RGB_REP, H264R_SCALE_AREA)              \
    X(bil1_area, h264r::RGB_BIL1, H264R_SCALE_AREA)            \
    X(bil2_area, h264r::RGB_BIL2, H264R_SCALE_AREA)
#define H264R_SCALE_KERNEL_DECL(NAME, MODE, FILTER) \
    extern "C" __global__ void k_output_rgb_scaled_##NAME(h264r::ScaleJob job, const h264r_out_frame* frames, uint8_t* dst, int* err);
H264R_SCALE_KERNELS(H264R_SCALE_KERNEL_DECL)
// k_output_boxes.hip: boxes of scaled RGB from a device table.  k_output_boxes_plan resolves every box into
// a BoxPlan (and refuses what out_box_status refuses, output_boxes.h); one kernel k_output_boxes_<name>
// per RgbMode and filter then writes the pixels of all of them.
extern "C" __global__ void k_output_boxes_plan(h264r::BoxesJob job, const h264r_out_frame* frames, const h264r_out_box* boxes,
                                               h264r::BoxPlan* plans, int* err);
#define H264R_BOXES_KERNEL_DECL(NAME, MODE, FILTER) \
    extern "C" __global__ void k_output_boxes_##NAME(h264r::BoxesJob job, const h264r_out_frame* frames, const h264r::BoxPlan* plans, uint8_t* dst);
H264R_SCALE_KERNELS(H264R_BOXES_KERNEL_DECL)
// k_output_resample.hip: Pillow-exact resampled RGB frames, one kernel k_output_rgb_resampled_<name> per RgbMode
#define H264R_RESAMPLE_KERNELS(X) \
    X(mono, h264r::RGB_MONO)      \
    X(full, h264r::RGB_FULL)      \
    X(gbr, h264r::RGB_GBR)        \
    X(rep, h264r::RGB_REP)        \
    X(bil1, h264r::RGB_BIL1)      \
    X(bil2, h264r::RGB_BIL2)
#define H264R_RESAMPLE_KERNEL_DECL(NAME, MODE) \
    extern "C" __global__ void k_output_rgb_resampled_##NAME(h264r::ResampleJob job, const h264r_out_frame* frames, uint8_t* dst, int* err);
H264R_RESAMPLE_KERNELS(H264R_RESAMPLE_KERNEL_DECL)
// k_deinterlace.hip: deinterlaced frames (h264r_deinterlace.h), every job and plane in one launch
static_assert(h264r::DEINT_TW == H264R_DEINT_TILE_W && h264r::DEINT_TH == H264R_DEINT_TILE_H, "the header names the kernel's tile");
extern "C" __global__ void k_deinterlace(h264r::DeintJob job, const h264r_out_frame* frames, const h264r_deint_job* jobs, uint8_t* dst,
                                         int* err);
