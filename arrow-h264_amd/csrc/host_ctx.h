// host_ctx.h -- what the host files share (h264r_host.hip, host_stream.hip, host_output.hip,
// h264r_group.hip): the context, its per-batch scratch, owned device memory (DevBuf) and the
// HIP_OK macro.  Host only: no kernel includes it.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "h264r.h"
#include "output_job.h"
#include "picture_stage.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
        fprintf(stderr, "h264r: %s failed: %s\n", #x, hipGetErrorString(e_)); return H264R_EDEVICE; } } while (0)

// not exported from libh264r.so
#define H264R_INTERNAL __attribute__((visibility("hidden")))

namespace h264r {

// A device buffer of cap elements that frees itself.  p and cap are for reading.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { reset(); }
    void reset()
    {
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
    }
    // Room for n elements: the buffer as it is when it fits, else a new one (the contents are lost).
    int reserve(size_t n)
    {
        if (n <= cap && p) return H264R_OK;
        // work still queued may read the old buffer (h264r_picture_end_async): drain it first
        if (p) (void)hipDeviceSynchronize();
        reset();
        if (hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) return H264R_ENOMEM;
        cap = n;
        return H264R_OK;
    }
};

constexpr int OVERLAP_MAX = 16;     // chunks of the overlapped schedule at most (H264R_OVERLAP)

// Per-batch scratch of one launch sequence.
struct Scratch {
    DevBuf<uint8_t> d_dbinfo;
    DevBuf<int> d_sync;             // a sync region (sync_words.h) per chunk of the overlapped schedule
    int tag = 0;                    // launch-sequence tag (> 0): k_inter4r's SP word
    // the SP word of each chunk: k_inter4r stores the launch tag there when it met an inter MB of
    // an SP slice.  Allocated and zeroed once and written by nothing else, so a word only ever
    // holds tags of earlier launches, whatever their shape
    DevBuf<int> d_sptag;
    DevBuf<uint8_t> d_hb;
    uint32_t epoch = 0;             // tag of the deblocking hand-off records of the last launch
    DevBuf<uint8_t> d_hb2;
    uint32_t epoch2 = 0;            // the same for k_deblock2 (< 2^20: its tags carry the row)
    DevBuf<uint16_t> d_lvl;         // intra dependency level per MB
    DevBuf<uint32_t> d_list;        // intra MBs by level (pic * nmb + addr)
    DevBuf<int> d_lcnt;             // [count | base | cursor] x LEVEL_IDS
    DevBuf<uint8_t> d_recon;        // MB-tiled reconstruction, 384 B per (picture, MB)
};

}  // namespace h264r

struct h264r_ctx {
    template <typename T> using DevBuf = h264r::DevBuf<T>;
    int device = 0;
    int max_w = 0, max_h = 0;
    int fmt = 1;                          // chroma_format_idc: 1 (4:2:0), 0 (4:0:0) / 2 (4:2:2) (run_422) or 3 (4:4:4, run_444)
    // 4:4:4: one colour plane's derived batch (k_derive444) -- records, slices, quant, DPB tables --
    // and the scratch its unused 4:2:0 chroma outputs go to
    DevBuf<h264r_mb> d444_mbs;
    DevBuf<h264r_slice> d444_slices;
    DevBuf<h264r_quant> d444_quant;
    DevBuf<const uint8_t*> d444_refs;
    DevBuf<uint8_t> d444_chroma;
    hipStream_t stream = nullptr;
    // DPB slots: one allocation each, slot[s][0] its base
    uint8_t* slot[H264R_MAX_SLOTS][3] = {};
    int slot_w[H264R_MAX_SLOTS] = {}, slot_h[H264R_MAX_SLOTS] = {};
    DevBuf<const uint8_t*> d_ref_planes;
    DevBuf<int> d_err;                    // [0] device error word (a bounded wait expired), [1] wait bound
    uint32_t wait_ticks = 0;              // err[1] as last written (s_memrealtime ticks, 100 MHz)
    uint32_t wait_val = 0;                // its host copy, the source of the async write
    DevBuf<h264r::BoxPlan> d_box_plans;   // h264r_output_rgb_boxes: a plan per box of the largest job so far
    // streaming-API staging: two pictures, so that one is parsed (h264r_picture_begin /
    // h264r_mb_submit) while the other is reconstructed (h264r_picture_end_async)
    struct StreamPic {
        h264r::PictureStage st;
        uint8_t* out = nullptr; size_t c_out = 0;   // pinned planes Y | Cb | Cr, then the error word
        hipEvent_t done = nullptr;                 // its uploads, launches and readback
        bool pending = false;
    };
    StreamPic sp[2];
    int sp_fill = 0, sp_wait = 0, sp_pending = 0;
    // device buffers of the streaming API
    DevBuf<h264r_mb> d_mbs;
    DevBuf<int16_t> d_levels;
    DevBuf<uint32_t> d_mv;
    DevBuf<int8_t> d_ref;
    DevBuf<h264r_slice> d_slices;
    DevBuf<h264r_pic> d_pic;
    DevBuf<h264r_quant> d_quant;
    DevBuf<h264r_field_poc> d_fpoc;
    DevBuf<uint8_t> d_out;
    // per-batch scratch of the launch sequence
    h264r::Scratch sc;
    int levels_grid = 0;                           // resident workgroups of k_intra_levels
    int nxcc = 0;                                  // XCDs of the device (k_deblock2's placement)
    // the per-batch scratch above is reused by every launch: a launch on a stream other
    // than the previous one first waits for the previous launch (ev_last, order_after_last)
    hipStream_t last_stream = nullptr;
    hipEvent_t ev_last = nullptr;
    // the overlapped schedule (launch_all): deblocking of picture chunk k on `side` while the
    // launch stream reconstructs chunk k + 1; ev_chunk[k] = chunk k reconstructed, ev_side =
    // the side stream's last deblocking launch (the launch stream waits for it at the end)
    hipStream_t side = nullptr;
    std::vector<hipEvent_t> ev_chunk;
    hipEvent_t ev_side = nullptr;
    hipEvent_t ev_fork = nullptr;              // the split deblocking walk: launch stream -> side stream
    // timing: every kernel of every launch bracketed by events on its stream
    bool timing = false;
    int debug = 0;
    struct Span { int kind; hipEvent_t a, b; };
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    std::vector<Span> spans;
    int timed_launches = 0;

    h264r_ctx() = default;
    h264r_ctx(const h264r_ctx&) = delete;
    h264r_ctx& operator=(const h264r_ctx&) = delete;
    // Everything the context owns that is no DevBuf; the caller has set the device and drained the
    // streams (h264r_destroy).
    ~h264r_ctx()
    {
        for (auto& s : slot) if (s[0]) (void)hipFree(s[0]);
        for (auto& p : sp) {
            if (p.out) (void)hipHostFree(p.out);
            if (p.done) (void)hipEventDestroy(p.done);
        }
        for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
        for (hipEvent_t e : ev_chunk) (void)hipEventDestroy(e);
        for (hipEvent_t e : {ev_last, ev_side, ev_fork}) if (e) (void)hipEventDestroy(e);
        for (hipStream_t s : {side, stream}) if (s) (void)hipStreamDestroy(s);
    }
};

namespace h264r {

// Bytes of one chroma plane of a w x h MB picture: 8 x 8 samples per MB (4:2:0), 8 x 16 (4:2:2)
// or 16 x 16 (4:4:4).
inline size_t chroma_bytes(const h264r_ctx* c, int w, int h)
{
    return (size_t)w * h * (c->fmt == 3 ? 256 : c->fmt == 2 ? 128 : c->fmt == 1 ? 64 : 0);     // 4:0:0: none
}

// h264r_host.hip, for host_stream.hip and host_output.hip
H264R_INTERNAL int ensure_slot(h264r_ctx* c, int slot, int w, int h);
H264R_INTERNAL int order_after_last(h264r_ctx* c, hipStream_t s);
H264R_INTERNAL int run_batch(h264r_ctx* c, const h264r_batch& b, hipStream_t s, int row0, int row1);

}  // namespace h264r
