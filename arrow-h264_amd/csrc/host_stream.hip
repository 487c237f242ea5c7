// host_stream.hip -- the streaming API of include/h264r.h (h264r_picture_begin / h264r_mb_submit /
// h264r_picture_end_async / h264r_picture_wait): each entry point checks its context, lets the
// picture's PictureStage (picture_stage.h) stage and judge the picture, and h264r_picture_end_async
// then uploads the stage and runs it as a batch of one picture.  Two stages, so that one picture is
// parsed while the other is reconstructed.
#include <hip/hip_runtime.h>

#include <cstring>

#include "h264r.h"
#include "host_ctx.h"

using namespace h264r;

int h264r_picture_begin(h264r_ctx* c, int w, int h, const h264r_pic* pic, const h264r_slice* slices,
                        const h264r_quant* quant)
{
    if (!c) return H264R_EINVAL;
    // both staging pictures in flight: the caller collects one first (h264r_picture_wait)
    return c->sp[c->sp_fill].st.begin(c->max_w, c->max_h, w, h, pic, slices, quant, c->sp_pending == 2);
}

int h264r_picture_field_pocs(h264r_ctx* c, const h264r_field_poc* rec)
{
    return c ? c->sp[c->sp_fill].st.field_pocs(rec) : H264R_EINVAL;
}

int h264r_mb_submit(h264r_ctx* c, int addr, const h264r_mb* mb, const int16_t* levels, int n_levels,
                    const uint32_t* mv, const int8_t* ref_idx)
{
    return c ? c->sp[c->sp_fill].st.submit(addr, mb, levels, n_levels, mv, ref_idx) : H264R_EINVAL;
}

int h264r_picture_end_async(h264r_ctx* c, int keep_slot)
{
    if (!c) return H264R_EINVAL;
    auto& R = c->sp[c->sp_fill];
    PictureStage& P = R.st;
    StageSlot slots[H264R_MAX_SLOTS];
    for (int k = 0; k < H264R_MAX_SLOTS; ++k) slots[k] = {c->slot[k][0] != nullptr, c->slot_w[k], c->slot_h[k]};
    int st = P.finish(c->fmt, keep_slot, slots);
    if (st) return st;
    (void)hipSetDevice(c->device);
    const size_t n = (size_t)P.pw * P.ph, ys = n * 256, cs = chroma_bytes(c, P.pw, P.ph);
    const int fld = P.field(), frame_h = P.ph << fld;
    // the device inputs are one set, reused in stream order (DevBuf::reserve drains before it frees)
    if ((st = c->d_mbs.reserve(n)) || (st = c->d_levels.reserve(P.h_levels.size())) ||
        (st = c->d_mv.reserve(P.h_mv.size())) || (st = c->d_ref.reserve(P.h_ref.size())) ||
        (st = c->d_slices.reserve(P.h_slices.size())) || (st = c->d_pic.reserve(1)) ||
        (st = c->d_quant.reserve(1)) || (st = c->d_out.reserve(ys + 2 * cs)) ||
        (P.has_fpoc && (st = c->d_fpoc.reserve(1))))
        return st;
    if (R.c_out < ys + 2 * cs + 16) {
        if (R.out) (void)hipHostFree(R.out);
        R.out = nullptr; R.c_out = 0;
        if (hipHostMalloc(reinterpret_cast<void**>(&R.out), ys + 2 * cs + 16) != hipSuccess) return H264R_ENOMEM;
        R.c_out = ys + 2 * cs + 16;
    }
    if (!R.done) HIP_OK(hipEventCreateWithFlags(&R.done, hipEventDisableTiming));
    hipStream_t s = c->stream;
    uint8_t* const d_out = c->d_out.p;
    HIP_OK(hipMemcpyAsync(c->d_mbs.p, P.h_mbs.data(), n * sizeof(h264r_mb), hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(c->d_levels.p, P.h_levels.data(), P.h_levels.size() * 2, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(c->d_mv.p, P.h_mv.data(), P.h_mv.size() * 4, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(c->d_ref.p, P.h_ref.data(), P.h_ref.size(), hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(c->d_slices.p, P.h_slices.data(), P.h_slices.size() * sizeof(h264r_slice), hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(c->d_pic.p, &P.h_pic, sizeof(h264r_pic), hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(c->d_quant.p, &P.h_quant, sizeof(h264r_quant), hipMemcpyHostToDevice, s));
    if (P.has_fpoc) HIP_OK(hipMemcpyAsync(c->d_fpoc.p, &P.h_fpoc, sizeof(h264r_field_poc), hipMemcpyHostToDevice, s));
    h264r_batch b{};
    b.num_pics = 1; b.width_mbs = P.pw; b.height_mbs = P.ph; b.slice_stride = (int)P.h_slices.size();
    b.mbs = c->d_mbs.p; b.levels = c->d_levels.p; b.mv = c->d_mv.p; b.ref_idx = c->d_ref.p; b.slices = c->d_slices.p;
    b.pics = c->d_pic.p; b.quant = c->d_quant.p; b.ref_planes = c->d_ref_planes.p;
    b.out_y = d_out; b.out_u = d_out + ys; b.out_v = d_out + ys + cs;
    b.mbaff = P.mbaff();
    b.field_poc = P.has_fpoc ? c->d_fpoc.p : nullptr;
    if ((st = run_batch(c, b, s, 0, b.height_mbs))) return st;
    if (keep_slot >= 0) {
        if ((st = ensure_slot(c, keep_slot, P.pw, frame_h))) return st;
        if (!fld) {
            HIP_OK(hipMemcpyAsync(c->slot[keep_slot][0], d_out, ys + 2 * cs, hipMemcpyDeviceToDevice, s));
        } else {
            // a field goes into its parity's rows of the slot's frame (the reference combines the
            // two fields of a frame with dpb_combine_field_yuv, picture.cc:578-622); the other
            // field's rows are left as they are
            const int bot = P.h_pic.structure == H264R_BOTTOM_FIELD;
            const size_t W = (size_t)P.pw * 16, Wc = W / 2;
            HIP_OK(hipMemcpy2DAsync(c->slot[keep_slot][0] + bot * W, 2 * W, d_out, W, W, (size_t)P.ph * 16,
                                    hipMemcpyDeviceToDevice, s));
            for (int k = 1; k < 3; ++k)
                HIP_OK(hipMemcpy2DAsync(c->slot[keep_slot][k] + bot * Wc, 2 * Wc, d_out + ys + (k - 1) * cs, Wc, Wc,
                                        (size_t)P.ph * 8, hipMemcpyDeviceToDevice, s));
        }
    }
    // planes and the device error word into this picture's pinned staging; the error word is
    // cleared behind it, so each picture reports its own failures
    HIP_OK(hipMemcpyAsync(R.out, d_out, ys + 2 * cs, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(R.out + ys + 2 * cs, c->d_err.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemsetAsync(c->d_err.p, 0, sizeof(int), s));
    HIP_OK(hipEventRecord(R.done, s));
    R.pending = true;
    ++c->sp_pending;
    c->sp_fill = 1 - c->sp_fill;
    return H264R_OK;
}

int h264r_picture_wait(h264r_ctx* c, uint8_t* y, uint8_t* u, uint8_t* v)
{
    if (!c) return H264R_EINVAL;
    auto& R = c->sp[c->sp_wait];
    if (!c->sp_pending || !R.pending) return H264R_ESTATE;
    (void)hipSetDevice(c->device);
    HIP_OK(hipEventSynchronize(R.done));
    R.pending = false;
    --c->sp_pending;
    c->sp_wait = 1 - c->sp_wait;
    const size_t n = (size_t)R.st.pw * R.st.ph, ys = n * 256, cs = chroma_bytes(c, R.st.pw, R.st.ph);
    if (y) memcpy(y, R.out, ys);
    if (u) memcpy(u, R.out + ys, cs);
    if (v) memcpy(v, R.out + ys + cs, cs);
    int e = 0;
    memcpy(&e, R.out + ys + 2 * cs, sizeof(int));
    return e ? H264R_EDEVICE : H264R_OK;
}

int h264r_picture_end(h264r_ctx* c, uint8_t* y, uint8_t* u, uint8_t* v, int keep_slot)
{
    if (!c) return H264R_EINVAL;
    if (c->sp_pending) return H264R_ESTATE;        // collect the asynchronous pictures first
    int st = h264r_picture_end_async(c, keep_slot);
    if (st) return st;
    return h264r_picture_wait(c, y, u, v);
}
