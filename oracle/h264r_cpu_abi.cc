/*
 * h264r_cpu_abi.cc -- TEST INFRASTRUCTURE ONLY.
 *
 * The per-picture streaming entry points of include/h264r.h implemented on the CPU
 * oracle (oracle/h264r_oracle.c), so that the reference's own parser + the drop-in
 * Decoder shim (shim/decoder_h264r.cc) can be linked and run in this container, which
 * has no GPU: oracle/_ref/ldecod_shim (oracle/Makefile `ref`).  It checks that the shim
 * feeds the boundary exactly what the reference reconstructs from (the shim build's
 * YUV == the unmodified reference's YUV), and it records what crossed the boundary:
 * with H264R_CAPTURE=<file> every picture's arrays (MB records, level pool, motion,
 * slices, picture parameters, quantisation tables, keep slot) and the oracle's planes
 * are appended to <file>, the replay fixtures of tests/test_stream_parity.py, which the
 * GPU tests decode through libh264r.so.  Never linked into the product.
 *
 * A picture is staged and judged by the product's own PictureStage (csrc/picture_stage.h), so
 * what is recorded here passed the checks of the library it is replayed through; the
 * quantisation tables and status strings are that header's too.  There is no
 * h264r_picture_field_pocs: the oracle takes no such record.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <vector>

#include "h264r.h"
#include "h264r_oracle.h"
#include "picture_stage.h"

struct h264r_ctx {
    int max_w = 0, max_h = 0;
    int cf = 1, cb = 64;        /* chroma_format_idc and chroma bytes per MB and plane (64, 128, 256) */
    std::vector<uint8_t> slot_mem[H264R_MAX_SLOTS];
    uint8_t* slot[H264R_MAX_SLOTS][3] = {};
    int slot_w[H264R_MAX_SLOTS] = {}, slot_h[H264R_MAX_SLOTS] = {};
    h264r::PictureStage st;
    std::vector<uint8_t> async_out[2];      /* h264r_picture_end_async staging, Y | Cb | Cr */
    int async_head = 0, n_async = 0;
};

int h264r_abi_version(void) { return H264R_ABI_VERSION; }
const char* h264r_strerror(int s) { return h264r::status_string(s); }
int h264r_device_count(void) { return 0; }
int h264r_quant_init_flat(h264r_quant* q) { return h264r::quant_init_flat(q); }
int h264r_quant_init_lists(h264r_quant* q, const int32_t* const qm[12]) { return h264r::quant_init_lists(q, qm); }

int h264r_create(h264r_ctx** out, int device, int max_w, int max_h, int chroma_format_idc, int bit_depth)
{
    (void)device;
    if (!out || max_w <= 0 || max_h <= 0) return H264R_EINVAL;
    if (chroma_format_idc < 0 || chroma_format_idc > 3 || bit_depth != 8) return H264R_EUNSUPPORTED;
    h264r_ctx* c = new (std::nothrow) h264r_ctx();
    if (!c) return H264R_ENOMEM;
    c->max_w = max_w; c->max_h = max_h;
    c->cf = chroma_format_idc;
    c->cb = chroma_format_idc == 3 ? 256 : chroma_format_idc == 2 ? 128 : chroma_format_idc == 1 ? 64 : 0;
    *out = c;
    return H264R_OK;
}

int h264r_destroy(h264r_ctx* c)
{
    if (!c) return H264R_EINVAL;
    delete c;
    return H264R_OK;
}

static int ensure_slot(h264r_ctx* c, int s, int w, int h)
{
    if (c->slot[s][0] && c->slot_w[s] == w && c->slot_h[s] == h) return H264R_OK;
    size_t ys = (size_t)w * h * 256, cs = (size_t)w * h * c->cb;
    c->slot_mem[s].assign(ys + 2 * cs, 0);
    uint8_t* b = c->slot_mem[s].data();
    c->slot[s][0] = b; c->slot[s][1] = b + ys; c->slot[s][2] = b + ys + cs;
    c->slot_w[s] = w; c->slot_h[s] = h;
    return H264R_OK;
}

int h264r_set_ref(h264r_ctx* c, int slot, const uint8_t* y, const uint8_t* u, const uint8_t* v, int w, int h)
{
    if (!c || slot < 0 || slot >= H264R_MAX_SLOTS || !y || (c->cb && (!u || !v))) return H264R_EINVAL;
    int st = ensure_slot(c, slot, w, h);
    if (st) return st;
    memcpy(c->slot[slot][0], y, (size_t)w * h * 256);
    if (c->cb) {
        memcpy(c->slot[slot][1], u, (size_t)w * h * c->cb);
        memcpy(c->slot[slot][2], v, (size_t)w * h * c->cb);
    }
    return H264R_OK;
}

int h264r_ref_planes(h264r_ctx* c, int slot, uint8_t** y, uint8_t** u, uint8_t** v)
{
    if (!c || slot < 0 || slot >= H264R_MAX_SLOTS) return H264R_EINVAL;
    if (y) *y = c->slot[slot][0];
    if (u) *u = c->slot[slot][1];
    if (v) *v = c->slot[slot][2];
    return c->slot[slot][0] ? H264R_OK : H264R_ESTATE;
}

int h264r_picture_begin(h264r_ctx* c, int w, int h, const h264r_pic* pic, const h264r_slice* slices,
                        const h264r_quant* quant)
{
    return c ? c->st.begin(c->max_w, c->max_h, w, h, pic, slices, quant, false) : H264R_EINVAL;
}

int h264r_mb_submit(h264r_ctx* c, int addr, const h264r_mb* mb, const int16_t* levels, int n_levels,
                    const uint32_t* mv, const int8_t* ref_idx)
{
    return c ? c->st.submit(addr, mb, levels, n_levels, mv, ref_idx) : H264R_EINVAL;
}

/* Capture record (little-endian): int32 header[8] = {'H4RC', W, H, num_slices, n_levels,
 * keep_slot, chroma_format_idc, 1}, then mbs, levels, mv, ref_idx, slices, pic, quant, Y, Cb, Cr
 * (header[7] 1: header[6] holds the chroma format; 0 in captures older than that: 4:2:0).
 * The levels are the pool as submitted, without the padding PictureStage::finish adds. */
static void capture(const h264r_ctx* c, int keep, uint8_t* const out[3])
{
    const char* path = getenv("H264R_CAPTURE");
    if (!path) return;
    FILE* f = fopen(path, "ab");
    if (!f) return;
    const h264r::PictureStage& P = c->st;
    const size_t n = (size_t)P.pw * P.ph;
    int32_t hdr[8] = {0x43523448, P.pw, P.ph, P.h_pic.num_slices, (int32_t)P.n_submitted, keep, c->cf, 1};
    fwrite(hdr, 4, 8, f);
    fwrite(P.h_mbs.data(), sizeof(h264r_mb), n, f);
    fwrite(P.h_levels.data(), 2, P.n_submitted, f);
    fwrite(P.h_mv.data(), 4, 2 * 16 * n, f);
    fwrite(P.h_ref.data(), 1, 2 * 16 * n, f);
    fwrite(P.h_slices.data(), sizeof(h264r_slice), P.h_pic.num_slices, f);
    fwrite(&P.h_pic, sizeof(h264r_pic), 1, f);
    fwrite(&P.h_quant, sizeof(h264r_quant), 1, f);
    fwrite(out[0], 1, n * 256, f);
    fwrite(out[1], 1, n * c->cb, f);
    fwrite(out[2], 1, n * c->cb, f);
    fclose(f);
}

static int picture_end(h264r_ctx* c, uint8_t* y, uint8_t* u, uint8_t* v, int keep)
{
    h264r::PictureStage& P = c->st;
    h264r::StageSlot slots[H264R_MAX_SLOTS];
    for (int s = 0; s < H264R_MAX_SLOTS; ++s) slots[s] = {c->slot[s][0] != NULL, c->slot_w[s], c->slot_h[s]};
    int st = P.finish(c->cf, keep, slots);
    if (st) return st;
    if (!y || (c->cb && (!u || !v))) return H264R_EINVAL;      /* the oracle writes the caller's planes */
    /* a field picture's slots are frames of twice its height (include/h264r.h); an MBAFF frame is a frame */
    const int fld = P.field(), frame_h = P.ph << fld;
    oracle_picture p;
    memset(&p, 0, sizeof(p));
    p.width_mbs = P.pw; p.height_mbs = P.ph;
    p.mbs = P.h_mbs.data(); p.levels = P.h_levels.data(); p.mv = P.h_mv.data(); p.ref_idx = P.h_ref.data();
    p.slices = P.h_slices.data(); p.pic = &P.h_pic; p.quant = &P.h_quant;
    for (int s = 0; s < H264R_MAX_SLOTS; ++s)
        if (c->slot[s][0] && c->slot_w[s] == P.pw && c->slot_h[s] == frame_h)
            for (int k = 0; k < 3; ++k) p.ref_planes[s][k] = c->slot[s][k];
    p.out[0] = y; p.out[1] = u; p.out[2] = v;
    p.chroma_format = c->cf;
    st = oracle_decode_picture(&p);
    if (st) {
        if (getenv("H264R_CPU_VERBOSE")) fprintf(stderr, "h264r (cpu): oracle_decode_picture -> %d\n", st);
        return H264R_EINVAL;
    }
    uint8_t* out[3] = {y, u, v};
    capture(c, keep, out);
    if (keep >= 0 && !fld) {
        if ((st = h264r_set_ref(c, keep, y, u, v, P.pw, P.ph))) return st;
    } else if (keep >= 0) {
        /* a field into its parity's rows of the slot's frame (dpb_combine_field_yuv
           picture.cc:578-622), the other field's rows left as they are */
        if ((st = ensure_slot(c, keep, P.pw, frame_h))) return st;
        const int bot = P.h_pic.structure == H264R_BOTTOM_FIELD;
        for (int k = 0; k < 3; ++k) {
            const int w = k ? P.pw * 8 : P.pw * 16, h = k ? P.ph * 8 : P.ph * 16;
            for (int r = 0; r < h; ++r) memcpy(c->slot[keep][k] + (size_t)(2 * r + bot) * w, out[k] + (size_t)r * w, w);
        }
    }
    return H264R_OK;
}

/* The asynchronous form: the CPU computes the picture at once into one of two staging sets,
 * h264r_picture_wait hands them out oldest first (the GPU library's contract). */
int h264r_picture_end_async(h264r_ctx* c, int keep)
{
    if (!c) return H264R_EINVAL;
    if (c->n_async == 2) return H264R_ESTATE;
    const size_t n = (size_t)c->st.pw * c->st.ph;
    std::vector<uint8_t>& buf = c->async_out[(c->async_head + c->n_async) % 2];
    buf.resize(n * (256 + 2 * c->cb));
    int st = picture_end(c, buf.data(), buf.data() + n * 256, buf.data() + n * (256 + c->cb), keep);
    if (st) return st;
    ++c->n_async;
    return H264R_OK;
}

int h264r_picture_wait(h264r_ctx* c, uint8_t* y, uint8_t* u, uint8_t* v)
{
    if (!c) return H264R_EINVAL;
    if (!c->n_async) return H264R_ESTATE;
    const std::vector<uint8_t>& buf = c->async_out[c->async_head];
    const size_t n = buf.size() / (256 + 2 * c->cb);
    if (y) memcpy(y, buf.data(), n * 256);
    if (u) memcpy(u, buf.data() + n * 256, n * c->cb);
    if (v) memcpy(v, buf.data() + n * (256 + c->cb), n * c->cb);
    c->async_head = (c->async_head + 1) % 2;
    --c->n_async;
    return H264R_OK;
}

int h264r_picture_end(h264r_ctx* c, uint8_t* y, uint8_t* u, uint8_t* v, int keep)
{
    if (!c) return H264R_EINVAL;
    if (c->n_async) return H264R_ESTATE;
    return picture_end(c, y, u, v, keep);
}

int h264r_check(h264r_ctx* c) { return c ? H264R_OK : H264R_EINVAL; }
