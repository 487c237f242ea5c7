// picture_stage.h -- the device-free part of the host layer, stated once: the LevelScale tables and
// the quantisation-table initialisers, the status strings, and PictureStage, which stages one
// picture of the streaming API (h264r_picture_begin / h264r_mb_submit / h264r_picture_end_async,
// include/h264r.h) on the host and decides what is accepted.  Plain C++17, no HIP: the GPU library
// (host_stream.hip), the CPU implementation of the ABI (oracle/h264r_cpu_abi.cc) and the CPU check
// of the stage (oracle/stage_check.cc) all include it.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "h264r.h"

namespace h264r {

inline constexpr int dequant_coef[6][3] = {{10, 13, 16}, {11, 14, 18}, {13, 16, 20}, {14, 18, 23}, {16, 20, 25}, {18, 23, 29}};
inline constexpr int dq8_v[6][6] = {{20, 18, 32, 19, 25, 24}, {22, 19, 35, 21, 28, 26}, {26, 23, 42, 24, 33, 31},
                                    {28, 25, 45, 26, 35, 33}, {32, 28, 51, 30, 40, 38}, {36, 32, 58, 34, 46, 43}};

// normative LevelScale(m, i, j) (transform.cc:93-170 tables dequant_coef / dequant_coef8)
inline int norm4(int m, int i, int j)
{
    if ((i & 1) == 0 && (j & 1) == 0) return dequant_coef[m][0];
    if ((i & 1) && (j & 1)) return dequant_coef[m][2];
    return dequant_coef[m][1];
}
inline int norm8(int m, int i, int j)
{
    if (i % 4 == 0 && j % 4 == 0) return dq8_v[m][0];
    if (i % 2 == 1 && j % 2 == 1) return dq8_v[m][1];
    if (i % 4 == 2 && j % 4 == 2) return dq8_v[m][2];
    if ((i % 4 == 0 && j % 2 == 1) || (i % 2 == 1 && j % 4 == 0)) return dq8_v[m][3];
    if ((i % 4 == 0 && j % 4 == 2) || (i % 4 == 2 && j % 4 == 0)) return dq8_v[m][4];
    return dq8_v[m][5];
}

// h264r_quant_init_flat
inline int quant_init_flat(h264r_quant* q)
{
    if (!q) return H264R_EINVAL;
    for (int t = 0; t < 2; ++t)
        for (int pl = 0; pl < 3; ++pl)
            for (int m = 0; m < 6; ++m) {
                for (int k = 0; k < 16; ++k) q->scale4x4[t][pl][m][k] = (int16_t)(norm4(m, k / 4, k % 4) * 16);
                for (int k = 0; k < 64; ++k) q->scale8x8[t][pl][m][k] = (int16_t)(norm8(m, k / 8, k % 8) * 16);
            }
    return H264R_OK;
}

// h264r_quant_init_lists
inline int quant_init_lists(h264r_quant* q, const int32_t* const qm[12])
{
    // Transform::set_quant (transform.cc:259-302): InvLevelScale = dequant_coef x qmatrix.
    if (!q || !qm) return H264R_EINVAL;
    for (int i = 0; i < 12; ++i) if (!qm[i]) return H264R_EINVAL;
    for (int pl = 0; pl < 3; ++pl)
        for (int m = 0; m < 6; ++m) {
            for (int k = 0; k < 16; ++k) {
                q->scale4x4[0][pl][m][k] = (int16_t)(norm4(m, k / 4, k % 4) * qm[pl][k]);
                q->scale4x4[1][pl][m][k] = (int16_t)(norm4(m, k / 4, k % 4) * qm[3 + pl][k]);
            }
            for (int k = 0; k < 64; ++k) {
                // 8x8 lists: 6 Intra Y, 7 Inter Y, 8 Intra Cb, 9 Inter Cb, 10 Intra Cr, 11 Inter Cr
                q->scale8x8[0][pl][m][k] = (int16_t)(norm8(m, k / 8, k % 8) * qm[6 + 2 * pl][k]);
                q->scale8x8[1][pl][m][k] = (int16_t)(norm8(m, k / 8, k % 8) * qm[7 + 2 * pl][k]);
            }
        }
    return H264R_OK;
}

// h264r_strerror
inline const char* status_string(int s)
{
    switch (s) {
    case H264R_OK: return "ok";
    case H264R_EINVAL: return "invalid argument";
    case H264R_ENOMEM: return "out of memory";
    case H264R_EDEVICE: return "HIP runtime error";
    case H264R_ESTATE: return "call out of order";
    case H264R_EUNSUPPORTED: return "unsupported configuration";
    case H264R_ENODEVICE: return "no gfx950 device";
    default: return "unknown status";
    }
}

// What PictureStage::finish needs to know of a DPB slot.
struct StageSlot {
    bool loaded = false;
    int w = 0, h = 0;              // the slot's frame, in MBs
};

// One picture of the streaming API on the host: the arrays a batch of one picture is made of, and
// every check of the picture that needs no device.  The vectors keep their storage from picture
// to picture.
struct PictureStage {
    int pw = 0, ph = 0;
    std::vector<h264r_mb> h_mbs;
    std::vector<int16_t> h_levels;             // the level pool: a 16-byte aligned block per MB
    std::vector<uint32_t> h_mv;
    std::vector<int8_t> h_ref;
    std::vector<h264r_slice> h_slices;
    h264r_pic h_pic{};
    h264r_quant h_quant{};
    h264r_field_poc h_fpoc{};                  // h264r_picture_field_pocs: this picture's record
    bool has_fpoc = false;
    std::vector<uint8_t> seen;
    bool open = false;                         // between begin and finish
    size_t n_submitted = 0;                    // the level pool as submitted, before finish pads it

    bool field() const { return h_pic.structure == H264R_TOP_FIELD || h_pic.structure == H264R_BOTTOM_FIELD; }
    bool mbaff() const { return h_pic.structure == H264R_MBAFF_FRAME; }

    // h264r_picture_begin.  busy: the caller has no room for another picture (H264R_ESTATE, after
    // the argument checks).
    int begin(int max_w, int max_h, int w, int h, const h264r_pic* pic, const h264r_slice* slices, const h264r_quant* quant,
              bool busy)
    {
        if (!pic || !slices || !quant || w <= 0 || h <= 0 || w > max_w || h > max_h || pic->num_slices <= 0 ||
            pic->num_slices > H264R_MAX_SLICES)
            return H264R_EINVAL;
        if (busy) return H264R_ESTATE;
        pw = w; ph = h;
        const size_t n = (size_t)w * h;
        h_mbs.assign(n, h264r_mb{});
        h_levels.clear();
        h_mv.assign(2 * 16 * n, 0);
        h_ref.assign(2 * 16 * n, -1);
        h_slices.assign(slices, slices + pic->num_slices);
        h_pic = *pic;
        h_quant = *quant;
        seen.assign(n, 0);
        has_fpoc = false;                                        // a record covers one picture
        open = true;
        return H264R_OK;
    }

    // h264r_picture_field_pocs
    int field_pocs(const h264r_field_poc* rec)
    {
        if (!open) return H264R_ESTATE;
        if (!rec || !mbaff()) return H264R_EINVAL;
        h_fpoc = *rec;
        has_fpoc = true;
        return H264R_OK;
    }

    // h264r_mb_submit
    int submit(int addr, const h264r_mb* mb, const int16_t* levels, int n_levels, const uint32_t* mv, const int8_t* ref_idx)
    {
        if (!open) return H264R_ESTATE;
        const int n = pw * ph;
        if (addr < 0 || addr >= n || !mb || n_levels < 0 || (n_levels && !levels) || !mv || !ref_idx) return H264R_EINVAL;
        if (mb->slice >= h_pic.num_slices) return H264R_EINVAL;
        if (mb->mb_type == H264R_SI) return H264R_EUNSUPPORTED;        // see include/h264r.h
        // lossless inter MBs: the kernels take intra_chroma_pred_mode as DC, which is what the
        // parser leaves in an inter MB (macroblock_t::init, slice_data.cc:482)
        if ((mb->flags & H264R_MBF_BYPASS) && !(mb->flags & H264R_MBF_INTRA) && mb->chroma_mode != 0) return H264R_EINVAL;
        h264r_mb m = *mb;
        // append the level block, 16-byte aligned
        h_levels.resize((h_levels.size() + 7) & ~(size_t)7, 0);
        m.coef_off = (uint32_t)h_levels.size();
        if (n_levels) h_levels.insert(h_levels.end(), levels, levels + n_levels);
        h_mbs[addr] = m;
        const int W4 = pw * 4, plane = W4 * ph * 4, x = addr % pw, y = addr / pw;
        for (int l = 0; l < 2; ++l)
            for (int k = 0; k < 16; ++k) {
                int idx = (y * 4 + k / 4) * W4 + x * 4 + k % 4;
                h_mv[(size_t)l * plane + idx] = mv[l * 16 + k];
                h_ref[(size_t)l * plane + idx] = ref_idx[l * 16 + k];
            }
        seen[addr] = 1;
        return H264R_OK;
    }

    // What h264r_picture_end_async decides before it touches the device, on a context of chroma
    // format fmt with the DPB slots[H264R_MAX_SLOTS]; pads the level pool.  The stage is closed
    // afterwards, whatever the status.
    int finish(int fmt, int keep_slot, const StageSlot* slots)
    {
        if (!open) return H264R_ESTATE;
        open = false;
        for (uint8_t s : seen) if (!s) return H264R_ESTATE;      // every MB must be submitted
        if (keep_slot >= H264R_MAX_SLOTS) return H264R_EINVAL;
        n_submitted = h_levels.size();
        if (h_levels.empty()) h_levels.push_back(0);
        // 4:4:4: frame pictures only; a PCM MB's Cr view reads 128 entries past its block (run_444)
        if (fmt != 1 && h_pic.structure != H264R_FRAME) return H264R_EUNSUPPORTED;
        if (fmt != 1)                                          // SP slices are 4:2:0 only (Extended profile)
            for (const h264r_slice& sl : h_slices) if (sl.slice_type == H264R_SLICE_SP) return H264R_EUNSUPPORTED;
        if (fmt == 3) h_levels.insert(h_levels.end(), 128, 0);
        if (fmt == 0) h_levels.insert(h_levels.end(), 64, 0);     // the luma pass's chroma view of a PCM MB
        if (h_pic.structure < H264R_FRAME || h_pic.structure > H264R_MBAFF_FRAME) return H264R_EINVAL;
        if (mbaff()) {
            // MBAFF (include/h264r.h): 4:2:0, MB pairs, implicit weights only with the picture's field POCs
            // (k_mbaff_inter flags the same cases, and an SP slice's 8x8 transforms and QsC >= 6, on the
            // device: h264r_picture_wait)
            if (ph & 1) return H264R_EINVAL;
            for (const h264r_slice& sl : h_slices)
                if (sl.wp_mode == 2 && !has_fpoc) return H264R_EUNSUPPORTED;
            for (size_t a = 0; a < h_mbs.size(); a += 1) {
                const size_t top = ((a / pw) & ~(size_t)1) * pw + a % pw;
                if ((h_mbs[a].flags ^ h_mbs[top].flags) & H264R_MBF_FIELD) return H264R_EINVAL;   // one flag per pair
            }
            // a field MB's refIdx names field refIdx / 2 of the list
            for (size_t a = 0; a < h_mbs.size(); ++a) {
                const h264r_mb& m = h_mbs[a];
                if (m.flags & H264R_MBF_INTRA) continue;
                const int x = (int)(a % pw), y = (int)(a / pw), W4 = pw * 4, plane = W4 * ph * 4;
                const int nr = (m.flags & H264R_MBF_FIELD) ? 2 : 1;
                for (int l = 0; l < 2; ++l)
                    for (int k = 0; k < 16; ++k) {
                        const int r = h_ref[(size_t)l * plane + (y * 4 + k / 4) * W4 + x * 4 + k % 4];
                        if (r >= nr * h_slices[m.slice].num_ref[l]) return H264R_EINVAL;
                    }
            }
        } else if (fmt == 1)
            for (const h264r_mb& m : h_mbs) if (m.flags & H264R_MBF_FIELD) return H264R_EINVAL;
        // every referenced slot must be loaded, with a frame of this picture's size (a field
        // picture: twice its height; its entries may name either field of a slot, include/h264r.h)
        const int fld = field(), frame_h = ph << fld;
        for (const h264r_slice& sl : h_slices)
            for (int l = 0; l < 2; ++l)
                for (int i = 0; i < sl.num_ref[l]; ++i) {
                    const int ref = sl.ref_slot[l][i];
                    const int slot = fld ? ref & ~H264R_REF_BOTTOM : ref;
                    if (ref < 0 || slot >= H264R_MAX_SLOTS) return H264R_EINVAL;
                    if (!slots[slot].loaded || slots[slot].w != pw || slots[slot].h != frame_h) return H264R_ESTATE;
                }
        return H264R_OK;
    }
};

}  // namespace h264r
