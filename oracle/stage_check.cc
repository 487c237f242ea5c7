// stage_check.cc -- TEST INFRASTRUCTURE ONLY.
//
// What the streaming API accepts, checked without a device: drives PictureStage
// (arrow-h264_amd/csrc/picture_stage.h, the header alone) on the smallest pictures that can go wrong --
// 2 x 2 MBs (one MBAFF pair row), 1 x 1 where no pair is needed -- and compares every status, and the
// order in which the checks win, with what h264r_picture_begin / h264r_mb_submit /
// h264r_picture_end_async of include/h264r.h have returned since before the stage was a header.
// Exit status 0 when every check holds; each failure is printed.  tests/test_picture_stage.py runs it.
#include <cstdio>
#include <cstring>
#include <vector>

#include "picture_stage.h"

using namespace h264r;

static int failures = 0;
#define CHECK(what, got, want) do { const long long g_ = (got), w_ = (want); if (g_ != w_) { ++failures; \
        printf("FAIL %s:%d %s: got %lld, want %lld\n", __FILE__, __LINE__, what, g_, w_); } } while (0)

// One picture of one slice, every MB the same unless mb[] / ref0[] say otherwise.
struct Setup {
    int w = 2, h = 2, fmt = 1, keep = -1, structure = H264R_FRAME;
    h264r_slice sl{};
    std::vector<h264r_mb> mb;            // per MB
    std::vector<int> ref0;               // per MB: the refIdx of its 16 list-0 blocks (list 1: -1)
    std::vector<int> n_levels;           // per MB
    int skip = -1;                       // the MB that is never submitted
    bool fpoc = false;
    StageSlot slots[H264R_MAX_SLOTS];
    Setup(int w_ = 2, int h_ = 2) : w(w_), h(h_)
    {
        h264r_mb m{};
        m.mb_type = H264R_I_16x16; m.flags = H264R_MBF_INTRA;
        mb.assign((size_t)w * h, m);
        ref0.assign((size_t)w * h, -1);
        n_levels.assign((size_t)w * h, 0);
        sl.slice_type = H264R_SLICE_I;
    }
    // every MB an inter MB of a P slice with one reference, DPB slot 0 holding a frame of this size
    Setup& inter()
    {
        for (auto& m : mb) { m.mb_type = H264R_P_16x8; m.flags = 0; }
        ref0.assign(ref0.size(), 0);
        sl.slice_type = H264R_SLICE_P; sl.num_ref[0] = 1; sl.ref_slot[0][0] = 0;
        slots[0] = {true, w, h};
        return *this;
    }
};

static const int16_t LEVELS[64] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17};

static int begin(PictureStage& S, const Setup& u)
{
    h264r_pic pic{};
    pic.num_slices = 1; pic.structure = u.structure;
    h264r_quant q{};
    return S.begin(64, 64, u.w, u.h, &pic, &u.sl, &q, false);
}

static int submit(PictureStage& S, const Setup& u, int a)
{
    uint32_t mv[32] = {};
    int8_t ref[32];
    for (int k = 0; k < 32; ++k) ref[k] = (int8_t)(k < 16 ? u.ref0[a] : -1);
    return S.submit(a, &u.mb[a], LEVELS, u.n_levels[a], mv, ref);
}

// begin, every MB but u.skip, the field POCs, finish: the status of finish (the earlier ones must be OK)
static int run(PictureStage& S, const Setup& u)
{
    CHECK("begin", begin(S, u), H264R_OK);
    for (int a = 0; a < u.w * u.h; ++a)
        if (a != u.skip) CHECK("submit", submit(S, u, a), H264R_OK);
    if (u.fpoc) { h264r_field_poc r{}; CHECK("field_pocs", S.field_pocs(&r), H264R_OK); }
    return S.finish(u.fmt, u.keep, u.slots);
}

static void check_begin_and_submit()
{
    PictureStage S;
    Setup u;
    h264r_pic pic{};
    pic.num_slices = 1;
    h264r_quant q{};
    uint32_t mv[32] = {};
    int8_t ref[32];
    memset(ref, -1, sizeof ref);
    h264r_field_poc rec{};
    CHECK("submit before begin", S.submit(0, &u.mb[0], nullptr, 0, mv, ref), H264R_ESTATE);
    CHECK("field_pocs before begin", S.field_pocs(&rec), H264R_ESTATE);
    CHECK("finish before begin", S.finish(1, -1, u.slots), H264R_ESTATE);

    CHECK("begin w > max_w", S.begin(1, 2, 2, 2, &pic, &u.sl, &q, false), H264R_EINVAL);
    CHECK("begin h > max_h", S.begin(2, 1, 2, 2, &pic, &u.sl, &q, false), H264R_EINVAL);
    CHECK("begin w 0", S.begin(2, 2, 0, 2, &pic, &u.sl, &q, false), H264R_EINVAL);
    pic.num_slices = 0;
    CHECK("begin num_slices 0", S.begin(2, 2, 2, 2, &pic, &u.sl, &q, false), H264R_EINVAL);
    pic.num_slices = H264R_MAX_SLICES + 1;
    CHECK("begin num_slices > max", S.begin(2, 2, 2, 2, &pic, &u.sl, &q, false), H264R_EINVAL);
    CHECK("begin: a bad argument wins over a full ring", S.begin(2, 2, 2, 2, &pic, &u.sl, &q, true), H264R_EINVAL);
    pic.num_slices = 1;
    CHECK("begin null pic", S.begin(2, 2, 2, 2, nullptr, &u.sl, &q, false), H264R_EINVAL);
    CHECK("begin null slices", S.begin(2, 2, 2, 2, &pic, nullptr, &q, false), H264R_EINVAL);
    CHECK("begin null quant", S.begin(2, 2, 2, 2, &pic, &u.sl, nullptr, false), H264R_EINVAL);
    CHECK("begin with a full ring", S.begin(2, 2, 2, 2, &pic, &u.sl, &q, true), H264R_ESTATE);
    CHECK("a refused begin opens nothing", S.submit(0, &u.mb[0], nullptr, 0, mv, ref), H264R_ESTATE);

    CHECK("begin", S.begin(2, 2, 2, 2, &pic, &u.sl, &q, false), H264R_OK);
    CHECK("field_pocs off MBAFF", S.field_pocs(&rec), H264R_EINVAL);
    CHECK("submit addr -1", S.submit(-1, &u.mb[0], nullptr, 0, mv, ref), H264R_EINVAL);
    CHECK("submit addr w*h", S.submit(4, &u.mb[0], nullptr, 0, mv, ref), H264R_EINVAL);
    CHECK("submit null record", S.submit(0, nullptr, nullptr, 0, mv, ref), H264R_EINVAL);
    CHECK("submit null levels", S.submit(0, &u.mb[0], nullptr, 3, mv, ref), H264R_EINVAL);
    CHECK("submit n_levels -1", S.submit(0, &u.mb[0], LEVELS, -1, mv, ref), H264R_EINVAL);
    CHECK("submit null mv", S.submit(0, &u.mb[0], nullptr, 0, nullptr, ref), H264R_EINVAL);
    CHECK("submit null ref_idx", S.submit(0, &u.mb[0], nullptr, 0, mv, nullptr), H264R_EINVAL);
    h264r_mb m = u.mb[0];
    m.slice = 1;
    CHECK("submit slice >= num_slices", S.submit(0, &m, nullptr, 0, mv, ref), H264R_EINVAL);
    m = u.mb[0];
    m.mb_type = H264R_SI;
    CHECK("submit SI", S.submit(0, &m, nullptr, 0, mv, ref), H264R_EUNSUPPORTED);
    m.slice = 1;
    CHECK("submit: the slice index wins over SI", S.submit(0, &m, nullptr, 0, mv, ref), H264R_EINVAL);
    m = h264r_mb{};
    m.mb_type = H264R_P_16x8; m.flags = H264R_MBF_BYPASS; m.chroma_mode = 1;
    CHECK("submit lossless inter, chroma_mode 1", S.submit(0, &m, nullptr, 0, mv, ref), H264R_EINVAL);
    m.chroma_mode = 0;
    CHECK("submit lossless inter, chroma_mode 0", S.submit(0, &m, nullptr, 0, mv, ref), H264R_OK);
    m.flags |= H264R_MBF_INTRA; m.chroma_mode = 1;
    CHECK("submit lossless intra, chroma_mode 1", S.submit(0, &m, nullptr, 0, mv, ref), H264R_OK);
    CHECK("the refused MBs were not staged", S.seen[1] + S.seen[2] + S.seen[3], 0);
}

static void check_finish()
{
    PictureStage S;
    {
        Setup u;
        u.skip = 3;
        CHECK("one MB missing", run(S, u), H264R_ESTATE);
        CHECK("closed after a refusal", S.finish(1, -1, u.slots), H264R_ESTATE);
        CHECK("closed: submit", submit(S, u, 3), H264R_ESTATE);
        u.keep = H264R_MAX_SLOTS;
        CHECK("the missing MB wins over keep_slot", run(S, u), H264R_ESTATE);
        u.skip = -1;
        CHECK("keep_slot == MAX_SLOTS", run(S, u), H264R_EINVAL);
        u.keep = H264R_MAX_SLOTS - 1;
        CHECK("keep_slot == MAX_SLOTS - 1", run(S, u), H264R_OK);
        CHECK("closed after success", S.finish(1, -1, u.slots), H264R_ESTATE);
    }
    for (int w = 1; w <= 2; ++w) {
        Setup u(w, w);
        CHECK("an intra frame", run(S, u), H264R_OK);
        for (int fmt : {0, 2, 3}) { u.fmt = fmt; CHECK("an intra frame off 4:2:0", run(S, u), H264R_OK); }
    }
    for (int st : {H264R_TOP_FIELD, H264R_BOTTOM_FIELD, H264R_MBAFF_FRAME})
        for (int fmt : {0, 2, 3}) {
            Setup u;
            u.structure = st; u.fmt = fmt;
            CHECK("no frame off 4:2:0", run(S, u), H264R_EUNSUPPORTED);
        }
    for (int fmt : {0, 2, 3}) {
        Setup u;
        u.fmt = fmt; u.sl.slice_type = H264R_SLICE_SP;
        CHECK("an SP slice off 4:2:0", run(S, u), H264R_EUNSUPPORTED);
        u.fmt = 1;
        CHECK("an SP slice on 4:2:0", run(S, u), H264R_OK);
    }
    // include/h264r.h: H264R_FRAME is structure 0; what lies outside FRAME .. MBAFF_FRAME is refused
    for (int st : {-1, 4, 5}) {
        Setup u;
        u.structure = st;
        CHECK("a structure out of range", run(S, u), H264R_EINVAL);
        u.fmt = 3;
        CHECK("off 4:2:0 it is no frame first", run(S, u), H264R_EUNSUPPORTED);
    }
    {
        Setup u;
        u.structure = H264R_TOP_FIELD;
        CHECK("an intra field", run(S, u), H264R_OK);
        u.structure = H264R_FRAME; u.mb[2].flags |= H264R_MBF_FIELD;
        CHECK("FIELD flag outside MBAFF, 4:2:0", run(S, u), H264R_EINVAL);
    }
}

static void check_mbaff()
{
    PictureStage S;
    {
        Setup u(1, 1);
        u.structure = H264R_MBAFF_FRAME;
        CHECK("MBAFF, odd height", run(S, u), H264R_EINVAL);
        Setup v(2, 3);
        v.structure = H264R_MBAFF_FRAME;
        CHECK("MBAFF, odd height", run(S, v), H264R_EINVAL);
    }
    {
        Setup u;
        u.structure = H264R_MBAFF_FRAME;
        CHECK("MBAFF intra", run(S, u), H264R_OK);
        u.sl.wp_mode = 2;
        CHECK("implicit weights without field POCs", run(S, u), H264R_EUNSUPPORTED);
        u.fpoc = true;
        CHECK("implicit weights with field POCs", run(S, u), H264R_OK);
        u.fpoc = false;
        CHECK("the record covers one picture", run(S, u), H264R_EUNSUPPORTED);
        u.h = 1; u.w = 4;
        CHECK("odd height wins over the weights", run(S, u), H264R_EINVAL);
    }
    for (int a = 0; a < 4; ++a) {
        Setup u;
        u.structure = H264R_MBAFF_FRAME;
        u.mb[a].flags |= H264R_MBF_FIELD;
        CHECK("a pair with one FIELD flag", run(S, u), H264R_EINVAL);
        u.mb[a ^ 2].flags |= H264R_MBF_FIELD;                    // the other MB of the pair (2 x 2: rows 0, 1)
        CHECK("a field pair", run(S, u), H264R_OK);
    }
    for (int num_ref : {1, 2}) {
        Setup u;
        u.inter().structure = H264R_MBAFF_FRAME;
        u.sl.num_ref[0] = (uint8_t)num_ref; u.sl.ref_slot[0][1] = 0;
        CHECK("MBAFF inter", run(S, u), H264R_OK);
        u.ref0[1] = num_ref - 1;
        CHECK("frame MB refIdx num_ref - 1", run(S, u), H264R_OK);
        u.ref0[1] = num_ref;
        CHECK("frame MB refIdx num_ref", run(S, u), H264R_EINVAL);
        u.mb[1].flags |= H264R_MBF_FIELD; u.mb[3].flags |= H264R_MBF_FIELD;
        u.ref0[1] = 2 * num_ref - 1;
        CHECK("field MB refIdx 2 num_ref - 1", run(S, u), H264R_OK);
        u.ref0[3] = 2 * num_ref;
        CHECK("field MB refIdx 2 num_ref", run(S, u), H264R_EINVAL);
        u.mb[3].flags |= H264R_MBF_INTRA;
        CHECK("an intra MB's refIdx is not looked at", run(S, u), H264R_OK);
    }
}

static void check_ref_slots()
{
    PictureStage S;
    {
        Setup u;
        u.inter();
        CHECK("a loaded slot", run(S, u), H264R_OK);
        u.sl.ref_slot[0][0] = -1;
        CHECK("slot -1", run(S, u), H264R_EINVAL);
        u.sl.ref_slot[0][0] = H264R_MAX_SLOTS;
        CHECK("slot MAX_SLOTS", run(S, u), H264R_EINVAL);
        u.sl.ref_slot[0][0] = H264R_REF_BOTTOM;
        CHECK("a frame names no field of a slot", run(S, u), H264R_EINVAL);
        u.sl.ref_slot[0][0] = H264R_MAX_SLOTS - 1;
        CHECK("slot not loaded", run(S, u), H264R_ESTATE);
        u.slots[H264R_MAX_SLOTS - 1] = {true, 2, 4};
        CHECK("slot of another height", run(S, u), H264R_ESTATE);
        u.slots[H264R_MAX_SLOTS - 1] = {true, 4, 2};
        CHECK("slot of another width", run(S, u), H264R_ESTATE);
        u.slots[H264R_MAX_SLOTS - 1] = {true, 2, 2};
        CHECK("slot of this size", run(S, u), H264R_OK);
        // list 1 is checked as list 0 is, and only as far as num_ref goes
        u.sl.ref_slot[1][0] = 5;
        CHECK("an entry beyond num_ref", run(S, u), H264R_OK);
        u.sl.num_ref[1] = 1;
        CHECK("list 1, slot not loaded", run(S, u), H264R_ESTATE);
        u.sl.ref_slot[0][0] = -1;
        CHECK("list 0 is looked at first", run(S, u), H264R_EINVAL);
    }
    for (int st : {H264R_TOP_FIELD, H264R_BOTTOM_FIELD}) {
        Setup u;
        u.inter().structure = st;
        CHECK("a field needs a frame of twice its height", run(S, u), H264R_ESTATE);
        u.slots[0] = {true, 2, 4};
        CHECK("a field over a frame", run(S, u), H264R_OK);
        u.sl.ref_slot[0][0] = 3 | H264R_REF_BOTTOM;
        CHECK("the bottom field of a slot not loaded", run(S, u), H264R_ESTATE);
        u.slots[3] = {true, 2, 4};
        CHECK("the bottom field of a slot", run(S, u), H264R_OK);
        u.sl.ref_slot[0][0] = H264R_MAX_SLOTS | H264R_REF_BOTTOM;
        CHECK("the bottom field of slot MAX_SLOTS", run(S, u), H264R_EINVAL);
    }
    {
        // the checks that need no slot win over the slots
        Setup u;
        u.inter().mb[0].flags |= H264R_MBF_FIELD;
        u.slots[0] = StageSlot{};
        CHECK("the FIELD flag wins over a missing slot", run(S, u), H264R_EINVAL);
    }
}

static void check_level_pool()
{
    PictureStage S;
    const int n_levels[4] = {3, 16, 0, 5};
    const uint32_t off[4] = {0, 8, 24, 24};
    for (int fmt = 0; fmt < 4; ++fmt) {
        const size_t pad = fmt == 3 ? 128 : fmt == 0 ? 64 : 0;
        Setup u;
        u.fmt = fmt;
        CHECK("no levels", run(S, u), H264R_OK);
        CHECK("no levels: nothing submitted", S.n_submitted, 0);
        CHECK("no levels: one entry and the format's padding", S.h_levels.size(), 1 + pad);
        u.n_levels.assign(n_levels, n_levels + 4);
        CHECK("levels", run(S, u), H264R_OK);
        for (int a = 0; a < 4; ++a) {
            CHECK("coef_off is a multiple of 8", S.h_mbs[a].coef_off % 8, 0);
            CHECK("coef_off", S.h_mbs[a].coef_off, off[a]);
            CHECK("the block is the MB's levels", memcmp(&S.h_levels[off[a]], LEVELS, 2 * n_levels[a]), 0);
        }
        CHECK("levels: as submitted", S.n_submitted, 29);
        CHECK("levels: the format's padding", S.h_levels.size(), 29 + pad);
        for (size_t k = 29; k < S.h_levels.size(); ++k) CHECK("the padding is zero", S.h_levels[k], 0);
        CHECK("the gap before an aligned block is zero", S.h_levels[3] | S.h_levels[7], 0);
    }
    // the motion of MB (x, y) lands in rows 4 y .. 4 y + 3 of the [list][4 H][4 W] arrays
    Setup u;
    u.inter().ref0[3] = 0;
    CHECK("inter", run(S, u), H264R_OK);
    CHECK("ref_idx arrays", S.h_ref.size(), 2 * 16 * 4);
    CHECK("list 0 of MB 3", S.h_ref[(4 + 3) * 8 + 4 + 3], 0);
    CHECK("list 1 of MB 3", S.h_ref[64 + (4 + 3) * 8 + 4 + 3], -1);
    // a smaller picture after a larger one keeps nothing of it
    Setup v(1, 1);
    CHECK("1 x 1", run(S, v), H264R_OK);
    CHECK("1 x 1: records", S.h_mbs.size(), 1);
    CHECK("1 x 1: motion", S.h_mv.size(), 32);
}

static void check_quant_and_strings()
{
    h264r_quant flat, lists;
    memset(&flat, 0, sizeof flat);
    memset(&lists, 1, sizeof lists);
    int32_t m16[64];
    for (int& v : m16) v = 16;
    const int32_t* qm[12];
    for (auto& p : qm) p = m16;
    CHECK("quant_init_flat", quant_init_flat(&flat), H264R_OK);
    CHECK("quant_init_lists", quant_init_lists(&lists, qm), H264R_OK);
    CHECK("flat lists give the flat tables", memcmp(&flat, &lists, sizeof flat), 0);
    CHECK("LevelScale4x4(0, 0, 0) x 16", flat.scale4x4[0][0][0][0], 160);
    CHECK("LevelScale4x4(5, 1, 1) x 16", flat.scale4x4[1][2][5][5], 29 * 16);
    CHECK("LevelScale8x8(0, 0, 0) x 16", flat.scale8x8[0][0][0][0], 320);
    CHECK("quant_init_flat(NULL)", quant_init_flat(nullptr), H264R_EINVAL);
    CHECK("quant_init_lists(NULL lists)", quant_init_lists(&lists, nullptr), H264R_EINVAL);
    qm[11] = nullptr;
    CHECK("quant_init_lists(a NULL list)", quant_init_lists(&lists, qm), H264R_EINVAL);
    for (int s = H264R_ENODEVICE; s <= H264R_OK; ++s)
        CHECK("a status has its own string", strcmp(status_string(s), status_string(1)) != 0, 1);
    CHECK("ok", strcmp(status_string(H264R_OK), "ok"), 0);
}

int main()
{
    check_begin_and_submit();
    check_finish();
    check_mbaff();
    check_ref_slots();
    check_level_pool();
    check_quant_and_strings();
    if (failures) printf("stage_check: %d checks failed\n", failures);
    else printf("stage_check: ok\n");
    return failures ? 1 : 0;
}
