// sync_words.h -- the sync region of one launch sequence (a whole batch, or one chunk of the
// overlapped schedule) as a named layout, shared by the host (h264r_host.hip) and the kernels
// that count in it.  Plain C++17, no HIP headers: tests/test_sync_words.py builds it alone.
//
// For P pictures of H MB rows, in ints:
//
//   [0]                 k_intra_pic's (band, picture) ticket counter
//   [1 .. 1 + P H)      the walk's progress word per (picture, MB row)
//   the fixed block, FIXED_WORDS ints:
//     spare (2)         no kernel touches them
//     level words (2)   LEVEL_DEEPEST: the deepest level k_level met (k_intra_levels stops there);
//                       the word before it is spare since the level barrier was sharded
//     spare (1)
//     luma tickets      the deblocking kernels' ticket set (k_deblock, k_deblock2, k_deblock2y):
//                       a counter per XCD, then the drain counter of xcd_drain_check
//     chroma tickets    the same for k_deblock2c, which runs beside k_deblock2y (the split walk)
//     level barrier     k_intra_levels' grid barrier: a counter per shard, then the top counter
//   pband[P]            per picture, the walk's bands holding an MB deeper than the level lists
//                       (k_level -> k_intra_pic)
//
// k_inter4r zeroes everything before pband at the head of every launch sequence (zeroed());
// k_level writes every pband word before k_intra_pic reads it.
#pragma once

#include <stddef.h>

namespace h264r {

constexpr int SYNC_XCDS = 8;                        // XCDs of a device at most: counters per ticket set, barrier shards
constexpr int TICKET_DRAIN = SYNC_XCDS;             // a ticket set: [0 .. SYNC_XCDS) per-XCD counters, then the drain counter
constexpr int TICKET_SET_WORDS = SYNC_XCDS + 1;
constexpr int BARRIER_TOP = SYNC_XCDS;              // the level barrier: [0 .. SYNC_XCDS) shard counters, then the top counter
constexpr int BARRIER_WORDS = SYNC_XCDS + 1;
constexpr int LEVEL_DEEPEST = 1;                    // the level words: [0] spare, [1] the deepest level
constexpr int LEVEL_WORDS = 2;

// the fixed block, each field behind the one before it
constexpr int FIXED_SPARE0 = 0;
constexpr int FIXED_LEVEL = FIXED_SPARE0 + 2;
constexpr int FIXED_SPARE1 = FIXED_LEVEL + LEVEL_WORDS;
constexpr int FIXED_TICKETS_Y = FIXED_SPARE1 + 1;
constexpr int FIXED_TICKETS_C = FIXED_TICKETS_Y + TICKET_SET_WORDS;
constexpr int FIXED_BARRIER = FIXED_TICKETS_C + TICKET_SET_WORDS;
constexpr int FIXED_WORDS = 32;
static_assert(FIXED_BARRIER + BARRIER_WORDS == FIXED_WORDS, "the fixed block's fields fill it exactly");
// the offsets the kernels were built and verified with: a field that moves is a new layout
static_assert(FIXED_LEVEL == 2 && FIXED_TICKETS_Y == 5 && FIXED_TICKETS_C == 14 && FIXED_BARRIER == 23, "fixed block layout");
static_assert(FIXED_SPARE0 < FIXED_LEVEL && FIXED_LEVEL + LEVEL_WORDS <= FIXED_SPARE1 && FIXED_SPARE1 < FIXED_TICKETS_Y &&
                  FIXED_TICKETS_Y + TICKET_SET_WORDS <= FIXED_TICKETS_C && FIXED_TICKETS_C + TICKET_SET_WORDS <= FIXED_BARRIER,
              "the fixed block's fields do not overlap");

// Offsets, in ints from the region's first word, for P pictures of H MB rows.
struct SyncWords {
    int P, H;
    static constexpr size_t intra_ticket() { return 0; }
    constexpr size_t progress(int pic) const { return 1 + (size_t)pic * H; }        // + the MB row
    constexpr size_t fixed() const { return 1 + (size_t)P * H; }
    constexpr size_t level() const { return fixed() + FIXED_LEVEL; }                 // LEVEL_WORDS
    constexpr size_t tickets_y() const { return fixed() + FIXED_TICKETS_Y; }         // TICKET_SET_WORDS
    constexpr size_t tickets_c() const { return fixed() + FIXED_TICKETS_C; }         // TICKET_SET_WORDS
    constexpr size_t barrier() const { return fixed() + FIXED_BARRIER; }             // BARRIER_WORDS
    constexpr size_t zeroed() const { return fixed() + FIXED_WORDS; }                // words [0, zeroed()): k_inter4r's
    constexpr size_t pband() const { return zeroed(); }                              // P words
    constexpr size_t total() const { return pband() + (size_t)P; }
};

}  // namespace h264r
