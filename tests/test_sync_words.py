"""The sync region of a launch sequence (arrow-h264_amd/csrc/sync_words.h): a host-only program
that includes nothing but that header prints every field for a few (P, H); the fields must tile
the region without overlap, and every offset must be the one the kernels were verified with
(written here as numbers, from the host and kernel code before the header existed).  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arrow-h264_amd", "csrc")
SHAPES = [(1, 1), (1, 68), (3, 18), (252, 68)]

SRC = r'''
#include "sync_words.h"
#include <cstdio>
using namespace h264r;
static void field(const char* name, size_t off, size_t len) { printf("%s %zu %zu\n", name, off, len); }
int main()
{
    const int shapes[][2] = {%SHAPES%};
    printf("const xcds %d drain %d ticket_set %d barrier_top %d barrier_words %d deepest %d level_words %d fixed_words %d\n",
           SYNC_XCDS, TICKET_DRAIN, TICKET_SET_WORDS, BARRIER_TOP, BARRIER_WORDS, LEVEL_DEEPEST, LEVEL_WORDS, FIXED_WORDS);
    for (const auto& s : shapes) {
        const SyncWords w{s[0], s[1]};
        printf("shape %d %d\n", w.P, w.H);
        field("intra_ticket", SyncWords::intra_ticket(), 1);
        field("progress", w.progress(0), w.progress(w.P) - w.progress(0));
        field("progress_last_pic", w.progress(w.P - 1), (size_t)w.H);
        field("spare0", w.fixed() + FIXED_SPARE0, FIXED_LEVEL - FIXED_SPARE0);
        field("level", w.level(), LEVEL_WORDS);
        field("spare1", w.fixed() + FIXED_SPARE1, FIXED_TICKETS_Y - FIXED_SPARE1);
        field("tickets_y", w.tickets_y(), TICKET_SET_WORDS);
        field("tickets_c", w.tickets_c(), TICKET_SET_WORDS);
        field("barrier", w.barrier(), BARRIER_WORDS);
        field("pband", w.pband(), (size_t)w.P);
        field("zeroed", 0, w.zeroed());
        field("total", 0, w.total());
    }
    return 0;
}
'''

# the fields that make up the region; progress_last_pic, zeroed and total are views of it
TILES = ["intra_ticket", "progress", "spare0", "level", "spare1", "tickets_y", "tickets_c", "barrier", "pband"]
ZEROED = [t for t in TILES if t != "pband"]        # the ticket, the progress words and the fixed block


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    td = tmp_path_factory.mktemp("sync_words")
    src = td / "sync_words_print.cc"
    src.write_text(SRC.replace("%SHAPES%", ", ".join("{%d, %d}" % s for s in SHAPES)))
    exe = td / "sync_words_print"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    consts, shapes, cur = {}, {}, None
    for ln in out:
        t = ln.split()
        if t[0] == "const":
            consts = {t[i]: int(t[i + 1]) for i in range(1, len(t), 2)}
        elif t[0] == "shape":
            cur = shapes.setdefault((int(t[1]), int(t[2])), {})
        else:
            cur[t[0]] = (int(t[1]), int(t[2]))
    return consts, shapes


def test_named_constants(layout):
    consts, _ = layout
    # a ticket set is 8 per-XCD counters and the drain counter behind them (the kernels' sync + 8);
    # the level barrier 8 shard counters and the top counter (bar[8]); lvsync[1] is the deepest level
    assert consts == dict(xcds=8, drain=8, ticket_set=9, barrier_top=8, barrier_words=9, deepest=1, level_words=2,
                          fixed_words=32)


@pytest.mark.parametrize("P,H", SHAPES)
def test_fields_tile_the_region(layout, P, H):
    f = layout[1][(P, H)]
    spans = sorted(f[t] for t in TILES)
    assert all(n > 0 for _, n in spans)
    for (o0, n0), (o1, _) in zip(spans, spans[1:]):
        assert o0 + n0 <= o1, f"fields overlap at word {o1}"
    # no gaps either: the total is exactly the fields, 1 + P H + 32 + P words
    assert sum(n for _, n in spans) == f["total"][1] == 1 + P * H + 32 + P
    assert spans[0][0] == 0 and spans[-1][0] + spans[-1][1] == f["total"][1]
    # k_inter4r zeroes exactly the ticket, the progress words and the fixed block
    z = sorted(f[t] for t in ZEROED)
    assert z[0][0] == 0 and z[-1][0] + z[-1][1] == f["zeroed"][1] == sum(n for _, n in z)
    assert f["pband"][0] == f["zeroed"][1]


@pytest.mark.parametrize("P,H", SHAPES)
def test_offsets_are_the_verified_ones(layout, P, H):
    f = layout[1][(P, H)]
    assert f["intra_ticket"] == (0, 1)                              # sync[0]
    assert f["progress"] == (1, P * H)                              # sync + 1 + pic * H
    assert f["progress_last_pic"] == (1 + (P - 1) * H, H)
    assert f["level"] == (1 + P * H + 2, 2)                         # sync + 1 + P H + 2
    assert f["tickets_y"] == (1 + P * H + 5, 9)                     # + 5
    assert f["tickets_c"] == (1 + P * H + 5 + 9, 9)                 # dsync + 9
    assert f["barrier"] == (1 + P * H + 23, 9)                      # + 23, "9 ints"
    assert f["pband"] == (1 + P * H + 32, P)                        # + 32
    assert f["zeroed"] == (0, 1 + P * H + 32)                       # nz
    assert f["total"] == (0, 1 + P * H + 32 + P)                    # sync_ints() without the SP tag word
