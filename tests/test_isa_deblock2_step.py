"""k_deblock2's step (csrc/k_deblock2.hip, csrc/mb_deblock2.h H264R_DB2_STEP), read from the library built
in the tree with tools/isa_dpp (the manner of test_isa_inter_waves5).

The band walk's occupancy is set by LDS: 8 waves per CU leave each 163840 / 8 = 20480 bytes, 2 waves per
SIMD 256 VGPRs.  The split walk's builds ask for 3 (k_deblock2y: 168 VGPRs, 512 / 3 in blocks of 8) and 4
(k_deblock2c: 128) waves per SIMD.  None of them may spill: a step is its instruction stream.  With the
halves of a dword written by their owner the horizontal pass needs no partner move, so k_deblock2 has
fewer DPP moves than the 28 (19 luma + 9 chroma rows) it had before.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_dpp  # noqa: E402

LIB = os.path.join(ROOT, "arrow-h264_amd", "lib", "libh264r.so")
VGPRS = {"k_deblock2": 256, "k_deblock2y": 168, "k_deblock2c": 128}
DPP_BEFORE = 28


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.skip("libh264r.so not built (__graft_entry__.build())")
    return LIB


@pytest.mark.parametrize("kernel", list(VGPRS))
def test_no_scratch_within_budget(lib, kernel):
    r = isa_dpp.kernel_resources(lib)[kernel]
    print(kernel, r)
    assert r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_spill_count"] == 0, r
    assert r["vgpr_count"] <= VGPRS[kernel], r


def test_k_deblock2_lds(lib):
    r = isa_dpp.kernel_resources(lib)["k_deblock2"]
    assert r["group_segment_fixed_size"] <= 20480, r


def test_k_deblock2_fewer_dpp_moves(lib):
    n = sum(c for (kern, _, _), c in isa_dpp.dpp_forms(lib).items() if kern == "k_deblock2")
    print("k_deblock2 DPP instructions", n)
    assert n < DPP_BEFORE, n
