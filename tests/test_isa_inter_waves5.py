"""k_inter4r at 5 waves per SIMD (csrc/k_recon.hip H264R_INTER_WAVES), read from the library built in
the tree with the helper of test_isa_inter_plain (tools/isa_dpp.kernel_resources).

5 waves per SIMD is 96 VGPRs at most (512 per SIMD in blocks of 8).  The generic instantiation of the
inter stages fits them because it parks state in LDS across the motion compensation (csrc/mb_inter4.h
Inter4Park) -- not because the compiler spills: round 6 measured a spilling 5-wave kernel a third
slower.  5 workgroups per CU leave each 163840 / 5 = 32768 bytes of LDS.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_dpp  # noqa: E402

LIB = os.path.join(ROOT, "arrow-h264_amd", "lib", "libh264r.so")


@pytest.fixture(scope="module")
def res():
    if not os.path.exists(LIB):
        pytest.skip("libh264r.so not built (__graft_entry__.build())")
    return isa_dpp.kernel_resources(LIB)


def test_k_inter4r_five_waves(res):
    r = res["k_inter4r"]
    print("k_inter4r", r)
    assert r["vgpr_count"] <= 96, r
    assert r["vgpr_spill_count"] == 0, r
    assert r["private_segment_fixed_size"] == 0, r
    assert r["group_segment_fixed_size"] <= 32768, r
