"""Register budget of k_inter4r with its two instantiations of the inter stages (csrc/k_recon.hip), read
from the library built in the tree (tools/isa_dpp.kernel_resources).

The plain instantiation (list 0 alone, default weights) lives in k_inter4r beside the generic one,
behind a wave-uniform branch; the kernel's allocation is the larger side's.  It must stay within 128
VGPRs (4 waves per SIMD: 512 per SIMD in blocks of 8) with nothing spilled and no scratch.  The
two-kernel form, whose k_inter4p fitted 96 VGPRs (91, 5 waves per SIMD), measured slower as a whole
(DESIGN.md section 7), so there is no k_inter4p to hold to 96.
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


def test_k_inter4r_within_128(res):
    r = res["k_inter4r"]
    print("k_inter4r", r)
    assert r["vgpr_count"] <= 128, r
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r

