"""What the built k_output_boxes kernels (arrow-h264_amd/csrc/k_output_boxes.hip: k_output_boxes_plan and one
k_output_boxes_<mode>_<filter> per RgbMode and filter) are made of, read from the library in the tree on the
CPU (tools/isa_dpp.py), as tests/test_isa_output_scale.py reads the k_output_rgb_scaled kernels.  The twelve
pixel kernels are held to those kernels' bars, although what is job-wide there -- the divisors, taps, T, the
region -- is read from a plan record per box here:

- No scratch and no spills, of VGPRs or of SGPRs: .sgpr_spill_count 0 in the code objects' metadata, and no
  v_readlane_b32 / v_writelane_b32 in the code.  No DPP.  Its only LDS is the 768-byte tile in which a
  workgroup's 8-bit results meet and the 26 words the threads that write a unit read: the scaled kernels'
  24 and the box's dst_x, dst_y.
- No v_ashr_pk_u8_i32 (tests/test_isa_output_rgb.py), and the conversion's v_mad_i32_i24.
- The binary16 path multiplies, then adds: nothing fused.
- global_ accesses only; 16-byte stores and 16-byte loads, 8-byte loads where SubWidthC is 2.

k_output_boxes_plan, one thread per box, has no LDS, no scratch, no spills, no DPP and global_ accesses
only.  Its 1 / d, 1 / (2 D) and 1 / (2 T) are correctly rounded binary32 divisions, which the compiler
expands with v_div_* and v_fma_f32; no pixel passes through it.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_dpp  # noqa: E402
from test_isa_output_scale import sgpr_spills  # noqa: E402

LIB = os.path.join(ROOT, "arrow-h264_amd", "lib", "libh264r.so")
PREFIX = "k_output_boxes_"
MODES = ("mono", "full", "gbr", "rep", "bil1", "bil2")
FILTERS = ("bilinear", "area")
KERNELS = [PREFIX + m + "_" + f for m in MODES for f in FILTERS]
PLAN = PREFIX + "plan"
LDS_BYTES = 768 + 4 * 26


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "libh264r.so not built (__graft_entry__.build())"
    return {"res": isa_dpp.kernel_resources(LIB), "sgpr_spills": sgpr_spills(LIB),
            "ops": {k: isa_dpp.opcode_histogram(LIB, k) for k in KERNELS + [PLAN]}}


def test_one_kernel_per_mode_and_filter_and_the_plan(lib):
    assert sorted(k for k in lib["res"] if k.startswith("k_output_boxes")) == sorted(KERNELS + [PLAN])


@pytest.mark.parametrize("kernel", KERNELS + [PLAN])
def test_no_scratch_no_spills_no_dpp(lib, kernel):
    res, ops = lib["res"][kernel], lib["ops"][kernel]
    print(kernel, res, "sgpr_spill_count", lib["sgpr_spills"][kernel])
    assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, res
    assert lib["sgpr_spills"][kernel] == 0
    assert not [o for o in ops if o.startswith(("v_readlane", "v_writelane"))]
    assert res["group_segment_fixed_size"] == (0 if kernel == PLAN else LDS_BYTES), res
    assert not [o for o in ops if o.startswith("scratch_") or "_dpp" in o]
    assert not [o for o in ops if o.startswith("flat_")]


@pytest.mark.parametrize("kernel", KERNELS)
def test_four_waves_per_simd(lib, kernel):
    assert lib["res"][kernel]["vgpr_count"] <= 128, lib["res"][kernel]


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_packed_shift_saturate(lib, kernel):
    ops = lib["ops"][kernel]
    assert not [o for o in ops if "ashr_pk" in o], "v_ashr_pk_u8_i32: see tests/test_isa_output_rgb.py"
    if "_gbr_" not in kernel:                               # GBR copies its samples: no matrix
        assert ops["v_mad_i32_i24"] > 0


@pytest.mark.parametrize("kernel", KERNELS)
def test_multiply_then_add(lib, kernel):
    ops = lib["ops"][kernel]
    fused = [o for o in ops if "fma" in o or "fmac" in o or "_mac_" in o or "mad_f" in o or "mad_mix" in o]
    assert not fused, fused
    assert ops["v_pk_mul_f32"] + ops["v_mul_f32_e32"] > 0 and ops["v_pk_add_f32"] + ops["v_add_f32_e32"] > 0


@pytest.mark.parametrize("kernel", KERNELS)
def test_global_accesses_and_wide_stores(lib, kernel):
    ops = lib["ops"][kernel]
    assert ops["global_store_dwordx4"] > 0
    assert ops["global_load_dwordx4"] > 0
    if any(m in kernel for m in ("_rep_", "_bil1_", "_bil2_")):
        assert ops["global_load_dwordx2"] > 0
