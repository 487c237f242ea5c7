"""What the built k_output_rgb_resampled kernels (arrow-h264_amd/csrc/k_output_resample.hip: one per
RgbMode, k_output_rgb_resampled_<mode>) are made of, read from the library in the tree on the CPU
(tools/isa_dpp.py), as tests/test_isa_output_rgb.py reads k_output_rgb.  Every kernel is held to all of it.

- No scratch and no spills, of VGPRs or of SGPRs: .sgpr_spill_count 0 in the code objects' metadata, and no
  v_readlane_b32 / v_writelane_b32 (how hipcc keeps a spilled SGPR in a VGPR's lanes) in the code.  Its LDS
  is dynamic, sized by the plan: no static LDS.
- No DPP form outside the set tests/test_isa.py admits (the kernels use none at all).
- No v_ashr_pk_u8_i32: clip8(acc >> 22) of neighbouring pixels is the pattern hipcc fuses into it, and both
  passes clamp in front of the shift (see tests/test_isa_output_rgb.py for what MI355X does with that
  instruction).  The taps are v_mad_i32_i24.
- The binary16 path multiplies, then adds: nothing fused.
- The planes, the tables and the frames are reached with global_ accesses, never flat_; whole aligned rows
  of a tile leave as 16-byte stores, whole source units arrive as 16-byte loads, and the converted units go
  to the strip as 16-byte LDS stores.
- At most 128 VGPRs: four waves per SIMD at the least.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_dpp  # noqa: E402

from test_isa_output_scale import sgpr_spills  # noqa: E402

LIB = os.path.join(ROOT, "arrow-h264_amd", "lib", "libh264r.so")
PREFIX = "k_output_rgb_resampled_"
MODES = ("mono", "full", "gbr", "rep", "bil1", "bil2")
KERNELS = [PREFIX + m for m in MODES]


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "libh264r.so not built (__graft_entry__.build())"
    return {"res": isa_dpp.kernel_resources(LIB), "sgpr_spills": sgpr_spills(LIB),
            "ops": {k: isa_dpp.opcode_histogram(LIB, k) for k in KERNELS}}


def test_one_kernel_per_mode(lib):
    assert sorted(k for k in lib["res"] if k.startswith(PREFIX)) == sorted(KERNELS)


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_no_spills_no_dpp(lib, kernel):
    res, ops = lib["res"][kernel], lib["ops"][kernel]
    print(kernel, res, "sgpr_spill_count", lib["sgpr_spills"][kernel])
    assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, res
    assert lib["sgpr_spills"][kernel] == 0
    assert not [o for o in ops if o.startswith(("v_readlane", "v_writelane"))]
    assert res["group_segment_fixed_size"] == 0, res
    assert res["vgpr_count"] <= 128, res
    assert not [o for o in ops if o.startswith("scratch_") or "_dpp" in o]


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_packed_shift_saturate(lib, kernel):
    ops = lib["ops"][kernel]
    assert not [o for o in ops if "ashr_pk" in o], "v_ashr_pk_u8_i32: see tests/test_isa_output_rgb.py"
    assert ops["v_mad_i32_i24"] >= 6                            # three channels in each pass, the matrix apart


@pytest.mark.parametrize("kernel", KERNELS)
def test_multiply_then_add(lib, kernel):
    ops = lib["ops"][kernel]
    fused = [o for o in ops if "fma" in o or "fmac" in o or "_mac_" in o or "mad_f" in o or "mad_mix" in o]
    assert not fused, fused
    assert ops["v_pk_mul_f32"] + ops["v_mul_f32_e32"] > 0 and ops["v_pk_add_f32"] + ops["v_add_f32_e32"] > 0


@pytest.mark.parametrize("kernel", KERNELS)
def test_global_accesses_and_wide_stores(lib, kernel):
    ops = lib["ops"][kernel]
    assert not [o for o in ops if o.startswith("flat_")]
    assert ops["global_store_dwordx4"] > 0
    assert ops["global_load_dwordx4"] > 0
    assert ops["ds_write_b128"] > 0
    if any(kernel.endswith(m) for m in ("_rep", "_bil1", "_bil2")):
        assert ops["global_load_dwordx2"] > 0
