"""What the built k_output_rgb (arrow-h264_amd/csrc/k_output.hip) is made of, read from the library
in the tree on the CPU (tools/isa_dpp.py), as tests/test_isa.py reads k_inter4r.

- Registers only: no LDS, no scratch, no spills, no DPP (include/h264r_output.h needs none of them).
- The binary16 path multiplies, then adds: a fused multiply-add would round once where the header's
  definition rounds twice.
- Whole aligned units leave as 16-byte stores; the colour bytes are interleaved with v_perm_b32.
- No v_ashr_pk_u8_i32.  hipcc fuses `clip255(a >> 17)` of two neighbouring pixels into that gfx950
  instruction and ORs the next pair in above it, taking the upper half of its result for zero.  MI355X
  leaves that half of the destination register as it was (tools/ashr_pk_probe.hip,
  profiles/ashr_pk_probe.txt: 0xdeadbeef becomes 0xdeadff64), so a kernel built that way returned
  wrong bytes from the third pixel of four on.  k_output_rgb clamps in front of the shift
  (rgb_clip255_sh17), which keeps the instruction out; this test fails if it comes back.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_dpp  # noqa: E402

LIB = os.path.join(ROOT, "arrow-h264_amd", "lib", "libh264r.so")
KERNEL = "k_output_rgb"


@pytest.fixture(scope="module")
def ops():
    assert os.path.exists(LIB), "libh264r.so not built (__graft_entry__.build())"
    return isa_dpp.opcode_histogram(LIB, KERNEL)


def test_registers_only(ops):
    res = isa_dpp.kernel_resources(LIB)[KERNEL]
    print(KERNEL, res)
    assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, res
    assert res["group_segment_fixed_size"] == 0, res
    assert res["vgpr_count"] <= 168, res                         # three waves per SIMD
    assert not [o for o in ops if o.startswith(("ds_", "scratch_")) or "_dpp" in o]


def test_multiply_then_add(ops):
    fused = [o for o in ops if "fma" in o or "fmac" in o or "_mac_" in o or "mad_f" in o or "mad_mix" in o]
    assert not fused, fused
    assert ops["v_pk_mul_f32"] + ops["v_mul_f32_e32"] > 0 and ops["v_pk_add_f32"] + ops["v_add_f32_e32"] > 0


def test_wide_stores_and_register_interleave(ops):
    assert ops["global_store_dwordx4"] > 0 and ops["v_perm_b32"] > 0
    assert ops["global_load_dwordx4"] > 0 and ops["global_load_dwordx2"] > 0
    assert not [o for o in ops if o.startswith("flat_")]


def test_no_packed_shift_saturate(ops):
    assert not [o for o in ops if "ashr_pk" in o], "v_ashr_pk_u8_i32 is back: see this file's docstring"
