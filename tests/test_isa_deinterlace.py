"""What the built k_deinterlace (arrow-h264_amd/csrc/k_deinterlace.hip) is made of, read from the library
in the tree on the CPU through tools/isa_dpp.py and nothing else, as tests/test_isa_output_resample.py reads
the resampling kernels.

- No scratch and no spills, of VGPRs (the metadata's vgpr_spill_count and private segment) or of SGPRs: no
  v_readlane_b32 / v_writelane_b32 (how hipcc keeps a spilled SGPR in a VGPR's lanes) and no scratch_
  instruction in the code.  No LDS.
- At most 128 VGPRs: four waves per SIMD at the least.
- The planes, the tables and the frames are reached with global_ accesses, never flat_; whole units arrive
  as 16-byte loads and leave as 16-byte stores.
- No DPP form outside the set tests/test_isa.py admits (the kernel uses none at all).
- The arithmetic the kernel's comment names: packed 16-bit pairs, v_perm_b32 to take rows apart, one v_sad_u8
  per pixel and direction.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_dpp  # noqa: E402

from test_isa import VERIFIED  # noqa: E402

LIB = os.path.join(ROOT, "arrow-h264_amd", "lib", "libh264r.so")
KERNEL = "k_deinterlace"


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "libh264r.so not built (__graft_entry__.build())"
    return {"res": isa_dpp.kernel_resources(LIB), "ops": isa_dpp.opcode_histogram(LIB, KERNEL),
            "dpp": [(op, mods) for (k, op, mods) in isa_dpp.dpp_forms(LIB) if k == KERNEL]}


def test_the_kernel_is_in_the_library(lib):
    assert KERNEL in lib["res"] and sum(lib["ops"].values()) > 0


def test_no_scratch_no_spills_no_lds(lib):
    res, ops = lib["res"][KERNEL], lib["ops"]
    print(KERNEL, res)
    assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, res
    assert not [o for o in ops if o.startswith(("v_readlane", "v_writelane", "scratch_"))]
    assert res["group_segment_fixed_size"] == 0, res
    assert not [o for o in ops if o.startswith("ds_")]


def test_at_most_128_vgprs(lib):
    assert lib["res"][KERNEL]["vgpr_count"] <= 128, lib["res"][KERNEL]


def test_global_accesses_and_wide_stores(lib):
    ops = lib["ops"]
    assert not [o for o in ops if o.startswith("flat_")]
    assert ops["global_store_dwordx4"] > 0
    assert ops["global_load_dwordx4"] > 0
    assert ops["global_atomic_or"] == 1                        # the refusal, and nothing else atomic
    assert not [o for o in ops if o.startswith(("buffer_", "global_atomic")) and o != "global_atomic_or"]


def test_no_dpp_form_outside_the_verified_set(lib):
    assert not [f for f in lib["dpp"] if f not in VERIFIED], lib["dpp"]
    assert not [o for o in lib["ops"] if "_dpp" in o]


def test_packed_arithmetic(lib):
    ops = lib["ops"]
    assert ops["v_sad_u8"] > 0 and ops["v_perm_b32"] > 0
    assert sum(n for o, n in ops.items() if o.startswith("v_pk_")) > ops["v_sad_u8"]
