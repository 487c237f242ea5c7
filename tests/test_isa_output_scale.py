"""What the built k_output_rgb_scaled kernels (arrow-h264_amd/csrc/k_output_scale.hip: one per RgbMode and
filter, k_output_rgb_scaled_<mode>_<filter>) are made of, read from the library in the tree on the CPU
(tools/isa_dpp.py), as tests/test_isa_output_rgb.py reads k_output_rgb.  Every kernel is held to all of it.

- No scratch and no spills, of VGPRs or of SGPRs: the code objects' metadata says .sgpr_spill_count 0,
  and no v_readlane_b32 / v_writelane_b32 (how hipcc keeps a spilled SGPR in a VGPR's lanes) is in the
  code.  No DPP.  Its only LDS is the 768-byte tile in which a workgroup's 8-bit results meet before they
  are written as units of 16 pixels, and the 24 words of the job that are read after the sums.
- No v_ashr_pk_u8_i32: the conversion is k_output_rgb's, clamp in front of the shift (see
  tests/test_isa_output_rgb.py for what MI355X does with that instruction).
- The binary16 path multiplies, then adds: nothing fused.  (The kernels' other binary32 operations
  are the first guesses of their integer quotients: a conversion and a multiplication.)
- The planes and the frames are reached with global_ accesses, never flat_; whole aligned units leave
  as 16-byte stores, whole source units arrive as 16- and 8-byte loads (4:0:0 has no 8-byte load:
  luma alone; 4:4:4 neither: its chroma is 16 bytes a unit).
"""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_dpp  # noqa: E402

LIB = os.path.join(ROOT, "arrow-h264_amd", "lib", "libh264r.so")
PREFIX = "k_output_rgb_scaled_"
MODES = ("mono", "full", "gbr", "rep", "bil1", "bil2")
FILTERS = ("bilinear", "area")
KERNELS = [PREFIX + m + "_" + f for m in MODES for f in FILTERS]


def sgpr_spills(path):
    """Per kernel, .sgpr_spill_count of the code objects' metadata notes (isa_dpp.kernel_resources has the
    VGPRs' alone)."""
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for k, co in enumerate(isa_dpp.code_objects(path)):
            f = os.path.join(td, f"co{k}.o")
            open(f, "wb").write(co)
            notes = subprocess.run([isa_dpp.READOBJ, "--notes", f], check=True, capture_output=True, text=True).stdout
            for block in re.split(r"^  - (?=\.)", notes, flags=re.M)[1:]:
                kv = dict(re.findall(r"^(?:    )?\.(\w+): +(\S+)$", block, flags=re.M))
                if "name" in kv:
                    out[kv["name"]] = int(kv["sgpr_spill_count"])
    return out


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "libh264r.so not built (__graft_entry__.build())"
    return {"res": isa_dpp.kernel_resources(LIB), "sgpr_spills": sgpr_spills(LIB),
            "ops": {k: isa_dpp.opcode_histogram(LIB, k) for k in KERNELS}}


def test_one_kernel_per_mode_and_filter(lib):
    assert sorted(k for k in lib["res"] if k.startswith("k_output_rgb_scaled")) == sorted(KERNELS)


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_no_spills_no_dpp(lib, kernel):
    res, ops = lib["res"][kernel], lib["ops"][kernel]
    print(kernel, res, "sgpr_spill_count", lib["sgpr_spills"][kernel])
    assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, res
    assert lib["sgpr_spills"][kernel] == 0
    assert not [o for o in ops if o.startswith(("v_readlane", "v_writelane"))]
    assert res["group_segment_fixed_size"] == 768 + 4 * 24, res
    assert not [o for o in ops if o.startswith("scratch_") or "_dpp" in o]


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
    assert not [o for o in ops if o.startswith("flat_")]
    assert ops["global_store_dwordx4"] > 0
    assert ops["global_load_dwordx4"] > 0
    if any(m in kernel for m in ("_rep_", "_bil1_", "_bil2_")):
        assert ops["global_load_dwordx2"] > 0
