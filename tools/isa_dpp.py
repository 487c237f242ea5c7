#!/usr/bin/env python3
"""tools/isa_dpp.py -- the DPP instruction forms in libh264r.so's gfx950 code objects.

The kernels exchange values between lanes with DPP moves (device_common.h lane_xor1 /
lane_xor4 / lane_lo4 / lane_hi4 / quad_bcast), and the compiler may fold a DPP move into the
VOP2 instruction that consumes it (GCNDPPCombine: v_add_u32_dpp, v_and_b32_dpp, ...).  On MI355X
a reversed VOP2 opcode with DPP (v_subrev_u32_dpp, v_lshlrev_b32_dpp) applies the lane select to
src1 instead of src0 (tools/dpp/dpp_fold_test.hip); round 5's wrong residuals were the lane ^ 1
low / high moves folded into v_subrev_u32_dpp.  This tool lists every (mnemonic, DPP modifiers)
pair in the built library so that tests/test_isa.py can refuse reversed opcodes and hold the rest
to the verified set -- a toolchain or source change that produces a new form fails at build time
instead of waiting for a GPU parity run.  kernel_resources gives each kernel's register, spill, scratch
and LDS figures from the code objects' metadata notes (tests/test_isa.py holds k_inter4r to its
occupancy budget with them), opcode_histogram a kernel's mnemonic counts for before / after records
(profiles/r08_a_inter_stages_isa.txt).

    python tools/isa_dpp.py [path/to/libh264r.so]
"""
from __future__ import annotations

import collections
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READOBJ = "/opt/rocm/lib/llvm/bin/llvm-readobj"
RESOURCES = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(path: str, arch: str = "gfx950") -> list[bytes]:
    """The device code objects of every offload bundle embedded in a host ELF (the
    clang-offload-bundler layout: magic, entry count, then {offset, size, triple} per entry,
    offsets relative to the bundle start)."""
    data = open(path, "rb").read()
    out, pos = [], 0
    while True:
        i = data.find(MAGIC, pos)
        if i < 0:
            return out
        off = i + len(MAGIC)
        (n,) = struct.unpack_from("<Q", data, off)
        off += 8
        for _ in range(n):
            eo, es, ts = struct.unpack_from("<QQQ", data, off)
            off += 24
            triple = data[off:off + ts].decode()
            off += ts
            if arch in triple and es:
                out.append(data[i + eo:i + eo + es])
        pos = i + len(MAGIC)


def _instructions(path: str):
    """(kernel, instruction text) of every disassembled instruction, comments stripped."""
    with tempfile.TemporaryDirectory() as td:
        for k, co in enumerate(code_objects(path)):
            f = os.path.join(td, f"co{k}.o")
            open(f, "wb").write(co)
            asm = subprocess.run([OBJDUMP, "-d", "--mcpu=gfx950", f], check=True, capture_output=True,
                                 text=True).stdout
            kern = None
            for ln in asm.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\w+)>:", ln)
                if m:
                    kern = m.group(1)
                elif kern and ln.startswith("\t"):
                    yield kern, ln.split("//")[0].strip()


def dpp_forms(path: str) -> collections.Counter:
    """Counter of (kernel, mnemonic, modifiers) over every DPP instruction."""
    forms: collections.Counter = collections.Counter()
    for kern, ins in _instructions(path):
        if "_dpp" in ins:
            toks = ins.split()
            forms[(kern, toks[0], " ".join(t for t in toks[1:] if ":" in t))] += 1
    return forms


def opcode_histogram(path: str, kernel: str) -> collections.Counter:
    """Counter of mnemonics over one kernel's instructions."""
    return collections.Counter(ins.split()[0] for kern, ins in _instructions(path) if kern == kernel and ins)


def kernel_resources(path: str) -> dict[str, dict[str, int]]:
    """Per kernel, the RESOURCES entries of the code objects' metadata notes (amdhsa.kernels)."""
    out: dict[str, dict[str, int]] = {}
    with tempfile.TemporaryDirectory() as td:
        for k, co in enumerate(code_objects(path)):
            f = os.path.join(td, f"co{k}.o")
            open(f, "wb").write(co)
            notes = subprocess.run([READOBJ, "--notes", f], check=True, capture_output=True, text=True).stdout
            # one "  - .key: value" / "    .key: value" block per kernel; its .args entries sit deeper
            for block in re.split(r"^  - (?=\.)", notes, flags=re.M)[1:]:
                kv = dict(re.findall(r"^(?:    )?\.(\w+): +(\S+)$", block, flags=re.M))
                if "name" in kv:
                    out[kv["name"]] = {r: int(kv[r]) for r in RESOURCES}
    return out


def main() -> int:
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "arrow-h264_amd", "lib", "libh264r.so")
    for (kern, op, mods), n in sorted(dpp_forms(path).items()):
        print(f"{n:4d}  {kern:16s} {op:18s} {mods}")
    for kern, res in sorted(kernel_resources(path).items()):
        print(f"{kern:16s} " + " ".join(f"{r} {v}" for r, v in res.items()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
