#!/usr/bin/env python3
"""Generate tests/golden/mbaff_ext.json from the compiled REFERENCE decoder: lossless
(TransformBypassModeFlag) MBs and SP slices in MBAFF frames.

Run where the reference sources are (the GPU box never has them):

    python tests/golden/make_mbaff_ext.py

The CPU oracle refuses these two combinations (oracle/h264r_oracle.c decode_mb), so unlike
tests/golden/make_golden.py there is no restatement to cross-check: the fixtures pin the library
directly to the unmodified reference (oracle/_ref/ref_driver, built from the reference sources by
oracle/Makefile).  In its place the script runs the reference TWICE per case and stage and refuses
to write a fixture whose two runs differ, so that a read of undefined state in the reference is
not pinned, and it asserts that every case holds the MBs it is there for (coverage() below, which
tests/test_mbaff_ext.py repeats on the committed fixtures).

Each entry has the fields of a golden.json fixture: the synth configuration and picture index
(inputs are regenerated), an MD5 of the generated input arrays, and per-plane MD5s of the
reconstruction before deblocking and of the output.  MD5s and configurations only, no samples.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import _oracle as O  # noqa: E402
from h264r import _abi as A  # noqa: E402
from h264r import synth  # noqa: E402

# name, SURVEY config index, W, H, overrides (structure = H264R_MBAFF_FRAME is added), picture indices.
# The smallest shapes at which each rule can go wrong: QCIF (11 x 8: 4 pair rows), CIF for slices.
CASES = [
    # lossless: DPCM by the block's prediction mode in frame and field pairs, intra (4x4 / 8x8 / 16x16,
    # chroma) and inter MBs (which read the ipred nibbles), PCM beside it, CIP, 8x8 blocks, B with weights
    ("imbaff_qcif_lossless", 2, 11, 8, dict(qp_min=0, qp_max=20, lossless_permille=450, pcm_permille=20), [0, 1]),
    # qp_min = 0: the generator refuses qp_min (default 20) > qp_max
    ("imbaff_qcif_lossless_4x4_cip", 2, 11, 8, dict(transform8x8=0, constrained_intra=1, lossless_permille=400,
                                                    qp_min=0, qp_max=10), [0]),
    ("pmbaff_qcif_lossless_t8", 3, 11, 8, dict(lossless_permille=450, transform8x8=1, intra_permille=300,
                                               num_refs=3, qp_max=30), [0, 1]),
    ("bmbaff_cif_lossless_explicit_3slices_idc2", 4, 22, 18, dict(wp_mode=1, lossless_permille=500, num_slices=3,
                                                                  deblock_idc=2, qp_max=20), [0]),
    # SP slices (inverse_transform_sp transform.cc:1267-1300): both sp_for_switch_flag values and
    # several QsY over the indices, as p_qcif_sp has them for frames; slices + CIP; the QP range, offsets
    ("pmbaff_qcif_sp", 3, 11, 8, dict(sp_slices=1, num_refs=2), [0, 1, 2]),
    ("pmbaff_cif_sp_3slices_cip", 3, 22, 18, dict(sp_slices=1, num_slices=3, deblock_idc=2, intra_permille=250,
                                                  constrained_intra=1), [0]),
    ("pmbaff_qcif_sp_qp0_51_offsets", 3, 11, 8, dict(sp_slices=1, qp_min=0, qp_max=51, num_refs=3,
                                                     filter_offset_a=6, filter_offset_b=-6), [0]),
]


def md5(a: np.ndarray) -> str:
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def coverage(p: synth.Picture) -> list[str]:
    """What a fixture picture must hold and does not (empty = covered), counted from the synth
    arrays: a lossless case bypass MBs, intra and (P / B) inter, in a field pair AND in a frame
    pair; an SP case an inter MB with cbp != 0 in a field pair and one in a frame pair, and an
    intra MB."""
    cfg, m = p.cfg, p.mbs
    intra = (m["flags"] & A.MBF_INTRA) != 0
    byp = (m["flags"] & A.MBF_BYPASS) != 0
    missing = []
    for what, fld in (("field", (m["flags"] & A.MBF_FIELD) != 0), ("frame", (m["flags"] & A.MBF_FIELD) == 0)):
        if cfg.lossless_permille:
            if not (byp & fld).any():
                missing.append(f"bypass MB in a {what} pair")
            if not (byp & intra & fld).any():
                missing.append(f"intra bypass MB in a {what} pair")
            if cfg.kind != A.SYNTH_INTRA and not (byp & ~intra & fld).any():
                missing.append(f"inter bypass MB in a {what} pair")
        if cfg.sp_slices:
            if not (~intra & (m["cbp"] != 0) & fld).any():
                missing.append(f"inter MB with cbp != 0 in a {what} pair")
    if cfg.sp_slices:
        if not intra.any():
            missing.append("intra MB")
        if not (p.slices["slice_type"] == A.SLICE_SP).all():
            missing.append("SP slices")
    return missing


def sp_variety(pictures) -> list[str]:
    """pmbaff_qcif_sp: over its indices both sp_for_switch_flag values and several QsY"""
    sw = {int(v) for p in pictures for v in p.slices["sp_switch"]}
    qs = {int(v) for p in pictures for v in p.slices["qs_y"]}
    return ([] if sw == {0, 1} else ["both sp_for_switch_flag values"]) + ([] if len(qs) >= 2 else ["several QsY"])


def main() -> int:
    if not O.reference_available():
        print("reference not available: fixtures cannot be regenerated here", file=sys.stderr)
        return 2
    L = O.lib()
    fixtures = []
    for name, cidx, W, H, over, indices in CASES:
        cfg = synth.default_cfg(L, cidx, W, H, structure=A.MBAFF_FRAME, **over)
        miss = sp_variety([synth.picture(L, cfg, i) for i in indices]) if name == "pmbaff_qcif_sp" else []
        if miss:
            print(f"COVERAGE {name}: no {', '.join(miss)}", file=sys.stderr)
            return 1
        for idx in indices:
            t0 = time.time()
            p = synth.picture(L, cfg, idx)
            miss = coverage(p)
            if miss:
                print(f"COVERAGE {name}[{idx}]: no {', '.join(miss)}", file=sys.stderr)
                return 1
            entry = {"name": name, "config": cidx, "cfg": cfg.as_dict(), "index": idx,
                     "input_md5": synth.input_digest(p)}
            for stage, recon_only in (("recon", True), ("out", False)):
                ref = O.run_reference(cfg, idx, recon_only=recon_only)
                again = O.run_reference(cfg, idx, recon_only=recon_only)
                for k, pl in enumerate("YUV"):
                    if not np.array_equal(ref[k], again[k]):
                        print(f"NOT DETERMINISTIC {name}[{idx}] {stage} plane {pl}: two runs of the reference differ",
                              file=sys.stderr)
                        return 1
                entry[f"{stage}_md5"] = {pl: md5(ref[k]) for k, pl in enumerate("YUV")}
            fixtures.append(entry)
            print(f"{name}[{idx}] {W}x{H} ok ({time.time() - t0:.2f}s)")
    with open(os.path.join(HERE, "mbaff_ext.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_mbaff_ext.py",
                   "reference": "luuvish/arrow-h264 decoder/*.cc compiled by oracle/Makefile, run twice per stage",
                   "fixtures": fixtures}, f, indent=1)
    print(f"wrote {len(fixtures)} fixtures")
    return 0


if __name__ == "__main__":
    sys.exit(main())
