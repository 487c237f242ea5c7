#!/usr/bin/env python3
"""Generate tests/golden/extremes.json from the compiled REFERENCE decoder: the directed
extreme-value cases of tests/extremes.py (residuals at the packed transforms' bound, 0 / 255
reference patterns, motion vectors at the limits and across every border, extreme explicit
weights, deblocking lines on the thresholds, strength from motion, directed intra prediction, the
thresholds again under per-plane chroma QPs, in 4:2:2, 4:4:4, field pictures and MBAFF frames).
New cases are appended to X.CASES: the entries already in the file come out unchanged.

Run where the reference sources are (the GPU box never has them):

    python tests/golden/make_extremes.py

The cases' inputs are not the generator's, so the driver takes them from a file
(O.run_reference(inputs=), H264R_INPUTS in oracle/ref_driver.cc).  Per case the file records the
builder's name (its parameters are the CASES table of tests/extremes.py), per picture the synth
configuration, index and MD5 of the built input arrays, an MD5 of the DPB planes, and per-plane
MD5s of the reference's reconstruction before deblocking and of its output.  MD5s and
configurations only, no samples.

The reference runs TWICE per picture and stage and a case whose runs differ is refused (a read of
undefined state would otherwise be pinned); the CPU oracle must agree with the reference on every
plane, or the script stops and names the first difference.  No case had to be taken out: the
reference neither asserts on nor is non-deterministic for any input of tests/extremes.py.
"""
from __future__ import annotations

import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import _oracle as O  # noqa: E402
import extremes as X  # noqa: E402
from h264r import synth  # noqa: E402


def main() -> int:
    if not O.reference_available():
        print("reference not available: fixtures cannot be regenerated here", file=sys.stderr)
        return 2
    cases = []
    for name in X.CASES:
        t0 = time.time()
        c = X.build(name)
        entry = {"name": name, "refs_md5": X.refs_digest(c.refs), "pictures": []}
        for i, p in enumerate(c.pics):
            pe = {"cfg": p.cfg.as_dict(), "index": p.index, "input_md5": synth.input_digest(p)}
            for stage, recon_only in (("recon", True), ("out", False)):
                ref = O.run_reference(p.cfg, p.index, recon_only=recon_only, inputs=(p, c.refs))
                again = O.run_reference(p.cfg, p.index, recon_only=recon_only, inputs=(p, c.refs))
                want = O.decode(p, c.refs, stage="recon" if recon_only else "full")
                for k, pl in enumerate("YUV"):
                    if not np.array_equal(ref[k], again[k]):
                        print(f"NOT DETERMINISTIC {name}[{i}] {stage} plane {pl}: two runs of the reference differ",
                              file=sys.stderr)
                        return 1
                    if not np.array_equal(ref[k], want[k]):
                        y, x = np.argwhere(ref[k] != want[k])[0]
                        print(f"ORACLE != REFERENCE {name}[{i}] {stage} plane {pl} at (x={x}, y={y}): "
                              f"reference {ref[k][y, x]} oracle {want[k][y, x]}", file=sys.stderr)
                        return 1
                pe[f"{stage}_md5"] = {pl: X.md5(ref[k]) for k, pl in enumerate("YUV")}
            entry["pictures"].append(pe)
        cases.append(entry)
        print(f"{name}: {len(c.pics)} pictures ok ({time.time() - t0:.2f}s)")
    with open(os.path.join(HERE, "extremes.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_extremes.py",
                   "reference": "luuvish/arrow-h264 decoder/*.cc compiled by oracle/Makefile, run twice per stage on "
                                "the inputs of tests/extremes.py (H264R_INPUTS)",
                   "cases": cases}, f, indent=1)
    print(f"wrote {len(cases)} cases, {sum(len(c['pictures']) for c in cases)} pictures")
    return 0


if __name__ == "__main__":
    sys.exit(main())
