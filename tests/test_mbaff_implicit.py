"""Implicit bi-prediction weights in MBAFF frames: the weight rule, the ABI of the field-POC record
and the assembled expectation the GPU tests compare against (tests/mbaff_implicit.py).  CPU only;
tests/test_gpu_mbaff_implicit.py holds the kernels to the same expectation on MI355X.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import _oracle as O
import h264r
import mbaff_implicit as M
from h264r import _abi as A
from h264r import synth


@pytest.fixture(scope="module")
def L():
    h264r.build()
    return h264r.lib()


def test_weight_rule_matches_library(L):
    """The Python restatement equals h264r_implicit_w1 for every tb, td in -130 .. 130 (beyond both
    clips) and both long-term flags."""
    bad = []
    for base in (0, 7):
        for td in range(-130, 131):
            for tb in range(-130, 131):
                for lt in range(4):
                    want = M.w1_rule(base + tb, base, base + td, lt & 1, lt >> 1)
                    got = L.h264r_implicit_w1(base + tb, base, base + td, lt & 1, lt >> 1)
                    if got != want:
                        bad.append((tb, td, lt, got, want))
    assert not bad, bad[:5]
    assert M.w1_rule(0, 0, 0) == 32 and M.w1_rule(2, 0, 4) == 32 and M.w1_rule(1, 0, 4) == 16


@pytest.mark.parametrize("structure", [A.FRAME, A.TOP_FIELD, A.BOTTOM_FIELD], ids=["frame", "top", "bottom"])
def test_weight_rule_matches_generator(L, structure):
    """... and the generator's implicit_w1 tables of frame and field pictures, which the reference
    fixtures pin (tests/golden/golden.json, bfield_cif_top_implicit among them)."""
    cfg = synth.default_cfg(L, 4, 11, 8, wp_mode=2, num_refs=4, structure=structure)
    n = 0
    for index in range(4):
        p = synth.picture(L, cfg, index)
        cur = int(p.pic["poc"][0])
        for sl in p.slices:
            for i0 in range(sl["num_ref"][0]):
                for i1 in range(sl["num_ref"][1]):
                    pocs = [L.h264r_synth_slot_poc(int(r) & 31) + (1 if int(r) & A.REF_BOTTOM else 0)
                            for r in (sl["ref_slot"][0][i0], sl["ref_slot"][1][i1])]
                    assert sl["implicit_w1"][i0][i1] == M.w1_rule(cur, *pocs), (index, i0, i1)
                    n += 1
    assert n >= 4 * 16


SELF = [dict(intra_permille=0, num_refs=3),
        dict(constrained_intra=1, intra_permille=250, num_refs=3, num_slices=3, deblock_idc=0)]


@pytest.mark.parametrize("over", SELF, ids=["intra_free", "cip"])
@pytest.mark.parametrize("wp_mode", [0, 1])
def test_assembler_reproduces_the_oracle(L, wp_mode, over):
    """Where the oracle decodes the MBAFF picture itself (default and explicit weights), the expectation
    assembled from the two derived field pictures, the list-1-stripped picture and
    oracle_deblock_picture equals it byte for byte, before and after the loop filter."""
    cfg = M.mbaff_cfg(L, wp_mode=wp_mode, **over)
    p = synth.picture(L, cfg, 0)
    refs = synth.refpics(L, cfg)
    assert M.field_mb_mask(p).sum() >= 100 and M.block_mask(p).sum() >= 500
    if over["intra_permille"]:
        assert (p.mbs["flags"] & A.MBF_INTRA).sum() >= 40
    rc = M.expect_recon(p, refs)
    for stage, got in (("recon", rc), ("full", M.deblock(p, refs, rc))):
        want = O.decode(p, refs, stage=stage)
        for k in range(3):
            assert np.array_equal(got[k], want[k]), f"{stage} plane {k}"
    assert any((a != b).any() for a, b in zip(rc, O.decode(p, refs)))          # the filter does something


@pytest.mark.parametrize("num_refs,index", M.CASES)
def test_evidence_census(L, num_refs, index):
    """The GPU pictures tell the right derivation from four wrong ones: in each parity at least 20
    field MBs differ from the expectation under default weights, with the reference fields' parities
    swapped, with frame POCs in place of field POCs, and with the other parity's current POC."""
    p, refs, rec = M.case(L, num_refs, index)
    assert M.block_mask(p).sum() >= 500
    right = M.expect_recon(p, refs, rec)
    p0 = M.clone(p)
    p0.slices["wp_mode"] = 0
    wrong = {"default": M.expect_recon(p0, refs)}
    for v in M.VARIANTS[1:]:
        wrong[v] = M.expect_recon(p, refs, rec, v)
    counts = {(v, a): M.differing_field_mbs(p, right, w, a) for v, w in wrong.items() for a in range(2)}
    print(counts)
    assert min(counts.values()) >= 20, counts


def test_field_poc_abi():
    """FIELD_POC_DTYPE and Batch.field_poc mirror the C structs."""
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "h264r.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %d\n", sizeof(h264r_field_poc), offsetof(h264r_field_poc, slot_poc),
         offsetof(h264r_field_poc, long_term), offsetof(h264r_batch, field_poc), sizeof(h264r_batch),
         sizeof(h264r_slice), H264R_ABI_VERSION);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "l.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "l")
        subprocess.run(["gcc", "-I", os.path.join(O.ROOT, "include"), c, "-o", exe], check=True)
        v = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert v == [A.FIELD_POC_DTYPE.itemsize, A.FIELD_POC_DTYPE.fields["slot_poc"][1],
                 A.FIELD_POC_DTYPE.fields["long_term"][1], A.Batch.field_poc.offset, C.sizeof(A.Batch),
                 A.SLICE_DTYPE.itemsize, A.ABI_VERSION]
    assert v[0] == 272 and v[5] == 752 and v[6] == 5


def test_generator_record(L):
    """synth.field_pocs: the generator's DPB, slot s at POC 4 s (top) and 4 s + 1 (bottom)."""
    p = synth.picture(L, M.mbaff_cfg(L, 11, 8, num_refs=3), 0)
    rec = synth.field_pocs(L, p)
    assert rec.dtype == A.FIELD_POC_DTYPE and rec.shape == (1,)
    assert rec["cur_poc"][0].tolist() == [int(p.pic["poc"][0])] * 2
    assert rec["slot_poc"][0, :3].tolist() == [[0, 1], [4, 5], [8, 9]] and not rec["long_term"].any()
