"""Lossless MBs and SP slices in MBAFF frames: the input generator and the reference fixtures
(tests/golden/mbaff_ext.json, written by tests/golden/make_mbaff_ext.py from the compiled
reference decoder alone -- the CPU oracle refuses these combinations, so nothing restates them).

CPU only; tests/test_gpu_mbaff_ext.py holds the library to the same fixtures on MI355X.
"""
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest

import _oracle as O
from h264r import _abi as A
from h264r import synth

_HERE = os.path.dirname(__file__)
EXT = json.load(open(os.path.join(_HERE, "golden", "mbaff_ext.json")))["fixtures"]
_IDS = [f"{f['name']}[{f['index']}]" for f in EXT]

_spec = importlib.util.spec_from_file_location("make_mbaff_ext", os.path.join(_HERE, "golden", "make_mbaff_ext.py"))
GEN = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GEN)


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_synth_accepts_mbaff_lossless_and_sp():
    """h264r_synth_picture takes H264R_MBAFF_FRAME with lossless_permille and with sp_slices, and
    still refuses it with implicit weights, other chroma formats and an odd MB-row count."""
    L = O.lib()
    p = synth.picture(L, synth.default_cfg(L, 3, 11, 8, structure=A.MBAFF_FRAME, qp_min=0, lossless_permille=400), 0)
    assert (p.mbs["flags"] & A.MBF_BYPASS).any() and (p.mbs["flags"] & A.MBF_FIELD).any()
    assert p.pic["structure"][0] == A.MBAFF_FRAME
    p = synth.picture(L, synth.default_cfg(L, 3, 11, 8, structure=A.MBAFF_FRAME, sp_slices=1), 0)
    assert (p.slices["slice_type"] == A.SLICE_SP).all()
    assert (p.slices["qs_c"] < 6).all() and (p.slices["qs_c"] >= 0).all()             # QsC < 6
    assert not (p.mbs["flags"] & A.MBF_T8x8).any()                                     # no 8x8 transform
    for bad in (dict(wp_mode=2), dict(wp_mode=2, lossless_permille=300), dict(chroma_format=2, wp_mode=0),
                dict(chroma_format=3, wp_mode=0)):
        with pytest.raises(ValueError):
            synth.picture(L, synth.default_cfg(L, 4, 11, 8, structure=A.MBAFF_FRAME, **bad), 0)
    with pytest.raises(ValueError):
        synth.picture(L, synth.default_cfg(L, 3, 11, 9, structure=A.MBAFF_FRAME, sp_slices=1), 0)


def test_fixture_cases():
    """The committed file holds the generator's cases, every index of each."""
    assert [(f["name"], f["index"]) for f in EXT] == [(c[0], i) for c in GEN.CASES for i in c[5]]
    for f in EXT:
        assert f["cfg"]["structure"] == A.MBAFF_FRAME
        assert set(f) == {"name", "config", "cfg", "index", "input_md5", "recon_md5", "out_md5"}     # MD5s only
    sp = [synth.picture(O.lib(), A.SynthCfg.from_dict(f["cfg"]), f["index"]) for f in EXT if f["name"] == "pmbaff_qcif_sp"]
    assert len(sp) == 3 and GEN.sp_variety(sp) == []


@pytest.mark.parametrize("fx", EXT, ids=_IDS)
def test_fixture_inputs_and_coverage(fx):
    """The regenerated inputs are the ones the reference decoded, and hold what the case is there
    for: bypass MBs (intra, and inter in P / B) in a field pair and in a frame pair; in an SP case
    an inter MB with residual in each kind of pair, and an intra MB."""
    p = synth.picture(O.lib(), A.SynthCfg.from_dict(fx["cfg"]), fx["index"])
    assert synth.input_digest(p) == fx["input_md5"], "synthetic generator drifted from the fixture"
    assert GEN.coverage(p) == []
    m = p.mbs
    if p.cfg.lossless_permille:
        # the bypass constraints of include/h264r.h (H264R_MBF_BYPASS): an inter MB's chroma_mode is 0
        byp_inter = ((m["flags"] & A.MBF_BYPASS) != 0) & ((m["flags"] & A.MBF_INTRA) == 0)
        assert (m["chroma_mode"][byp_inter] == 0).all()
    top = m["flags"].reshape(p.cfg.height_mbs // 2, 2, p.cfg.width_mbs)
    assert ((top[:, 0] ^ top[:, 1]) & A.MBF_FIELD == 0).all()                          # one field flag per pair


@pytest.mark.reference
@pytest.mark.skipif(not O.reference_available(), reason="needs the reference sources")
@pytest.mark.parametrize("name", ["imbaff_qcif_lossless", "pmbaff_qcif_sp"])
def test_live_reference_reproduces_fixture(name):
    """The two smallest cases (one lossless, one SP) straight from the compiled reference."""
    fx = next(f for f in EXT if f["name"] == name and f["index"] == 0)
    cfg = A.SynthCfg.from_dict(fx["cfg"])
    rec = O.run_reference(cfg, fx["index"], recon_only=True)
    assert {k: md5(rec[i]) for i, k in enumerate("YUV")} == fx["recon_md5"]
    out = O.run_reference(cfg, fx["index"])
    assert {k: md5(out[i]) for i, k in enumerate("YUV")} == fx["out_md5"]
