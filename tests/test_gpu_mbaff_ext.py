"""Lossless MBs and SP slices in MBAFF frames on MI355X (k_mbaff.hip), and the device-side refusals.

The CPU oracle refuses lossless MBs and SP slices in MBAFF frames, so the library is held directly
to the reference decoder's own MD5s (tests/golden/mbaff_ext.json, tests/golden/make_mbaff_ext.py):
bit-exact on every plane, before and after the loop filter, through the streaming API and as
device-resident batches.  What the MBAFF launch sequence does not decode must be reported by
h264r_check for a batch, which no host check sees (include/h264r.h H264R_MBAFF_FRAME).
"""
import hashlib
import json
import os

import numpy as np
import pytest

import _oracle as O
import h264r
from h264r import _abi as A
from h264r import batch as B
from h264r import synth

pytestmark = pytest.mark.gpu

EXT = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "mbaff_ext.json")))["fixtures"]


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def md5s(planes):
    return {k: md5(planes[i]) for i, k in enumerate("YUV")}


@pytest.fixture(scope="module")
def L():
    h264r.build()
    return h264r.lib()


@pytest.fixture(scope="module")
def dec(L):
    d = h264r.Decoder(0, 32, 32)
    yield d
    d.close()


def _set_refs(dec, refs):
    for s, (y, u, v) in enumerate(refs):
        dec.set_ref(s, y, u, v)


def _case(L, name):
    fxs = [f for f in EXT if f["name"] == name]
    cfg = A.SynthCfg.from_dict(fxs[0]["cfg"])
    return fxs, cfg, [synth.picture(L, cfg, f["index"]) for f in fxs]


@pytest.mark.parametrize("fx", EXT, ids=[f"{f['name']}[{f['index']}]" for f in EXT])
def test_gpu_mbaff_ext_matches_reference_fixture(L, dec, fx):
    """The streaming API: the reconstruction before the loop filter and the output, per plane, at
    the reference's MD5s."""
    cfg = A.SynthCfg.from_dict(fx["cfg"])
    p = synth.picture(L, cfg, fx["index"])
    assert synth.input_digest(p) == fx["input_md5"]
    refs = synth.refpics(L, cfg)
    rec = md5s(dec.decode_picture(p, refs, no_deblock=True))
    out = md5s(dec.decode_picture(p, refs))
    bad = [f"recon {k}" for k in "YUV" if rec[k] != fx["recon_md5"][k]]
    bad += [f"out {k}" for k in "YUV" if out[k] != fx["out_md5"][k]]
    assert not bad, f"planes off the reference: {', '.join(bad)}"


@pytest.mark.parametrize("name", ["imbaff_qcif_lossless", "pmbaff_qcif_lossless_t8", "pmbaff_qcif_sp"])
def test_gpu_mbaff_ext_batch(L, dec, name):
    """A case's pictures as one device-resident batch (h264r_decode_batch, mbaff = 1): every
    picture at the reference's output MD5s, and nothing flagged."""
    fxs, cfg, pics = _case(L, name)
    _set_refs(dec, synth.refpics(L, cfg))
    db = B.to_device(B.pack(pics, h264r.quant_flat()), len(pics), None)
    assert db.batch.mbaff == 1
    dec.decode_batch(db.batch)
    dec.check()
    for i, fx in enumerate(fxs):
        assert md5s(db.planes(i)) == fx["out_md5"], f"picture {i} (index {fx['index']})"


def _wp2(host):
    host["slices"]["wp_mode"] = 2


def _field_flag(host):
    host["mbs"]["flags"][0] ^= A.MBF_FIELD                 # the top MB of pair 0 alone


def _structure(host):
    host["pics"]["structure"] = A.FRAME


@pytest.mark.parametrize("mutate", [_wp2, _field_flag, _structure], ids=["wp_mode2", "field_flag", "structure"])
def test_gpu_mbaff_batch_refusals(L, dec, mutate):
    """What the MBAFF kernels do not decode is flagged on the device: h264r_check raises for the
    launch (implicit weights; a pair whose MBs disagree on the field flag; a picture that is no
    MBAFF frame in a batch with mbaff set), and the unmodified batch then decodes as the oracle does."""
    cfg = synth.default_cfg(L, 4, 11, 8, structure=A.MBAFF_FRAME, wp_mode=0)
    pics = [synth.picture(L, cfg, i) for i in range(2)]
    refs = synth.refpics(L, cfg)
    _set_refs(dec, refs)
    host = B.pack(pics, h264r.quant_flat())
    good = B.to_device(host, len(pics), None)
    bad_host = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in host.items()}
    mutate(bad_host)
    bad = B.to_device(bad_host, len(pics), None)
    bad.batch.mbaff = 1
    dec.decode_batch(bad.batch)
    with pytest.raises(h264r.H264RError):
        dec.check()
    dec.decode_batch(good.batch)
    dec.check()
    for i, p in enumerate(pics):
        want = O.decode(p, refs)
        got = good.planes(i)
        for k in range(3):
            assert np.array_equal(got[k], want[k]), f"picture {i} plane {k} after the refusal"


def test_gpu_mbaff_sp_refusals_streaming(L, dec):
    """An SP slice's 8x8-transform MB and QsC >= 6 are outside what the reference defines
    (include/h264r.h H264R_SLICE_SP): flagged on the device, reported for the picture."""
    fx = next(f for f in EXT if f["name"] == "pmbaff_qcif_sp")
    cfg = A.SynthCfg.from_dict(fx["cfg"])
    refs = synth.refpics(L, cfg)
    bad = synth.picture(L, cfg, fx["index"])
    bad.slices["qs_c"] = 6
    with pytest.raises(h264r.H264RError):
        dec.decode_picture(bad, refs)
    bad = synth.picture(L, cfg, fx["index"])
    bad.mbs["flags"][3] |= A.MBF_T8x8
    with pytest.raises(h264r.H264RError):
        dec.decode_picture(bad, refs)
    assert md5s(dec.decode_picture(synth.picture(L, cfg, fx["index"]), refs)) == fx["out_md5"]


def test_gpu_mbaff_ordinary_after_ext(L, dec):
    """An ordinary MBAFF P picture (no SP, no lossless) still equals the oracle after the lossless
    and the SP paths ran on the same context."""
    for name in ("pmbaff_qcif_lossless_t8", "pmbaff_qcif_sp"):
        fxs, cfg, pics = _case(L, name)
        assert md5s(dec.decode_picture(pics[0], synth.refpics(L, cfg))) == fxs[0]["out_md5"]
    cfg = synth.default_cfg(L, 3, 11, 8, structure=A.MBAFF_FRAME, num_refs=3, intra_permille=250)
    p = synth.picture(L, cfg, 0)
    refs = synth.refpics(L, cfg)
    got = dec.decode_picture(p, refs)
    want = O.decode(p, refs)
    for k in range(3):
        assert np.array_equal(got[k], want[k]), f"plane {k}"
