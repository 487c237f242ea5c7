"""Slice bands of MBAFF frames on MI355X: h264r_decode_batch_rows with batch.mbaff (k_mbaff.hip).

A band is whole MB pairs (even rows) starting at a slice boundary whose top edge is not filtered
(idc 2 here).  Each band decoded alone equals the oracle's rows of that band -- the oracle decodes
the whole picture -- and writes nothing outside it; all bands one after another give the whole
picture.  Layouts: 22 x 18 MBs in 3 slices (bands of 3 pair rows), 11 x 8 in 2 slices, and 11 x 8
in 4 slices, where every band is one pair row, so its first and last diagonals coincide.
Bit-exact on every sample.
"""
import numpy as np
import pytest

import _oracle as O
import h264r
import mbaff_implicit as M
from h264r import _abi as A
from h264r import batch as B
from h264r import synth

pytestmark = pytest.mark.gpu

MARK = 0xA5
LAYOUTS = {"22x18s3": (22, 18, 3), "11x8s2": (11, 8, 2), "11x8s4": (11, 8, 4)}
KINDS = {
    "I": (2, dict(pcm_permille=20)),
    "P": (3, dict(num_refs=3, constrained_intra=1, wp_mode=1, intra_permille=300)),
    "B": (4, dict(wp_mode=1, num_refs=2)),
}
NPICS = 4


@pytest.fixture(scope="module")
def L():
    h264r.build()
    return h264r.lib()


@pytest.fixture(scope="module")
def dec(L):
    d = h264r.Decoder(0, 32, 32)
    yield d
    d.close()


def _diff(a, b):
    bad = np.argwhere(a != b)
    if not len(bad):
        return None
    y, x = bad[0]
    return f"{len(bad)} samples differ, first at (x={x}, y={y}): gpu={a[y, x]} want={b[y, x]}"


def _set_refs(dec, refs):
    for s, (y, u, v) in enumerate(refs):
        dec.set_ref(s, y, u, v)


def _bands(p):
    """[(row0, row1)] of the picture's slices: whole pair rows each (synth.c)."""
    H, W = p.cfg.height_mbs, p.cfg.width_mbs
    s = p.mbs["slice"].reshape(H, W)
    assert (s == s[:, :1]).all()
    first = [0] + [r for r in range(1, H) if s[r, 0] != s[r - 1, 0]] + [H]
    assert all(r % 2 == 0 for r in first)
    return list(zip(first[:-1], first[1:]))


_cases = {}


def _case(L, layout, kind):
    """(pictures, refs, oracle planes full / recon, bands) of one layout and kind; computed once."""
    key = (layout, kind)
    if key not in _cases:
        W, H, ns = LAYOUTS[layout]
        cidx, over = KINDS[kind]
        cfg = synth.default_cfg(L, cidx, W, H, structure=A.MBAFF_FRAME, num_slices=ns, deblock_idc=2, **over)
        pics = [synth.picture(L, cfg, i) for i in range(NPICS)]
        refs = synth.refpics(L, cfg)
        want = [O.decode(p, refs) for p in pics]
        bands = _bands(pics[0])
        assert len(bands) == ns
        _cases[key] = (pics, refs, want, bands)
    return _cases[key]


def _mark(db):
    for k in ("out_y", "out_u", "out_v"):
        db.tensors[k].fill_(MARK)


def _launch(dec, db, rows, no_deblock=False):
    dec.set_debug(A.DBG_NO_DEBLOCK if no_deblock else 0)
    try:
        dec.decode_batch(db.batch, rows=rows)
        dec.check()
    finally:
        dec.set_debug(0)


def _check_band(db, want, band, what):
    """Rows [band) of every plane of every picture equal `want`; every other row holds the marker."""
    r0, r1 = band
    for i in range(db.num_pics):
        got = db.planes(i)
        for k in range(3):
            n = 16 if k == 0 else 8
            d = _diff(got[k][r0 * n:r1 * n], want[i][k][r0 * n:r1 * n])
            assert d is None, f"{what} band {band} picture {i} plane {k}: {d}"
            outside = np.concatenate([got[k][:r0 * n], got[k][r1 * n:]])
            assert (outside == MARK).all(), \
                f"{what} band {band} picture {i} plane {k}: {int((outside != MARK).sum())} samples written outside the band"


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_gpu_mbaff_band_parity(L, dec, layout, kind):
    """Every band alone (its rows against the oracle, the marker everywhere else), then all bands
    one after another into one set of planes: the whole oracle picture."""
    pics, refs, want, bands = _case(L, layout, kind)
    _set_refs(dec, refs)
    db = B.to_device(B.pack(pics, h264r.quant_flat()), NPICS, None)
    assert db.batch.mbaff == 1
    for band in bands:
        _mark(db)
        _launch(dec, db, band)
        _check_band(db, want, band, f"{layout} {kind}")
    _mark(db)
    for band in bands:
        _launch(dec, db, band)
    for i in range(NPICS):
        got = db.planes(i)
        for k in range(3):
            assert _diff(got[k], want[i][k]) is None, f"{layout} {kind} all bands, picture {i} plane {k}: {_diff(got[k], want[i][k])}"
    # the last bands first: a band does not depend on the bands above it having been decoded
    _mark(db)
    for band in reversed(bands):
        _launch(dec, db, band)
    for i in range(NPICS):
        got = db.planes(i)
        for k in range(3):
            assert _diff(got[k], want[i][k]) is None, f"{layout} {kind} bands in reverse, picture {i} plane {k}"


def test_gpu_mbaff_band_whole_picture_rows(L, dec):
    """rows = (0, height_mbs) is the whole picture's launch sequence."""
    pics, refs, want, _ = _case(L, "22x18s3", "P")
    _set_refs(dec, refs)
    db = B.to_device(B.pack(pics, h264r.quant_flat()), NPICS, None)
    _mark(db)
    _launch(dec, db, (0, 18))
    _check_band(db, want, (0, 18), "whole")


@pytest.mark.parametrize("layout", ["22x18s3", "11x8s4"])
def test_gpu_mbaff_band_reconstruction_only(L, dec, layout):
    """H264R_DBG_NO_DEBLOCK: a band's reconstruction before the loop filter against the oracle's."""
    pics, refs, _, bands = _case(L, layout, "B")
    recon = [O.decode(p, refs, stage="recon") for p in pics]
    _set_refs(dec, refs)
    db = B.to_device(B.pack(pics, h264r.quant_flat()), NPICS, None)
    for band in bands[1:]:
        _mark(db)
        _launch(dec, db, band, no_deblock=True)
        _check_band(db, recon, band, f"{layout} recon")


def test_gpu_mbaff_band_field_poc_implicit_weights(L, dec):
    """Implicit weights from field POCs (h264r_batch.field_poc) in a band: constrained intra
    prediction, a quarter intra MBs, 3 slices with idc 2; the expectation is tests/mbaff_implicit.py's."""
    cfg = M.mbaff_cfg(L, 22, 18, constrained_intra=1, intra_permille=250, num_refs=3, num_slices=3, deblock_idc=2)
    p0 = synth.picture(L, cfg, 0)
    rec = M.record(L, p0)
    p = M.implicit_picture(p0, rec)
    refs = synth.refpics(L, cfg)
    want = M.expect(p, refs, rec)
    bands = _bands(p)
    assert M.block_mask(p).reshape(18, 4, -1)[6:12].any(), "no bi-predicted field MB in the middle band"
    _set_refs(dec, refs)
    db = B.to_device(B.pack([p], h264r.quant_flat(), field_pocs=[rec]), 1, None)
    assert db.batch.mbaff == 1 and db.batch.field_poc
    for band in (bands[1], bands[2], bands[0]):
        _mark(db)
        _launch(dec, db, band)
        _check_band(db, [want], band, "implicit weights")
    # without the record the band is refused on the device, as the whole picture is
    bare = B.to_device(B.pack([p], h264r.quant_flat()), 1, None)
    dec.decode_batch(bare.batch, rows=bands[1])
    with pytest.raises(h264r.H264RError) as e:
        dec.check()
    assert e.value.status == A.EDEVICE
    _mark(db)
    _launch(dec, db, bands[1])
    _check_band(db, [want], bands[1], "implicit weights, after the refusal")


def test_gpu_mbaff_band_refusals(L, dec):
    """Odd rows are H264R_EINVAL; a middle band of an idc-0 picture and a band that starts inside a
    slice of an idc-2 picture are flagged on the device (h264r_check), the launch drains, and the
    context decodes a correct band afterwards."""
    pics, refs, want, bands = _case(L, "22x18s3", "P")
    _set_refs(dec, refs)
    db = B.to_device(B.pack(pics, h264r.quant_flat()), NPICS, None)

    def good():
        _mark(db)
        _launch(dec, db, bands[1])
        _check_band(db, want, bands[1], "after a refusal")

    _mark(db)
    for rows in ((1, 6), (6, 11), (5, 13), (0, 17)):
        with pytest.raises(h264r.H264RError) as e:
            dec.decode_batch(db.batch, rows=rows)
        assert e.value.status == A.EINVAL, rows
    for k in ("out_y", "out_u", "out_v"):
        assert bool((db.tensors[k] == MARK).all()), "a refused launch wrote samples"
    good()
    # a band that starts inside a slice (idc 2): its first pair row's top edges are filtered
    _mark(db)
    dec.decode_batch(db.batch, rows=(2, 6))
    with pytest.raises(h264r.H264RError) as e:
        dec.check()
    assert e.value.status == A.EDEVICE
    for i in range(NPICS):                                   # the rows above the band were still not written
        got = db.planes(i)
        assert (got[0][:32] == MARK).all() and (got[1][:16] == MARK).all() and (got[2][:16] == MARK).all()
    good()
    # idc 0: every slice edge is filtered, so no band below row 0 is independent
    W, H, ns = LAYOUTS["22x18s3"]
    cfg0 = synth.default_cfg(L, 3, W, H, structure=A.MBAFF_FRAME, num_slices=ns, deblock_idc=0, num_refs=3)
    pics0 = [synth.picture(L, cfg0, i) for i in range(2)]
    db0 = B.to_device(B.pack(pics0, h264r.quant_flat()), 2, None)
    dec.decode_batch(db0.batch, rows=bands[1])
    with pytest.raises(h264r.H264RError) as e:
        dec.check()
    assert e.value.status == A.EDEVICE
    # ... while the picture as a whole decodes on the same context
    want0 = [O.decode(p, refs) for p in pics0]
    _mark(db0)
    _launch(dec, db0, (0, H))
    _check_band(db0, want0, (0, H), "idc 0 whole")
    good()
