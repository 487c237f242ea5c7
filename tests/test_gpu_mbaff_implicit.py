"""Implicit bi-prediction weights in MBAFF frames on MI355X (k_mbaff.hip, h264r_field_poc).

Neither the reference driver nor the CPU oracle decodes a field MB with implicit weights, so the
kernels are held to the expectation tests/mbaff_implicit.py assembles from what the oracle does
decode (field pictures with implicit weights, which the reference pins; the MBAFF picture without
its field MBs' second list; the loop filter) -- tests/test_mbaff_implicit.py checks that assembly
against the oracle wherever the oracle decodes the MBAFF picture itself.  Bit-exact on every sample.
"""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
import h264r
import mbaff_implicit as M
from h264r import _abi as A
from h264r import batch as B
from h264r import synth

pytestmark = pytest.mark.gpu


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


def _same(got, want, what):
    for k in range(3):
        assert _diff(got[k], want[k]) is None, f"{what} plane {k}: {_diff(got[k], want[k])}"


def _set_refs(dec, refs):
    for s, (y, u, v) in enumerate(refs):
        dec.set_ref(s, y, u, v)


def _batch(dec, pics, recs, no_deblock=False):
    db = B.to_device(B.pack(pics, h264r.quant_flat(), field_pocs=recs), len(pics), None)
    assert db.batch.mbaff == 1 and (db.batch.field_poc is not None) == (recs is not None)
    dec.set_debug(A.DBG_NO_DEBLOCK if no_deblock else 0)
    try:
        dec.decode_batch(db.batch)
        dec.check()
    finally:
        dec.set_debug(0)
    return db


@pytest.fixture(scope="module")
def cases(L):
    """The three 22 x 18 pictures, one set of DPB frames (a slot's frame depends on the seed alone)
    and each picture's expected reconstruction."""
    out = [M.case(L, nr, i) for nr, i in M.CASES]
    refs = max((c[1] for c in out), key=len)
    return [(p, rec, M.expect_recon(p, refs, rec)) for p, _, rec in out], refs


def test_gpu_field_mbs_batch(L, dec, cases):
    """One three-picture batch, each picture with its own record (current POCs (poc, poc + 1)): the
    reconstruction of every MB -- field MBs against the derived field pictures, frame MBs against the
    oracle's decode of the picture without the field MBs' second list."""
    cs, refs = cases
    _set_refs(dec, refs)
    db = _batch(dec, [c[0] for c in cs], [c[1] for c in cs], no_deblock=True)
    for i, (p, rec, want) in enumerate(cs):
        got = db.planes(i)
        for a in range(2):
            assert M.differing_field_mbs(p, got, want, a) == 0, f"picture {i}: field MBs of parity {a}"
        _same(got, want, f"picture {i}")


def test_gpu_field_mbs_streaming(L, dec, cases):
    """The same through the streaming API (h264r_picture_field_pocs)."""
    cs, refs = cases
    p, rec, want = cs[0]
    _same(dec.decode_picture(p, refs, no_deblock=True, field_pocs=rec), want, "streaming")


@pytest.fixture(scope="module")
def cip(L):
    p, refs, rec = M.cip_case(L)
    return p, refs, rec, M.expect(p, refs, rec)


def test_gpu_whole_pipeline(L, dec, cip, cases):
    """Constrained intra prediction, intra MBs, 3 slices and the loop filter on every edge: the full
    output through the batch, the synchronous and the asynchronous streaming forms -- the last with a
    second picture staged behind it, each with its own record."""
    p, refs, rec, want = cip
    assert (p.mbs["flags"] & A.MBF_INTRA).sum() >= 40 and len(p.slices) == 3
    _set_refs(dec, refs)
    _same(_batch(dec, [p], [rec]).planes(0), want, "batch")
    _same(dec.decode_picture(p, field_pocs=rec), want, "streaming")
    from h264r.mbview import iter_mbs
    (p2, rec2, want2), refs2 = cases[0][0], cases[1]
    _set_refs(dec, refs2)                                  # the same frames, slot by slot
    dec.set_debug(0)
    for q, r in ((p, rec), (p2, rec2)):
        dec.init(q.cfg.width_mbs, q.cfg.height_mbs, q.pic, q.slices)
        dec.field_pocs(r)
        for addr, m, lv, mv, rr in iter_mbs(q):
            dec.decode(addr, m, lv, mv, rr)
        dec.deblock_filter_async()
    _same(dec.wait(), want, "async, first")
    _same(dec.wait(), M.deblock(p2, refs2, want2), "async, second")


def _raw_w1(tb, td):
    tx = M.cdiv(16384 + abs(M.cdiv(td, 2)), td)
    return M.clip3(-1024, 1023, (tx * tb + 32) >> 6) >> 2


def _triple(target, floor_differs=False):
    """(cur, poc0, poc1) with poc0 = 0 whose unclamped weight1 is `target` (tb, td within the clips);
    floor_differs: a negative odd td for which a flooring division would give another weight."""
    for td in range(-127, 128):
        for tb in range(-127, 128):
            if td == 0:
                continue
            if floor_differs:
                if td >= 0 or td % 2 == 0:
                    continue
                fl = M.clip3(-1024, 1023, (((16384 + abs(td // 2)) // td) * tb + 32) >> 6) >> 2
                if fl != _raw_w1(tb, td) and -64 <= _raw_w1(tb, td) <= 128 and -64 <= fl <= 128:
                    return tb, 0, td
            elif _raw_w1(tb, td) == target:
                return tb, 0, td
    raise AssertionError(f"no POC triple reaches {target}")


def _rows(L, p):
    """The directed records: (name, record)."""
    def rec(cur, s0, s1, lt=(0, 0)):
        r = M.record(L, p, cur)
        r["slot_poc"][0, 0], r["slot_poc"][0, 1], r["long_term"][0] = s0, s1, lt
        return r

    def both(t):                                           # the triple on (slot 0, slot 1), fields alike
        cur, p0, p1 = t
        return rec((cur, cur), (p0, p0), (p1, p1))
    rows = [("generator", M.record(L, p)),
            ("td == 0", rec((2, 3), (0, 1), (0, 1))),
            ("long-term top field of slot 0", rec((2, 3), (0, 1), (4, 5), (1, 0))),
            ("w1 == -64", both(_triple(-64))), ("w1 == -65 -> 32", both(_triple(-65))),
            ("w1 == 128", both(_triple(128))), ("w1 == 129 -> 32", both(_triple(129))),
            ("distances beyond the clips", rec((300, -500), (0, -900), (1000, 700))),
            ("negative odd td", both(_triple(None, floor_differs=True))),
            ("current POCs far apart", rec((2, 90), (0, 1), (4, 5)))]
    return rows


def test_gpu_directed_poc_rows(L, dec):
    """One 11 x 8 intra-free picture as a batch of N copies with N records on the weight rule's edges:
    td == 0, a long-term field, weight1 at -64 and 128 and just outside, POC distances beyond the
    clips, a negative odd td (the truncating division), current field POCs far apart."""
    cfg = M.mbaff_cfg(L, 11, 8, intra_permille=0, num_refs=2)
    p0 = synth.picture(L, cfg, 0)
    refs = synth.refpics(L, cfg)
    rows = _rows(L, p0)
    t = _triple(-64)
    assert M.w1_rule(*t) == -64 and M.w1_rule(*_triple(-65)) == 32
    assert M.w1_rule(*_triple(128)) == 128 and M.w1_rule(*_triple(129)) == 32
    pics = [M.implicit_picture(p0, r) for _, r in rows]
    wants = [M.expect_recon(q, refs, r) for q, (_, r) in zip(pics, rows)]
    for i in range(1, len(rows)):                          # every row is evidence of its own
        n = sum(M.differing_field_mbs(p0, wants[i], wants[i - 1], a) for a in range(2))
        assert n >= 1, f"row '{rows[i][0]}' changes no field MB against '{rows[i - 1][0]}'"
    _set_refs(dec, refs)
    db = _batch(dec, pics, [r for _, r in rows], no_deblock=True)
    for i, (name, _) in enumerate(rows):
        _same(db.planes(i), wants[i], f"row '{name}'")


def test_gpu_frame_mbs_alone(L, dec, cases):
    """A picture whose field MBs predict from one list each: the oracle decodes all of it (frame MBs
    take the slice's implicit_w1 table, as in a frame picture), loop filter included."""
    (p, rec, _), refs = cases[0][0], cases[1]
    q = M.strip_field_bipred(p)
    assert not M.block_mask(q).any()
    f = q.mbs["flags"].reshape(q.cfg.height_mbs, q.cfg.width_mbs)
    frame_bi = np.repeat(np.repeat((f & (A.MBF_FIELD | A.MBF_INTRA)) == 0, 4, 0), 4, 1) & (q.ref_idx >= 0).all(0)
    assert frame_bi.sum() >= 500
    _set_refs(dec, refs)
    _same(_batch(dec, [q], [rec]).planes(0), O.decode(q, refs), "frame MBs")


def test_gpu_refusals_kept_and_added(L, dec, cases):
    """Without the record wp_mode 2 is refused as before, on the device for a batch and by
    h264r_picture_end; the record is taken only inside an MBAFF picture and covers that picture alone."""
    (p, rec, want), refs = cases[0][0], cases[1]
    _set_refs(dec, refs)
    bare = B.to_device(B.pack([p], h264r.quant_flat()), 1, None)
    assert not bare.batch.field_poc
    dec.set_debug(A.DBG_NO_DEBLOCK)
    try:
        dec.decode_batch(bare.batch)
        with pytest.raises(h264r.H264RError) as e:
            dec.check()
        assert e.value.status == A.EDEVICE
    finally:
        dec.set_debug(0)
    _same(_batch(dec, [p], [rec], no_deblock=True).planes(0), want, "with the record")
    # the streaming call's states
    r = np.ascontiguousarray(rec, A.FIELD_POC_DTYPE)
    assert L.h264r_picture_field_pocs(dec.handle, A.ptr(r)) == A.ESTATE              # outside a picture
    fcfg = synth.default_cfg(L, 4, 11, 8, wp_mode=0)
    fp = synth.picture(L, fcfg, 0)
    dec.init(11, 8, fp.pic, fp.slices)
    assert L.h264r_picture_field_pocs(dec.handle, A.ptr(r)) == A.EINVAL              # a frame picture
    dec.init(p.cfg.width_mbs, p.cfg.height_mbs, p.pic, p.slices)
    assert L.h264r_picture_field_pocs(dec.handle, None) == A.EINVAL
    assert L.h264r_picture_field_pocs(dec.handle, A.ptr(r)) == A.OK
    # a record given for one picture does not cover the next
    _same(dec.decode_picture(p, no_deblock=True, field_pocs=rec), want, "streaming")
    with pytest.raises(h264r.H264RError) as e:
        dec.decode_picture(p, no_deblock=True)
    assert e.value.status == A.EUNSUPPORTED
    _same(dec.decode_picture(p, no_deblock=True, field_pocs=rec), want, "streaming, after the refusal")
