"""Directed extreme-value parity on MI355X: every case of tests/extremes.py through
h264r_decode_batch, every plane byte-equal to the oracle's decode.

The inputs sit exactly on the bounds the kernels are argued exact under (csrc/mb_inter4.h: the
packed 16-bit residual's PK_RES_MAX and its saturating construction, the packed 6-taps and the fp32
rounding of j, the clamped windows, wp_apply4; csrc/mb_deblock2.h and mb_deblock.h: the 16-bit sign
masks of the filter decisions), where the generator's random pictures come only by chance.
tests/test_extremes.py asserts on the host that each case hits its target and pins the oracle to the
reference decoder on the same inputs; nothing here reads the reference.
"""
import numpy as np
import pytest

import _oracle as O
import extremes as X
import extremes_d2 as D2
import h264r
from h264r import _abi as A
from h264r import batch as B
from test_gpu_inter_residual import DEBLOCKS, _first_diff

pytestmark = pytest.mark.gpu

S_PLAIN = [n for n in X.S_CASES if n not in ("s_422_v", "s_mbaff_v")]
D2_420 = D2.D2_CQP + D2.D2_FIELD                         # 4:2:0 contexts: Cb != Cr in frames, field pictures
ALL_SCHEDULES = X.D_CASES + ["w_explicit_b_flat"] + S_PLAIN + D2_420     # the D, S, D2 cases and one B case: all four schedules
SPECIAL = {"x_422_p", "s_422_v", "i_422"} | set(D2.D2_422) | set(D2.D2_444)      # their own context (chroma_format_idc 2 / 3)
DEBLOCKS_FMT = (A.DBG_DEBLOCK_MB, A.DBG_DEBLOCK_ROWS, A.DBG_DEBLOCK_SPLIT)        # the schedules the 4:2:2 and 4:4:4 paths have


@pytest.fixture(scope="module")
def L():
    h264r.build()
    return h264r.lib()


@pytest.fixture(scope="module")
def dec(L):
    d = h264r.Decoder(0, 16, 16)
    yield d
    d.close()


@pytest.fixture(scope="module")
def dec422(L):
    d = h264r.Decoder(0, 16, 16, chroma_format=2)
    yield d
    d.close()


@pytest.fixture(scope="module")
def dec444(L):
    d = h264r.Decoder(0, 16, 16, chroma_format=3)
    yield d
    d.close()


def _batch_vs_oracle(dec, c, deblocks):
    for s, (y, u, v) in enumerate(c.refs):
        dec.set_ref(s, y, u, v)
    host = B.pack(c.pics, h264r.quant_flat())
    want = [O.decode(p, c.refs) for p in c.pics]
    cw, _ = A.chroma_mb(c.chroma_format)
    for db_flag in deblocks:
        db = B.to_device(host, len(c.pics), None)
        dec.set_debug(db_flag)
        try:
            dec.decode_batch(db.batch)
            dec.check()
        finally:
            dec.set_debug(0)
        for i in range(len(c.pics)):
            got = db.planes(i)
            for k in range(3):
                d = _first_diff(got[k], want[i][k], 16 if k == 0 else cw)
                assert d is None, f"{c.name} deblock flag {db_flag} picture {i} plane {k}: {d}"


@pytest.mark.parametrize("name", [n for n in X.CASES if n not in ALL_SCHEDULES and n not in SPECIAL])
def test_gpu_extreme_case(dec, name):
    """R / M / W cases and the MBAFF cases under the band walk."""
    c = X.build(name)
    if name in ("x_mbaff_p", "s_mbaff_v", "x_mbaff_cqp", "d_mbaff"):
        assert all(int(p.pic["structure"][0]) == A.MBAFF_FRAME for p in c.pics)      # k_mbaff's launch sequence
    _batch_vs_oracle(dec, c, (A.DBG_DEBLOCK_ROWS,))


@pytest.mark.parametrize("name", ALL_SCHEDULES)
def test_gpu_extreme_case_all_schedules(dec, name):
    """The deblocking-threshold cases, the strength-from-motion cases and one B case under all four
    deblocking schedules."""
    _batch_vs_oracle(dec, X.build(name), DEBLOCKS)


def test_gpu_extreme_422(dec422):
    """M1 patterns + amplified levels through k_chroma422."""
    _batch_vs_oracle(dec422, X.build("x_422_p"), (A.DBG_DEBLOCK_ROWS,))


def test_gpu_extreme_s_422(dec422):
    """Strength from motion through k_chroma422, which filters its chroma with the luma strengths,
    under the three schedules the 4:2:2 path has."""
    _batch_vs_oracle(dec422, X.build("s_422_v"), (A.DBG_DEBLOCK_MB, A.DBG_DEBLOCK_ROWS, A.DBG_DEBLOCK_SPLIT))


def _stream_vs_oracle(dec, name):
    c = X.build(name)
    for s, (y, u, v) in enumerate(c.refs):
        dec.set_ref(s, y, u, v)
    for i, p in enumerate(c.pics[:2] + c.pics[-2:]):
        got = dec.decode_picture(p)
        want = O.decode(p, c.refs)
        for k in range(3):
            d = _first_diff(got[k], want[k], 16 if k == 0 else 8)
            assert d is None, f"{name} picture {i} plane {k}: {d}"


@pytest.mark.parametrize("name", ["r2_over", "m2_borders_p", "s_b_v", "d_cqp_v", "d_mbaff"])
def test_gpu_extreme_streaming(dec, name):
    """The streaming API (picture_begin / mb_submit / picture_end) stages its inputs on a host path
    of its own: the over-bound residuals, the border-crossing vectors, the two-list motion of the
    strength cases, the per-plane chroma QPs of the threshold cases and the MBAFF threshold pictures
    (k_mbaff's launch sequence) through it."""
    _stream_vs_oracle(dec, name)


@pytest.mark.parametrize("name", D2.D2_422)
def test_gpu_extreme_d2_422(dec422, name):
    """Threshold lines on the two vertical and four horizontal chroma edges of 4:2:2 MBs, Cb and Cr
    under different QPs, through k_chroma422's loop filter under its three schedules."""
    _batch_vs_oracle(dec422, X.build(name), DEBLOCKS_FMT)


@pytest.mark.parametrize("name", D2.D2_444)
def test_gpu_extreme_d2_444(dec444, name):
    """4:4:4: Cb and Cr through the luma filter under their own QPs (k_derive444 moves qp_c into the
    luma slot of each plane's launch sequence), 8x8-transform MBs included."""
    _batch_vs_oracle(dec444, X.build(name), DEBLOCKS_FMT)


def test_gpu_extreme_d2_422_streaming(dec422):
    _stream_vs_oracle(dec422, "d_422_h")


def test_gpu_extreme_d_mbaff_bands(dec):
    """The picture of d_mbaff whose second slice (deblock_idc 2) starts at pair row 1, through
    h264r_decode_batch_rows as two bands of whole pairs: each band alone equals the oracle's rows of
    it and writes nothing else, both bands in either order give the whole picture (the restatement,
    equal to the oracle, does not filter the edge between them)."""
    c = X.build("d_mbaff")
    p = c.pics[-1]
    H = p.cfg.height_mbs
    split = D2.MBAFF_SPLIT
    assert [int(s["deblock_idc"]) for s in p.slices] == [0, 2] and split % 2 == 0
    assert (p.mbs["slice"].reshape(H, -1) == (np.arange(H) >= split)[:, None]).all()
    for s, (y, u, v) in enumerate(c.refs):
        dec.set_ref(s, y, u, v)
    want = O.decode(p, c.refs)
    db = B.to_device(B.pack([p], h264r.quant_flat()), 1, None)
    assert db.batch.mbaff == 1
    bands = [(0, split), (split, H)]
    for order in (bands[:1], bands[1:], bands, bands[::-1]):
        for k in ("out_y", "out_u", "out_v"):
            db.tensors[k].fill_(0xA5)
        for band in order:
            dec.decode_batch(db.batch, rows=band)
            dec.check()
        got = db.planes(0)
        rows = np.zeros(H, bool)
        for r0, r1 in order:
            rows[r0:r1] = True
        for k in range(3):
            n = 16 if k == 0 else 8
            inside = np.repeat(rows, n)
            d = _first_diff(got[k][inside], want[k][inside], n)
            assert d is None, f"bands {order} plane {k}: {d}"
            assert (got[k][~inside] == 0xA5).all(), f"bands {order} plane {k}: samples written outside the bands"
