"""Directed extreme-value parity on MI355X: every case of tests/extremes.py through
h264r_decode_batch, every plane byte-equal to the oracle's decode.

The inputs sit exactly on the bounds the kernels are argued exact under (csrc/mb_inter4.h: the
packed 16-bit residual's PK_RES_MAX and its saturating construction, the packed 6-taps and the fp32
rounding of j, the clamped windows, wp_apply4; csrc/mb_deblock2.h and mb_deblock.h: the 16-bit sign
masks of the filter decisions), where the generator's random pictures come only by chance.
tests/test_extremes.py asserts on the host that each case hits its target and pins the oracle to the
reference decoder on the same inputs; nothing here reads the reference.
"""
import pytest

import _oracle as O
import extremes as X
import h264r
from h264r import _abi as A
from h264r import batch as B
from test_gpu_inter_residual import DEBLOCKS, _first_diff

pytestmark = pytest.mark.gpu

S_PLAIN = [n for n in X.S_CASES if n not in ("s_422_v", "s_mbaff_v")]
ALL_SCHEDULES = X.D_CASES + ["w_explicit_b_flat"] + S_PLAIN      # the D and S cases and one B case: all four schedules
SPECIAL = {"x_422_p", "s_422_v", "i_422"}                # their own context (chroma_format_idc 2)


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
    if name in ("x_mbaff_p", "s_mbaff_v"):
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


@pytest.mark.parametrize("name", ["r2_over", "m2_borders_p", "s_b_v"])
def test_gpu_extreme_streaming(dec, name):
    """The streaming API (picture_begin / mb_submit / picture_end) stages its inputs on a host path
    of its own: the over-bound residuals, the border-crossing vectors and the two-list motion of the
    strength cases through it."""
    c = X.build(name)
    for s, (y, u, v) in enumerate(c.refs):
        dec.set_ref(s, y, u, v)
    for i, p in enumerate(c.pics[:2] + c.pics[-2:]):
        got = dec.decode_picture(p)
        want = O.decode(p, c.refs)
        for k in range(3):
            d = _first_diff(got[k], want[k], 16 if k == 0 else 8)
            assert d is None, f"{name} picture {i} plane {k}: {d}"
