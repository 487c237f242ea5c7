"""Directed intra-prediction parity on MI355X: the I family of tests/extremes.py (tests/extremes_i.py)
through every intra code path, every plane byte-equal to the oracle's decode.

tests/test_extremes.py holds the census of these cases (every legal (mode, block, availability) cell
with random neighbours and a mutation check, value patterns, DC rounding, plane extremes and clips) and
pins the oracle to the reference decoder on them; nothing here reads the reference.

Every plain 4:2:0 case runs three ways:
  * the default schedule: level lists; the I_4x4 sites go two to a wave through intra_pair_i4, a
    leftover single MB and the I_8x8 / I_16x16 sites through intra_mb2.  All pictures as one batch,
    and the batch without its last picture: the count of level-1 pairable MBs (I_4x4, not lossless)
    is odd in one and even in the other -- asserted on the host -- so a lone MB is left over in one;
  * the walk (A.DBG_INTRA_WALK): everything through k_intra_pic / intra_mb_compute;
  * the streaming API (dec.decode_picture), first and last picture of the I_4x4 and the I_8x8 case.
i_422 runs on the 4:2:2 context (k_c422_intra) under both schedules, the field pictures under both,
i_mbaff through k_mbaff_intra under the band walk as x_mbaff_p does.

Which MB of a pair lands on lanes 0..31 is decided by the order in which k_level_scatter's atomics
file the list on the device.  The host cannot predict it, and nothing here asserts it: both halves
run the same code on their own MB's words, and across the family's pairs either order occurs.
"""
import pytest

import _oracle as O
import extremes as X
import extremes_i as I
import h264r
from h264r import _abi as A
from h264r import batch as B
from test_gpu_inter_residual import _first_diff

pytestmark = pytest.mark.gpu

SCHEDULES = {"levels": 0, "walk": A.DBG_INTRA_WALK}
_want = {}


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


def _oracle(c, i):
    """The oracle's planes of picture i, once per process."""
    if (c.name, i) not in _want:
        _want[(c.name, i)] = O.decode(c.pics[i], c.refs)
    return _want[(c.name, i)]


def _batch(dec, c, flag, count=None):
    """The first `count` pictures of the case as one batch under debug flag `flag`."""
    n = len(c.pics) if count is None else count
    for s, (y, u, v) in enumerate(c.refs):
        dec.set_ref(s, y, u, v)
    db = B.to_device(B.pack(c.pics[:n], h264r.quant_flat()), n, None)
    dec.set_debug(flag)
    try:
        dec.decode_batch(db.batch)
        dec.check()
    finally:
        dec.set_debug(0)
    cw, _ = A.chroma_mb(c.chroma_format)
    for i in range(n):
        got = db.planes(i)
        for k in range(3):
            d = _first_diff(got[k], _oracle(c, i)[k], 16 if k == 0 else cw)
            assert d is None, f"{c.name} flag {flag} batch of {n} picture {i} plane {k}: {d}"


@pytest.mark.parametrize("name", I.I_PLAIN)
def test_gpu_intra_levels(dec, name):
    """Default schedule, the whole case and the case without its last picture (the other parity of
    the level-1 pair list)."""
    c = X.build(name)
    counts = [I.pairable_level1(p) for p in c.pics]
    assert sum(counts) % 2 != sum(counts[:-1]) % 2 and sum(counts) > 2, counts
    _batch(dec, c, SCHEDULES["levels"])
    _batch(dec, c, SCHEDULES["levels"], len(c.pics) - 1)


@pytest.mark.parametrize("name", I.I_PLAIN)
def test_gpu_intra_walk(dec, name):
    """Everything through k_intra_pic / intra_mb_compute."""
    _batch(dec, X.build(name), SCHEDULES["walk"])


@pytest.mark.parametrize("name", ["i_4x4", "i_8x8"])
def test_gpu_intra_streaming(dec, name):
    """The streaming API stages records and levels on a host path of its own."""
    c = X.build(name)
    for s, (y, u, v) in enumerate(c.refs):
        dec.set_ref(s, y, u, v)
    for i in (0, len(c.pics) - 1):
        got = dec.decode_picture(c.pics[i])
        dec.check()
        for k in range(3):
            d = _first_diff(got[k], _oracle(c, i)[k], 16 if k == 0 else 8)
            assert d is None, f"{name} picture {i} plane {k}: {d}"


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_gpu_intra_422(dec422, schedule):
    """k_c422_intra's 8 x 16 chroma prediction; the luma through the shared path."""
    _batch(dec422, X.build("i_422"), SCHEDULES[schedule])


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("name", ["i_top", "i_bottom"])
def test_gpu_intra_fields(dec, name, schedule):
    """One site picture as a top and as a bottom field."""
    c = X.build(name)
    assert int(c.pics[0].pic["structure"][0]) == (A.TOP_FIELD if name == "i_top" else A.BOTTOM_FIELD)
    _batch(dec, c, SCHEDULES[schedule])


def test_gpu_intra_mbaff(dec):
    """k_mbaff_intra: gather_tab, pred_16x16_tab, pred_chroma_tab over value patterns."""
    c = X.build("i_mbaff")
    assert all(int(p.pic["structure"][0]) == A.MBAFF_FRAME for p in c.pics)
    _batch(dec, c, A.DBG_DEBLOCK_ROWS)
