"""The generic stages of k_inter4r at 5 waves per SIMD (csrc/k_recon.hip, csrc/mb_inter4.h Inter4Park): a
wave that is not a plain one keeps each list's prediction, list 1's motion word and the MB record in
per-lane LDS slots across the motion compensation, and forms its lane roles again after it.  Every
kind of picture that takes those stages -- B pictures with default, explicit and implicit weights, P
pictures with explicit weights, a P picture of 9 slices, field pictures, and a batch that mixes plain
and other pictures -- decoded in batches of 3, every plane byte-equal to the oracle's decode (the
method of test_gpu_inter_plain), under DBG_DEBLOCK_ROWS and DBG_DEBLOCK_MB.

Sizes: 7 x 5 MBs = 35 MBs, two full 16-MB groups and a group of 3 MBs (one wave with a lane quad past
the end, three waves that leave before any parking), and 4 x 4 MBs, exactly one group.  The 7 x 5
pictures have a slice per MB row and filter inside their slices only (idc 2), so rows 1..3 decoded
as a band (h264r_decode_batch_rows) equal the same rows of the whole picture: every 7 x 5 case runs
as a whole and as a band against one oracle decode.

test_cases_are_generic runs without a GPU: the oracle decodes every case (the inputs are legal), and
the records show that each case has what it claims -- a block that predicts from two lists, a
weighted slice with an inter MB, or an inter MB with a slice index of 8 or more -- and that no
picture meant for the generic stages is a plain one.
"""
import numpy as np
import pytest

import _oracle as O
import h264r
from h264r import _abi as A
from h264r import batch as B
from h264r import synth

SIZES = {"7x5": (7, 5), "4x4": (4, 4)}
BAND = (1, 4)                      # MB rows of the band launch (7 x 5 only)
SEED = 0x5a17                      # one seed for every configuration of a batch: one set of reference frames
NPICS = 3
PLAIN_SLICES = 8                   # INTER4_PLAIN_SLICES (csrc/mb_inter4.h)
DEBLOCKS = (A.DBG_DEBLOCK_ROWS, A.DBG_DEBLOCK_MB)


@pytest.fixture(scope="module")
def L():
    h264r.build()
    return h264r.lib()


@pytest.fixture(scope="module")
def dec(L):
    d = h264r.Decoder(0, 16, 16)
    yield d
    d.close()


# ---------------------------------------------------------------- what a picture is, on the host
def is_plain(p) -> bool:
    """inter4_plain_picture (csrc/mb_inter4.h)."""
    n = int(p.pic["num_slices"][0])
    s = p.slices[:n]
    return (1 <= n <= PLAIN_SLICES and all(int(t) in (A.SLICE_P, A.SLICE_I) for t in s["slice_type"])
            and all(int(m) == 0 for m in s["wp_mode"]))


def _inter(p):
    return (p.mbs["flags"] & A.MBF_INTRA) == 0


def _block_mask(p, mb_mask):
    """mb_mask [H*W] spread over the 4x4 blocks [4H, 4W]."""
    Wm, Hm = p.cfg.width_mbs, p.cfg.height_mbs
    return np.repeat(np.repeat(mb_mask.reshape(Hm, Wm), 4, axis=0), 4, axis=1)


def two_list_blocks(p) -> int:
    """4x4 blocks of inter MBs that predict from both lists."""
    return int(np.count_nonzero(_block_mask(p, _inter(p)) & (p.ref_idx[0] >= 0) & (p.ref_idx[1] >= 0)))


def weighted_mbs(p) -> int:
    """Inter MBs of slices with explicit or implicit weights."""
    return int(np.count_nonzero(_inter(p) & (p.slices["wp_mode"][p.mbs["slice"]] != 0)))


def far_slice_mbs(p) -> int:
    """Inter MBs with a slice index past what a plain picture may have."""
    return int(np.count_nonzero(_inter(p) & (p.mbs["slice"] >= PLAIN_SLICES)))


# ---------------------------------------------------------------- the pictures
def _cfg(L, cidx, size, **over):
    W, H = SIZES[size]
    over.setdefault("seed", SEED)
    if size == "7x5":                                   # a slice per MB row, filtered inside it: bands
        over.setdefault("num_slices", H)
        over.setdefault("deblock_idc", 2)
    return synth.default_cfg(L, cidx, W, H, **over)


def _pics(L, cidx, size, **over):
    cfg = _cfg(L, cidx, size, **over)
    return [synth.picture(L, cfg, i) for i in range(NPICS)]


def _nine_slices(L, size):
    """P pictures (config 3, default weights) of 9 slices.  The generator cuts slices at MB rows and both
    sizes have fewer than 9 rows, so the pictures are generated with a slice per row and rows are then
    cut further, in front of an inter MB (an intra MB there would lose the left neighbour it was
    generated with).  Every slice keeps its row's header."""
    W, H = SIZES[size]
    pics = _pics(L, 3, size, num_slices=H, deblock_idc=2)
    for p in pics:
        inter = _inter(p).reshape(H, W)
        cuts = [[0] for _ in range(H)]                      # first MB column of each slice of a row
        total, row, progress = H, 0, True
        while total < 9:
            if row == 0:                                    # a whole pass over the rows without a cut
                assert progress, "no inter MB left to cut a slice at"
                progress = False
            free = [x for x in range(1, W) if inter[row, x] and x not in cuts[row]]
            if free:
                cuts[row].append(free[len(free) // 2])
                total += 1
                progress = True
            row = (row + 1) % H
        headers, index = [], np.zeros((H, W), np.uint16)
        for r in range(H):
            starts = sorted(cuts[r])
            for k, x0 in enumerate(starts):
                x1 = starts[k + 1] if k + 1 < len(starts) else W
                index[r, x0:x1] = len(headers)
                headers.append(p.slices[r])
        assert len(headers) == 9
        p.slices = np.array(headers, dtype=p.slices.dtype)
        p.mbs["slice"] = index.reshape(-1)
        p.pic["num_slices"] = 9
    return pics


def _mixed(L, size):
    """A plain picture between two others: explicit-weight P and implicit-weight B."""
    return [synth.picture(L, _cfg(L, 3, size, wp_mode=1), 0), synth.picture(L, _cfg(L, 3, size), 1),
            synth.picture(L, _cfg(L, 4, size, wp_mode=2), 2)]


# name: (builder(L, size), what the case claims of each of its non-plain pictures)
KINDS = {
    "b_default": (lambda L, s: _pics(L, 4, s, wp_mode=0), two_list_blocks),
    "b_explicit": (lambda L, s: _pics(L, 4, s, wp_mode=1), lambda p: min(two_list_blocks(p), weighted_mbs(p))),
    "b_implicit": (lambda L, s: _pics(L, 4, s, wp_mode=2), lambda p: min(two_list_blocks(p), weighted_mbs(p))),
    "p_explicit": (lambda L, s: _pics(L, 3, s, wp_mode=1), weighted_mbs),
    "p_nine_slices": (_nine_slices, far_slice_mbs),
    "b_top_field": (lambda L, s: _pics(L, 4, s, structure=A.TOP_FIELD), two_list_blocks),
    "b_bottom_field": (lambda L, s: _pics(L, 4, s, structure=A.BOTTOM_FIELD), two_list_blocks),
    "mixed": (_mixed, lambda p: two_list_blocks(p) + weighted_mbs(p)),
}
CASES = [(k, s) for k in KINDS for s in SIZES]
_built = {}


def _case(L, kind, size):
    """(pictures, reference frames, the oracle's planes) of a case, built once."""
    if (kind, size) not in _built:
        pics = KINDS[kind][0](L, size)
        refsets = [synth.refpics(L, p.cfg) for p in pics]
        refs = max(refsets, key=len)
        for rs in refsets:                                    # one seed: the slots of every configuration agree
            for s, planes in enumerate(rs):
                assert all(np.array_equal(planes[k], refs[s][k]) for k in range(3))
        _built[(kind, size)] = (pics, refs, [O.decode(p, refs) for p in pics])
    return _built[(kind, size)]


@pytest.mark.parametrize("kind,size", CASES)
def test_cases_are_generic(L, kind, size):
    """The oracle decodes the case, and its pictures are what the case says.  No GPU needed."""
    pics, _, want = _case(L, kind, size)
    assert len(pics) == NPICS and all(w is not None for w in want)
    cls = [is_plain(p) for p in pics]
    claim = [KINDS[kind][1](p) for p in pics]
    print(kind, size, cls, claim)
    if kind == "mixed":
        assert cls == [False, True, False], cls
    else:
        assert not any(cls), cls
    assert all(c >= 1 for c, plain in zip(claim, cls) if not plain), claim
    if kind == "p_nine_slices":
        assert all(int(p.pic["num_slices"][0]) == 9 and int(p.mbs["slice"].max()) == 8 for p in pics)
        assert all(int(t) == A.SLICE_P and int(m) == 0 for p in pics for t, m in zip(p.slices["slice_type"], p.slices["wp_mode"]))
    if kind.endswith("_field"):
        assert all(int(p.pic["structure"][0]) != A.FRAME for p in pics)


# ---------------------------------------------------------------- GPU parity
def _diff(a, b, n):
    bad = np.argwhere(a != b)
    if not len(bad):
        return None
    y, x = bad[0]
    return f"{len(bad)} samples differ, first at (x={x}, y={y}) MB ({x // n}, {y // n}): gpu={a[y, x]} want={b[y, x]}"


def _decode_and_compare(L, dec, kind, size, rows):
    pics, refs, want = _case(L, kind, size)
    for s, (y, u, v) in enumerate(refs):
        dec.set_ref(s, y, u, v)
    host = B.pack(pics, h264r.quant_flat())
    r0, r1 = rows if rows else (0, pics[0].cfg.height_mbs)
    for db_flag in DEBLOCKS:
        db = B.to_device(host, len(pics), None)
        dec.set_debug(db_flag)
        try:
            dec.decode_batch(db.batch, rows=rows)
            dec.check()
        finally:
            dec.set_debug(0)
        for i in range(len(pics)):
            got = db.planes(i)
            for k in range(3):
                m = 16 if k == 0 else 8
                d = _diff(got[k][r0 * m:r1 * m], want[i][k][r0 * m:r1 * m], m)
                assert d is None, f"{kind} {size} rows {rows} deblock flag {db_flag} picture {i} plane {k}: {d}"


@pytest.mark.gpu
@pytest.mark.parametrize("kind,size", CASES)
def test_gpu_generic(L, dec, kind, size):
    """Whole pictures."""
    _decode_and_compare(L, dec, kind, size, None)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_gpu_generic_band(L, dec, kind):
    """MB rows 1..3 of the 7 x 5 pictures (h264r_decode_batch_rows)."""
    _decode_and_compare(L, dec, kind, "7x5", BAND)
