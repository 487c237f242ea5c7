"""k_deblock2's horizontal pass with halves written by their owner (csrc/k_deblock2.hip HALVES): lane (q, h)
of a unit filters the adjacent columns {2h, 2h + 1} of its dword and stores them as the dword's 16-bit half
h -- rows 0..13 of the ring slot, rows -3..-1 (chroma -1) into the staging of the unit above or into UpLds
-- and an edge's bS bytes reach the filters through one permute (csrc/mb_deblock2.h bs_tagged).  Batches
of 3 pictures (a wave holds 2, so the second wave's second picture slot is empty) are decoded under the
band walk (DBG_DEBLOCK_ROWS: k_deblock2) and the split walk (DBG_DEBLOCK_SPLIT: k_deblock2y + k_deblock2c),
each also with DBG_DEBLOCK_GLOBAL, and compared byte for byte with the oracle in all three planes (the
method of test_gpu_inter_park).

Sizes (MBs wide x high; a band is 4 MB rows, a staging group 4 MBs):
  1x1  no left MB, no staging partner
  2x4  one full band
  5x5  a 4-MB staging group plus a cut group, and a band of one row
  3x9  two full bands and a one-row band: rows 13..15 go through UpLds and through the upper unit's staging
Pictures: P (config 3's settings) and B with transform8x8 (config 4's, as one slice filtered across every
edge), whose 8x8 MBs skip their internal edges 1 and 3.

test_filter_reaches_every_class runs without a GPU.  A half written to the wrong place shows only where the
filter changed a sample, so for every case the oracle decodes each picture with and without the filter
(deblock_idc 0 and 1), and every (row in the MB, x mod 4) class of each plane must hold a sample that
differs, over the case's three pictures.  For luma that is all 64 classes.  A chroma edge changes p0 and q0
only (filter_normal with chromaStyleFilteringFlag, the strong chroma filter likewise), so chroma columns
with x mod 4 in {1, 2} change through horizontal edges alone: in rows 3 and 4 (the internal edge) and, where
the picture has an MB row above or below, rows 0 and 7.  Rows 1, 2, 5, 6 of those columns are out of the
filter's reach in any picture; the test asks for every class the filter can reach at the case's size.  The
seeds were searched for this condition; a size that fails it wants another seed, not another condition.
"""
import copy

import numpy as np
import pytest

import _oracle as O
import h264r
from h264r import _abi as A
from h264r import batch as B
from h264r import synth

SIZES = {"1x1": (1, 1), "2x4": (2, 4), "5x5": (5, 5), "3x9": (3, 9)}
NPICS = 3
KINDS = {"p": dict(cidx=3), "b_t8x8": dict(cidx=4, num_slices=1, deblock_idc=0)}
SEED = 0xdb2a
# (kind, size): seed, where SEED's pictures leave a class unchanged (few MBs: few filtered edges)
SEEDS = {("p", "1x1"): 118, ("p", "2x4"): 0xdb2f, ("b_t8x8", "1x1"): 0xdbaf, ("b_t8x8", "2x4"): 0xdb2d}
SCHEDULES = (A.DBG_DEBLOCK_ROWS, A.DBG_DEBLOCK_SPLIT, A.DBG_DEBLOCK_ROWS | A.DBG_DEBLOCK_GLOBAL,
             A.DBG_DEBLOCK_SPLIT | A.DBG_DEBLOCK_GLOBAL)
CASES = [(k, s) for k in KINDS for s in SIZES]
_built = {}


@pytest.fixture(scope="module")
def L():
    h264r.build()
    return h264r.lib()


@pytest.fixture(scope="module")
def dec(L):
    d = h264r.Decoder(0, 16, 16)
    yield d
    d.close()


def _case(L, kind, size):
    """(pictures, reference frames, the oracle's planes) of a case, built once."""
    if (kind, size) not in _built:
        W, H = SIZES[size]
        over = dict(KINDS[kind])
        cfg = synth.default_cfg(L, over.pop("cidx"), W, H, seed=SEEDS.get((kind, size), SEED), **over)
        assert cfg.transform8x8 == (kind == "b_t8x8")
        pics = [synth.picture(L, cfg, i) for i in range(NPICS)]
        refs = synth.refpics(L, cfg)
        _built[(kind, size)] = (pics, refs, [O.decode(p, refs) for p in pics])
    return _built[(kind, size)]


def _unfiltered(p, refs):
    """The oracle's planes of p with the filter off in every slice (deblock_idc 1)."""
    u = copy.copy(p)
    u.slices = p.slices.copy()
    u.slices["deblock_idc"] = 1
    return O.decode(u, refs)


def reachable(plane, r, c, H):
    """Whether the filter can change a sample of row r (in its MB), column class c = x mod 4, at all."""
    if plane == 0 or c in (0, 3):
        return True                                    # vertical edges: p1 p0 | q0 q1 (chroma p0 | q0)
    return r in (3, 4) or (r in (0, 7) and H > 1)      # chroma, horizontal edges: p0 | q0


@pytest.mark.parametrize("kind,size", CASES)
def test_filter_reaches_every_class(L, kind, size):
    pics, refs, want = _case(L, kind, size)
    H = SIZES[size][1]
    hit = [np.zeros((16 if k == 0 else 8, 4), bool) for k in range(3)]
    for p, w in zip(pics, want):
        raw = _unfiltered(p, refs)
        for k in range(3):
            n = 16 if k == 0 else 8
            ys, xs = np.nonzero(w[k] != raw[k])
            hit[k][ys % n, xs % 4] = True
    if kind == "b_t8x8":
        assert any(np.count_nonzero(p.mbs["flags"] & A.MBF_T8x8) for p in pics), "no MB with the 8x8 transform"
    for k in range(3):
        missing = [(r, c) for r in range(hit[k].shape[0]) for c in range(4)
                   if reachable(k, r, c, H) and not hit[k][r, c]]
        print(kind, size, "plane", k, "classes changed", int(hit[k].sum()), "missing", missing)
        assert not missing, f"{kind} {size} plane {k}: no changed sample in (row, x mod 4) classes {missing}"
        out_of_reach = [(r, c) for r in range(hit[k].shape[0]) for c in range(4)
                        if not reachable(k, r, c, H) and hit[k][r, c]]
        assert not out_of_reach, f"{kind} {size} plane {k}: the filter changed classes {out_of_reach}"


def _diff(a, b, n):
    bad = np.argwhere(a != b)
    if not len(bad):
        return None
    y, x = bad[0]
    return (f"{len(bad)} samples differ, first at (x={x}, y={y}) MB ({x // n}, {y // n}) row {y % n} "
            f"x mod 4 = {x % 4}: gpu={a[y, x]} want={b[y, x]}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,size", CASES)
def test_gpu_halves(L, dec, kind, size):
    pics, refs, want = _case(L, kind, size)
    for s, (y, u, v) in enumerate(refs):
        dec.set_ref(s, y, u, v)
    host = B.pack(pics, h264r.quant_flat())
    for flag in SCHEDULES:
        db = B.to_device(host, len(pics), None)
        dec.set_debug(flag)
        try:
            dec.decode_batch(db.batch)
            dec.check()
        finally:
            dec.set_debug(0)
        for i in range(len(pics)):
            got = db.planes(i)
            for k in range(3):
                d = _diff(got[k], want[i][k], 16 if k == 0 else 8)
                assert d is None, f"{kind} {size} deblock flags {flag} picture {i} plane {k}: {d}"
