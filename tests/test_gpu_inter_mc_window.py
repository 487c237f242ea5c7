"""k_inter4r's luma window across the picture's edges (csrc/mb_inter4.h luma_window_edge: an edge lane's window is
fixed up once, in a block that a wave without such a lane skips) against the oracle, byte for byte.

tests/test_gpu_inter_mc_forms.py enumerates windows across exactly one edge.  Here, on its construction (3 x 2 MBs,
every MB P_8x8 / B_8x8 with 4x4 sub-partitions, one vector per block; checkerboard, two-sample stripes and seeded
random reference planes):
  - corners: windows across two edges at once, four corners x {near 1 .. 8, far > 9} x 16 phases;
  - a wave with no edge lane: every window inside; and exactly one block across the left edge (one edge lane among
    63 interior ones);
  - two lists in one lane: a B picture whose list-0 window is inside and whose list-1 window crosses an edge, and
    the reverse, in every phase (the generic stages, parking);
  - a field picture pair referencing both parities, windows across the left and right edges and past the field's
    last row;
  - an intra and an I_PCM MB (lanes without a reference) beside edge-crossing inter MBs in one wave.
Every census function reads the vectors back from the pictures: a condition on the inputs.
"""
import functools

import numpy as np
import pytest

import _oracle as O
import extremes as X
import h264r
from h264r import _abi as A
from h264r import synth
import test_gpu_inter_mc_forms as F

pytestmark = pytest.mark.gpu

W3, H3 = F.W3, F.H3
CORNERS = (("left", "top"), ("right", "top"), ("left", "bottom"), ("right", "bottom"))
LR = ("left", "right")


@pytest.fixture(scope="module")
def dec():
    h264r.lib()
    d = h264r.Decoder(0, 16, 16)
    yield d
    d.close()


def crossings(p, x4, y4, mvx, mvy):
    """{edge: samples past it} of the 9x9 window of block (x4, y4) under the vector, positive entries only."""
    PW, PH = 16 * p.cfg.width_mbs, 16 * p.cfg.height_mbs
    x, y = 4 * x4 + (mvx >> 2), 4 * y4 + (mvy >> 2)
    out = dict(left=2 - x, right=x + 6 - (PW - 1), top=2 - y, bottom=y + 6 - (PH - 1))
    return {e: k for e, k in out.items() if k > 0}


def corner_vector(x4, y4, PW, PH, ph, corner, kx, ky):
    """The vector that puts the window of block (x4, y4) kx samples past the corner's vertical edge and ky past its
    horizontal one, at quarter phase ph."""
    x, y = 4 * x4, 4 * y4
    ix = 2 - kx - x if corner[0] == "left" else PW - 7 + kx - x
    iy = 2 - ky - y if corner[1] == "top" else PH - 7 + ky - y
    return ix * 4 + (ph & 3), iy * 4 + (ph >> 2)


def corner_combos():
    """(phase, corner, kx, ky): near = both reaches in 1 .. 8, far = both past 9; 128 cells."""
    out = []
    for ph in range(16):
        for c, corner in enumerate(CORNERS):
            out.append((ph, corner, 1 + (ph + 3 * c) % 8, 1 + (5 * ph + c) % 8))
            out.append((ph, corner, F.FAR[(ph + c) % 4], F.FAR[(ph + 2 * c + 1) % 4]))
    return out


def _p_cfg(L, **over):
    kw = dict(num_refs=2, transform8x8=0, intra_permille=0, pcm_permille=0)
    kw.update(over)
    return synth.default_cfg(L, 3, W3, H3, **kw)


@functools.lru_cache(maxsize=None)
def corner_pictures():
    L = h264r.lib()
    cfg = _p_cfg(L)
    C, n, pics = corner_combos(), [0], []
    for i in range(2):                                   # 2 x 96 blocks over 128 cells
        p = synth.picture(L, cfg, i)
        F.all_8x8(p)
        PW, PH = 16 * W3, 16 * H3

        def mvfn(l, x4, y4, old):
            ph, corner, kx, ky = C[n[0] % len(C)]
            n[0] += 1
            return corner_vector(x4, y4, PW, PH, ph, corner, kx, ky)
        X.retile_4x4(p, mvfn, lambda l, x8, y8: (x8 + y8) % 2)
        X.check_bounds(p)
        pics.append(p)
    return tuple(pics)


def corner_census(pics):
    cells = set()
    for p in pics:
        for _, x4, y4, _, mvx, mvy in X.predicted_blocks(p):
            c = crossings(p, x4, y4, mvx, mvy)
            if len(c) == 2:
                ks = list(c.values())
                reach = "near" if max(ks) <= 8 else ("far" if min(ks) > 9 else None)
                corner = tuple(e for e in ("left", "right", "top", "bottom") if e in c)
                cells.add(((mvx & 3) | ((mvy & 3) << 2), corner, reach))
    return cells


def test_corner_census():
    pics = corner_pictures()
    assert all(int(m["mb_type"]) == A.P_8x8 for p in pics for m in p.mbs)
    want = {(ph, c, r) for ph in range(16) for c in CORNERS for r in ("near", "far")}
    assert len(want) == 128
    cells = corner_census(pics)
    assert want <= cells, sorted(want - cells)


@pytest.mark.parametrize("plane", F.PLANES)
def test_corners(dec, plane):
    F._equal(dec, corner_pictures(), F.planes(plane, W3, H3), f"corners {plane}")


# ---------------------------------------------------------------- a wave with no edge lane, and with one
@functools.lru_cache(maxsize=None)
def inside_pictures():
    """Picture 0: every window inside, the phases in turn.  Picture 1: the same, but block (0, 1) of MB 0 reaches
    3 samples past the left edge."""
    L = h264r.lib()
    cfg = _p_cfg(L)
    pics = []
    for i in range(2):
        p = synth.picture(L, cfg, 0)
        F.all_8x8(p)
        n = [0]

        def mvfn(l, x4, y4, old):
            n[0] += 1
            if i == 1 and (x4, y4) == (0, 1):
                return F.vector(x4, y4, 16 * W3, 16 * H3, 6, "left", 3, old)
            return F.vector(x4, y4, 16 * W3, 16 * H3, n[0] % 16, "inside", 0, old)
        X.retile_4x4(p, mvfn, lambda l, x8, y8: (x8 + y8) % 2)
        X.check_bounds(p)
        pics.append(p)
    return tuple(pics)


def test_inside_census():
    p0, p1 = inside_pictures()
    c0 = [crossings(p0, x4, y4, mx, my) for _, x4, y4, _, mx, my in X.predicted_blocks(p0)]
    assert len(c0) == 96 and not any(c0)
    assert {(mx & 3) | ((my & 3) << 2) for _, _, _, _, mx, my in X.predicted_blocks(p0)} == set(range(16))
    c1 = {(x4, y4): crossings(p1, x4, y4, mx, my) for _, x4, y4, _, mx, my in X.predicted_blocks(p1)}
    assert {k: v for k, v in c1.items() if v} == {(0, 1): {"left": 3}}


@pytest.mark.parametrize("plane", F.PLANES)
def test_no_edge_lane_and_one(dec, plane):
    F._equal(dec, inside_pictures(), F.planes(plane, W3, H3), f"inside {plane}")


# ---------------------------------------------------------------- two lists in one lane
@functools.lru_cache(maxsize=None)
def two_list_picture():
    """A B picture: where a block uses both lists, one list's window is inside and the other's across the left or
    the right edge, alternating, the phases in turn."""
    L = h264r.lib()
    cfg = synth.default_cfg(L, 4, W3, H3, wp_mode=0, num_refs=2, num_slices=1, transform8x8=0, intra_permille=0,
                            pcm_permille=0)
    p = synth.picture(L, cfg, 0)
    F.all_8x8(p)
    p.ref_idx[:] = 0                                    # every block predicts from both lists
    PW, PH = 16 * W3, 16 * H3

    def mvfn(l, x4, y4, old):
        n = y4 * 4 * W3 + x4
        edge_list = (n // 16) % 2                      # which list crosses, 16 phases each
        if l == edge_list:
            return F.vector(x4, y4, PW, PH, n % 16, LR[(n // 32) % 2], 1 + n % 8, old)
        return F.vector(x4, y4, PW, PH, (n * 7 + 3) % 16, "inside", 0, old)
    X.retile_4x4(p, mvfn)
    X.check_bounds(p)
    return p


def two_list_census(p):
    by = {}
    for l, x4, y4, _, mx, my in X.predicted_blocks(p):
        by.setdefault((x4, y4), {})[l] = (bool(crossings(p, x4, y4, mx, my)), (mx & 3) | ((my & 3) << 2))
    cells = set()
    for v in by.values():
        if len(v) == 2 and v[0][0] != v[1][0]:
            edge = 0 if v[0][0] else 1
            cells.add((edge, v[edge][1]))
    return cells


def test_two_list_census():
    p = two_list_picture()
    assert all(int(s["slice_type"]) == A.SLICE_B for s in p.slices)
    cells = two_list_census(p)
    want = {(l, ph) for l in range(2) for ph in range(16)}
    assert want <= cells, sorted(want - cells)


@pytest.mark.parametrize("plane", ("checker", "random"))
def test_two_lists(dec, plane):
    F._equal(dec, (two_list_picture(),), F.planes(plane, W3, H3), f"two lists {plane}")


# ---------------------------------------------------------------- a field picture pair
@functools.lru_cache(maxsize=None)
def field_pictures():
    L = h264r.lib()
    pics = []
    for structure in (A.TOP_FIELD, A.BOTTOM_FIELD):
        cfg = _p_cfg(L, structure=structure, num_refs=4)
        p = synth.picture(L, cfg, 0)
        F.all_8x8(p)
        PW, PH = 16 * p.cfg.width_mbs, 16 * p.cfg.height_mbs
        pos = ("left", "right", "bottom", "inside")

        def mvfn(l, x4, y4, old):
            n = y4 * 4 * W3 + x4
            return F.vector(x4, y4, PW, PH, n % 16, pos[(n // 4) % 4], 1 + (n * 3) % 8 if n % 3 else 12, old)
        X.retile_4x4(p, mvfn, lambda l, x8, y8: (x8 + 2 * y8) % 4)
        X.check_bounds(p)
        pics.append(p)
    return tuple(pics)


def test_field_census():
    for p in field_pictures():
        assert int(p.pic["structure"][0]) != A.FRAME
        seen, parity = set(), set()
        for _, x4, y4, slot, mx, my in X.predicted_blocks(p):
            seen |= set(crossings(p, x4, y4, mx, my))
            parity.add(bool(slot & A.REF_BOTTOM))
        assert {"left", "right", "bottom"} <= seen, seen
        assert parity == {False, True}, parity


def test_field_pair(dec):
    pics = field_pictures()
    refs = synth.refpics(h264r.lib(), pics[0].cfg)
    assert all(np.array_equal(a[k], b[k]) for a, b in zip(refs, synth.refpics(h264r.lib(), pics[1].cfg)) for k in range(3))
    F._equal(dec, pics, tuple(tuple(r) for r in refs), "field pair")


# ---------------------------------------------------------------- lanes without a reference
@functools.lru_cache(maxsize=None)
def mixed_picture():
    """An intra MB and an I_PCM MB among the first four MBs (one wave), the wave's inter MBs with every window across
    the left or the right edge."""
    L = h264r.lib()
    cfg = _p_cfg(L, intra_permille=300, pcm_permille=250)
    for i in range(600):
        p = synth.picture(L, cfg, i)
        t, intra = p.mbs["mb_type"][:4], (p.mbs["flags"][:4] & A.MBF_INTRA) != 0
        part = ~intra & (t >= A.P_16x16) & (t <= A.P_8x8) & ((p.mbs["flags"][:4] & A.MBF_T8x8) == 0)
        if (t == A.I_PCM).any() and (intra & (t != A.I_PCM)).any() and part.sum() >= 1:
            break
    else:
        raise AssertionError("no picture of the generator mixes the kinds in its first wave")
    PW, PH = 16 * W3, 16 * H3

    def mvfn(l, x4, y4, old):
        n = y4 * 4 * W3 + x4
        return F.vector(x4, y4, PW, PH, n % 16, LR[n % 2], 1 + n % 8 if n % 5 else 24, old)
    X.retile_4x4(p, mvfn)
    X.check_bounds(p)
    return p


def test_mixed_census():
    p = mixed_picture()
    t, intra = p.mbs["mb_type"][:4], (p.mbs["flags"][:4] & A.MBF_INTRA) != 0
    assert (t == A.I_PCM).any() and (intra & (t != A.I_PCM)).any()
    first = [c for _, x4, y4, _, mx, my in X.predicted_blocks(p) if (y4 // 4) * W3 + x4 // 4 < 4
             for c in [crossings(p, x4, y4, mx, my)] if int(p.mbs["mb_type"][(y4 // 4) * W3 + x4 // 4]) == A.P_8x8]
    assert first and all(first) and {e for c in first for e in c} == set(LR)


def test_lanes_without_a_reference(dec):
    F._equal(dec, (mixed_picture(),), F.planes("random", W3, H3), "mixed wave")
