"""k_inter4r's luma prediction and workgroup shape (csrc/mb_inter4.h luma_block_pred, csrc/k_recon.hip
inter4_groups) against the oracle, byte for byte, on inputs laid out by enumeration.

Phases: P pictures of 3 x 2 MBs whose MBs are all P_8x8 with 4x4 sub-partitions, every 4x4 block with a
vector of its own.  The vectors run through a list of (quarter phase, window position, reach): the
block's 9x9 luma window fully inside the picture, or across exactly one of its four edges by 1 .. 8
samples ("near") or by more than 9 ("far": the whole window outside).  census() reads the vectors back
from the pictures and the test asserts that every cell of 16 phases x (inside + 4 edges x 2 reaches) is
there and that every reach 1 .. 8 occurs on every edge: a condition on the inputs.

Reference planes: a {0, 255} checkerboard (b, h and j overshoot both ends of the clip), {0, 255} stripes
two samples wide (b1 = 16 * 255 on every fourth column, so j1 = 32 * b1 = 130560 = 127.5 * 1024: the
half-way value of (j1 + 512) >> 10), and seeded random bytes; each with the generator's residual and
without any.

Shapes: a B picture with explicit weights (the generic stages with parking, both lists); a picture that
mixes intra, I_PCM and P_SKIP MBs with the above; 9 x 2 MBs whole and as the band rows (1, 2) -- 18 and
9 MBs: a last 8-MB workgroup that is half empty, a 16-MB unit split over two workgroups, a band that
starts in the middle of one; 1 x 34 MBs with a slice per MB, each slice with its own reference order
(136 ref-table entries: past the 128 threads of a two-wave workgroup).
"""
import functools

import numpy as np
import pytest

import _oracle as O
import extremes as X
import h264r
from h264r import _abi as A
from h264r import batch as B
from h264r import synth

pytestmark = pytest.mark.gpu

W3, H3 = 3, 2
EDGES = ("left", "right", "top", "bottom")
FAR = (10, 13, 24, 70)                      # samples past the edge: more than the window's 9
PLANES = ("checker", "stripes2", "random")


def combos():
    """(phase, position, samples past the edge) in the order the blocks take them."""
    out = []
    for ph in range(16):
        out.append((ph, "inside", 0))
        for e, edge in enumerate(EDGES):
            out.append((ph, edge, 1 + (ph + 3 * e) % 8))
            out.append((ph, edge, FAR[(ph + e) % len(FAR)]))
    return out


def vector(x4, y4, PW, PH, ph, pos, k, old=(0, 0)):
    """The quarter-sample vector that puts the 9x9 window of block (x4, y4) at `pos`: columns
    x - 2 .. x + 6, rows y - 2 .. y + 6 of the integer position (x, y); the free coordinate keeps its
    window inside."""
    x, y = 4 * x4, 4 * y4
    ix = int(np.clip(old[0] >> 2, 2 - x, PW - 7 - x))
    iy = int(np.clip(old[1] >> 2, 2 - y, PH - 7 - y))
    if pos == "left":
        ix = 2 - k - x
    elif pos == "right":
        ix = PW - 7 + k - x
    elif pos == "top":
        iy = 2 - k - y
    elif pos == "bottom":
        iy = PH - 7 + k - y
    return ix * 4 + (ph & 3), iy * 4 + (ph >> 2)


def census(pics):
    """{(phase, position, "near" / "far" / None)} and {(edge, k)} of every predicted block, from the vectors."""
    cells, reach = set(), set()
    for p in pics:
        PW, PH = 16 * p.cfg.width_mbs, 16 * p.cfg.height_mbs
        for _, x4, y4, _, mvx, mvy in X.predicted_blocks(p):
            x, y = 4 * x4 + (mvx >> 2), 4 * y4 + (mvy >> 2)
            out = dict(left=2 - x, right=x + 6 - (PW - 1), top=2 - y, bottom=y + 6 - (PH - 1))
            crossed = [e for e in EDGES if out[e] > 0]
            ph = (mvx & 3) | ((mvy & 3) << 2)
            if not crossed:
                cells.add((ph, "inside", None))
            elif len(crossed) == 1:
                k = out[crossed[0]]
                reach.add((crossed[0], k))
                if k <= 8 or k > 9:
                    cells.add((ph, crossed[0], "near" if k <= 8 else "far"))
    return cells, reach


def all_8x8(p):
    """Every inter MB a P_8x8 / B_8x8 candidate of retile_4x4 (a skipped MB: the same MB, coded)."""
    for m in p.mbs:
        if int(m["mb_type"]) == A.P_SKIP and not int(m["flags"]) & A.MBF_INTRA:
            m["mb_type"] = A.P_8x8


def drop_residual(p):
    for m in p.mbs:
        if int(m["mb_type"]) != A.I_PCM:
            m["cbp"], m["cbp_blks"] = 0, 0


def enumerate_vectors(p, state, reffn=None):
    """The 4x4 blocks of p take the combos in turn, from state[0] on."""
    PW, PH = 16 * p.cfg.width_mbs, 16 * p.cfg.height_mbs
    C = combos()

    def mvfn(l, x4, y4, old):
        ph, pos, k = C[(state[0] + 5 * l) % len(C)]
        state[0] += 1
        return vector(x4, y4, PW, PH, ph, pos, k, old)
    X.retile_4x4(p, mvfn, reffn)


@functools.lru_cache(maxsize=None)
def phase_pictures(residual: bool):
    L = h264r.lib()
    cfg = synth.default_cfg(L, 3, W3, H3, num_refs=2, transform8x8=0, intra_permille=0, pcm_permille=0)
    pics, state = [], [0]
    for i in range(2):                                   # 2 x 96 blocks over 144 combos
        p = synth.picture(L, cfg, i)
        all_8x8(p)
        enumerate_vectors(p, state, reffn=lambda l, x8, y8: (x8 + y8) % 2)
        if not residual:
            drop_residual(p)
        X.check_bounds(p)
        pics.append(p)
    return tuple(pics)


@functools.lru_cache(maxsize=None)
def planes(name: str, W: int, H: int, nslots: int = 2):
    """DPB slots of one kind: luma and both chroma planes of the pattern (slot 1: the other orientation
    or polarity), or seeded random bytes."""
    out = []
    for s in range(nslots):
        slot = []
        for k, (h, w) in enumerate(((16 * H, 16 * W), (8 * H, 8 * W), (8 * H, 8 * W))):
            y, x = np.mgrid[0:h, 0:w]
            if name == "checker":
                a = ((x + y + s + k) & 1) * 255
            elif name == "stripes2":
                a = ((((x, y)[(s + k) % 2] >> 1) + (s >> 1)) & 1) * 255
            else:
                a = np.random.default_rng([0x4D43, s, k, W, H]).integers(0, 256, (h, w))
            slot.append(np.ascontiguousarray(a.astype(np.uint8)))
        out.append(tuple(slot))
    return tuple(out)


def _first_diff(a, b, n):
    bad = np.argwhere(a != b)
    if not len(bad):
        return None
    y, x = bad[0]
    return f"{len(bad)} samples differ, first at (x={x}, y={y}) MB ({x // n}, {y // n}): gpu={a[y, x]} want={b[y, x]}"


@pytest.fixture(scope="module")
def dec():
    h264r.lib()
    d = h264r.Decoder(0, 16, 34)
    yield d
    d.close()


def _decode(dec, pics, refs, rows=None, fill=None):
    for s, (y, u, v) in enumerate(refs):
        dec.set_ref(s, y, u, v)
    db = B.to_device(B.pack(list(pics), h264r.quant_flat()), len(pics), None)
    if fill is not None:
        for k in ("out_y", "out_u", "out_v"):
            db.tensors[k].fill_(fill)
    dec.set_debug(A.DBG_DEBLOCK_ROWS)
    try:
        dec.decode_batch(db.batch, rows=rows)
        dec.check()
    finally:
        dec.set_debug(0)
    return [db.planes(i) for i in range(len(pics))]


def _equal(dec, pics, refs, what):
    got = _decode(dec, pics, refs)
    for i, p in enumerate(pics):
        want = O.decode(p, list(refs))
        for k in range(3):
            d = _first_diff(got[i][k], want[k], 16 if k == 0 else 8)
            assert d is None, f"{what} picture {i} plane {k}: {d}"


def test_phase_census():
    """Every phase in every window position, near and far, and every reach 1 .. 8 on every edge."""
    for residual in (False, True):
        pics = phase_pictures(residual)
        assert all(int(m["mb_type"]) == A.P_8x8 for p in pics for m in p.mbs)
        cells, reach = census(pics)
        want = {(ph, "inside", None) for ph in range(16)} | {(ph, e, r) for ph in range(16) for e in EDGES for r in ("near", "far")}
        assert want <= cells, sorted(want - cells)
        assert {(e, k) for e in EDGES for k in range(1, 9)} <= reach
        assert any(k > 9 for _, k in reach)
    coded = sum(int(m["cbp"]) != 0 for p in phase_pictures(True) for m in p.mbs)
    assert coded and not any(int(m["cbp"]) for p in phase_pictures(False) for m in p.mbs)


@pytest.mark.parametrize("residual", (False, True), ids=("pred", "residual"))
@pytest.mark.parametrize("plane", PLANES)
def test_phases(dec, plane, residual):
    _equal(dec, phase_pictures(residual), planes(plane, W3, H3), f"{plane} residual={residual}")


def test_stripes_reach_the_half_way_j():
    """The 2-wide stripes put j1 on (2 n + 1) * 512: the value the rounding of j must send up."""
    y = planes("stripes2", W3, H3)[0][0]
    _, _, j1 = X.luma_taps(y, 17, 8)
    assert (np.abs(j1) % 1024 == 512).any(), j1


def test_b_explicit_weights(dec):
    """Both lists, explicit weights: the generic stages, their parking and the combine."""
    L = h264r.lib()
    cfg = synth.default_cfg(L, 4, W3, H3, wp_mode=1, num_refs=2, num_slices=2, transform8x8=0, intra_permille=0,
                            pcm_permille=0)
    p = synth.picture(L, cfg, 0)
    enumerate_vectors(p, [7])
    X.check_bounds(p)
    use = (p.ref_idx >= 0)
    assert (use[0] & use[1]).any() and (use[0] & ~use[1]).any() and (~use[0] & use[1]).any()
    assert all(int(s["wp_mode"]) == 1 and int(s["slice_type"]) == A.SLICE_B for s in p.slices)
    _equal(dec, (p,), planes("random", W3, H3), "B explicit")


def test_mixed_mb_kinds(dec):
    """Intra, I_PCM and P_SKIP MBs in one picture with the enumerated P_8x8 MBs."""
    L = h264r.lib()
    cfg = synth.default_cfg(L, 3, W3, H3, num_refs=2, transform8x8=0, intra_permille=250, pcm_permille=200)
    for i in range(400):
        p = synth.picture(L, cfg, i)
        t, intra = p.mbs["mb_type"], (p.mbs["flags"] & A.MBF_INTRA) != 0
        part = ~intra & (t >= A.P_16x16) & (t <= A.P_8x8)
        if (t == A.I_PCM).any() and (intra & (t != A.I_PCM)).any() and (~intra & (t == A.P_SKIP)).any() and part.sum() >= 2:
            break
    else:
        raise AssertionError("no picture of the generator mixes the four kinds")
    enumerate_vectors(p, [31])
    X.check_bounds(p)
    _equal(dec, (p,), planes("checker", W3, H3), "mixed")


@functools.lru_cache(maxsize=None)
def wide_picture():
    L = h264r.lib()
    cfg = synth.default_cfg(L, 3, 9, 2, num_refs=2, transform8x8=0, intra_permille=0, pcm_permille=0, num_slices=2,
                            deblock_idc=1)
    p = synth.picture(L, cfg, 0)
    all_8x8(p)
    enumerate_vectors(p, [0], reffn=lambda l, x8, y8: (x8 + y8) % 2)
    X.check_bounds(p)
    return p


def test_nine_by_two_whole(dec):
    """18 MBs: the last 8-MB workgroup holds 2, the second 16-MB unit is split."""
    _equal(dec, (wide_picture(),), planes("random", 9, 2), "9 x 2")


def test_nine_by_two_band(dec):
    """Rows (1, 2): 9 MBs from MB 9 on, and nothing written outside the band."""
    p = wide_picture()
    refs = planes("random", 9, 2)
    assert (p.mbs["slice"].reshape(2, 9) == np.array([[0], [1]])).all() and all(int(s["deblock_idc"]) == 1 for s in p.slices)
    got = _decode(dec, (p,), refs, rows=(1, 2), fill=0xA5)[0]
    want = O.decode(p, list(refs))
    for k in range(3):
        n = 16 if k == 0 else 8
        d = _first_diff(got[k][n:], want[k][n:], n)
        assert d is None, f"band plane {k}: {d}"
        assert (got[k][:n] == 0xA5).all(), f"band plane {k}: samples written above the band"


def test_slice_per_mb(dec):
    """34 slices, each with its own order of the three references: the workgroup's LDS copy of the ref
    tables has 136 entries."""
    L = h264r.lib()
    n = 34
    cfg = synth.default_cfg(L, 3, 1, n, num_refs=3, num_slices=n, transform8x8=0, intra_permille=0, pcm_permille=0)
    p = synth.picture(L, cfg, 0)
    assert len(p.slices) == n and (p.mbs["slice"] == np.arange(n)).all()
    for s, sl in enumerate(p.slices):
        sl["ref_slot"][0][:3] = np.roll(np.array(sl["ref_slot"][0][:3]), s % 3)
    assert len({tuple(int(v) for v in sl["ref_slot"][0][:3]) for sl in p.slices[32:]}) == 2
    all_8x8(p)
    X.retile_4x4(p, reffn=lambda l, x8, y8: (x8 + y8) % 3)
    X.check_bounds(p)
    _equal(dec, (p,), planes("random", 1, n, 3), "34 slices")
