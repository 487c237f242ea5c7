"""k_inter4r's two instantiations of the inter stages (csrc/k_recon.hip): a wave of a plain picture -- at
most 8 slices, each P or I with wp_mode 0 -- takes the one-list, default-weight stages, every other wave
the generic ones, and so does a wave of a plain picture that meets what the plain stages do not cover.
Synthetic pictures decoded in one batch, every plane byte-equal to the oracle's decode (the method of
test_gpu_inter_residual._batch_vs_oracle), under DBG_DEBLOCK_ROWS and DBG_DEBLOCK_MB.

5 x 3 MBs is 15 MBs per picture: one partial 16-MB group whose last wave has invalid lanes.
test_classes_covered works the class of every picture used here out on the host, and which waves of
the plain ones fall back to the generic stages, so that no path can go untested silently.
"""
import numpy as np
import pytest

import _oracle as O
import h264r
from h264r import _abi as A
from h264r import batch as B
from h264r import synth

W5, H3 = 5, 3
SEED = 0x2643                      # one seed for every configuration of a batch: one set of reference frames
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


# ---------------------------------------------------------------- the classes, on the host
def is_plain(p) -> bool:
    """inter4_plain_picture (csrc/mb_inter4.h)."""
    n = int(p.pic["num_slices"][0])
    s = p.slices[:n]
    return (1 <= n <= PLAIN_SLICES and all(int(t) in (A.SLICE_P, A.SLICE_I) for t in s["slice_type"])
            and all(int(m) == 0 for m in s["wp_mode"]))


def fallback_waves(p, rows=None):
    """The waves (first MB address of each) of a plain picture that take the generic stages after all:
    inter4_plain_wave -- list-1 motion in reach of a lane (its block, the block left of it, the block
    above it), or an inter MB's block without a list-0 ref_idx.  (Slice indices past num_slices and
    empty RefPicList entries do not occur in these pictures.)"""
    Wm, Hm = p.cfg.width_mbs, p.cfg.height_mbs
    r0, r1 = rows if rows else (0, Hm)
    intra = (p.mbs["flags"] & A.MBF_INTRA) != 0
    out = []
    for a0 in range(r0 * Wm, r1 * Wm, 4):
        bad = False
        for a in range(a0, a0 + 4):
            a = min(a, r1 * Wm - 1)                       # invalid lanes read the range's last MB
            mbx, mby = a % Wm, a // Wm
            for by in range(4):
                for bx in range(4):
                    y, x = mby * 4 + by, mbx * 4 + bx
                    for yy, xx in ((y, x), (y, max(x - 1, 0)), (max(y - 1, 0), x)):
                        bad |= int(p.ref_idx[1, yy, xx]) >= 0 or int(p.mv[1, yy, xx]) != 0
                    bad |= (not intra[a]) and int(p.ref_idx[0, y, x]) < 0
        if bad:
            out.append(a0)
    return out


# ---------------------------------------------------------------- the pictures
def _cfg(L, cidx, H=H3, **over):
    over.setdefault("seed", SEED)
    return synth.default_cfg(L, cidx, W5, H, **over)


def _inter_block(p, a_lo, a_hi):
    """(y, x) in 4x4 units of block (1, 1) of the first inter MB with address in [a_lo, a_hi)."""
    Wm = p.cfg.width_mbs
    for a in range(a_lo, a_hi):
        if not (int(p.mbs["flags"][a]) & A.MBF_INTRA):
            return (a // Wm) * 4 + 1, (a % Wm) * 4 + 1
    raise AssertionError(f"no inter MB in [{a_lo}, {a_hi})")


def _list1_entry(p):
    """RefPicList1[0] of the picture's slices := RefPicList0[0]: a P slice has no list 1, and the oracle
    refuses a block that predicts from an empty entry."""
    p.slices["ref_slot"][:, 1, 0] = p.slices["ref_slot"][:, 0, 0]


def _edited(L):
    """Plain config-3 pictures, two of them edited after generation: in picture 1 one block in the
    middle of the second wave (MBs 4..7) gets ref_idx[1] = 0 (bi-predicted), in picture 3 one inter
    block of the third wave (MBs 8..11) gets ref_idx[0] = -1 and predicts from list 1 alone.  Pictures
    0, 2 and 4 stay as generated."""
    cfg = _cfg(L, 3)
    pics = [synth.picture(L, cfg, i) for i in range(5)]
    y, x = _inter_block(pics[1], 5, 7)
    pics[1].ref_idx[1, y, x] = 0
    _list1_entry(pics[1])
    y, x = _inter_block(pics[3], 8, 12)
    pics[3].ref_idx[0, y, x] = -1
    pics[3].ref_idx[1, y, x] = 0
    _list1_entry(pics[3])
    return pics


def _noref(L):
    """An inter block with ref_idx[0] = -1 and no list 1 either (picture 1): the plain wave must fall back,
    because the generic stages predict such a block from list 1's zeros and not as 'no reference'.  The
    oracle refuses the picture (test_classes_covered asserts it), so its bytes are compared with those
    of its twin (picture 2): the same arrays with wp_mode 2 in the slice header, which weights no
    one-list block but makes the picture the generic stages'.  This case is a self-reference: the library's
    plain-picture fallback against the library's own generic decode, not against the oracle."""
    cfg = _cfg(L, 3)
    pics = [synth.picture(L, cfg, i) for i in (0, 3, 3, 4)]
    for p in pics[1:3]:
        y, x = _inter_block(p, 8, 12)
        p.ref_idx[0, y, x] = -1
    pics[2].slices["wp_mode"][:] = 2
    return pics


def _mixed(L):
    """Plain pictures interleaved with non-plain ones: config 3 with explicit weights, B pictures with
    default and with implicit weights, a P picture of SP slices."""
    plain = _cfg(L, 3)
    others = [_cfg(L, 3, wp_mode=1), _cfg(L, 4, wp_mode=0), _cfg(L, 4, wp_mode=2), _cfg(L, 3, sp_slices=1)]
    pics = []
    for i, c in enumerate(others):
        pics += [synth.picture(L, plain, 2 * i), synth.picture(L, c, 2 * i + 1)]
    return pics + [synth.picture(L, plain, 2 * len(others))]


def _half_weighted(L):
    """Two slices, only the second weighted: not plain as a whole."""
    pics = [synth.picture(L, _cfg(L, 3, num_slices=2, wp_mode=1), i) for i in range(2)]
    for p in pics:
        p.slices["wp_mode"][0] = 0
    return pics


CASES = {
    # name: (builder, rows, {picture the oracle refuses: its twin})
    "config3": (lambda L: [synth.picture(L, _cfg(L, 3), i) for i in range(4)], None, {}),
    "config3_top": (lambda L: [synth.picture(L, _cfg(L, 3, structure=A.TOP_FIELD), i) for i in range(3)], None, {}),
    "config3_bottom": (lambda L: [synth.picture(L, _cfg(L, 3, structure=A.BOTTOM_FIELD), i) for i in range(3)], None, {}),
    "mixed": (_mixed, None, {}),
    "half_weighted": (_half_weighted, None, {}),
    "nine_slices": (lambda L: [synth.picture(L, _cfg(L, 3, H=9, num_slices=9), i) for i in range(2)], None, {}),
    "fallback": (_edited, None, {}),
    "noref": (_noref, None, {1: 2}),
    # a slice per MB row, filtered inside its slice only (idc 2): a band equals the same rows of the whole picture
    "row_band": (lambda L: [synth.picture(L, _cfg(L, 3, num_slices=3, deblock_idc=2), i) for i in range(3)], (1, 3), {}),
}
_built = {}


def _case(L, name):
    """(pictures, reference frames, the oracle's planes -- None for a picture with a twin --, rows,
    twins) of a case, built once."""
    if name not in _built:
        build, rows, twins = CASES[name]
        pics = build(L)
        refsets = [synth.refpics(L, p.cfg) for p in pics]
        refs = max(refsets, key=len)
        for rs in refsets:                                    # one seed: the slots of every configuration agree
            for s, planes in enumerate(rs):
                assert all(np.array_equal(planes[k], refs[s][k]) for k in range(3))
        # (a twin is the same refused picture: it is the reference here, compared with nothing)
        skip = set(twins) | set(twins.values())
        want = [None if i in skip else O.decode(p, refs) for i, p in enumerate(pics)]
        _built[name] = (pics, refs, want, rows, twins)
    return _built[name]


def test_classes_covered(L):
    """Plain pictures, non-plain pictures of every kind and waves that fall back are all among the cases,
    and where the cases mean them to be.  No GPU needed."""
    cls = {name: [is_plain(p) for p in _case(L, name)[0]] for name in CASES}
    print(cls)
    for name in ("config3", "config3_top", "config3_bottom", "row_band", "fallback"):
        assert all(cls[name]), (name, cls[name])
    assert cls["mixed"] == [True, False] * 4 + [True]
    assert not any(cls["half_weighted"]) and not any(cls["nine_slices"])
    kinds = set()
    for p in _case(L, "mixed")[0] + _case(L, "half_weighted")[0] + _case(L, "nine_slices")[0]:
        if not is_plain(p):
            n = int(p.pic["num_slices"][0])
            kinds.add((int(p.slices["slice_type"][0]), tuple(int(m) for m in p.slices["wp_mode"][:min(n, 2)]), n > PLAIN_SLICES))
    print(sorted(kinds))
    assert {(A.SLICE_P, (1,), False), (A.SLICE_B, (0, 0), False), (A.SLICE_B, (2, 2), False), (A.SLICE_SP, (0,), False),
            (A.SLICE_P, (0, 1), False), (A.SLICE_P, (0, 0), True)} <= kinds, kinds
    # no wave of the untouched plain pictures falls back; of each edited one exactly its edited wave
    for name in ("config3", "config3_top", "config3_bottom", "row_band"):
        pics, _, _, rows, _ = _case(L, name)
        assert all(fallback_waves(p, rows) == [] for p in pics), name
    over = [fallback_waves(p) for p in _case(L, "fallback")[0]]
    print(over)
    assert over == [[], [4], [], [8], []], over
    assert all(fallback_waves(p) == [] for p in _case(L, "mixed")[0] if is_plain(p))
    # the block without any reference: its wave falls back, the oracle gives no bytes for it, and its
    # twin differs from it in the slice header's wp_mode alone and is not plain
    pics, refs = _case(L, "noref")[:2]
    assert cls["noref"] == [True, True, False, True]
    assert [fallback_waves(p) for p in pics[:2]] == [[], [8]]
    with pytest.raises(RuntimeError):
        O.decode(pics[1], refs)
    assert all(np.array_equal(getattr(pics[1], f), getattr(pics[2], f)) for f in ("mbs", "levels", "mv", "ref_idx", "pic"))


# ---------------------------------------------------------------- GPU parity
def _diff(a, b, n):
    bad = np.argwhere(a != b)
    if not len(bad):
        return None
    y, x = bad[0]
    return f"{len(bad)} samples differ, first at (x={x}, y={y}) MB ({x // n}, {y // n}): gpu={a[y, x]} want={b[y, x]}"


def _decode_and_compare(L, dec, name, times=1):
    pics, refs, want, rows, twins = _case(L, name)
    for s, (y, u, v) in enumerate(refs):
        dec.set_ref(s, y, u, v)
    host = B.pack(pics, h264r.quant_flat())
    r0, r1 = rows if rows else (0, pics[0].cfg.height_mbs)
    for db_flag in DEBLOCKS:
        for t in range(times):
            db = B.to_device(host, len(pics), None)
            dec.set_debug(db_flag)
            try:
                dec.decode_batch(db.batch, rows=rows)
                dec.check()
            finally:
                dec.set_debug(0)
            for i in range(len(pics)):
                if i in twins.values():
                    continue
                got = db.planes(i)
                ref = db.planes(twins[i]) if i in twins else want[i]
                for k in range(3):
                    m = 16 if k == 0 else 8
                    d = _diff(got[k][r0 * m:r1 * m], ref[k][r0 * m:r1 * m], m)
                    assert d is None, f"{name} deblock flag {db_flag} launch {t} picture {i} plane {k}: {d}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["config3", "config3_top", "config3_bottom"])
def test_gpu_plain(L, dec, name):
    """(a) Config 3 as it is, and as top and bottom field pictures: the plain stages alone."""
    _decode_and_compare(L, dec, name)


@pytest.mark.gpu
def test_gpu_mixed_batch(L, dec):
    """(b) Both instantiations do real work in one launch, each on its own pictures."""
    _decode_and_compare(L, dec, "mixed")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["half_weighted", "nine_slices"])
def test_gpu_not_plain_as_a_whole(L, dec, name):
    """(c) One weighted slice of two, and nine slices: the generic stages'."""
    _decode_and_compare(L, dec, name)


@pytest.mark.gpu
def test_gpu_fallback(L, dec):
    """(d) A block with list-1 motion, and an inter block without a list-0 reference, in plain pictures:
    the bytes the oracle gives for the edited pictures, in the edited waves and in their neighbours."""
    _decode_and_compare(L, dec, "fallback")


@pytest.mark.gpu
def test_gpu_fallback_no_reference(L, dec):
    """(d) An inter block with no reference in either list: its wave falls back, and the picture equals
    the generic stages' decode of its twin."""
    _decode_and_compare(L, dec, "noref")


@pytest.mark.gpu
def test_gpu_fallback_twice(L, dec):
    """(e) The same batch decoded twice with one decoder: nothing of the first launch's fallbacks reaches
    the second."""
    _decode_and_compare(L, dec, "fallback", times=2)


@pytest.mark.gpu
def test_gpu_row_band(L, dec):
    """(f) Rows 1..2 of plain pictures (h264r_decode_batch_rows)."""
    _decode_and_compare(L, dec, "row_band")
