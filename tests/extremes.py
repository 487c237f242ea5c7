"""Directed extreme-value inputs (TEST INFRASTRUCTURE): synthetic pictures and reference planes
overwritten in numpy so that the kernels' stated bounds are met exactly, where csrc/synth.c draws
mild values only.

Every builder starts from synth.picture / synth.refpics, changes arrays of the returned Picture and
the DPB planes, keeps the record consistent with the levels (cbp_blks recomputed the way synth.c
does, I_16x16 AC and chroma AC position 0 zero, unused lists ref_idx -1 / zero MV) and asserts on the
host, in Python integers, that every level * scale * 2^per stays below 2^31 and every block's
sum |d| at or below 2^24 (the reference's `int` arithmetic then never overflows).  B.pack,
Decoder.set_ref, O.decode and O.run_reference(inputs=) take the result unchanged.

Families (case names in CASES):
  R  residual: blocks whose sum |d| is exactly PK_RES_MAX = 32700 (packed transforms), 32701 and
     beyond (the wave falls back), coefficients past int16, residuals past int16 after >> 6, over
     prediction bytes 0 / 255; the chroma measure at its boundary; amplify() on intra and 8x8 pictures
  M  motion compensation: 0 / 255 reference patterns that drive the 6-tap intermediates to their
     limits; motion vectors at the level limits and windows straddling each border by 0..8 samples
  W  explicit weighted prediction at logWD 0 / 7, weights -128..127, offsets -128 / 127
  D  deblocking: pictures whose samples before the loop filter are known by construction, with
     lines exactly on the alpha / beta / tc / strong-filter thresholds: across MB edges (bS 1, 2, 4,
     each line checked on its own) and, in the d_every cases, across every edge, inner ones included
     (bS 3, Intra_16x16 at high QP, the 8x8 transform), checked by restating the whole loop filter
  S  strength from motion (tests/extremes_s.py): one-dimensional pictures without residual whose edges
     are decided by the motion comparison alone, every row of that rule (limits per component, picture
     identity against ref_idx, both pairings of two lists, slice boundaries) on its thresholds
  I  intra prediction (tests/extremes_i.py): intra MBs without residual whose neighbours are I_PCM
     MBs with crafted samples or, under constrained_intra_pred, inter MBs that leave poison behind:
     every legal (mode, block, availability) of I_4x4, I_8x8, I_16x16 and chroma (4:2:0 and 4:2:2) with
     random neighbours, value patterns, DC sums on both sides of every rounding, the plane predictors
     at +-9180 / +-2550 and clipping at both ends; picture borders, slice boundaries, a chain of
     dependency levels 1..7, field pictures, and a generated MBAFF case with its levels zeroed; checked
     against a restatement of 8.3 in Python integers with a mutation check per cell
  D2 deblocking thresholds under the settings D leaves out (tests/extremes_d2.py): Cb and Cr under
     different chroma QP offsets (every record legal: _set_qp(m, qp, offs)), 4:2:2, 4:4:4 and field
     pictures, by build_d and build_d_every with a pair of offsets per picture and each chroma plane on
     the thresholds of its own QPc, checked by restating the whole loop filter (deblock_restate with a
     QP grid per plane and the format's chroma geometry).  MBAFF frames (d_mbaff): crafted MBs in frame
     and field pairs of every neighbourhood, every class of edge between them on its thresholds,
     checked against deblock_restate_mbaff.  A mutation check per mistake a kernel could make.
     r4_chroma_cqp: R4 with Cb and Cr dequantised at different QPs
tests/test_extremes.py holds the census (each family hits its target, from the inputs and the oracle
alone) and pins the oracle to the reference decoder on these inputs (tests/golden/extremes.json);
tests/test_gpu_extremes.py compares the GPU with the oracle.
"""
from __future__ import annotations

import functools
import hashlib
from dataclasses import dataclass, field

import numpy as np

import _oracle as O
from h264r import _abi as A
from h264r import synth

PK_RES_MAX = 32700          # csrc/mb_inter4.h
C6 = np.array([1, -5, 20, 20, -5, 1], np.int64)

# Tables 8-16 / 8-17 and the chroma QP mapping (Table 8-15, chroma_qp_index_offset 0)
ALPHA = [0] * 16 + [4, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15, 17, 20, 22, 25, 28, 32, 36, 40, 45, 50, 56, 63, 71, 80, 90,
                    101, 113, 127, 144, 162, 182, 203, 226, 255, 255]
BETA = [0] * 16 + [2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15,
                   15, 16, 16, 17, 17, 18, 18]
TC0 = [(0, 0, 0)] * 17 + [(0, 0, 1)] * 4 + [(0, 1, 1)] * 2 + [(1, 1, 1)] * 4 + [(1, 1, 2)] * 4 + [
    (1, 2, 3), (1, 2, 3), (2, 2, 3), (2, 2, 4), (2, 3, 4), (2, 3, 4), (3, 3, 5), (3, 4, 6), (3, 4, 6), (4, 5, 7),
    (4, 5, 8), (4, 6, 9), (5, 7, 10), (6, 8, 11), (6, 8, 13), (7, 10, 14), (8, 11, 16), (9, 12, 18), (10, 13, 20),
    (11, 15, 23), (13, 17, 25)]
assert len(ALPHA) == len(BETA) == len(TC0) == 52
QP_C = list(range(30)) + [29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39]


@dataclass
class Case:
    name: str
    pics: list                  # synth.Picture
    refs: list                  # [(y, u, v)] per DPB slot
    chroma_format: int = 1      # chroma_format_idc of the decoder context
    info: dict = field(default_factory=dict)   # what the builder designed, for the census


def md5(a) -> str:
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def refs_digest(refs) -> str:
    h = hashlib.md5()
    for planes in refs:
        for a in planes:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------- level layout and the host bounds
def layout(m, idc: int = 1):
    """Offsets, relative to coef_off, of the parts of one (not PCM) MB's level block
    (include/h264r.h): ([b8 0..3 or None], chroma AC, luma DC, chroma DC, total)."""
    cbpl, cbpc = int(m["cbp"]) & 15, int(m["cbp"]) >> 4
    off, b8 = 0, [None] * 4
    for q in range(4):
        if (cbpl >> q) & 1:
            b8[q] = off
            off += 64
    i16 = int(m["mb_type"]) == A.I_16x16
    cac = ldc = cdc = None
    if idc == 2:
        if i16:
            ldc, off = off, off + 16
        if cbpc == 2:
            cac, off = off, off + 256
        if cbpc:
            cdc, off = off, off + 16
    else:
        if cbpc == 2:
            cac, off = off, off + 128
        if i16:
            ldc, off = off, off + 16
        if cbpc:
            cdc, off = off, off + 8
    return b8, cac, ldc, cdc, off


def dq4(lev, scale, per):
    return ((int(lev) * int(scale) << per) + 8) >> 4


def recompute_blks(p: synth.Picture) -> None:
    """cbp_blks from the levels, as csrc/synth.c derives it (the luma plane's coded 4x4 mask)."""
    idc = A.idc_of(p.cfg.chroma_format)
    for m in p.mbs:
        if int(m["mb_type"]) == A.I_PCM:
            continue
        b8, _, _, _, _ = layout(m, idc)
        t8 = bool(int(m["flags"]) & A.MBF_T8x8)
        blks = 0
        for q in range(4):
            if b8[q] is None:
                continue
            blk = p.levels[int(m["coef_off"]) + b8[q]: int(m["coef_off"]) + b8[q] + 64]
            if t8:
                if blk.any():
                    blks |= 0x33 << (((q >> 1) * 2) * 4 + (q & 1) * 2)
            else:
                for b4 in range(4):
                    if blk[b4 * 16: b4 * 16 + 16].any():
                        blks |= 1 << (((q >> 1) * 2 + (b4 >> 1)) * 4 + (q & 1) * 2 + (b4 & 1))
        m["cbp_blks"] = blks


def check_bounds(p: synth.Picture, quant=None) -> None:
    """The host-side bounds of every builder: |level * scale * 2^per| < 2^31 for every coefficient
    (a DC block: the sum of its |levels|, which bounds every Hadamard output) and sum |d| <= 2^24 for
    every block, in Python integers.  Also the record's consistency with the levels."""
    q = (O.quant_flat() if quant is None else quant)[0]
    idc = A.idc_of(p.cfg.chroma_format)
    nb = 8 if idc == 2 else 4
    want = p.mbs["cbp_blks"].copy()
    recompute_blks(p)
    assert (p.mbs["cbp_blks"] == want).all(), "cbp_blks does not match the levels"
    for m in p.mbs:
        if int(m["mb_type"]) == A.I_PCM or int(m["flags"]) & A.MBF_BYPASS:
            continue
        intra = int(m["flags"]) & A.MBF_INTRA
        inter = 0 if intra else 1
        t8 = bool(int(m["flags"]) & A.MBF_T8x8)
        i16 = int(m["mb_type"]) == A.I_16x16
        lv = [int(x) for x in p.levels[int(m["coef_off"]):int(m["coef_off"]) + 816]]
        b8, cac, ldc, cdc, _ = layout(m, idc)
        qpl = int(m["qp_scaled"][0])
        dcl = 0
        if ldc is not None:
            f = sum(abs(x) for x in lv[ldc:ldc + 16])
            prod = f * int(q["scale4x4"][0][0][qpl % 6][0]) << (qpl // 6)
            assert prod < 2 ** 31, prod
            dcl = (prod >> 6) + 1
        for qd in range(4):
            if b8[qd] is None:
                continue
            blk = lv[b8[qd]:b8[qd] + 64]
            if t8:
                sc = q["scale8x8"][inter][0][qpl % 6]
                prods = [abs(blk[i]) * int(sc[i]) << (qpl // 6) for i in range(64)]
                assert max(prods) < 2 ** 31 and sum(x >> 6 for x in prods) <= 2 ** 24, (max(prods), sum(prods) >> 6)
            else:
                sc = q["scale4x4"][inter][0][qpl % 6]
                for b4 in range(4):
                    if i16:
                        assert blk[b4 * 16] == 0, "I_16x16 AC position 0"
                    prods = [abs(blk[b4 * 16 + i]) * int(sc[i]) << (qpl // 6) for i in range(16)]
                    assert max(prods) < 2 ** 31 and sum(x >> 4 for x in prods) + dcl <= 2 ** 24, max(prods)
        if i16 and not any(x is not None for x in b8):
            assert dcl <= 2 ** 24
        for pl in range(2):
            if cdc is None:
                break
            qpc = int(m["qp_scaled"][1 + pl])
            sc = q["scale4x4"][inter][1 + pl][qpc % 6]
            f = sum(abs(x) for x in lv[cdc + pl * nb: cdc + pl * nb + nb])
            prod = f * int(sc[0]) << (qpc // 6)
            assert prod < 2 ** 31, prod
            dcc = (prod >> 5) + 1
            for b in range(nb):
                s = dcc
                if cac is not None:
                    blk = lv[cac + (pl * nb + b) * 16: cac + (pl * nb + b) * 16 + 16]
                    assert blk[0] == 0, "chroma AC position 0"
                    prods = [abs(blk[i]) * int(sc[i]) << (qpc // 6) for i in range(16)]
                    assert max(prods) < 2 ** 31
                    s += sum(x >> 4 for x in prods)
                assert s <= 2 ** 24, s
    # unused lists
    un = p.ref_idx < 0
    assert (p.mv[un] == 0).all(), "an unused list keeps a zero MV"


# ---------------------------------------------------------------- the packed-residual guard, on the host
def wave_sums(p, quant):
    """Per wave of k_inter4r (four consecutive MBs of the picture): (luma_coded, luma sums, blocked by an
    8x8-transform MB, chroma_coded, chroma sums) -- sum |d| of each 4x4 luma block's dequantised
    coefficients and the chroma measure of each chroma block (over the block's four lanes, the
    larger plane sum of each).  Mirrors luma_res_4x4 / inter4_chroma_residual: the lanes of intra,
    PCM and lossless MBs take no part in the test."""
    s4 = quant["scale4x4"]
    out = []
    nmb = len(p.mbs)
    for a0 in range(0, nmb, 4):
        luma_sums, chroma_sums, t8_any, luma_coded, chroma_coded = [], [], False, False, False
        for m in p.mbs[a0:a0 + 4]:
            flags, cbp = int(m["flags"]), int(m["cbp"])
            if flags & A.MBF_INTRA:
                continue
            cbpl, cbpc = cbp & 15, cbp >> 4
            luma_coded |= cbpl != 0
            chroma_coded |= cbpc != 0
            if flags & A.MBF_BYPASS:
                continue
            t8_any |= bool(flags & A.MBF_T8x8)
            lv = p.levels[int(m["coef_off"]):]
            off = 0
            qpl = int(m["qp_scaled"][0])
            for b8 in range(4):
                if not (cbpl >> b8) & 1:
                    continue
                if not flags & A.MBF_T8x8:
                    for k in range(4):
                        blk = lv[off + k * 16: off + k * 16 + 16]
                        luma_sums.append(sum(abs(dq4(blk[i], s4[1][0][qpl % 6][i], qpl // 6)) for i in range(16)))
                off += 64
            cac = off if cbpc == 2 else -1
            off += 128 if cbpc == 2 else 0
            cdc = off                      # (an inter MB has no luma DC block)
            if cbpc:
                for cb in range(4):
                    quad = np.zeros((2, 4), np.int64)      # [plane][quadrant of the 4x4 block]
                    for pl in range(2):
                        qpc = int(m["qp_scaled"][1 + pl])
                        sc, per = s4[1][1 + pl][qpc % 6], qpc // 6
                        c = [int(x) for x in lv[cdc + pl * 4: cdc + pl * 4 + 4]]
                        f = (c[0] + c[1] + c[2] + c[3], c[0] - c[1] + c[2] - c[3],
                             c[0] + c[1] - c[2] - c[3], c[0] - c[1] - c[2] + c[3])[cb]
                        for pos in range(16):
                            if pos == 0:
                                v = ((f * int(sc[0])) << per) >> 5
                            elif cbpc == 2:
                                v = dq4(lv[cac + pl * 64 + cb * 16 + pos], sc[pos], per)
                            else:
                                v = 0
                            quad[pl][(pos // 8) * 2 + (pos % 4) // 2] += abs(v)
                    # the kernel's measure: over the block's four lanes, the larger plane sum of each
                    chroma_sums.append(int(np.maximum(quad[0], quad[1]).sum()))
        out.append((luma_coded, luma_sums, t8_any, chroma_coded, chroma_sums))
    return out


def wave_paths(p, quant):
    """Per wave which residual path its luma and its chroma take: 'packed', 'fallback' or None (no
    coded residual, or a path without the test)."""
    def path(coded, sums, blocked):
        if not coded or blocked or not sums:
            return None
        return "packed" if max(sums) <= PK_RES_MAX else "fallback"
    return [(path(lc, ls, t8), path(cc, cs, False)) for lc, ls, t8, cc, cs in wave_sums(p, quant)]


def idct4x4_trace(d):
    """The 4x4 inverse transform of dequantised coefficients d [4][4] in Python integers, rows then
    columns, + 32 folded into d[0][0] as the packed kernel does: (largest |intermediate or output
    before the shift|, residual [4][4])."""
    x = [[int(v) for v in row] for row in d]
    x[0][0] += 32
    big = max(abs(v) for row in x for v in row)

    def one(a, b, c, e):
        nonlocal big
        e0, e1, e2, e3 = a + c, a - c, (b >> 1) - e, b + (e >> 1)
        o = (e0 + e3, e1 + e2, e1 - e2, e0 - e3)
        big = max(big, *(abs(v) for v in (e0, e1, e2, e3) + o))
        return o
    x = [list(one(*row)) for row in x]
    cols = [one(x[0][c], x[1][c], x[2][c], x[3][c]) for c in range(4)]
    return big, [[cols[c][r] >> 6 for c in range(4)] for r in range(4)]


def solve_sum(target: int, units):
    return _solve_sum(int(target), tuple(int(u) for u in units))


@functools.lru_cache(maxsize=None)
def _solve_sum(target: int, units: tuple):
    """Non-negative counts n[i] with sum n[i] * units[i] == target, the bulk on units[0] and as little
    as possible elsewhere (each other count below 64); None when there are none."""
    best = None
    others = units[1:]

    def rec(i, left, cnt):
        nonlocal best
        if i == len(others):
            if left >= 0 and left % units[0] == 0:
                c = [left // units[0]] + cnt
                if best is None or sum(c[1:]) < sum(best[1:]):
                    best = c
            return
        for n in range(64):
            if n * others[i] > left:
                break
            rec(i + 1, left - n * others[i], cnt + [n])
    rec(0, target, [])
    return best


def first_reachable(target: int, units, mixed=(1, 4, 5)) -> int:
    """The smallest sum >= target that levels on the even positions and `mixed` reach (the scales of
    QP >= 6 are even: 32701 itself is reachable at QP 0..5 only)."""
    return next(t for t in range(target, target + 64) if solve_sum(t, [units[0]] + [units[i] for i in mixed]))


# ---------------------------------------------------------------- R: residual
R_QPS = (0, 5, 7)           # flat scales that reach 32700 exactly; 32701 too at QP 0 and 5 (odd scales)


def _r_cfg(L, qp, **over):
    return synth.default_cfg(L, 3, 5, 3, qp_min=qp, qp_max=qp, **over)


def _luma_units(quant, qp):
    sc = quant["scale4x4"][1][0][qp % 6]
    return [dq4(1, sc[i], qp // 6) for i in range(16)]


def r_block(units, target, a=1, b=1, g=1, mixed=(1, 4, 5)):
    """16 raster levels of one 4x4 block whose sum |d| is exactly `target`: the bulk on the positions
    with unit weights through both passes, (0,0) (0,2) (2,0) (2,2), the remainder on `mixed`
    positions (other scales).  Signs: coefficient (u, v) of the even positions takes g * a^(u/2) *
    b^(v/2); with a = b = 1 every coefficient has the sign g and sample (0,0) is g * sum |d|."""
    even = (0, 2, 8, 10)
    n = solve_sum(target, [units[0]] + [units[i] for i in mixed])
    assert n is not None, (target, units)
    lev = [0] * 16
    share, extra = divmod(n[0], 4)
    for k, pos in enumerate(even):
        s = g * (a if pos >= 8 else 1) * (b if pos % 4 == 2 else 1)
        lev[pos] = s * (share + (1 if k < extra else 0))
    for cnt, pos in zip(n[1:], mixed):
        lev[pos] = g * cnt
    assert sum(abs(v) * units[i] for i, v in enumerate(lev)) == target
    assert max(abs(v) for v in lev) < 32768
    return lev


def r_corner_block(units, target, row3: bool, col3: bool, g=1):
    """sum |d| == target with about a third of the mass on the odd positions (0,1), (1,0), (1,1), signed
    so that ONE corner sample -- (0,0), (0,3), (3,0) or (3,3) -- is g * sum |d| and the other three
    corners are smaller: basis 1 weighs the two ends +1 and -1, bases 0 and 2 weigh them +1 and +1."""
    su, sv = (-1 if row3 else 1), (-1 if col3 else 1)
    odd = {1: sv, 4: su, 5: su * sv}
    lev = [0] * 16
    for pos in odd:
        lev[pos] = target // 9 // units[pos]
    rest = target - sum(lev[p] * units[p] for p in odd)
    n = next(m for m in (solve_sum(rest - k * units[1], [units[0]]) and (k, rest - k * units[1]) for k in range(64)) if m)
    lev[1] += n[0]
    share, extra = divmod(n[1] // units[0], 4)
    for k, pos in enumerate((0, 2, 8, 10)):
        lev[pos] = share + (1 if k < extra else 0)
    lev = [g * v * odd.get(i, 1) for i, v in enumerate(lev)]
    assert sum(abs(v) * units[i] for i, v in enumerate(lev)) == target
    return lev


def _single(units, want, pos=0, above=False):
    """One coefficient at `pos` whose dequantised value is the nearest at or below (above: at or
    above) `want` in magnitude, with want's sign."""
    n = abs(want) // units[pos] + (1 if above and abs(want) % units[pos] else 0)
    lev = [0] * 16
    lev[pos] = n if want > 0 else -n
    return lev


def r_over_blocks(units):
    """The blocks of R2: each sends its wave to the 32-bit code (name, levels)."""
    u = units
    t1, t2, t3 = (first_reachable(t, u) for t in (PK_RES_MAX + 1, 32736, 32768))
    return [
        (f"sum{t1}+", r_block(u, t1, g=1)), (f"sum{t1}-", r_block(u, t1, g=-1)),
        (f"sum{t2}+", r_block(u, t2, g=1)),        # + 32 passes int16: what a larger PK_RES_MAX would break
        (f"sum{t3}-", r_block(u, t3, g=-1)),
        ("one<=32767", _single(u, 32767)), ("one>=32768", _single(u, 32768, above=True)),
        ("one<=-32768", _single(u, -32768, above=True)), ("one40000", _single(u, 40000, pos=5)),
    ]


def _inter4_mbs(p):
    return [i for i, m in enumerate(p.mbs) if not int(m["flags"]) & (A.MBF_INTRA | A.MBF_T8x8 | A.MBF_BYPASS)
            and int(m["cbp"]) & 15]


def _set_luma_blocks(p, mi, blocks):
    """Overwrite every coded 4x4 luma block of MB mi with next(blocks)."""
    m = p.mbs[mi]
    b8, _, _, _, _ = layout(m)
    for q in range(4):
        if b8[q] is None:
            continue
        for b4 in range(4):
            o = int(m["coef_off"]) + b8[q] + b4 * 16
            p.levels[o:o + 16] = next(blocks)


def _cycle(seq, start=0):
    i = start
    while True:
        yield seq[i % len(seq)]
        i += 1


def flat_refs(L, cfg, values=(0, 255)):
    """DPB planes of one value per slot (R3: prediction bytes 0 and 255 whatever the motion)."""
    refs = synth.refpics(L, cfg)
    return [tuple(np.full_like(a, values[s % len(values)]) for a in planes) for s, planes in enumerate(refs)]


def build_r_luma(L, over_bound: bool, flat: bool) -> Case:
    """R1 (over_bound False): every coded inter 4x4 luma block has sum |d| exactly 32700, under the
    eight sign patterns and with mixed positions where the scales ask for them.  R2 (True): one block
    of each wave is one of r_over_blocks, so every such wave falls back.  R3 (flat): the same over
    all-0 / all-255 references."""
    quant = O.quant_flat()[0]
    pics, design = [], []
    for qp in R_QPS:
        units = _luma_units(quant, qp)
        at = [r_block(units, PK_RES_MAX, a, b, g) for g in (1, -1) for a in (1, -1) for b in (1, -1)]
        at += [r_block(units, PK_RES_MAX, 1, 1, g, mixed=(3, 12, 15)) for g in (1, -1)]
        at += [r_corner_block(units, PK_RES_MAX, r3, c3, g) for g in (1, -1) for r3 in (False, True) for c3 in (False, True)]
        over = r_over_blocks(units)
        for idx in range(2 if over_bound else 1):
            p = synth.picture(L, _r_cfg(L, qp), idx)
            mbs = _inter4_mbs(p)
            for n, mi in enumerate(mbs):
                _set_luma_blocks(p, mi, _cycle(at, 3 * n))
            if over_bound:
                for w in range(0, len(p.mbs), 4):
                    mine = [mi for mi in mbs if w <= mi < w + 4]
                    if not mine:
                        continue
                    name, lev = over[(idx * 4 + w // 4) % len(over)]
                    m = p.mbs[mine[0]]
                    o = int(m["coef_off"]) + next(x for x in layout(m)[0] if x is not None)
                    p.levels[o:o + 16] = lev
                    design.append((len(pics), w // 4, name))
            recompute_blks(p)
            check_bounds(p)
            pics.append(p)
    if over_bound:
        # |d| near 2^24: the residual after >> 6 is past int16 (pk_sat); QP 48, both signs
        qp = 48
        units = _luma_units(quant, qp)
        p = synth.picture(L, _r_cfg(L, qp), 0)
        for n, mi in enumerate(_inter4_mbs(p)):
            lev = _single(units, (1 << 24) * (1 if n % 2 == 0 else -1), pos=(0, 5, 10, 3)[n % 4])
            _set_luma_blocks(p, mi, _cycle([lev, [0] * 16, [-v for v in lev], [0] * 16]))
            design.append((len(pics), mi // 4, "near2^24"))
        recompute_blks(p)
        check_bounds(p)
        pics.append(p)
    cfg = pics[0].cfg
    refs = flat_refs(L, cfg) if flat else synth.refpics(L, cfg)
    name = ("r3_" if flat else "") + ("r2_over" if over_bound else "r1_at_bound")
    return Case(name, pics, refs, info=dict(design=design))


def _chroma_units(quant, qp, pl):
    sc, per = quant["scale4x4"][1][1 + pl][qp % 6], qp // 6
    u = [dq4(1, sc[i], per) for i in range(16)]
    u[0] = ((1 * int(sc[0])) << per) >> 5        # the DC, through the 2x2 Hadamard and >> 5
    assert ((1000 * int(sc[0])) << per) >> 5 == 1000 * u[0]
    return u


R4_SPECS = ((0, (0, 0)), (7, (0, 0)))               # (qp_y, chroma QP offsets) per picture
# Cb and Cr at different qp_scaled, both at QPs whose flat scales reach 32700: (QPc 0, QPc 7) and (7, 0)
R4_SPECS_CQP = ((3, (-3, 4)), (5, (2, -5)))


def build_r_chroma(L, over_bound: bool, specs=R4_SPECS, name=None) -> Case:
    """R4: the chroma measure of inter4_chroma_residual at 32700 (over_bound: one MB per wave at 32701
    or, DC only, the next reachable value): cbpc 2 with the mass in one plane, in the other, and
    split over the planes in different quadrants; cbpc 1 through the Hadamard.  With chroma QP offsets
    (r4_chroma_cqp) every MB's planes are dequantised at different QPs, each plane's levels solved in
    its own units, and no MB is split: one plane is at the bound, the other far below it."""
    quant = O.quant_flat()[0]
    pics, design = [], []
    for qp, co in specs:
        qpc = [qpc_of(qp, co[pl]) for pl in range(2)]
        units = [_chroma_units(quant, qpc[pl], pl) for pl in range(2)]

        def ac_block(total, positions, sign=1, u=None):
            """levels of one plane's 4x4 block (DC excluded) with sum |d| == total on `positions`"""
            u = units[0] if u is None else u
            n = solve_sum(total, [u[i] for i in positions]) if total else [0] * len(positions)
            assert n is not None, (total, positions)
            lev = [0] * 16
            for cnt, pos in zip(n, positions):
                lev[pos] = sign * cnt
            return lev

        def mb_levels(m, big_pl, total, split=False):
            """Set MB m's chroma: plane big_pl carries `total` in quadrant 0 (DC and positions 1, 4, 5)
            of every block, the other plane a level of 1; split: 20000 of it there and the rest in the
            other plane's quadrant 3."""
            _, cac, _, cdc, _ = layout(m)
            o = int(m["coef_off"])
            cbpc = int(m["cbp"]) >> 4
            u, uo = units[big_pl], units[1 - big_pl]
            p_.levels[o + cdc:o + cdc + 8] = 0
            if cbpc == 1:
                assert total % u[0] == 0
                c0 = total // u[0]
                # through the Hadamard: {c0, 0, 0, 0} gives every block f = c0; {h, h, 0, 0} blocks 0, 2
                dc = [c0, 0, 0, 0] if c0 % 2 else [c0 // 2, c0 // 2, 0, 0]
                p_.levels[o + cdc + big_pl * 4: o + cdc + big_pl * 4 + 4] = dc
                p_.levels[o + cdc + (1 - big_pl) * 4] = -1
                return
            p_.levels[o + cac:o + cac + 128] = 0
            first = 20000 if split else total
            # about half of the plane's share through the DC, the rest on AC positions it can reach
            dcv = next(v for v in range((first // 2) // u[0], 0, -1)
                       if solve_sum(first - v * u[0], [u[i] for i in (1, 4, 5)]))
            rest = first - dcv * u[0]
            p_.levels[o + cdc + big_pl * 4] = dcv
            for cb in range(4):
                base = o + cac + big_pl * 64 + cb * 16
                p_.levels[base:base + 16] = ac_block(rest, (1, 4, 5), -1 if cb & 1 else 1, u)
                other = o + cac + (1 - big_pl) * 64 + cb * 16
                p_.levels[other:other + 16] = ac_block(total - first, (10, 11, 14, 15), u=uo) if split else ac_block(uo[1], (1,), u=uo)

        p_ = synth.picture(L, _r_cfg(L, qp), 2)
        cqp = co != (0, 0)
        if cqp:
            for m in p_.mbs:
                _set_qp(m, int(m["qp_y"]), co)
        mbs = [i for i, m in enumerate(p_.mbs) if not int(m["flags"]) & A.MBF_INTRA and int(m["cbp"]) >> 4]
        at_dc = [PK_RES_MAX - PK_RES_MAX % units[pl][0] for pl in range(2)]
        for n, mi in enumerate(mbs):
            m = p_.mbs[mi]
            if int(m["cbp"]) >> 4 == 1:
                mb_levels(m, n % 2, at_dc[n % 2])
            else:
                mb_levels(m, n % 2, PK_RES_MAX, split=n % 3 == 2 and not cqp)
        if over_bound:
            for w in range(0, len(p_.mbs), 4):
                mine = [mi for mi in mbs if w <= mi < w + 4]
                if not mine:
                    continue
                m = p_.mbs[mine[-1]]
                big = (w // 4) % 2
                if int(m["cbp"]) >> 4 == 1:
                    mb_levels(m, big, at_dc[big] + units[big][0])
                else:
                    mb_levels(m, big, PK_RES_MAX + (1 if qpc[big] < 6 else 2), split=big == 1 and not cqp)   # QP >= 6: even scales
                design.append((len(pics), w // 4, int(m["cbp"]) >> 4) + ((big,) if cqp else ()))
        recompute_blks(p_)
        check_bounds(p_)
        pics.append(p_)
    return Case(name or ("r4_chroma_over" if over_bound else "r4_chroma_at_bound"), pics, synth.refpics(L, pics[0].cfg),
                info=dict(design=design))


def build_r_chroma_cqp(L) -> Case:
    """r4_chroma_cqp: the at-bound pictures, then the over-bound ones, under R4_SPECS_CQP."""
    at, over = (build_r_chroma(L, ob, R4_SPECS_CQP, "r4_chroma_cqp") for ob in (False, True))
    design = [(d[0] + len(at.pics),) + tuple(d[1:]) for d in over.info["design"]]
    return Case("r4_chroma_cqp", at.pics + over.pics, at.refs, info=dict(design=design, at_bound=len(at.pics)))


def amplify(p: synth.Picture, k: int) -> None:
    """Multiply every generated level of p by k (PCM samples are not levels)."""
    pcm = np.zeros(len(p.levels), bool)
    idc = A.idc_of(p.cfg.chroma_format)
    npcm = {2: 256, 3: 384, 0: 128}.get(idc, 192)
    for m in p.mbs:
        if int(m["mb_type"]) == A.I_PCM:
            pcm[int(m["coef_off"]):int(m["coef_off"]) + npcm] = True
    v = p.levels.astype(np.int64) * k
    assert np.abs(v[~pcm]).max() < 32768
    p.levels[~pcm] = v[~pcm].astype(np.int16)


def max_gain(p: synth.Picture, cap: int = 4000) -> int:
    """The largest k <= cap for which amplify(p, k) keeps the host-side bounds."""
    lo, hi = 1, cap
    while lo < hi:
        k = (lo + hi + 1) // 2
        t = synth.Picture(p.cfg, p.index, p.mbs.copy(), p.levels.copy(), p.mv, p.ref_idx, p.slices, p.pic)
        try:
            amplify(t, k)
            check_bounds(t)
            lo = k
        except AssertionError:
            hi = k - 1
    return lo


def build_r_amplified(L, cidx: int, W: int, H: int, n: int, refs=None, name=None, **over) -> Case:
    """R5: generated pictures with every level multiplied by the largest k the host-side bounds
    allow (two QP ranges: the bounds bind at high QP, the saturation is widest at low QP)."""
    pics, gains = [], []
    for i in range(n):
        qp = ((0, 20), (20, 40), (30, 51))[i % 3]
        cfg = synth.default_cfg(L, cidx, W, H, **dict(dict(qp_min=qp[0], qp_max=qp[1]), **over))
        p = synth.picture(L, cfg, i)
        k = max_gain(p)
        amplify(p, k)
        check_bounds(p)
        pics.append(p)
        gains.append(k)
    cfg = pics[0].cfg
    return Case(name or f"r5_amplified_c{cidx}", pics, refs(L, cfg) if refs else synth.refpics(L, cfg),
                chroma_format=A.idc_of(cfg.chroma_format), info=dict(gains=gains))


# ---------------------------------------------------------------- M: motion compensation
STRIPE = np.array([255, 0, 255], np.uint8)       # 255, 0, 255, 255, 0, 255: the 6-tap's maximum 42 * 255


def pattern(name: str, h: int, w: int, seed: int = 0) -> np.ndarray:
    """One 0 / 255 plane: flat0 flat255 checker1 checker2 stripe_x stripe_x_inv stripe_y stripe_y_inv
    outer_max (stripe_x * stripe_y: j1 = 42 * 42 * 255) outer_min (stripe_x * inverse stripe_y:
    j1 = -10 * 42 * 255) xnor / xor (255 where the two taps' signs agree / differ: the extremes of j1
    over all 0 / 255 windows, (42 * 42 + 10 * 10) * 255 = 475320 and -2 * 42 * 10 * 255 = -214200) random."""
    y, x = np.mgrid[0:h, 0:w]
    sx, sy = (STRIPE[x % 3] > 0), (STRIPE[y % 3] > 0)
    if name == "random":
        bits = np.random.default_rng(seed).integers(0, 2, (h, w)).astype(bool)
    else:
        bits = {"flat0": np.zeros((h, w), bool), "flat255": np.ones((h, w), bool),
                "checker1": ((x + y) & 1) == 0, "checker2": (((x >> 1) + (y >> 1)) & 1) == 0,
                "stripe_x": sx, "stripe_x_inv": ~sx, "stripe_y": sy, "stripe_y_inv": ~sy,
                "outer_max": sx & sy, "outer_min": sx & ~sy, "xnor": sx == sy, "xor": sx != sy}[name]
    return np.ascontiguousarray(np.where(bits, 255, 0).astype(np.uint8))


CHROMA_OF = {"flat0": ("flat255", "flat0"), "flat255": ("flat0", "flat255")}


def pattern_refs(L, cfg, names, seed=7):
    """DPB planes: slot s holds luma pattern names[s % len]; the chroma planes their own patterns (a
    checkerboard and seeded random 0 / 255; the flat ones the opposite value in Cb)."""
    out = []
    for s, (y, u, v) in enumerate(synth.refpics(L, cfg)):
        nm = names[s % len(names)]
        if nm == "generated":
            out.append((y, u, v))
            continue
        cu, cv = CHROMA_OF.get(nm, ("checker1" if s % 2 == 0 else "stripe_x", "random"))
        out.append((pattern(nm, *y.shape, seed=seed + s), pattern(cu, *u.shape, seed=seed + 100 + s),
                    pattern(cv, *v.shape, seed=seed + 200 + s)))
    return out


def pack_mv(x, y):
    return np.uint32((int(x) & 0xFFFF) | ((int(y) & 0xFFFF) << 16))


def mv_xy(v):
    v = int(v)
    x, y = v & 0xFFFF, v >> 16
    return x - 0x10000 if x & 0x8000 else x, y - 0x10000 if y & 0x8000 else y


def retile_4x4(p: synth.Picture, mvfn=None, reffn=None) -> None:
    """Every inter MB with partitions (not skip, not 8x8 transform) becomes P_8x8 / B_8x8 whose
    sub-blocks are 4x4, so that each 4x4 block may carry a vector of its own: mvfn(list, x4, y4, old
    (x, y)) -> (x, y) in quarter samples; reffn(list, x8, y8) -> ref_idx for the lists
    the 8x8 block uses.  Lists a block does not use keep ref_idx -1 and a zero MV."""
    W = p.cfg.width_mbs
    for mi, m in enumerate(p.mbs):
        if int(m["flags"]) & (A.MBF_INTRA | A.MBF_T8x8) or not A.P_16x16 <= int(m["mb_type"]) <= A.P_8x8:
            continue
        m["mb_type"] = A.P_8x8
        x0, y0 = (mi % W) * 4, (mi // W) * 4
        for l in range(2):
            for by in range(4):
                for bx in range(4):
                    x4, y4 = x0 + bx, y0 + by
                    r = int(p.ref_idx[l, y4, x4])
                    if r < 0:
                        continue
                    if reffn is not None:
                        p.ref_idx[l, y4, x4] = reffn(l, x4 // 2, y4 // 2)
                    if mvfn is not None:
                        p.mv[l, y4, x4] = pack_mv(*mvfn(l, x4, y4, mv_xy(p.mv[l, y4, x4])))


def predicted_blocks(p: synth.Picture):
    """(list, x4, y4, slot, mvx, mvy) of every 4x4 block an inter MB predicts from a list."""
    W = p.cfg.width_mbs
    for mi, m in enumerate(p.mbs):
        if int(m["flags"]) & A.MBF_INTRA:
            continue
        sl = p.slices[int(m["slice"])]
        for l in range(2):
            for by in range(4):
                for bx in range(4):
                    x4, y4 = (mi % W) * 4 + bx, (mi // W) * 4 + by
                    r = int(p.ref_idx[l, y4, x4])
                    if r >= 0:
                        yield (l, x4, y4, int(sl["ref_slot"][l][r])) + mv_xy(p.mv[l, y4, x4])


def luma_taps(plane: np.ndarray, x: int, y: int):
    """Unrounded 6-tap intermediates of the 4x4 block at integer position (x, y) with clamped
    coordinates: b1 [9 window rows][4], h1 [4][5 columns x .. x + 4 - 1 + 1], j1 [4][4]."""
    h, w = plane.shape
    win = plane[np.ix_(np.clip(np.arange(y - 2, y + 7), 0, h - 1), np.clip(np.arange(x - 2, x + 7), 0, w - 1))].astype(np.int64)
    b1 = sum(C6[k] * win[:, k:k + 4] for k in range(6))                     # rows y-2 .. y+6
    h1 = sum(C6[k] * win[k:k + 4, 2:7] for k in range(6))                   # columns x .. x+4
    j1 = sum(C6[k] * b1[k:k + 4, :] for k in range(6))
    return b1, h1, j1


def build_m_patterns(L, names, name, cidx=3, W=5, H=3, n=6, **over) -> Case:
    """M1: the generator's motion (every inter MB retiled to 4x4 sub-blocks, the fractional part of
    each vector replaced so that all 16 phases come up on every slot) over 0 / 255 patterns."""
    over = dict(dict(num_refs=len(names), transform8x8=0), **over)
    cfg = synth.default_cfg(L, cidx, W, H, **over)
    pics = []
    for i in range(n):
        p = synth.picture(L, cfg, i)
        count = [0]

        def mvfn(l, x4, y4, old, i=i, count=count):
            count[0] += 1
            ph = (count[0] * 7 + i + 5 * l) % 16
            return (old[0] & ~3) | (ph & 3), (old[1] & ~3) | (ph >> 2)
        retile_4x4(p, mvfn)
        check_bounds(p)
        pics.append(p)
    return Case(name, pics, pattern_refs(L, cfg, names))


BORDERS = ("L", "R", "T", "B", "TL", "TR", "BL", "BR")
LIMIT_MVS = ((8191, 2047), (-8192, -2048), (8191, -2048), (-8192, 2047))


def build_m_borders(L, bslice: bool) -> Case:
    """M2: every predicted 4x4 block's vector overwritten.  Pictures 0..: for each border and corner,
    integer offsets that put the 9x9 luma window k = 0..8 samples across it (k = 0: touching, still
    inside), under all 16 phases; the last picture: the level-5.1 limits (8191, 2047), (-8192, -2048)
    and the mixed corners.  References: the generator's, and 0 / 255 patterns."""
    W, H = (6, 4) if bslice else (5, 3)
    cfg = synth.default_cfg(L, 4 if bslice else 3, W, H, num_refs=3, transform8x8=0,
                            **(dict(wp_mode=0, num_slices=4) if bslice else {}))
    PW, PH = 16 * W, 16 * H
    combos = [(b, k, ph) for ph in range(16) for k in range(9) for b in BORDERS]
    npics = 3 if bslice else 8
    pics, at = [], 0
    for i in range(npics):
        p = synth.picture(L, cfg, i)
        if i == npics - 1:
            cnt = [0]

            def mvfn(l, x4, y4, old, cnt=cnt):
                cnt[0] += 1
                return LIMIT_MVS[(cnt[0] + l) % 4]
        else:
            state = [at]

            def mvfn(l, x4, y4, old, state=state):
                b, k, ph = combos[(state[0] * (5 if bslice else 1)) % len(combos)]
                state[0] += 1
                x, y = 4 * x4, 4 * y4
                ix, iy = old[0] >> 2, old[1] >> 2
                # keep the free coordinate's window inside, so that only the named border is crossed
                ix = int(np.clip(ix, 2 - x, PW - 7 - x))
                iy = int(np.clip(iy, 2 - y, PH - 7 - y))
                if b in ("L", "TL", "BL"):
                    ix = 2 - k - x
                if b in ("R", "TR", "BR"):
                    ix = PW - 7 + k - x
                if b in ("T", "TL", "TR"):
                    iy = 2 - k - y
                if b in ("B", "BL", "BR"):
                    iy = PH - 7 + k - y
                return ix * 4 + (ph & 3), iy * 4 + (ph >> 2)
        retile_4x4(p, mvfn)
        if i != npics - 1:
            at = state[0]
        check_bounds(p)
        pics.append(p)
    return Case("m2_borders_b" if bslice else "m2_borders_p", pics,
                pattern_refs(L, cfg, ("generated", "random", "checker1")), info=dict(combos=min(at, len(combos))))


def straddle(p: synth.Picture, x4, y4, mvx, mvy):
    """How far the 9x9 luma window of a 4x4 block crosses each border: {border: samples} for the
    borders it touches or crosses by 0..8 (corner names when it does so on two sides)."""
    PW, PH = 16 * p.cfg.width_mbs, 16 * p.cfg.height_mbs
    x, y = 4 * x4 + (mvx >> 2), 4 * y4 + (mvy >> 2)
    k = {"L": 2 - x, "R": x + 6 - (PW - 1), "T": 2 - y, "B": y + 6 - (PH - 1)}
    return {b: v for b, v in k.items() if 0 <= v <= 8}


# ---------------------------------------------------------------- W: weighted prediction
W_WEIGHTS = (-128, -1, 0, 1, 127)
W_OFFSETS = (-128, 127)
W_COMBOS = [(w, o) for w in W_WEIGHTS for o in W_OFFSETS]


def build_w_explicit_p(L, ref_names=("flat255", "flat0", "random", "random")) -> Case:
    """Explicit P: three slices per picture, logWD 0 / 7 (luma and chroma differing), each of the four
    references of a slice with its own (weight, offset) from W_COMBOS, every 8x8 block's reference
    chosen so that every entry is used."""
    cfg = synth.default_cfg(L, 3, 5, 3, wp_mode=1, num_refs=4, num_slices=3)
    pics = []
    for i in range(4):
        p = synth.picture(L, cfg, i)
        for s, sl in enumerate(p.slices):
            d = (i + s) % 2 * 7
            sl["luma_log2_wd"], sl["chroma_log2_wd"] = d, 7 - d
            for r in range(4):
                kl = ((i * 3 + s) // 2 * 4 + r) % len(W_COMBOS)
                for pl in range(3):
                    w, o = W_COMBOS[(kl + 3 * pl) % len(W_COMBOS)] if pl else W_COMBOS[kl]
                    sl["wp_weight"][0][r][pl], sl["wp_offset"][0][r][pl] = w, o
        retile_4x4(p, reffn=lambda l, x8, y8: (x8 + y8) % 4)
        check_bounds(p)
        pics.append(p)
    return Case("w_explicit_p", pics, pattern_refs(L, cfg, ref_names))


# (weights of list 0, of list 1) per reference, for logWD 0 and for logWD 7 (every pair's sum in -128..127)
W_B_SETS = {0: [((127, -128), (127, -128)), ((-1, 0), (1, 127))],
            7: [((127, 1), (-128, -1)), ((-128, 0), (127, 1))]}


def build_w_explicit_b(L, ref_names=("flat255", "flat0")) -> Case:
    """Explicit B: four slices per picture; bi-prediction pairs (127, 127) and (-128, -128) at logWD 0,
    (127, -128) and (-128, 127) at logWD 7; single-list MBs as the generator draws them."""
    cfg = synth.default_cfg(L, 4, 6, 4, wp_mode=1, num_refs=2, transform8x8=0)
    pics = []
    for i in range(4):
        p = synth.picture(L, cfg, i)
        for s, sl in enumerate(p.slices):
            d = (i + s) % 2 * 7
            sl["luma_log2_wd"], sl["chroma_log2_wd"] = d, 7 - d
            for pl in range(3):
                dd = 7 - d if pl else d
                w0, w1 = W_B_SETS[dd][((i + s) // 2 + (pl > 0)) % 2]
                for r in range(2):
                    sl["wp_weight"][0][r][pl], sl["wp_weight"][1][r][pl] = w0[r], w1[r]
                    sl["wp_offset"][0][r][pl] = W_OFFSETS[(r + s + pl) % 2]
                    sl["wp_offset"][1][r][pl] = W_OFFSETS[(r + i) % 2]
        retile_4x4(p, reffn=lambda l, x8, y8: ((x8 + 2 * y8) >> l) & 1)
        check_bounds(p)
        pics.append(p)
    return Case("w_explicit_b_" + ref_names[0], pics, pattern_refs(L, cfg, ref_names))


def wp_census(case: Case):
    """From the inputs alone: the set of (plane kind, logWD, weight, offset) used by a single-list 8x8
    block, the set of (plane kind, logWD, w0, w1) used by a bi-predicted one, and the smallest and
    largest value wp_apply4 clips (the reference samples taken at the block's integer position)."""
    single, pairs, lo, hi = set(), set(), 0, 255
    for p in case.pics:
        W = p.cfg.width_mbs
        for mi, m in enumerate(p.mbs):
            if int(m["flags"]) & A.MBF_INTRA:
                continue
            sl = p.slices[int(m["slice"])]
            for b8 in range(4):
                x4, y4 = (mi % W) * 4 + (b8 & 1) * 2, (mi // W) * 4 + (b8 >> 1) * 2
                r = [int(p.ref_idx[l, y4, x4]) for l in range(2)]
                for pl in range(3):
                    d = int(sl["chroma_log2_wd" if pl else "luma_log2_wd"])
                    w = [int(sl["wp_weight"][l][max(r[l], 0)][pl]) for l in range(2)]
                    o = [int(sl["wp_offset"][l][max(r[l], 0)][pl]) for l in range(2)]
                    v = []
                    for l in range(2):
                        if r[l] < 0:
                            v.append(None)
                            continue
                        plane = case.refs[int(sl["ref_slot"][l][r[l]])][pl]
                        mx, my = mv_xy(p.mv[l, y4, x4])
                        sx, sy = (4 * x4 + (mx >> 2), 4 * y4 + (my >> 2)) if pl == 0 else (2 * x4 + (mx >> 3), 2 * y4 + (my >> 3))
                        v.append(int(plane[np.clip(sy, 0, plane.shape[0] - 1), np.clip(sx, 0, plane.shape[1] - 1)]))
                    if r[0] >= 0 and r[1] >= 0:
                        pairs.add((pl > 0, d, w[0], w[1]))
                        pre = ((v[0] * w[0] + v[1] * w[1] + (1 << d)) >> (d + 1)) + ((o[0] + o[1] + 1) >> 1)
                    else:
                        l = 0 if r[0] >= 0 else 1
                        single.add((pl > 0, d, w[l], o[l]))
                        pre = ((v[l] * w[l] + (1 << (d - 1))) >> d if d else v[l] * w[l]) + o[l]
                    lo, hi = min(lo, pre), max(hi, pre)
    return single, pairs, lo, hi


# ---------------------------------------------------------------- D: deblocking thresholds
def filter_line(s, alpha, beta, bS, chroma, tc0):
    """8.7.2.3 / 8.7.2.4 on one line of samples across an edge, s = [p3, p2, p1, p0, q0, q1, q2, q3]
    (chroma: [p1, p0, q0, q1]); returns the filtered line."""
    s = [int(v) for v in s]
    n = len(s) // 2
    P = lambda i: s[n - 1 - i]
    Q = lambda i: s[n + i]
    p0, p1, q0, q1 = P(0), P(1), Q(0), Q(1)
    out = list(s)
    if not (bS and abs(p0 - q0) < alpha and abs(p1 - p0) < beta and abs(q1 - q0) < beta):
        return out
    clip = lambda lo, hi, v: max(lo, min(hi, v))
    if chroma:
        if bS == 4:
            out[n - 1], out[n] = (2 * p1 + p0 + q1 + 2) >> 2, (2 * q1 + q0 + p1 + 2) >> 2
        else:
            d = clip(-(tc0 + 1), tc0 + 1, ((q0 - p0) * 4 + (p1 - q1) + 4) >> 3)
            out[n - 1], out[n] = clip(0, 255, p0 + d), clip(0, 255, q0 - d)
        return out
    p2, q2, p3, q3 = P(2), Q(2), P(3), Q(3)
    ap, aq = abs(p2 - p0) < beta, abs(q2 - q0) < beta
    if bS == 4:
        small = abs(p0 - q0) < (alpha >> 2) + 2
        if ap and small:
            out[3], out[2], out[1] = (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3, (p2 + p1 + p0 + q0 + 2) >> 2, (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3
        else:
            out[3] = (2 * p1 + p0 + q1 + 2) >> 2
        if aq and small:
            out[4], out[5], out[6] = (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3, (p0 + q0 + q1 + q2 + 2) >> 2, (2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3
        else:
            out[4] = (2 * q1 + q0 + p1 + 2) >> 2
        return out
    tc = tc0 + ap + aq
    d = clip(-tc, tc, ((q0 - p0) * 4 + (p1 - q1) + 4) >> 3)
    out[3], out[4] = clip(0, 255, p0 + d), clip(0, 255, q0 - d)
    if ap:
        out[2] = p1 + clip(-tc0, tc0, (p2 + ((p0 + q0 + 1) >> 1) - 2 * p1) >> 1)
    if aq:
        out[5] = q1 + clip(-tc0, tc0, (q2 + ((p0 + q0 + 1) >> 1) - 2 * q1) >> 1)
    return out


def classify(s, alpha, beta, bS, chroma, tc0):
    """What one designed line exercises, from its samples and parameters alone."""
    n = len(s) // 2
    p = [int(s[n - 1 - i]) for i in range(n)]
    q = [int(s[n + i]) for i in range(n)]
    c = dict(step=abs(p[0] - q[0]), dp1=abs(p[1] - p[0]), dq1=abs(q[1] - q[0]))
    c["on"] = bool(bS) and c["step"] < alpha and c["dp1"] < beta and c["dq1"] < beta
    if not chroma:
        c["ap"], c["aq"] = abs(p[2] - p[0]), abs(q[2] - q[0])
    if c["on"] and bS < 4:
        tc = tc0 + 1 if chroma else tc0 + (c["ap"] < beta) + (c["aq"] < beta)
        raw = ((q[0] - p[0]) * 4 + (p[1] - q[1]) + 4) >> 3
        c["tc"] = tc
        c["clip"] = 1 if raw > tc else -1 if raw < -tc else 0
        d = max(-tc, min(tc, raw))
        c["clamp"] = 255 if (p[0] + d > 255 or q[0] - d > 255) else 0 if (p[0] + d < 0 or q[0] - d < 0) else None
    return c


def luma_designs(alpha, beta, bS, base, sgn):
    """Lines [p3 .. q3] around `base` (offsets times sgn) on the thresholds of one edge: |p0 - q0| at
    alpha - 1, alpha, alpha + 1 (both polarities: the delta clips at + tc and - tc); |p1 - p0| and
    |q1 - q0| at beta - 1 and beta; |p2 - p0| and |q2 - q0| at beta - 1 / beta in the four
    combinations; bS 4: |p0 - q0| at (alpha >> 2) + 1, + 2, + 3 under the same four, p3 and q3 distinct."""
    out = []

    def add(*off):
        v = [base + sgn * o for o in off]
        shift = max(0, -min(v)) - max(0, max(v) - 255)        # a line too tall for its base moves as a whole
        v = [x + shift for x in v]
        if min(v) >= 0 and max(v) <= 255:
            out.append(v)
    for s in (alpha - 1, alpha, alpha + 1):
        add(0, 0, 0, 0, s, s, s, s)
        add(s, s, s, s, 0, 0, 0, 0)
    for t in (beta - 1, beta):
        add(t, t, t, 0, 1, 1, 1, 1)
        add(0, 0, 0, 0, 1, 1 + t, 1 + t, 1 + t)
    steps = ((alpha >> 2) + 1, (alpha >> 2) + 2, (alpha >> 2) + 3) if bS == 4 else (2,)
    for s in steps:
        for a in (beta - 1, beta):
            for b in (beta - 1, beta):
                add(a + 3, a, 1, 0, s, s + 1, s + b, s + b + 4)
                add(-a - 3, -a, -1, 0, s, s - 1, s - b, s - b - 4)
    return out


def chroma_designs(alpha, beta, base, sgn):
    out = []

    def add(*off):
        v = [base + sgn * o for o in off]
        shift = max(0, -min(v)) - max(0, max(v) - 255)        # a line too tall for its base moves as a whole
        v = [x + shift for x in v]
        if min(v) >= 0 and max(v) <= 255:
            out.append(v)
    for s in (alpha - 1, alpha, alpha + 1):
        add(0, 0, s, s)
        add(s, s, 0, 0)
    for t in (beta - 1, beta):
        add(t, 0, 1, 1)
        add(0, 0, 1, 1 + t)
        add(1, 0, 3, 3 + t - 1)
    return out


# lines that reach 0 and 255 whatever the thresholds: clamp255 on p0 + d and on q0 - d, and at 0
CLAMP_LINES = [[255, 255, 255, 255, 255, 251, 251, 251], [251, 251, 251, 255, 255, 255, 255, 255],
               [0, 0, 0, 0, 0, 4, 4, 4], [4, 4, 4, 0, 0, 0, 0, 0],
               [255, 255, 255, 255, 254, 250, 250, 250], [0, 0, 0, 0, 1, 5, 5, 5]]


def qpc_of(qp, off=0):
    """QPc of 8.5.8 / Table 8-15 for QPY `qp` under chroma_qp_index_offset `off` (-12..12)."""
    return QP_C[min(51, max(0, int(qp) + int(off)))]


def _set_qp(m, qp, offs=(0, 0)):
    """qp_y and the two chroma QPs it implies under (chroma_qp_index_offset, second_chroma_qp_index_offset)."""
    assert all(-12 <= o <= 12 for o in offs)
    m["qp_y"], m["qp_scaled"][0] = qp, qp
    for pl in range(2):
        m["qp_c"][pl] = m["qp_scaled"][1 + pl] = qpc_of(qp, offs[pl])


def build_d(L, kind: str, horizontal: bool, grids, name: str, idc: int = 1, structures=None) -> Case:
    """Pictures whose samples before the loop filter are known by construction: every MB is an inter
    MB with zero motion (it copies the crafted plane held by every DPB slot, minus the flat
    residual of its DC-only coded blocks) or an I_PCM MB (its samples are the crafted plane's), and
    every line across a filtered MB edge is one of luma_designs / chroma_designs for that edge's
    alpha and beta.  Built for vertical edges in a logical picture and transposed for horizontal ones.

    kind "bs1": neighbouring MBs reference different DPB slots holding identical planes (bS 1 on
      every MB edge across the filter direction, 0 elsewhere); any QP.
    kind "mix": adjacent 4-line segments of an edge with different bS: 0 / 1 from the 8x8 blocks'
      references, 2 from DC-only coded blocks on either side.  Segments alternate between a dark and a
      bright band more than alpha apart, which keeps every edge along the other direction (and the
      coded blocks' inner edges) off; QP up to 36 (alpha <= 50).
    kind "pcm": I_PCM MBs (QP 0) between inter MBs: bS 4 on the MB edges, the strong filter's
      thresholds.
    grids: per picture (FilterOffsetA, FilterOffsetB, QP per logical MB [rows][columns]) and, for the
    cases of tests/extremes_d2.py, the chroma QP offsets (Cb, Cr) and the picture's own kind.
    idc 3 (4:4:4): Cb and Cr are full-size planes whose lines are luma_designs under each plane's own
    alpha / beta.  structures: per picture A.FRAME or a field parity; a field picture's crafted planes
    sit in its own parity's rows of the two DPB frames (the other parity's field would be read with a
    chroma offset), and its horizontal intra MB edges have bS 3."""
    Wl, Hl = (3, 5) if horizontal else (5, 3)
    quant = O.quant_flat()[0]
    pics, lines, refs_all, design = [], [], None, []
    kind0 = kind
    cm = 16 if idc == 3 else 8              # chroma samples per MB, along both axes
    for pi, g in enumerate(grids):
        offa, offb, grid = g[:3]
        offs = g[3] if len(g) > 3 else (0, 0)
        kind = g[4] if len(g) > 4 else kind0
        structure = structures[pi % len(structures)] if structures else A.FRAME
        fld = structure != A.FRAME
        assert not (idc == 3 and (kind == "mix" or fld)) and not (fld and kind == "mix")
        # one DPB for the case: picture pi's crafted plane sits in slots 2 pi and 2 pi + 1
        over = dict(num_refs=2 * len(grids), filter_offset_a=offa, filter_offset_b=offb)
        if idc == 3:
            over["chroma_format"] = 3
        if fld:
            over.update(structure=structure, num_refs=4 * len(grids))       # fields: 2 len(grids) frames
        cfg = synth.default_cfg(L, 3, 5, 3, **over)
        p = synth.picture(L, cfg, pi)
        if fld:
            par = A.REF_BOTTOM if structure == A.BOTTOM_FIELD else 0
            for sl in p.slices:
                sl["ref_slot"][:] = -1
                sl["ref_slot"][0][:2] = [2 * pi | par, (2 * pi + 1) | par]
                sl["num_ref"][0] = 2
            entry = [0, 1]
        else:
            entry = [[int(v) for v in p.slices["ref_slot"][0][0]].index(s) for s in (2 * pi, 2 * pi + 1)]
        Y = np.full((16 * Hl, 16 * Wl), 128, np.int64)
        C = [np.full((cm * Hl, cm * Wl), 128, np.int64) for _ in range(2)]
        res = np.zeros_like(Y)                     # residual of the coded blocks
        mbs = np.zeros((Hl, Wl), A.MB_DTYPE)
        ref8 = np.zeros((2 * Hl, 2 * Wl), np.int8)
        pcm = np.zeros((Hl, Wl), bool)
        coded = np.zeros((4 * Hl, 4 * Wl), np.int16)       # DC-only level of a 4x4 block, 0 = not coded
        banded = kind == "mix"
        for cy in range(Hl):
            for cx in range(Wl):
                m = mbs[cy, cx]
                m["mb_type"] = A.P_16x16
                _set_qp(m, int(grid[cy][cx]), offs)
                ref8[2 * cy:2 * cy + 2, 2 * cx:2 * cx + 2] = cx & 1 if kind != "pcm" else 0
                if kind == "pcm" and cx & 1:
                    pcm[cy, cx] = True
                    m["mb_type"], m["flags"], m["cbp_blks"] = A.I_PCM, A.MBF_INTRA, 0xFFFF
                    _set_qp(m, 0, offs)
        # the bS of each 4-line segment of each vertical MB edge
        seg_bs = np.zeros((4 * Hl, Wl), np.int64)
        for cy in range(Hl):
            for cx in range(1, Wl):
                if kind == "bs1":
                    seg_bs[4 * cy:4 * cy + 4, cx] = 1
                elif kind == "pcm":
                    seg_bs[4 * cy:4 * cy + 4, cx] = 3 if fld and horizontal else 4
                else:
                    pat = [(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (1, 0, 2), (2, 1, 0)][(cx + 2 * cy + pi) % 6]
                    pat = [pat[0], pat[1], pat[2], pat[(cx + cy) % 3]]
                    # 0 / 1: an 8x8 block's reference equal to / other than its left neighbour's (one
                    # reference per 8 lines: segments 0, 1 and 2, 3 share it unless a coded block gives 2)
                    for half in range(2):
                        want = [b for b in pat[2 * half:2 * half + 2] if b != 2]
                        same = (want[0] if want else 0) == 0
                        if len(want) == 2 and want[0] != want[1]:
                            pat[2 * half + 1] = 2
                        left = ref8[2 * cy + half, 2 * cx - 1]
                        ref8[2 * cy + half, 2 * cx:2 * cx + 2] = left if same else 1 - left
                    mbs[cy, cx]["mb_type"] = A.P_8x8
                    for k in range(4):
                        if pat[k] == 2:            # coded on the q side, or on the p side
                            if (k + cx) & 1:
                                coded[4 * cy + k, 4 * cx] = 1
                            else:
                                coded[4 * cy + k, 4 * cx - 1] = 1
                        seg_bs[4 * cy + k, cx] = pat[k]
        # the lines
        for cx in range(1, Wl):
            x = 16 * cx
            n_line = 0
            for yy in range(16 * Hl):
                cy, seg = yy // 16, yy // 4
                bS = int(seg_bs[seg, cx])
                mp, mq = mbs[cy, cx - 1], mbs[cy, cx]
                qpav = (int(mp["qp_y"]) + int(mq["qp_y"]) + 1) >> 1
                ia, ib = int(np.clip(qpav + offa, 0, 51)), int(np.clip(qpav + offb, 0, 51))
                alpha, beta = ALPHA[ia], BETA[ib]
                tc0 = TC0[ia][bS - 1] if 0 < bS < 4 else 0
                hi = banded and seg & 1
                base, sgn = (235, -1) if hi else (20, 1)
                if not banded:
                    base, sgn = ((20, 1), (235, -1), (90, 1), (170, -1))[(yy + cx) % 4]
                ds = luma_designs(alpha, beta, bS if bS else 1, base, sgn)
                if not banded:
                    ds += CLAMP_LINES
                if banded:
                    ds = [d for d in ds if (min(d) >= 175 if hi else max(d) <= 80)]
                line = ds[(yy % 16 + 16 * ((pi + cx + cy) % 3)) % len(ds)] if ds else [base] * 8     # an MB's 16 lines: one third of the designs
                n_line += 1
                Y[yy, x - 4:x + 4] = line
                if banded:
                    # beyond the line: a value more than alpha from its ends, so that a coded block's
                    # inner edge (bS 2, at x +- 4) stays off
                    Y[yy, x - 8:x - 4] = 255 if line[0] < 128 else 0
                    Y[yy, x + 4:x + 8] = 255 if line[7] < 128 else 0
                lines.append(dict(pic=pi, plane=0, edge=x, at=yy, bS=bS, alpha=alpha, beta=beta, tc0=tc0, line=line))
            for pl in range(2):
                n_line = 0
                for yc in range(cm * Hl):
                    cy, seg = yc // cm, yc * (16 // cm) // 4
                    bS = int(seg_bs[seg, cx])
                    mp, mq = mbs[cy, cx - 1], mbs[cy, cx]
                    qpav = (int(mp["qp_c"][pl]) + int(mq["qp_c"][pl]) + 1) >> 1
                    ia, ib = int(np.clip(qpav + offa, 0, 51)), int(np.clip(qpav + offb, 0, 51))
                    alpha, beta = ALPHA[ia], BETA[ib]
                    tc0 = TC0[ia][bS - 1] if 0 < bS < 4 else 0
                    hi = banded and seg & 1
                    base, sgn = (235, -1) if hi else (20, 1)
                    if not banded:
                        base, sgn = ((20, 1), (235, -1), (90, 1), (170, -1))[(yc + cx + pl) % 4]
                    if idc == 3:
                        ds = luma_designs(alpha, beta, bS if bS else 1, base, sgn) + CLAMP_LINES
                    else:
                        ds = chroma_designs(alpha, beta, base, sgn)
                        if not banded:
                            ds += [c[2:6] for c in CLAMP_LINES]
                        else:
                            ds = [d for d in ds if (min(d) >= 175 if hi else max(d) <= 80)]
                    line = ds[(yc % cm + cm * ((pi + cx + cy + pl) % 3)) % len(ds)] if ds else [base] * 4
                    n_line += 1
                    C[pl][yc, cm * cx - len(line) // 2:cm * cx + len(line) // 2] = line
                    if banded:
                        C[pl][yc, 8 * cx - 4:8 * cx - 2] = line[0]
                        C[pl][yc, 8 * cx + 2:8 * cx + 4] = line[3]
                    lines.append(dict(pic=pi, plane=1 + pl, edge=cm * cx, at=yc, bS=bS, alpha=alpha, beta=beta, tc0=tc0,
                                      line=line))
        if banded:          # the MBs' first and last columns lie in no line: give them their band too
            for yy in range(16 * Hl):
                v = 235 if (yy // 4) & 1 else 20
                Y[yy, 0:8], Y[yy, 16 * Wl - 8:] = v, v
                for pl in range(2):
                    C[pl][yy // 2, 0:4], C[pl][yy // 2, 8 * Wl - 4:] = v, v
        # the coded blocks: a DC-only level whose flat residual the reference plane is short of
        for by in range(4 * Hl):
            for bx in range(4 * Wl):
                if not coded[by, bx]:
                    continue
                qp = int(mbs[by // 4, bx // 4]["qp_y"])
                blk = Y[4 * by:4 * by + 4, 4 * bx:4 * bx + 4]
                for lev in (1, -1, 2, -2):
                    r = (dq4(lev, quant["scale4x4"][1][0][qp % 6][0], qp // 6) + 32) >> 6
                    if r != 0 and 0 <= blk.min() - r and blk.max() - r <= 255:
                        break
                else:
                    raise AssertionError("no DC level fits")
                coded[by, bx] = lev
                res[4 * by:4 * by + 4, 4 * bx:4 * bx + 4] = r
        # realise: records, levels, motion, planes (transposed for horizontal edges)
        T = (lambda a: np.ascontiguousarray(a.T)) if horizontal else (lambda a: np.ascontiguousarray(a))
        W, H = 5, 3
        pool, recs = [], np.zeros(W * H, A.MB_DTYPE)
        ref4 = np.repeat(np.repeat(ref8, 2, 0), 2, 1)
        for cy in range(Hl):
            for cx in range(Wl):
                m = mbs[cy, cx].copy()
                px, py = (cy, cx) if horizontal else (cx, cy)
                m["coef_off"] = sum(len(a) for a in pool)
                if pcm[cy, cx]:
                    raw = np.concatenate([T(Y[16 * cy:16 * cy + 16, 16 * cx:16 * cx + 16]).ravel()] +
                                         [T(C[pl][cm * cy:cm * cy + cm, cm * cx:cm * cx + cm]).ravel() for pl in range(2)])
                    pool.append(raw.astype(np.uint8).view(np.int16))
                else:
                    cb = coded[4 * cy:4 * cy + 4, 4 * cx:4 * cx + 4]
                    cbt = cb.T if horizontal else cb
                    cbp = blks = 0
                    for q in range(4):
                        sub = cbt[(q >> 1) * 2:(q >> 1) * 2 + 2, (q & 1) * 2:(q & 1) * 2 + 2]
                        if not sub.any():
                            continue
                        cbp |= 1 << q
                        lv = np.zeros(64, np.int16)
                        for b4 in range(4):
                            lv[b4 * 16] = sub[b4 >> 1, b4 & 1]
                            if lv[b4 * 16]:
                                blks |= 1 << (((q >> 1) * 2 + (b4 >> 1)) * 4 + (q & 1) * 2 + (b4 & 1))
                        pool.append(lv)
                    m["cbp"], m["cbp_blks"] = cbp, blks
                recs[py * W + px] = m
        p.mbs[:] = recs
        p.levels = np.concatenate(pool + [np.zeros(8 + (128 if idc == 3 else 0), np.int16)])     # (4:4:4: include/h264r.h)
        p.mv[:] = 0
        p.ref_idx[0] = np.array(entry, np.int8)[T(ref4)]
        p.ref_idx[1] = -1
        for mi, m in enumerate(p.mbs):                  # an intra MB predicts from no list
            if int(m["flags"]) & A.MBF_INTRA:
                p.ref_idx[0, 4 * (mi // W):4 * (mi // W) + 4, 4 * (mi % W):4 * (mi % W) + 4] = -1
        check_bounds(p)
        planes = tuple(T(a).astype(np.uint8) for a in (Y - res, C[0], C[1]))
        want = tuple(T(a).astype(np.uint8) for a in (Y, C[0], C[1]))
        if fld:                 # the crafted field in its parity's rows of two DPB frames, poison in the other rows
            frames = tuple(np.full((2 * a.shape[0], a.shape[1]), 77, np.uint8) for a in planes)
            for f, a in zip(frames, planes):
                f[int(structure == A.BOTTOM_FIELD)::2] = a
            planes = frames
        if refs_all is None:
            refs_all = [tuple(np.zeros_like(a) for a in planes) for _ in range(2 * len(grids))]
        refs_all[2 * pi] = refs_all[2 * pi + 1] = planes
        got = O.decode(p, refs_all, stage="recon")
        for k in range(3):
            assert np.array_equal(got[k], want[k]), f"{name}[{pi}] plane {k}: the reconstruction is not the crafted plane"
        pics.append(p)
        qy = p.mbs["qp_y"].reshape(H, W).astype(np.int64)
        design.append(dict(want=want, qp_y=qy, qp_c=[p.mbs["qp_c"][:, pl].reshape(H, W).astype(np.int64) for pl in range(2)],
                           offa=offa, offb=offb, offs=offs, kind=kind, structure=structure))
    # a line's position in the picture's planes: `edge` along x (vertical edges) or along y
    return Case(name, pics, refs_all, chroma_format=idc, info=dict(lines=lines, horizontal=horizontal, design=design))


# FilterOffsetA / B and the QP of each logical MB [rows][columns]: indexA 16 (the first non-zero alpha),
# mid-range and 51, reached with QPs that differ across the edge and with offsets +-12 (both clips)
D_GRIDS = [
    (0, 0, [[16, 16, 24, 36, 51], [17, 20, 30, 40, 51], [16, 18, 33, 45, 50]]),
    (12, -12, [[4, 5, 30, 40, 51], [3, 4, 26, 44, 48], [10, 12, 20, 39, 51]]),
    (-12, 12, [[28, 28, 40, 51, 51], [27, 30, 45, 50, 51], [29, 33, 36, 48, 51]]),
]
D_GRIDS_MIX = [
    (0, 0, [[16, 16, 24, 30, 36], [17, 20, 28, 33, 35], [22, 18, 26, 31, 36]]),
    (6, -6, [[10, 10, 20, 26, 30], [12, 14, 22, 28, 29], [11, 16, 24, 27, 30]]),
]
D_GRIDS_PCM = [
    (0, 0, [[31, 0, 40, 0, 51], [32, 0, 44, 0, 50], [36, 0, 47, 0, 51]]),
    (12, 12, [[7, 0, 30, 0, 51], [8, 0, 36, 0, 45], [12, 0, 40, 0, 51]]),
]


def _grids(grids, horizontal):
    """The logical picture of horizontal edges is 3 columns by 5 rows: the grids transposed."""
    return [(a, b, [list(r) for r in zip(*g)] if horizontal else g) for a, b, g in grids]


def build_d_case(L, kind: str, horizontal: bool) -> Case:
    grids = {"bs1": D_GRIDS, "mix": D_GRIDS_MIX, "pcm": D_GRIDS_PCM}[kind]
    return build_d(L, kind, horizontal, _grids(grids, horizontal), f"d_{kind}_{'h' if horizontal else 'v'}")


# ---------------------------------------------------------------- the cases
def _patterns(names):
    return lambda L, cfg: pattern_refs(L, cfg, names)


CASES = {
    # R: residual
    "r1_at_bound": lambda L: build_r_luma(L, False, False),
    "r2_over": lambda L: build_r_luma(L, True, False),
    "r3_flat_at_bound": lambda L: build_r_luma(L, False, True),
    "r3_flat_over": lambda L: build_r_luma(L, True, True),
    "r4_chroma_at_bound": lambda L: build_r_chroma(L, False),
    "r4_chroma_over": lambda L: build_r_chroma(L, True),
    "r5_amplified_intra": lambda L: build_r_amplified(L, 2, 5, 3, 3),
    "r5_amplified_b": lambda L: build_r_amplified(L, 4, 6, 4, 3),
    # M: motion compensation
    "m1_stripes": lambda L: build_m_patterns(L, ("stripe_x", "stripe_x_inv", "stripe_y", "stripe_y_inv"), "m1_stripes"),
    "m1_outer_random": lambda L: build_m_patterns(L, ("outer_max", "outer_min", "xnor", "xor", "random"), "m1_outer_random"),
    "m1_flat_checker_b": lambda L: build_m_patterns(L, ("flat0", "flat255", "checker2", "random"), "m1_flat_checker_b",
                                                    cidx=4, W=6, H=4, n=3, wp_mode=0),
    "m2_borders_p": lambda L: build_m_borders(L, False),
    "m2_borders_b": lambda L: build_m_borders(L, True),
    # W: explicit weighted prediction
    "w_explicit_p": lambda L: build_w_explicit_p(L),
    "w_explicit_b_flat": lambda L: build_w_explicit_b(L, ("flat255", "flat0")),
    "w_explicit_b_random": lambda L: build_w_explicit_b(L, ("random", "flat255")),
    # D: deblocking thresholds
    "d_bs1_v": lambda L: build_d_case(L, "bs1", False), "d_bs1_h": lambda L: build_d_case(L, "bs1", True),
    "d_mix_v": lambda L: build_d_case(L, "mix", False), "d_mix_h": lambda L: build_d_case(L, "mix", True),
    "d_pcm_v": lambda L: build_d_case(L, "pcm", False), "d_pcm_h": lambda L: build_d_case(L, "pcm", True),
    # kernels with their own code: M1 patterns + R5 through k_mbaff and k_chroma422
    "x_mbaff_p": lambda L: build_r_amplified(L, 3, 6, 4, 2, refs=_patterns(("outer_max", "random")), name="x_mbaff_p",
                                             structure=A.MBAFF_FRAME, wp_mode=0),
    "x_422_p": lambda L: build_r_amplified(L, 3, 5, 3, 2, refs=_patterns(("outer_max", "random")), name="x_422_p",
                                           chroma_format=2),
}
D_CASES = [n for n in CASES if n.startswith("d_")]
_built = {}


def build(name: str) -> Case:
    """The case, built once per process (everything is seeded: two builds are byte-identical)."""
    if name not in _built:
        c = CASES[name](O.lib())
        c.name = name
        assert len(c.pics) <= 8
        _built[name] = c
    return _built[name]


def digests(c: Case) -> dict:
    return dict(inputs=[synth.input_digest(p) for p in c.pics], refs=refs_digest(c.refs))


# ---------------------------------------------------------------- M: what the blocks actually predicted reach
def uses(xf, yf):
    """Which of the unrounded intermediates a phase's samples are made of (8.4.2.2.1)."""
    b = (yf == 0 and xf != 0) or (xf != 0 and yf in (1, 3))
    h = (xf == 0 and yf != 0) or (yf != 0 and xf in (1, 3))
    j = (xf == 2 and yf != 0) or (yf == 2 and xf != 0)
    return b, h, j


def mc_census(c: Case) -> dict:
    """Over the 4x4 blocks the case predicts: extremes of the unrounded b1 / h1 / j1 that the block's
    phase uses, whether their rounded values are clipped at each end, rounding ties of j, the phases
    met per DPB slot, and how far the luma and chroma windows cross each border."""
    r = dict(b=[0, 0], h=[0, 0], j=[0, 0], bclip=set(), jclip=set(), ties=0, phases={}, straddle=set(),
             straddle_phase=set(), corner=set(), chroma=set(), mvs=set())
    for p in c.pics:
        PW, PH = 16 * p.cfg.width_mbs, 16 * p.cfg.height_mbs
        for l, x4, y4, slot, mx, my in predicted_blocks(p):
            xf, yf = mx & 3, my & 3
            r["phases"].setdefault(slot, set()).add((xf, yf))
            r["mvs"].add((mx, my))
            st = straddle(p, x4, y4, mx, my)
            for bx in "LR":
                for by in "TB":
                    if bx in st and by in st and st[bx] == st[by]:
                        r["corner"].add((by + bx, st[bx], xf * 4 + yf))
            for bd, k in st.items():
                r["straddle"].add((bd, k))
                r["straddle_phase"].add((bd, xf * 4 + yf))
            xc, yc = 2 * x4 + (mx >> 3), 2 * y4 + (my >> 3)
            for bd, k in (("L", -xc), ("R", xc + 2 - (PW // 2 - 1)), ("T", -yc), ("B", yc + 2 - (PH // 2 - 1))):
                if 0 <= k <= 2:
                    r["chroma"].add((bd, k))
            ub, uh, uj = uses(xf, yf)
            if not (ub or uh or uj):
                continue
            b1, h1, j1 = luma_taps(c.refs[slot][0], 4 * x4 + (mx >> 2), 4 * y4 + (my >> 2))
            if ub:
                bb = b1[2 + (yf == 3):6 + (yf == 3)]
                r["b"] = [min(r["b"][0], int(bb.min())), max(r["b"][1], int(bb.max()))]
                r["bclip"] |= ({0} if ((bb + 16) >> 5).min() < 0 else set()) | ({255} if ((bb + 16) >> 5).max() > 255 else set())
            if uh:
                hh = h1[:, (xf == 3):4 + (xf == 3)]
                r["h"] = [min(r["h"][0], int(hh.min())), max(r["h"][1], int(hh.max()))]
            if uj:
                r["j"] = [min(r["j"][0], int(j1.min())), max(r["j"][1], int(j1.max()))]
                v = (j1 + 512) >> 10
                r["jclip"] |= ({0} if v.min() < 0 else set()) | ({255} if v.max() > 255 else set())
                r["ties"] += int((((j1 + 512) % 1024 == 0) & (v >= 1) & (v <= 255)).sum())
    return r


def luma_blocks(p: synth.Picture, quant):
    """(MB index, dequantised coefficients [4][4]) of every coded 4x4 luma block of the inter MBs
    that take the packed-residual test."""
    for mi in _inter4_mbs(p):
        m = p.mbs[mi]
        qp = int(m["qp_scaled"][0])
        sc = quant["scale4x4"][1][0][qp % 6]
        for q in layout(m)[0]:
            if q is None:
                continue
            for b4 in range(4):
                o = int(m["coef_off"]) + q + b4 * 16
                yield mi, [[dq4(p.levels[o + 4 * r + c], sc[4 * r + c], qp // 6) for c in range(4)] for r in range(4)]


def one_mb(p: synth.Picture, mi: int) -> synth.Picture:
    """A view of p holding MB mi alone (for wave_sums of one MB)."""
    return synth.Picture(p.cfg, p.index, p.mbs[mi:mi + 1], p.levels, p.mv, p.ref_idx, p.slices, p.pic)


# ---------------------------------------------------------------- D, every edge: inner edges, bS 3, Intra_16x16, 8x8 transform
def deblock_restate(planes, W, H, qp_y, qp_c, bsV, bsH, offa, offb, log=None, probe=None, idc=1, wrong=()):
    """8.7 on a whole picture given the bS of every edge segment, in Python integers: per MB in raster
    order the vertical edges left to right, then the horizontal ones, luma and chroma.
    planes: [Y, Cb, Cr] int arrays, filtered in place.  qp_y [H][W]; qp_c [H][W], or one such grid per
    chroma plane; bsV[by][bx] the bS of the vertical edge left of 4x4 block (bx, by), bsH[by][bx] of the
    horizontal edge above it (0: not filtered).
    idc, the chroma geometry: 1 (4:2:0) an MB's chroma is 8 x 8, edges 0 and 2 of either direction at
    chroma offsets 0 and 4, a line taking the bS of the luma line twice as far along the edge; 2
    (4:2:2) 8 wide and 16 high: vertical edges at columns 0 and 4 of 16 lines each, line y under the bS
    of luma row y >> 2 of luma edges 0 and 2, and FOUR horizontal edges at rows 0, 4, 8, 12, edge e
    under bsH of luma edge e at luma column 2 x; 3 (4:4:4) Cb and Cr are filtered as luma is, on every
    luma edge with the luma's bS, under alpha / beta of their own QPs.
    log(plane, vertical, inner, mb, bS, alpha, beta, tc0, line before): one call per line.
    probe(plane, vertical, (x, y) of q0, bS, alpha, beta, indexA, line before): one call per line of
    every edge the walk meets, those of bS 0 included.
    wrong: names of deliberate mistakes, for the mutation checks of tests/test_extremes.py:
    "swap_planes" (Cb under Cr's QP and the reverse), "qpc_from_qpy" (both planes under QP_C[qp_y]),
    "q_side_qp" (the q side's QP instead of the average), "422_v_row_half" (4:2:2 vertical chroma bS
    from luma row y >> 1), "422_h_drop" (4:2:2 chroma rows 4 and 12 not filtered), "444_chroma_filter"
    (4:4:4 Cb / Cr through the chroma filter)."""
    qp_c = np.asarray(qp_c)
    qp_c = [qp_c, qp_c] if qp_c.ndim == 2 else [qp_c[0], qp_c[1]]
    cw, ch = {1: (8, 8), 2: (8, 16), 3: (16, 16)}[idc]

    def qp_at(pl, y, x):
        if pl == 0:
            return int(qp_y[y][x])
        if "qpc_from_qpy" in wrong:
            return QP_C[int(qp_y[y][x])]
        return int(qp_c[2 - pl if "swap_planes" in wrong else pl - 1][y][x])
    for my in range(H):
        for mx in range(W):
            for vertical in (True, False):
                for e in range(4):
                    if e == 0 and (mx == 0 if vertical else my == 0):
                        continue
                    px, py = (mx - (e == 0), my) if vertical else (mx, my - (e == 0))
                    for pl in range(3):
                        like_luma = pl == 0 or idc == 3
                        four = idc == 2 and pl and not vertical         # 4:2:2: a chroma edge per luma edge
                        if not like_luma and e & 1 and not (four and "422_h_drop" not in wrong):
                            continue
                        qpav = (qp_at(pl, py, px) + qp_at(pl, my, mx) + 1) >> 1
                        if "q_side_qp" in wrong:
                            qpav = qp_at(pl, my, mx)
                        ia, ib = min(51, max(0, qpav + offa)), min(51, max(0, qpav + offb))
                        mw, mh = (16, 16) if like_luma else (cw, ch)
                        n = 4 if like_luma else 2
                        pos = 4 * e if like_luma or four else 2 * e
                        size = mh if vertical else mw
                        img = planes[pl]
                        for k in range(size):
                            seg = k * 16 // size // 4
                            if idc == 2 and pl and vertical and "422_v_row_half" in wrong:
                                seg = (k >> 1) & 3
                            bS = int(bsV[4 * my + seg][4 * mx + e]) if vertical else int(bsH[4 * my + e][4 * mx + seg])
                            if not bS and probe is None:
                                continue
                            if vertical:
                                y, x = mh * my + k, mw * mx + pos
                                line = [int(v) for v in img[y, x - n:x + n]]
                            else:
                                y, x = mh * my + pos, mw * mx + k
                                line = [int(v) for v in img[y - n:y + n, x]]
                            if probe:
                                probe(pl, vertical, (x, y), bS, ALPHA[ia], BETA[ib], ia, line)
                            if not bS:
                                continue
                            tc0 = TC0[ia][bS - 1] if bS < 4 else 0
                            if log:
                                log(pl, vertical, e > 0, (mx, my), bS, ALPHA[ia], BETA[ib], tc0, line)
                            if idc == 3 and pl and "444_chroma_filter" in wrong:
                                out = line[:2] + filter_line(line[2:6], ALPHA[ia], BETA[ib], bS, True, tc0) + line[6:]
                            else:
                                out = filter_line(line, ALPHA[ia], BETA[ib], bS, not like_luma, tc0)
                            if vertical:
                                img[y, x - n:x + n] = out
                            else:
                                img[y - n:y + n, x] = out
    return planes


D_KINDS0 = "PTPCP"          # the first logical MB row (no Intra_16x16 vertical prediction there)
D_KINDS = "IPTIP"
# FilterOffsetA / B and the QP range per picture: indexA at 51 and clipped from both sides, mid-range, low;
# the last reaches index 51 for chroma too (QPc ends at 39)
D_EVERY = [(0, 0, 44, 51), (0, 0, 28, 40), (6, -6, 16, 30), (-12, 12, 40, 51), (12, -12, 30, 45), (12, 6, 44, 51)]


def build_d_every(L, horizontal: bool, name=None, offs=None, idc: int = 1) -> Case:
    """Threshold lines on EVERY luma and chroma edge of the filter direction, inner ones included, in
    pictures mixing: P_8x8 MBs whose 8x8 columns alternate between two DPB slots with identical planes
    (bS 1 on MB edges and on the inner 8x8 edge) and DC-only coded 4x4 blocks (bS 2, any QP);
    P_16x16 MBs with the 8x8 transform and DC-only coded 8x8 blocks (bS 2 on edges 0 and 2, the 4x4
    inner edges not filtered); Intra_16x16 MBs with vertical prediction, cbp 0 and zero DC levels,
    which copy the bottom row of the crafted MB above at any QP (bS 4 on MB edges with alpha up to
    255, bS 3 inside); an I_PCM MB.  The plane is a row of 4-sample cells: across each edge
    |p0 - q0| takes alpha - 1, alpha, alpha + 1, (alpha >> 2) + 1 .. + 3 and small values, |p1 - p0|
    and |q1 - q0| take 0, beta - 1, beta.  The edges of the other direction are filtered too, on
    whatever the rows hold: the census restates the whole loop filter (deblock_restate) from the
    designed bS of every segment.  Logical picture, transposed for horizontal edges (the prediction
    is then horizontal).
    The cases of tests/extremes_d2.py: offs, per picture the chroma QP offsets (Cb, Cr), each chroma
    plane crafted on the thresholds of its own QPc; idc 2 (4:2:2: no 8x8 transform, its MBs become
    P_8x8 ones; an MB's chroma is 8 x 16, so a horizontal case has four chroma edges per MB) and idc 3
    (4:4:4: Cb and Cr crafted like luma; the coded blocks' levels are luma's alone)."""
    Wl, Hl = (3, 5) if horizontal else (5, 3)
    W, H = 5, 3
    pics, refs_all, design = [], None, []
    # an MB's chroma in the logical picture: (cells of 4 samples along x, rows)
    ccell, crow = {1: (2, 8), 2: (4, 8) if horizontal else (2, 16), 3: (4, 16)}[idc]
    for pi, (offa, offb, qlo, qhi) in enumerate(D_EVERY):
        co = offs[pi] if offs else (0, 0)
        over = dict(num_refs=2 * len(D_EVERY), filter_offset_a=offa, filter_offset_b=offb, transform8x8=int(idc != 2))
        if idc != 1:
            over["chroma_format"] = idc
        cfg = synth.default_cfg(L, 3, W, H, **over)
        p = synth.picture(L, cfg, pi)
        entry = [[int(v) for v in p.slices["ref_slot"][0][0]].index(s) for s in (2 * pi, 2 * pi + 1)]
        kind = [[(D_KINDS0[(cx + pi) % 5] if cy == 0 else D_KINDS[(cx + cy + pi) % 5]) for cx in range(Wl)] for cy in range(Hl)]
        if idc == 2:
            kind = [[("P" if k == "T" else k) for k in row] for row in kind]
        qp = np.array([[0 if kind[cy][cx] == "C" else qlo + (7 * cx + 5 * cy + 3 * pi) % (qhi - qlo + 1)
                        for cx in range(Wl)] for cy in range(Hl)])
        qpc = [np.array([[qpc_of(v, co[pl]) for v in row] for row in qp]) for pl in range(2)]
        intra = np.array([[k in "IC" for k in row] for row in kind])
        ref4 = np.zeros((4 * Hl, 4 * Wl), np.int64)
        coded = np.zeros((4 * Hl, 4 * Wl), bool)
        for by in range(4 * Hl):
            for bx in range(4 * Wl):
                k = kind[by // 4][bx // 4]
                ref4[by, bx] = (bx // 2) & 1 if k == "P" else 0
                if k == "P":
                    coded[by, bx] = (bx + 2 * by + pi) % 5 == 0
                elif k == "T":
                    coded[by, bx] = ((bx // 2) + (by // 2) + pi) % 2 == 0
        # the designed bS of every edge segment (8.7.2.1 for these zero-motion P pictures)
        def bs_of(bq, bp, mb_edge, inner_skipped, same_mb_16x16):
            (qy, qx), (py_, px_) = bq, bp
            if inner_skipped:
                return 0
            if intra[qy // 4, qx // 4] or intra[py_ // 4, px_ // 4]:
                return 4 if mb_edge else 3
            if coded[qy, qx] or coded[py_, px_]:
                return 2
            if same_mb_16x16:
                return 0
            return int(ref4[qy, qx] != ref4[py_, px_])
        bsV = np.zeros((4 * Hl, 4 * Wl), np.int64)
        bsH = np.zeros((4 * Hl, 4 * Wl), np.int64)
        for by in range(4 * Hl):
            for bx in range(4 * Wl):
                t8 = kind[by // 4][bx // 4] == "T"
                if bx:
                    bsV[by, bx] = bs_of((by, bx), (by, bx - 1), bx % 4 == 0, t8 and bx % 2 == 1, t8 and bx % 4 != 0)
                if by:
                    bsH[by, bx] = bs_of((by, bx), (by - 1, bx), by % 4 == 0, t8 and by % 2 == 1, t8 and by % 4 != 0)
        # the crafted planes: rows of 4-sample cells [c + a, c, c, c + b]
        def craft(width_cells, rows, qq, per_mb, mbh):
            out = np.zeros((rows, 4 * width_cells), np.int64)

            def edge_ab(cyq, k):                        # alpha, beta of the edge left of cell k
                qpav = (int(qq[cyq][(k - 1) // per_mb]) + int(qq[cyq][k // per_mb]) + 1) >> 1
                return ALPHA[min(51, max(0, qpav + offa))], BETA[min(51, max(0, qpav + offb))]
            for y in range(rows):
                cy = y // mbh
                # the last row of an MB row is what an Intra_16x16 MB below repeats 16 times: its cells
                # under such an MB sit on THAT MB's thresholds (t, by the cell: alpha - 1, alpha, then
                # beta - 1, beta on the q side and on the p side)
                below = cy + 1 if y % mbh == mbh - 1 and cy + 1 < Hl else None

                def tsel(k):
                    if below is None or k <= 0 or k >= width_cells or kind[below][k // per_mb] != "I":
                        return None
                    return (k + pi + cy) % 6
                c, b_prev = 110 + (y * 7 + pi * 13) % 40, 0
                for k in range(width_cells):
                    a = b = 0
                    t = tsel(k)
                    if k:
                        al, be = edge_ab(cy if t is None else below, k)
                        steps = [s for s in (al - 1, al, al + 1, (al >> 2) + 1, (al >> 2) + 2, (al >> 2) + 3, 1, 0, 2) if 0 <= s <= 66]
                        s = steps[(y + 3 * k + pi) % len(steps)]
                        if t is not None:
                            s = (al - 1, al)[t] if t < 2 and al <= 66 else (al >> 2) + 1 + k % 3 if t < 2 else 1
                        edge = c + b_prev                        # p0
                        q0 = edge + s if edge + s <= 165 and ((y + k) & 1 or edge - s < 95) else edge - s
                        q0 = min(165, max(95, q0))       # with |a|, |b| <= 18 and residuals up to 56: inside 0..255
                        a = (0, be - 1, be, 0, -(be - 1))[(y + k + pi) % 5] if be else 0
                        if t is not None:
                            a = (0, 0, be - 1, be, 0, 0)[t] if be else 0
                        c = q0 - a
                    if k + 1 < width_cells:
                        tn = tsel(k + 1)
                        _, be = edge_ab(cy if tn is None else below, k + 1)
                        b = (0, 0, be - 1, -be, be)[(y + 2 * k + pi) % 5] if be else 0
                        if tn is not None:
                            b = (0, 0, 0, 0, be - 1, be)[tn] if be else 0
                    out[y, 4 * k:4 * k + 4] = (c + a, c, c, c + b)
                    b_prev = b
            return np.clip(out, 0, 255)
        Y = craft(4 * Wl, 16 * Hl, qp, 4, 16)
        C = [craft(ccell * Wl, crow * Hl, qpc[pl], ccell, crow) + d for pl, d in enumerate((0, 3))]
        cwl = 4 * ccell
        for cy in range(1, Hl):                       # Intra_16x16 vertical: the row above, 16 times
            for cx in range(Wl):
                if kind[cy][cx] == "I":
                    Y[16 * cy:16 * cy + 16, 16 * cx:16 * cx + 16] = Y[16 * cy - 1, 16 * cx:16 * cx + 16]
                    for pl in range(2):
                        C[pl][crow * cy:crow * cy + crow, cwl * cx:cwl * cx + cwl] = C[pl][crow * cy - 1, cwl * cx:cwl * cx + cwl]
        # realise (transposed for horizontal edges)
        T = (lambda a: np.ascontiguousarray(a.T)) if horizontal else (lambda a: np.ascontiguousarray(a))
        pool, recs = [], np.zeros(W * H, A.MB_DTYPE)
        for cy in range(Hl):
            for cx in range(Wl):
                m = np.zeros(1, A.MB_DTYPE)[0]
                k = kind[cy][cx]
                _set_qp(m, int(qp[cy, cx]), co)
                m["coef_off"] = sum(len(a) for a in pool)
                n0 = len(pool)
                if k == "C":
                    m["mb_type"], m["flags"], m["cbp_blks"] = A.I_PCM, A.MBF_INTRA, 0xFFFF
                    raw = np.concatenate([T(Y[16 * cy:16 * cy + 16, 16 * cx:16 * cx + 16]).ravel()] +
                                         [T(C[pl][crow * cy:crow * cy + crow, cwl * cx:cwl * cx + cwl]).ravel() for pl in range(2)])
                    pool.append(raw.astype(np.uint8).view(np.int16))
                elif k == "I":
                    m["mb_type"], m["flags"] = A.I_16x16, A.MBF_INTRA
                    m["i16_mode"], m["chroma_mode"] = (1, 1) if horizontal else (0, 2)
                    pool.append(np.zeros(16, np.int16))
                else:
                    cb = coded[4 * cy:4 * cy + 4, 4 * cx:4 * cx + 4]
                    cb = cb.T if horizontal else cb
                    m["mb_type"] = A.P_8x8 if k == "P" else A.P_16x16
                    m["flags"] = A.MBF_T8x8 if k == "T" else 0
                    cbp = blks = 0
                    for q in range(4):
                        sub = cb[(q >> 1) * 2:(q >> 1) * 2 + 2, (q & 1) * 2:(q & 1) * 2 + 2]
                        if not sub.any():
                            continue
                        cbp |= 1 << q
                        lv = np.zeros(64, np.int16)
                        if k == "T":
                            lv[0] = 1
                            blks |= 0x33 << (((q >> 1) * 2) * 4 + (q & 1) * 2)
                        else:
                            for b4 in range(4):
                                if sub[b4 >> 1, b4 & 1]:
                                    lv[b4 * 16] = 1
                                    blks |= 1 << (((q >> 1) * 2 + (b4 >> 1)) * 4 + (q & 1) * 2 + (b4 & 1))
                        pool.append(lv)
                    m["cbp"], m["cbp_blks"] = cbp, blks
                if idc == 3 and k != "C":              # Cb and Cr blocks like the luma one, all levels zero
                    pool += [np.zeros(len(a), np.int16) for a in pool[n0:]] * 2
                px, py = (cy, cx) if horizontal else (cx, cy)
                recs[py * W + px] = m
        p.mbs[:] = recs
        p.levels = np.concatenate(pool + [np.zeros(8 + (128 if idc == 3 else 0), np.int16)])
        p.mv[:] = 0
        p.ref_idx[0] = np.array(entry, np.int8)[T(np.repeat(np.repeat(ref4, 1, 0), 1, 1))]
        p.ref_idx[1] = -1
        for mi, m in enumerate(p.mbs):
            if int(m["flags"]) & A.MBF_INTRA:
                p.ref_idx[0, 4 * (mi // W):4 * (mi // W) + 4, 4 * (mi % W):4 * (mi % W) + 4] = -1
        check_bounds(p)
        want = tuple(T(a).astype(np.uint8) for a in (Y, C[0], C[1]))
        if refs_all is None:
            refs_all = [tuple(np.zeros_like(a) for a in want) for _ in range(2 * len(D_EVERY))]
        # the coded blocks' flat residual: what the oracle adds to a plane without it, taken off the DPB plane
        refs_all[2 * pi] = refs_all[2 * pi + 1] = want
        first = O.decode(p, refs_all, stage="recon")
        res = first[0].astype(np.int64) - want[0].astype(np.int64)
        res[T(np.repeat(np.repeat(intra, 16, 0), 16, 1))] = 0
        short = want[0].astype(np.int64) - res
        assert short.min() >= 0 and short.max() <= 255 and (np.abs(res) <= 64).all(), (short.min(), short.max(), np.abs(res).max(), np.argwhere(np.abs(res) > 64)[:3])
        planes = (short.astype(np.uint8), want[1], want[2])
        refs_all[2 * pi] = refs_all[2 * pi + 1] = planes
        got = O.decode(p, refs_all, stage="recon")
        for k in range(3):
            assert np.array_equal(got[k], want[k]), (f"d_every[{pi}] plane {k}: the reconstruction is not the crafted plane",
                                                     np.argwhere(got[k] != want[k])[:4], kind)
        pics.append(p)
        Tq = (lambda a: np.ascontiguousarray(np.asarray(a).T)) if horizontal else (lambda a: np.asarray(a))
        design.append(dict(want=want, qp_y=Tq(qp), qp_c=[Tq(qpc[0]), Tq(qpc[1])], offa=offa, offb=offb, offs=co,
                           bsV=Tq(bsH) if horizontal else bsV, bsH=Tq(bsV) if horizontal else bsH,
                           kind=[[kind[cx][cy] for cx in range(Hl)] for cy in range(Wl)] if horizontal else kind))
    return Case(name or "d_every_" + ("h" if horizontal else "v"), pics, refs_all, chroma_format=idc,
                info=dict(design=design, horizontal=horizontal))


CASES["d_every_v"] = lambda L: build_d_every(L, False)
CASES["d_every_h"] = lambda L: build_d_every(L, True)
D_LINE_CASES = list(D_CASES)                    # lines across MB edges, each checked on its own
D_EVERY_CASES = ["d_every_v", "d_every_h"]      # every edge, checked by the whole-picture restatement
D_CASES = D_LINE_CASES + D_EVERY_CASES

# ---------------------------------------------------------------- S: strength from motion
import extremes_s as _S  # noqa: E402  (the builders need the helpers above)

CASES.update(_S.S_CASES)
S_CASES = list(_S.S_CASES)

# ---------------------------------------------------------------- I: intra prediction
import extremes_i as _I  # noqa: E402

CASES.update(_I.I_CASES)
I_CASES = list(_I.I_CASES)

# ---------------------------------------------------------------- D2: deblocking thresholds, per-plane chroma QP and other formats
import extremes_d2 as _D2  # noqa: E402

CASES.update(_D2.D2_CASES)
D2_CASES = list(_D2.D2_CASES)
CASES["r4_chroma_cqp"] = build_r_chroma_cqp       # family R; after the others: tests/golden/extremes.json only grows
CASES.update(_D2.D2_X_CASES)
