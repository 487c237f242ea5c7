"""Family D2 of tests/extremes.py (TEST INFRASTRUCTURE): the deblocking thresholds of family D under
the settings family D leaves out.  D is 4:2:0 frame pictures whose two chroma planes share one QP
(qp_c[0] == qp_c[1] == QP_C[qp_y]); here

  d_cqp_*     4:2:0 frames with chroma_qp_index_offset != second_chroma_qp_index_offset, so that Cb and
              Cr have different alpha / beta / tc0 on one edge: build_d (kinds bs1, mix, pcm) and
              build_d_every with a pair of offsets per picture;
  d_422_*     4:2:2 (an MB's chroma is 8 x 16): build_d_every without the 8x8 transform, chroma lines
              on the thresholds of the two vertical and the four horizontal chroma edges of an MB;
  d_444_*     4:4:4: Cb and Cr are full-size planes through the LUMA filter (strong filter, ap / aq)
              under their own QPs: build_d (bs1, pcm) and build_d_every with 8x8-transform MBs;
  d_field_*   top and bottom field pictures: I_PCM and bS 1 pictures of build_d; a horizontal intra MB
              edge is bS 3 there, a vertical one bS 4;
  d_mbaff     MBAFF frames of crafted I_PCM, inter, DC-coded and flat Intra_16x16 MBs in frame and field
              pairs of every neighbourhood, every class of edge on its thresholds, against
              deblock_restate_mbaff (8.7 for such pictures, from the records alone);
  x_mbaff_cqp generated MBAFF frames with Cb != Cr, pinned to the reference and shown to depend on which
              plane's qp_c is read.

Every record is legal: qp_c[pl] = QP_C[clip3(0, 51, qp_y + offset[pl])] with offsets in -12 .. 12,
qp_scaled[1 + pl] = qp_c[pl], an I_PCM MB has qp_y 0 (X._set_qp).  As in D, the samples before the loop
filter are known by construction and each builder asserts so against the oracle's reconstruction.

restate() is the whole loop filter of one picture in Python integers: the strengths from
extremes_s.strength_restate (the records alone), the filter from X.deblock_restate with the
picture's chroma geometry and a QP grid per chroma plane.  tests/test_extremes.py requires it to equal
the oracle's output on every picture, takes the census from its log, and requires every deliberately
wrong variant of it (WRONG) to differ from the oracle on some picture of every case it applies to.
"""
from __future__ import annotations

import numpy as np

import extremes as X
import extremes_s as S
from h264r import _abi as A
from h264r import synth

# chroma QP offset pairs (Cb, Cr): the two extremes crossed, unequal pairs of one sign, (0, k)
P_LO_HI, P_HI_LO = (-12, 12), (12, -12)


def _tg(g, horizontal):
    """One grid entry with its QP grid transposed for the 3 x 5 logical picture of horizontal edges."""
    return g[:2] + ([list(r) for r in zip(*g[2])] if horizontal else g[2],) + g[3:]


# (FilterOffsetA, FilterOffsetB, QP grid, chroma offsets, kind): consecutive pictures differ in pair and
# grid (k_deblock2 walks two pictures per wave).  An I_PCM MB's inner edges are bS 3 under qp_y 0:
# they stay off as long as QP_C[offset] + FilterOffsetA < 16, which the pcm pictures keep.
CQP_GRIDS = [
    X.D_GRIDS[0] + (P_LO_HI, "bs1"),
    X.D_GRIDS[1] + (P_HI_LO, "bs1"),
    X.D_GRIDS_MIX[0] + ((5, 2), "mix"),
    X.D_GRIDS_MIX[1] + ((0, 10), "mix"),
    X.D_GRIDS_PCM[0] + (P_HI_LO, "pcm"),
    X.D_GRIDS_PCM[1] + ((-12, 3), "pcm"),
]
G444_GRIDS = [
    X.D_GRIDS[0] + (P_LO_HI, "bs1"),
    X.D_GRIDS_PCM[1] + ((3, -12), "pcm"),
    X.D_GRIDS[2] + ((5, 11), "bs1"),
    X.D_GRIDS_PCM[0] + ((0, -9), "pcm"),
]
FIELD_GRIDS = [
    X.D_GRIDS_PCM[0] + (P_LO_HI, "pcm"),
    X.D_GRIDS_PCM[1] + ((2, -12), "pcm"),
    X.D_GRIDS[0] + (P_HI_LO, "bs1"),
    X.D_GRIDS[2] + ((0, 6), "bs1"),
]
# per picture of X.D_EVERY
EVERY_OFFS = [P_LO_HI, P_HI_LO, (-12, 8), (5, -12), (0, 9), (-6, 1)]


def build_lines(L, name, horizontal, grids, **kw):
    return X.build_d(L, None, horizontal, [_tg(g, horizontal) for g in grids], name, **kw)


D2_CASES = {
    "d_cqp_v": lambda L: build_lines(L, "d_cqp_v", False, CQP_GRIDS),
    "d_cqp_h": lambda L: build_lines(L, "d_cqp_h", True, CQP_GRIDS),
    "d_cqp_every_v": lambda L: X.build_d_every(L, False, "d_cqp_every_v", EVERY_OFFS),
    "d_cqp_every_h": lambda L: X.build_d_every(L, True, "d_cqp_every_h", EVERY_OFFS),
    "d_422_v": lambda L: X.build_d_every(L, False, "d_422_v", EVERY_OFFS, idc=2),
    "d_422_h": lambda L: X.build_d_every(L, True, "d_422_h", EVERY_OFFS, idc=2),
    "d_444_v": lambda L: build_lines(L, "d_444_v", False, G444_GRIDS, idc=3),
    "d_444_h": lambda L: build_lines(L, "d_444_h", True, G444_GRIDS, idc=3),
    "d_444_every_v": lambda L: X.build_d_every(L, False, "d_444_every_v", EVERY_OFFS, idc=3),
    "d_444_every_h": lambda L: X.build_d_every(L, True, "d_444_every_h", EVERY_OFFS, idc=3),
    "d_field_v": lambda L: build_lines(L, "d_field_v", False, FIELD_GRIDS, structures=(A.TOP_FIELD, A.BOTTOM_FIELD)),
    "d_field_h": lambda L: build_lines(L, "d_field_h", True, FIELD_GRIDS, structures=(A.TOP_FIELD, A.BOTTOM_FIELD)),
}
D2_LINE_CASES = ["d_cqp_v", "d_cqp_h", "d_444_v", "d_444_h", "d_field_v", "d_field_h"]      # build_d: designed lines
D2_EVERY_CASES = [n for n in D2_CASES if n not in D2_LINE_CASES]                            # build_d_every: every edge
D2_CQP, D2_422, D2_444, D2_FIELD = (["d_cqp_v", "d_cqp_h", "d_cqp_every_v", "d_cqp_every_h"], ["d_422_v", "d_422_h"],
                                    ["d_444_v", "d_444_h", "d_444_every_v", "d_444_every_h"], ["d_field_v", "d_field_h"])

# the deliberately wrong restatements and the cases each must be told from the oracle on
WRONG = {
    "swap_planes": list(D2_CASES), "qpc_from_qpy": list(D2_CASES), "q_side_qp": list(D2_CASES),
    "422_v_row_half": D2_422, "422_h_drop": D2_422, "444_chroma_filter": D2_444,
    # d_field_v's only horizontal intra MB edges lie between two I_PCM MBs (qp_y 0, indexA < 16): no bS shows there
    "field_hor_bs4": ["d_field_h"],
}


X_MBAFF_OFFS = (P_LO_HI, P_HI_LO, (-7, 9))


def build_x_mbaff_cqp(L) -> X.Case:
    """Generated MBAFF P frames (frame and field pairs mixed, the generator's own mild levels and DPB
    planes, so that the loop filter is on in many places) whose records carry a pair of chroma QP
    offsets: k_mbaff's loop filter reads qp_c[pl - 1] of a neighbour chosen per line, and no other
    generated MBAFF input has Cb != Cr.  The restatement (deblock_restate_mbaff) does not derive bS
    from motion, so the case is pinned to the reference, and the census shows on the oracle that its
    output depends on which plane's qp_c is read (with_qpc)."""
    pics = []
    for i, offs in enumerate(X_MBAFF_OFFS):
        lo, hi = ((24, 40), (30, 51), (20, 34))[i]
        cfg = synth.default_cfg(L, 3, 6, 4, qp_min=lo, qp_max=hi, structure=A.MBAFF_FRAME, wp_mode=0)
        p = synth.picture(L, cfg, i)
        for m in p.mbs:
            X._set_qp(m, int(m["qp_y"]), offs)
        X.check_bounds(p)
        pics.append(p)
    return X.Case("x_mbaff_cqp", pics, synth.refpics(L, pics[0].cfg), info=dict(offs=list(X_MBAFF_OFFS)))


def with_qpc(p, how: str):
    """A copy of picture p whose DEBLOCKING chroma QPs (qp_c; qp_scaled, the dequantisation's, stays) are
    wrong in one way: "swap" (Cb's for Cr and the reverse) or "qpy" (QP_C[qp_y] for both)."""
    mbs = p.mbs.copy()
    if how == "swap":
        mbs["qp_c"] = p.mbs["qp_c"][:, ::-1]
    else:
        mbs["qp_c"] = np.array([[X.QP_C[int(q)]] * 2 for q in p.mbs["qp_y"]])
    return synth.Picture(p.cfg, p.index, mbs, p.levels, p.mv, p.ref_idx, p.slices, p.pic)


D2_X_CASES = {"x_mbaff_cqp": build_x_mbaff_cqp}         # registered with D2_CASES; no restatement, its own census


def restate(c: X.Case, pi: int, wrong=(), log=None, probe=None):
    """The loop filter of picture pi of a D2 case restated: its output planes [Y, Cb, Cr] and the
    restated strengths (bsV, bsH)."""
    p, d = c.pics[pi], c.info["design"][pi]
    W, H = p.cfg.width_mbs, p.cfg.height_mbs
    bsV, bsH = S.strength_restate(p)
    if "field_hor_bs4" in wrong:
        bsH[0::4][bsH[0::4] == 3] = 4
    planes = [a.astype(np.int64) for a in d["want"]]
    X.deblock_restate(planes, W, H, d["qp_y"], d["qp_c"], bsV, bsH, d["offa"], d["offb"], log=log, probe=probe, idc=c.chroma_format,
                      wrong=[w for w in wrong if w != "field_hor_bs4"])
    return planes, (bsV, bsH)


# ---------------------------------------------------------------- MBAFF frames: the loop filter restated
def _mbaff_rows(pr, bot, fld, n):
    """Picture rows of the n rows (16 luma, 8 chroma) of the MB (pair row pr, bottom?) by its kind."""
    return [2 * n * pr + (2 * k + bot if fld else n * bot + k) for k in range(n)]


def deblock_restate_mbaff(planes, p, log=None, wrong=()):
    """8.7 on an MBAFF frame in Python integers, from the records alone; for pictures of
    zero-motion refIdx-0 inter MBs, I_PCM and intra MBs without the 8x8 transform, so that the
    strength is 4 / 3 (intra), 2 (a coded 4x4 block on either side), 1 (a frame MB against a field
    MB) or 0.  Per MB in address order (pair by pair, top then bottom) the vertical edges, then the
    horizontal ones.  Samples are taken by position: a field MB's rows are every second row of its
    pair; the p side of an MB edge is whichever MB holds the sample p0.
      vertical MB edge, pairs of two kinds: the left MB changes with the line (a frame MB's line y
        faces the left pair's field MB of parity y & 1; a field MB's line k the left frame MB that
        holds picture row 2 k + parity), and with it the QP and the coded bit; intra: bS 4;
        a chroma line takes the luma line 2 pel (+ (pel & 1) across pairs of two kinds);
      top edge of a top frame MB under a field pair: filtered twice with field stride, rows 0, 2, 4
        against the upper top-field MB, then rows 1, 3, 5 against the upper bottom-field MB;
      a field MB's top MB edge: with field stride against the upper pair's MB of its parity, or the
        upper frame pair's bottom MB; horizontal edges are bS 4 only between two frame MBs.
    A slice with deblock_idc 2 leaves its edges to other slices alone.
    log(plane, vertical, class, address of the p-side MB, bS, alpha, beta, tc0, line, [(y, x)]).
    wrong: deliberate mistakes for the mutation checks: "v_left_top", "h2b_drop", "h2_frame_stride",
    "field_hor_bs4", "no_mixed_floor", "chroma_idx_no_parity", and "swap_planes", "qpc_from_qpy", "q_side_qp" as in
    X.deblock_restate."""
    W, H = p.cfg.width_mbs, p.cfg.height_mbs
    mbs = p.mbs.reshape(H, W)

    def M(mx, pr, bot):
        return mbs[2 * pr + bot, mx]

    def addr(mx, pr, bot):
        return 2 * (pr * W + mx) + bot
    is_fld = lambda m: bool(int(m["flags"]) & A.MBF_FIELD)
    intra = lambda m: bool(int(m["flags"]) & A.MBF_INTRA)
    coded = lambda m, r, c: (int(m["cbp_blks"]) >> (4 * r + c)) & 1

    def run(pl, vertical, cls, pmb, qmb, bS, coords):
        if not bS:
            return
        sl = p.slices[int(qmb[3]["slice"])]
        offa, offb = int(sl["filter_offset_a"]), int(sl["filter_offset_b"])
        qp = [int(m[3]["qp_y"]) if pl == 0 else X.QP_C[int(m[3]["qp_y"])] if "qpc_from_qpy" in wrong else
              int(m[3]["qp_c"][2 - pl if "swap_planes" in wrong else pl - 1]) for m in (pmb, qmb)]
        qpav = qp[1] if "q_side_qp" in wrong else (qp[0] + qp[1] + 1) >> 1
        ia, ib = min(51, max(0, qpav + offa)), min(51, max(0, qpav + offb))
        img = planes[pl]
        line = [int(img[y, x]) for y, x in coords]
        tc0 = X.TC0[ia][bS - 1] if bS < 4 else 0
        if log:
            log(pl, vertical, cls, addr(*pmb[:3]), bS, X.ALPHA[ia], X.BETA[ib], tc0, line, coords)
        out = X.filter_line(line, X.ALPHA[ia], X.BETA[ib], bS, pl > 0, tc0)
        for (y, x), v in zip(coords, out):
            img[y, x] = v

    def strength(pmb, qmb, pblk, qblk, mb_edge, vertical, mixed):
        if intra(pmb[3]) or intra(qmb[3]):
            if not mb_edge:
                return 3
            if vertical:
                return 4
            frames = not is_fld(pmb[3]) and not is_fld(qmb[3])
            return 4 if frames or "field_hor_bs4" in wrong and is_fld(qmb[3]) else 3
        if coded(pmb[3], *pblk) or coded(qmb[3], *qblk):
            return 2
        return 1 if mixed and "no_mixed_floor" not in wrong else 0

    def other_slice(pmb, qmb):
        return int(p.slices[int(qmb[3]["slice"])]["deblock_idc"]) == 2 and int(pmb[3]["slice"]) != int(qmb[3]["slice"])
    for pr in range(H // 2):
        for mx in range(W):
            for bot in (0, 1):
                m = M(mx, pr, bot)
                if int(p.slices[int(m["slice"])]["deblock_idc"]) == 1:
                    continue
                cur = (mx, pr, bot, m)
                f = is_fld(m)
                ry, rc = _mbaff_rows(pr, bot, f, 16), _mbaff_rows(pr, bot, f, 8)
                # ---- vertical edges
                for e in range(4):
                    if e == 0 and mx == 0:
                        continue
                    lf = is_fld(M(mx - 1, pr, 0)) if e == 0 else f
                    mixed = e == 0 and lf != f

                    def left_of(k):
                        """(MB, its row) on the p side of luma line k of the left MB edge"""
                        if e:
                            return cur, k
                        if not mixed:
                            return (mx - 1, pr, bot, M(mx - 1, pr, bot)), k
                        yp = ry[k] - 32 * pr
                        b, r = (yp & 1, yp >> 1) if lf else (yp >> 4, yp & 15)
                        if "v_left_top" in wrong:
                            b = 0
                        return (mx - 1, pr, b, M(mx - 1, pr, b)), r
                    cls = "Inner" if e else ("V2" if f else "V1") if not mixed else ("V4" if f else "V3") + "tb"[bot]
                    for pl in range(3):
                        if pl and e & 1:
                            continue
                        for k in range(16 if pl == 0 else 8):
                            kl = k if pl == 0 else 2 * k + (1 if mixed and k & 1 and "chroma_idx_no_parity" not in wrong else 0)
                            pmb, prow = left_of(kl)
                            if e == 0 and other_slice(pmb, cur):
                                continue
                            bS = strength(pmb, cur, (prow >> 2, (e - 1) & 3), (kl >> 2, e), e == 0, True, mixed)
                            if pl == 0:
                                y, x = ry[k], 16 * mx + 4 * e
                                coords = [(y, x + i) for i in range(-4, 4)]
                            else:
                                y, x = rc[k], 8 * mx + 2 * e
                                coords = [(y, x + i) for i in range(-2, 2)]
                            run(pl, True, cls, pmb, cur, bS, coords)
                # ---- horizontal edges
                for e in range(4):
                    passes = []                 # (class, p MB, p rows nearest first, q rows, mixed)
                    if e:
                        passes.append(("Inner", cur, None, None, False))
                    elif not f and bot:
                        passes.append(("H3", (mx, pr, 0, M(mx, pr, 0)), None, None, False))
                    elif pr == 0:
                        continue
                    else:
                        uf = is_fld(M(mx, pr - 1, 0))
                        if not f and not uf:
                            passes.append(("H1", (mx, pr - 1, 1, M(mx, pr - 1, 1)), None, None, False))
                        elif not f and "h2_frame_stride" in wrong:
                            passes.append(("H2a", (mx, pr - 1, 1, M(mx, pr - 1, 1)), None, None, True))
                        elif not f:
                            for t in (0, 1):
                                if t and "h2b_drop" in wrong:
                                    continue
                                passes.append(("H2" + "ab"[t], (mx, pr - 1, t, M(mx, pr - 1, t)), t, None, True))
                        else:
                            cls = ("H4" if uf else "H5") if not bot else ("H6" if uf else "H7")
                            passes.append((cls, (mx, pr - 1, bot if uf else 1, M(mx, pr - 1, bot if uf else 1)), bot, None, not uf))
                    for cls, pmb, par, _, mixed in passes:
                        if e == 0 and other_slice(pmb, cur):
                            continue
                        for pl in range(3):
                            if pl and e & 1:
                                continue
                            n, rows, base = (4, ry, 32 * pr) if pl == 0 else (2, rc, 16 * pr)
                            pos = (4 if pl == 0 else 2) * e
                            if e or cls in ("H1", "H3") or (cls == "H2a" and par is None):
                                qrows = [rows[pos + i] for i in range(n)] if e or cls == "H3" else [base + i for i in range(n)]
                                prows = [rows[pos - 1 - i] for i in range(n)] if e else [qrows[0] - 1 - i for i in range(n)]
                            else:               # field stride across the pair boundary, parity par
                                qrows = [base + 2 * i + par for i in range(n)]
                                prows = [base - 2 * (i + 1) + par for i in range(n)]
                            for j in range(16 if pl == 0 else 8):
                                c4 = (j if pl == 0 else 2 * j) >> 2
                                bS = strength(pmb, cur, (3 if e == 0 else e - 1, c4), (e, c4), e == 0, False, mixed)
                                x = (16 if pl == 0 else 8) * mx + j
                                coords = [(y, x) for y in reversed(prows)] + [(y, x) for y in qrows]
                                run(pl, False, cls, pmb, cur, bS, coords)
    return planes


# ---------------------------------------------------------------- d_mbaff: MBAFF frames on the thresholds
MBAFF_W, MBAFF_H = 4, 6
MBAFF_PAIRS = ["FffF", "ffFF", "FfFf"]          # pair kinds per pair row: all four (current, left) and (current, upper)
# (FilterOffsetA, FilterOffsetB, QP range, chroma offsets, designed direction, slices)
# (an I_PCM MB has qp_y 0: its MB edges reach indexA and indexB of 16 and more only under offsets above 0)
# (horizontal edges come in twelve classes and cells, vertical ones in seven: four pictures for them)
# (chroma offsets: QP_C is flat from 48 on, so two QPs 8 apart give two QPc as long as the lower stays below it)
# (an I_PCM MB's chroma QP is QP_C[offset]: its INNER chroma edges, bS 3, are live where QP_C[offset] + FilterOffset
#  reaches 16 -- both planes in pictures 0 (vertical), 2 and 3 (horizontal), for alpha, beta and tc0 of their own)
MBAFF_PICS = [(12, 11, 22, 40, (12, 10), "v", 1), (6, 8, 30, 46, (4, -12), "h", 1), (12, 12, 20, 40, (12, 9), "h", 1),
              (12, 10, 22, 42, (6, 11), "h", 1), (0, 3, 36, 51, (-6, 3), "v", 1), (2, 4, 34, 51, (-8, 0), "h", 2)]
MBAFF_KINDS, MBAFF_KIND_SHIFT = "CPDDD", 2
MBAFF_SPLIT = 2                                 # the last picture's second slice (deblock_idc 2) starts at this MB row


def _steep(alpha, beta, base, sgn):
    """A luma line with |p0 - q0| = alpha - 1 whose p2 and q2 are beta away (ap and aq false: tc = tc0), so that
    the delta is clipped even at the small alpha of an edge against an I_PCM MB."""
    s = alpha - 1
    v = [base + sgn * o for o in (beta + 1, beta, 0, 0, s, s, s + beta, s + beta + 1)]
    shift = max(0, -min(v)) - max(0, max(v) - 255)
    v = [x + shift for x in v]
    return [v] if alpha > 1 and min(v) >= 0 and max(v) <= 255 else []


def _steep_c(alpha, beta, base, sgn):
    """A chroma line with |p0 - q0| = alpha - 1 whose p1 and q1 lean towards the other side by beta - 1: the
    largest delta a line that is on can have, (3 (alpha - 1) + 2 (beta - 1) + 4) >> 3, for the clip at small alpha."""
    s, t = alpha - 1, beta - 1
    out = []
    # (and, beside the flat Intra_16x16 MB at high QP, flat sides 100 apart: a step that fits next to 128 and passes tc)
    for off in [(t, 0, s, s - t)] + ([(0, 0, 100, 100), (100, 100, 0, 0)] if alpha > 101 else []):
        v = [base + sgn * o for o in off]
        shift = max(0, -min(v)) - max(0, max(v) - 255)
        v = [x + shift for x in v]
        if alpha > 1 and beta > 1 and min(v) >= 0 and max(v) <= 255:
            out.append(v)
    return out


def _line_items(line, alpha, beta, bS, chroma, tc0):
    """What a designed line would show of its cell's thresholds if it reaches its edge as designed."""
    c = X.classify(line, alpha, beta, bS, chroma, tc0)
    it = {"on" if c["on"] else "off"}
    if alpha and c["dp1"] < beta and c["dq1"] < beta and c["step"] - alpha in (-1, 0):
        it.add(("a", c["step"] - alpha))
    if beta > 1:
        it |= {("b", c[k] - beta) for k in ("dp1", "dq1") if c[k] - beta in (-1, 0)}
    if c["on"] and bS < 4 and c["clip"]:
        it.add("clip")
    if c["on"] and bS == 4 and not chroma:
        it |= {("small", c["step"] < (alpha >> 2) + 2), ("ap", c["ap"] < beta), ("aq", c["aq"] < beta)}
    return it


def build_d_mbaff(L) -> X.Case:
    """MBAFF frames of 4 x 6 MBs whose samples before the loop filter are known by construction:
    I_PCM MBs, zero-motion refIdx-0 inter MBs (frame and field MBs alike copy the DPB frame), the
    same with DC-only coded 4x4 blocks, and cbp-0 Intra_16x16 DC MBs all of whose neighbours are inter
    MBs under constrained_intra_pred (128 flat at any QP).  The two MBs of a pair differ in qp_y, in both
    qp_c and in which of their edge blocks are coded (an I_PCM MB counts as coded throughout).  The lines are laid out from the restatement's own walk over the
    records: every line of the designed direction (MBAFF_PICS: vertical edges in two pictures, horizontal
    ones in four), inner edges first and MB edges over them, is one of luma_designs / chroma_designs /
    CLAMP_LINES for the alpha, beta and bS it will be filtered under.  The last picture has two
    slices, the second (deblock_idc 2) starting at pair row 1."""
    W, H = MBAFF_W, MBAFF_H
    quant = X.O.quant_flat()[0]
    pics, design, refs = [], [], [None] * len(MBAFF_PICS)
    got_items = {}                              # per census cell, over the whole case
    for pi, (offa, offb, qlo, qhi, offs, direction, ns) in enumerate(MBAFF_PICS):
        rng = np.random.default_rng(4200 + pi)
        cfg = synth.default_cfg(L, 3, W, H, structure=A.MBAFF_FRAME, num_refs=len(MBAFF_PICS), deblock_idc=0, wp_mode=0,
                                num_slices=ns, constrained_intra=1, transform8x8=0, filter_offset_a=offa,
                                filter_offset_b=offb, qp_min=qlo, qp_max=qhi)
        p = synth.picture(L, cfg, pi)
        assert int(p.pic["constrained_intra_pred"][0]) == 1 and int(p.pic["structure"][0]) == A.MBAFF_FRAME
        for s, sl in enumerate(p.slices):
            sl["ref_slot"][:] = -1
            sl["ref_slot"][0][0] = pi
            sl["num_ref"][0], sl["num_ref"][1] = 1, 0
            sl["deblock_idc"] = 2 if s else 0
        fld = np.array([[ch == "f" for ch in (row[pi % W:] + row[:pi % W])] for row in MBAFF_PAIRS])
        # kinds: C I_PCM, P inter, D inter with DC-only coded blocks, I Intra_16x16 DC (placed last)
        # neighbours of every pairing, left / right and up / down, and never two alike in a pair but D D
        kind = np.array([[MBAFF_KINDS[(mx + 2 * my + pi + MBAFF_KIND_SHIFT) % 5] for mx in range(W)] for my in range(H)])
        placed = []
        for pr, mx in ((1 + pi % 2, 1 + pi % 3), (pi % 3, 3 - pi % 2)):
            # the MBs an Intra_16x16 DC MB could predict from: its own pair's other MB, the left and the upper pair
            near = [(a, b) for a, b in ((pr, mx), (pr, mx - 1), (pr - 1, mx)) if a >= 0 and b >= 0]
            if any(abs(a - pr) + abs(b - mx) <= 1 for a, b in placed):
                continue
            bot = (pr + mx + pi) & 1
            for a, b in near:
                for t in (0, 1):
                    if (a, b, t) != (pr, mx, bot) and kind[2 * a + t, b] == "C":
                        kind[2 * a + t, b] = "P"
            kind[2 * pr + bot, mx] = "I"
            kind[2 * pr + 1 - bot, mx] = "D"            # (its pair's other MB has coded edge blocks, the flat MB has none)
            placed.append((pr, mx))
        qp = rng.integers(qlo, qhi + 1, (H, W))
        qp[kind == "I"] = np.minimum(qhi, qp[kind == "I"] + 8)
        for pr in range(H // 2):                # the two MBs of a pair: QPs far enough apart for different alpha with a third MB
            for mx in range(W):
                a, b = int(qp[2 * pr, mx]), int(qp[2 * pr + 1, mx])
                if abs(a - b) < 7:
                    t = int(kind[2 * pr + 1, mx] == "I")            # move the MB that is not the Intra_16x16 one
                    o = (a, b)[t]
                    qp[2 * pr + 1 - t, mx] = o - 8 if o - 8 >= qlo else o + 8
        qp[kind == "C"] = 0
        coded = rng.random((H, W, 4, 4)) < 0.4
        coded[..., 0, 0] |= ~coded.reshape(H, W, 16).any(-1)
        coded[kind != "D"] = False
        edge = np.zeros((4, 4), bool)
        edge[[0, 3]], edge[:, [0, 3]] = True, True
        for pr in range(H // 2):                # the two MBs of a pair differ in which of their edge blocks are coded
            for mx in range(W):
                if kind[2 * pr, mx] == kind[2 * pr + 1, mx] == "D" and \
                        ((coded[2 * pr, mx] ^ coded[2 * pr + 1, mx]) & edge).sum() < 4:
                    coded[2 * pr + 1, mx] = ~coded[2 * pr, mx]
        p.mbs[:] = np.zeros(W * H, A.MB_DTYPE)
        p.mv[:] = 0
        p.ref_idx[:] = -1
        pool = []
        mbs = p.mbs.reshape(H, W)
        for my in range(H):
            for mx in range(W):
                m, k = mbs[my, mx], kind[my, mx]
                X._set_qp(m, int(qp[my, mx]), offs)
                m["flags"] = (A.MBF_FIELD if fld[my // 2, mx] else 0) | (A.MBF_INTRA if k in "CI" else 0)
                m["slice"] = int(ns > 1 and my >= MBAFF_SPLIT)
                m["coef_off"] = sum(len(a) for a in pool)
                if k == "C":
                    m["mb_type"], m["cbp_blks"] = A.I_PCM, 0xFFFF
                    pool.append(np.zeros(192, np.int16))            # filled below, from the crafted planes
                elif k == "I":
                    m["mb_type"], m["i16_mode"], m["chroma_mode"] = A.I_16x16, 2, 0
                    pool.append(np.zeros(16, np.int16))
                else:
                    m["mb_type"] = A.P_16x16
                    p.ref_idx[0, 4 * my:4 * my + 4, 4 * mx:4 * mx + 4] = 0
                    cbp = blks = 0
                    for q in range(4):
                        lv = np.zeros(64, np.int16)
                        for b4 in range(4):
                            r, c = (q >> 1) * 2 + (b4 >> 1), (q & 1) * 2 + (b4 & 1)
                            if coded[my, mx, r, c]:
                                lv[16 * b4] = 1
                                blks |= 1 << (4 * r + c)
                        if lv.any():
                            cbp |= 1 << q
                            pool.append(lv)
                    m["cbp"], m["cbp_blks"] = cbp, blks
        p.levels = np.concatenate(pool + [np.zeros(8, np.int16)])
        # the lines the loop filter will meet, with the parameters it will filter them under
        met = []
        blank = [np.zeros((16 * H, 16 * W), np.int64), np.zeros((8 * H, 8 * W), np.int64), np.zeros((8 * H, 8 * W), np.int64)]
        deblock_restate_mbaff(blank, p, log=lambda *a: met.append(a))
        want = [np.full_like(a, 128) for a in blank]
        fixed = [np.zeros(a.shape, bool) for a in blank]
        for my in range(H):
            for mx in range(W):
                if kind[my, mx] == "I":
                    f, bot = fld[my // 2, mx], my & 1
                    fixed[0][np.ix_(_mbaff_rows(my // 2, bot, f, 16), range(16 * mx, 16 * mx + 16))] = True
                    for pl in (1, 2):
                        fixed[pl][np.ix_(_mbaff_rows(my // 2, bot, f, 8), range(8 * mx, 8 * mx + 8))] = True
        count = {}
        for inner in (True, False):
            for pl, vertical, cls, pa, bS, alpha, beta, tc0, _, coords in met:
                if vertical != (direction == "v") or (cls == "Inner") != inner:
                    continue
                cell = (cls if cls != "Inner" else cls + "vh"[not vertical] + str(coords[1][0] - coords[0][0]), pl, bS)
                n = count[cell] = count.get(cell, -1) + 1
                # dark and bright bands of four lines along the edge (the blocks of the q-side MB): the edges of
                # the other direction, which lie between bands, find a step beyond alpha and leave the lines alone
                qy, qx = coords[len(coords) // 2]
                size = 16 if pl == 0 else 8
                if vertical:
                    band = ((qy % (2 * size)) // (size // 2) if fld[qy // (2 * size), qx // size] else qy // 4) & 1
                else:
                    band = (qx // 4) & 1
                base, sgn = ((70, 1), (235, -1))[band]         # (a coded block's residual, up to 64, must fit under the dark band)
                clamp = [c for c in X.CLAMP_LINES if (max(c) <= 5, min(c) >= 250)[band]]
                ds = (X.luma_designs(alpha, beta, bS, base, sgn) + _steep(alpha, beta, base, sgn) + clamp) if pl == 0 else \
                    (X.chroma_designs(alpha, beta, base, sgn) + _steep_c(alpha, beta, base, sgn) + [c[2:6] for c in clamp])
                fx = [fixed[pl][y, x] for y, x in coords]
                if any(fx):                 # a side inside an Intra_16x16 MB is 128 flat: the designs with that side flat, moved there
                    vals = [[d[i] for i in range(len(d)) if fx[i]] for d in ds]
                    ds = [[v + 128 - vs[0] for v in d] for d, vs in zip(ds, vals) if len(set(vs)) == 1]
                    ds = [d for d in ds if min(d) >= 0 and max(d) <= 255]
                if not ds:
                    continue
                # the design that shows most of what the line's census cell has seen least
                # (two lines per item: an edge of the other direction may still reach one of them first)
                seen = got_items.setdefault(cell, {})
                need = lambda d: sum(seen.get(i, 0) < 2 for i in _line_items(d, alpha, beta, bS, pl > 0, tc0))
                pick = max(ds[(n + pi) % len(ds):] + ds[:(n + pi) % len(ds)], key=need)
                for i in _line_items(pick, alpha, beta, bS, pl > 0, tc0):
                    seen[i] = seen.get(i, 0) + 1
                for (y, x), v in zip(coords, pick):
                    want[pl][y, x] = v
        assert all((w[f] == 128).all() for w, f in zip(want, fixed))
        # coded blocks: the residual must fit under or over the block's samples
        for my in range(H):
            for mx in range(W):
                if kind[my, mx] != "D":
                    continue
                q = int(qp[my, mx])
                r = (X.dq4(1, quant["scale4x4"][1][0][q % 6][0], q // 6) + 32) >> 6
                rows = _mbaff_rows(my // 2, my & 1, fld[my // 2, mx], 16)
                for br in range(4):
                    for bc in range(4):
                        if coded[my, mx, br, bc]:
                            ix = np.ix_(rows[4 * br:4 * br + 4], range(16 * mx + 4 * bc, 16 * mx + 4 * bc + 4))
                            want[0][ix] = np.maximum(want[0][ix], r)
        want = tuple(a.astype(np.uint8) for a in want)
        for my in range(H):
            for mx in range(W):
                if kind[my, mx] == "C":
                    f, bot = fld[my // 2, mx], my & 1
                    raw = np.concatenate([want[0][np.ix_(_mbaff_rows(my // 2, bot, f, 16), range(16 * mx, 16 * mx + 16))].ravel()] +
                                         [want[pl][np.ix_(_mbaff_rows(my // 2, bot, f, 8), range(8 * mx, 8 * mx + 8))].ravel() for pl in (1, 2)])
                    o = int(mbs[my, mx]["coef_off"])
                    p.levels[o:o + 192] = raw.view(np.int16)
        X.check_bounds(p)
        for s in range(len(refs)):
            refs[s] = refs[s] or tuple(np.zeros_like(a) for a in want)
        refs[pi] = tuple(np.full_like(a, 128) for a in want)       # the coded blocks' flat residual, over mid-grey
        first = X.O.decode(p, refs, stage="recon")
        res = first[0].astype(np.int64) - 128
        for my in range(H):                     # an intra MB has no part in it
            for mx in range(W):
                if kind[my, mx] in "CI":
                    res[np.ix_(_mbaff_rows(my // 2, my & 1, fld[my // 2, mx], 16), range(16 * mx, 16 * mx + 16))] = 0
        short = want[0].astype(np.int64) - res
        assert short.min() >= 0 and short.max() <= 255 and (np.abs(res) <= 64).all(), (pi, short.min(), short.max())
        refs[pi] = (short.astype(np.uint8), want[1], want[2])
        got = X.O.decode(p, refs, stage="recon")
        for k in range(3):
            assert np.array_equal(got[k], want[k]), (f"d_mbaff[{pi}] plane {k}: the reconstruction is not the crafted plane",
                                                     np.argwhere(got[k] != want[k])[:4])
        pics.append(p)
        design.append(dict(want=want, kind=kind, fld=fld, offs=offs, direction=direction, coded=coded))
    return X.Case("d_mbaff", pics, refs, info=dict(design=design))


def restate_mbaff(c: X.Case, pi: int, wrong=(), log=None):
    planes = [a.astype(np.int64) for a in c.info["design"][pi]["want"]]
    return deblock_restate_mbaff(planes, c.pics[pi], log=log, wrong=wrong)


D2_X_CASES["d_mbaff"] = build_d_mbaff
WRONG_MBAFF = ["v_left_top", "h2b_drop", "h2_frame_stride", "field_hor_bs4", "no_mixed_floor", "chroma_idx_no_parity",
               "swap_planes", "qpc_from_qpy", "q_side_qp"]
