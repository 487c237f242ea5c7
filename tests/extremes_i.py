"""Family I of tests/extremes.py ("intra prediction", TEST INFRASTRUCTURE): directed intra MBs whose
neighbours are known by construction, and a plain restatement of 8.3 to census them with.

A SITE is one intra MB T without residual (cbp 0: its bytes are the prediction alone) at MB
(3 i + 1, 2 j + 1) of a P picture with constrained_intra_pred = 1, so that no two sites share a
neighbour MB.  Each of its neighbours A (left), B (above), C (above right), D (above left) is an
I_PCM MB (available, its samples crafted) or an inter MB (P_16x16, zero vector, no residual: not
available under CIP).  The one DPB plane a picture references IS the picture's crafted plane, so an
inter MB reproduces it, and where it is not painted it holds seeded random bytes: the POISON an
unavailable neighbour leaves behind.  A kernel that reads it changes T.  All 16 masks
(avA, avB, avC, avD) are reached at interior MBs; unavailability through the picture border and
through a slice boundary -- other code in every kernel -- in the i_edges case; a chain of intra MBs,
each the left neighbour of the next (dependency levels 1..7, half of them with a DC-only residual),
in i_chain.  Every slice has deblock_idc 1: the output is the reconstruction.

intra_restate() is 8.3.1.2, 8.3.2.2 with the 8.3.2.2.1 filter, 8.3.3 and 8.3.4 (4:2:2 included) in
Python integers over a picture in raster order; neighbour availability comes from 6.4.12 (picture,
address order, slice, CIP), not from the builders.  It logs every block and lets a visitor recompute
the block under another mode or with one availability bit flipped (the mutation check of the
census, tests/test_extremes.py).
"""
from __future__ import annotations

import numpy as np

import _oracle as O
import extremes as X
from h264r import _abi as A
from h264r import synth
from h264r.mbview import level_count

W_MBS, H_MBS = 15, 16           # 5 x 8 sites; the generic GPU context of the extremes holds 16 x 16 MBs
QP = 26
NXN_NEEDS = {2: "", 0: "B", 3: "B", 7: "B", 1: "A", 8: "A", 4: "ABD", 5: "ABD", 6: "ABD"}
I16_NEEDS = {2: "", 0: "B", 1: "A", 3: "ABD"}
CHROMA_NEEDS = {0: "", 1: "A", 2: "B", 3: "ABD"}
I16_TO_CHROMA = {0: 2, 1: 1, 2: 0, 3: 3}          # the chroma mode of the same direction
MASKS = [(a, b, c, d) for a in (0, 1) for b in (0, 1) for c in (0, 1) for d in (0, 1)]
PATTERNS = ("zero", "max", "alt0", "alt1", "ramp_up", "ramp_down")
# (shift, last sum mod 2^shift that rounds down, first that rounds up) of every DC form
DC_SHIFTS = {"i4": (2, 3), "i8": (3, 4), "i16": (4, 5), "cb": (2, 3), "cr": (2, 3)}


def legal(needs, aA, aB, aD):
    have = {"A": aA, "B": aB, "D": aD}
    return sorted(m for m, n in needs.items() if all(have[c] for c in n))


def blk4_xy(b):
    """(bx, by) of luma4x4BlkIdx b, in 4x4 blocks."""
    return ((b >> 2) & 1) * 2 + (b & 1), (b >> 3) * 2 + ((b >> 1) & 1)


def avail4(b, mask):
    """(aA, aB, tv, aD) of I_4x4 block b under the MB mask, by block position (the census's own geometry:
    intra_restate derives the same from sample locations, 6.4.12)."""
    avA, avB, avC, avD = mask
    bx, by = blk4_xy(b)
    aD = avD if (bx, by) == (0, 0) else avA if bx == 0 else avB if by == 0 else 1
    # below row 0 the upper right is there or not by position (blkIdx 5 lies in row 0: MB C)
    tv = (avB if bx < 3 else avC) if by == 0 else 0 if b in (3, 7, 11, 13, 15) else 1
    return (1 if bx else avA), (1 if by else avB), tv, aD


def avail8(b, mask):
    """(aA, aB, aC, aD) of I_8x8 block b.  Block 0's upper right, samples (8 .. 15, -1), lies in MB B (6.4.12:
    xN < 16), so its aC is avB and MB C is read by block 1 alone."""
    avA, avB, avC, avD = mask
    return [(avA, avB, avB, avD), (1, avB, avC, avB), (avA, 1, 1, avA), (1, 1, 0, 1)][b]


# ---------------------------------------------------------------- 8.3, restated
def _clip(v):
    return 0 if v < 0 else 255 if v > 255 else v


def _gather(img, px, py, N, bits):
    """p[x, -1] (x = -1 .. 2 N - 1) and p[-1, y] of the N x N block at (px, py) as the bits say
    (8.3.1.2 / 8.3.2.2: without C, p[N .. 2 N - 1, -1] repeat p[N - 1, -1]); None when a bit asks for a
    sample outside the plane."""
    aA, aB, aC, aD = bits
    h, w = len(img), len(img[0])
    if (aA or aD) and px == 0 or (aB or aD) and py == 0 or aB and aC and px + 2 * N > w:
        return None
    p = {}
    if aD:
        p[-1, -1] = int(img[py - 1][px - 1])
    if aA:
        for y in range(N):
            p[-1, y] = int(img[py + y][px - 1])
    if aB:
        for x in range(N):
            p[x, -1] = int(img[py - 1][px + x])
        for x in range(N, 2 * N):
            p[x, -1] = int(img[py - 1][px + x]) if aC else p[N - 1, -1]
    return p


def _filter8(p, bits):
    """8.3.2.2.1."""
    aA, aB, _, aD = bits
    f = {}
    if aB:
        f[0, -1] = (p[-1, -1] + 2 * p[0, -1] + p[1, -1] + 2) >> 2 if aD else (3 * p[0, -1] + p[1, -1] + 2) >> 2
        for x in range(1, 15):
            f[x, -1] = (p[x - 1, -1] + 2 * p[x, -1] + p[x + 1, -1] + 2) >> 2
        f[15, -1] = (p[14, -1] + 3 * p[15, -1] + 2) >> 2
    if aD:
        if aA and aB:
            f[-1, -1] = (p[0, -1] + 2 * p[-1, -1] + p[-1, 0] + 2) >> 2
        elif aB:
            f[-1, -1] = (3 * p[-1, -1] + p[0, -1] + 2) >> 2
        elif aA:
            f[-1, -1] = (3 * p[-1, -1] + p[-1, 0] + 2) >> 2
        else:
            f[-1, -1] = p[-1, -1]
    if aA:
        f[-1, 0] = (p[-1, -1] + 2 * p[-1, 0] + p[-1, 1] + 2) >> 2 if aD else (3 * p[-1, 0] + p[-1, 1] + 2) >> 2
        for y in range(1, 7):
            f[-1, y] = (p[-1, y - 1] + 2 * p[-1, y] + p[-1, y + 1] + 2) >> 2
        f[-1, 7] = (p[-1, 6] + 3 * p[-1, 7] + 2) >> 2
    return f


def _pred_nxn(p, mode, N, bits, info):
    """8.3.1.2.1-9 / 8.3.2.2.2-10: the N x N prediction [y][x] from p (an I_8x8 block: the filtered p')."""
    aA, aB = bits[0], bits[1]
    need = NXN_NEEDS[mode]
    assert all(bits["ABCD".index(c)] for c in need), (mode, bits)
    T = lambda x: p[x, -1]
    Lf = lambda y: p[-1, y]
    out = [[0] * N for _ in range(N)]
    if mode == 2:
        s = (sum(Lf(y) for y in range(N)) if aA else 0) + (sum(T(x) for x in range(N)) if aB else 0)
        sh = (1 if N == 4 else 2) + aA + aB
        if aA or aB:
            info["dc"] = (sh, s % (1 << sh))
            v = (s + (1 << (sh - 1))) >> sh
        else:
            v = 128
        return [[v] * N for _ in range(N)]
    for y in range(N):
        for x in range(N):
            if mode == 0:
                v = T(x)
            elif mode == 1:
                v = Lf(y)
            elif mode == 3:
                v = (T(2 * N - 2) + 3 * T(2 * N - 1) + 2) >> 2 if x == y == N - 1 else \
                    (T(x + y) + 2 * T(x + y + 1) + T(x + y + 2) + 2) >> 2
            elif mode == 4:
                if x > y:
                    v = (T(x - y - 2) + 2 * T(x - y - 1) + T(x - y) + 2) >> 2
                elif x < y:
                    v = (Lf(y - x - 2) + 2 * Lf(y - x - 1) + Lf(y - x) + 2) >> 2
                else:
                    v = (T(0) + 2 * p[-1, -1] + Lf(0) + 2) >> 2
            elif mode == 5:
                z, k = 2 * x - y, x - (y >> 1)
                if z >= 0 and z % 2 == 0:
                    v = (T(k - 1) + T(k) + 1) >> 1
                elif z >= 0:
                    v = (T(k - 2) + 2 * T(k - 1) + T(k) + 2) >> 2
                elif z == -1:
                    v = (Lf(0) + 2 * p[-1, -1] + T(0) + 2) >> 2
                else:
                    v = (Lf(y - 2 * x - 1) + 2 * Lf(y - 2 * x - 2) + Lf(y - 2 * x - 3) + 2) >> 2
            elif mode == 6:
                z, k = 2 * y - x, y - (x >> 1)
                if z >= 0 and z % 2 == 0:
                    v = (Lf(k - 1) + Lf(k) + 1) >> 1
                elif z >= 0:
                    v = (Lf(k - 2) + 2 * Lf(k - 1) + Lf(k) + 2) >> 2
                elif z == -1:
                    v = (Lf(0) + 2 * p[-1, -1] + T(0) + 2) >> 2
                else:
                    v = (T(x - 2 * y - 1) + 2 * T(x - 2 * y - 2) + T(x - 2 * y - 3) + 2) >> 2
            elif mode == 7:
                k = x + (y >> 1)
                v = (T(k) + T(k + 1) + 1) >> 1 if y % 2 == 0 else (T(k) + 2 * T(k + 1) + T(k + 2) + 2) >> 2
            else:
                z, k = x + 2 * y, y + (x >> 1)
                if z > 2 * N - 3:
                    v = Lf(N - 1)
                elif z == 2 * N - 3:
                    v = (Lf(N - 2) + 3 * Lf(N - 1) + 2) >> 2
                elif z % 2 == 0:
                    v = (Lf(k) + Lf(k + 1) + 1) >> 1
                else:
                    v = (Lf(k) + 2 * Lf(k + 1) + Lf(k + 2) + 2) >> 2
            out[y][x] = v
    return out


def _block_nxn(img, px, py, N, mode, bits, info=None):
    info = {} if info is None else info
    p = _gather(img, px, py, N, bits)
    if p is None:
        return None
    if N == 8:
        p = {**p, **_filter8(p, bits)}
    return _pred_nxn(p, mode, N, bits, info)


def _edges(img, px, py, w, h, bits):
    """p[-1, -1], p[x, -1] (x < w), p[-1, y] (y < h) of a whole-MB predictor; bits (avA, avB, avD)."""
    aA, aB, aD = bits
    if (aA or aD) and px == 0 or (aB or aD) and py == 0:
        return None
    p = {}
    if aD:
        p[-1, -1] = int(img[py - 1][px - 1])
    if aA:
        for y in range(h):
            p[-1, y] = int(img[py + y][px - 1])
    if aB:
        for x in range(w):
            p[x, -1] = int(img[py - 1][px + x])
    return p


def _plane(p, w, h, info):
    """8.3.3.4 (w = h = 16) and 8.3.4.4 (w = 8: xCF 0, yCF 0 or 4)."""
    xcf, ycf = (4, 4) if w == 16 else (0, 4 if h == 16 else 0)
    Hs = sum((x + 1) * (p[4 + xcf + x, -1] - p[2 + xcf - x, -1]) for x in range(4 + xcf))
    Vs = sum((y + 1) * (p[-1, 4 + ycf + y] - p[-1, 2 + ycf - y]) for y in range(4 + ycf))
    a = 16 * (p[-1, h - 1] + p[w - 1, -1])
    b = ((5 if w == 16 else 34) * Hs + 32) >> 6
    c = ((5 if h == 16 else 34) * Vs + 32) >> 6
    raw = [[(a + b * (x - 3 - xcf) + c * (y - 3 - ycf) + 16) >> 5 for x in range(w)] for y in range(h)]
    info["plane"] = (Hs, Vs, min(min(r) for r in raw), max(max(r) for r in raw))
    return [[_clip(v) for v in r] for r in raw]


def _pred_16(img, px, py, mode, bits, info=None):
    info = {} if info is None else info
    aA, aB, aD = bits
    assert all({"A": aA, "B": aB, "D": aD}[c] for c in I16_NEEDS[mode]), (mode, bits)
    p = _edges(img, px, py, 16, 16, bits)
    if p is None:
        return None
    if mode == 0:
        return [[p[x, -1] for x in range(16)] for _ in range(16)]
    if mode == 1:
        return [[p[-1, y]] * 16 for y in range(16)]
    if mode == 2:
        s = (sum(p[-1, y] for y in range(16)) if aA else 0) + (sum(p[x, -1] for x in range(16)) if aB else 0)
        sh = 3 + aA + aB
        if aA or aB:
            info["dc"] = (sh, s % (1 << sh))
        v = (s + (1 << (sh - 1))) >> sh if aA or aB else 128
        return [[v] * 16 for _ in range(16)]
    return _plane(p, 16, 16, info)


def chroma_dc_uses(xO, yO, aA, aB):
    """8.3.4.1-3: which sums the DC of the chroma block at (xO, yO) takes: (left, top)."""
    if (xO, yO) == (0, 0) or (xO > 0 and yO > 0):
        return aA, aB
    if xO > 0:                       # yO == 0: the top alone when it is there
        return (0, 1) if aB else (aA, 0)
    return (1, 0) if aA else (0, aB)


def _pred_chroma(img, px, py, h, mode, bits, info=None):
    """8.3.4 for one chroma plane of an MB, 8 wide and h (8 or 16) high."""
    info = {} if info is None else info
    aA, aB, aD = bits
    assert all({"A": aA, "B": aB, "D": aD}[c] for c in CHROMA_NEEDS[mode]), (mode, bits)
    p = _edges(img, px, py, 8, h, bits)
    if p is None:
        return None
    if mode == 1:
        return [[p[-1, y]] * 8 for y in range(h)]
    if mode == 2:
        return [[p[x, -1] for x in range(8)] for _ in range(h)]
    if mode == 3:
        return _plane(p, 8, h, info)
    out = [[0] * 8 for _ in range(h)]
    info["blocks"] = []
    for blk in range(h // 2):
        xO, yO = (blk & 1) * 4, (blk >> 1) * 4
        uA, uB = chroma_dc_uses(xO, yO, aA, aB)
        s = (sum(p[-1, yO + k] for k in range(4)) if uA else 0) + (sum(p[xO + k, -1] for k in range(4)) if uB else 0)
        sh = 1 + uA + uB
        v = (s + (1 << (sh - 1))) >> sh if uA or uB else 128
        info["blocks"].append((blk, sh, s % (1 << sh) if uA or uB else None))
        for y in range(4):
            out[yO + y][xO:xO + 4] = [v] * 4
    return out


def intra_restate(p: synth.Picture, planes, log=None, visit=None):
    """8.3 over picture p in raster MB order, in place on planes = [Y, Cb, Cr] (lists of lists or int
    arrays) that hold the samples of every I_PCM and inter MB.  Availability by 6.4.12: inside the
    picture, decoded before, in the MB's slice, and intra when constrained_intra_pred is set.  A luma
    residual is added where the MB codes DC-only 4x4 blocks (the chain); anything else must be
    uncoded.  log(entry): one dict per predicted block: kind "i4" / "i8" / "i16" / "cb" / "cr", mb,
    blk, mode, bits, out (rows), dc (shift, sum mod 2^shift), plane (Hs, Vs, min, max unclipped),
    blocks (a chroma DC's (blk, shift, sum mod) per 4x4 block).  visit(entry, redo): redo(mode=, bits=)
    predicts the block again under another mode or other bits from the samples as they stand, None
    where that reads outside the plane."""
    W, H = p.cfg.width_mbs, p.cfg.height_mbs
    idc = A.idc_of(p.cfg.chroma_format)
    ch = A.chroma_mb(idc)[1]
    cip = int(p.pic["constrained_intra_pred"][0])
    sc = O.quant_flat()[0]["scale4x4"][0][0]

    def avail(a, nx, ny):
        if nx < 0 or ny < 0 or nx >= W or ny >= H:
            return 0
        n = ny * W + nx
        if n >= a or int(p.mbs[n]["slice"]) != int(p.mbs[a]["slice"]):
            return 0
        return int(not cip or bool(int(p.mbs[n]["flags"]) & A.MBF_INTRA))

    def emit(e, redo):
        if log is not None:
            log(e)
        if visit is not None:
            visit(e, redo)

    for a in range(W * H):
        m = p.mbs[a]
        t = int(m["mb_type"])
        if not int(m["flags"]) & A.MBF_INTRA or t == A.I_PCM:
            continue
        mx, my = a % W, a // W
        av = dict(A=avail(a, mx - 1, my), B=avail(a, mx, my - 1), C=avail(a, mx + 1, my - 1), D=avail(a, mx - 1, my - 1))

        def at(xN, yN):                     # 6.4.12 for a luma location of this MB
            if yN < 0:
                return av["D"] if xN < 0 else av["B"] if xN < 16 else av["C"]
            return av["A"] if xN < 0 else 0 if xN > 15 else 1
        Y = planes[0]
        x0, y0 = 16 * mx, 16 * my
        cbp, blks = int(m["cbp"]), int(m["cbp_blks"])
        assert cbp >> 4 == 0 and (cbp == 0 or t == A.I_4x4), "the restatement adds DC-only I_4x4 luma residuals alone"
        b8off = X.layout(m, idc)[0]
        if t in (A.I_4x4, A.I_8x8):
            N = 4 if t == A.I_4x4 else 8
            assert bool(int(m["flags"]) & A.MBF_T8x8) == (N == 8)
            for b in range(16 if N == 4 else 4):
                bx, by = blk4_xy(b) if N == 4 else (b & 1, b >> 1)
                xO, yO = bx * N, by * N
                mode = (int(m["ipred"][b >> 1]) >> ((b & 1) * 4)) & 15
                aC = at(xO + N, yO - 1)
                if N == 4 and b in (3, 11):           # 8.3.1.2: decoded later
                    aC = 0
                bits = (at(xO - 1, yO), at(xO, yO - 1), aC, at(xO - 1, yO - 1))
                e = dict(kind="i4" if N == 4 else "i8", mb=(mx, my), blk=b, mode=mode, bits=bits)
                out = _block_nxn(Y, x0 + xO, y0 + yO, N, mode, bits, e)
                e["out"] = out
                emit(e, lambda mode=mode, bits=bits, px=x0 + xO, py=y0 + yO, N=N: _block_nxn(Y, px, py, N, mode, bits))
                r = 0
                if N == 4 and (blks >> (by * 4 + bx)) & 1:
                    o = int(m["coef_off"]) + b8off[b >> 2] + (b & 3) * 16
                    lv = [int(v) for v in p.levels[o:o + 16]]
                    assert lv[0] and not any(lv[1:])
                    qp = int(m["qp_scaled"][0])
                    r = (X.dq4(lv[0], sc[qp % 6][0], qp // 6) + 32) >> 6
                for y in range(N):
                    for x in range(N):
                        Y[y0 + yO + y][x0 + xO + x] = _clip(out[y][x] + r)
        else:
            assert t == A.I_16x16, t
            mode, bits = int(m["i16_mode"]), (av["A"], av["B"], av["D"])
            e = dict(kind="i16", mb=(mx, my), blk=0, mode=mode, bits=bits)
            out = _pred_16(Y, x0, y0, mode, bits, e)
            e["out"] = out
            emit(e, lambda mode=mode, bits=bits: _pred_16(Y, x0, y0, mode, bits))
            for y in range(16):
                for x in range(16):
                    Y[y0 + y][x0 + x] = out[y][x]
        if idc in (1, 2):
            mode, bits = int(m["chroma_mode"]), (av["A"], av["B"], av["D"])
            for pl in (1, 2):
                img = planes[pl]
                cx0, cy0 = 8 * mx, ch * my
                e = dict(kind="cb" if pl == 1 else "cr", mb=(mx, my), blk=0, mode=mode, bits=bits)
                out = _pred_chroma(img, cx0, cy0, ch, mode, bits, e)
                e["out"] = out
                emit(e, lambda mode=mode, bits=bits, img=img, cx0=cx0, cy0=cy0: _pred_chroma(img, cx0, cy0, ch, mode, bits))
                for y in range(ch):
                    for x in range(8):
                        img[cy0 + y][cx0 + x] = out[y][x]
    return planes


# ---------------------------------------------------------------- crafted content
def pattern_mb(name, w, h, rng):
    y, x = np.mgrid[0:h, 0:w]
    if name == "random":
        return rng.integers(0, 256, (h, w)).astype(np.uint8)
    ramp = ((x + y) * 255) // (w + h - 2)
    return {"zero": np.zeros((h, w), np.int64), "max": np.full((h, w), 255), "alt0": ((x + y) & 1) * 255,
            "alt1": ((x + y + 1) & 1) * 255, "ramp_up": ramp, "ramp_down": 255 - ramp}[name].astype(np.uint8)


def paint(base, mb, name, rng):
    """MB (mx, my) of every plane takes the pattern."""
    mx, my = mb
    for a in base:
        h, w = (16, 16) if a is base[0] else (a.shape[0] * 16 // base[0].shape[0], 8)
        a[h * my:h * my + h, w * mx:w * mx + w] = pattern_mb(name, w, h, rng)


def paint_halves(base, mb, across_x, first):
    """One half of the MB `first`, the other 255 - first (split along x: columns, else rows)."""
    mx, my = mb
    for a in base:
        h, w = (16, 16) if a is base[0] else (a.shape[0] * 16 // base[0].shape[0], 8)
        blk = a[h * my:h * my + h, w * mx:w * mx + w]
        blk[:] = first
        if across_x:
            blk[:, w // 2:] = 255 - first
        else:
            blk[h // 2:, :] = 255 - first


PLANE_DESIGNS = {           # name: (D value, B halves (first value) or None: random, A halves or None)
    "H+": (0, 0, None), "H-": (255, 255, None), "V+": (0, None, 0), "V-": (255, None, 255),
    "++": (0, 0, 0), "--": (255, 255, 255),
    "+-": (0, 0, 255)}      # chroma: b = 1355, c = -813 round a = 4080: clips at 0 and at 255 in one MB


# ---------------------------------------------------------------- realisation
def realise(L, pi, nslots, W, H, T, pcm, base, slice_at=None, nslices=1, intra_pic=False, structure=A.FRAME,
            chroma_format=0):
    """One picture: T {(x, y): spec} intra MBs, pcm the I_PCM MBs (their samples: base), every other MB
    inter, copying base from DPB slot pi.  spec: kind, modes (NxN), i16, cmode, and for the chain
    dc (the 16 DC-only luma levels of an I_4x4 MB, 0: not coded)."""
    over = dict(transform8x8=1, deblock_idc=1, num_slices=nslices, structure=structure)
    if chroma_format:
        over["chroma_format"] = chroma_format
    # (an I picture comes from the P configuration too, its slices retyped: the case has one DPB)
    cfg = synth.default_cfg(L, 3, W, H, num_refs=nslots, constrained_intra=0 if intra_pic else 1, wp_mode=0, **over)
    p = synth.picture(L, cfg, pi)
    idc = A.idc_of(chroma_format)
    ch = A.chroma_mb(idc)[1]
    mbs = np.zeros(W * H, A.MB_DTYPE)
    pool, off = [], 0
    ref = np.full((4 * H, 4 * W), -1, np.int8)
    for a in range(W * H):
        x, y = a % W, a // W
        m = mbs[a]
        m["slice"] = slice_at(x, y) if slice_at else 0
        m["coef_off"] = off
        lv = None
        if (x, y) in pcm:
            m["mb_type"], m["flags"], m["cbp_blks"] = A.I_PCM, A.MBF_INTRA, 0xFFFF
            X._set_qp(m, 0)
            raw = np.concatenate([base[0][16 * y:16 * y + 16, 16 * x:16 * x + 16].ravel()] +
                                 [base[k][ch * y:ch * y + ch, 8 * x:8 * x + 8].ravel() for k in (1, 2)])
            lv = raw.astype(np.uint8).view(np.int16)
        elif (x, y) in T:
            s = T[(x, y)]
            m["mb_type"], m["flags"] = s["kind"], A.MBF_INTRA | (A.MBF_T8x8 if s["kind"] == A.I_8x8 else 0)
            X._set_qp(m, QP)
            m["chroma_mode"] = s["cmode"]
            if s["kind"] == A.I_16x16:
                m["i16_mode"] = s["i16"]
                lv = np.zeros(16, np.int16)
            else:
                for b, mode in enumerate(s["modes"]):
                    m["ipred"][b >> 1] |= mode << ((b & 1) * 4)
                dc = s.get("dc")
                if dc is not None:
                    cbp, lv = 0, []
                    for q in range(4):
                        if any(dc[4 * q:4 * q + 4]):
                            cbp |= 1 << q
                            blk = np.zeros(64, np.int16)
                            blk[0::16] = dc[4 * q:4 * q + 4]
                            lv.append(blk)
                    m["cbp"] = cbp
                    lv = np.concatenate(lv) if lv else None
        else:
            assert not intra_pic
            m["mb_type"] = A.P_16x16
            X._set_qp(m, QP)
            ref[4 * y:4 * y + 4, 4 * x:4 * x + 4] = 0
        if lv is not None:
            pool.append(lv)
            off += len(lv)
    p.mbs[:] = mbs
    p.levels = np.concatenate(pool + [np.zeros(8, np.int16)])
    p.mv[:] = 0
    p.ref_idx[0], p.ref_idx[1] = ref, -1
    for sl in p.slices:
        assert int(sl["deblock_idc"]) == 1
        if intra_pic:
            sl["slice_type"], sl["ref_slot"], sl["num_ref"] = A.SLICE_I, 0, 0
        else:
            sl["ref_slot"][:] = -1
            # a field references the slot's field of its own parity (another parity moves the chroma vector)
            sl["ref_slot"][0][0] = pi | (A.REF_BOTTOM if structure == A.BOTTOM_FIELD else 0)
            sl["num_ref"][0], sl["num_ref"][1] = 1, 0
    X.recompute_blks(p)
    X.check_bounds(p)
    return p


def random_base(rng, W, H, ch):
    return [rng.integers(0, 256, (16 * H, 16 * W)).astype(np.uint8), rng.integers(0, 256, (ch * H, 8 * W)).astype(np.uint8),
            rng.integers(0, 256, (ch * H, 8 * W)).astype(np.uint8)]


def _tune(work, base, tx, ty, spec, ch):
    """DC rounding: the last sample of block 0's left column (in A) moves through 0 .. 255, the one two
    rows above it through eight values, until block 0's sum mod 2^shift is the target; for luma and for
    each chroma plane."""
    bits3 = (spec["mask"][0], spec["mask"][1], spec["mask"][3])
    for kind, shift, target in spec["tune"]:
        pl = {"cb": 1, "cr": 2}.get(kind, 0)
        n = {"i4": 4, "i8": 8, "i16": 16}.get(kind, 4)
        sx, sy = ((16 * tx - 1, 16 * ty + n - 1) if pl == 0 else (8 * tx - 1, ch * ty + 3))
        first = work[pl][sy - 2][sx]
        for v in range(8 * 256):            # (the I_8x8 filter skips some sums: a second sample shifts them)
            work[pl][sy - 2][sx] = (first + v // 256) % 256
            base[pl][sy - 2, sx] = work[pl][sy - 2][sx]
            v %= 256
            work[pl][sy][sx] = v
            info = {}
            if kind in ("i4", "i8"):
                _block_nxn(work[0], 16 * tx, 16 * ty, n, 2, (avail4 if n == 4 else avail8)(0, spec["mask"]), info)
                got = info.get("dc")
            elif kind == "i16":
                _pred_16(work[0], 16 * tx, 16 * ty, 2, bits3, info)
                got = info.get("dc")
            else:
                _pred_chroma(work[pl], 8 * tx, ch * ty, ch, 0, bits3, info)
                got = info["blocks"][0][1:]
            if got == (shift, target):
                base[pl][sy, sx] = v
                break
        else:
            raise AssertionError(("no sample value reaches", kind, shift, target))


def build_sites(L, name, specs, seed, structure=A.FRAME, chroma_format=0, H=H_MBS, odd_tail=False):
    """The specs laid on sites, 5 per site row, as many pictures as they need.  spec: kind, modes / i16,
    cmode, mask, pat {neighbour: pattern} (default: seeded random), design (a PLANE_DESIGNS name),
    tune [(kind, shift, target)], tag."""
    W = W_MBS
    nx, per = W // 3, (W // 3) * (H // 2)
    idc = A.idc_of(chroma_format)
    ch = A.chroma_mb(idc)[1]
    fld = structure != A.FRAME
    chunks = [specs[i:i + per] for i in range(0, len(specs), per)]
    if odd_tail and sum(s["kind"] == A.I_4x4 for s in chunks[-1]) % 2 == 0:
        # the level-1 pairable count of the last picture is odd (one picture less: the other parity)
        if len(chunks[-1]) < per:
            chunks[-1] = chunks[-1] + _fill4(1, seed + 7)
        else:
            chunks.append(_fill4(1, seed + 7))
    assert len(chunks) <= 8, len(chunks)
    pics, refs, sites = [], [], []
    for pi, chunk in enumerate(chunks):
        rng = np.random.default_rng([seed, pi])
        base = random_base(rng, W, H, ch)
        T, pcm, tuned = {}, set(), []
        for k, s in enumerate(chunk):
            tx, ty = 3 * (k % nx) + 1, 2 * (k // nx) + 1
            nb = dict(A=(tx - 1, ty), B=(tx, ty - 1), C=(tx + 1, ty - 1), D=(tx - 1, ty - 1))
            for bit, key in zip(s["mask"], "ABCD"):
                if bit:
                    pcm.add(nb[key])
                    if s.get("pat", {}).get(key):
                        paint(base, nb[key], s["pat"][key], rng)
            if s.get("design"):
                dv, bh, ah = PLANE_DESIGNS[s["design"]]
                paint(base, nb["D"], "max" if dv else "zero", rng)
                for first, key, across in ((bh, "B", True), (ah, "A", False)):
                    if first is not None:
                        paint_halves(base, nb[key], across, first)
            T[(tx, ty)] = s
            if s.get("tune"):
                tuned.append((tx, ty, s))
            sites.append(dict(pic=pi, mb=(tx, ty), tag=s["tag"], mask=s["mask"], pat=s.get("pat", {}),
                              design=s.get("design"), tune=s.get("tune")))
        if tuned:
            work = [a.astype(np.int64).tolist() for a in base]
            for tx, ty, s in tuned:
                _tune(work, base, tx, ty, s, ch)
        p = realise(L, pi, len(chunks), W, H, T, pcm, base, structure=structure, chroma_format=chroma_format)
        pics.append(p)
        if fld:                                           # both fields of the slot's frame hold the plane
            refs.append(tuple(np.ascontiguousarray(np.repeat(a, 2, 0)) for a in base))
        else:
            refs.append(tuple(np.ascontiguousarray(a) for a in base))
    if fld:
        import ctypes
        refs = refs[:L.h264r_synth_ref_frames(ctypes.byref(pics[0].cfg))]
    return X.Case(name, pics, refs, chroma_format=idc, info=dict(sites=sites))


# ---------------------------------------------------------------- the site lists
def _cm(mask, k):
    lg = legal(CHROMA_NEEDS, mask[0], mask[1], mask[3])
    return lg[k % len(lg)]


def nxn_specs(kind, seed, reps=9):
    """Every mask, `reps` sites each: every block runs through its legal modes (from an offset drawn
    per mask and block, so that a block's neighbours inside T differ from mask to mask); every mode
    over every value pattern (all blocks one mode, all four neighbours one pattern); DC rounding."""
    rng = np.random.default_rng(seed)
    n, av = (16, avail4) if kind == A.I_4x4 else (4, avail8)
    key = "i4" if kind == A.I_4x4 else "i8"
    out = []
    for mask in MASKS:
        offs = rng.integers(0, 9, n)
        for k in range(reps):
            modes = []
            for b in range(n):
                aA, aB, _, aD = av(b, mask)
                lg = legal(NXN_NEEDS, aA, aB, aD)
                modes.append(lg[(k + int(offs[b])) % len(lg)])
            out.append(dict(kind=kind, modes=modes, cmode=_cm(mask, k), mask=mask, tag="mask"))
    full = (1, 1, 1, 1)
    for pat in PATTERNS:
        for mode in range(9):
            out.append(dict(kind=kind, modes=[mode] * n, cmode=mode % 4, mask=full, pat=dict.fromkeys("ABCD", pat),
                            tag="values"))
    lo, hi = DC_SHIFTS[key]
    for mask, sh, csh in (((1, 0, 0, 0), lo, 2), (full, hi, 3)):
        for up in (0, 1):                 # the last sum that rounds down, the first that rounds up
            out.append(dict(kind=kind, modes=[2] * n, cmode=0, mask=mask, tag="dc",
                            tune=[(key, sh, (1 << (sh - 1)) - 1 + up), ("cb", csh, (1 << (csh - 1)) - 1 + up),
                                  ("cr", csh, (1 << (csh - 1)) - 1 + up)]))
    return out


def i16_specs(seed, reps=2):
    out = []
    for r in range(reps):
        for mask in MASKS:
            for mode in legal(I16_NEEDS, mask[0], mask[1], mask[3]):
                out.append(dict(kind=A.I_16x16, i16=mode, cmode=I16_TO_CHROMA[mode], mask=mask, tag="mask"))
    full = (1, 1, 1, 1)
    for pat in PATTERNS:
        for mode in range(4):
            out.append(dict(kind=A.I_16x16, i16=mode, cmode=I16_TO_CHROMA[mode], mask=full, pat=dict.fromkeys("ABCD", pat),
                            tag="values"))
    for mask, sh, csh in (((1, 0, 0, 0), 4, 2), (full, 5, 3)):
        for up in (0, 1):
            out.append(dict(kind=A.I_16x16, i16=2, cmode=0, mask=mask, tag="dc",
                            tune=[("i16", sh, (1 << (sh - 1)) - 1 + up), ("cb", csh, (1 << (csh - 1)) - 1 + up),
                                  ("cr", csh, (1 << (csh - 1)) - 1 + up)]))
    for d in PLANE_DESIGNS:
        out.append(dict(kind=A.I_16x16, i16=3, cmode=3, mask=full, design=d, tag="plane"))
    return out


def build_i_nxn(L, name, kind, seed):
    specs = nxn_specs(kind, seed)
    if kind != A.I_4x4:                   # a few pairable MBs among them, for the pair list
        specs = specs + _fill4(5, seed + 1)
    return build_sites(L, name, specs, seed, odd_tail=True)


def _fill4(n, seed):
    """n extra I_4x4 sites of drawn legal modes (they make a case's pairable count what it has to be)."""
    return nxn_specs(A.I_4x4, seed, reps=1)[3:3 + n]


def build_i_16(L, name, seed, chroma_format=0):
    specs = i16_specs(seed)
    if not chroma_format:
        specs = specs + _fill4(5, seed + 1)
    return build_sites(L, name, specs, seed, chroma_format=chroma_format, odd_tail=not chroma_format)


def build_i_field(L, name, structure, seed):
    """One site picture as a field of 15 x 8 MBs: 20 sites, the three kinds in turn, over all 16 masks."""
    s4, s8, s16 = nxn_specs(A.I_4x4, seed), nxn_specs(A.I_8x8, seed + 1), i16_specs(seed + 2, reps=1)
    specs = []
    for i in range(20):
        mi = (7 * i) % 16
        of16 = [s for s in s16 if s["mask"] == MASKS[mi] and s["tag"] == "mask"]
        specs.append((s4[9 * mi + i % 9], s8[9 * mi + (i + 5) % 9], of16[i % len(of16)])[i % 3])     # (+ 5: all nine I_8x8 modes)
    return build_sites(L, name, specs, seed, structure=structure, H=8)


def _mask_of(W, H, x, y, slice_at, intra_at, cip):
    def av(nx, ny):
        if nx < 0 or ny < 0 or nx >= W or ny >= H or ny * W + nx >= y * W + x:
            return 0
        return int(slice_at(nx, ny) == slice_at(x, y) and (not cip or intra_at(nx, ny)))
    return av(x - 1, y), av(x, y - 1), av(x + 1, y - 1), av(x - 1, y - 1)


def _drawn_spec(rng, k, mask, tag):
    """A site of kind k % 3 with modes drawn among the legal ones of its mask."""
    kind = (A.I_4x4, A.I_8x8, A.I_16x16)[k % 3]
    cm = legal(CHROMA_NEEDS, mask[0], mask[1], mask[3])
    s = dict(kind=kind, cmode=int(rng.choice(cm)), mask=mask, tag=tag)
    if kind == A.I_16x16:
        s["i16"] = int(rng.choice(legal(I16_NEEDS, mask[0], mask[1], mask[3])))
    else:
        n, av = (16, avail4) if kind == A.I_4x4 else (4, avail8)
        s["modes"] = []
        for b in range(n):
            aA, aB, _, aD = av(b, mask)
            s["modes"].append(int(rng.choice(legal(NXN_NEEDS, aA, aB, aD))))
    return s


def _last_odd(make):
    """make(extra) -> (picture, ...): the variant whose level-1 pair list holds an odd count of MBs (a
    batch without this picture then has the other parity), by one extra isolated I_4x4 site if need be."""
    r = make(False)
    if pairable_level1(r[0]) % 2 == 0:
        r = make(True)
    assert pairable_level1(r[0]) % 2 == 1
    return r


def build_i_edges(L, name="i_edges", seed=71):
    """Picture 0: an I picture of I_PCM MBs with sites on the four corners and along the four edges
    (hd.nin: the picture border) and some inside.  Picture 1: a P picture (CIP) of I_PCM MBs in four
    slices that start in the middle of MB rows 3, 9 and 13, with sites after a slice start and in the row
    below it (the slice compare)."""
    W, H = W_MBS, H_MBS
    pics, refs, sites = [], [], []

    def make(pi, extra):
        rng = np.random.default_rng([seed, pi])
        base = random_base(rng, W, H, 8)
        if pi == 0:
            at = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
            at += [(x, 0) for x in range(2, W - 2, 2)] + [(x, H - 1) for x in range(2, W - 2, 2)]
            at += [(0, y) for y in range(2, H - 2, 2)] + [(W - 1, y) for y in range(2, H - 2, 2)]
            at += [(x, y) for y in (3, 7, 11) for x in range(2, W - 2, 3)]          # interior: all four there
            slice_at = lambda x, y: 0
        else:
            starts = (3 * W + 7, 9 * W + 7, 13 * W + 7)
            slice_at = lambda x, y: sum(y * W + x >= s for s in starts)
            # in the start's row: the slice's first MB (7, 3), then (9, 3): A alone; in the row below a
            # start: B, C, D of the other slice (x < 6), C alone of this one (6), D alone not (7)
            at = [(2, 3), (4, 3), (7, 3), (9, 3), (12, 3)] + [(x, 10) for x in (0, 3, 6, 9, 12)]
            at += [(x, 14) for x in (1, 4, 7, 10, 13)] + [(x, 6) for x in range(1, W, 2)] + [(x, 1) for x in range(1, W, 2)]
        T, mine = {}, []
        for k, (x, y) in enumerate(at + ([(12, 12)] if extra else [])):
            mask = _mask_of(W, H, x, y, slice_at, lambda nx, ny: True, pi == 1)
            T[(x, y)] = _drawn_spec(rng, 0 if (x, y) == (12, 12) else k + pi, mask, "border" if pi == 0 else "slice")
            mine.append(dict(pic=pi, mb=(x, y), tag=T[(x, y)]["tag"], mask=mask, pat={}, design=None, tune=None))
        for (x, y) in T:                                 # isolated: no site is another's neighbour
            assert not any((x + dx, y + dy) in T for dx, dy in ((-1, 0), (0, -1), (1, -1), (-1, -1)))
        pcm = {(x, y) for y in range(H) for x in range(W)} - set(T)
        p = realise(L, pi, 2, W, H, T, pcm, base, slice_at=slice_at, nslices=1 + 3 * pi, intra_pic=pi == 0)
        return p, base, mine
    for pi in range(2):
        p, base, mine = make(pi, False) if pi == 0 else _last_odd(lambda extra: make(pi, extra))
        pics.append(p)
        sites += mine
        refs.append(tuple(np.ascontiguousarray(a) for a in base))
    return X.Case(name, pics, refs, info=dict(sites=sites))


CHAIN_LEN = 7


def build_i_chain(L, name="i_chain", seed=83):
    """Two pictures of eight rows, each row an I_PCM MB followed by CHAIN_LEN intra MBs, every one the
    left neighbour of the next (dependency levels 1 .. CHAIN_LEN: with three list levels the deeper ones
    go to the walk in the same launch).  The MB row above a chain is I_PCM (all of A, B, C, D there) or
    inter (A alone).  The MBs at odd positions are I_4x4 with a DC-only residual in every 4x4 block
    (levels -8 .. 8, residuals within +-27: far inside check_bounds), the others run through the
    three kinds."""
    W, H = W_MBS, H_MBS
    pics, refs, sites = [], [], []

    def make(pi, extra):
        rng = np.random.default_rng([seed, pi])
        base = random_base(rng, W, H, 8)
        T, pcm = {}, set()
        for r, y in enumerate(range(1, H, 2)):
            above_pcm = (r + pi) % 2 == 0
            pcm.add((0, y))
            if above_pcm:
                pcm |= {(x, y - 1) for x in range(W)}
            for i in range(CHAIN_LEN):
                mask = (1, int(above_pcm), int(above_pcm), int(above_pcm))
                s = _drawn_spec(rng, 0 if i % 2 else (i // 2 + r + pi) % 3, mask, "chain")
                if i % 2:
                    s["dc"] = [int(v) for v in rng.integers(1, 9, 16) * rng.choice((-1, 1), 16)]
                T[(1 + i, y)] = s
        if extra:                                        # among the inter MBs right of a chain
            T[(12, 3 - 2 * pi)] = _drawn_spec(rng, 0, (0, 0, 0, 0), "chain")
        p = realise(L, pi, 2, W, H, T, pcm, base)
        return p, base, [dict(pic=pi, mb=k, tag="chain", mask=v["mask"]) for k, v in T.items()]
    for pi in range(2):
        p, base, mine = make(pi, False) if pi == 0 else _last_odd(lambda extra: make(pi, extra))
        pics.append(p)
        sites += mine
        refs.append(tuple(np.ascontiguousarray(a) for a in base))
    return X.Case(name, pics, refs, info=dict(sites=sites))


def levels_of(p: synth.Picture):
    """The dependency level of every MB as DESIGN.md states it: 0 for inter and I_PCM MBs, else
    1 + the largest level among the intra neighbours A, B, C, D."""
    W, H = p.cfg.width_mbs, p.cfg.height_mbs
    lv = np.zeros((H, W), np.int64)
    for a, m in enumerate(p.mbs):
        if int(m["flags"]) & A.MBF_INTRA and int(m["mb_type"]) != A.I_PCM:
            x, y = a % W, a // W
            nb = [(x - 1, y), (x, y - 1), (x + 1, y - 1), (x - 1, y - 1)]
            lv[y, x] = 1 + max([int(lv[ny, nx]) for nx, ny in nb if 0 <= nx < W and ny >= 0], default=0)
    return lv


def pairable_level1(p: synth.Picture) -> int:
    """How many MBs the first level's pair list holds: I_4x4, not lossless, level 1."""
    lv = levels_of(p).ravel()
    return sum(1 for a, m in enumerate(p.mbs) if lv[a] == 1 and int(m["mb_type"]) == A.I_4x4 and not int(m["flags"]) & A.MBF_BYPASS)


# ---------------------------------------------------------------- MBAFF: generated, then overwritten
# seed 0x1A7 left 2 of the 144 I_4x4 (blkIdx, mode) out at this size; 0x1A8 holds them all
MBAFF_SEED, MBAFF_W, MBAFF_H, MBAFF_PICS = 0x1A8, 12, 16, 4


def build_i_mbaff(L, name="i_mbaff"):
    """MBAFF frames as the generator draws them (CIP, mostly intra, many I_PCM MBs: only modes that are
    legal under the reference's MBAFF availability), then every level of the intra MBs zeroed (cbp and
    cbp_blks with them), every I_PCM MB's samples and the DPB planes replaced by value patterns and
    seeded random bytes.  No restatement covers MBAFF neighbours: the case is pinned to the reference."""
    pics = []
    cfg = synth.default_cfg(L, 3, MBAFF_W, MBAFF_H, structure=A.MBAFF_FRAME, constrained_intra=1, intra_permille=700,
                            pcm_permille=350, transform8x8=1, deblock_idc=1, wp_mode=0, num_refs=2, seed=MBAFF_SEED)
    names = ("random",) + PATTERNS
    for i in range(MBAFF_PICS):
        p = synth.picture(L, cfg, i)
        rng = np.random.default_rng([MBAFF_SEED, i])
        pool, off, k = [], 0, 0
        for m in p.mbs:                                  # storage order: coef_off only has to be consistent
            t, intra = int(m["mb_type"]), int(m["flags"]) & A.MBF_INTRA
            o = int(m["coef_off"])
            if t == A.I_PCM:
                lv = np.concatenate([pattern_mb(names[(k + i) % len(names)], w, h, rng).ravel() for w, h in ((16, 16), (8, 8), (8, 8))])
                lv = lv.view(np.int16)
                k += 1
            elif intra:
                m["cbp"], m["cbp_blks"] = 0, 0
                lv = np.zeros(16, np.int16) if t == A.I_16x16 else None
            else:
                lv = p.levels[o:o + level_count(m)].copy()
            m["coef_off"] = off
            if lv is not None and len(lv):
                pool.append(lv)
                off += len(lv)
        p.levels = np.concatenate(pool + [np.zeros(8, np.int16)])
        want = p.mbs["cbp_blks"].copy()
        X.recompute_blks(p)
        assert (p.mbs["cbp_blks"] == want).all()
        X.check_bounds(p)
        pics.append(p)
    refs = []
    for s, planes in enumerate(synth.refpics(L, cfg)):
        rng = np.random.default_rng([MBAFF_SEED, 100 + s])
        refs.append(tuple(np.ascontiguousarray(np.where(rng.integers(0, 4, a.shape) == 0, rng.integers(0, 2, a.shape) * 255,
                                                        rng.integers(0, 256, a.shape)).astype(np.uint8)) for a in planes))
    return X.Case(name, pics, refs, info=dict(seed=MBAFF_SEED, size=(MBAFF_W, MBAFF_H)))


def mbaff_census(c):
    """{(kind, mode, field MB?)}, {(I_4x4 blkIdx, mode)}, {(I_8x8 blk, mode)} of the intra MBs."""
    kinds, c4, c8 = set(), set(), set()
    for p in c.pics:
        for m in p.mbs:
            t = int(m["mb_type"])
            if not int(m["flags"]) & A.MBF_INTRA or t == A.I_PCM:
                continue
            fld = bool(int(m["flags"]) & A.MBF_FIELD)
            kinds.add(("c", int(m["chroma_mode"]), fld))
            if t == A.I_16x16:
                kinds.add(("i16", int(m["i16_mode"]), fld))
                continue
            for b in range(16 if t == A.I_4x4 else 4):
                mode = (int(m["ipred"][b >> 1]) >> ((b & 1) * 4)) & 15
                kinds.add(("i4" if t == A.I_4x4 else "i8", mode, fld))
                (c4 if t == A.I_4x4 else c8).add((b, mode))
    return kinds, c4, c8


I_CASES = {
    "i_4x4": lambda L: build_i_nxn(L, "i_4x4", A.I_4x4, 41),
    "i_8x8": lambda L: build_i_nxn(L, "i_8x8", A.I_8x8, 43),
    "i_16x16": lambda L: build_i_16(L, "i_16x16", 47),
    "i_edges": lambda L: build_i_edges(L),
    "i_chain": lambda L: build_i_chain(L),
    "i_422": lambda L: build_i_16(L, "i_422", 53, chroma_format=2),
    "i_top": lambda L: build_i_field(L, "i_top", A.TOP_FIELD, 59),
    "i_bottom": lambda L: build_i_field(L, "i_bottom", A.BOTTOM_FIELD, 59),
    "i_mbaff": lambda L: build_i_mbaff(L),
}
I_PLAIN = ["i_4x4", "i_8x8", "i_16x16", "i_edges", "i_chain"]          # frames, 4:2:0
I_RESTATED = I_PLAIN + ["i_422", "i_top", "i_bottom"]


# ---------------------------------------------------------------- the census
# the availability bits (index into A, B, C, D) an I_8x8 mode reads besides those it needs: through the
# reference-sample filter the corner reaches p'[0, -1] and p'[-1, 0], the upper right p'[7, -1]
I8_READS = {0: (2, 3), 1: (3,), 3: (2, 3), 7: (2, 3), 4: (2,), 5: (2,), 6: (), 8: (3,)}


def reads(kind, mode, bits):
    """The bits whose flip must change the block, given that the mode stays legal."""
    if kind == "i4":
        return {2: (0, 1), 3: (2,), 7: (2,)}.get(mode, ())
    if kind == "i8":
        if mode == 2:
            aA, aB = bits[0], bits[1]
            return (0, 1) + ((2,) if aB else ()) + ((3,) if aA or aB else ())
        return I8_READS[mode]
    return (0, 1) if mode == (2 if kind == "i16" else 0) else ()


_census = {}


def census(name):
    """The case restated, once per process: per picture whether it equals the oracle's reconstruction,
    and every logged block with the mutation results: others (every other legal mode changes the
    bytes), flips {bit: changed}."""
    if name in _census:
        return _census[name]
    c = X.build(name)
    entries, equal = [], []
    for pi, p in enumerate(c.pics):
        fld = int(p.pic["structure"][0]) != A.FRAME
        base = c.refs[pi if not fld else 0]
        planes = [(a[0::2] if fld else a).astype(np.int64).tolist() for a in base]

        def visit(e, redo, pi=pi):
            e["pic"] = pi
            kind, mode, bits = e["kind"], e["mode"], e["bits"]
            needs = NXN_NEEDS if kind in ("i4", "i8") else I16_NEEDS if kind == "i16" else CHROMA_NEEDS
            iD = 3 if kind in ("i4", "i8") else 2
            lg = legal(needs, bits[0], bits[1], bits[iD])
            assert mode in lg, (e["mb"], kind, mode, bits)
            alts = [redo(mode=m) for m in lg if m != mode]
            e["others"] = all(r != e["out"] for r in alts)
            e["flips"] = {}
            dc = kind in ("cb", "cr") and mode == 0
            rows = lambda r, blk: [row[(blk & 1) * 4:(blk & 1) * 4 + 4] for row in r[(blk >> 1) * 4:(blk >> 1) * 4 + 4]]
            if dc:                           # per 4x4 chroma block
                e["blk_others"] = [all(rows(r, b) != rows(e["out"], b) for r in alts) for b in range(len(e["blocks"]))]
                e["blk_flips"] = {}
            for i in range(len(bits)):
                nb = tuple(b ^ (j == i) for j, b in enumerate(bits))
                if mode not in legal(needs, nb[0], nb[1], nb[iD]):
                    continue
                r = redo(bits=nb)
                if r is not None:
                    e["flips"][i] = r != e["out"]
                    if dc:
                        e["blk_flips"][i] = [rows(r, b) != rows(e["out"], b) for b in range(len(e["blocks"]))]
            entries.append(e)
        intra_restate(p, planes, visit=visit)
        rec = O.decode(p, c.refs, stage="recon")
        equal.append(all(np.array_equal(np.array(planes[k], np.uint8), rec[k]) for k in range(3)))
    _census[name] = (entries, equal)
    return _census[name]


def required_cells(chroma_blocks=4):
    """The cells the census requires, from the legality rules and the block geometry alone: {kind: set}
    (chroma_blocks: 4x4 blocks per chroma plane of an MB, 4 in 4:2:0 and 8 in 4:2:2)."""
    req = {"i4": set(), "i8": set(), "i16": set(), "c": set(), "cdc": set()}
    for mask in MASKS:
        for b in range(16):
            aA, aB, tv, aD = avail4(b, mask)
            for mode in legal(NXN_NEEDS, aA, aB, aD):
                req["i4"].add((b, mode) + ((aA, aB) if mode == 2 else (tv,) if mode in (3, 7) else ()))
        for b in range(4):
            bits = avail8(b, mask)
            for mode in legal(NXN_NEEDS, bits[0], bits[1], bits[3]):
                req["i8"].add((b, mode, bits[0], bits[1], bits[2] if bits[1] else 0, bits[3]))
        avA, avB, _, avD = mask
        for mode in legal(I16_NEEDS, avA, avB, avD):
            req["i16"].add((mode, avA, avB, avD))
        for pl in ("cb", "cr"):
            for mode in legal(CHROMA_NEEDS, avA, avB, avD):
                req["c"].add((pl, mode, avA, avB, avD))
            for blk in range(chroma_blocks):
                req["cdc"].add((pl, blk, avA, avB))
    return req


def cell_of(e):
    kind, mode, bits = e["kind"], e["mode"], e["bits"]
    if kind == "i4":
        return (e["blk"], mode) + ((bits[0], bits[1]) if mode == 2 else (bits[2] if bits[1] else 0,) if mode in (3, 7) else ())
    if kind == "i8":
        return (e["blk"], mode, bits[0], bits[1], bits[2] if bits[1] else 0, bits[3])
    if kind == "i16":
        return (mode,) + tuple(bits)
    return (kind, mode) + tuple(bits)


# how many cells required_cells() holds in 4:2:0, counted by hand from the rules (a changed rule shows here)
# I_4x4: 9 inner blocks x 9; row 0, bx 1 and 2: 10 each, bx 3: 12 (two tv); column 0: 10 each; block 0: 12.
# I_8x8 (the upper right counted only where the top is there): blk 0 23 + 8, blk 1 18 + 3, blk 2 13, blk 3 9.
CELL_COUNTS = {"i4": 81 + 20 + 12 + 30 + 12, "i8": 31 + 21 + 13 + 9, "i16": 8 + 4 + 4 + 1, "c": 2 * 17, "cdc": 2 * 4 * 4}
