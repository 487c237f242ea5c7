"""Family S of tests/extremes.py ("strength from motion", TEST INFRASTRUCTURE): directed pictures
whose only filtered edges are the ones 8.7.2.1 decides by comparing the motion of two blocks
(bS 0 against bS 1), each table row of that rule laid on its thresholds.

Every picture is ONE-DIMENSIONAL.  In a vertical-edge case (_v) every DPB plane is a function of x
only (a ramp of 4-sample cells), every block's mvx, reference and prediction direction are
functions of its block column only, there is no residual, no intra MB and one QP: the
reconstruction is a function of x, so the only steps the loop filter finds are those across vertical
edges.  (Once two neighbouring segments of one edge are filtered under different bS their rows
differ by up to tc, and the horizontal edge between them is no longer idle: the census restates
the whole filter from the restated bS instead of assuming it.)  mvy is free per block: dmvx rows of
the table sit on whole column edges, dmvy rows on single 4-line segments.  A horizontal-edge case
(_h) is the transposition.  A wrong 0 / 1 then changes samples wherever the edge's step is live.

Layout (logical picture, transposed for _h).  Block columns come in units:
  O  two columns of one 8x8 block column, P | Q: the designed edge is inside an 8x8 block (edges 1
     and 3 of an MB), so P and Q share ref_idx and direction;
  E  four columns P P | Q Q: the designed edge is an 8x8 boundary (an MB edge when the unit starts
     on column 2 of an MB, edge 2 otherwise); P and Q may name different entries;
  F  two filler columns.
Edges between units are not designed; the census restates their bS like every other.

Rows 13 / 14 flag an MB of MB row 0 as 8x8-transform / P_Skip.  The 8x8-transform MB keeps 4x4
blocks with differing vectors, which no bitstream carries (cbp 0 has no transform_size_8x8_flag):
that its odd edges are skipped BEFORE the motion comparison shows only so.  The skipped MB has one
vector, as the reference predicts it from one: its inner edges are live and must stay unfiltered,
but the rule cannot be told from the motion comparison there.
"""
from __future__ import annotations

import ctypes

import numpy as np

import _oracle as O
import extremes as X
from h264r import _abi as A
from h264r import synth

X0, Y0 = 16, -8             # the base vector (quarter samples): one cell to the right
FAR = 48                    # a second base, far from the first in both components


def mot(p0=None, x0=0, p1=None, x1=0, v0=0, v1=0):
    """The motion of one block column: picture names per list (None: unused), which list entry of that
    picture (0 the first, 1 a second entry with equal weights, 2 one with another offset), mvx."""
    return dict(pic=(p0, p1), var=(v0, v1), x=(x0 if p0 else 0, x1 if p1 else 0))


def seg(row, bs, py, qy, sx=0, sy=0):
    """One segment design: table row, expected bS, mvy of P and of Q per list."""
    return dict(row=row, bs=bs, py=py, qy=qy, sx=sx, sy=sy)


def _sgn(v):
    return (v > 0) - (v < 0)


def sp_dx(dx, lim, l=0, pic="A", var=(0, 0), kind=None, x0=X0):
    """Rows 1-4 (row 6 when the two sides name the picture through different entries): one list,
    one picture, a difference of dx along the designed direction on the whole edge, and across it
    0, +-(limit - 1), +-limit (and +-3 where the limit is 2) on its segments.  lim = (limit along,
    limit across): (4, 4) in frames; in field pictures the limit on mvy is 2, which is the limit across
    in a _v case and the limit along in a _h case."""
    lx, lim = lim
    one = lambda x, v: mot(pic, x, None, 0, v) if l == 0 else mot(None, 0, pic, x, 0, v)
    yy = lambda y: (y, 0) if l == 0 else (0, y)
    segs = []
    for dy in (0, lim - 1, 1 - lim, lim, -lim) + ((3, -3) if lim == 2 else ()):
        near = abs(dx) < lx and abs(dy) < lim
        row = 6 if var[0] != var[1] else 1 if (dx, dy) == (0, 0) else 2 if dy == 0 else 3 if dx == 0 else 4
        segs.append(seg(row, 0 if near else 1, yy(Y0), yy(Y0 + dy), _sgn(dx), _sgn(dy)))
    return dict(P=one(x0, var[0]), Q=one(x0 + dx, var[1]), segs=segs, kind=kind)


def sp_limits(lim, hz):
    """Row 5: vectors at the level limits ((8191, 2047) against (8188, 2044): limit - 1 away in both
    components of a frame).  Both sides read the plane's clamped border, so the step that makes the
    edge live comes from naming the picture through an entry with another offset."""
    a, b = ((2047, 8191), (-2048, -8192)) if hz else ((8191, 2047), (-8192, -2048))
    one = lambda P, Q, bs: dict(P=mot("A", P[0]), Q=mot("A", Q[0], v0=2), kind=None,
                                segs=[seg(5, bs, (P[1], 0), (Q[1], 0), _sgn(Q[0] - P[0]), _sgn(Q[1] - P[1]))])
    return [one(a, (a[0] + 1 - lim[0], a[1] + 1 - lim[1]), 0), one(a, b, 1), one(b, b, 0), one(b, a, 1)]


def sp_other(lim, other):
    """Row 7 (row 8 across a slice boundary): another picture, the same vector -> 1; the picture
    `other` is slot B of a frame case and the other parity of slot A in a field case."""
    s = [seg(7, 1, (Y0, 0), (Y0, 0))]
    return [dict(P=mot("A", X0), Q=mot(other, X0), segs=s, kind=None),
            dict(P=mot(other, X0), Q=mot("A", X0), segs=s, kind=None)]


def p_specs(lim, other="B", t8=True, hz=False):
    """(O units, E units on MB edges, E units on edge 2) of a P case; lim: see sp_dx."""
    n, f = lim[0] - 1, lim[0]                      # near and far along the designed direction
    dxs = (0, n, -n, f, -f)
    O_ = []
    if t8:
        O_ += [sp_dx(f, lim, kind="T"), sp_dx(-f, lim, kind="T")]                 # row 13
    skip = dict(P=mot("A", X0), Q=mot("A", X0), segs=[seg(1, 0, (Y0, 0), (Y0, 0))], kind="S")
    O_ += [skip, skip]                                                             # row 14
    O_ += [sp_dx(d, lim) for d in dxs] + [sp_dx(d, lim, x0=X0 + 4) for d in (n, -f)]
    if not t8:
        O_ += [sp_dx(d, lim, x0=X0 - 4) for d in (-n, f)]
    six = [sp_dx(d, lim, var=(0, 1)) for d in (n, -n, f, -f, 0)]
    oth, lims = sp_other(lim, other), sp_limits(lim, hz)
    # MB edges; units 1..3 of the first picture sit on slice boundaries
    E0 = [sp_dx(0, lim)] + oth + [sp_dx(d, lim) for d in (n, -n, f, -f)] + [six[4], lims[0]]
    E2 = lims + six[:4] + [oth[1]]
    return O_, E0, E2


def bi(P, Q, segs):
    return dict(P=P, Q=Q, segs=segs, kind=None)


def b_specs(lim, n1="B"):
    """(O units, E units) of a B case: rows 1-4 from list 0 and from list 1, rows 9-12.  Pictures A
    and n1 (slot B; the other parity of slot A in field pictures) are entries 0 and 1 of both lists."""
    (Lx, L), F = lim, FAR
    Nx, N = Lx - 1, L - 1
    AB = lambda x0, x1: mot("A", x0, n1, x1)
    BA = lambda x0, x1: mot(n1, x0, "A", x1)
    AA = lambda x0, x1: mot("A", x0, "A", x1)
    z = (Y0, Y0 + 20)
    # --- O units: P and Q share ref_idx and direction
    nine = [
        bi(AB(X0, F), AB(X0 + Lx, F), [seg(9, 1, z, z, 1, 0)]),                       # the L0 pair alone at the limit (x)
        bi(AB(X0, F), AB(X0, F - Lx), [seg(9, 1, z, z, -1, 0)]),                      # the L1 pair alone (x)
        bi(AB(X0, F), AB(X0 + Nx, F - Nx), [                                          # both at limit - 1, then y decides
            seg(9, 0, z, (z[0] + N, z[1] - N), 1, 1), seg(9, 1, z, (z[0] + L, z[1]), 1, 1),
            seg(9, 1, z, (z[0], z[1] - L), 1, -1), seg(9, 0, z, (z[0] - N, z[1] + N), 1, -1),
            seg(9, 1, z, (z[0] - L, z[1] + N), 1, -1)]),
    ]
    eleven = [
        bi(AA(X0, F), AA(X0 + Nx, F - Nx), [seg(11, 0, z, (z[0] + N, z[1] - N)), seg(11, 0, z, z)]),      # direct near
        bi(AA(X0, F), AA(F, X0), [seg(11, 0, z, (z[1], z[0])), seg(11, 0, z, (z[1] - N, z[0] + N))]),   # crossed near
        bi(AA(X0, F), AA(X0 + 16, F + 20), [seg(11, 1, z, z), seg(11, 1, z, (z[1], z[0]))]),            # neither (x)
        bi(AA(X0, X0 + 1), AA(X0 + 1, F), [seg("11m", 1, (Y0, Y0), (Y0, Y0))]),                         # mixed (x)
        bi(AA(X0, X0), AA(X0, X0), [                                                                  # the same on y
            seg(11, 0, z, (z[0] + N, z[1] - N)), seg(11, 0, z, (z[1], z[0])), seg(11, 1, z, (z[0] + 10, z[1] + 10)),
            seg("11m", 1, (Y0, Y0 + 1), (Y0 + 1, Y0 + 20)), seg("11m", 1, (Y0 + 1, Y0), (Y0 + 20, Y0 + 1)),
            seg("11m", 1, (Y0 + 1, Y0 + 20), (Y0, Y0 + 1))]),        # mirrored: it is P that has the vector without a partner
        bi(AA(X0 + 1, F), AA(X0, X0 + 1), [seg("11m", 1, (Y0, Y0), (Y0, Y0))]),                         # mixed, mirrored (x)
    ]
    # list 0 alone first: in a _v case MB columns 0..3, whose waves of MB rows 0 and 2 hold no list-1 motion
    O_ = [sp_dx(d, lim) for d in (0, Nx, -Nx, Lx, -Lx)] + [sp_dx(d, lim, x0=X0 + 4) for d in (-Nx, Lx, 0)]
    O_ += nine + eleven + [sp_dx(d, lim, l=1) for d in (0, Nx, -Nx, Lx, -Lx)]
    # --- E units: the two sides may differ in entries and direction
    ten = [
        bi(AB(X0, F), BA(F, X0), [                                                   # crossed equal, direct far -> 0
            seg(10, 0, z, (z[1], z[0])), seg(10, 0, z, (z[1] - N, z[0] + N)), seg(10, 1, z, (z[1], z[0] + L)),
            seg(10, 1, z, (z[1] - L, z[0]))]),
        bi(AB(X0, F), BA(X0, F), [seg(10, 1, z, z)]),                                # direct equal, crossed far -> 1
        bi(AB(X0, F), BA(F + Nx, X0 - Nx), [seg(10, 0, z, (z[1], z[0]))]),
        bi(AB(X0, F), BA(F + Lx, X0), [seg(10, 1, z, (z[1], z[0]))]),
    ]
    twelve = [
        bi(mot("A", X0), mot(None, 0, "A", X0), [                                    # L0 only against L1 only: by vector
            seg(12, 0, (Y0, 0), (0, Y0)), seg(12, 0, (Y0, 0), (0, Y0 + N)), seg(12, 1, (Y0, 0), (0, Y0 + L)),
            seg(12, 1, (Y0, 0), (0, Y0 - L))]),
        bi(mot("A", X0), mot(None, 0, "A", X0 + Lx), [seg(12, 1, (Y0, 0), (0, Y0))]),
        bi(mot(None, 0, "A", X0), mot("A", X0 - Nx), [seg(12, 0, (0, Y0), (Y0, 0))]),
        bi(mot("A", X0), AB(X0, F), [seg(12, 1, (Y0, 0), (Y0, Y0))]),                # (A, -) against (A, B)
        bi(mot("A", X0), AA(X0, X0), [seg(12, 1, (Y0, 0), (Y0, Y0))]),               # (A, -) against (A, A)
        bi(AA(X0, X0), mot("A", X0), [seg(12, 1, (Y0, Y0), (Y0, 0))]),
    ]
    E_ = ten[:2] + twelve[:3] + [sp_dx(Nx, lim)] + ten[2:] + twelve[3:] + [sp_dx(-Lx, lim)]
    return O_, E_


# ---------------------------------------------------------------- realisation
def _content(name, n, cell, chroma):
    """The 1-D samples of picture `name` along the designed direction: a ramp of cells (one 4x4
    block's extent: 4 luma samples) with a step of 5 (chroma: 3) per cell, offset per picture."""
    off = {"A": 0, "B": 9, "a": 4, "b": 13, "C": 17}[name]
    k = np.arange(n) // cell
    return ((170 + off - 3 * k) if chroma else (190 + off - 5 * k)).astype(np.uint8)


def _layout(kind, units, Wl, at):
    """One picture's columns: [(column of the designed edge or None, spec)] -> per column (spec, side)."""
    cols, designed = [], []
    def filler():
        cols.extend([(None, None)] * 2)
    if kind == "E0":
        filler()
    while len(cols) + (2 if kind == "O" else 4) <= 4 * Wl - 2:       # the last two columns read the clamped border
        sp = units[at[0] % len(units)]
        at[0] += 1
        if kind == "O":
            designed.append((len(cols) + 1, sp))
            cols += [(sp, "P"), (sp, "Q")]
        else:
            designed.append((len(cols) + 2, sp))
            cols += [(sp, "P"), (sp, "P"), (sp, "Q"), (sp, "Q")]
    while len(cols) < 4 * Wl:
        filler()
    return cols, designed


def build_s(L, name, horizontal: bool, plan, field_case=False, chroma_format=0, qps=(44, 48, 46)):
    """plan: [(unit kind "O" / "E0" / "E2", the units' queue, B picture?, structure)] per picture."""
    W, H = 6, 4
    Wl, Hl = (H, W) if horizontal else (W, H)
    idc = A.idc_of(chroma_format)
    pics, design = [], []
    n1 = "a" if field_case else "B"
    slot = {"A": 0, "B": 1, "a": 0 | A.REF_BOTTOM, "b": 1 | A.REF_BOTTOM, "C": 2}
    counters = {}
    for pi, (ukind, units, kind_b, structure) in enumerate(plan):
        over = dict(num_refs=4, transform8x8=1, deblock_idc=0, wp_mode=0 if kind_b and pi % 2 == 0 else 1,
                    num_slices=1 if kind_b else 4, structure=structure, qp_min=20, qp_max=40)
        if chroma_format:
            over["chroma_format"] = chroma_format
        cfg = synth.default_cfg(L, 4 if kind_b else 3, W, H, **over)
        p = synth.picture(L, cfg, pi)
        qp = qps[pi % len(qps)]
        cols, des = _layout(ukind, units, Wl, counters.setdefault(id(units), [0]))
        # slices of the logical MBs: _v four slices starting at MBs 0, 2, W + 3, 2 W + 4 (so that the MB
        # edges 2, 3 and 4 of MB rows 0, 1 and 2 are slice boundaries); _h one slice per physical MB row
        def slice_of(cx, cy):
            if kind_b:
                return 0
            if horizontal:
                return cx
            return sum(cy * Wl + cx >= b for b in (2, Wl + 3, 2 * Wl + 4))
        # the lists: P slices alternate between two orders; entries 2 and 3 name picture A again, entry 3
        # with another offset.  B slices: A and n1 in both lists.
        orders = [["A", n1, "A", "A"], [n1, "A", "A", "A"]]
        for s, sl in enumerate(p.slices):
            sl["ref_slot"][:] = -1
            names = ["A", n1] if kind_b else orders[s % 2]
            for l in range(2 if kind_b else 1):
                sl["ref_slot"][l][:len(names)] = [slot[n] for n in names]
                sl["num_ref"][l] = len(names)
            sl["luma_log2_wd"] = sl["chroma_log2_wd"] = 5
            sl["wp_weight"][:] = 32
            sl["wp_offset"][:] = 0
            if not kind_b:
                sl["wp_offset"][0][3][:] = 3
            sl["implicit_w1"][:] = 32

        def entry(s, l, nm, var):
            if kind_b:
                return ["A", n1].index(nm)
            o = orders[s % 2]
            return [i for i, n in enumerate(o) if n == nm][var]
        # MB kinds (MB row 0 only) and records
        kinds = {}
        for c, (sp, side) in enumerate(cols):
            if sp is not None and sp["kind"]:
                assert kinds.setdefault(c // 4, sp["kind"]) == sp["kind"]
        mbs = np.zeros((Hl, Wl), A.MB_DTYPE)
        for cy in range(Hl):
            for cx in range(Wl):
                m = mbs[cy, cx]
                k = kinds.get(cx) if cy == 0 else None
                m["mb_type"] = A.P_SKIP if k == "S" else A.P_8x8
                m["flags"] = A.MBF_T8x8 if k == "T" else 0
                m["slice"] = slice_of(cx, cy)
                X._set_qp(m, qp)
        # motion
        ref = np.full((2, 4 * Hl, 4 * Wl), -1, np.int64)
        mvx = np.zeros((2, 4 * Hl, 4 * Wl), np.int64)
        mvy = np.zeros((2, 4 * Hl, 4 * Wl), np.int64)
        fill = mot("A", X0)
        for c, (sp, side) in enumerate(cols):
            mo = fill if sp is None else sp[side]
            for r in range(4 * Hl):
                sg = None if sp is None else sp["segs"][(r + pi) % len(sp["segs"])]
                for l in range(2):
                    if mo["pic"][l] is None:
                        continue
                    ref[l, r, c] = entry(slice_of(c // 4, r // 4), l, mo["pic"][l], mo["var"][l])
                    mvx[l, r, c] = mo["x"][l]
                    mvy[l, r, c] = Y0 if sg is None else sg["py" if side == "P" else "qy"][l]
        assert (ref[:, :, 0::2] == ref[:, :, 1::2]).all() and (ref[:, 0::2] == ref[:, 1::2]).all()      # per 8x8 block
        # the designed segments, with the precedence of the MB kinds of MB row 0
        dl = []
        for c, sp in des:
            for r in range(4 * Hl):
                sg = sp["segs"][(r + pi) % len(sp["segs"])]
                row, bs = sg["row"], sg["bs"]
                k = kinds.get(c // 4) if r < 4 else None
                if k == "T" and c % 2 == 1:
                    row, bs = (13 if bs else row), 0
                elif k == "S" and c % 4:
                    row, bs = 14, 0
                sp_, sq_ = slice_of((c - 1) // 4, r // 4), slice_of(c // 4, r // 4)
                if sp_ != sq_:
                    row = 8
                if horizontal:                     # rows 2 / 3 and the signs name the picture's own mvx / mvy
                    row = {2: 3, 3: 2}.get(row, row)
                sx, sy = (sg["sy"], sg["sx"]) if horizontal else (sg["sx"], sg["sy"])
                dl.append(dict(c=c, r=r, bs=bs, row=row, sx=sx, sy=sy,
                               same_idx=bool((ref[:, r, c] == ref[:, r, c - 1]).all()),
                               same_pic=sp["P"]["pic"] == sp["Q"]["pic"], single=sp["P"]["pic"][1] is None and sp["Q"]["pic"][1] is None))
        # realise (transposed for horizontal edges: x and y change places)
        T = (lambda a: np.ascontiguousarray(np.swapaxes(a, -1, -2))) if horizontal else (lambda a: np.ascontiguousarray(a))
        p.mbs[:] = T(mbs).ravel()
        p.levels = np.zeros(8, np.int16)
        px, py = (mvy, mvx) if horizontal else (mvx, mvy)
        p.mv[:] = ((T(px) & 0xFFFF) | ((T(py) & 0xFFFF) << 16)).astype(np.uint32)
        p.ref_idx[:] = T(ref).astype(np.int8)
        X.check_bounds(p)
        pics.append(p)
        design.append(dict(segs=dl, qp=qp, kinds=kinds))
    # the DPB: slot 0 holds A (a field case: A in its top rows, a in its bottom rows), slot 1 B / b
    cw, ch = A.chroma_mb(idc)
    def plane(nm, k):
        mw, mh = (16, 16) if k == 0 else (cw, ch)             # the plane's samples per MB
        along, across = (mh, mw) if horizontal else (mw, mh)
        a = np.repeat(_content(nm, along * Wl, along // 4, k > 0)[None, :], across * Hl, 0)
        return np.ascontiguousarray(a.T) if horizontal else a
    refs = []
    for top, bot in (("A", "a"), ("B", "b"), ("C", "C"), ("C", "C")):
        planes = []
        for k in range(3):
            t = plane(top, k)
            if field_case:
                f = np.empty((2 * t.shape[0], t.shape[1]), np.uint8)
                f[0::2], f[1::2] = t, plane(bot, k)
                t = f
            planes.append(np.ascontiguousarray(t))
        refs.append(tuple(planes))
    refs = refs[:L.h264r_synth_ref_frames(ctypes.byref(pics[0].cfg))]      # a field case's DPB: (num_refs + 1) / 2 frames
    return X.Case(name, pics, refs, chroma_format=idc, info=dict(design=design, horizontal=horizontal,
                                                                 lim=2 if field_case else 4))


def _plan(Wl, queues, structures=(A.FRAME,)):
    """Pictures until every queue is laid out once: [(unit kind, queue, B picture?, structure)]."""
    plan = []
    for kind, q, is_b in queues:
        cap = {"O": 2 * Wl - 1, "E0": Wl - 1, "E2": Wl - 1}[kind]
        for _ in range(-(-len(q) // cap)):
            plan.append((kind, q, is_b, structures[len(plan) % len(structures)]))
    assert len(plan) <= 8, len(plan)
    return plan


def build_s_p(L, name, horizontal, chroma_format=0):
    O_, E0, E2 = p_specs((4, 4), "B", t8=chroma_format == 0, hz=horizontal)
    plan = _plan(4 if horizontal else 6, [("O", O_, False), ("E0", E0, False), ("E2", E2, False)])
    return build_s(L, name, horizontal, plan, chroma_format=chroma_format)


def build_s_b(L, name, horizontal):
    O_, E_ = b_specs((4, 4))
    h = len(E_) // 2
    plan = _plan(4 if horizontal else 6, [("O", O_, True), ("E0", E_[:h], True), ("E2", E_[h:], True)])
    return build_s(L, name, horizontal, plan)


def build_s_field(L, name, horizontal):
    """Top- and bottom-field P pictures and B field pictures: the limit on mvy is 2 (on mvx still
    4), and the two parities of one slot are different pictures (picture "a": the bottom field of
    slot 0).  A shorter table than the frame cases', one layout per picture."""
    lim = (2, 4) if horizontal else (4, 2)
    n, f = lim[0] - 1, lim[0]
    O_, E0, E2 = p_specs(lim, "a", hz=horizontal)
    po = O_[:7 if horizontal else 11]                             # one picture: rows 13, 14, then rows 1-4
    six, lims, oth = [sp_dx(d, lim, var=(0, 1)) for d in (n, -f)], sp_limits(lim, horizontal), sp_other(lim, "a")
    pe0 = [sp_dx(0, lim)] + oth + [sp_dx(f, lim), sp_dx(-f, lim), six[1]]
    pe2 = [lims[0], lims[1], six[0], oth[1]]
    bo_, be_ = b_specs(lim, "a")
    # of b_specs: both pairs at limit - 1 (row 9), the mixed pairing on y (row 11); crossed lists (row
    # 10), L0 only against L1 only and (A, -) against (A, a) (row 12)
    bo = [sp_dx(d, lim) for d in (0, n, -f)] + [bo_[10], bo_[15], sp_dx(-n, lim, l=1), sp_dx(f, lim, l=1)]
    be = [be_[0], be_[2], be_[8]]
    plan = _plan(4 if horizontal else 6, [("O", po, False), ("E0", pe0, False), ("E2", pe2, False), ("O", bo, True),
                                          ("E0", be, True)], structures=(A.TOP_FIELD, A.BOTTOM_FIELD))
    return build_s(L, name, horizontal, plan, field_case=True)


# ---------------------------------------------------------------- MBAFF frames, vertical edges
def mb_unit(dx=0, dy=0, var=(0, 0), par=(0, 0), pq=("A", "A"), x0=X0, limits=None):
    """One unit of the MBAFF case, as a function of the MB kind (field MB or frame MB) of its columns:
    in an MBAFF frame everything is uniform along y, mvy included, so a dmvy row takes a whole edge
    too.  dy: 0, "n" / "-n" (limit - 1), "l" / "-l" (the limit), "m" / "-m" (3 in a field MB, where
    it is far).  par: the parity bit of a field MB's refIdx (refIdx 2 e + par names a field of entry
    e; a frame MB names the frame either way).  limits: (P, Q) vectors at the level limits, Q's mvy
    given for the frame MB and moved to limit - 1 in a field MB."""
    def of(field):
        ly = 2 if field else 4
        d = {0: 0, "n": ly - 1, "-n": 1 - ly, "l": ly, "-l": -ly, "m": 3 if field else 4, "-m": -3 if field else -4}[dy]
        P, Q = (x0, Y0), (x0 + dx, Y0 + d)
        if limits:
            P, Q = limits
            if Q[1] == P[1] - 3:
                Q = (Q[0], P[1] - (ly - 1))
        same = pq[0] == pq[1] and (not field or par[0] == par[1])
        far = abs(P[0] - Q[0]) >= 4 or abs(P[1] - Q[1]) >= ly
        row = 7 if not same else 5 if limits else 6 if var[0] != var[1] else \
            1 if P == Q else 2 if P[1] == Q[1] else 3 if P[0] == Q[0] else 4
        return dict(P=P, Q=Q, pq=pq, var=var, par=par, row=row, bs=int(far or not same),
                    sx=_sgn(Q[0] - P[0]), sy=_sgn(Q[1] - P[1]))
    return of


def mbaff_queues():
    u = mb_unit
    rows14 = [u(), u(3), u(-3), u(4), u(-4), u(0, "n"), u(0, "-n"), u(0, "l"), u(0, "-l"), u(0, "m"), u(0, "-m"),
              u(3, "n"), u(-3, "-n"), u(3, "-n"), u(-3, "n"), u(3, "l"), u(-3, "-l"), u(4, "n"), u(-4, "-n"), u(3, "-m"),
              u(-3, "l"), u(0, 0, x0=X0 + 4)]
    a, b = (8191, 2047), (-8192, -2048)
    inner = [u(3, "n", var=(0, 1)), u(-4, 0, var=(0, 1)), u(par=(0, 1)), u(limits=(a, (8188, 2044)), var=(0, 2)),
             u(limits=(a, b), var=(0, 2))]                       # rows 6, 7, 5 on edge 2
    # MB edges: units 1 and 3 sit between a frame pair and a field pair (row 15: identical motion -> 1)
    edges = [[u(pq=("A", "B")), u(), u(-3, "-n", var=(0, 1)), u(), u(0, "l", var=(0, 1))],
             [u(par=(1, 0)), u(), u(limits=(b, b), var=(0, 2)), u(), u(limits=(b, a), var=(0, 2))]]
    return rows14, inner, edges


def build_s_mbaff(L, name="s_mbaff_v"):
    """MBAFF P frames, vertical edges: rows 1-7 between two frame MBs and between two field MBs (mvy
    limit 2, the two parities of a frame different pictures), row 15 between a frame and a field MB.
    Every block column is uniform along y (MB kind, entries, vectors), so every horizontal edge compares
    identical motion of one kind and the output is one-dimensional too."""
    W, H = 6, 4
    rows14, inner, edges = mbaff_queues()
    plan = []
    for k in range(2):                                           # each layout under both kind patterns
        plan += [("O", rows14[:11], "FfFfFf", k), ("O", rows14[11:], "fFfFfF", k)]
    plan += [("E2", inner, "FfFfFf", 0), ("E2", inner, "FfFfFf", 1)]
    plan += [("E0", edges[0], "FFffFF", 0), ("E0", edges[1], "FFffFF", 1)]
    names = ["A", "A", "B", "A"]                                 # list 0: entries 1 and 3 name A again, 3 with another offset
    ent = {("A", 0): 0, ("A", 1): 1, ("A", 2): 3, ("B", 0): 2}
    pics, design = [], []
    for pi, (ukind, units, pattern, flip) in enumerate(plan):
        cfg = synth.default_cfg(L, 3, W, H, num_refs=4, transform8x8=0, deblock_idc=0, wp_mode=1, num_slices=1,
                                structure=A.MBAFF_FRAME, qp_min=20, qp_max=40)
        p = synth.picture(L, cfg, pi)
        qp = (44, 48, 46)[pi % 3]
        field = [(ch == "f") != bool(flip) for ch in pattern]      # per MB column
        cols, des = _layout(ukind, [dict(fn=fn) for fn in units], W, [0])
        sl = p.slices[0]
        sl["ref_slot"][:] = -1
        sl["ref_slot"][0][:4] = [{"A": 0, "B": 1}[n] for n in names]
        sl["num_ref"][0], sl["num_ref"][1] = 4, 0
        sl["luma_log2_wd"] = sl["chroma_log2_wd"] = 5
        sl["wp_weight"][:] = 32
        sl["wp_offset"][:] = 0
        sl["wp_offset"][0][3][:] = 3
        p.mbs[:] = np.zeros(W * H, A.MB_DTYPE)
        for mi, m in enumerate(p.mbs):
            m["mb_type"], m["flags"] = A.P_8x8, A.MBF_FIELD if field[mi % W] else 0
            X._set_qp(m, qp)
        p.levels = np.zeros(8, np.int16)
        p.mv[:] = 0
        p.ref_idx[:] = -1
        dl = []
        for c, (sp, side) in enumerate(cols):
            fm = field[c // 4]
            if sp is None:
                e, par, vec = 0, 0, (X0, Y0)
            else:
                d = sp["fn"](fm)
                k = 0 if side == "P" else 1
                e, par, vec = ent[(d["pq"][k], d["var"][k])], d["par"][k], d[side]
            p.ref_idx[0, :, c] = 2 * e + par if fm else e
            p.mv[0, :, c] = X.pack_mv(*vec)
        for c, sp in des:
            mixed = field[(c - 1) // 4] != field[c // 4]
            d = dict(sp["fn"](field[c // 4]))
            if mixed:
                assert d["P"] == d["Q"] and d["pq"][0] == d["pq"][1]         # row 15: identical motion and reference
                d.update(row=15, bs=1)
            dl.append(dict(c=c, bs=d["bs"], row=d["row"], sx=d["sx"], sy=d["sy"], field=field[c // 4]))
        X.check_bounds(p)
        pics.append(p)
        design.append(dict(segs=dl, qp=qp, field=field))
    refs = []
    for nm in ("A", "B", "C", "C"):
        refs.append(tuple(np.ascontiguousarray(np.repeat(_content(nm, (16 if k == 0 else 8) * W, 4 if k == 0 else 2, k > 0)[None, :],
                                                         (16 if k == 0 else 8) * H, 0)) for k in range(3)))
    return X.Case(name, pics, refs, info=dict(design=design, horizontal=False, lim=None))


def strength_restate_mbaff_v(p: synth.Picture):
    """bsV [4 H][4 W] of an MBAFF frame without residual, intra, skipped or 8x8-transform MBs whose left
    neighbour MB is of its own kind or of the other: a frame MB against a field MB is 1 whatever the
    motion; two MBs of one kind compare the blocks of one storage row, a field MB's pictures being
    fields ((slot, parity): refIdx r names parity r & 1 relative to the MB's own) and its mvy limit 2."""
    W, H = p.cfg.width_mbs, p.cfg.height_mbs
    bsV = np.zeros((4 * H, 4 * W), np.int64)
    sl = p.slices[0]

    def motion(x4, y4):
        m = p.mbs[(y4 // 4) * W + x4 // 4]
        fld = bool(int(m["flags"]) & A.MBF_FIELD)
        r = int(p.ref_idx[0, y4, x4])
        assert r >= 0 and int(p.ref_idx[1, y4, x4]) < 0 and not int(m["cbp_blks"]) and int(m["mb_type"]) == A.P_8x8
        bottom_mb = (y4 // 4) & 1
        ident = (int(sl["ref_slot"][0][r >> 1]), (r & 1) != bottom_mb) if fld else (int(sl["ref_slot"][0][r]),)
        return fld, ident, X.mv_xy(p.mv[0, y4, x4])
    for y4 in range(4 * H):
        for x4 in range(1, 4 * W):
            (fp, ip, vp), (fq, iq, vq) = motion(x4 - 1, y4), motion(x4, y4)
            if fp != fq:
                bsV[y4, x4] = 1
            else:
                bsV[y4, x4] = int(ip != iq or abs(vp[0] - vq[0]) >= 4 or abs(vp[1] - vq[1]) >= (2 if fq else 4))
    return bsV


S_CASES = {
    "s_p_v": lambda L: build_s_p(L, "s_p_v", False), "s_p_h": lambda L: build_s_p(L, "s_p_h", True),
    "s_b_v": lambda L: build_s_b(L, "s_b_v", False), "s_b_h": lambda L: build_s_b(L, "s_b_h", True),
    "s_field_v": lambda L: build_s_field(L, "s_field_v", False), "s_field_h": lambda L: build_s_field(L, "s_field_h", True),
    "s_mbaff_v": lambda L: build_s_mbaff(L),
    "s_422_v": lambda L: build_s_p(L, "s_422_v", False, chroma_format=2),
}


# ---------------------------------------------------------------- the strength derivation, restated
def strength_restate(p: synth.Picture):
    """bsV / bsH of a frame or field picture from its inputs alone (records, motion arrays, slices),
    in the rule order of the reference's strength derivation (8.7.2.1): bsV[y4][x4] is the bS of the
    vertical edge left of 4x4 block (x4, y4), bsH[y4][x4] of the horizontal edge above it."""
    W, H = p.cfg.width_mbs, p.cfg.height_mbs
    fld = int(p.pic["structure"][0]) != A.FRAME
    lim = 2 if fld else 4
    bsV = np.zeros((4 * H, 4 * W), np.int64)
    bsH = np.zeros((4 * H, 4 * W), np.int64)

    def mb(x4, y4):
        return p.mbs[(y4 // 4) * W + x4 // 4]

    def motion(x4, y4):
        sl = p.slices[int(mb(x4, y4)["slice"])]
        out = []
        for l in range(2):
            r = int(p.ref_idx[l, y4, x4])
            out.append((None if r < 0 else int(sl["ref_slot"][l][r]),) + X.mv_xy(p.mv[l, y4, x4]))
        return out

    def far(a, b):
        return abs(a[1] - b[1]) >= 4 or abs(a[2] - b[2]) >= lim

    def by_motion(P, Q):
        (p0, p1), (q0, q1) = (P[0][0], P[1][0]), (Q[0][0], Q[1][0])
        if not ((p0 == q0 and p1 == q1) or (p0 == q1 and p1 == q0)):
            return 1                                        # not the same set of pictures
        direct = far(P[0], Q[0]) or far(P[1], Q[1])
        crossed = far(P[0], Q[1]) or far(P[1], Q[0])
        if p0 != p1:
            return int(direct if p0 == q0 else crossed)
        return int(direct and crossed)                      # both lists name one picture: either pairing may match

    def special(m):
        return int(p.slices[int(m["slice"])]["slice_type"]) in (A.SLICE_SP, A.SLICE_SI)

    for y4 in range(4 * H):
        for x4 in range(4 * W):
            q = mb(x4, y4)
            sl = p.slices[int(q["slice"])]
            idc = int(sl["deblock_idc"])
            for vertical in (True, False):
                e = (x4 if vertical else y4) % 4
                nx, ny = (x4 - 1, y4) if vertical else (x4, y4 - 1)
                if idc == 1 or nx < 0 or ny < 0:
                    continue
                pm = mb(nx, ny)
                if e == 0 and idc == 2 and int(pm["slice"]) != int(q["slice"]):
                    continue
                if e & 1 and int(q["flags"]) & A.MBF_T8x8:
                    continue
                intra = bool((int(q["flags"]) | int(pm["flags"])) & A.MBF_INTRA)
                spec = special(q) or special(pm)
                pskip = int(sl["slice_type"]) == A.SLICE_P and int(q["mb_type"]) == A.P_SKIP
                strong = 4 if e == 0 and (vertical or not fld) else 3
                bq, bp = (y4 % 4) * 4 + x4 % 4, (ny % 4) * 4 + nx % 4
                coded = (int(q["cbp_blks"]) >> bq) & 1 or (int(pm["cbp_blks"]) >> bp) & 1
                one_part = e > 0 and int(q["mb_type"]) in (A.P_16x16, A.P_16x8 if vertical else A.P_8x16)
                if vertical:
                    v = strong if spec else 0 if e and pskip else strong if intra else 2 if coded else 0 if one_part else None
                else:
                    v = strong if spec or intra else 0 if e and pskip else 2 if coded else 0 if one_part else None
                if v is None:
                    v = by_motion(motion(nx, ny), motion(x4, y4))
                (bsV if vertical else bsH)[y4, x4] = v
    return bsV, bsH


def one_list_waves(p: synth.Picture):
    """inter4_one_list of csrc/mb_inter4.h on the host: per wave of k_inter4r (four consecutive MBs)
    whether no lane's block, left block or upper block has list-1 motion."""
    W, H = p.cfg.width_mbs, p.cfg.height_mbs
    used = (p.ref_idx[1] >= 0) | (p.mv[1] != 0)
    out = []
    for a0 in range(0, W * H, 4):
        any_used = False
        for a in range(a0, min(a0 + 4, W * H)):
            x0, y0 = (a % W) * 4, (a // W) * 4
            any_used |= bool(used[y0:y0 + 4, max(x0 - 1, 0):x0 + 4].any() or used[max(y0 - 1, 0):y0 + 4, x0:x0 + 4].any())
        out.append(not any_used)
    return out
