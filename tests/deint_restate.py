"""The deinterlacer of include/h264r_deinterlace.h restated from the header's text, twice: a plain scalar
loop (interp_scalar) and a vectorised numpy form (interp_numpy); tests/test_deinterlace.py holds the two to
each other.  Nothing here calls the library: geometry comes from h264r/output.py's host-side restatement of
the SPS cropping (OUT.geometry), and every byte from the functions below.

Names are the header's.  A *field* is an int32 array Hf x w: field p of a source inside one plane's cropped
rectangle.  A *source* is a frame-table row on the host, (kind, [(y, u, v)]) or (kind, [(y, u, v) of the
top field, (y, u, v) of the bottom field]), as tests/test_gpu_output_rgb.py:_sources builds them.

The numpy form also counts what the tests' coverage conditions ask about (stats=) and takes the mutations
of the definition that the tests must be able to tell from it (mutate=).
"""
import numpy as np

from h264r import output as OUT

BOB, ADAPTIVE = 0, 1
SUB = {0: (1, 1), 1: (2, 2), 2: (2, 1), 3: (1, 1)}             # SubWidthC, SubHeightC
MUTATIONS = ("second", "wrap", "no2", "nomnmx", "framerows", "zeros")


# ------------------------------------------------------------------------------ the definition, scalar
def interp_scalar(K, Pb, Pa, Qb, Qa, q, mode):
    """The interpolated rows out[2 m + q] for m = 0 .. Hf - 1, as an int32 array Hf x w."""
    Hf, w = K.shape
    cl = lambda a: min(max(a, 0), Hf - 1)
    cx = lambda a: min(max(a, 0), w - 1)
    out = np.zeros((Hf, w), np.int32)
    for m in range(Hf):
        ia, ib = cl(m + q - 1), cl(m + q)
        mu, md = cl(m - 1), cl(m + 1)
        for x in range(w):
            c, e = int(K[ia][x]), int(K[ib][x])
            if mode == BOB:
                out[m][x] = (c + e + 1) >> 1
                continue
            d = (int(Qb[m][x]) + int(Qa[m][x])) >> 1
            t0 = abs(int(Qb[m][x]) - int(Qa[m][x]))
            t1 = (abs(int(Pb[ia][x]) - c) + abs(int(Pb[ib][x]) - e)) >> 1
            t2 = (abs(int(Pa[ia][x]) - c) + abs(int(Pa[ib][x]) - e)) >> 1
            diff = max(t0 >> 1, t1, t2)
            S = lambda j: sum(abs(int(K[ia][cx(x + k + j)]) - int(K[ib][cx(x + k - j)])) for k in (-1, 0, 1))
            pr = lambda j: (int(K[ia][cx(x + j)]) + int(K[ib][cx(x - j)])) >> 1
            sp, score = (c + e) >> 1, S(0) - 1
            for s in (-1, 1):
                if S(s) < score:
                    score, sp = S(s), pr(s)
                    if S(2 * s) < score:
                        score, sp = S(2 * s), pr(2 * s)
            b = (int(Qb[mu][x]) + int(Qa[mu][x])) >> 1
            f = (int(Qb[md][x]) + int(Qa[md][x])) >> 1
            mx = max(d - e, d - c, min(b - c, f - e))
            mn = min(d - e, d - c, max(b - c, f - e))
            diff = max(diff, mn, -mx)
            out[m][x] = min(max(sp, d - diff), d + diff)
    return out


# ------------------------------------------------------------------------------ the definition, vectorised
def interp_rows(A, B, PbA, PbB, PaA, PaB, Qbu, Qbm, Qbd, Qau, Qam, Qad, mode, mutate=None, stats=None):
    """The interpolated rows from the rows the definition names, gathered already (each Hf x w): A, B =
    K[ia], K[ib]; PbA, PbB = Pb[ia], Pb[ib]; the same of Pa; Qb and Qa at mu, m, md."""
    c, e = A, B
    if mode == BOB:
        return (c + e + 1) >> 1
    Hf, w = A.shape
    x = np.arange(w)
    cx = (lambda a: a % w) if mutate == "wrap" else (lambda a: np.clip(a, 0, w - 1))
    d = (Qbm + Qam) >> 1
    t0 = np.abs(Qbm - Qam)
    t1 = (np.abs(PbA - c) + np.abs(PbB - e)) >> 1
    t2 = (np.abs(PaA - c) + np.abs(PaB - e)) >> 1
    diff = np.maximum(t0 >> 1, np.maximum(t1, t2))
    S = lambda j: sum(np.abs(A[:, cx(x + k + j)] - B[:, cx(x + k - j)]) for k in (-1, 0, 1))
    pr = lambda j: (A[:, cx(x + j)] + B[:, cx(x - j)]) >> 1
    sp, score = (c + e) >> 1, S(0) - 1
    direction = np.zeros((Hf, w), np.int32)
    for s in (-1, 1):
        first = S(s) < score
        score = np.where(first, S(s), score)
        sp = np.where(first, pr(s), sp)
        direction = np.where(first, s, direction)
        if mutate != "no2":
            then = first & (S(2 * s) < score)
            score = np.where(then, S(2 * s), score)
            sp = np.where(then, pr(2 * s), sp)
            direction = np.where(then, 2 * s, direction)
    b = (Qbu + Qau) >> 1
    f = (Qbd + Qad) >> 1
    mx = np.maximum(np.maximum(d - e, d - c), np.minimum(b - c, f - e))
    mn = np.minimum(np.minimum(d - e, d - c), np.maximum(b - c, f - e))
    raised = np.maximum(mn, -mx) > diff
    if mutate != "nomnmx":
        diff = np.maximum(diff, np.maximum(mn, -mx))
    out = np.minimum(np.maximum(sp, d - diff), d + diff)
    if stats is not None:
        stats["dir"] = direction
        stats["clamp"] = np.where(sp < d - diff, -1, np.where(sp > d + diff, 1, 0))
        stats["raised"] = raised
    return out


def interp_numpy(K, Pb, Pa, Qb, Qa, q, mode, mutate=None, stats=None):
    """interp_scalar on whole arrays.  mutate: "wrap" (columns wrap instead of clamping), "no2" (the +-2
    step dropped), "nomnmx" (the mn / -mx line dropped).  stats: a dict that receives, per interpolated
    sample, the direction chosen ("dir": 0, -1, -2, 1, 2), the last line's outcome ("clamp": -1 the lower
    bound d - diff, 1 the upper d + diff, 0 neither) and whether the mn / -mx line raised diff ("raised")."""
    K, Pb, Pa, Qb, Qa = (np.asarray(a, np.int32) for a in (K, Pb, Pa, Qb, Qa))
    Hf = K.shape[0]
    m = np.arange(Hf)
    cl = lambda a: np.clip(a, 0, Hf - 1)
    ia, ib, mu, md = cl(m + q - 1), cl(m + q), cl(m - 1), cl(m + 1)
    return interp_rows(K[ia], K[ib], Pb[ia], Pb[ib], Pa[ia], Pa[ib], Qb[mu], Qb, Qb[md], Qa[mu], Qa, Qa[md], mode, mutate, stats)


def interp_frame_rows(C, P, N, keep, second, mode):
    """The mutation "framerows": the sources woven, every row index formed and clamped in rows of the woven
    frame -- row r interpolated from rows r - 1 and r + 1 of cur, r - 2, r, r + 2 of the other parity's
    sources -- so a row that clamps lands on a row of the other parity."""
    q = 1 - keep
    weave = lambda X: np.stack([X[0], X[1]], axis=1).reshape(-1, X[0].shape[1])
    FC, FP, FN = weave(C), weave(P), weave(N)
    h = FC.shape[0]
    r = 2 * np.arange(h // 2) + q
    cr = lambda a: np.clip(a, 0, h - 1)
    up, dn, uu, dd = cr(r - 1), cr(r + 1), cr(r - 2), cr(r + 2)
    FQb, FQa = (FP, FC) if second == 0 else (FC, FN)
    return interp_rows(FC[up], FC[dn], FP[up], FP[dn], FN[up], FN[dn], FQb[uu], FQb[r], FQb[dd], FQa[uu], FQa[r], FQa[dd], mode)


# ------------------------------------------------------------------------------ a plane
def plane(C, P, N, keep, second, mode, impl=interp_numpy, mutate=None, stats=None):
    """One output plane h x w (uint8) from the fields of the sources: C, P, N = (field 0, field 1) each;
    P / N None: prev / next == -1.  mutate: those of interp_numpy, and "second" (second swapped),
    "framerows" (rows clamped in frame rows instead of field rows), "zeros" (a missing source is zeros
    instead of C)."""
    C = tuple(np.asarray(a, np.int32) for a in C)
    missing = (np.zeros_like(C[0]), np.zeros_like(C[1])) if mutate == "zeros" else C
    P = missing if P is None else tuple(np.asarray(a, np.int32) for a in P)
    N = missing if N is None else tuple(np.asarray(a, np.int32) for a in N)
    if mutate == "second":
        second = 1 - second
    q = 1 - keep
    K, Pb, Pa = C[keep], P[keep], N[keep]
    Qb, Qa = (P[q], C[q]) if second == 0 else (C[q], N[q])
    Hf, w = K.shape
    out = np.zeros((2 * Hf, w), np.int32)
    out[keep::2] = K
    if mutate == "framerows":
        out[q::2] = interp_frame_rows(C, P, N, keep, second, mode)
    else:
        kw = {} if impl is interp_scalar else dict(mutate=mutate, stats=stats)
        out[q::2] = impl(K, Pb, Pa, Qb, Qa, q, mode, **kw)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


# ------------------------------------------------------------------------------ sources and frames
def field(kind, planes, p, rect):
    """Field p of a source inside the cropped rectangle rect = (x0, y0, w, h) of one plane: `planes` =
    [the plane of source 0] or [of the top field, of the bottom field]."""
    x0, y0, w, h = rect
    assert y0 % 2 == 0 and h % 2 == 0
    if kind == OUT.OUT_FRAME:
        return planes[0][y0 + p:y0 + h:2, x0:x0 + w]
    if kind == OUT.OUT_FIELD_PAIR:
        return planes[p][y0 // 2:(y0 + h) // 2, x0:x0 + w]
    assert p == (0 if kind == OUT.OUT_UNPAIRED_TOP else 1)
    return planes[0][y0 // 2:(y0 + h) // 2, x0:x0 + w]


def layout(W, H, crop, fmt):
    """rect[k], plane_off[k], plane_pitch[k], coded rows[k] for the planes of a context of chroma format
    fmt, and frame_bytes: three coded-size planes (4:0:0: luma alone)."""
    g = OUT.geometry(W, H, crop, fmt)
    sw, sh = SUB[fmt]
    rects = [g.luma] + ([g.chroma, g.chroma] if fmt else [])
    pitch = [16 * W] + ([16 * W // sw] * 2 if fmt else [])
    rows = [16 * H] + ([16 * H // sh] * 2 if fmt else [])
    off, total = [], 0
    for p, r in zip(pitch, rows):
        off.append(total)
        total += p * r
    return rects, off, pitch, rows, total


def frame(job, table, W, H, crop, fmt, out, impl=interp_numpy, mutate=None):
    """Output frame of one job -- (cur, prev, next, keep, second, mode) -- over the host frame table
    [(kind, srcs)], written into `out` (a uint8 vector the caller prefilled): only the bytes inside the
    cropped rectangles are touched.  Returns frame_bytes."""
    cur, prev, nxt, keep, second, mode = (int(v) for v in job)
    rects, off, pitch, rows, total = layout(W, H, crop, fmt)
    for k, rect in enumerate(rects):
        def both(idx):
            kind, srcs = table[idx]
            planes = [s[k] for s in srcs]
            if kind in (OUT.OUT_UNPAIRED_TOP, OUT.OUT_UNPAIRED_BOT):    # BOB alone: the other field is never read
                f = field(kind, planes, keep, rect)
                return (f, f)
            return (field(kind, planes, 0, rect), field(kind, planes, 1, rect))
        C = both(cur)
        P = both(prev) if prev >= 0 and mode == ADAPTIVE else None
        N = both(nxt) if nxt >= 0 and mode == ADAPTIVE else None
        res = plane(C, P, N, keep, second, mode, impl, mutate)
        x0, y0, w, h = rect
        view = out[off[k]:off[k] + pitch[k] * rows[k]].reshape(rows[k], pitch[k])
        view[y0:y0 + h, x0:x0 + w] = res
    return total


# ------------------------------------------------------------------------------ what the GPU tests run on
TILE_W, TILE_H = OUT.DEINT_TILE_W, OUT.DEINT_TILE_H
# (chroma format, width_mbs, frame_height_mbs, (crop_left, crop_right, crop_top, crop_bottom, frame_mbs_only)):
# cropped luma widths of one below, at and one above TILE_W (odd ones on 4:4:4 and 4:0:0, the nearest even
# ones elsewhere), of more than two tiles, and down to 2; heights of 4 (Hf = 2: every vertical clamp fires; in
# 4:2:0 the chroma has Hf = 1) and, on 4:4:4 and 4:0:0, of 2; heights below, at and above TILE_H.
CASES = [
    (1, 2, 2, (0, 0, 0, 0, 0)),        # 32 x 32: TILE_W
    (1, 3, 4, (1, 6, 0, 0, 0)),        # 34 x 64: above TILE_W, TILE_H
    (1, 2, 4, (0, 1, 0, 2, 1)),        # 30 x 60: below TILE_W, below TILE_H
    (1, 8, 2, (3, 0, 1, 0, 0)),        # 122 x 28 at (6, 4): four tiles, chroma 61
    (1, 5, 2, (0, 7, 0, 0, 0)),        # 66 x 32: two tiles and 2 columns, chroma 33
    (1, 2, 2, (0, 15, 0, 7, 0)),       # 2 x 4: chroma 1 x 2
    (1, 4, 5, (0, 1, 0, 3, 0)),        # 62 x 68: above TILE_H, two tiles high
    (2, 3, 2, (7, 0, 2, 26, 1)),       # 34 x 4 at (14, 2), chroma 17 x 4
    (2, 8, 4, (0, 0, 0, 0, 0)),        # 128 x 64: four tiles, TILE_H
    (3, 2, 2, (0, 1, 0, 15, 0)),       # 31 x 2: below TILE_W, Hf = 1
    (3, 3, 4, (5, 10, 0, 2, 1)),       # 33 x 62 at (5, 0): above TILE_W, below TILE_H
    (3, 5, 2, (1, 14, 1, 0, 0)),       # 65 x 30 at (1, 2): two tiles and 1 column
    (3, 2, 2, (15, 15, 7, 7, 0)),      # 2 x 4 at (15, 14)
    (0, 2, 2, (0, 0, 8, 7, 0)),        # 32 x 2 at (0, 16)
    (0, 8, 4, (0, 1, 0, 0, 1)),        # 127 x 64
    (0, 3, 2, (14, 1, 1, 0, 0)),       # 33 x 30 at (14, 2)
]


def noise_source(kind, W, H, fmt, rng):
    """Host planes of uniform noise for one frame-table row of `kind`: [(y, u, v)], two of them for a field
    pair; a field picture has half the frame's rows."""
    sw, sh = SUB[fmt]
    fld = 0 if kind == OUT.OUT_FRAME else 1
    shapes = [(16 * H >> fld, 16 * W)] + ([(16 * H // sh >> fld, 16 * W // sw)] * 2 if fmt else [])
    return [tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in shapes) for _ in range(2 if kind == OUT.OUT_FIELD_PAIR else 1)]


def other_naming(kind, srcs):
    """The same bytes named the other way: a frame as a pair of its fields, a pair as its woven frame."""
    if kind == OUT.OUT_FRAME:
        return OUT.OUT_FIELD_PAIR, [tuple(np.ascontiguousarray(p[0::2]) for p in srcs[0]), tuple(np.ascontiguousarray(p[1::2]) for p in srcs[0])]
    woven = []
    for t, b in zip(srcs[0], srcs[1]):
        f = np.zeros((2 * t.shape[0], t.shape[1]), np.uint8)
        f[0::2], f[1::2] = t, b
        woven.append(f)
    return OUT.OUT_FRAME, [tuple(woven)]


def case_table(k):
    """The host frame table of case k: a frame, two pairs and a frame of noise, then entries 1 and 0 named
    the other way (4, 5), then an unpaired top and an unpaired bottom field (6, 7)."""
    fmt, W, H, _ = CASES[k]
    rng = np.random.default_rng(7000 + k)
    kinds = [OUT.OUT_FRAME, OUT.OUT_FIELD_PAIR, OUT.OUT_FIELD_PAIR, OUT.OUT_FRAME]
    table = [(kind, noise_source(kind, W, H, fmt, rng)) for kind in kinds]
    table += [other_naming(*table[1]), other_naming(*table[0])]
    table += [(kind, noise_source(kind, W, H, fmt, rng)) for kind in (OUT.OUT_UNPAIRED_TOP, OUT.OUT_UNPAIRED_BOT)]
    return table


def case_jobs():
    """The jobs every case runs: keep x second x mode in the middle of the table, prev and / or next -1,
    prev == cur == next, the other namings of the same bytes, BOB from the unpaired fields."""
    jobs = [(1, 0, 2, keep, second, mode) for keep in (0, 1) for second in (0, 1) for mode in (BOB, ADAPTIVE)]
    jobs += [(2, -1, 3, 0, 0, ADAPTIVE), (2, 1, -1, 1, 1, ADAPTIVE), (0, -1, -1, 1, 0, ADAPTIVE), (3, -1, -1, 0, 1, ADAPTIVE),
             (1, 1, 1, 0, 1, ADAPTIVE), (3, 3, 3, 1, 0, ADAPTIVE)]
    jobs += [(4, 5, 2, 0, 0, ADAPTIVE), (4, 0, 2, 1, 1, ADAPTIVE), (1, 5, 2, 0, 0, ADAPTIVE), (4, -1, -1, 1, 0, BOB)]
    jobs += [(6, -1, -1, 0, 0, BOB), (7, 0, 1, 1, 1, BOB)]
    return jobs
