"""The RGB frames of include/h264r_output.h, restated in numpy from the header's text alone.

Nothing here comes from the library but the values of its enums.  The source frame -- crop, weave,
the 128 rows of an unpaired field -- is the planar frame h264r/output.py:frame_bytes writes (the
reference's bytes, pinned by tests/test_output.py) over planes woven by the rule of
tests/streams.py:output_frames; the chroma interpolation, the integer matrix, the channel order, the
four formats and the row pitch follow the header's comment line by line.
"""
from fractions import Fraction

import numpy as np

from h264r import output as OUT

BT601, BT709, BT2020, GBR = OUT.CSC_BT601, OUT.CSC_BT709, OUT.CSC_BT2020, OUT.CSC_GBR
REPLICATE, BILINEAR = OUT.UP_REPLICATE, OUT.UP_BILINEAR
PACKED_U8, PACKED_U8X4, PLANAR_U8, PLANAR_F16 = OUT.RGB_PACKED_U8, OUT.RGB_PACKED_U8X4, OUT.RGB_PLANAR_U8, OUT.RGB_PLANAR_F16

K = {BT601: (Fraction(299, 1000), Fraction(114, 1000)), BT709: (Fraction(2126, 10000), Fraction(722, 10000)),
     BT2020: (Fraction(2627, 10000), Fraction(593, 10000))}
SUB = {0: (1, 1), 1: (2, 2), 2: (2, 1), 3: (1, 1)}             # SubWidthC, SubHeightC
BYTES_PER_PIXEL = {PACKED_U8: 3, PACKED_U8X4: 4, PLANAR_U8: 1, PLANAR_F16: 2}


def reals(matrix, full_range):
    """The five real coefficients and yo, as exact fractions."""
    kr, kb = K[matrix]
    kg = 1 - kr - kb
    ys, cs, yo = (255, 255, 0) if full_range else (219, 224, 16)
    return (Fraction(255, ys), 255 * 2 * (1 - kr) / cs, -255 * 2 * kb * (1 - kb) / (kg * cs),
            -255 * 2 * kr * (1 - kr) / (kg * cs), 255 * 2 * (1 - kb) / cs), yo


def coefficients(matrix, full_range):
    """cy, crv, cgu, cgv, cbu, yo: floor(real * 2^14 + 1/2)."""
    r, yo = reals(matrix, full_range)
    return tuple((x * 2 ** 14 + Fraction(1, 2)).__floor__() for x in r) + (yo,)


def matrix_int(Y, cb8, cr8, coef):
    """R, G, B (int32 arrays) of Y (0..255) and Cb8, Cr8 (units of 1 / 8) by the header's formula."""
    cy, crv, cgu, cgv, cbu, yo = coef
    Y, cb, cr = Y.astype(np.int32), cb8.astype(np.int32) - 1024, cr8.astype(np.int32) - 1024
    yt = 8 * cy * (Y - yo) + 65536
    clip = lambda v: np.clip(v >> 17, 0, 255)
    return clip(yt + crv * cr), clip(yt + cgu * cb + cgv * cr), clip(yt + cbu * cb)


def matrix_real(Y, cb8, cr8, matrix, full_range):
    """clip255(floor(x + 1/2)) of the same expression in float64."""
    (cy, crv, cgu, cgv, cbu), yo = reals(matrix, full_range)
    cy, crv, cgu, cgv, cbu = (float(x) for x in (cy, crv, cgu, cgv, cbu))
    Y, cb, cr = Y.astype(np.float64) - yo, cb8.astype(np.float64) / 8 - 128, cr8.astype(np.float64) / 8 - 128
    fin = lambda v: np.clip(np.floor(v + 0.5), 0, 255).astype(np.int32)
    return fin(cy * Y + crv * cr), fin(cy * Y + cgu * cb + cgv * cr), fin(cy * Y + cbu * cb)


def chroma8(c, lw, lh, sub_w, sub_h, up):
    """C8 at every luma sample of the lh x lw rectangle, from the cropped chroma plane c (ch x cw)."""
    c = c.astype(np.int32)
    ch, cw = c.shape
    assert lw == sub_w * cw and lh == sub_h * ch
    r, x = np.arange(lh), np.arange(lw)
    if up == REPLICATE:
        return 8 * c[(r // sub_h)[:, None], (x // sub_w)[None, :]]
    if sub_w == 2:
        even = x % 2 == 0
        i0 = np.where(even, x // 2, (x - 1) // 2)
        i1 = np.where(even, i0, np.minimum(i0 + 1, cw - 1))
        h = c[:, i0] + c[:, i1]                                   # wh 2, or 1 and 1
    else:
        h = 2 * c[:, x]
    if sub_h == 2:
        even = r % 2 == 0
        j0 = np.where(even, r // 2, (r - 1) // 2)
        j1 = np.where(even, np.maximum(j0 - 1, 0), np.minimum(j0 + 1, ch - 1))
        return 3 * h[j0] + h[j1]
    return 4 * h[r]


def weave(kind, srcs):
    """The coded-size frame planes of one output frame (tests/streams.py:output_frames' rule; the rows
    of an unpaired field's missing parity are 128)."""
    if kind == OUT.OUT_FRAME:
        return tuple(srcs[0])
    planes = []
    for k, a in enumerate(srcs[0]):
        f = np.full((2 * a.shape[0], a.shape[1]), 128, np.uint8)
        if kind == OUT.OUT_FIELD_PAIR:
            f[0::2], f[1::2] = a, srcs[1][k]
        else:
            f[(0 if kind == OUT.OUT_UNPAIRED_TOP else 1)::2] = a
        planes.append(f)
    return tuple(planes)


def source_frame(planes, W, H, crop, fmt):
    """Y, Cb, Cr of the header's source frame (Cb = Cr = None on 4:0:0), cut out of the bytes
    h264r/output.py:frame_bytes writes for the coded-size (woven) planes."""
    geom = OUT.geometry(W, H, crop, fmt)
    y, u, v = (tuple(planes) + (None, None))[:3]
    x0, y0, lw, lh = geom.luma
    if fmt == 0:                                 # luma alone (frame_bytes appends the reference's fake chroma)
        return np.asarray(y)[y0:y0 + lh, x0:x0 + lw], None, None
    data = np.frombuffer(OUT.frame_bytes(y, u, v, geom), np.uint8)
    Y = data[:lw * lh].reshape(lh, lw)
    cw, ch = geom.chroma[2:]
    n = cw * ch
    return Y, data[lw * lh:lw * lh + n].reshape(ch, cw), data[lw * lh + n:lw * lh + 2 * n].reshape(ch, cw)


def channels(Y, Cb, Cr, fmt, matrix=BT709, full_range=False, up=REPLICATE, bgr=False):
    """(c0, c1, c2) as uint8 arrays lh x lw."""
    lh, lw = Y.shape
    if matrix == GBR:
        assert fmt == 3
        R, G, B = Cr, Y, Cb
    else:
        sw, sh = SUB[fmt]
        if fmt == 0:
            cb8 = cr8 = np.full((lh, lw), 1024, np.int32)
        else:
            cb8, cr8 = chroma8(Cb, lw, lh, sw, sh, up), chroma8(Cr, lw, lh, sw, sh, up)
        R, G, B = matrix_int(Y, cb8, cr8, coefficients(matrix, full_range))
    c = (B, G, R) if bgr else (R, G, B)
    return tuple(np.asarray(p).astype(np.uint8) for p in c)


def pitch_of(lw, format, align):
    row = BYTES_PER_PIXEL[format] * lw
    return row if align <= 1 else -(-row // align) * align


def layout(lw, lh, format, align):
    """plane_off, plane_pitch, frame_bytes."""
    pitch = pitch_of(lw, format, align)
    if format in (PACKED_U8, PACKED_U8X4):
        return (0, 0, 0), (pitch, 0, 0), pitch * lh
    return (0, pitch * lh, 2 * pitch * lh), (pitch,) * 3, 3 * pitch * lh


def half_bits(c, scale, bias):
    """binary16 bits of float(v) * scale + bias: a float32 product, a float32 sum, one conversion."""
    f = c.astype(np.float32) * np.float32(scale) + np.float32(bias)
    return f.astype(np.float16).view(np.uint16)


def write_frame(out, c, format, align, alpha=255, scale=(1 / 255,) * 3, bias=(0,) * 3):
    """Write the frame of channels c into `out` (a uint8 vector the caller prefilled): only the frame's
    bytes are touched.  Returns frame_bytes."""
    lh, lw = c[0].shape
    off, pitches, total = layout(lw, lh, format, align)
    pitch = pitches[0]
    if format in (PACKED_U8, PACKED_U8X4):
        px = list(c) + ([np.full((lh, lw), alpha, np.uint8)] if format == PACKED_U8X4 else [])
        rows = np.stack(px, axis=2).reshape(lh, -1)
        out[:total].reshape(lh, pitch)[:, :rows.shape[1]] = rows
        return total
    for k in range(3):
        if format == PLANAR_U8:
            rows = c[k]
        else:
            rows = half_bits(c[k], scale[k], bias[k]).astype("<u2").view(np.uint8).reshape(lh, 2 * lw)
        out[off[k]:off[k] + pitch * lh].reshape(lh, pitch)[:, :rows.shape[1]] = rows
    return total


def frame(kind, srcs, W, H, crop, fmt, out, *, matrix=BT709, full_range=False, up=REPLICATE, format=PLANAR_U8,
          bgr=False, alpha=255, scale=(1 / 255,) * 3, bias=(0,) * 3, align=0):
    """One RGB frame from its source pictures (host planes), written into `out`; returns frame_bytes."""
    Y, Cb, Cr = source_frame(weave(kind, srcs), W, H, crop, fmt)
    c = channels(Y, Cb, Cr, fmt, matrix, full_range, up, bgr)
    return write_frame(out, c, format, align, alpha, scale, bias)
