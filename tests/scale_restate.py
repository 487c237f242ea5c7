"""The scaled RGB frames of include/h264r_output.h, restated in numpy from the header's text alone.

The source is what tests/rgb_restate.py:channels returns -- the three 8-bit channel planes of the
full-size RGB frame; the region of interest, the two filters and the rounding follow the header's
comment line by line; the bytes leave through rgb_restate.write_frame, at the output size.  Nothing
here comes from the library but the values of its enums.
"""
import numpy as np

import rgb_restate as R
from h264r import output as OUT

BILINEAR, AREA = OUT.SCALE_BILINEAR, OUT.SCALE_AREA
MAX_OUT = 16384
AREA_MAX_T = 2 ** 23


def bilinear_axis(S, D):
    """i0, i1, w0, w1 for every output index d: half-sample centres, 8-bit weights."""
    d = np.arange(D, dtype=np.int64)
    p = np.clip((2 * d + 1) * S - D, 0, 2 * D * (S - 1))
    i0 = p // (2 * D)
    f = p - 2 * D * i0
    w1 = (256 * f + D) // (2 * D)
    return i0, np.minimum(i0 + 1, S - 1), 256 - w1, w1


def area_axis(S, D):
    """o[d][i]: the coverage of source sample i by output d, in units of 1 / D of a sample."""
    d = np.arange(D, dtype=np.int64)[:, None]
    i = np.arange(S, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((d + 1) * S, (i + 1) * D) - np.maximum(d * S, i * D))


def bilinear_sums(c, out_h, out_w):
    """The sum in front of the + 32768 of the header's formula, int64 out_h x out_w."""
    c = c.astype(np.int64)
    r0, r1, wv0, wv1 = bilinear_axis(c.shape[0], out_h)
    x0, x1, wh0, wh1 = bilinear_axis(c.shape[1], out_w)
    top = wh0[None, :] * c[r0][:, x0] + wh1[None, :] * c[r0][:, x1]
    bot = wh0[None, :] * c[r1][:, x0] + wh1[None, :] * c[r1][:, x1]
    return wv0[:, None] * top + wv1[:, None] * bot


def area_sums(c, out_h, out_w):
    """A of the header's formula in the unreduced unit, int64 out_h x out_w; T = S_h * S_w."""
    return area_axis(c.shape[0], out_h) @ c.astype(np.int64) @ area_axis(c.shape[1], out_w).T


def resample(c, out_h, out_w, filter):
    """One channel plane (uint8, S_h x S_w) to out_h x out_w."""
    if filter == BILINEAR:
        return np.ascontiguousarray(((bilinear_sums(c, out_h, out_w) + 32768) >> 16).astype(np.uint8))
    assert filter == AREA
    T = c.shape[0] * c.shape[1]
    return np.ascontiguousarray(((2 * area_sums(c, out_h, out_w) + T) // (2 * T)).astype(np.uint8))


def region(lw, lh, roi):
    """x, y, S_w, S_h of an roi argument (None or w == h == 0: the whole rectangle)."""
    x, y, w, h = (0, 0, 0, 0) if roi is None else roi
    if w == 0 and h == 0:
        w, h = lw, lh
    assert x >= 0 and y >= 0 and w > 0 and h > 0 and x + w <= lw and y + h <= lh
    return x, y, w, h


def scaled(c, out_w, out_h, roi=None, filter=AREA):
    """The three channel planes of rgb_restate.channels, scaled."""
    lh, lw = c[0].shape
    x, y, w, h = region(lw, lh, roi)
    return tuple(resample(p[y:y + h, x:x + w], out_h, out_w, filter) for p in c)


def area_supported(S_w, S_h, out_w, out_h):
    rw, rh = S_w // np.gcd(S_w, out_w), S_h // np.gcd(S_h, out_h)
    return int(rw) * int(rh) <= AREA_MAX_T


def frame(kind, srcs, W, H, crop, fmt, out, out_w, out_h, *, roi=None, filter=AREA, matrix=R.BT709, full_range=False,
          up=R.REPLICATE, format=R.PLANAR_U8, bgr=False, alpha=255, scale=(1 / 255,) * 3, bias=(0,) * 3, align=0):
    """One scaled frame from its source pictures (host planes), written into `out`; returns frame_bytes."""
    Y, Cb, Cr = R.source_frame(R.weave(kind, srcs), W, H, crop, fmt)
    c = R.channels(Y, Cb, Cr, fmt, matrix, full_range, up, bgr)
    return R.write_frame(out, scaled(c, out_w, out_h, roi, filter), format, align, alpha, scale, bias)
