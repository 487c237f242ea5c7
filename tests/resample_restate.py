"""The resampled RGB frames of include/h264r_output.h, restated in Python from the header's text alone:
Pillow's 8-bit resampler (Resample.c) -- binary64 coefficients rounded to 22-bit integers, a horizontal
and a vertical integer pass with a clip to 8 bits after each.

Python's float is binary64 and every expression below is one operation per operator, in the header's
order; math.sin is the C library's sin.  The source is what tests/rgb_restate.py:channels returns; the bytes
leave through rgb_restate.write_frame, at the output size.  Nothing here comes from the library but the
values of its enums.
"""
import math

import numpy as np

import rgb_restate as R
import scale_restate as SR
from h264r import output as OUT

TRIANGLE, BICUBIC, LANCZOS = OUT.RESAMPLE_TRIANGLE, OUT.RESAMPLE_BICUBIC, OUT.RESAMPLE_LANCZOS
FILTERS = (TRIANGLE, BICUBIC, LANCZOS)
SUPPORT = {TRIANGLE: 1.0, BICUBIC: 2.0, LANCZOS: 3.0}
MAX_TAPS = 97
PIL_NAMES = {TRIANGLE: "BILINEAR", BICUBIC: "BICUBIC", LANCZOS: "LANCZOS"}


def _triangle(x):
    if x < 0.0:
        x = -x
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * 3.14159265358979323846
    return math.sin(x) / x


def _lanczos(x):
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


KERNEL = {TRIANGLE: _triangle, BICUBIC: _bicubic, LANCZOS: _lanczos}


def ksize_of(filter, in0, in1, out_size):
    scale = (in1 - in0) / out_size
    filterscale = max(scale, 1.0)
    return 2 * math.ceil(SUPPORT[filter] * filterscale) + 1


def axis(filter, in_size, in0, in1, out_size):
    """xmin [out_size], count [out_size], kk [out_size][ksize] (int64, zero behind count), ksize."""
    f = KERNEL[filter]
    scale = (in1 - in0) / out_size
    filterscale = max(scale, 1.0)
    support = SUPPORT[filter] * filterscale
    ss = 1.0 / filterscale
    ksize = 2 * math.ceil(support) + 1
    xmin, count = np.zeros(out_size, np.int64), np.zeros(out_size, np.int64)
    kk = np.zeros((out_size, ksize), np.int64)
    for d in range(out_size):
        center = in0 + (d + 0.5) * scale
        lo = max(0, int(center - support + 0.5))
        hi = min(in_size, int(center + support + 0.5))
        k = [f((j + lo - center + 0.5) * ss) for j in range(hi - lo)]
        ww = 0.0
        for w in k:
            ww += w
        if ww != 0.0:
            k = [w / ww for w in k]
        for j, w in enumerate(k):
            kk[d, j] = int(w * 4194304.0 + 0.5) if w >= 0 else int(w * 4194304.0 - 0.5)
        xmin[d], count[d] = lo, hi - lo
    return xmin, count, kk, ksize


def _pass(c, table, clip=True):
    """One pass along the LAST axis of c (int64): out[..., d] = (2^21 + sum_j kk[d][j] * c[..., xmin[d] + j]) >> 22."""
    xmin, count, kk, _ = table
    out = np.zeros(c.shape[:-1] + (len(xmin),), np.int64)
    for d in range(len(xmin)):
        n = int(count[d])
        out[..., d] = ((1 << 21) + c[..., xmin[d]:xmin[d] + n] @ kk[d, :n]) >> 22
    return np.clip(out, 0, 255) if clip else out


def resample(c, roi, out_w, out_h, filter, clip_between=True, clamp_to_region=False):
    """One channel plane (uint8, lh x lw: the whole cropped rectangle) to out_h x out_w; roi = (x, y, w, h).
    clip_between=False leaves out the clip after the horizontal pass, clamp_to_region=True is
    crop(box).resize(): two things the definition is NOT, for the tests that tell them apart."""
    lh, lw = c.shape
    x, y, w, h = roi
    if clamp_to_region:
        c, lw, lh, x, y = c[y:y + h, x:x + w], w, h, 0, 0
    t = _pass(c.astype(np.int64), axis(filter, lw, x, x + w, out_w), clip_between)
    v = _pass(t.T, axis(filter, lh, y, y + h, out_h)).T
    return np.ascontiguousarray(v.astype(np.uint8))


def resampled(c, out_w, out_h, roi=None, filter=BICUBIC, **kw):
    """The three channel planes of rgb_restate.channels, resampled."""
    lh, lw = c[0].shape
    r = SR.region(lw, lh, roi)
    return tuple(resample(p, r, out_w, out_h, filter, **kw) for p in c)


def frame(kind, srcs, W, H, crop, fmt, out, out_w, out_h, *, roi=None, filter=BICUBIC, matrix=R.BT709, full_range=False,
          up=R.REPLICATE, format=R.PLANAR_U8, bgr=False, alpha=255, scale=(1 / 255,) * 3, bias=(0,) * 3, align=0):
    """One resampled frame from its source pictures (host planes), written into `out`; returns frame_bytes."""
    Y, Cb, Cr = R.source_frame(R.weave(kind, srcs), W, H, crop, fmt)
    c = R.channels(Y, Cb, Cr, fmt, matrix, full_range, up, bgr)
    return R.write_frame(out, resampled(c, out_w, out_h, roi, filter), format, align, alpha, scale, bias)


# ------------------------------------------------------------------------------ the cases recorded from Pillow
def edges(h, w, rng):
    """Noise with 0 / 255 step edges: vertical and horizontal bars over the left and the top part."""
    c = rng.integers(0, 256, (h, w), dtype=np.uint8)
    bars = ((np.arange(w) // 3) % 2 * 255).astype(np.uint8)
    c[:max(1, h // 2), :] = bars[None, :]
    c[:, :max(1, w // 3)] = (((np.arange(h) // 2) % 2) * 255).astype(np.uint8)[:, None]
    return c


def blocks(h, w):
    """3 x 3 blocks of 0 and 255, a checkerboard: edges in both directions everywhere.  Under BICUBIC the
    horizontal pass overshoots at every vertical edge, and the vertical pass then weighs those values: the
    input on which the clip between the passes shows (MUTATION: its size and its output size)."""
    y, x = np.mgrid[0:h, 0:w]
    return (((x // 3 + y // 3) % 2) * 255).astype(np.uint8)


MUTATION = dict(w=48, h=32, out_w=40, out_h=27, filter=BICUBIC)


# (in_w, in_h, out_w, out_h, box or None): downscale, upscale, identity, to and from one sample, regions inside
SHAPES = [(37, 23, 7, 5, None), (37, 23, 50, 40, None), (37, 23, 37, 23, None), (16, 16, 1, 1, None), (1, 1, 5, 3, None),
          (37, 23, 7, 5, (3, 2, 30, 17)), (37, 23, 50, 40, (5, 4, 21, 13)), (37, 23, 11, 9, (10, 6, 11, 9)),
          (64, 48, 9, 7, (1, 1, 62, 46)), (200, 120, 12, 7, None)]
CASES = [(f, s) for f in FILTERS for s in SHAPES]


def case_input(k):
    """The input plane of case k: numpy.random.default_rng(k)."""
    _, (w, h, _, _, _) = CASES[k]
    return edges(h, w, np.random.default_rng(k))


def case_restated(k):
    f, (w, h, ow, oh, box) = CASES[k]
    return resample(case_input(k), box or (0, 0, w, h), ow, oh, f)


def case_pillow(k):
    """The same case through PIL.Image.resize (mode L)."""
    from PIL import Image
    f, (w, h, ow, oh, box) = CASES[k]
    kw = {} if box is None else dict(box=(box[0], box[1], box[0] + box[2], box[1] + box[3]))
    im = Image.fromarray(case_input(k)).resize((ow, oh), getattr(Image.Resampling, PIL_NAMES[f]), **kw)
    return np.asarray(im)
