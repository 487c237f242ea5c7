"""The boxes of include/h264r_output.h (h264r_output_rgb_boxes), restated in numpy from the header's text
alone, on top of tests/scale_restate.py and tests/rgb_restate.py.

For each box in table order: the three channel planes of its frame (rgb_restate.channels), its region
resampled to its output size (scale_restate.scaled), and its pixels placed at (dst_y, dst_x) of its image
by the byte rules of rgb_restate.write_frame -- into a buffer the caller prefilled, of which only the
boxes' pixels are touched.  The refusal rule is restated too (status).  Nothing here comes from the
library but the values of its enums and the record layout of the box table.
"""
from math import gcd

import numpy as np

import rgb_restate as R
import scale_restate as SR
from h264r import _abi as A
from h264r import output as OUT

FIELDS = ("frame", "image", "roi_x", "roi_y", "roi_w", "roi_h", "dst_x", "dst_y", "out_w", "out_h")


def box(frame=0, image=0, roi=None, dst=(0, 0), out=(1, 1), pad=(0, 0)):
    """One box as a dict of the header's fields."""
    x, y, w, h = (0, 0, 0, 0) if roi is None else roi
    return dict(frame=frame, image=image, roi_x=x, roi_y=y, roi_w=w, roi_h=h, dst_x=dst[0], dst_y=dst[1], out_w=out[0],
                out_h=out[1], pad=tuple(pad))


def table(boxes):
    """The host box table (OUT.OUT_BOX_DTYPE) of a list of box() dicts."""
    tab = np.zeros(len(boxes), OUT.OUT_BOX_DTYPE)
    for i, b in enumerate(boxes):
        for k in FIELDS:
            tab[i][k] = b[k]
        tab[i]["pad"] = b.get("pad", (0, 0))
    return tab


def status(b, lw, lh, image_w, image_h, max_out_w, max_out_h, filter, num_frames, num_images):
    """The header's rule for one box, in its order: A.OK, A.EINVAL or A.EUNSUPPORTED."""
    if not 0 <= b["frame"] < num_frames or not 0 <= b["image"] < num_images:
        return A.EINVAL
    x, y, w, h = b["roi_x"], b["roi_y"], b["roi_w"], b["roi_h"]
    if min(x, y, w, h) < 0 or (w == 0) != (h == 0):
        return A.EINVAL
    if w == 0:
        w, h = lw, lh
    if x + w > lw or y + h > lh:
        return A.EINVAL
    if not 1 <= b["out_w"] <= max_out_w or not 1 <= b["out_h"] <= max_out_h:
        return A.EINVAL
    if b["dst_x"] < 0 or b["dst_y"] < 0 or b["dst_x"] + b["out_w"] > image_w or b["dst_y"] + b["out_h"] > image_h:
        return A.EINVAL
    if any(b.get("pad", (0, 0))):
        return A.EINVAL
    if filter == SR.AREA and (w // gcd(w, b["out_w"])) * (h // gcd(h, b["out_h"])) > SR.AREA_MAX_T:
        return A.EUNSUPPORTED
    return A.OK


def place(out, c, dst_x, dst_y, image_w, image_h, format, align, alpha=255, scale=(1 / 255,) * 3, bias=(0,) * 3):
    """rgb_restate.write_frame's byte rules for the channels c (three uint8 arrays out_h x out_w) at pixel
    (dst_y, dst_x) of the image that starts at out[0]: only the pixels' bytes are touched."""
    oh, ow = c[0].shape
    assert 0 <= dst_x and dst_x + ow <= image_w and 0 <= dst_y and dst_y + oh <= image_h
    off, pitches, total = R.layout(image_w, image_h, format, align)
    pitch = pitches[0]
    bpp = R.BYTES_PER_PIXEL[format]
    if format in (R.PACKED_U8, R.PACKED_U8X4):
        px = list(c) + ([np.full((oh, ow), alpha, np.uint8)] if format == R.PACKED_U8X4 else [])
        rows = np.stack(px, axis=2).reshape(oh, -1)
        out[:total].reshape(image_h, pitch)[dst_y:dst_y + oh, bpp * dst_x:bpp * (dst_x + ow)] = rows
        return total
    for k in range(3):
        if format == R.PLANAR_U8:
            rows = c[k]
        else:
            rows = R.half_bits(c[k], scale[k], bias[k]).astype("<u2").view(np.uint8).reshape(oh, 2 * ow)
        out[off[k]:off[k] + pitch * image_h].reshape(image_h, pitch)[dst_y:dst_y + oh, bpp * dst_x:bpp * (dst_x + ow)] = rows
    return total


def images(out, stride, boxes, chans, image_w, image_h, *, filter=SR.AREA, format=R.PLANAR_U8, align=0, alpha=255,
           scale=(1 / 255,) * 3, bias=(0,) * 3, skip=()):
    """Every box of `boxes` (box() dicts, table order; those whose index is in `skip` left out) into the
    images at out[k * stride:]: chans[f] = the channel planes (c0, c1, c2) of frame-table entry f, or a
    function that returns them.  Returns frame_bytes of one image."""
    cache = {}
    for i, b in enumerate(boxes):
        if i in skip:
            continue
        f = b["frame"]
        if f not in cache:
            cache[f] = chans[f]() if callable(chans[f]) else chans[f]
        roi = (b["roi_x"], b["roi_y"], b["roi_w"], b["roi_h"])
        c = SR.scaled(cache[f], b["out_w"], b["out_h"], roi, filter)
        place(out[b["image"] * stride:], c, b["dst_x"], b["dst_y"], image_w, image_h, format, align, alpha, scale, bias)
    return R.layout(image_w, image_h, format, align)[2]


def frame_channels(kind, srcs, W, H, crop, fmt, matrix=R.BT709, full_range=False, up=R.REPLICATE, bgr=False):
    """The channel planes of one frame-table entry from its host planes, as scale_restate.frame makes them."""
    Y, Cb, Cr = R.source_frame(R.weave(kind, srcs), W, H, crop, fmt)
    return R.channels(Y, Cb, Cr, fmt, matrix, full_range, up, bgr)
