"""Boxes of scaled RGB on MI355X: h264r_output_rgb_boxes (include/h264r_output.h, the k_output_boxes kernels
of k_output_boxes.hip).

Every comparison is byte-exact against tests/boxes_restate.py, the numpy restatement of the header's
definition on top of tests/scale_restate.py and tests/rgb_restate.py; no expected byte comes from the
library.  Destinations are prefilled with 0xA5 and compared whole, so a byte written outside a box's
pixels (the rest of its image, pitch padding, the gap between images, images no box names, the bytes
around the buffer) fails like a wrong pixel.  Boxes that share an image never overlap here: where they
do, the header leaves the winner open.  Plane contents, sources and crops are those of
tests/test_gpu_output_rgb.py.
"""
import ctypes as C

import numpy as np
import pytest

import boxes_restate as BR
import h264r
import rgb_restate as R
import scale_restate as SR
from h264r import _abi as A
from h264r import output as OUT
from h264r import synth
from test_gpu_output_rgb import (FILL, FORMATS, IMAGENET, KINDS, ROWS, UNIT, _decode, _hcrops, _sources, _split_planar, _upload,
                                 _vcrops)

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 7, 16, 17, 33)
DST_X = (0, 1, 5, 15, 16)
IMAGE_WIDTHS = (64, 49, 63)                                       # 0, 1 and 15 mod 16
FILTERS = (SR.BILINEAR, SR.AREA)
SLOT = 34                                                         # rows of an image a box of the directed jobs has to itself


@pytest.fixture(scope="module")
def L():
    h264r.build()
    return h264r.lib()


@pytest.fixture(scope="module")
def decs(L):
    """One context per chroma format (the output stage takes the format from its context)."""
    d = {fmt: h264r.Decoder(0, 32, 32, chroma_format=fmt) for fmt in (0, 1, 2, 3)}
    yield d
    for x in d.values():
        x.close()


def _rois(lw, lh):
    """The whole frame by the 0 shorthand; an odd origin and an odd size; one sample; a region that touches
    the crop's last row and column (tests/test_gpu_output_scale.py's four)."""
    x, y = min(1, lw - 1), min(1, lh - 1)
    w, h = (lw - x - 1) | 1 if lw - x > 1 else 1, (lh - y - 1) | 1 if lh - y > 1 else 1
    w, h = min(w, lw - x), min(h, lh - y)
    if w % 2 == 0:
        w -= 1
    if h % 2 == 0:
        h -= 1
    tw, th = min(lw, 5), min(lh, 3)
    return [None, (x, y, w, h), (lw // 2, lh // 2, 1, 1), (lw - tw, lh - th, tw, th)]


def _par(par, align):
    return dict(format=par["format"], align=align, alpha=par.get("alpha", 255), scale=par.get("scale", UNIT["scale"]),
                bias=par.get("bias", UNIT["bias"]))


def _job(dec, fmt, out, table, nframes, chans, boxes, iw, ih, nimg, lead, gap, filter, max_out=None, also_skipped=(), order=None,
         **par):
    """Run one job into a 0xA5 buffer (images `gap` bytes apart beyond their size, the first `lead` bytes off
    the allocation) and compare every byte of the buffer with boxes_restate.  chans[f]: the channel planes of
    frame-table entry f, or a function that makes them.  Exactly the boxes h264r_out_box_status refuses, and
    those of also_skipped (a bad frame-table entry), keep their 0xA5, and check() then reports H264R_EDEVICE.
    order: the table order the device sees (a permutation of the boxes; the expectation does not depend on it)."""
    import torch
    align = out.desc.pitch_align
    fb = R.layout(iw, ih, par["format"], align)[2]
    stride = fb + gap
    total = lead + nimg * stride + 64
    d = OUT.boxes_desc(OUT.rgb_desc(out.desc, **par), iw, ih, max_out, filter)
    assert OUT.boxes_geometry(d, fmt).frame_bytes == fb
    tab = BR.table(boxes)
    status = [OUT.box_status(d, tab[i], nframes, nimg, fmt) for i in range(len(boxes))]
    skip = {i for i, s in enumerate(status) if s != A.OK} | set(also_skipped)
    want = np.full(total, FILL, np.uint8)
    BR.images(want[lead:], stride, boxes, chans, iw, ih, filter=filter, skip=skip, **_par(par, align))
    buf = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    dst = buf[lead:lead + nimg * stride].view(nimg, stride)
    view = out.rgb_boxes(table, tab if order is None else tab[list(order)], iw, ih, nimg, n=nframes, max_out=max_out, filter=filter,
                         dst=dst, **par)
    if skip:
        with pytest.raises(h264r.H264RError) as e:
            dec.check()
        assert e.value.status == A.EDEVICE
    else:
        dec.check()
    got = buf.cpu().numpy()
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        at = bad[0] - lead
        pytest.fail(f"fmt {fmt} image {iw}x{ih} x {nimg} filter {filter} align {align} lead {lead} gap {gap} {par} status {status}: "
                    f"{len(bad)} bytes differ, first at byte {at % stride} of image {at // stride} (got {got[bad[0]]}, "
                    f"want {want[bad[0]]}); boxes {boxes}")
    return view, got


def _setup(dec, fmt, W, H, crop, kinds, host, align, **par):
    """Upload the sources; the DeviceOutput, the frame table, the lazily restated channels and the pool."""
    pool, addr = _upload(host)
    out = OUT.DeviceOutput(dec, W, H, crop, pitch_align=align)
    table = out.frames_from([(k,) + tuple(addr[i]) for i, k in enumerate(kinds)])
    rp = dict(matrix=par.get("matrix", R.BT709), full_range=par.get("full_range", 0), up=par.get("chroma_up", R.REPLICATE),
              bgr=par.get("bgr", 0))
    chans = [lambda i=i, k=k: BR.frame_channels(k, host[i], W, H, crop, fmt, **rp) for i, k in enumerate(kinds)]
    return out, table, chans, pool


# ------------------------------------------------------------------------------ 1. directed small shapes
def _mixed_boxes(job, lw, lh, n, nimg, iw):
    """The boxes of one directed job: three slots of SLOT rows per image, all filled but those of the last
    image of five (an image no box names).  The frames are named in a permuted order, several boxes to a
    frame, and frame 1 by none where there is more than one; region, output size and dst_x cycle."""
    rois = _rois(lw, lh)
    frames = [f for f in reversed(range(n)) if n == 1 or f != 1]
    frames = frames[job % len(frames):] + frames[:job % len(frames)]
    boxes, seen = [], set()
    for s in range(3 * (nimg - 1 if nimg == 5 else nimg)):
        k = job + s
        ow, oh = SIZES[(k + k // 7) % 7], SIZES[(2 * k + 3 + job // 7) % 7]
        dx = min(DST_X[(k + k // 5) % 5], iw - ow)
        dy = SLOT * (s % 3) + (k % 2)
        r = (k + k // 4) % 4
        boxes.append(BR.box(frames[s % len(frames)], s // 3, rois[r], (dx, dy), (ow, oh)))
        seen |= {("ow", ow), ("oh", oh), ("dx", dx), ("roi", r)}
    return boxes, seen


@pytest.mark.parametrize("W,H", [(1, 1), (3, 2), (11, 9)])
@pytest.mark.parametrize("fmt", [1, 2, 3, 0], ids=["420", "422", "444", "400"])
def test_directed_small_shapes(decs, fmt, W, H):
    """Every horizontal crop x every format x both chroma_up values x both filters, as
    tests/test_gpu_output_scale.py draws them; each job's boxes mix the regions, the output sizes and the
    placements, and the counts, kinds, matrix rows, bgr, pitch_align, leads and image widths cycle so that each
    of their values meets each filter (and each format where the format matters)."""
    dec = decs[fmt]
    sw, sh = R.SUB[fmt]
    rng = np.random.default_rng(3000 * fmt + 16 * W + H)
    vcrops = _vcrops(H, sh)
    seen = set()
    job = 0
    for (l, r), format, up, filter in [(c, f, u, s) for c in _hcrops(W, sw) for f in FORMATS for u in (R.REPLICATE, R.BILINEAR)
                                       for s in FILTERS]:
        t, b, fmo = vcrops[(job // 4) % len(vcrops)]
        crop = OUT.Crop(l, r, t, b, frame_mbs_only=fmo)
        lw, lh = OUT.geometry(W, H, crop, fmt).luma[2:]
        field_ok = H % 2 == 0                                     # a field picture has half the frame's MB rows
        n = (1, 2, 5)[(job // 2) % 3]
        nimg = (1, 2, 5)[(job // 2 + job // 6) % 3]
        kinds = [KINDS[(job // 2 + 3 * i) % 4] if field_ok else OUT.OUT_FRAME for i in range(n)]
        matrix, fr = ROWS[(job // 6) % 6]
        bgr = (job // 10) % 2
        align = (0, 64)[(job // 14) % 2]
        f16 = format == R.PLANAR_F16
        lead = (0, 2)[(job // 16) % 2] if f16 else (0, 1, 5, 15)[(job // 16) % 4]
        gap = (0, 38, 48)[(job // 4) % 3] if f16 else (0, 37, 48)[(job // 4) % 3]
        iw = IMAGE_WIDTHS[(job // 2 + job // 12) % 3]
        ih = 3 * SLOT + 2
        host = [_sources(k, W, H, fmt, (job // 2 + i) % 3, rng) for i, k in enumerate(kinds)]
        par = dict(format=format, chroma_up=up, matrix=matrix, full_range=fr, bgr=bgr, alpha=(255, 0, 0x5A)[job % 3])
        par.update((UNIT, IMAGENET)[(job // 8) % 2] if f16 else {})
        out, table, chans, pool = _setup(dec, fmt, W, H, crop, kinds, host, align, **par)
        boxes, what = _mixed_boxes(job // 2, lw, lh, n, nimg, iw)
        _job(dec, fmt, out, table, n, chans, boxes, iw, ih, nimg, lead, gap, filter, max_out=(33, 33), **par)
        del pool
        seen |= {("kind", filter, k) for k in kinds} | {("row", matrix, fr), ("bgr", format, bgr), ("align", format, align),
                                                        ("lead", format, lead), ("n", n), ("nimg", filter, nimg), ("iw", filter, iw),
                                                        ("up", filter, up)} | {(k, filter, v) for k, v in what}
        job += 1
    assert {x[1:] for x in seen if x[0] == "row"} == set(ROWS)
    assert {x[1] for x in seen if x[0] == "n"} == {1, 2, 5}
    for format in FORMATS:
        assert {x[2] for x in seen if x[:2] == ("bgr", format)} == {0, 1}
        assert {x[2] for x in seen if x[:2] == ("align", format)} == {0, 64}
        assert {x[2] for x in seen if x[:2] == ("lead", format)} == ({0, 2} if format == R.PLANAR_F16 else {0, 1, 5, 15})
    for filter in FILTERS:
        assert {x[2] for x in seen if x[:2] == ("ow", filter)} == set(SIZES)
        assert {x[2] for x in seen if x[:2] == ("oh", filter)} == set(SIZES)
        assert {x[2] for x in seen if x[:2] == ("dx", filter)} >= set(DST_X)
        assert {x[2] for x in seen if x[:2] == ("roi", filter)} == {0, 1, 2, 3}
        assert {x[2] for x in seen if x[:2] == ("nimg", filter)} == {1, 2, 5}
        assert {x[2] for x in seen if x[:2] == ("iw", filter)} == set(IMAGE_WIDTHS)
        assert {x[2] for x in seen if x[:2] == ("up", filter)} == {R.REPLICATE, R.BILINEAR}
        if H % 2 == 0:
            assert {x[2] for x in seen if x[:2] == ("kind", filter)} == set(KINDS)


@pytest.mark.parametrize("fmt", [1, 2, 3, 0], ids=["420", "422", "444", "400"])
def test_every_kind_in_one_job_and_gbr(decs, fmt):
    """3 x 2 MBs: all four kinds in one frame table, boxes from each of them side by side in one image;
    GBR on 4:4:4."""
    dec = decs[fmt]
    rng = np.random.default_rng(277 + fmt)
    W, H = 3, 2
    crop = OUT.Crop(1, 2 if fmt else 1, 1, 0, frame_mbs_only=0)
    lw, lh = OUT.geometry(W, H, crop, fmt).luma[2:]
    rows = [ROWS[(2 * fmt + 1) % 6]] + ([(R.GBR, 0)] if fmt == 3 else [])
    for j, ((matrix, fr), up, filter) in enumerate((row, up, f) for row in rows for up in (R.REPLICATE, R.BILINEAR) for f in FILTERS):
        kinds = KINDS[j % 4:] + KINDS[:j % 4]
        host = [_sources(k, W, H, fmt, (i + j) % 3, rng) for i, k in enumerate(kinds)]
        par = dict(format=FORMATS[j % 4], chroma_up=up, matrix=matrix, full_range=fr, bgr=j % 2, **IMAGENET)
        out, table, chans, pool = _setup(dec, fmt, W, H, crop, kinds, host, 64, **par)
        boxes = [BR.box(f, 0, (None, (3, 5, 21, 9), (lw - 5, lh - 3, 5, 3), (1, 1, 7, 7))[(f + j) % 4], (17 * (f % 2) + f // 2, 18 * (f // 2)),
                        ((17, 16), (16, 17), (7, 3), (3, 7))[(f + j) % 4]) for f in (2, 0, 3, 1)]
        _job(dec, fmt, out, table, 4, chans, boxes, 35, 36, 1, 0, 16, filter, max_out=(17, 17), **par)
        del pool


# ------------------------------------------------------------------------------ 2. ratios inside one launch
RATIOS = [((0, 0, 16, 7), 16, 7),                                 # 1 : 1
          ((4, 2, 8, 8), 16, 16), ((1, 1, 8, 1), 16, 2),          # 2 x up
          ((5, 3, 7, 3), 16, 7), ((0, 0, 3, 2), 33, 33),          # non-integer up
          ((1, 3, 28, 28), 7, 7), ((0, 0, 32, 32), 16, 16),       # 4 x and 2 x down
          ((1, 1, 17, 31), 7, 3), ((0, 0, 47, 31), 33, 17),       # coprime
          ((0, 0, 48, 32), 3, 2),                                 # 48 -> 3 columns: a window wider than one unit
          (None, 1, 1), ((1, 0, 47, 32), 1, 1), (None, 1, 33), (None, 33, 1)]   # the whole frame to one pixel, row, column


@pytest.mark.parametrize("filter", FILTERS, ids=["bilinear", "area"])
@pytest.mark.parametrize("fmt", [1, 3], ids=["420", "444"])
def test_ratios_that_differ_inside_one_launch(decs, fmt, filter):
    """48 x 32 (3 x 2 MBs): one job whose boxes each have their own ratio -- taps, the divisors and T are
    per box, where k_output_rgb_scaled has them job-wide -- in table order and in reversed table order."""
    dec = decs[fmt]
    rng = np.random.default_rng(131 + fmt)
    W, H = 3, 2
    kinds = [OUT.OUT_FRAME] * 2
    host = [_sources(OUT.OUT_FRAME, W, H, fmt, what, rng) for what in (2, 0)]
    for up in (R.REPLICATE, R.BILINEAR):
        par = dict(format=R.PLANAR_U8, chroma_up=up, matrix=ROWS[up][0], full_range=ROWS[up][1])
        out, table, chans, pool = _setup(dec, fmt, W, H, OUT.Crop(), kinds, host, 0, **par)
        boxes, y = [], 0
        for j, (roi, ow, oh) in enumerate(RATIOS):                # one under the other, two to a row where they fit
            boxes.append(BR.box(j % 2, 0, roi, ((j % 3) * 5, y), (ow, oh)))
            if ow <= 16:
                boxes.append(BR.box(1 - j % 2, 0, roi, (33, y), (ow, oh)))
            y += oh
        iw, ih = 49, y
        _, a = _job(dec, fmt, out, table, 2, chans, boxes, iw, ih, 1, 0, 0, filter, **par)
        _, b = _job(dec, fmt, out, table, 2, chans, boxes, iw, ih, 1, 0, 0, filter, order=reversed(range(len(boxes))), **par)
        assert np.array_equal(a, b)
        del pool


@pytest.mark.parametrize("fmt", [1, 0], ids=["420", "400"])
def test_boxes_smaller_than_the_grids_bound(decs, fmt):
    """Boxes of 3 x 2 under max_out 33 x 17: the grid covers 17 rows of three units per box, of which a box
    fills two units; and one box of the full bound among them."""
    dec = decs[fmt]
    rng = np.random.default_rng(77 + fmt)
    W, H, crop = 3, 2, OUT.Crop(1, 0, 0, 1)
    lw, lh = OUT.geometry(W, H, crop, fmt).luma[2:]
    kinds = [OUT.OUT_FRAME, OUT.OUT_FIELD_PAIR]
    host = [_sources(k, W, H, fmt, 2, rng) for k in kinds]
    for filter, format in ((SR.AREA, R.PACKED_U8), (SR.BILINEAR, R.PLANAR_F16)):
        par = dict(format=format, chroma_up=R.BILINEAR, **IMAGENET)
        out, table, chans, pool = _setup(dec, fmt, W, H, crop, kinds, host, 0, **par)
        small = [BR.box(i % 2, i // 6, (i, i, lw - 2 * i, lh - 2 * i), (1 + 5 * (i % 6), 18 + i % 3), (3, 2)) for i in range(12)]
        for boxes in (small, small[:5] + [BR.box(1, 1, None, (0, 0), (33, 17))] + small[5:]):
            _job(dec, fmt, out, table, 2, chans, boxes, 33, 22, 2, 0, 6, filter, max_out=(33, 17), **par)
        del pool


# ------------------------------------------------------------------------------ 3. device against device
@pytest.mark.parametrize("fmt", [1, 2, 3, 0], ids=["420", "422", "444", "400"])
def test_every_box_is_what_output_rgb_scaled_writes(decs, fmt):
    """Each box of a mixed job against h264r_output_rgb_scaled on a one-entry frame table with the box's
    region and size: device output against device output, in every format under both filters."""
    import torch
    dec = decs[fmt]
    rng = np.random.default_rng(141 + fmt)
    W, H, crop = 3, 2, OUT.Crop(1, 2 if fmt else 1, 1, 0, frame_mbs_only=0)
    lw, lh = OUT.geometry(W, H, crop, fmt).luma[2:]
    host = [_sources(k, W, H, fmt, i % 3, rng) for i, k in enumerate(KINDS)]
    for align in (0, 64):
        out, table, chans, pool = _setup(dec, fmt, W, H, crop, KINDS, host, align)
        for j, (format, filter) in enumerate((f, s) for f in FORMATS for s in FILTERS):
            par = dict(format=format, chroma_up=j % 2, matrix=ROWS[j % 6][0], full_range=ROWS[j % 6][1], bgr=j % 2, alpha=9, **IMAGENET)
            boxes, _ = _mixed_boxes(j, lw, lh, 4, 2, 49)
            view = out.rgb_boxes(table, BR.table(boxes), 49, 3 * SLOT + 2, 2, max_out=(33, 33), filter=filter, **par)
            dec.check()
            packed = format in (R.PACKED_U8, R.PACKED_U8X4)
            for b in boxes:
                roi = (b["roi_x"], b["roi_y"], b["roi_w"], b["roi_h"])
                one = out.rgb_scaled(table.tensor.data_ptr() + 56 * b["frame"], b["out_w"], b["out_h"], 1, roi=roi, filter=filter, **par)
                dec.check()
                ys, xs = slice(b["dst_y"], b["dst_y"] + b["out_h"]), slice(b["dst_x"], b["dst_x"] + b["out_w"])
                part = view[b["image"]][ys, xs] if packed else view[b["image"]][:, ys, xs]
                assert torch.equal(part, one[0]), (format, filter, align, b)
        del pool


# ------------------------------------------------------------------------------ 4. more boxes than a grid axis holds
@pytest.mark.parametrize("filter", FILTERS, ids=["bilinear", "area"])
def test_more_than_65535_boxes(decs, filter):
    """70,000 boxes of one pixel from four regions of a 1 x 1-MB frame, box b to pixel (b / 512, b % 512) of
    one 512 x 137 image: the four values tiled, and 0xA5 behind the last box."""
    import torch
    dec = decs[1]
    rng = np.random.default_rng(65535)
    host = [_sources(OUT.OUT_FRAME, 1, 1, 1, 2, rng)]
    par = dict(format=R.PLANAR_U8, chroma_up=R.BILINEAR)
    out, table, chans, pool = _setup(dec, 1, 1, 1, OUT.Crop(), [OUT.OUT_FRAME], host, 0, **par)
    regions = [(0, 0, 16, 16), (3, 5, 7, 9), (15, 15, 1, 1), (1, 0, 15, 2)]
    c = chans[0]()
    four = np.stack([np.array([p[0, 0] for p in SR.scaled(c, 1, 1, roi, filter)]) for roi in regions])    # [region, channel]
    assert len({tuple(v) for v in four}) == 4
    n, iw, ih = 70000, 512, 137
    tab = np.zeros(n, OUT.OUT_BOX_DTYPE)
    b = np.arange(n)
    for k, name in enumerate(("roi_x", "roi_y", "roi_w", "roi_h")):
        tab[name] = np.array(regions)[b % 4, k]
    tab["dst_x"], tab["dst_y"], tab["out_w"], tab["out_h"] = b % iw, b // iw, 1, 1
    want = np.full((3, ih * iw), FILL, np.uint8)
    want[:, :n] = four[b % 4].T
    dst = torch.full((1, 3 * iw * ih + 32), FILL, dtype=torch.uint8, device="cuda")
    view = out.rgb_boxes(table, tab, iw, ih, 1, max_out=(1, 1), filter=filter, dst=dst, **par)
    dec.check()
    assert tuple(view.shape) == (1, 3, ih, iw)
    got = dst.cpu().numpy()[0]
    assert np.array_equal(got[:3 * iw * ih].reshape(3, ih * iw), want)
    assert np.all(got[3 * iw * ih:] == FILL)
    del pool


# ------------------------------------------------------------------------------ 5. refusals
IW, IH, MW, MH = 40, 30, 17, 16


def _among_good(bad):
    """The bad box third of five: the good ones around it have places of their own."""
    good = [BR.box(0, 0, None, (0, 0), (17, 7)), BR.box(1, 1, (3, 1, 9, 11), (5, 20), (7, 3)), BR.box(1, 0, (0, 0, 1, 1), (39, 29), (1, 1)),
            BR.box(0, 1, (7, 7, 16, 16), (23, 0), (16, 16))]
    return good[:2] + [bad] + good[2:]


BAD_BOXES = [
    ("frame -1", BR.box(-1, 0, None, (20, 10), (7, 3))), ("frame num_frames", BR.box(2, 0, None, (20, 10), (7, 3))),
    ("image -1", BR.box(0, -1, None, (20, 10), (7, 3))), ("image num_images", BR.box(0, 2, None, (20, 10), (7, 3))),
    ("region outside the crop", BR.box(0, 0, (41, 0, 8, 8), (20, 10), (7, 3))),
    ("region one row too many", BR.box(0, 0, (0, 2, 47, 31), (20, 10), (7, 3))),
    ("out_w 0", BR.box(0, 0, None, (20, 10), (0, 3))), ("out_w max_out_w + 1", BR.box(0, 0, None, (20, 10), (MW + 1, 3))),
    ("out_h max_out_h + 1", BR.box(0, 0, None, (20, 10), (7, MH + 1))),
    ("one pixel past the right edge", BR.box(0, 0, None, (IW - 6, 10), (7, 3))),
    ("one pixel past the bottom edge", BR.box(0, 0, None, (20, IH - 2), (7, 3))),
    ("pad", BR.box(0, 0, None, (20, 10), (7, 3), pad=(0, 1))),
]


@pytest.mark.parametrize("format,filter", [(R.PACKED_U8, SR.AREA), (R.PLANAR_F16, SR.BILINEAR)], ids=["packed-area", "f16-bilinear"])
def test_refused_boxes_are_skipped_and_reported(decs, format, filter):
    """Each bad box among good ones: exactly the boxes h264r_out_box_status refuses keep their 0xA5, the others
    are written, check() reports H264R_EDEVICE, and a job of good boxes after it leaves the error word clean."""
    dec = decs[1]
    rng = np.random.default_rng(164)
    W, H, crop = 3, 2, OUT.Crop()                                 # 48 x 32
    kinds = [OUT.OUT_FRAME, OUT.OUT_FIELD_PAIR]
    host = [_sources(k, W, H, 1, 2 - i, rng) for i, k in enumerate(kinds)]
    par = dict(format=format, chroma_up=R.BILINEAR, **IMAGENET)
    out, table, chans, pool = _setup(dec, 1, W, H, crop, kinds, host, 0, **par)
    d = OUT.boxes_desc(OUT.rgb_desc(out.desc, **par), IW, IH, (MW, MH), filter)
    for why, bad in BAD_BOXES:
        boxes = _among_good(bad)
        st = [OUT.box_status(d, BR.table([b])[0], 2, 2, 1) for b in boxes]
        assert st == [A.OK, A.OK, A.EINVAL, A.OK, A.OK], (why, st)
        _job(dec, 1, out, table, 2, chans, boxes, IW, IH, 2, 1 if format != R.PLANAR_F16 else 2, 10, filter, max_out=(MW, MH), **par)
        _job(dec, 1, out, table, 2, chans, _among_good(BR.box(1, 1, None, (5, 10), (7, 3))), IW, IH, 2, 0, 0, filter, max_out=(MW, MH),
             **par)                                               # the report cleared the error word
    del pool


def test_refused_frame_entries_are_skipped_and_reported(decs):
    """A box whose frame-table entry has a kind outside 0..3 or a NULL plane the kind needs is skipped like a
    refused box.  The bad entries hold NULL or valid pointers only, tested before any is used."""
    import torch
    dec = decs[1]
    rng = np.random.default_rng(264)
    W, H, crop = 3, 2, OUT.Crop(1, 0, 0, 1)
    out = OUT.DeviceOutput(dec, W, H, crop)
    hfrm = _sources(OUT.OUT_FRAME, W, H, 1, 2, rng)
    hfld = _sources(OUT.OUT_FIELD_PAIR, W, H, 1, 1, rng)
    frm = tuple(torch.from_numpy(a).cuda() for a in hfrm[0])
    fld = [tuple(torch.from_numpy(a).cuda() for a in s) for s in hfld]
    good = [lambda: BR.frame_channels(OUT.OUT_FRAME, hfrm, W, H, crop, 1), lambda: BR.frame_channels(OUT.OUT_FIELD_PAIR, hfld, W, H, crop, 1)]
    bad_entries = [(9, frm), (-1, frm), (OUT.OUT_FRAME, (frm[0], None, frm[2])), (OUT.OUT_FRAME, (None, frm[1], frm[2])),
                   (OUT.OUT_FIELD_PAIR, fld[0], (None, fld[1][1], fld[1][2])), (OUT.OUT_FIELD_PAIR, fld[0], (fld[1][0], fld[1][1], None)),
                   (OUT.OUT_UNPAIRED_BOT, (None, fld[0][1], fld[0][2]))]
    for j, entry in enumerate(bad_entries):
        table = out.frames_from([(OUT.OUT_FRAME, frm), entry, (OUT.OUT_FIELD_PAIR, fld[0], fld[1])])
        chans = [good[0], None, good[1]]
        boxes = [BR.box(0, 0, None, (0, 0), (17, 7)), BR.box(1, 0, None, (20, 10), (7, 3)), BR.box(2, 1, (3, 1, 9, 11), (5, 20), (7, 3)),
                 BR.box(1, 1, (0, 0, 1, 1), (0, 0), (1, 1)), BR.box(2, 0, (7, 7, 16, 16), (23, 14), (16, 16))]
        filter, format = FILTERS[j % 2], FORMATS[j % 4]
        _job(dec, 1, out, table, 3, chans, boxes, IW, IH, 2, 0, 16, filter, max_out=(MW, MH), also_skipped=(1, 3), format=format)
        _job(dec, 1, out, table, 3, chans, [boxes[0], boxes[2], boxes[4]], IW, IH, 2, 0, 16, filter, max_out=(MW, MH), format=format)


def test_area_bound_on_a_400_context(decs):
    """182 x 182 MBs cropped to 2897 x 2897 on a 4:0:0 context (tests/test_gpu_output_scale.py builds 181 x 181):
    the whole frame to one pixel has T = 2897^2 > 2^23 and is refused on the device under AREA -- and written
    under BILINEAR; the region of 2896 x 2896 beside it (T = 8,386,816) is written under both."""
    import torch
    dec = decs[0]
    n = 182
    crop = OUT.Crop(right=15, bottom=15)
    y = torch.full((16 * n, 16 * n), 255, dtype=torch.uint8, device="cuda")
    y[8 * n:] = 0
    out = OUT.DeviceOutput(dec, n, n, crop)
    assert OUT.geometry(n, n, crop, 0).luma[2:] == (2897, 2897)
    table = out.frames_from([(OUT.OUT_FRAME, (y, None, None))])
    host_y = np.full((2897, 2897), 255, np.uint8)
    host_y[8 * n:] = 0
    chans = [(host_y,) * 3]                                       # full range, 4:0:0: R = G = B = Y
    boxes = [BR.box(0, 0, (1, 1, 2896, 2896), (0, 0), (1, 1)), BR.box(0, 0, None, (2, 0), (1, 1)), BR.box(0, 0, (0, 0, 2896, 1456), (4, 0), (2, 1))]
    par = dict(format=R.PLANAR_U8, full_range=True, matrix=R.BT709)
    d = OUT.boxes_desc(OUT.rgb_desc(out.desc, **par), 6, 1, (2, 1), SR.AREA)
    assert [OUT.box_status(d, BR.table([b])[0], 1, 1, 0) for b in boxes] == [A.OK, A.EUNSUPPORTED, A.OK]
    _, got = _job(dec, 0, out, table, 1, chans, boxes, 6, 1, 1, 0, 0, SR.AREA, max_out=(2, 1), **par)
    assert got[:6].tolist() == [128, FILL, FILL, FILL, 255, 255]  # rows 1..2896: 1455 of 255, 1441 of 0 -> 128.2 ...
    _job(dec, 0, out, table, 1, chans, boxes, 6, 1, 1, 0, 0, SR.BILINEAR, max_out=(2, 1), **par)


# ------------------------------------------------------------------------------ 6. decoded input
def _boxes_equal_restated_yuv(dec, table, W, H, crop, fmt):
    """h264r_output_frames planar on the table; boxes_restate on those bytes == h264r_output_rgb_boxes: a
    letterbox of every frame (letterbox_boxes) and, in further images, crops of them."""
    yuv = OUT.DeviceOutput(dec, W, H, crop, fake_chroma=fmt == 0).run(table)
    dec.check()
    yuv = yuv.cpu().numpy()
    lw, lh = OUT.geometry(W, H, crop, fmt).luma[2:]
    n = table.n
    iw, ih = 63, 64
    letter = OUT.letterbox_boxes(n, lw, lh, iw, ih)
    assert letter["out_w"][0] == iw and letter["out_h"][0] < ih and letter["dst_y"][0] > 0
    boxes = [dict(zip(BR.FIELDS, (int(b[k]) for k in BR.FIELDS))) for b in letter]
    boxes += [BR.box(n - 1 - i, n + i % 2, (lw - 41 - i, lh - 33, 41, 33), (16 * (i % 3) + i, 22 * (i // 3)), (16, 17)) for i in range(min(n, 6))]
    jobs = [(format, up, filter) for format in FORMATS for up in (R.REPLICATE, R.BILINEAR) for filter in FILTERS]
    for j, (format, up, filter) in enumerate(jobs):
        par = dict(matrix=ROWS[j % 6][0], full_range=ROWS[j % 6][1], bgr=j % 2, chroma_up=up, format=format, **IMAGENET)
        out = OUT.DeviceOutput(dec, W, H, crop, pitch_align=(0, 64)[j % 2])
        chans = [lambda k=k: R.channels(*_split_planar(yuv[k], W, H, crop, fmt), fmt, par["matrix"], par["full_range"], up, par["bgr"])
                 for k in range(n)]
        _job(dec, fmt, out, table, n, chans, boxes, iw, ih, n + 2, 0, 0, filter, **par)


@pytest.mark.parametrize("fmt", [1, 2, 3, 0], ids=["420", "422", "444", "400"])
def test_frame_batch_from_decoder(L, decs, fmt):
    """A decoded frame batch: the boxes job reads the batch's own out planes on the same stream."""
    dec = decs[fmt]
    over = {} if fmt == 1 else dict(chroma_format={2: 2, 3: 3, 0: A.SYNTH_CHROMA_400}[fmt])
    db = _decode(L, dec, [synth.default_cfg(L, 3, 11, 9, **over)], 3)
    crop = OUT.Crop(1, 2, 1, 3)
    t = db.tensors
    out = OUT.DeviceOutput(dec, 11, 9, crop)
    table = out.frames_from([(OUT.OUT_FRAME, (t["out_y"][i], t["out_u"][i] if fmt else None, t["out_v"][i] if fmt else None))
                             for i in (2, 0, 1)])
    _boxes_equal_restated_yuv(dec, table, 11, 9, crop, fmt)


def test_field_batches_woven_pairwise(L, decs):
    """Top fields and bottom fields (11 x 4 MBs each) woven pairwise into 11 x 8 frames, and two unpaired."""
    dec = decs[1]
    top = synth.default_cfg(L, 3, 11, 4, structure=1, seed=0x51)
    bot = synth.default_cfg(L, 3, 11, 4, structure=2, seed=0x52)
    n = 3
    db = _decode(L, dec, [top, bot], n)
    crop = OUT.Crop(2, 1, 1, 1, frame_mbs_only=0)
    t = db.tensors
    pic = lambda i: (t["out_y"][i], t["out_u"][i], t["out_v"][i])
    spec = [(OUT.OUT_FIELD_PAIR, i, n + i) for i in (1, 2, 0)] + [(OUT.OUT_UNPAIRED_TOP, 0), (OUT.OUT_UNPAIRED_BOT, n)]
    table = OUT.DeviceOutput(dec, 11, 8, crop).frames_from([(s[0],) + tuple(pic(i) for i in s[1:]) for s in spec])
    _boxes_equal_restated_yuv(dec, table, 11, 8, crop, 1)


# ------------------------------------------------------------------------------ 7. the torch wrapper
@pytest.mark.parametrize("align", [0, 64])
@pytest.mark.parametrize("fmt", [1, 0], ids=["420", "400"])
def test_wrapper_views(decs, fmt, align):
    import torch
    dec = decs[fmt]
    W, H, crop, n = 3, 2, OUT.Crop(3, 4 if fmt else 3, 1, 0), 2
    rng = np.random.default_rng(153)
    host = [_sources(OUT.OUT_FRAME, W, H, fmt, 2, rng) for _ in range(n)]
    out, table, chans, pool = _setup(dec, fmt, W, H, crop, [OUT.OUT_FRAME] * n, host, align, bgr=True)
    iw, ih, nimg = 21, 13, 3
    boxes = [BR.box(1, 0, (1, 3, 30, 21), (2, 1), (17, 7)), BR.box(0, 2, None, (16, 9), (5, 4))]
    for format in FORMATS:
        t = out.rgb_boxes(table, boxes, iw, ih, nimg, filter=SR.AREA, format=format, bgr=True, alpha=7)
        dec.check()
        pitch = R.pitch_of(iw, format, align)
        fb = R.layout(iw, ih, format, align)[2]
        if format in (R.PACKED_U8, R.PACKED_U8X4):
            ch = 3 if format == R.PACKED_U8 else 4
            assert t.dtype == torch.uint8 and tuple(t.shape) == (nimg, ih, iw, ch) and t.stride() == (fb, pitch, ch, 1)
        elif format == R.PLANAR_U8:
            assert t.dtype == torch.uint8 and tuple(t.shape) == (nimg, 3, ih, iw) and t.stride() == (fb, pitch * ih, pitch, 1)
        else:
            assert t.dtype == torch.float16 and tuple(t.shape) == (nimg, 3, ih, iw)
            assert t.stride() == (fb // 2, pitch * ih // 2, pitch // 2, 1)
        assert t.is_contiguous() == (align == 0)
        # dst=None: new images, zero outside the boxes -- padding included
        base = t.untyped_storage()
        raw = torch.empty(0, dtype=torch.uint8, device="cuda").set_(base)[:nimg * fb].cpu().numpy()
        want = np.zeros(nimg * fb, np.uint8)
        BR.images(want, fb, boxes, chans, iw, ih, filter=SR.AREA, format=format, align=align, alpha=7)
        assert np.array_equal(raw, want), format
        assert not raw[fb:2 * fb].any()
    # the defaults: AREA, planar u8, max_out the image's size; rows of ten numbers are boxes too
    t = out.rgb_boxes(table, [(0, 0, 0, 0, 0, 0, 0, 0, iw, ih)], iw, ih, 1, bgr=True)
    dec.check()
    assert np.array_equal(t[0].cpu().numpy(), np.stack(SR.scaled(chans[0](), iw, ih)))
    # a device table, and a raw address with its count
    dev = torch.from_numpy(BR.table(boxes).view(np.uint8).reshape(-1).copy()).cuda()
    a = out.rgb_boxes(table, dev, iw, ih, nimg, bgr=True)
    b = out.rgb_boxes(table.tensor.data_ptr(), dev.data_ptr(), iw, ih, nimg, n=n, num_boxes=2, bgr=True)
    c = out.rgb_boxes(table, boxes, iw, ih, nimg, bgr=True)
    dec.check()
    assert torch.equal(a, b) and torch.equal(a, c) and a.any()
    # no boxes: nothing is written
    dst = torch.full((nimg, fb + 5), FILL, dtype=torch.uint8, device="cuda")
    out.rgb_boxes(table, [], iw, ih, nimg, dst=dst)
    out.rgb_boxes(table, dev, iw, ih, nimg, num_boxes=0, dst=dst)
    dec.check()
    assert bool((dst == FILL).all())
    with pytest.raises(ValueError):
        out.rgb_boxes(table.tensor.data_ptr(), boxes, iw, ih, nimg)
    with pytest.raises(ValueError):
        out.rgb_boxes(table, dev.data_ptr(), iw, ih, nimg)
    with pytest.raises(ValueError):
        out.rgb_boxes(table, boxes, iw, ih, nimg, dst=torch.zeros(4, dtype=torch.uint8, device="cuda"))
    del pool


def test_host_refusals_on_a_context(decs):
    import torch
    dec = decs[1]
    out = OUT.DeviceOutput(dec, 3, 2)
    y = torch.zeros(32 * 48, dtype=torch.uint8, device="cuda")
    table = out.frames_from([(OUT.OUT_FRAME, (y, y, y))])
    dev = torch.from_numpy(BR.table([BR.box(0, 1, None, (3, 1), (17, 7))]).view(np.uint8).reshape(-1).copy()).cuda()
    call = lambda desc, tab, n, bx, nb, d, stride, ni: dec._L.h264r_output_rgb_boxes(
        dec.handle, C.byref(desc) if desc is not None else None, tab, n, bx, nb, d, stride, ni, None)
    tp, bp = table.tensor.data_ptr(), dev.data_ptr()
    for format in FORMATS:
        desc = OUT.boxes_desc(OUT.rgb_desc(out.desc, format=format), 21, 9, (17, 7))
        fb = OUT.boxes_geometry(desc, 1).frame_bytes
        dst = torch.zeros(2 * fb + 16, dtype=torch.uint8, device="cuda")
        dp = dst.data_ptr()
        assert call(desc, tp, 1, bp, 1, dp, fb - 1, 2) == A.EINVAL       # images would overlap
        assert call(desc, None, 1, bp, 1, dp, fb, 2) == A.EINVAL and call(desc, tp, 1, None, 1, dp, fb, 2) == A.EINVAL
        assert call(desc, tp, 1, bp, 1, None, fb, 2) == A.EINVAL and call(None, tp, 1, bp, 1, dp, fb, 2) == A.EINVAL
        assert call(desc, tp, -1, bp, 1, dp, fb, 2) == A.EINVAL and call(desc, tp, 1, bp, -1, dp, fb, 2) == A.EINVAL
        assert call(desc, tp, 1, bp, 1, dp, fb, -1) == A.EINVAL
        assert call(desc, tp, 1, bp, 0, dp, fb, 2) == A.OK                # nothing to do
        odd = A.EINVAL if format == R.PLANAR_F16 else A.OK               # binary16 wants even addresses
        assert call(desc, tp, 1, bp, 1, dp + 1, fb, 2) == odd and call(desc, tp, 1, bp, 1, dp, fb + 1, 2) == odd
        assert call(desc, tp, 1, bp, 1, dp, fb, 2) == A.OK
    assert call(OUT.boxes_desc(OUT.rgb_desc(out.desc), 21, 9, (22, 7)), tp, 1, bp, 1, dp, fb, 2) == A.EINVAL
    assert call(OUT.boxes_desc(OUT.rgb_desc(out.desc), 21, 9, (17, 7), filter=2), tp, 1, bp, 1, dp, fb, 2) == A.EINVAL
    assert call(OUT.boxes_desc(OUT.rgb_desc(out.desc, matrix=R.GBR), 21, 9, (17, 7)), tp, 1, bp, 1, dp, fb, 2) == A.EUNSUPPORTED
    dec.check()
