"""The host half of h264r_output_rgb_boxes (include/h264r_output.h): the exports, the layout of
h264r_out_box and h264r_boxes_desc, h264r_output_rgb_boxes_geometry, every host refusal, the refusal rule
of a box (h264r_out_box_status against its restatement, tests/boxes_restate.py), letterbox_boxes, and the
restatement itself against tests/scale_restate.py.  No GPU is needed.
"""
import ctypes as C
import itertools
import os
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

import boxes_restate as BR
import h264r
import rgb_restate as R
import scale_restate as SR
from h264r import _abi as A
from h264r import output as OUT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = (R.PACKED_U8, R.PACKED_U8X4, R.PLANAR_U8, R.PLANAR_F16)
FILTERS = (SR.BILINEAR, SR.AREA)


def _src(W=11, H=9, crop=OUT.Crop(), align=0):
    return OUT._desc(W, H, crop, OUT.PLANAR, align, False)


def _desc(image_w=40, image_h=30, max_out=None, filter=SR.AREA, src=None, **rgb):
    return OUT.boxes_desc(OUT.rgb_desc(src or _src(), **rgb), image_w, image_h, max_out, filter)


def _status(desc, fmt=1):
    return h264r.lib().h264r_output_rgb_boxes_geometry(fmt, C.byref(desc), C.byref(OUT.RgbGeom()))


# ------------------------------------------------------------------------------ the ABI
def test_library_exports_the_three_functions():
    L = h264r.lib()
    for name in ("h264r_output_rgb_boxes_geometry", "h264r_out_box_status", "h264r_output_rgb_boxes"):
        assert hasattr(L, name), name
    assert L.h264r_abi_version() == 5 == A.ABI_VERSION


def test_struct_layouts_match_c():
    box = ["frame", "image", "roi_x", "roi_y", "roi_w", "roi_h", "dst_x", "dst_y", "out_w", "out_h", "pad"]
    desc = ["rgb", "image_w", "image_h", "max_out_w", "max_out_h", "filter", "pad"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "h264r_output.h"\nint main(void) {\n'
           '  printf("%zu %zu %zu %d\\n", sizeof(h264r_out_box), sizeof(h264r_boxes_desc), sizeof(h264r_rgb_desc), H264R_ABI_VERSION);\n'
           + "".join(f'  printf("%zu\\n", offsetof(h264r_out_box, {n}));\n' for n in box)
           + "".join(f'  printf("%zu\\n", offsetof(h264r_boxes_desc, {n}));\n' for n in desc) + "  return 0; }\n")
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "l.c")
        with open(c, "w") as f:
            f.write(src)
        exe = os.path.join(td, "l")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        v = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert v[:4] == [C.sizeof(OUT.OutBox), C.sizeof(OUT.BoxesDesc), C.sizeof(OUT.RgbDesc), 5]
    assert v[4:4 + len(box)] == [getattr(OUT.OutBox, n).offset for n in box]
    assert v[4 + len(box):] == [getattr(OUT.BoxesDesc, n).offset for n in desc]
    assert C.sizeof(OUT.OutBox) == 48 == OUT.OUT_BOX_DTYPE.itemsize
    assert C.sizeof(OUT.BoxesDesc) == C.sizeof(OUT.RgbDesc) + 24
    assert [OUT.OUT_BOX_DTYPE.fields[n][1] for n in box] == [getattr(OUT.OutBox, n).offset for n in box]


# ------------------------------------------------------------------------------ geometry
GRID = [(11, 9, (0, 0, 0, 0)), (11, 9, (1, 2, 3, 2)), (120, 68, (0, 0, 0, 4)), (1, 1, (1, 2, 1, 1))]
IMAGES = ((1, 1), (7, 3), (224, 224), (33, 17), (640, 640), (16384, 1))


@pytest.mark.parametrize("fmt", (0, 1, 2, 3))
@pytest.mark.parametrize("format", FORMATS)
def test_geometry_is_the_rgb_layout_at_the_image_size(fmt, format):
    n = 0
    for (W, H, (l, r, t, b)), align, (iw, ih) in itertools.product(GRID, (0, 64, 256), IMAGES):
        for max_out, filter in ((None, SR.AREA), ((1, 1), SR.BILINEAR), ((iw, 1), SR.AREA)):
            d = _desc(iw, ih, max_out, filter, src=_src(W, H, OUT.Crop(l, r, t, b), align), format=format)
            g = OUT.boxes_geometry(d, fmt)
            off, pitch, total = R.layout(iw, ih, format, align)
            assert (g.width, g.height) == (iw, ih)
            assert (g.plane_off, g.plane_pitch, g.frame_bytes) == (off, pitch, total), (W, H, align, iw, ih)
            # and it is h264r_output_rgb_scaled_geometry's layout for an output of that size
            s = OUT.scaled_geometry(OUT.scale_desc(d.rgb, iw, ih, None, SR.BILINEAR), fmt)
            assert s == g
            n += 1
    assert n == len(GRID) * 3 * len(IMAGES) * 3


# ------------------------------------------------------------------------------ host refusals
def test_geometry_refuses_what_the_rgb_geometry_refuses():
    assert _status(_desc()) == A.OK
    for side in ("left", "right", "top", "bottom"):
        assert _status(_desc(src=_src(crop=OUT.Crop(**{side: -1})))) == A.EINVAL, side
    assert _status(_desc(src=_src(crop=OUT.Crop(left=44, right=44)))) == A.EINVAL
    for bad in (-1, 3, 48, 8192):
        assert _status(_desc(src=_src(align=bad))) == A.EINVAL, bad
    assert _status(_desc(src=_src(W=0))) == A.EINVAL and _status(_desc(src=_src(H=1025))) == A.EINVAL
    assert _status(_desc(), 4) == A.EINVAL and _status(_desc(), -1) == A.EINVAL
    assert _status(_desc(src=OUT._desc(11, 9, OUT.Crop(), OUT.SEMIPLANAR, 0, False))) == A.EINVAL
    assert _status(_desc(src=OUT._desc(11, 9, OUT.Crop(), OUT.PLANAR, 0, True)), 0) == A.EINVAL
    for name, bad in (("matrix", (-1, 4)), ("chroma_up", (-1, 2)), ("format", (-1, 4)), ("alpha", (-1, 256))):
        for v in bad:
            assert _status(_desc(**{name: v})) == A.EINVAL, (name, v)
    for name in ("full_range", "bgr"):
        for v in (-1, 2):
            d = _desc()
            setattr(d.rgb, name, v)
            assert _status(d) == A.EINVAL, (name, v)
    for name in ("scale", "bias"):
        for v in (float("nan"), float("inf")):
            assert _status(_desc(**{name: (1.0, v, 1.0)})) == A.EINVAL, (name, v)
    L = h264r.lib()
    assert L.h264r_output_rgb_boxes_geometry(1, None, C.byref(OUT.RgbGeom())) == A.EINVAL
    assert L.h264r_output_rgb_boxes_geometry(1, C.byref(_desc()), None) == A.EINVAL


def test_geometry_refuses_a_bad_image_bound_filter_or_pad():
    for iw, ih in ((1, 1), (16384, 16384), (16384, 1), (1, 16384)):
        assert _status(_desc(iw, ih, filter=SR.BILINEAR)) == A.OK, (iw, ih)
    for iw, ih in ((0, 5), (5, 0), (-1, 5), (5, -1), (16385, 5), (5, 16385)):
        assert _status(_desc(iw, ih, max_out=(1, 1))) == A.EINVAL, (iw, ih)
    for mo in ((40, 30), (1, 1), (40, 1), (1, 30)):
        assert _status(_desc(max_out=mo)) == A.OK, mo
    for mo in ((0, 5), (5, 0), (-1, 5), (5, -1), (41, 30), (40, 31), (2 ** 31 - 1, 1)):
        assert _status(_desc(max_out=mo)) == A.EINVAL, mo
    for f in (-1, 2, 7):
        assert _status(_desc(filter=f)) == A.EINVAL, f
    d = _desc()
    d.pad = 1
    assert _status(d) == A.EINVAL
    # GBR off 4:4:4 is unsupported, and an argument error comes first
    for fmt in (0, 1, 2):
        assert _status(_desc(matrix=R.GBR), fmt) == A.EUNSUPPORTED
        assert _status(_desc(matrix=R.GBR, max_out=(41, 30)), fmt) == A.EINVAL
    assert _status(_desc(matrix=R.GBR), 3) == A.OK


def test_the_call_refuses_null_arguments_and_negative_counts_without_a_context():
    L = h264r.lib()
    d = _desc()
    one = C.c_void_p(16)                                          # never dereferenced: the context is NULL
    assert L.h264r_output_rgb_boxes(None, C.byref(d), one, 1, one, 1, one, 1 << 20, 1, None) == A.EINVAL
    box = OUT.OutBox(0, 0, 0, 0, 0, 0, 0, 0, 1, 1)
    S = L.h264r_out_box_status
    assert S(1, C.byref(d), C.byref(box), 1, 1) == A.OK
    assert S(1, None, C.byref(box), 1, 1) == A.EINVAL and S(1, C.byref(d), None, 1, 1) == A.EINVAL
    assert S(1, C.byref(d), C.byref(box), -1, 1) == A.EINVAL and S(1, C.byref(d), C.byref(box), 1, -1) == A.EINVAL
    assert S(4, C.byref(d), C.byref(box), 1, 1) == A.EINVAL
    bad = _desc()
    bad.pad = 3
    assert S(1, C.byref(bad), C.byref(box), 1, 1) == A.EINVAL


# ------------------------------------------------------------------------------ the rule of a box
LW, LH = 170, 134                                                 # 11 x 9 MBs, 4:2:0, crop (1, 2, 3, 2)
CROP = OUT.Crop(1, 2, 3, 2)
IW, IH, MW, MH = 40, 30, 33, 17
GOOD = [
    BR.box(), BR.box(0, 0, None, (0, 0), (MW, MH)), BR.box(2, 4, (0, 0, LW, LH), (IW - MW, IH - MH), (MW, MH)),
    BR.box(1, 1, (LW - 1, LH - 1, 1, 1), (IW - 1, IH - 1), (1, 1)), BR.box(0, 3, (5, 3, 9, 11), (1, 5), (7, 3)),
    BR.box(2, 0, (1, 1, LW - 1, LH - 1), (15, 16), (16, 1)),
]
BAD = [                                                           # each refusal reason alone
    ("frame below", BR.box(-1), A.EINVAL), ("frame past", BR.box(3), A.EINVAL), ("frame far", BR.box(2 ** 31 - 1), A.EINVAL),
    ("image below", BR.box(0, -1), A.EINVAL), ("image past", BR.box(0, 5), A.EINVAL), ("image far", BR.box(0, -2 ** 31), A.EINVAL),
    ("roi_x < 0", BR.box(roi=(-1, 0, 4, 4)), A.EINVAL), ("roi_y < 0", BR.box(roi=(0, -1, 4, 4)), A.EINVAL),
    ("roi_w < 0", BR.box(roi=(0, 0, -4, 4)), A.EINVAL), ("roi_h < 0", BR.box(roi=(0, 0, 4, -4)), A.EINVAL),
    ("roi_w alone 0", BR.box(roi=(0, 0, 0, 4)), A.EINVAL), ("roi_h alone 0", BR.box(roi=(0, 0, 4, 0)), A.EINVAL),
    ("all from x 1", BR.box(roi=(1, 0, 0, 0)), A.EINVAL), ("all from y 1", BR.box(roi=(0, 1, 0, 0)), A.EINVAL),
    ("past the right", BR.box(roi=(1, 0, LW, LH)), A.EINVAL), ("past the bottom", BR.box(roi=(0, 1, LW, LH)), A.EINVAL),
    ("wider than the crop", BR.box(roi=(0, 0, LW + 1, LH)), A.EINVAL), ("origin on the edge", BR.box(roi=(LW, 0, 1, 1)), A.EINVAL),
    ("a sum that wraps", BR.box(roi=(2 ** 31 - 1, 0, 2, 2)), A.EINVAL), ("a size that wraps", BR.box(roi=(1, 1, 2 ** 31 - 1, 2 ** 31 - 1)), A.EINVAL),
    ("out_w 0", BR.box(out=(0, 1)), A.EINVAL), ("out_h 0", BR.box(out=(1, 0)), A.EINVAL), ("out_w < 0", BR.box(out=(-1, 1)), A.EINVAL),
    ("out_w past max", BR.box(out=(MW + 1, 1)), A.EINVAL), ("out_h past max", BR.box(out=(1, MH + 1)), A.EINVAL),
    ("dst_x < 0", BR.box(dst=(-1, 0)), A.EINVAL), ("dst_y < 0", BR.box(dst=(0, -1)), A.EINVAL),
    ("one past the right", BR.box(dst=(IW - 6, 0), out=(7, 3)), A.EINVAL), ("one past the bottom", BR.box(dst=(0, IH - 2), out=(7, 3)), A.EINVAL),
    ("dst that wraps", BR.box(dst=(2 ** 31 - 1, 0), out=(7, 3)), A.EINVAL),
    ("pad[0]", BR.box(pad=(1, 0)), A.EINVAL), ("pad[1]", BR.box(pad=(0, -1)), A.EINVAL),
]


@pytest.mark.parametrize("filter", FILTERS)
def test_box_status_is_the_rule(filter):
    d = _desc(IW, IH, (MW, MH), filter, src=_src(crop=CROP))
    assert OUT.geometry(11, 9, CROP, 1).luma[2:] == (LW, LH)
    rule = lambda b, nf=3, ni=5: BR.status(b, LW, LH, IW, IH, MW, MH, filter, nf, ni)
    for b in GOOD:
        assert OUT.box_status(d, BR.table([b])[0], 3, 5) == A.OK == rule(b), b
    for why, b, want in BAD:
        assert OUT.box_status(d, BR.table([b])[0], 3, 5) == want == rule(b), why
    # the counts are the job's: the same box under other counts
    b = BR.box(2, 4)
    assert OUT.box_status(d, BR.table([b])[0], 2, 5) == A.EINVAL == rule(b, 2, 5)
    assert OUT.box_status(d, BR.table([b])[0], 3, 4) == A.EINVAL == rule(b, 3, 4)
    assert OUT.box_status(d, BR.table([BR.box()])[0], 0, 1) == A.EINVAL and OUT.box_status(d, BR.table([BR.box()])[0], 1, 0) == A.EINVAL
    # an OutBox is taken as it is
    assert OUT.box_status(d, OUT.OutBox(2, 4, 5, 3, 9, 11, 1, 5, 7, 3), 3, 5) == A.OK


def test_box_status_area_bound_and_einval_ahead_of_eunsupported():
    """rw * rh > 2^23 on a 4:0:0 descriptor of 182 x 182 MBs cropped to 2897 x 2897 (test_output_scale.py's)."""
    crop = OUT.Crop(right=15, bottom=15)
    src = _src(182, 182, crop)
    st = lambda b, filter=SR.AREA, nf=1, ni=1: OUT.box_status(_desc(8, 8, None, filter, src=src), BR.table([b])[0], nf, ni, 0)
    whole, part = BR.box(), BR.box(roi=(1, 1, 2896, 2896))
    assert st(whole) == A.EUNSUPPORTED == BR.status(whole, 2897, 2897, 8, 8, 8, 8, SR.AREA, 1, 1)
    assert st(whole, SR.BILINEAR) == A.OK and st(part) == A.OK             # AREA's bound alone; the region counts
    assert st(BR.box(out=(1, 8))) == A.EUNSUPPORTED and st(BR.box(out=(8, 1))) == A.EUNSUPPORTED
    assert st(BR.box(roi=(0, 0, 2897, 2896), out=(1, 8))) == A.OK          # rh = 362
    # every other reason comes first
    for b in (BR.box(1), BR.box(0, 1), BR.box(out=(9, 1)), BR.box(dst=(8, 0)), BR.box(pad=(0, 1)), BR.box(roi=(1, 0, 0, 0))):
        assert st(b) == A.EINVAL == BR.status(b, 2897, 2897, 8, 8, 8, 8, SR.AREA, 1, 1), b
    # the descriptor's EUNSUPPORTED (GBR off 4:4:4) yields to a box's argument error, and stands otherwise
    gbr = _desc(IW, IH, (MW, MH), SR.AREA, matrix=R.GBR)
    assert OUT.box_status(gbr, BR.table([BR.box()])[0], 1, 1, 1) == A.EUNSUPPORTED
    assert OUT.box_status(gbr, BR.table([BR.box(1)])[0], 1, 1, 1) == A.EINVAL
    assert OUT.box_status(gbr, BR.table([BR.box()])[0], 1, 1, 3) == A.OK


# ------------------------------------------------------------------------------ letterbox_boxes
@pytest.mark.parametrize("lw,lh,iw,ih", [(1920, 1080, 640, 640), (1080, 1920, 640, 640), (170, 134, 640, 360), (176, 144, 33, 17),
                                         (500, 500, 224, 224), (1, 1, 7, 3), (16384, 1, 5, 5), (1, 16384, 5, 5), (48, 32, 1, 1),
                                         (1920, 1080, 640, 360), (3, 2, 1, 16), (1919, 1080, 641, 360)])
def test_letterbox_boxes_against_fractions(lw, lh, iw, ih):
    tab = OUT.letterbox_boxes(3, lw, lh, iw, ih)
    assert tab.dtype == OUT.OUT_BOX_DTYPE and len(tab) == 3
    ratio = min(Fraction(iw, lw), Fraction(ih, lh))               # aspect kept: one ratio for both axes
    if Fraction(iw, lw) >= Fraction(ih, lh):                      # the height fills the image
        want_h, want_w = ih, max(1, (lw * ratio + Fraction(1, 2)).__floor__())
    else:
        want_w, want_h = iw, max(1, (lh * ratio + Fraction(1, 2)).__floor__())
    for i, b in enumerate(tab):
        assert (b["frame"], b["image"]) == (i, i) and (b["roi_x"], b["roi_y"], b["roi_w"], b["roi_h"]) == (0, 0, 0, 0)
        assert (b["out_w"], b["out_h"]) == (want_w, want_h) and tuple(b["pad"]) == (0, 0)
        assert (b["dst_x"], b["dst_y"]) == ((iw - want_w) // 2, (ih - want_h) // 2)
        assert 1 <= b["out_w"] <= iw and 1 <= b["out_h"] <= ih
        # centred: the borders differ by one pixel at the most
        assert 0 <= (iw - want_w - b["dst_x"]) - b["dst_x"] <= 1 and 0 <= (ih - want_h - b["dst_y"]) - b["dst_y"] <= 1
    if lw <= 1024 * 16 and lh <= 1024 * 16 and lw % 16 == 0 and lh % 16 == 0:
        d = _desc(iw, ih, None, SR.BILINEAR, src=_src(lw // 16, lh // 16))
        assert all(OUT.box_status(d, b, 3, 3) == A.OK for b in tab)


def test_letterbox_named_cases():
    b = OUT.letterbox_boxes(1, 1920, 1080, 640, 640)[0]
    assert (b["out_w"], b["out_h"], b["dst_x"], b["dst_y"]) == (640, 360, 0, 140)
    b = OUT.letterbox_boxes(1, 1080, 1920, 640, 640)[0]
    assert (b["out_w"], b["out_h"], b["dst_x"], b["dst_y"]) == (360, 640, 140, 0)
    b = OUT.letterbox_boxes(1, 16384, 1, 5, 5)[0]
    assert (b["out_w"], b["out_h"], b["dst_x"], b["dst_y"]) == (5, 1, 0, 2)
    assert len(OUT.letterbox_boxes(0, 4, 4, 4, 4)) == 0
    with pytest.raises(ValueError):
        OUT.letterbox_boxes(1, 0, 4, 4, 4)


def test_boxes_table_takes_rows_mappings_and_arrays():
    tab = OUT.boxes_table([(1, 2, 3, 4, 5, 6, 7, 8, 9, 10), BR.box(1, 2, (3, 4, 5, 6), (7, 8), (9, 10))])
    assert tab[0] == tab[1] and tab[0]["out_h"] == 10 and tuple(tab[0]["pad"]) == (0, 0)
    assert np.array_equal(OUT.boxes_table(tab), tab)
    assert np.array_equal(BR.table([BR.box(1, 2, (3, 4, 5, 6), (7, 8), (9, 10))]), tab[:1])
    with pytest.raises(ValueError):
        OUT.boxes_table([(1, 2, 3)])


# ------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("format", FORMATS)
@pytest.mark.parametrize("filter", FILTERS)
def test_a_box_at_the_origin_of_an_image_of_its_size_is_the_scaled_frame(format, filter):
    rng = np.random.default_rng(4 + format)
    W, H, crop, fmt = 3, 2, OUT.Crop(1, 2, 1, 0), 1
    planes = [(rng.integers(0, 256, (32, 48), dtype=np.uint8), rng.integers(0, 256, (16, 24), dtype=np.uint8),
               rng.integers(0, 256, (16, 24), dtype=np.uint8))]
    par = dict(matrix=R.BT601, full_range=1, up=R.BILINEAR, bgr=True)
    c = BR.frame_channels(OUT.OUT_FRAME, planes, W, H, crop, fmt, **par)
    for align, (ow, oh), roi in ((0, (7, 3), (5, 3, 9, 11)), (64, (17, 16), None), (0, (1, 1), (41, 29, 1, 1))):
        want = np.full(8192, 0xA5, np.uint8)
        n = SR.frame(OUT.OUT_FRAME, planes, W, H, crop, fmt, want, ow, oh, roi=roi, filter=filter, format=format, align=align,
                     alpha=9, scale=(0.5, 0.25, 2.0), bias=(1.0, -1.0, 0.0), **par)
        got = np.full(8192, 0xA5, np.uint8)
        m = BR.images(got, 0, [BR.box(0, 0, roi, (0, 0), (ow, oh))], [c], ow, oh, filter=filter, format=format, align=align, alpha=9,
                      scale=(0.5, 0.25, 2.0), bias=(1.0, -1.0, 0.0))
        assert m == n and np.array_equal(got, want), (align, ow, oh, roi)
        if format == R.PLANAR_U8 and align == 0:
            assert np.array_equal(got[:n].reshape(3, oh, ow), np.stack(SR.scaled(c, ow, oh, roi, filter)))


def test_placement_touches_the_boxes_pixels_alone():
    rng = np.random.default_rng(9)
    c = tuple(rng.integers(0, 256, (9, 11), dtype=np.uint8) for _ in range(3))
    iw, ih = 21, 13
    for format in FORMATS:
        for align in (0, 64):
            off, pitch, total = R.layout(iw, ih, format, align)
            stride = total + 7
            out = np.full(3 * stride, 0xA5, np.uint8)
            boxes = [BR.box(0, 2, (2, 1, 5, 4), (16, 9), (5, 4)), BR.box(0, 0, None, (0, 0), (3, 2)), BR.box(0, 0, (0, 0, 2, 2), (1, 1), (9, 9))]
            BR.images(out, stride, boxes, [c], iw, ih, filter=SR.BILINEAR, format=format, align=align, skip=(2,))
            assert np.all(out[stride:2 * stride] == 0xA5)                     # an image no box names
            bpp = R.BYTES_PER_PIXEL[format]
            planes = 1 if format in (R.PACKED_U8, R.PACKED_U8X4) else 3
            touched = np.flatnonzero(out != 0xA5)
            # identity at equal sizes: image 2 holds the region itself in the bottom right corner
            assert touched.size <= planes * bpp * (5 * 4 + 3 * 2)
            img = out[2 * stride:2 * stride + total]
            if format == R.PLANAR_U8:
                assert np.array_equal(img[:pitch[0] * ih].reshape(ih, pitch[0])[9:13, 16:21], c[0][1:5, 2:7])
            assert np.all(out[2 * stride + total:] == 0xA5) and np.all(out[total:stride] == 0xA5)
