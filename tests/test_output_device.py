"""The host half of the device-side output stage (include/h264r_output.h): h264r_output_geometry.

It must state the crop windows exactly as h264r/output.py:geometry does (the reference's
output.cc:135-165, already pinned by tests/test_output.py and the streams' MD5s), lay the planes of a
frame out as the header says for both layouts and every pitch alignment, and refuse what the header
lists.  No GPU is needed: the function is pure host code of libh264r.so.
"""
import ctypes as C
import itertools

import pytest

import h264r
from h264r import _abi as A
from h264r import output as OUT

FORMATS = (0, 1, 2, 3)
SUB = {0: (1, 1), 1: (2, 2), 2: (2, 1), 3: (1, 1)}        # SubWidthC, SubHeightC (4:0:0: the crop units)

# (width_mbs, frame_height_mbs, (left, right, top, bottom)): no crop, every single offset, all four,
# the committed streams' crops, the 1080p crop, and crops that leave almost nothing
GRID = [
    (11, 9, (0, 0, 0, 0)), (11, 9, (1, 0, 0, 0)), (11, 9, (0, 1, 0, 0)), (11, 9, (0, 0, 1, 0)), (11, 9, (0, 0, 0, 1)),
    (11, 9, (1, 2, 3, 2)), (22, 18, (3, 1, 2, 5)), (22, 18, (2, 1, 0, 3)), (40, 30, (1, 2, 0, 4)),
    (120, 68, (0, 0, 0, 4)), (120, 68, (0, 0, 0, 2)), (3, 2, (5, 4, 3, 2)), (1, 2, (3, 2, 1, 2)), (1, 1, (1, 2, 1, 1)),
]


def _expect_layout(fmt, py, layout, align, fake):
    """plane_off / plane_pitch / frame_bytes from the header's rule and output.py's rectangles."""
    lw, lh = py.luma[2:]
    cw, ch = py.chroma[2:]
    if fmt:
        planes = [(lw, lh), (2 * cw, ch)] if layout == OUT.SEMIPLANAR else [(lw, lh), (cw, ch), (cw, ch)]
    elif fake and py.fake_uv:
        planes = [(lw, lh), (2 * py.fake_uv, 1)] if layout == OUT.SEMIPLANAR else [(lw, lh), (py.fake_uv, 1), (py.fake_uv, 1)]
    else:
        planes = [(lw, lh)]
    off, offs, pitches = 0, [], []
    for w, h in planes:
        pitch = w if align <= 1 else -(-w // align) * align
        offs.append(off)
        pitches.append(pitch)
        off += pitch * h
    pad = [0] * (3 - len(planes))
    return tuple(offs + pad), tuple(pitches + pad), off


@pytest.mark.parametrize("fmt", FORMATS)
def test_geometry_equals_output_py(fmt):
    for (W, H, (l, r, t, b)), fmo in itertools.product(GRID, (1, 0)):
        crop = OUT.Crop(l, r, t, b, frame_mbs_only=fmo)
        try:
            py = OUT.geometry(W, H, crop, fmt)
        except ValueError:
            with pytest.raises(h264r.H264RError) as e:
                OUT.device_geometry(W, H, crop, fmt)
            assert e.value.status == A.EINVAL, (fmt, W, H, crop)
            continue
        g = OUT.device_geometry(W, H, crop, fmt, fake_chroma=fmt == 0)
        assert g.luma == py.luma and g.chroma == py.chroma, (fmt, W, H, crop)
        assert g.frame_bytes == py.frame_bytes, (fmt, W, H, crop)          # rows contiguous: the reference's bytes
        sw, sh = SUB[fmt]
        assert g.luma[0] == sw * l and g.luma[1] == sh * t * (2 - fmo)


def test_geometry_named_cases():
    # hp400_cif_ippp_8x8_wp: 4:0:0, CropUnitX 1, an odd width and height
    g = OUT.device_geometry(22, 18, OUT.Crop(3, 1, 2, 5), 0, fake_chroma=True)
    assert g.luma == (3, 2, 348, 281) and g.chroma == (0, 0, 0, 0)
    assert g.plane_off == (0, 348 * 281, 348 * 281 + (348 * 281) // 4) and g.frame_bytes == 348 * 281 + 2 * ((348 * 281) // 4)
    # one MB cropped to 2 x 2 luma samples
    g = OUT.device_geometry(1, 1, OUT.Crop(3, 4, 3, 4), 1)
    assert g.luma == (6, 6, 2, 2) and g.chroma == (3, 3, 1, 1) and g.frame_bytes == 6
    g = OUT.device_geometry(1, 1, OUT.Crop(7, 7, 7, 7), 3)
    assert g.luma == (7, 7, 2, 2) and g.chroma == (7, 7, 2, 2) and g.frame_bytes == 12
    # frame_mbs_only 0 doubles the vertical unit: 1080i in 68 MB rows
    g = OUT.device_geometry(120, 68, OUT.Crop(bottom=2, frame_mbs_only=0), 1)
    assert g.luma == (0, 0, 1920, 1080) and g.chroma == (0, 0, 960, 540)


@pytest.mark.parametrize("layout", [OUT.PLANAR, OUT.SEMIPLANAR])
@pytest.mark.parametrize("align", [0, 1, 64, 256])
@pytest.mark.parametrize("fmt", FORMATS)
def test_layout_offsets_and_pitches(fmt, align, layout):
    for (W, H, (l, r, t, b)), fmo, fake in itertools.product(GRID, (1, 0), (False, True)):
        if fake and fmt:
            continue
        crop = OUT.Crop(l, r, t, b, frame_mbs_only=fmo)
        try:
            py = OUT.geometry(W, H, crop, fmt)
        except ValueError:
            continue
        g = OUT.device_geometry(W, H, crop, fmt, layout, align, fake)
        off, pitch, total = _expect_layout(fmt, py, layout, align, fake)
        assert (g.plane_off, g.plane_pitch, g.frame_bytes) == (off, pitch, total), (fmt, W, H, crop, fake)
        if align > 1:
            assert all(o % align == 0 and p % align == 0 for o, p in zip(g.plane_off, g.plane_pitch))


def _status(fmt, **kw):
    d = dict(width_mbs=11, frame_height_mbs=9, crop_left=0, crop_right=0, crop_top=0, crop_bottom=0,
             frame_mbs_only=1, layout=OUT.PLANAR, pitch_align=0, fake_chroma=0)
    d.update(kw)
    return h264r.lib().h264r_output_geometry(fmt, C.byref(OUT.OutDesc(**d)), C.byref(OUT.OutGeom()))


def test_refusals():
    assert _status(1) == A.OK
    for side in ("crop_left", "crop_right", "crop_top", "crop_bottom"):
        assert _status(1, **{side: -1}) == A.EINVAL, side                       # a negative crop
    # crops that leave nothing: by width, by height, by the doubled vertical unit alone
    assert _status(1, crop_left=44, crop_right=44) == A.EINVAL
    assert _status(1, crop_top=36, crop_bottom=36) == A.EINVAL
    assert _status(1, crop_top=18, crop_bottom=17) == A.OK
    assert _status(1, crop_top=18, crop_bottom=18, frame_mbs_only=0) == A.EINVAL
    assert _status(3, crop_left=100, crop_right=76) == A.EINVAL
    assert _status(0, crop_left=100, crop_right=75) == A.OK                     # 4:0:0: one luma column left
    assert _status(1, layout=2) == A.EINVAL and _status(1, layout=-1) == A.EINVAL
    for bad in (-1, 3, 48, 8192, 4097):
        assert _status(1, pitch_align=bad) == A.EINVAL, bad
    for good in (0, 1, 2, 16, 64, 256, 4096):
        assert _status(1, pitch_align=good) == A.OK, good
    for fmt in (1, 2, 3):
        assert _status(fmt, fake_chroma=1) == A.EUNSUPPORTED
    assert _status(0, fake_chroma=1) == A.OK
    assert _status(4) == A.EINVAL and _status(-1) == A.EINVAL
    assert _status(1, width_mbs=0) == A.EINVAL and _status(1, frame_height_mbs=0) == A.EINVAL
    assert _status(1, frame_mbs_only=2) == A.EINVAL
    L = h264r.lib()
    assert L.h264r_output_geometry(1, None, C.byref(OUT.OutGeom())) == A.EINVAL
    assert L.h264r_output_geometry(1, C.byref(OUT.OutDesc(11, 9, 0, 0, 0, 0, 1, 0, 0, 0)), None) == A.EINVAL


def test_output_frames_refuses_bad_arguments_without_a_device():
    """h264r_output_frames checks its host arguments before it touches the GPU: a NULL context is
    H264R_EINVAL here, where there is none (the stride and table checks run on the GPU box)."""
    d = OUT.OutDesc(11, 9, 0, 0, 0, 0, 1, 0, 0, 0)
    assert h264r.lib().h264r_output_frames(None, C.byref(d), None, 1, None, 0, None) == A.EINVAL


def test_pair_fields_follows_the_stream_helper():
    """DeviceOutput's pairing helper states the rule of tests/streams.py:output_frames, on every
    committed capture that holds field pictures."""
    import numpy as np
    import streams as S
    names = [n for n, c in S.STREAMS.items() if c.get("field")]
    assert len(names) == 8
    for name in names:
        pics = S.load_capture(S.capture_path(name))
        tags = [(np.full((1, 1), i, np.uint8),) for i in range(len(pics))]      # one 1 x 1 "plane" naming the picture
        want = [tuple(int(v) for v in f[0][:, 0]) for f in S.output_frames(pics, tags)]
        got = OUT.pair_fields([S.structure(p) for p in pics], [int(p["pic"]["poc"][0]) for p in pics])
        assert [tuple(i for i in f[1:] if i >= 0) for f in got] == want, name
        assert all((k == OUT.OUT_FIELD_PAIR) == (b >= 0) for k, _, b in got)
    # a field whose partner never comes is an unpaired field of its parity
    assert OUT.pair_fields([A.TOP_FIELD, A.FRAME, A.BOTTOM_FIELD], [0, 2, 4]) == [
        (OUT.OUT_UNPAIRED_TOP, 0, -1), (OUT.OUT_FRAME, 1, -1), (OUT.OUT_UNPAIRED_BOT, 2, -1)]
