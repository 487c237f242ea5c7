"""The host half of the RGB output stage (include/h264r_output.h): h264r_rgb_coefficients,
h264r_output_rgb_geometry and the host refusals of h264r_output_rgb.  No GPU is needed: these are pure
host functions of libh264r.so.  The expected values are tests/rgb_restate.py's, written from the header.
"""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import h264r
import rgb_restate as R
from h264r import _abi as A
from h264r import output as OUT

ROWS = [(m, fr) for m in (R.BT601, R.BT709, R.BT2020) for fr in (0, 1)]
TABLE = {
    (R.BT601, 0): (19077, 26149, -6419, -13320, 33050, 16), (R.BT601, 1): (16384, 22970, -5638, -11700, 29032, 0),
    (R.BT709, 0): (19077, 29372, -3494, -8731, 34610, 16), (R.BT709, 1): (16384, 25802, -3069, -7670, 30402, 0),
    (R.BT2020, 0): (19077, 27503, -3069, -10657, 35091, 16), (R.BT2020, 1): (16384, 24160, -2696, -9361, 30825, 0),
}
FORMATS = (R.PACKED_U8, R.PACKED_U8X4, R.PLANAR_U8, R.PLANAR_F16)
# the crop grid of tests/test_output_device.py
GRID = [
    (11, 9, (0, 0, 0, 0)), (11, 9, (1, 0, 0, 0)), (11, 9, (0, 1, 0, 0)), (11, 9, (0, 0, 1, 0)), (11, 9, (0, 0, 0, 1)),
    (11, 9, (1, 2, 3, 2)), (22, 18, (3, 1, 2, 5)), (22, 18, (2, 1, 0, 3)), (40, 30, (1, 2, 0, 4)),
    (120, 68, (0, 0, 0, 4)), (120, 68, (0, 0, 0, 2)), (3, 2, (5, 4, 3, 2)), (1, 2, (3, 2, 1, 2)), (1, 1, (1, 2, 1, 1)),
]


def _lib_coefficients(matrix, full_range):
    k = (C.c_int32 * 6)()
    assert h264r.lib().h264r_rgb_coefficients(matrix, full_range, k) == A.OK
    return tuple(k)


@pytest.mark.parametrize("matrix,full_range", ROWS)
def test_coefficients_are_the_derivation_and_the_table(matrix, full_range):
    got = _lib_coefficients(matrix, full_range)
    assert got == R.coefficients(matrix, full_range) == TABLE[(matrix, full_range)]
    # the same in floating point, as the header writes it
    kr, kb = (float(x) for x in R.K[matrix])
    kg = 1 - kr - kb
    ys, cs, yo = (255, 255, 0) if full_range else (219, 224, 16)
    real = (255 / ys, 255 * 2 * (1 - kr) / cs, -255 * 2 * kb * (1 - kb) / (kg * cs), -255 * 2 * kr * (1 - kr) / (kg * cs),
            255 * 2 * (1 - kb) / cs)
    assert got == tuple(math.floor(x * 2 ** 14 + 0.5) for x in real) + (yo,)


def test_coefficients_refusals():
    L = h264r.lib()
    k = (C.c_int32 * 6)()
    assert L.h264r_rgb_coefficients(R.BT709, 0, None) == A.EINVAL
    for m in (-1, R.GBR, 4):
        assert L.h264r_rgb_coefficients(m, 0, k) == A.EINVAL, m
    for fr in (-1, 2):
        assert L.h264r_rgb_coefficients(R.BT709, fr, k) == A.EINVAL, fr


@pytest.mark.parametrize("matrix,full_range", ROWS)
def test_integer_matrix_is_within_one_of_float64(matrix, full_range):
    """Over 256 Y x (every C8 multiple of 8)^2 and 256 Y x (a step-3 grid of C8 in 0..2040)^2: the integer
    formula differs from clip255(floor(float64 + 1/2)) by at most 1, in fewer than 0.2 % of the samples
    (measured: at most 0.13 %), and no accumulator reaches 2^27."""
    coef = R.coefficients(matrix, full_range)
    cy, crv, cgu, cgv, cbu, yo = coef
    (fy, frv, fgu, fgv, fbu), _ = R.reals(matrix, full_range)
    fy, frv, fgu, fgv, fbu = (float(x) for x in (fy, frv, fgu, fgv, fbu))
    for grid in (np.arange(0, 2041, 8), np.arange(0, 2041, 3)):
        c = grid.astype(np.int32) - 1024
        cf = grid.astype(np.float64) / 8 - 128
        # the chroma terms once: rows = Cb8, columns = Cr8 (R depends on Cr8 alone, B on Cb8 alone)
        terms = [(crv * c, frv * cf), ((cgu * c)[:, None] + (cgv * c)[None, :], (fgu * cf)[:, None] + (fgv * cf)[None, :]),
                 (cbu * c, fbu * cf)]
        assert all(np.abs(t[0]).max() < 2 ** 27 for t in terms)
        diff = total = 0
        for Y in range(256):
            yt = 8 * cy * (Y - yo) + 65536
            assert abs(yt) < 2 ** 27
            for ti, tf in terms:
                acc = yt + ti
                assert np.abs(acc).max() < 2 ** 27
                got = np.clip(acc >> 17, 0, 255)
                want = np.clip(np.floor(fy * (Y - yo) + tf + 0.5), 0, 255).astype(np.int32)
                d = np.abs(got - want)
                assert d.max() <= 1, (Y, int(d.max()))
                # R and B stand for a whole line of the cube each: weigh them as such
                w = 1 if ti.ndim == 2 else len(grid)
                diff += int(np.count_nonzero(d)) * w
                total += d.size * w
        share = diff / total
        print(f"matrix {matrix} full_range {full_range} grid step {grid[1]}: {100 * share:.4f} % differ")
        assert share < 0.002
    # and rgb_restate's two functions say the same on a random draw of the cube
    rng = np.random.default_rng(5)
    Y, cb8, cr8 = rng.integers(0, 256, 4096), rng.integers(0, 2041, 4096), rng.integers(0, 2041, 4096)
    for a, b in zip(R.matrix_int(Y, cb8, cr8, coef), R.matrix_real(Y, cb8, cr8, matrix, full_range)):
        assert np.abs(a - b).max() <= 1


def _py_desc(W, H, crop, align):
    return OUT._desc(W, H, crop, OUT.PLANAR, align, False)


@pytest.mark.parametrize("fmt", (0, 1, 2, 3))
@pytest.mark.parametrize("format", FORMATS)
def test_geometry_equals_the_python_geometry(fmt, format):
    for (W, H, (l, r, t, b)), fmo, align in itertools.product(GRID, (1, 0), (0, 64, 256)):
        crop = OUT.Crop(l, r, t, b, frame_mbs_only=fmo)
        d = OUT.rgb_desc(_py_desc(W, H, crop, align), format=format)
        try:
            py = OUT.geometry(W, H, crop, fmt)
        except ValueError:
            with pytest.raises(h264r.H264RError) as e:
                OUT.rgb_geometry(d, fmt)
            assert e.value.status == A.EINVAL, (fmt, W, H, crop)
            continue
        g = OUT.rgb_geometry(d, fmt)
        lw, lh = py.luma[2:]
        off, pitch, total = R.layout(lw, lh, format, align)
        assert (g.width, g.height) == (lw, lh), (fmt, W, H, crop)
        assert (g.plane_off, g.plane_pitch, g.frame_bytes) == (off, pitch, total), (fmt, format, W, H, crop, align)
        if align > 1:
            assert all(o % align == 0 and p % align == 0 for o, p in zip(g.plane_off, g.plane_pitch))


def test_geometry_named_cases():
    d = OUT.rgb_desc(_py_desc(120, 68, OUT.Crop(bottom=4), 0), format=R.PACKED_U8)
    g = OUT.rgb_geometry(d, 1)
    assert (g.width, g.height, g.plane_pitch, g.frame_bytes) == (1920, 1080, (5760, 0, 0), 3 * 1920 * 1080)
    d = OUT.rgb_desc(_py_desc(22, 18, OUT.Crop(3, 1, 2, 5), 64), format=R.PLANAR_F16)      # 348 x 281
    g = OUT.rgb_geometry(d, 0)
    assert (g.width, g.height) == (348, 281) and g.plane_pitch == (704,) * 3
    assert g.plane_off == (0, 704 * 281, 2 * 704 * 281) and g.frame_bytes == 3 * 704 * 281


def _status(fmt=1, src=None, **kw):
    s = dict(width_mbs=11, frame_height_mbs=9, crop_left=0, crop_right=0, crop_top=0, crop_bottom=0,
             frame_mbs_only=1, layout=OUT.PLANAR, pitch_align=0, fake_chroma=0)
    s.update(src or {})
    d = OUT.rgb_desc(OUT.OutDesc(**s))
    for k, v in kw.items():
        if k in ("scale", "bias"):
            setattr(d, k, (C.c_float * 3)(*v))
        else:
            setattr(d, k, v)
    return h264r.lib().h264r_output_rgb_geometry(fmt, C.byref(d), C.byref(OUT.RgbGeom()))


def test_host_refusals():
    assert _status() == A.OK
    # everything h264r_output_geometry refuses
    for side in ("crop_left", "crop_right", "crop_top", "crop_bottom"):
        assert _status(src={side: -1}) == A.EINVAL, side
    assert _status(src=dict(crop_left=44, crop_right=44)) == A.EINVAL
    assert _status(src=dict(crop_top=18, crop_bottom=18, frame_mbs_only=0)) == A.EINVAL
    for bad in (-1, 3, 48, 8192):
        assert _status(src=dict(pitch_align=bad)) == A.EINVAL, bad
    assert _status(src=dict(width_mbs=0)) == A.EINVAL and _status(src=dict(frame_height_mbs=1025)) == A.EINVAL
    assert _status(src=dict(frame_mbs_only=2)) == A.EINVAL
    assert _status(4) == A.EINVAL and _status(-1) == A.EINVAL
    # the source is the planar frame, and never the fake chroma
    for layout in (OUT.SEMIPLANAR, 2, -1):
        assert _status(src=dict(layout=layout)) == A.EINVAL, layout
    assert _status(src=dict(fake_chroma=1)) == A.EINVAL and _status(0, src=dict(fake_chroma=1)) == A.EINVAL
    # the enums, the flags, alpha
    for name, bad in (("matrix", (-1, 4)), ("chroma_up", (-1, 2)), ("format", (-1, 4)), ("full_range", (-1, 2)),
                      ("bgr", (-1, 2)), ("alpha", (-1, 256))):
        for v in bad:
            assert _status(**{name: v}) == A.EINVAL, (name, v)
    assert _status(alpha=0) == A.OK and _status(alpha=255) == A.OK
    # scale / bias: finite
    for name in ("scale", "bias"):
        for v in (float("nan"), float("inf"), float("-inf")):
            for k in range(3):
                vals = [1.0, 1.0, 1.0]
                vals[k] = v
                assert _status(**{name: vals}) == A.EINVAL, (name, v, k)
        assert _status(**{name: (-3.5, 0.0, 1e30)}) == A.OK
    # GBR is 4:4:4's
    for fmt in (0, 1, 2):
        assert _status(fmt, matrix=R.GBR) == A.EUNSUPPORTED, fmt
    assert _status(3, matrix=R.GBR) == A.OK
    assert _status(1, matrix=R.GBR, format=9) == A.EINVAL          # an argument error comes first
    L = h264r.lib()
    assert L.h264r_output_rgb_geometry(1, None, C.byref(OUT.RgbGeom())) == A.EINVAL
    assert L.h264r_output_rgb_geometry(1, C.byref(OUT.rgb_desc(OUT.OutDesc(11, 9, 0, 0, 0, 0, 1, 0, 0, 0))), None) == A.EINVAL


def test_output_rgb_refuses_a_null_context_without_a_device():
    d = OUT.rgb_desc(OUT.OutDesc(11, 9, 0, 0, 0, 0, 1, 0, 0, 0))
    assert h264r.lib().h264r_output_rgb(None, C.byref(d), None, 1, None, 0, None) == A.EINVAL


def test_layout_two_of_the_yuv_stage_stays_refused():
    """RGB is an entry point of its own, not a third layout of h264r_output_geometry."""
    d = OUT.OutDesc(11, 9, 0, 0, 0, 0, 1, 2, 0, 0)
    assert h264r.lib().h264r_output_geometry(1, C.byref(d), C.byref(OUT.OutGeom())) == A.EINVAL
