"""The host half of the scaled RGB output stage (include/h264r_output.h): the exports, the layout of
h264r_scale_desc, h264r_output_rgb_scaled_geometry and every host refusal; and the properties of the
definition itself, checked on its numpy restatement (tests/scale_restate.py).  No GPU is needed.
"""
import ctypes as C
import itertools
import os
import subprocess
import tempfile
from fractions import Fraction
from math import gcd

import numpy as np
import pytest

import h264r
import rgb_restate as R
import scale_restate as SR
from h264r import _abi as A
from h264r import output as OUT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = (R.PACKED_U8, R.PACKED_U8X4, R.PLANAR_U8, R.PLANAR_F16)
FILTERS = (SR.BILINEAR, SR.AREA)
SIZES = (1, 2, 3, 7, 16, 17, 33)


def _src(W=11, H=9, crop=OUT.Crop(), align=0):
    return OUT._desc(W, H, crop, OUT.PLANAR, align, False)


def _desc(out_w=7, out_h=5, roi=None, filter=SR.AREA, src=None, **rgb):
    return OUT.scale_desc(OUT.rgb_desc(src or _src(), **rgb), out_w, out_h, roi, filter)


def _status(desc, fmt=1):
    return h264r.lib().h264r_output_rgb_scaled_geometry(fmt, C.byref(desc), C.byref(OUT.RgbGeom()))


# ------------------------------------------------------------------------------ the ABI
def test_library_exports_the_two_functions():
    L = h264r.lib()
    assert hasattr(L, "h264r_output_rgb_scaled_geometry") and hasattr(L, "h264r_output_rgb_scaled")
    assert (OUT.SCALE_BILINEAR, OUT.SCALE_AREA) == (0, 1)


def test_struct_layout_matches_c():
    names = ["rgb", "roi_x", "roi_y", "roi_w", "roi_h", "out_w", "out_h", "filter", "pad"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "h264r_output.h"\nint main(void) {\n'
           '  printf("%zu %zu %d %d %d\\n", sizeof(h264r_scale_desc), sizeof(h264r_rgb_desc), H264R_SCALE_BILINEAR, '
           'H264R_SCALE_AREA, H264R_SCALE_MAX_OUT);\n'
           + "".join(f'  printf("%zu\\n", offsetof(h264r_scale_desc, {n}));\n' for n in names) + "  return 0; }\n")
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "l.c")
        with open(c, "w") as f:
            f.write(src)
        exe = os.path.join(td, "l")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        v = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert v[:5] == [C.sizeof(OUT.ScaleDesc), C.sizeof(OUT.RgbDesc), OUT.SCALE_BILINEAR, OUT.SCALE_AREA, SR.MAX_OUT]
    assert v[5:] == [getattr(OUT.ScaleDesc, n).offset for n in names]
    assert C.sizeof(OUT.ScaleDesc) == C.sizeof(OUT.RgbDesc) + 32


# ------------------------------------------------------------------------------ geometry
GRID = [(11, 9, (0, 0, 0, 0)), (11, 9, (1, 2, 3, 2)), (22, 18, (3, 1, 2, 5)), (120, 68, (0, 0, 0, 4)), (3, 2, (5, 4, 3, 2)),
        (1, 1, (1, 2, 1, 1))]


@pytest.mark.parametrize("fmt", (0, 1, 2, 3))
@pytest.mark.parametrize("format", FORMATS)
def test_geometry_is_the_rgb_layout_at_the_output_size(fmt, format):
    n = 0
    for (W, H, (l, r, t, b)), align, (ow, oh) in itertools.product(GRID, (0, 64, 256), ((1, 1), (7, 3), (224, 224), (33, 17))):
        crop = OUT.Crop(l, r, t, b)
        lw, lh = OUT.geometry(W, H, crop, fmt).luma[2:]
        for roi in (None, (0, 0, lw, lh), (lw // 2, lh // 3, lw - lw // 2, lh - lh // 3), (lw - 1, lh - 1, 1, 1)):
            for filter in FILTERS:
                d = _desc(ow, oh, roi, filter, src=_src(W, H, crop, align), format=format)
                g = OUT.scaled_geometry(d, fmt)
                off, pitch, total = R.layout(ow, oh, format, align)
                assert (g.width, g.height) == (ow, oh)
                assert (g.plane_off, g.plane_pitch, g.frame_bytes) == (off, pitch, total), (W, H, crop, align, ow, oh, roi)
                n += 1
    assert n == len(GRID) * 3 * 4 * 4 * 2


def test_geometry_named_cases():
    src = _src(120, 68, OUT.Crop(bottom=4))
    g = OUT.scaled_geometry(_desc(224, 224, src=src, format=R.PLANAR_F16), 1)
    assert (g.width, g.height, g.plane_pitch, g.frame_bytes) == (224, 224, (448,) * 3, 3 * 448 * 224)
    g = OUT.scaled_geometry(_desc(960, 540, src=src, format=R.PACKED_U8), 1)
    assert (g.plane_pitch, g.plane_off, g.frame_bytes) == ((2880, 0, 0), (0, 0, 0), 2880 * 540)
    g = OUT.scaled_geometry(_desc(33, 17, src=_src(120, 68, OUT.Crop(bottom=4), 64), format=R.PLANAR_U8), 1)
    assert g.plane_pitch == (64,) * 3 and g.plane_off == (0, 64 * 17, 2 * 64 * 17)


# ------------------------------------------------------------------------------ refusals
def test_refuses_what_the_rgb_geometry_refuses():
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
    assert L.h264r_output_rgb_scaled_geometry(1, None, C.byref(OUT.RgbGeom())) == A.EINVAL
    assert L.h264r_output_rgb_scaled_geometry(1, C.byref(_desc()), None) == A.EINVAL
    assert L.h264r_output_rgb_scaled(None, C.byref(_desc()), None, 1, None, 0, None) == A.EINVAL


def test_refuses_a_bad_region_size_filter_or_pad():
    lw, lh = 176, 144                                             # 11 x 9 MBs, no crop
    ok = [(0, 0, 0, 0), (0, 0, lw, lh), (5, 3, 1, 1), (lw - 1, lh - 1, 1, 1), (1, 1, lw - 1, lh - 1), (0, 7, lw, 1)]
    for roi in ok:
        assert _status(_desc(roi=roi)) == A.OK, roi
    bad = [(-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, -4, 4), (0, 0, 4, -4), (0, 0, 0, 4), (0, 0, 4, 0), (1, 0, 0, 0), (0, 1, 0, 0),
           (1, 0, lw, lh), (0, 1, lw, lh), (0, 0, lw + 1, lh), (0, 0, lw, lh + 1), (lw, 0, 1, 1), (0, lh, 1, 1),
           (2 ** 31 - 1, 0, 2, 2), (0, 0, 2 ** 31 - 1, 2 ** 31 - 1)]
    for roi in bad:
        assert _status(_desc(roi=roi)) == A.EINVAL, roi
    # the region is inside the CROPPED rectangle
    crop = OUT.Crop(1, 2, 3, 2)                                   # 4:2:0: 170 x 134
    assert _status(_desc(roi=(0, 0, 170, 134), src=_src(crop=crop))) == A.OK
    assert _status(_desc(roi=(0, 0, 171, 134), src=_src(crop=crop))) == A.EINVAL
    assert _status(_desc(roi=(1, 0, 170, 134), src=_src(crop=crop))) == A.EINVAL
    for ow, oh in ((0, 5), (5, 0), (-1, 5), (5, -1), (16385, 5), (5, 16385)):
        assert _status(_desc(ow, oh)) == A.EINVAL, (ow, oh)
    assert _status(_desc(16384, 1, filter=SR.BILINEAR)) == A.OK and _status(_desc(1, 16384, filter=SR.BILINEAR)) == A.OK
    for f in (-1, 2, 7):
        assert _status(_desc(filter=f)) == A.EINVAL, f
    d = _desc()
    d.pad = 1
    assert _status(d) == A.EINVAL


def test_unsupported_gbr_off_444_and_argument_errors_come_first():
    for fmt in (0, 1, 2):
        assert _status(_desc(matrix=R.GBR), fmt) == A.EUNSUPPORTED, fmt
        assert _status(_desc(matrix=R.GBR, roi=(0, 0, 177, 1)), fmt) == A.EINVAL
        assert _status(_desc(0, 5, matrix=R.GBR), fmt) == A.EINVAL
    assert _status(_desc(matrix=R.GBR), 3) == A.OK


def test_area_bound():
    """rw * rh <= 2^23, in the reduced unit of each axis."""
    full = lambda n: _src(n, n)                                   # 4:0:0: any crop of one sample
    mono = lambda d: _status(d, 0)
    assert 2896 * 2896 == 8386816 <= 2 ** 23 < 2897 * 2897
    assert mono(_desc(1, 1, src=full(181))) == A.OK               # 2896 x 2896 -> 1 x 1
    crop = OUT.Crop(right=15, bottom=15)                          # 182 MBs = 2912, less 15: 2897
    assert OUT.geometry(182, 182, crop, 0).luma[2:] == (2897, 2897)
    assert mono(_desc(1, 1, src=_src(182, 182, crop))) == A.EUNSUPPORTED
    assert mono(_desc(1, 1, src=_src(182, 182, crop), filter=SR.BILINEAR)) == A.OK      # AREA's bound alone
    assert mono(_desc(1, 1, roi=(1, 1, 2896, 2896), src=_src(182, 182, crop))) == A.OK  # the region counts, not the crop
    assert mono(_desc(224, 224, src=full(1024))) == A.OK          # 16384 -> 224: the reduced size is 512 x 512
    assert 16384 // gcd(16384, 224) == 512
    assert mono(_desc(223, 223, src=full(1024))) == A.EUNSUPPORTED
    assert mono(_desc(1, 2897, src=_src(182, 182, crop))) == A.OK  # rh = 1
    assert SR.area_supported(2896, 2896, 1, 1) and not SR.area_supported(2897, 2897, 1, 1)
    assert SR.area_supported(16384, 16384, 224, 224)


# ------------------------------------------------------------------------------ the definition's properties
PAIRS = sorted(set(itertools.product((1, 2, 3, 7, 16, 17, 33, 134, 170, 1080, 1920), SIZES + (224, 540, 960))))


def test_identity_at_equal_sizes():
    rng = np.random.default_rng(1)
    for h, w in ((1, 1), (1, 7), (7, 1), (16, 17), (33, 2)):
        c = rng.integers(0, 256, (h, w), dtype=np.uint8)
        for f in FILTERS:
            assert np.array_equal(SR.resample(c, h, w, f), c), (h, w, f)
    # per axis: the other axis scaled, this one untouched
    c = rng.integers(0, 256, (16, 17), dtype=np.uint8)
    for f in FILTERS:
        assert np.array_equal(SR.resample(c, 16, 17, f), c)


def test_weights_sum_to_256_and_to_S():
    for S, D in PAIRS:
        i0, i1, w0, w1 = SR.bilinear_axis(S, D)
        assert np.all(w0 + w1 == 256) and w1.min() >= 0 and w1.max() <= 256
        assert i0.min() >= 0 and i1.max() <= S - 1 and np.all((i1 == i0 + 1) | ((i1 == i0) & (w1 == 0)))
        if D == S:
            assert np.all(w1 == 0) and np.array_equal(i0, np.arange(S))
        o = SR.area_axis(S, D)
        assert np.all(o.sum(axis=1) == S) and np.all(o.sum(axis=0) == D) and o.min() >= 0
        # a window is contiguous and holds ceil(S / D) + 1 samples at most
        for d in range(D):
            nz = np.flatnonzero(o[d])
            assert nz[-1] - nz[0] + 1 == len(nz) <= -(-S // D) + 1
            assert nz[0] == d * S // D and nz[-1] + 1 == -(-(d + 1) * S // D)
        # the unit does not matter
        g = gcd(S, D)
        if g > 1:
            small = SR.area_axis(S // g, D // g)
            assert np.array_equal(o.reshape(g, D // g, g, S // g).sum(axis=(0, 2)), g * g * small)
            assert all(np.array_equal(o[k * (D // g):(k + 1) * (D // g), k * (S // g):(k + 1) * (S // g)], g * small) for k in range(g))


def test_accumulators_stay_inside_their_bounds():
    for S, D in ((16384, 16384), (16384, 1), (1, 16384), (16383, 16384), (16384, 16383)):
        d = np.array([0, D // 2, D - 1], dtype=np.int64)
        p = np.clip((2 * d + 1) * S - D, 0, 2 * D * (S - 1))
        f = p - 2 * D * (p // (2 * D))
        assert max(((2 * d + 1) * S).max(), p.max(), (256 * f + D).max()) < 2 ** 31
    c = np.full((3, 5), 255, np.uint8)
    assert SR.bilinear_sums(c, 7, 2).max() == 255 * 65536 < 2 ** 24
    # AREA in the reduced unit: 2 A + T <= 511 T < 2^32 for T <= 2^23
    assert 511 * SR.AREA_MAX_T < 2 ** 32
    c = np.full((6, 9), 255, np.uint8)
    for oh, ow in ((1, 1), (4, 6), (5, 7)):
        a = SR.area_sums(c, oh, ow)
        assert np.all(a == 255 * 6 * 9)
    # the accumulator an implementation keeps: A in the reduced unit, at the largest T the bound admits.
    # 5792 -> 2 columns reduce to 2896 -> 1, so T = 2896 * 2896 = 8,386,816 <= 2^23 although S_h * S_w is twice that.
    sh, sw, oh, ow = 2896, 5792, 1, 2
    gh, gw = gcd(sh, oh), gcd(sw, ow)
    T = (sh // gh) * (sw // gw)
    assert T == 8386816 <= SR.AREA_MAX_T and SR.area_supported(sw, sh, ow, oh)
    wv, wh = SR.area_axis(sh, oh) // gh, SR.area_axis(sw, ow) // gw          # the reduced unit's weights
    assert np.array_equal(wv * gh, SR.area_axis(sh, oh)) and np.array_equal(wh * gw, SR.area_axis(sw, ow))
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
    noise[:, sw // 2:] |= 0xF0                                               # one output dark to bright, one bright
    half = np.zeros((sh, sw), np.uint8)
    half[:sh // 2] = 255
    for c in (np.full((sh, sw), 255, np.uint8), half, noise):
        A = wv @ c.astype(np.int64) @ wh.T
        assert A.max() <= 255 * T and (2 * A + T).max() < 2 ** 32
        v = ((2 * A + T).astype(np.uint32) // np.uint32(2 * T)).astype(np.uint8)    # in 32 bits, as the kernel has it
        assert np.array_equal(v, SR.resample(c, oh, ow, SR.AREA))
    assert 2 * 255 * T + T == 511 * T > 2 ** 31                              # and it needs all 32 of them


def test_bilinear_is_within_one_and_a_half_of_float64():
    rng = np.random.default_rng(2)
    worst = 0.0
    for (sh, sw), (dh, dw) in (((9, 11), (33, 17)), ((33, 17), (7, 16)), ((16, 16), (3, 33)), ((2, 3), (17, 7)), ((134, 170), (33, 33)),
                               ((1, 5), (2, 16))):
        c = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
        got = SR.resample(c, dh, dw, SR.BILINEAR).astype(np.float64)

        def axis(S, D):
            pos = np.clip((np.arange(D) + 0.5) * S / D - 0.5, 0, S - 1)
            i0 = np.floor(pos).astype(int)
            return i0, np.minimum(i0 + 1, S - 1), pos - i0
        r0, r1, fv = axis(sh, dh)
        x0, x1, fh = axis(sw, dw)
        cf = c.astype(np.float64)
        top = cf[r0][:, x0] * (1 - fh) + cf[r0][:, x1] * fh
        bot = cf[r1][:, x0] * (1 - fh) + cf[r1][:, x1] * fh
        want = top * (1 - fv)[:, None] + bot * fv[:, None]
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"bilinear against float64: worst {worst:.3f}")
    assert worst <= 1.5                                           # 255 * 2 / 512 from the two 8-bit weights, 1/2 from the rounding


def test_area_is_round_half_up_of_the_exact_mean():
    rng = np.random.default_rng(3)
    for (sh, sw), (dh, dw) in (((9, 11), (2, 3)), ((16, 16), (4, 8)), ((7, 5), (3, 7)), ((4, 6), (1, 1)), ((3, 2), (7, 3)), ((17, 33), (16, 17))):
        c = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
        got = SR.resample(c, dh, dw, SR.AREA)
        for dy in range(dh):
            for dx in range(dw):
                total = Fraction(0)
                for r in range(sh):
                    ov = max(Fraction(0), min(Fraction((dy + 1) * sh, dh), r + 1) - max(Fraction(dy * sh, dh), r))
                    for x in range(sw):
                        oh = max(Fraction(0), min(Fraction((dx + 1) * sw, dw), x + 1) - max(Fraction(dx * sw, dw), x))
                        total += ov * oh * int(c[r, x])
                mean = total / (Fraction(sh, dh) * Fraction(sw, dw))
                assert int(got[dy, dx]) == (mean + Fraction(1, 2)).__floor__(), (sh, sw, dh, dw, dy, dx)
    # the rounding term exactly on the half: top half 255, bottom half 0
    c = np.zeros((4, 2), np.uint8)
    c[:2] = 255
    assert SR.resample(c, 1, 1, SR.AREA)[0, 0] == 128


def test_region_and_frame_compose_with_the_rgb_restatement():
    rng = np.random.default_rng(4)
    W, H, crop, fmt = 3, 2, OUT.Crop(1, 2, 1, 0), 1
    planes = [(rng.integers(0, 256, (32, 48), dtype=np.uint8), rng.integers(0, 256, (16, 24), dtype=np.uint8),
               rng.integers(0, 256, (16, 24), dtype=np.uint8))]
    c = R.channels(*R.source_frame(planes[0], W, H, crop, fmt), fmt, R.BT601, 1, R.BILINEAR, True)
    lh, lw = c[0].shape
    out = np.full(4096, 0xA5, np.uint8)
    n = SR.frame(OUT.OUT_FRAME, planes, W, H, crop, fmt, out, 7, 3, roi=(5, 3, 9, 11), filter=SR.BILINEAR, matrix=R.BT601,
                 full_range=1, up=R.BILINEAR, format=R.PLANAR_U8, bgr=True, align=64)
    assert n == 3 * 64 * 3 and np.all(out[n:] == 0xA5)
    for k in range(3):
        want = SR.resample(c[k][3:14, 5:14], 3, 7, SR.BILINEAR)
        assert np.array_equal(out[k * 192:(k + 1) * 192].reshape(3, 64)[:, :7], want)
    # a region of one sample makes every output that sample
    one = SR.scaled(c, 5, 4, (lw - 1, lh - 1, 1, 1), SR.AREA)
    assert all(np.all(one[k] == c[k][-1, -1]) for k in range(3))
