"""The host half of the resampled RGB output stage (include/h264r_output.h): the exports, the layout of
h264r_resample_desc, h264r_output_rgb_resampled_geometry and its refusals, h264r_resample_axis against the
restatement's tables; and the restatement itself (tests/resample_restate.py) against Pillow -- against
PIL where it imports, and against the MD5s recorded from Pillow 12.2 (tests/golden/resample_pillow.json)
everywhere.  No GPU is needed.
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import h264r
import resample_restate as RR
import rgb_restate as R
from h264r import _abi as A
from h264r import output as OUT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resample_pillow.json")
FORMATS = (R.PACKED_U8, R.PACKED_U8X4, R.PLANAR_U8, R.PLANAR_F16)

# (in_size, in0, in1, out_size): 1920 / 1080 -> 224, scale 16 (LANCZOS ksize 97), scale 1 / 8, odd ratios, regions
# inside the axis, windows clamped at both ends (5 -> 1, 1 -> 5, 16 -> 1, 48 -> 1), out_size 1, one sample
# inside, identity, one more and one fewer, a ksize far beyond the kernel's (16384 -> 224)
AXES = [(1920, 0, 1920, 224), (1080, 0, 1080, 224), (176, 0, 176, 11), (144, 0, 144, 9), (16, 0, 16, 128), (37, 0, 37, 7),
        (37, 3, 33, 7), (23, 2, 19, 40), (5, 0, 5, 1), (1, 0, 1, 5), (16, 0, 16, 1), (48, 0, 48, 1), (200, 10, 170, 10),
        (64, 1, 63, 9), (3, 1, 2, 7), (176, 0, 176, 176), (100, 0, 100, 99), (99, 0, 99, 100), (16384, 0, 16384, 224),
        (177, 0, 177, 11), (832, 9, 825, 17)]
GRID = [(f,) + a for f in RR.FILTERS for a in AXES]


def _src(W=11, H=9, crop=OUT.Crop(), align=0):
    return OUT._desc(W, H, crop, OUT.PLANAR, align, False)


def _desc(out_w=50, out_h=37, roi=None, filter=RR.BICUBIC, src=None, **rgb):
    return OUT.resample_desc(OUT.rgb_desc(src or _src(), **rgb), out_w, out_h, roi, filter)


def _status(desc, fmt=1):
    return h264r.lib().h264r_output_rgb_resampled_geometry(fmt, C.byref(desc), C.byref(OUT.RgbGeom()))


# ------------------------------------------------------------------------------ the ABI
def test_library_exports_the_entry_points():
    L = h264r.lib()
    for name in ("h264r_output_rgb_resampled_geometry", "h264r_resample_axis", "h264r_resample_plan_create",
                 "h264r_resample_plan_destroy", "h264r_output_rgb_resampled"):
        assert hasattr(L, name), name


def test_struct_layout_and_constants_match_c():
    names = ["rgb", "roi_x", "roi_y", "roi_w", "roi_h", "out_w", "out_h", "filter", "pad"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "h264r_output.h"\nint main(void) {\n'
           '  printf("%zu %d %d %d %d %d %d\\n", sizeof(h264r_resample_desc), H264R_RESAMPLE_TRIANGLE, H264R_RESAMPLE_BICUBIC, '
           'H264R_RESAMPLE_LANCZOS, H264R_RESAMPLE_MAX_TAPS, H264R_RESAMPLE_TILE_W, H264R_RESAMPLE_TILE_H);\n'
           + "".join(f'  printf("%zu\\n", offsetof(h264r_resample_desc, {n}));\n' for n in names) + "  return 0; }\n")
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "l.c")
        with open(c, "w") as f:
            f.write(src)
        exe = os.path.join(td, "l")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        v = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert v[:7] == [C.sizeof(OUT.ResampleDesc), OUT.RESAMPLE_TRIANGLE, OUT.RESAMPLE_BICUBIC, OUT.RESAMPLE_LANCZOS,
                     OUT.RESAMPLE_MAX_TAPS, OUT.RESAMPLE_TILE_W, OUT.RESAMPLE_TILE_H]
    assert v[7:] == [getattr(OUT.ResampleDesc, n).offset for n in names]
    assert C.sizeof(OUT.ResampleDesc) == C.sizeof(OUT.ScaleDesc) and RR.MAX_TAPS == OUT.RESAMPLE_MAX_TAPS >= 97


# ------------------------------------------------------------------------------ the restatement is Pillow's resampler
def test_restatement_equals_the_recorded_pillow_outputs():
    """MD5s of PIL.Image.resize's bytes (Pillow 12.2, mode L) for resample_restate.CASES, inputs from
    numpy.random.default_rng(k): compared wherever the suite runs."""
    gold = json.load(open(GOLDEN))
    assert len(gold["cases"]) == len(RR.CASES) == 30
    for k, rec in enumerate(gold["cases"]):
        f, shape = RR.CASES[k]
        assert (rec["filter"], tuple(rec["in"]), tuple(rec["out"]), rec["box"] and tuple(rec["box"])) == (RR.PIL_NAMES[f], shape[:2], shape[2:4], shape[4])
        assert hashlib.md5(case_bytes(RR.case_restated(k))).hexdigest() == rec["md5"], (k, RR.CASES[k])


def case_bytes(a):
    return np.ascontiguousarray(a).tobytes()


def test_restatement_equals_pillow_where_it_is_installed():
    pytest.importorskip("PIL")
    for k in range(len(RR.CASES)):
        assert np.array_equal(RR.case_restated(k), RR.case_pillow(k)), (k, RR.CASES[k])
    # and through an RGB image: Pillow resamples the bands alike
    from PIL import Image
    rng = np.random.default_rng(99)
    c = tuple(RR.edges(23, 37, rng) for _ in range(3))
    im = Image.fromarray(np.stack(c, axis=2)).resize((11, 9), Image.Resampling.LANCZOS, box=(3, 2, 33, 19))
    want = RR.resampled(c, 11, 9, (3, 2, 30, 17), RR.LANCZOS)
    assert np.array_equal(np.asarray(im), np.stack(want, axis=2))


def test_the_clip_between_the_passes_shows_on_the_mutation_input():
    m = RR.MUTATION
    y = RR.blocks(m["h"], m["w"])
    assert set(np.unique(y)) == {0, 255}
    roi = (0, 0, m["w"], m["h"])
    a = RR.resample(y, roi, m["out_w"], m["out_h"], m["filter"])
    b = RR.resample(y, roi, m["out_w"], m["out_h"], m["filter"], clip_between=False)
    assert not np.array_equal(a, b)
    # a region's windows read past it: not crop(box).resize()
    c = RR.edges(32, 48, np.random.default_rng(7))
    assert not np.array_equal(RR.resample(c, (11, 7, 20, 12), 9, 5, RR.BICUBIC), RR.resample(c, (11, 7, 20, 12), 9, 5, RR.BICUBIC, clamp_to_region=True))


# ------------------------------------------------------------------------------ h264r_resample_axis
@pytest.fixture(scope="module")
def tables():
    """The restatement's table of every axis of GRID, built once."""
    return {g: RR.axis(*g) for g in GRID}


def test_axis_equals_the_restatement(tables):
    for g in GRID:
        xmin, count, kk = OUT.resample_axis(*g)
        rx, rc, rk, ks = tables[g]
        assert kk.shape == (g[4], ks) and ks == RR.ksize_of(g[0], g[2], g[3], g[4]), g
        assert np.array_equal(xmin, rx) and np.array_equal(count, rc) and np.array_equal(kk, rk), g
    assert tables[(RR.LANCZOS, 176, 0, 176, 11)][3] == 97 and tables[(RR.LANCZOS, 177, 0, 177, 11)][3] == 99
    assert tables[(RR.TRIANGLE, 48, 0, 48, 1)][3] == 97 and tables[(RR.BICUBIC, 16, 0, 16, 128)][3] == 5


def test_tables_keep_every_accumulator_in_32_bits(tables):
    worst = 0
    for g, (xmin, count, kk, ks) in tables.items():
        mag = np.abs(kk).sum(axis=1)
        assert np.all(255 * mag + 2 ** 21 < 2 ** 31), g
        assert np.abs(kk).max() < 2 ** 23, g                       # a tap is one 24-bit factor
        assert np.all(count >= 1) and np.all(count <= ks) and np.all(xmin >= 0) and np.all(xmin + count <= g[1]), g
        assert np.all(np.diff(xmin) >= 0) and np.all(np.diff(xmin + count) >= 0), g      # the kernel's tile spans rely on it
        assert np.all(np.abs(kk.sum(axis=1) - 2 ** 22) <= ks), g   # normalised: each tap is rounded once
        worst = max(worst, int(mag.max()))
    print(f"largest sum of |kk|: {worst} = {worst / 2 ** 22:.3f} x 2^22")


def test_axis_refusals():
    L = h264r.lib()
    ks = C.c_int32(77)
    call = lambda *a: L.h264r_resample_axis(*a, None, None, None, C.byref(ks))
    assert call(RR.BICUBIC, 176, 0, 176, 11) == A.OK and ks.value == 2 * 32 + 1   # support 2 x 16
    for bad in ((-1, 4, 0, 4, 2), (3, 4, 0, 4, 2), (0, 0, 0, 0, 2), (0, 4, 2, 2, 2), (0, 4, 3, 2, 2), (0, 4, 0, 5, 2), (0, 4, -1, 4, 2),
                (0, 4, 0, 4, 0), (0, 4, 0, 4, 16385)):
        assert call(*bad) == A.EINVAL, bad
    assert L.h264r_resample_axis(0, 4, 0, 4, 2, None, None, None, None) == A.EINVAL
    one = (C.c_int32 * 2)()
    assert L.h264r_resample_axis(0, 4, 0, 4, 2, one, None, None, C.byref(ks)) == A.EINVAL
    with pytest.raises(h264r.H264RError):
        OUT.resample_axis(3, 4, 0, 4, 2)


def test_stand_alone_table_check_under_the_sanitizers(tables):
    """tools/resample_tables_check.cc includes the device-free table header, is built with
    -fsanitize=address,undefined and run over GRID with arrays of exactly the stated sizes: no write leaves
    them, and its tables are the restatement's (ksize and a checksum over xmin, count and every tap)."""
    def checksum(xmin, count, kk):
        M, s = 2 ** 64 - 1, 1469598103934665603
        for i in range(len(xmin)):
            for v in kk[i].tolist() + [int(xmin[i]), int(count[i])]:
                s = ((s ^ (v & M)) * 1099511628211) & M
        return s
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "resample_tables_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "arrow-h264_amd", "csrc"), os.path.join(ROOT, "tools", "resample_tables_check.cc"),
                        "-o", exe], check=True)
        run = subprocess.run([exe], input="".join(" ".join(str(x) for x in g) + "\n" for g in GRID), capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.split("\n")[:-1]
    assert len(lines) == len(GRID)
    for g, line in zip(GRID, lines):
        xmin, count, kk, ks = tables[g]
        assert line == f"{ks} {checksum(xmin, count, kk)}", g


# ------------------------------------------------------------------------------ geometry
def test_geometry_is_the_rgb_layout_at_the_output_size():
    n = 0
    for fmt in (0, 1, 2, 3):
        for format in FORMATS:
            for align, (ow, oh), filter in ((0, (50, 37), RR.TRIANGLE), (64, (224, 224), RR.BICUBIC), (256, (33, 17), RR.LANCZOS)):
                for roi in (None, (16, 8, 100, 90), (175, 143, 1, 1)):
                    g = OUT.resampled_geometry(_desc(ow, oh, roi, filter, src=_src(align=align), format=format), fmt)
                    off, pitch, total = R.layout(ow, oh, format, align)
                    assert (g.width, g.height, g.plane_off, g.plane_pitch, g.frame_bytes) == (ow, oh, off, pitch, total)
                    n += 1
    assert n == 4 * 4 * 3 * 3
    src = _src(120, 68, OUT.Crop(bottom=4))
    for f in RR.FILTERS:                                           # the flagship job under each filter
        g = OUT.resampled_geometry(_desc(224, 224, filter=f, src=src, format=R.PLANAR_F16), 1)
        assert (g.width, g.height, g.plane_pitch, g.frame_bytes) == (224, 224, (448,) * 3, 3 * 448 * 224)


def test_refuses_what_the_scaled_geometry_refuses():
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
    assert L.h264r_output_rgb_resampled_geometry(1, None, C.byref(OUT.RgbGeom())) == A.EINVAL
    assert L.h264r_output_rgb_resampled_geometry(1, C.byref(_desc()), None) == A.EINVAL
    assert L.h264r_output_rgb_resampled(None, None, None, 1, None, 0, None) == A.EINVAL
    assert L.h264r_resample_plan_create(None, C.byref(_desc()), C.byref(C.c_void_p())) == A.EINVAL
    # the region, the size, the filter, the pad
    lw, lh = 176, 144
    for roi in ((0, 0, 0, 0), (0, 0, lw, lh), (5, 3, 16, 16), (lw - 16, lh - 16, 16, 16), (1, 1, lw - 1, lh - 1)):
        assert _status(_desc(roi=roi)) == A.OK, roi
    for roi in ((-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, -4, 4), (0, 0, 4, -4), (0, 0, 0, 4), (0, 0, 4, 0), (1, 0, 0, 0), (0, 1, 0, 0),
                (1, 0, lw, lh), (0, 1, lw, lh), (0, 0, lw + 1, lh), (0, 0, lw, lh + 1), (lw, 0, 1, 1), (0, lh, 1, 1),
                (2 ** 31 - 1, 0, 2, 2), (0, 0, 2 ** 31 - 1, 2 ** 31 - 1)):
        assert _status(_desc(roi=roi)) == A.EINVAL, roi
    crop = OUT.Crop(1, 2, 3, 2)                                   # 4:2:0: 170 x 134 -- the region is inside the CROP
    assert _status(_desc(roi=(0, 0, 170, 134), src=_src(crop=crop))) == A.OK
    assert _status(_desc(roi=(0, 0, 171, 134), src=_src(crop=crop))) == A.EINVAL
    for ow, oh in ((0, 5), (5, 0), (-1, 5), (5, -1), (16385, 50), (50, 16385)):
        assert _status(_desc(ow, oh)) == A.EINVAL, (ow, oh)
    assert _status(_desc(16384, 16384)) == A.OK
    for f in (-1, 3, 7):
        assert _status(_desc(filter=f)) == A.EINVAL, f
    d = _desc()
    d.pad = 1
    assert _status(d) == A.EINVAL


def test_unsupported_beyond_max_taps_and_argument_errors_come_first():
    """ksize = H264R_RESAMPLE_MAX_TAPS passes and one step above it (ksize is odd: 99) does not, on either
    axis, under each filter at its own largest scale; H264R_EINVAL comes before H264R_EUNSUPPORTED."""
    wide = lambda w, h: _src(-(-w // 16), -(-h // 16), OUT.Crop(right=-w % 16, bottom=-h % 16))   # 4:0:0: any size
    mono = lambda d: _status(d, 0)
    for f, s in ((RR.TRIANGLE, 48), (RR.BICUBIC, 24), (RR.LANCZOS, 16)):
        n = 11 * s
        assert OUT.geometry(-(-(n + 1) // 16), 9, OUT.Crop(right=-(n + 1) % 16), 0).luma[2] == n + 1
        assert RR.ksize_of(f, 0, n, 11) == 97 and RR.ksize_of(f, 0, n + 1, 11) == 99
        assert mono(_desc(11, 9, filter=f, src=wide(n, 144))) == A.OK
        assert mono(_desc(11, 9, filter=f, src=wide(n + 1, 144))) == A.EUNSUPPORTED
        assert mono(_desc(9, 11, filter=f, src=wide(144, n))) == A.OK
        assert mono(_desc(9, 11, filter=f, src=wide(144, n + 1))) == A.EUNSUPPORTED
        assert mono(_desc(11, 9, roi=(1, 0, n, 144), filter=f, src=wide(n + 1, 144))) == A.OK      # the region counts, not the crop
        # every scale up to 16 on both axes passes under every filter
        assert mono(_desc(120, 68, filter=f, src=wide(1920, 1088))) == A.OK
    assert mono(_desc(224, 224, filter=RR.LANCZOS, src=wide(16384, 16384))) == A.EUNSUPPORTED
    assert mono(_desc(1024, 1024, filter=RR.LANCZOS, src=wide(16384, 16384))) == A.OK
    # argument errors first
    big = wide(1920, 1088)
    assert mono(_desc(1, 1, src=big)) == A.EUNSUPPORTED
    assert mono(_desc(1, 0, src=big)) == A.EINVAL and mono(_desc(1, 1, roi=(0, 0, 1921, 4), src=big)) == A.EINVAL
    assert mono(_desc(1, 1, filter=3, src=big)) == A.EINVAL
    for fmt in (0, 1, 2):
        assert _status(_desc(matrix=R.GBR), fmt) == A.EUNSUPPORTED, fmt
        assert _status(_desc(matrix=R.GBR, roi=(0, 0, 177, 1)), fmt) == A.EINVAL
        assert _status(_desc(0, 5, matrix=R.GBR), fmt) == A.EINVAL
    assert _status(_desc(matrix=R.GBR), 3) == A.OK
