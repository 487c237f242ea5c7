"""Scaled RGB frames on MI355X: h264r_output_rgb_scaled (include/h264r_output.h, k_output_rgb_scaled in
k_output_scale.hip).

Every comparison is byte-exact against tests/scale_restate.py, the numpy restatement of the header's
definition on top of tests/rgb_restate.py; no expected byte comes from the library.  Destinations are
prefilled with 0xA5 and compared whole, so a byte written outside a frame's rows (pitch padding, the
gap between frames, the bytes around the buffer) fails like a wrong pixel.  Plane contents, sources
and crops are those of tests/test_gpu_output_rgb.py.

Output sizes come from SIZES per axis; the widths take 31 as well, the one size here that is 15 mod 16.
"""
import numpy as np
import pytest

import h264r
import rgb_restate as R
import scale_restate as SR
from h264r import _abi as A
from h264r import output as OUT
from h264r import synth
from test_gpu_output_rgb import (FILL, FORMATS, IMAGENET, KINDS, ROWS, UNIT, _content, _decode, _hcrops, _sources, _split_planar,
                                 _upload, _vcrops)

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 7, 16, 17, 33)
WIDTHS = SIZES + (31,)
FILTERS = (SR.BILINEAR, SR.AREA)


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
    """None; an odd origin and an odd size; one sample; a region that touches the crop's last row and
    column (a bilinear chroma tap clamps inside it)."""
    x, y = min(1, lw - 1), min(1, lh - 1)
    w, h = (lw - x - 1) | 1 if lw - x > 1 else 1, (lh - y - 1) | 1 if lh - y > 1 else 1
    w, h = min(w, lw - x), min(h, lh - y)
    if w % 2 == 0:
        w -= 1
    if h % 2 == 0:
        h -= 1
    tw, th = min(lw, 5), min(lh, 3)
    return [None, (x, y, w, h), (lw // 2, lh // 2, 1, 1), (lw - tw, lh - th, tw, th)]


def _job(dec, fmt, W, H, crop, kinds, host, lead, gap, align, ow, oh, roi, filter, **par):
    """Run one job into a 0xA5 buffer (frames `gap` bytes apart beyond their size, the first `lead` bytes
    off the allocation) and compare every byte of the buffer with scale_restate."""
    import torch
    n = len(kinds)
    pool, addr = _upload(host)
    out = OUT.DeviceOutput(dec, W, H, crop, pitch_align=align)
    rp = dict(matrix=par.get("matrix", R.BT709), full_range=par.get("full_range", 0), up=par.get("chroma_up", R.REPLICATE),
              format=par["format"], bgr=par.get("bgr", 0), alpha=par.get("alpha", 255), scale=par.get("scale", UNIT["scale"]),
              bias=par.get("bias", UNIT["bias"]), align=align, roi=roi, filter=filter)
    fb = R.layout(ow, oh, par["format"], align)[2]
    stride = fb + gap
    total = lead + n * stride + 64
    want = np.full(total, FILL, np.uint8)
    for i, k in enumerate(kinds):
        assert SR.frame(k, host[i], W, H, crop, fmt, want[lead + i * stride:], ow, oh, **rp) == fb
    buf = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    dst = buf[lead:lead + n * stride].view(n, stride)
    table = out.frames_from([(k,) + tuple(addr[i]) for i, k in enumerate(kinds)])
    view = out.rgb_scaled(table, ow, oh, roi=roi, filter=filter, dst=dst, **par)
    dec.check()
    got = buf.cpu().numpy()
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        pytest.fail(f"fmt {fmt} {W}x{H} crop {crop} kinds {kinds} -> {ow}x{oh} roi {roi} filter {filter} align {align} lead {lead} "
                    f"gap {gap} {par}: {len(bad)} bytes differ, first at {bad[0] - lead} of frame stride {stride} "
                    f"(got {got[bad[0]]}, want {want[bad[0]]})")
    del pool
    return view


# ------------------------------------------------------------------------------ 1. directed small shapes
@pytest.mark.parametrize("W,H", [(1, 1), (3, 2), (11, 9)])
@pytest.mark.parametrize("fmt", [1, 2, 3, 0], ids=["420", "422", "444", "400"])
def test_directed_small_shapes(decs, fmt, W, H):
    """Every horizontal crop x every format x both chroma_up values x both filters; the output size, the
    region, and the parameters of the RGB stage are drawn so that each of their values meets each
    filter (and each format where the format matters)."""
    dec = decs[fmt]
    sw, sh = R.SUB[fmt]
    rng = np.random.default_rng(2000 * fmt + 16 * W + H)
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
        kinds = [KINDS[(job // 2 + 3 * i) % 4] if field_ok else OUT.OUT_FRAME for i in range(n)]
        matrix, fr = ROWS[(job // 6) % 6]
        bgr = (job // 10) % 2
        align = (0, 64)[(job // 14) % 2]
        f16 = format == R.PLANAR_F16
        lead = (0, 2)[(job // 16) % 2] if f16 else (0, 1, 5, 15)[(job // 16) % 4]
        gap = (0, 38, 48)[(job // 4) % 3] if f16 else (0, 37, 48)[(job // 4) % 3]
        ow, oh = WIDTHS[(job // 2) % 8], SIZES[(job // 2 + job // 16) % 7]
        rois = _rois(lw, lh)
        roi = rois[(job // 2 + job // 8) % 4]
        host = [_sources(k, W, H, fmt, (job // 2 + i) % 3, rng) for i, k in enumerate(kinds)]
        par = dict(format=format, chroma_up=up, matrix=matrix, full_range=fr, bgr=bgr, alpha=(255, 0, 0x5A)[job % 3])
        par.update((UNIT, IMAGENET)[(job // 8) % 2] if f16 else {})
        _job(dec, fmt, W, H, crop, kinds, host, lead, gap, align, ow, oh, roi, filter, **par)
        seen |= {("kind", filter, k) for k in kinds} | {("row", matrix, fr), ("bgr", format, bgr), ("align", format, align),
                                                        ("lead", format, lead), ("n", n), ("ow", filter, ow), ("oh", filter, oh),
                                                        ("roi", filter, rois.index(roi)), ("up", filter, up)}
        job += 1
    assert {x[1:] for x in seen if x[0] == "row"} == set(ROWS)
    assert {x[1] for x in seen if x[0] == "n"} == {1, 2, 5}
    for format in FORMATS:
        assert {x[2] for x in seen if x[:2] == ("bgr", format)} == {0, 1}
        assert {x[2] for x in seen if x[:2] == ("align", format)} == {0, 64}
        assert {x[2] for x in seen if x[:2] == ("lead", format)} == ({0, 2} if format == R.PLANAR_F16 else {0, 1, 5, 15})
    for filter in FILTERS:
        assert {x[2] for x in seen if x[:2] == ("ow", filter)} == set(WIDTHS)
        assert {x[2] for x in seen if x[:2] == ("oh", filter)} == set(SIZES)
        assert {x[2] for x in seen if x[:2] == ("roi", filter)} == {0, 1, 2, 3}
        assert {x[2] for x in seen if x[:2] == ("up", filter)} == {R.REPLICATE, R.BILINEAR}
        if H % 2 == 0:
            assert {x[2] for x in seen if x[:2] == ("kind", filter)} == set(KINDS)


@pytest.mark.parametrize("fmt", [1, 2, 3, 0], ids=["420", "422", "444", "400"])
def test_every_kind_under_a_matrix_row_and_gbr(decs, fmt):
    """3 x 2 MBs: all four kinds in one job; one (matrix, range) row per format under both filters and
    both chroma_up values, and GBR on 4:4:4."""
    dec = decs[fmt]
    rng = np.random.default_rng(177 + fmt)
    W, H = 3, 2
    crop = OUT.Crop(1, 2, 1, 0, frame_mbs_only=0)
    rows = [ROWS[(2 * fmt + 1) % 6]] + ([(R.GBR, 0)] if fmt == 3 else [])
    for j, ((matrix, fr), up, filter) in enumerate((row, up, f) for row in rows for up in (R.REPLICATE, R.BILINEAR) for f in FILTERS):
        kinds = KINDS[j % 4:] + KINDS[:j % 4]
        host = [_sources(k, W, H, fmt, (i + j) % 3, rng) for i, k in enumerate(kinds)]
        _job(dec, fmt, W, H, crop, kinds, host, 0, 16, 64, (17, 33, 7, 16)[j % 4], (7, 16, 33, 3)[j % 4], (None, (3, 5, 21, 9))[j % 2],
             filter, format=FORMATS[j % 4], chroma_up=up, matrix=matrix, full_range=fr, bgr=j % 2, **IMAGENET)


# ------------------------------------------------------------------------------ 2. ratios
@pytest.mark.parametrize("fmt", [1, 3], ids=["420", "444"])
def test_named_ratios(decs, fmt):
    """On 48 x 32 (3 x 2 MBs): identity, 2 x and non-integer upscale, 2 x and 4 x integer downscale, coprime
    ratios, the whole frame to 1 x 1 -- per axis and both at once, under both filters."""
    dec = decs[fmt]
    rng = np.random.default_rng(31 + fmt)
    W, H = 3, 2
    host = [_sources(OUT.OUT_FRAME, W, H, fmt, what, rng) for what in (2, 0)]
    cases = [((0, 0, 16, 7), 16, 7), ((2, 1, 33, 17), 33, 17),          # identity
             ((4, 2, 8, 8), 16, 16), ((1, 1, 8, 1), 16, 2), ((5, 3, 7, 3), 16, 7), ((0, 0, 3, 2), 33, 33),   # upscale
             ((0, 0, 32, 32), 16, 16), ((3, 1, 34, 14), 17, 7), ((1, 3, 28, 28), 7, 7), ((0, 0, 48, 32), 3, 2),   # 2 x, 4 x, 16 x down
             ((1, 1, 17, 31), 7, 3), ((0, 0, 47, 31), 33, 17), ((0, 0, 48, 7), 31, 16),                         # coprime, mixed
             (None, 1, 1), ((1, 0, 47, 32), 1, 1), (None, 1, 33), (None, 33, 1)]
    for j, (roi, ow, oh) in enumerate(cases):
        for filter in FILTERS:
            _job(dec, fmt, W, H, OUT.Crop(), [OUT.OUT_FRAME] * 2, host, 0, 0, 0, ow, oh, roi, filter, format=R.PLANAR_U8,
                 chroma_up=j % 2, matrix=ROWS[j % 6][0], full_range=ROWS[j % 6][1])


@pytest.mark.parametrize("fmt", [1, 2, 3, 0], ids=["420", "422", "444", "400"])
def test_identity_is_what_output_rgb_writes(decs, fmt):
    """D == S: the scaled job's bytes are those h264r_output_rgb writes for the same table, device output
    against device output, in every format under both filters; and a region at its own size is that
    region of the RGB frame."""
    import torch
    dec = decs[fmt]
    rng = np.random.default_rng(41 + fmt)
    W, H, crop = 3, 2, OUT.Crop(1, 2 if fmt else 1, 1, 0, frame_mbs_only=0)
    kinds = KINDS
    host = [_sources(k, W, H, fmt, i % 3, rng) for i, k in enumerate(kinds)]
    pool, addr = _upload(host)
    lw, lh = OUT.geometry(W, H, crop, fmt).luma[2:]
    for align in (0, 64):
        out = OUT.DeviceOutput(dec, W, H, crop, pitch_align=align)
        table = out.frames_from([(k,) + tuple(addr[i]) for i, k in enumerate(kinds)])
        for j, (format, filter) in enumerate((f, s) for f in FORMATS for s in FILTERS):
            par = dict(format=format, chroma_up=j % 2, matrix=ROWS[j % 6][0], full_range=ROWS[j % 6][1], bgr=j % 2, alpha=9, **IMAGENET)
            fb = R.layout(lw, lh, format, align)[2]
            a = torch.full((len(kinds), fb), FILL, dtype=torch.uint8, device="cuda")
            b = torch.full((len(kinds), fb), FILL, dtype=torch.uint8, device="cuda")
            full = out.rgb(table, dst=a, **par)
            out.rgb_scaled(table, lw, lh, filter=filter, dst=b, **par)
            dec.check()
            assert torch.equal(a, b), (format, filter, align)
            if format == R.PLANAR_U8:
                roi = (3, 1, 17, 7)
                part = out.rgb_scaled(table, 17, 7, roi=roi, filter=filter, **par)
                dec.check()
                assert torch.equal(part, full[:, :, 1:8, 3:20]), (filter, align)
    del pool


# ------------------------------------------------------------------------------ 3. the AREA bound
def test_area_bound_on_a_400_context(decs):
    """181 x 181 MBs (2896 x 2896, T = 8,386,816 <= 2^23) at full range to 1 x 1: all 255 gives 255; the
    top half 255 and the bottom half 0 gives 128 -- the rounding term at 2 A + T = 256 T."""
    import torch
    dec = decs[0]
    n = 181
    y = torch.full((2, 16 * n, 16 * n), 255, dtype=torch.uint8, device="cuda")
    y[1, 8 * n:] = 0
    out = OUT.DeviceOutput(dec, n, n)
    table = out.frames_from([(OUT.OUT_FRAME, (y[0], None, None)), (OUT.OUT_FRAME, (y[1], None, None))])
    got = out.rgb_scaled(table, 1, 1, filter=SR.AREA, full_range=True, matrix=R.BT709, format=R.PLANAR_U8)
    dec.check()
    got = got.cpu().numpy()
    assert got.shape == (2, 3, 1, 1)
    assert got[0].reshape(-1).tolist() == [255] * 3 and got[1].reshape(-1).tolist() == [128] * 3


# ------------------------------------------------------------------------------ 4. against the existing stage
def _scaled_equals_restated_yuv(dec, table, W, H, crop, fmt):
    """h264r_output_frames planar on the table; scale_restate on those bytes == h264r_output_rgb_scaled."""
    yuv = OUT.DeviceOutput(dec, W, H, crop, fake_chroma=fmt == 0).run(table)
    out = OUT.DeviceOutput(dec, W, H, crop)
    dec.check()
    yuv = yuv.cpu().numpy()
    lw, lh = OUT.geometry(W, H, crop, fmt).luma[2:]
    jobs = [(format, up, filter) for format in FORMATS for up in (R.REPLICATE, R.BILINEAR) for filter in FILTERS]
    for j, (format, up, filter) in enumerate(jobs):
        par = dict(matrix=ROWS[j % 6][0], full_range=ROWS[j % 6][1], bgr=j % 2)
        ow, oh = (33, 17, 16, 7)[j % 4], (17, 33, 7, 16)[(j // 4) % 4]
        roi = (None, (lw - 41, lh - 33, 41, 33))[(j // 2) % 2]
        got = out.rgb_scaled(table, ow, oh, roi=roi, filter=filter, format=format, chroma_up=up, **par, **IMAGENET)
        dec.check()
        raw = got.cpu().numpy()
        for k in range(table.n):
            c = R.channels(*_split_planar(yuv[k], W, H, crop, fmt), fmt, par["matrix"], par["full_range"], up, par["bgr"])
            want = np.zeros(R.layout(ow, oh, format, 0)[2], np.uint8)
            R.write_frame(want, SR.scaled(c, ow, oh, roi, filter), format, 0, 255, IMAGENET["scale"], IMAGENET["bias"])
            g = np.ascontiguousarray(raw[k])
            assert np.array_equal(g.view(np.uint8).reshape(-1), want), f"frame {k} format {format} chroma_up {up} filter {filter}"


@pytest.mark.parametrize("fmt", [1, 2, 3, 0], ids=["420", "422", "444", "400"])
def test_frame_batch_from_decoder(L, decs, fmt):
    """A decoded frame batch: the scaled job reads the batch's own out planes on the same stream."""
    dec = decs[fmt]
    over = {} if fmt == 1 else dict(chroma_format={2: 2, 3: 3, 0: A.SYNTH_CHROMA_400}[fmt])
    db = _decode(L, dec, [synth.default_cfg(L, 3, 11, 9, **over)], 3)
    crop = OUT.Crop(1, 2, 1, 3)
    t = db.tensors
    out = OUT.DeviceOutput(dec, 11, 9, crop)
    table = out.frames_from([(OUT.OUT_FRAME, (t["out_y"][i], t["out_u"][i] if fmt else None, t["out_v"][i] if fmt else None))
                             for i in (2, 0, 1)])
    _scaled_equals_restated_yuv(dec, table, 11, 9, crop, fmt)


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
    _scaled_equals_restated_yuv(dec, table, 11, 8, crop, 1)


# ------------------------------------------------------------------------------ 5. the torch wrapper
@pytest.mark.parametrize("align", [0, 64])
@pytest.mark.parametrize("fmt", [1, 0], ids=["420", "400"])
def test_wrapper_views(decs, fmt, align):
    import torch
    dec = decs[fmt]
    W, H, crop, n = 3, 2, OUT.Crop(3, 4 if fmt else 3, 1, 0), 2
    rng = np.random.default_rng(53)
    host = [_sources(OUT.OUT_FRAME, W, H, fmt, 2, rng) for _ in range(n)]
    pool, addr = _upload(host)
    out = OUT.DeviceOutput(dec, W, H, crop, pitch_align=align)
    table = out.frames_from([(OUT.OUT_FRAME,) + tuple(addr[i]) for i in range(n)])
    ow, oh, roi = 17, 7, (1, 3, 30, 21)
    for format in FORMATS:
        t = out.rgb_scaled(table, ow, oh, roi=roi, filter=SR.AREA, format=format, bgr=True, alpha=7)
        dec.check()
        pitch = R.pitch_of(ow, format, align)
        fb = R.layout(ow, oh, format, align)[2]
        if format in (R.PACKED_U8, R.PACKED_U8X4):
            ch = 3 if format == R.PACKED_U8 else 4
            assert t.dtype == torch.uint8 and tuple(t.shape) == (n, oh, ow, ch) and t.stride() == (fb, pitch, ch, 1)
        elif format == R.PLANAR_U8:
            assert t.dtype == torch.uint8 and tuple(t.shape) == (n, 3, oh, ow) and t.stride() == (fb, pitch * oh, pitch, 1)
        else:
            assert t.dtype == torch.float16 and tuple(t.shape) == (n, 3, oh, ow)
            assert t.stride() == (fb // 2, pitch * oh // 2, pitch // 2, 1)
        assert t.is_contiguous() == (align == 0)
        got = t.cpu().numpy()
        for i in range(n):
            c = R.channels(*R.source_frame(host[i][0], W, H, crop, fmt), fmt, R.BT709, 0, R.REPLICATE, True)
            c = SR.scaled(c, ow, oh, roi, SR.AREA)
            if format in (R.PACKED_U8, R.PACKED_U8X4):
                px = list(c) + ([np.full_like(c[0], 7)] if format == R.PACKED_U8X4 else [])
                assert np.array_equal(got[i], np.stack(px, axis=2))
            elif format == R.PLANAR_U8:
                assert np.array_equal(got[i], np.stack(c))
            else:
                want = np.stack([R.half_bits(c[k], 1 / 255, 0) for k in range(3)])
                assert np.array_equal(got[i].view(np.uint16), want)
    # the defaults: the whole rectangle, AREA, planar u8
    t = out.rgb_scaled(table, 3, 2)
    dec.check()
    c = SR.scaled(R.channels(*R.source_frame(host[0][0], W, H, crop, fmt), fmt), 3, 2)
    assert np.array_equal(t[0].cpu().numpy(), np.stack(c))
    # a raw table needs its count, a destination its shape
    with pytest.raises(ValueError):
        out.rgb_scaled(table.tensor.data_ptr(), 3, 2)
    with pytest.raises(ValueError):
        out.rgb_scaled(table, 3, 2, dst=torch.zeros(4, dtype=torch.uint8, device="cuda"))
    del pool


# ------------------------------------------------------------------------------ 6. refusals
def test_refused_frames_are_skipped_and_reported(decs):
    """A kind outside 0..3 and a NULL plane the kind needs: the frame keeps its 0xA5, its neighbours are
    written, check() reports H264R_EDEVICE once, and the next good job passes.  The bad entries hold NULL
    or valid pointers only, and the kernel tests them before it uses any."""
    import torch
    dec = decs[1]
    W, H = 3, 2
    crop = OUT.Crop(1, 0, 0, 1)
    rng = np.random.default_rng(64)
    out = OUT.DeviceOutput(dec, W, H, crop)
    hfrm = _sources(OUT.OUT_FRAME, W, H, 1, 2, rng)
    hfld = _sources(OUT.OUT_FIELD_PAIR, W, H, 1, 1, rng)
    frm = tuple(torch.from_numpy(a).cuda() for a in hfrm[0])
    fld = [tuple(torch.from_numpy(a).cuda() for a in s) for s in hfld]
    ow, oh = 17, 7
    for format, up, filter in ((R.PACKED_U8, R.BILINEAR, SR.AREA), (R.PLANAR_F16, R.REPLICATE, SR.BILINEAR)):
        rp = dict(format=format, up=up, filter=filter)
        fb = R.layout(ow, oh, format, 0)[2]
        good_frame, good_pair = np.zeros(fb, np.uint8), np.zeros(fb, np.uint8)
        assert SR.frame(OUT.OUT_FRAME, hfrm, W, H, crop, 1, good_frame, ow, oh, **rp) == fb
        SR.frame(OUT.OUT_FIELD_PAIR, hfld, W, H, crop, 1, good_pair, ow, oh, **rp)
        untouched = np.full(fb, FILL, np.uint8)
        jobs = [
            ([(OUT.OUT_FRAME, frm), (9, frm), (OUT.OUT_FIELD_PAIR, fld[0], fld[1])], [good_frame, untouched, good_pair]),
            ([(OUT.OUT_FIELD_PAIR, fld[0], (None, fld[1][1], fld[1][2])), (OUT.OUT_FRAME, frm)], [untouched, good_frame]),
            ([(OUT.OUT_FIELD_PAIR, fld[0], (fld[1][0], fld[1][1], None)), (OUT.OUT_FRAME, frm)], [untouched, good_frame]),
            ([(-1, frm), (OUT.OUT_FRAME, (frm[0], None, frm[2])), (OUT.OUT_UNPAIRED_BOT, (None, fld[0][1], fld[0][2]))],
             [untouched] * 3),
        ]
        for rows, wants in jobs:
            dst = torch.full((len(rows), fb), FILL, dtype=torch.uint8, device="cuda")
            out.rgb_scaled(out.frames_from(rows), ow, oh, filter=filter, dst=dst, format=format, chroma_up=up)
            with pytest.raises(h264r.H264RError) as e:
                dec.check()
            assert e.value.status == A.EDEVICE
            got = dst.cpu().numpy()
            for i, w in enumerate(wants):
                assert np.array_equal(got[i], w), f"frame {i} of {[r[0] for r in rows]}"
            # the error word is cleared by the report: a good job after it passes
            dst = torch.full((2, fb), FILL, dtype=torch.uint8, device="cuda")
            out.rgb_scaled(out.frames_from([(OUT.OUT_FIELD_PAIR, fld[0], fld[1]), (OUT.OUT_FRAME, frm)]), ow, oh, filter=filter,
                           dst=dst, format=format, chroma_up=up)
            dec.check()
            got = dst.cpu().numpy()
            assert np.array_equal(got[0], good_pair) and np.array_equal(got[1], good_frame)


def test_host_refusals_on_a_context(decs):
    import ctypes as C
    import torch
    dec = decs[1]
    out = OUT.DeviceOutput(dec, 3, 2)
    y = torch.zeros(32 * 48, dtype=torch.uint8, device="cuda")
    table = out.frames_from([(OUT.OUT_FRAME, (y, y, y))])
    call = lambda desc, tab, n, d, stride: dec._L.h264r_output_rgb_scaled(dec.handle, C.byref(desc) if desc is not None else None,
                                                                          tab, n, d, stride, None)
    tp = table.tensor.data_ptr()
    for format in FORMATS:
        desc = OUT.scale_desc(OUT.rgb_desc(out.desc, format=format), 17, 7)
        fb = OUT.scaled_geometry(desc, 1).frame_bytes
        dst = torch.zeros(fb + 16, dtype=torch.uint8, device="cuda")
        dp = dst.data_ptr()
        assert call(desc, tp, 1, dp, fb - 1) == A.EINVAL               # frames would overlap
        assert call(desc, None, 1, dp, fb) == A.EINVAL and call(desc, tp, 1, None, fb) == A.EINVAL
        assert call(desc, tp, -1, dp, fb) == A.EINVAL
        assert call(None, tp, 1, dp, fb) == A.EINVAL
        assert call(desc, tp, 0, dp, fb) == A.OK                        # nothing to do
        odd = A.EINVAL if format == R.PLANAR_F16 else A.OK             # binary16 wants even addresses
        assert call(desc, tp, 1, dp + 1, fb) == odd and call(desc, tp, 1, dp, fb + 1) == odd
        assert call(desc, tp, 1, dp, fb) == A.OK
    assert call(OUT.scale_desc(OUT.rgb_desc(out.desc), 17, 7, roi=(0, 0, 49, 32)), tp, 1, dp, fb) == A.EINVAL
    assert call(OUT.scale_desc(OUT.rgb_desc(out.desc), 17, 7, filter=2), tp, 1, dp, fb) == A.EINVAL
    assert call(OUT.scale_desc(OUT.rgb_desc(out.desc, matrix=R.GBR), 17, 7), tp, 1, dp, fb) == A.EUNSUPPORTED
    dec.check()
