"""Resampled RGB frames on MI355X: h264r_output_rgb_resampled (include/h264r_output.h, the
k_output_rgb_resampled kernels of k_output_resample.hip).

Every comparison is byte-exact against tests/resample_restate.py -- Pillow's 8-bit resampler restated from
the header, itself held to Pillow's own bytes by tests/test_output_resample.py -- applied to the planes of
tests/rgb_restate.py; no expected byte comes from the library.  Destinations are prefilled with 0xA5 and
compared whole, so a byte written outside a frame's rows fails like a wrong pixel.  Plane contents, sources
and crops are those of tests/test_gpu_output_rgb.py; noise fills the planes outside the crop.
"""
import ctypes as C

import numpy as np
import pytest

import h264r
import resample_restate as RR
import rgb_restate as R
from h264r import _abi as A
from h264r import output as OUT
from h264r import synth
from test_gpu_output_rgb import (FILL, FORMATS, IMAGENET, KINDS, ROWS, UNIT, _decode, _hcrops, _sources, _split_planar, _upload,
                                 _vcrops)

pytestmark = pytest.mark.gpu

TW, TH = OUT.RESAMPLE_TILE_W, OUT.RESAMPLE_TILE_H
FILTERS = RR.FILTERS
# output sizes: one, odd ones, one below / at / one above the kernel's tile, more than two tiles
WIDTHS = (1, 7, TW - 1, TW, TW + 1, 37, 50)
HEIGHTS = (1, 5, TH - 1, TH, TH + 1, 33, 37)


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


def _supported(lw, lh, roi, ow, oh, filter):
    x, y, w, h = RR.SR.region(lw, lh, roi)
    return max(RR.ksize_of(filter, x, x + w, ow), RR.ksize_of(filter, y, y + h, oh)) <= RR.MAX_TAPS


def _job(dec, fmt, W, H, crop, kinds, host, lead, gap, align, ow, oh, roi, filter, **par):
    """Run one job into a 0xA5 buffer (frames `gap` bytes apart beyond their size, the first `lead` bytes
    off the allocation) and compare every byte of the buffer with resample_restate."""
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
        assert RR.frame(k, host[i], W, H, crop, fmt, want[lead + i * stride:], ow, oh, **rp) == fb
    buf = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    dst = buf[lead:lead + n * stride].view(n, stride)
    table = out.frames_from([(k,) + tuple(addr[i]) for i, k in enumerate(kinds)])
    with out.resample_plan(ow, oh, roi, filter, **par) as plan:
        view = out.rgb_resampled(table, plan, dst=dst)
        dec.check()
    got = buf.cpu().numpy()
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        pytest.fail(f"fmt {fmt} {W}x{H} crop {crop} kinds {kinds} -> {ow}x{oh} roi {roi} filter {filter} align {align} lead {lead} "
                    f"gap {gap} {par}: {len(bad)} bytes differ, first at {bad[0] - lead} of frame stride {stride} "
                    f"(got {got[bad[0]]}, want {want[bad[0]]})")
    del pool
    return view


def _rois(lw, lh):
    """None; an odd origin and an odd size inside the crop; a region that touches the crop's last row and
    column."""
    x, y = min(1, lw - 1), min(1, lh - 1)
    w, h = max(1, (lw - x - 1) | 1), max(1, (lh - y - 1) | 1)
    w, h = min(w, lw - x), min(h, lh - y)
    tw, th = min(lw, 21), min(lh, 13)
    return [None, (x, y, w, h), (lw - tw, lh - th, tw, th)]


# ------------------------------------------------------------------------------ 1. directed small shapes
@pytest.mark.parametrize("W,H", [(1, 1), (3, 2), (11, 9)])
@pytest.mark.parametrize("fmt", [1, 2, 3, 0], ids=["420", "422", "444", "400"])
def test_directed_small_shapes(decs, fmt, W, H):
    """Every horizontal crop x every format x both chroma_up values, the filter and the other parameters
    drawn so that each of their values meets each filter (and each format where the format matters):
    kinds, matrices and ranges, bgr, pitch_align, the destination's offset, the frame count with permuted
    sources, the vertical crop (odd heights where the format has them), the region, the output size."""
    dec = decs[fmt]
    sw, sh = R.SUB[fmt]
    rng = np.random.default_rng(3000 * fmt + 16 * W + H)
    vcrops = _vcrops(H, sh)
    seen = set()
    job = 0
    for (l, r), format, up in [(c, f, u) for c in _hcrops(W, sw) for f in FORMATS for u in (R.REPLICATE, R.BILINEAR)]:
        filter = FILTERS[(job // 8 + job // 2 + job) % 3]         # crop + format + chroma_up: each pair of them meets
        t, b, fmo = vcrops[(job // 2) % len(vcrops)]
        crop = OUT.Crop(l, r, t, b, frame_mbs_only=fmo)
        lw, lh = OUT.geometry(W, H, crop, fmt).luma[2:]
        field_ok = H % 2 == 0                                     # a field picture has half the frame's MB rows
        n = (1, 2, 5)[(job // 2) % 3]
        kinds = [KINDS[(job // 2 + 3 * i) % 4] if field_ok else OUT.OUT_FRAME for i in range(n)]
        matrix, fr = ROWS[(job // 3) % 6]
        bgr = (job // 5) % 2
        align = (0, 64)[(job // 7) % 2]
        f16 = format == R.PLANAR_F16
        lead = (0, 2)[(job // 8) % 2] if f16 else (0, 1, 5)[(job // 8) % 3]
        gap = (0, 38, 48)[(job // 4) % 3] if f16 else (0, 37, 48)[(job // 4) % 3]
        rois = _rois(lw, lh)
        roi = rois[(job // 2 + job // 6) % 3]
        ow, oh = WIDTHS[(job // 3) % 7], HEIGHTS[(job // 3 + job // 21) % 7]
        while not _supported(lw, lh, roi, ow, oh, filter):       # 176 -> 1 is beyond every filter: the next size up
            ow, oh = WIDTHS[(WIDTHS.index(ow) + 1) % 7], HEIGHTS[(HEIGHTS.index(oh) + 1) % 7]
        host = [_sources(k, W, H, fmt, (job // 2 + i) % 3, rng) for i, k in enumerate(kinds)]
        par = dict(format=format, chroma_up=up, matrix=matrix, full_range=fr, bgr=bgr, alpha=(255, 0, 0x5A)[job % 3])
        par.update((UNIT, IMAGENET)[(job // 8) % 2] if f16 else {})
        _job(dec, fmt, W, H, crop, kinds, host, lead, gap, align, ow, oh, roi, filter, **par)
        seen |= {("kind", filter, k) for k in kinds} | {("row", matrix, fr), ("bgr", format, bgr), ("align", format, align),
                                                        ("lead", format, lead), ("n", n), ("fmt", filter, format),
                                                        ("roi", filter, rois.index(roi)), ("up", filter, up), ("lw", lw % 16),
                                                        ("lh", lh % 2)}
        job += 1
    assert {x[1:] for x in seen if x[0] == "row"} == set(ROWS)
    assert {x[1] for x in seen if x[0] == "n"} == {1, 2, 5}
    assert {x[1] for x in seen if x[0] == "lw"} >= {0, 2, 14}
    assert {x[1] for x in seen if x[0] == "lh"} == ({0} if sh == 2 else {0, 1})
    for format in FORMATS:
        assert {x[2] for x in seen if x[:2] == ("bgr", format)} == {0, 1}
        assert {x[2] for x in seen if x[:2] == ("align", format)} == {0, 64}
        assert {x[2] for x in seen if x[:2] == ("lead", format)} == ({0, 2} if format == R.PLANAR_F16 else {0, 1, 5})
    for filter in FILTERS:
        assert {x[2] for x in seen if x[:2] == ("fmt", filter)} == set(FORMATS)
        assert {x[2] for x in seen if x[:2] == ("roi", filter)} == {0, 1, 2}
        assert {x[2] for x in seen if x[:2] == ("up", filter)} == {R.REPLICATE, R.BILINEAR}
        if H % 2 == 0:
            assert {x[2] for x in seen if x[:2] == ("kind", filter)} == set(KINDS)


@pytest.mark.parametrize("fmt", [1, 2, 3, 0], ids=["420", "422", "444", "400"])
def test_every_kind_under_a_matrix_row_and_gbr(decs, fmt):
    """3 x 2 MBs: all four kinds in one job; one (matrix, range) row per format under every filter and
    both chroma_up values, and GBR on 4:4:4."""
    dec = decs[fmt]
    rng = np.random.default_rng(277 + fmt)
    W, H = 3, 2
    crop = OUT.Crop(1, 2, 1, 0, frame_mbs_only=0)
    rows = [ROWS[(2 * fmt + 1) % 6]] + ([(R.GBR, 0)] if fmt == 3 else [])
    for j, ((matrix, fr), up, filter) in enumerate((row, up, f) for row in rows for up in (R.REPLICATE, R.BILINEAR) for f in FILTERS):
        kinds = KINDS[j % 4:] + KINDS[:j % 4]
        host = [_sources(k, W, H, fmt, (i + j) % 3, rng) for i, k in enumerate(kinds)]
        _job(dec, fmt, W, H, crop, kinds, host, 0, 16, 64, (17, 33, 7, 16)[j % 4], (7, 16, 33, 3)[j % 4], (None, (3, 5, 21, 9))[j % 2],
             filter, format=FORMATS[j % 4], chroma_up=up, matrix=matrix, full_range=fr, bgr=j % 2, **IMAGENET)


# ------------------------------------------------------------------------------ 2. ratios and tiles
@pytest.mark.parametrize("filter", FILTERS, ids=["triangle", "bicubic", "lanczos"])
@pytest.mark.parametrize("fmt", [1, 3], ids=["420", "444"])
def test_named_ratios(decs, fmt, filter):
    """On 176 x 144 (11 x 9 MBs): identity, 2 : 1, the non-integer 176 x 144 -> 50 x 37, an upscale of a
    16 x 16 region to 45 x 50, down on one axis and up on the other, the largest window the filters share
    (176 x 144 -> 11 x 9: scale 16, LANCZOS ksize 97), and 1 x 1 at each filter's own largest scale."""
    dec = decs[fmt]
    rng = np.random.default_rng(31 + fmt)
    W, H = 11, 9
    host = [_sources(OUT.OUT_FRAME, W, H, fmt, what, rng) for what in (2, 0)]
    top = {RR.TRIANGLE: 48, RR.BICUBIC: 24, RR.LANCZOS: 16}[filter]
    cases = [(None, 176, 144), ((2, 1, 33, 17), 33, 17), (None, 88, 72), ((3, 1, 34, 14), 17, 7), (None, 50, 37),
             ((80, 64, 16, 16), 45, 50), (None, 50, 200), ((5, 3, 160, 21), 20, 63), (None, 11, 9), ((7, 5, top, top), 1, 1),
             ((0, 0, 16, 144), 1, 9)]
    assert RR.ksize_of(RR.LANCZOS, 0, 176, 11) == RR.MAX_TAPS and RR.ksize_of(filter, 7, 7 + top, 1) == RR.MAX_TAPS
    for j, (roi, ow, oh) in enumerate(cases):
        _job(dec, fmt, W, H, OUT.Crop(), [OUT.OUT_FRAME] * 2, host, 0, 0, 0, ow, oh, roi, filter, format=R.PLANAR_U8,
             chroma_up=j % 2, matrix=ROWS[j % 6][0], full_range=ROWS[j % 6][1])


@pytest.mark.parametrize("fmt", [1, 0], ids=["420", "400"])
def test_upscale_of_a_whole_small_picture(decs, fmt):
    """16 x 16 (one MB) -> 45 x 50 and -> 1 x 1: every window clamps at both ends of the crop."""
    dec = decs[fmt]
    rng = np.random.default_rng(37 + fmt)
    host = [_sources(OUT.OUT_FRAME, 1, 1, fmt, 2, rng)]
    for j, filter in enumerate(FILTERS):
        for ow, oh in ((45, 50), (1, 1), (16, 16)):
            _job(dec, fmt, 1, 1, OUT.Crop(), [OUT.OUT_FRAME], host, 0, 0, 0, ow, oh, None, filter, format=FORMATS[j], chroma_up=1)


@pytest.mark.parametrize("filter", FILTERS, ids=["triangle", "bicubic", "lanczos"])
def test_output_sizes_around_the_tile(decs, filter):
    """One below, at and one above RESAMPLE_TILE_W and RESAMPLE_TILE_H, on both axes at once, and two tiles
    and three pixels: the last tile's columns and rows repeat the frame's last, and none of them is written."""
    dec = decs[1]
    rng = np.random.default_rng(43)
    W, H = 3, 2
    host = [_sources(OUT.OUT_FRAME, W, H, 1, 2, rng)]
    sizes = [(w, h) for w in (TW - 1, TW, TW + 1) for h in (TH - 1, TH, TH + 1)] + [(2 * TW + 1, 2 * TH + 1), (2 * TW, 3), (3, 2 * TH)]
    for j, (ow, oh) in enumerate(sizes):
        _job(dec, 1, W, H, OUT.Crop(1, 0, 0, 1), [OUT.OUT_FRAME], host, (0, 1, 5)[j % 3], 0, (0, 64)[j % 2], ow, oh, None, filter,
             format=FORMATS[j % 3], chroma_up=j % 2)


def test_widest_windows_fill_the_lds(decs):
    """832 x 832 (52 x 52 MBs, 4:2:0) to 17 x 17 at each filter's largest scale, from a region at an odd
    column: full tiles of H264R_RESAMPLE_MAX_TAPS taps on both axes, the most LDS a workgroup takes (TRIANGLE
    at scale 48), two tiles on each axis."""
    dec = decs[1]
    rng = np.random.default_rng(47)
    W = H = 52
    host = [_sources(OUT.OUT_FRAME, W, H, 1, 2, rng)]
    for filter, s in ((RR.TRIANGLE, 48), (RR.BICUBIC, 24), (RR.LANCZOS, 16)):
        roi = (9, 5, 17 * s, 17 * s)
        assert RR.ksize_of(filter, 9, 9 + 17 * s, 17) == RR.MAX_TAPS
        _job(dec, 1, W, H, OUT.Crop(), [OUT.OUT_FRAME], host, 0, 0, 0, 17, 17, roi, filter, format=R.PLANAR_U8, chroma_up=1)


# ------------------------------------------------------------------------------ 3. what the definition is not
def test_the_clip_between_the_passes(decs):
    """resample_restate.MUTATION (0 / 255 blocks under BICUBIC): the restatement without the intermediate
    clip differs there (tests/test_output_resample.py), and the GPU gives the one with it.  A 4:0:0 context
    at full range copies the luma plane into all three channels."""
    dec = decs[0]
    m = RR.MUTATION
    W, H = m["w"] // 16, m["h"] // 16
    y = RR.blocks(m["h"], m["w"])
    c = R.channels(y, None, None, 0, R.BT709, 1)
    assert all(np.array_equal(p, y) for p in c)
    roi = (0, 0, m["w"], m["h"])
    with_clip = RR.resample(y, roi, m["out_w"], m["out_h"], m["filter"])
    without = RR.resample(y, roi, m["out_w"], m["out_h"], m["filter"], clip_between=False)
    assert not np.array_equal(with_clip, without)
    view = _job(dec, 0, W, H, OUT.Crop(), [OUT.OUT_FRAME], [[(y,)]], 0, 0, 0, m["out_w"], m["out_h"], None, m["filter"],
                format=R.PLANAR_U8, full_range=1)
    assert np.array_equal(view[0, 0].cpu().numpy(), with_clip)


@pytest.mark.parametrize("filter", FILTERS, ids=["triangle", "bicubic", "lanczos"])
def test_a_region_reads_the_real_samples_around_it(decs, filter):
    """A region inside the crop, in a plane that is noise outside the crop too: the windows reach past the
    region into the crop's real samples (Pillow's box=), which is not crop(box).resize() -- the two
    restatements differ on this case, and the GPU gives the first."""
    dec = decs[1]
    rng = np.random.default_rng(59)
    W, H, crop = 3, 2, OUT.Crop(2, 1, 1, 1)
    host = [_sources(OUT.OUT_FRAME, W, H, 1, 2, rng)]
    roi, ow, oh = (11, 7, 20, 12), 9, 5
    view = _job(dec, 1, W, H, crop, [OUT.OUT_FRAME], host, 0, 0, 0, ow, oh, roi, filter, format=R.PLANAR_U8, chroma_up=1)
    c = R.channels(*R.source_frame(host[0][0], W, H, crop, 1), 1, R.BT709, 0, R.BILINEAR, False)
    box = RR.resampled(c, ow, oh, roi, filter)
    cropped = RR.resampled(c, ow, oh, roi, filter, clamp_to_region=True)
    assert not all(np.array_equal(a, b) for a, b in zip(box, cropped))
    assert np.array_equal(view[0].cpu().numpy(), np.stack(box))
    # and what lies outside the CROP does not matter: other noise there, the same bytes
    other = [tuple(p.copy() for p in host[0][0])]
    g = OUT.geometry(W, H, crop, 1)
    for p, (x0, y0, w, h) in zip(other[0], (g.luma, g.chroma, g.chroma)):
        keep = p[y0:y0 + h, x0:x0 + w].copy()
        p[:] = rng.integers(0, 256, p.shape, dtype=np.uint8)
        p[y0:y0 + h, x0:x0 + w] = keep
    again = _job(dec, 1, W, H, crop, [OUT.OUT_FRAME], [other], 0, 0, 0, ow, oh, roi, filter, format=R.PLANAR_U8, chroma_up=1)
    assert np.array_equal(again.cpu().numpy(), view.cpu().numpy())


# ------------------------------------------------------------------------------ 4. against the existing stage
@pytest.mark.parametrize("fmt", [1, 2, 3, 0], ids=["420", "422", "444", "400"])
def test_frame_batch_from_decoder(L, decs, fmt):
    """A decoded frame batch: the resampled job reads the batch's own out planes on the same stream, and
    its bytes are the restatement of what h264r_output_frames writes for the same table."""
    dec = decs[fmt]
    over = {} if fmt == 1 else dict(chroma_format={2: 2, 3: 3, 0: A.SYNTH_CHROMA_400}[fmt])
    db = _decode(L, dec, [synth.default_cfg(L, 3, 11, 9, **over)], 3)
    W, H, crop = 11, 9, OUT.Crop(1, 2, 1, 3)
    t = db.tensors
    out = OUT.DeviceOutput(dec, W, H, crop)
    table = out.frames_from([(OUT.OUT_FRAME, (t["out_y"][i], t["out_u"][i] if fmt else None, t["out_v"][i] if fmt else None))
                             for i in (2, 0, 1)])
    yuv = OUT.DeviceOutput(dec, W, H, crop, fake_chroma=fmt == 0).run(table)
    dec.check()
    yuv = yuv.cpu().numpy()
    lw, lh = OUT.geometry(W, H, crop, fmt).luma[2:]
    for j, (format, filter) in enumerate((f, s) for f in FORMATS for s in FILTERS):
        par = dict(matrix=ROWS[j % 6][0], full_range=ROWS[j % 6][1], bgr=j % 2)
        up = j % 2
        ow, oh = (33, 17, 16, 50)[j % 4], (17, 33, 37, 16)[(j // 4) % 4]
        roi = (None, (lw - 41, lh - 33, 41, 33))[(j // 2) % 2]
        with out.resample_plan(ow, oh, roi, filter, format=format, chroma_up=up, **par, **IMAGENET) as plan:
            got = out.rgb_resampled(table, plan)
            dec.check()
        raw = got.cpu().numpy()
        for k in range(table.n):
            c = R.channels(*_split_planar(yuv[k], W, H, crop, fmt), fmt, par["matrix"], par["full_range"], up, par["bgr"])
            want = np.zeros(R.layout(ow, oh, format, 0)[2], np.uint8)
            R.write_frame(want, RR.resampled(c, ow, oh, roi, filter), format, 0, 255, IMAGENET["scale"], IMAGENET["bias"])
            g = np.ascontiguousarray(raw[k])
            assert np.array_equal(g.view(np.uint8).reshape(-1), want), f"frame {k} format {format} filter {filter}"


# ------------------------------------------------------------------------------ 5. plans
def test_one_plan_two_calls_two_streams(decs):
    """One plan, two calls on two streams of the caller's, two destinations: the same bytes, the restatement's."""
    import torch
    dec = decs[1]
    rng = np.random.default_rng(61)
    W, H, crop = 3, 2, OUT.Crop(0, 1, 0, 0)
    host = [_sources(OUT.OUT_FRAME, W, H, 1, 2, rng) for _ in range(3)]
    pool, addr = _upload(host)
    out = OUT.DeviceOutput(dec, W, H, crop)
    table = out.frames_from([(OUT.OUT_FRAME,) + tuple(addr[i]) for i in range(3)])
    ow, oh = 21, 13
    fb = R.layout(ow, oh, R.PACKED_U8, 0)[2]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with out.resample_plan(ow, oh, None, RR.LANCZOS, format=R.PACKED_U8) as plan:
        a = torch.full((3, fb), FILL, dtype=torch.uint8, device="cuda")
        b = torch.full((3, fb), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        out.rgb_resampled(table, plan, dst=a, stream=s1.cuda_stream)
        out.rgb_resampled(table, plan, dst=b, stream=s2.cuda_stream)
        s1.synchronize()
        s2.synchronize()
        dec.check()
    want = np.zeros((3, fb), np.uint8)
    for i in range(3):
        RR.frame(OUT.OUT_FRAME, host[i], W, H, crop, 1, want[i], ow, oh, filter=RR.LANCZOS, format=R.PACKED_U8)
    assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), want)
    assert plan.handle is None
    with pytest.raises(ValueError):
        out.rgb_resampled(table, plan)                            # a closed plan
    with pytest.raises(ValueError):
        out.rgb_resampled(table.tensor.data_ptr(), out.resample_plan(3, 2))   # a raw table needs its count
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
    for format, up, filter in ((R.PACKED_U8, R.BILINEAR, RR.BICUBIC), (R.PLANAR_F16, R.REPLICATE, RR.TRIANGLE)):
        rp = dict(format=format, up=up, filter=filter)
        fb = R.layout(ow, oh, format, 0)[2]
        good_frame, good_pair = np.zeros(fb, np.uint8), np.zeros(fb, np.uint8)
        assert RR.frame(OUT.OUT_FRAME, hfrm, W, H, crop, 1, good_frame, ow, oh, **rp) == fb
        RR.frame(OUT.OUT_FIELD_PAIR, hfld, W, H, crop, 1, good_pair, ow, oh, **rp)
        untouched = np.full(fb, FILL, np.uint8)
        jobs = [
            ([(OUT.OUT_FRAME, frm), (9, frm), (OUT.OUT_FIELD_PAIR, fld[0], fld[1])], [good_frame, untouched, good_pair]),
            ([(OUT.OUT_FIELD_PAIR, fld[0], (None, fld[1][1], fld[1][2])), (OUT.OUT_FRAME, frm)], [untouched, good_frame]),
            ([(OUT.OUT_FIELD_PAIR, fld[0], (fld[1][0], fld[1][1], None)), (OUT.OUT_FRAME, frm)], [untouched, good_frame]),
            ([(-1, frm), (OUT.OUT_FRAME, (frm[0], None, frm[2])), (OUT.OUT_UNPAIRED_BOT, (None, fld[0][1], fld[0][2]))],
             [untouched] * 3),
        ]
        with out.resample_plan(ow, oh, None, filter, format=format, chroma_up=up) as plan:
            for rows, wants in jobs:
                dst = torch.full((len(rows), fb), FILL, dtype=torch.uint8, device="cuda")
                out.rgb_resampled(out.frames_from(rows), plan, dst=dst)
                with pytest.raises(h264r.H264RError) as e:
                    dec.check()
                assert e.value.status == A.EDEVICE
                got = dst.cpu().numpy()
                for i, w in enumerate(wants):
                    assert np.array_equal(got[i], w), f"frame {i} of {[r[0] for r in rows]}"
                # the error word is cleared by the report: a good job after it passes
                dst = torch.full((2, fb), FILL, dtype=torch.uint8, device="cuda")
                out.rgb_resampled(out.frames_from([(OUT.OUT_FIELD_PAIR, fld[0], fld[1]), (OUT.OUT_FRAME, frm)]), plan, dst=dst)
                dec.check()
                got = dst.cpu().numpy()
                assert np.array_equal(got[0], good_pair) and np.array_equal(got[1], good_frame)


def test_host_refusals_on_a_context(decs):
    import torch
    dec = decs[1]
    out = OUT.DeviceOutput(dec, 3, 2)
    y = torch.zeros(32 * 48, dtype=torch.uint8, device="cuda")
    table = out.frames_from([(OUT.OUT_FRAME, (y, y, y))])
    Lb = dec._L
    call = lambda ctx, plan, tab, n, d, stride: Lb.h264r_output_rgb_resampled(ctx, plan, tab, n, d, stride, None)
    tp = table.tensor.data_ptr()
    for format in FORMATS:
        with out.resample_plan(17, 7, format=format) as plan:
            fb = plan.geom.frame_bytes
            assert fb == R.layout(17, 7, format, 0)[2]
            dst = torch.zeros(fb + 16, dtype=torch.uint8, device="cuda")
            dp = dst.data_ptr()
            h, ph = dec.handle, plan.handle
            assert call(h, ph, tp, 1, dp, fb - 1) == A.EINVAL            # frames would overlap
            assert call(h, ph, None, 1, dp, fb) == A.EINVAL and call(h, ph, tp, 1, None, fb) == A.EINVAL
            assert call(h, ph, tp, -1, dp, fb) == A.EINVAL
            assert call(h, None, tp, 1, dp, fb) == A.EINVAL and call(None, ph, tp, 1, dp, fb) == A.EINVAL
            assert call(decs[0].handle, ph, tp, 1, dp, fb) == A.EINVAL   # a plan belongs to its context
            assert call(h, ph, tp, 0, dp, fb) == A.OK                    # nothing to do
            odd = A.EINVAL if format == R.PLANAR_F16 else A.OK           # binary16 wants even addresses
            assert call(h, ph, tp, 1, dp + 1, fb) == odd and call(h, ph, tp, 1, dp, fb + 1) == odd
            assert call(h, ph, tp, 1, dp, fb) == A.OK
            dec.check()
    # creation refuses what the geometry refuses, and leaves no plan behind
    rgb = OUT.rgb_desc(out.desc)
    create = lambda d: Lb.h264r_resample_plan_create(dec.handle, C.byref(d), C.byref(hp))
    hp = C.c_void_p(1)
    assert create(OUT.resample_desc(rgb, 17, 7, roi=(0, 0, 49, 32))) == A.EINVAL and hp.value is None
    assert create(OUT.resample_desc(rgb, 17, 7, filter=3)) == A.EINVAL
    assert create(OUT.resample_desc(OUT.rgb_desc(out.desc, matrix=R.GBR), 17, 7)) == A.EUNSUPPORTED
    assert create(OUT.resample_desc(rgb, 1, 1, filter=RR.LANCZOS)) == A.EUNSUPPORTED        # 48 -> 1: ksize 289
    assert create(OUT.resample_desc(rgb, 1, 1, filter=RR.TRIANGLE)) == A.OK and hp.value   # 48 -> 1: ksize 97
    Lb.h264r_resample_plan_destroy(hp)
    Lb.h264r_resample_plan_destroy(None)
    assert Lb.h264r_resample_plan_create(dec.handle, None, C.byref(hp)) == A.EINVAL
    assert Lb.h264r_resample_plan_create(None, C.byref(OUT.resample_desc(rgb, 17, 7)), C.byref(hp)) == A.EINVAL
    assert Lb.h264r_resample_plan_create(dec.handle, C.byref(OUT.resample_desc(rgb, 17, 7)), None) == A.EINVAL
    dec.check()
