"""RGB frames on MI355X: h264r_output_rgb (include/h264r_output.h, k_output_rgb in k_output.hip).

Every comparison is byte-exact against tests/rgb_restate.py, the numpy restatement of the header's
definition; no expected byte comes from the library.  Destinations are prefilled with 0xA5 and compared
whole, so a byte written outside a frame's rows (pitch padding, the gap between frames, the bytes
around the buffer) fails like a wrong pixel.
"""
import os
import subprocess

import numpy as np
import pytest

import h264r
import rgb_restate as R
import streams as S
from h264r import _abi as A
from h264r import batch as B
from h264r import output as OUT
from h264r import synth

pytestmark = pytest.mark.gpu

GOLD = S.golden()["streams"]
FILL = 0xA5
KINDS = [OUT.OUT_FRAME, OUT.OUT_FIELD_PAIR, OUT.OUT_UNPAIRED_TOP, OUT.OUT_UNPAIRED_BOT]
FORMATS = [R.PACKED_U8, R.PACKED_U8X4, R.PLANAR_U8, R.PLANAR_F16]
ROWS = [(m, fr) for m in (R.BT601, R.BT709, R.BT2020) for fr in (0, 1)]
IMAGENET = dict(scale=tuple(1 / (255 * s) for s in (0.229, 0.224, 0.225)),
                bias=tuple(-m / s for m, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))))
UNIT = dict(scale=(1 / 255,) * 3, bias=(0.0,) * 3)


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


# ------------------------------------------------------------------------------ plane contents
def _content(h, w, sw, sh, plane, what, rng):
    """One plane (plane 0 luma of h x w, 1 / 2 chroma subsampled by sw, sh).  what 0: 4 x 4 luma blocks
    running through all eight (Y, Cb, Cr) triples of 0 / 255 -- every channel clips both ways under every
    matrix; 1: ramps whose neighbours differ in both directions, so that every pair of bilinear taps
    and weights gives its own value; 2: random."""
    y, x = np.mgrid[0:h, 0:w]
    if what == 0:
        if plane:
            y, x = y * sh, x * sw
        idx = (x // 4 + 3 * (y // 4)) % 8
        return (255 * ((idx >> plane) & 1)).astype(np.uint8)
    if what == 1:
        a, b, c = ((1, 3, 0), (7, 31, 40), (13, 53, 100))[plane]
        return ((a * x + b * y + c) & 255).astype(np.uint8)
    return rng.integers(0, 256, (h, w), dtype=np.uint8)


def _sources(kind, W, H, fmt, what, rng):
    """Host planes of the sources one frame of `kind` needs: [(y, u, v)] or two of them for a field pair."""
    cw, ch = A.chroma_mb(fmt)
    sw, sh = R.SUB[fmt]
    fld = 0 if kind == OUT.OUT_FRAME else 1
    srcs = []
    for s in range(2 if kind == OUT.OUT_FIELD_PAIR else 1):
        shapes = [(16 * H >> fld, 16 * W)] + ([(ch * H >> fld, cw * W)] * 2 if fmt else [])
        srcs.append(tuple(_content(h, w, sw, sh, p, (what + s) % 3, rng) for p, (h, w) in enumerate(shapes)))
    return srcs


def _upload(host):
    """The sources of a job back to back in one device buffer, in the REVERSE of output order; returns
    the pool (keep it alive) and the frame-table rows' plane addresses."""
    import torch
    flat, where = [], {}
    for i in reversed(range(len(host))):
        for s, planes in enumerate(host[i]):
            for p, a in enumerate(planes):
                where[(i, s, p)] = sum(x.size for x in flat)
                flat.append(a.reshape(-1))
    pool = torch.from_numpy(np.concatenate(flat)).cuda()
    base = pool.data_ptr()
    addr = [[tuple(base + where[(i, s, p)] if p < len(host[i][s]) else None for p in range(3)) for s in range(len(host[i]))]
            for i in range(len(host))]
    return pool, addr


def _job(dec, fmt, W, H, crop, kinds, host, lead, gap, align, **par):
    """Run one job into a 0xA5 buffer (frames `gap` bytes apart beyond their size, the first `lead` bytes
    off the allocation) and compare every byte of the buffer with rgb_restate."""
    import torch
    n = len(kinds)
    pool, addr = _upload(host)
    out = OUT.DeviceOutput(dec, W, H, crop, pitch_align=align)
    rp = dict(matrix=par.get("matrix", R.BT709), full_range=par.get("full_range", 0), up=par.get("chroma_up", R.REPLICATE),
              format=par["format"], bgr=par.get("bgr", 0), alpha=par.get("alpha", 255), scale=par.get("scale", UNIT["scale"]),
              bias=par.get("bias", UNIT["bias"]), align=align)
    lw, lh = OUT.geometry(W, H, crop, fmt).luma[2:]
    fb = R.layout(lw, lh, par["format"], align)[2]
    stride = fb + gap
    total = lead + n * stride + 64
    want = np.full(total, FILL, np.uint8)
    for i, k in enumerate(kinds):
        assert R.frame(k, host[i], W, H, crop, fmt, want[lead + i * stride:], **rp) == fb
    buf = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    dst = buf[lead:lead + n * stride].view(n, stride)
    table = out.frames_from([(k,) + tuple(addr[i]) for i, k in enumerate(kinds)])
    view = out.rgb(table, dst=dst, **par)
    dec.check()
    got = buf.cpu().numpy()
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        pytest.fail(f"fmt {fmt} {W}x{H} crop {crop} kinds {kinds} align {align} lead {lead} gap {gap} {par}: {len(bad)} bytes "
                    f"differ, first at {bad[0] - lead} of frame stride {stride} (got {got[bad[0]]}, want {want[bad[0]]})")
    del pool
    return view


# ------------------------------------------------------------------------------ 1. directed small shapes
# (left, right) for a width of W MBs: lw mod 16 on 0, 2, 14 (and 1, 15 where CropUnitX is 1), and the
# narrowest picture: lw = 2 (1), where both horizontal taps clamp to the same sample
def _hcrops(W, unit):
    if unit == 2:
        return [(0, 0), (3, 4), (1, 0), (8 * W - 1, 0), (2, 8 * W - 3)]
    return [(0, 0), (3, 12), (14, 0), (1, 1), (0, 1), (5, 16 * W - 6), (16 * W - 2, 0)]


# (top, bottom, frame_mbs_only) for a height of H MBs by SubHeightC: lh even and, where the format
# allows, odd; the lowest picture the format has (lh = 1, or 2 in 4:2:0) -- both vertical taps clamp
def _vcrops(H, sub_h):
    if sub_h == 2:
        return [(0, 0, 1), (1, 0, 1), (0, 1, 0), (1, 1, 0), (8 * H - 1, 0, 1), (2, 8 * H - 3, 1)]
    return [(0, 0, 1), (1, 0, 1), (0, 1, 0), (2, 1, 1), (16 * H - 1, 0, 1), (3, 16 * H - 4, 1)]


def test_crop_lists_cover_what_they_claim():
    for W in (1, 3, 11):
        for unit, want in ((2, {0, 2, 14}), (1, {0, 1, 2, 14, 15})):
            lws = [16 * W - unit * (l + r) for l, r in _hcrops(W, unit)]
            assert all(x > 0 for x in lws) and {x % 16 for x in lws} >= want and min(lws) == unit
    for H in (1, 2, 9):
        for sub_h in (2, 1):
            lhs = [16 * H - sub_h * (2 - fmo) * (t + b) for t, b, fmo in _vcrops(H, sub_h)]
            assert all(x > 0 for x in lhs) and min(lhs) == sub_h and (sub_h == 2 or any(x % 2 for x in lhs))


@pytest.mark.parametrize("W,H", [(1, 1), (3, 2), (11, 9)])
@pytest.mark.parametrize("fmt", [1, 2, 3, 0], ids=["420", "422", "444", "400"])
def test_directed_small_shapes(decs, fmt, W, H):
    """Every horizontal crop x every format x both chroma_up values, the other parameters drawn so that
    each of their values meets each format: kinds, matrices and ranges, bgr, pitch_align, the
    destination's offset, the frame count, the vertical crop, the plane contents."""
    dec = decs[fmt]
    sw, sh = R.SUB[fmt]
    rng = np.random.default_rng(1000 * fmt + 16 * W + H)
    vcrops = _vcrops(H, sh)
    seen = set()
    job = 0
    for (l, r), format, up in [(c, f, u) for c in _hcrops(W, sw) for f in FORMATS for u in (R.REPLICATE, R.BILINEAR)]:
        t, b, fmo = vcrops[(job // 2) % len(vcrops)]
        field_ok = H % 2 == 0                                     # a field picture has half the frame's MB rows
        n = (1, 2, 5)[job % 3]
        kinds = [KINDS[(job + 3 * i) % 4] if field_ok else OUT.OUT_FRAME for i in range(n)]
        matrix, fr = ROWS[(job // 3) % 6]
        bgr = (job // 5) % 2
        align = (0, 64)[(job // 7) % 2]
        f16 = format == R.PLANAR_F16
        lead = (0, 2)[(job // 8) % 2] if f16 else (0, 1, 5, 15)[(job // 8) % 4]
        gap = (0, 38, 48)[(job // 2) % 3] if f16 else (0, 37, 48)[(job // 2) % 3]
        host = [_sources(k, W, H, fmt, (job + i) % 3, rng) for i, k in enumerate(kinds)]
        par = dict(format=format, chroma_up=up, matrix=matrix, full_range=fr, bgr=bgr, alpha=(255, 0, 0x5A)[job % 3])
        par.update((UNIT, IMAGENET)[(job // 4) % 2] if f16 else {})
        _job(dec, fmt, W, H, OUT.Crop(l, r, t, b, frame_mbs_only=fmo), kinds, host, lead, gap, align, **par)
        seen |= {("kind", format, k) for k in kinds} | {("row", matrix, fr), ("bgr", format, bgr), ("align", format, align),
                                                      ("lead", format, lead), ("n", n), ("v", up, (t, b, fmo))}
        job += 1
    assert {x[1:] for x in seen if x[0] == "row"} == set(ROWS)
    assert {x[1] for x in seen if x[0] == "n"} == {1, 2, 5}
    for format in FORMATS:
        assert {x[2] for x in seen if x[:2] == ("bgr", format)} == {0, 1}
        assert {x[2] for x in seen if x[:2] == ("align", format)} == {0, 64}
        assert {x[2] for x in seen if x[:2] == ("lead", format)} == ({0, 2} if format == R.PLANAR_F16 else {0, 1, 5, 15})
        if H % 2 == 0:
            assert {x[2] for x in seen if x[:2] == ("kind", format)} == set(KINDS)
    for up in (R.REPLICATE, R.BILINEAR):
        assert {x[2] for x in seen if x[:2] == ("v", up)} == set(vcrops)


@pytest.mark.parametrize("fmt", [1, 2, 3, 0], ids=["420", "422", "444", "400"])
def test_every_kind_under_every_matrix_row(decs, fmt):
    """3 x 2 MBs: all four kinds in one job, for every (matrix, range) row under both chroma_up values."""
    dec = decs[fmt]
    rng = np.random.default_rng(77 + fmt)
    W, H = 3, 2
    crop = OUT.Crop(1, 2, 1, 0, frame_mbs_only=0)
    for j, ((matrix, fr), up) in enumerate((row, up) for row in ROWS for up in (R.REPLICATE, R.BILINEAR)):
        kinds = KINDS[j % 4:] + KINDS[:j % 4]
        host = [_sources(k, W, H, fmt, (i + j) % 3, rng) for i, k in enumerate(kinds)]
        _job(dec, fmt, W, H, crop, kinds, host, 0, 16, 64, format=FORMATS[j % 3], chroma_up=up, matrix=matrix, full_range=fr,
             bgr=j % 2)


def test_gbr_copies_the_planes_of_444(decs):
    dec = decs[3]
    rng = np.random.default_rng(9)
    for j, ((W, H), (l, r)) in enumerate([((1, 1), (0, 0)), ((1, 1), (15, 0)), ((3, 2), (3, 12)), ((3, 2), (0, 1)), ((11, 9), (1, 1))]):
        kinds = [KINDS[(j + i) % 4] if H % 2 == 0 else OUT.OUT_FRAME for i in range(3)]
        host = [_sources(k, W, H, 3, 2, rng) for k in kinds]
        par = dict(format=FORMATS[j % 4], matrix=R.GBR, full_range=j % 2, chroma_up=(j // 2) % 2, bgr=(j // 2) % 2)
        par.update(IMAGENET if par["format"] == R.PLANAR_F16 else {})
        view = _job(dec, 3, W, H, OUT.Crop(l, r, 1, 2), kinds, host, 0, 0, 0, **par)
        if par["format"] == R.PLANAR_U8 and kinds[0] == OUT.OUT_FRAME:      # G = Y, B = Cb, R = Cr, as they are
            y, u, v = (a[1:16 * H - 2, l:16 * W - r] for a in host[0][0])
            got = view[0].cpu().numpy()
            want = (u, y, v) if par["bgr"] else (v, y, u)
            assert all(np.array_equal(got[k], want[k]) for k in range(3))


# ------------------------------------------------------------------------------ 2. against the existing stage
def _decode(L, dec, cfgs, n):
    """n pictures of every cfg as one batch; returns the DeviceBatch (its out planes stay on the device)."""
    pics = [synth.picture(L, cfg, i) for cfg in cfgs for i in range(n)]
    for s, (y, u, v) in enumerate(synth.refpics(L, cfgs[0])):
        dec.set_ref(s, y, u, v)
    db = B.to_device(B.pack(pics, h264r.quant_flat()), len(pics), None)
    dec.decode_batch(db.batch)
    return db


def _split_planar(frame, W, H, crop, fmt):
    """Y, Cb, Cr out of one planar frame of h264r_output_frames (rows contiguous)."""
    g = OUT.geometry(W, H, crop, fmt)
    lw, lh = g.luma[2:]
    if not fmt:
        return frame[:lw * lh].reshape(lh, lw), None, None
    cw, ch = g.chroma[2:]
    return (frame[:lw * lh].reshape(lh, lw), frame[lw * lh:lw * lh + cw * ch].reshape(ch, cw),
            frame[lw * lh + cw * ch:lw * lh + 2 * cw * ch].reshape(ch, cw))


def _rgb_equals_restated_yuv(dec, table, W, H, crop, fmt):
    """h264r_output_frames planar on the table, rgb_restate on those bytes == h264r_output_rgb on the table."""
    yuv = OUT.DeviceOutput(dec, W, H, crop, fake_chroma=fmt == 0).run(table)
    out = OUT.DeviceOutput(dec, W, H, crop)
    dec.check()
    yuv = yuv.cpu().numpy()
    for j, (format, up) in enumerate((f, u) for f in FORMATS for u in (R.REPLICATE, R.BILINEAR)):
        par = dict(matrix=ROWS[j % 6][0], full_range=ROWS[j % 6][1], bgr=j % 2)
        got = out.rgb(table, format=format, chroma_up=up, **par, **IMAGENET)
        dec.check()
        raw = got.cpu().numpy()
        for k in range(table.n):
            c = R.channels(*_split_planar(yuv[k], W, H, crop, fmt), fmt, par["matrix"], par["full_range"], up, par["bgr"])
            want = np.zeros(R.layout(c[0].shape[1], c[0].shape[0], format, 0)[2], np.uint8)
            R.write_frame(want, c, format, 0, 255, IMAGENET["scale"], IMAGENET["bias"])
            g = np.ascontiguousarray(raw[k])
            assert np.array_equal(g.view(np.uint8).reshape(-1), want), f"frame {k} format {format} chroma_up {up}"


@pytest.mark.parametrize("fmt", [1, 2, 3, 0], ids=["420", "422", "444", "400"])
def test_frame_batch_from_decoder(L, decs, fmt):
    """A decoded frame batch: the RGB job reads the batch's own out planes on the same stream."""
    dec = decs[fmt]
    over = {} if fmt == 1 else dict(chroma_format={2: 2, 3: 3, 0: A.SYNTH_CHROMA_400}[fmt])
    db = _decode(L, dec, [synth.default_cfg(L, 3, 11, 9, **over)], 3)
    crop = OUT.Crop(1, 2, 1, 3)
    t = db.tensors
    out = OUT.DeviceOutput(dec, 11, 9, crop)
    table = out.frames_from([(OUT.OUT_FRAME, (t["out_y"][i], t["out_u"][i] if fmt else None, t["out_v"][i] if fmt else None))
                             for i in (2, 0, 1)])
    _rgb_equals_restated_yuv(dec, table, 11, 9, crop, fmt)


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
    _rgb_equals_restated_yuv(dec, table, 11, 8, crop, 1)


# ------------------------------------------------------------------------------ 3. binary16
@pytest.mark.parametrize("norm", [UNIT, IMAGENET], ids=["unit", "imagenet"])
def test_f16_is_numpys_float32_pipeline(decs, norm):
    """Every 8-bit value in every channel: the tensor's bits are those of
    float16(float32(v) * float32(scale) + float32(bias))."""
    import torch
    dec = decs[3]
    W, H = 1, 1
    planes = [np.arange(256, dtype=np.uint8).reshape(16, 16), np.arange(256, dtype=np.uint8).reshape(16, 16).T.copy(),
              np.arange(255, -1, -1, dtype=np.uint8).reshape(16, 16)]
    dev = tuple(torch.from_numpy(p).cuda() for p in planes)
    out = OUT.DeviceOutput(dec, W, H)
    table = out.frames_from([(OUT.OUT_FRAME, dev)])
    for matrix, bgr in ((R.GBR, 0), (R.GBR, 1), (R.BT601, 0)):
        got = out.rgb(table, format=R.PLANAR_F16, matrix=matrix, bgr=bgr, **norm)
        dec.check()
        assert got.dtype == torch.float16 and tuple(got.shape) == (1, 3, 16, 16)
        c = R.channels(*planes, 3, matrix, 0, R.REPLICATE, bgr)
        bits = got.cpu().numpy().view(np.uint16)
        for k in range(3):
            want = (c[k].astype(np.float32) * np.float32(norm["scale"][k]) + np.float32(norm["bias"][k])).astype(np.float16)
            assert np.array_equal(bits[0, k], want.view(np.uint16)), (matrix, bgr, k)
            assert matrix != R.GBR or set(c[k].reshape(-1).tolist()) == set(range(256))


# ------------------------------------------------------------------------------ 4. the torch wrapper
@pytest.mark.parametrize("align", [0, 64])
@pytest.mark.parametrize("fmt", [1, 0], ids=["420", "400"])
def test_wrapper_views(decs, fmt, align):
    import torch
    dec = decs[fmt]
    W, H, crop, n = 3, 2, OUT.Crop(3, 4 if fmt else 3, 1, 0), 2
    rng = np.random.default_rng(3)
    host = [_sources(OUT.OUT_FRAME, W, H, fmt, 2, rng) for _ in range(n)]
    pool, addr = _upload(host)
    out = OUT.DeviceOutput(dec, W, H, crop, pitch_align=align)
    table = out.frames_from([(OUT.OUT_FRAME,) + tuple(addr[i]) for i in range(n)])
    lw, lh = OUT.geometry(W, H, crop, fmt).luma[2:]
    assert lw % 16 and lw * 2 % 64
    for format in FORMATS:
        t = out.rgb(table, format=format, bgr=True, alpha=7)
        dec.check()
        pitch = R.pitch_of(lw, format, align)
        fb = R.layout(lw, lh, format, align)[2]
        if format in (R.PACKED_U8, R.PACKED_U8X4):
            ch = 3 if format == R.PACKED_U8 else 4
            assert t.dtype == torch.uint8 and tuple(t.shape) == (n, lh, lw, ch) and t.stride() == (fb, pitch, ch, 1)
        elif format == R.PLANAR_U8:
            assert t.dtype == torch.uint8 and tuple(t.shape) == (n, 3, lh, lw) and t.stride() == (fb, pitch * lh, pitch, 1)
        else:
            assert t.dtype == torch.float16 and tuple(t.shape) == (n, 3, lh, lw)
            assert t.stride() == (fb // 2, pitch * lh // 2, pitch // 2, 1)
        assert t.is_contiguous() == (align == 0)
        got = t.cpu().numpy()
        for i in range(n):
            c = R.channels(*R.source_frame(host[i][0], W, H, crop, fmt), fmt, R.BT709, 0, R.REPLICATE, True)
            if format in (R.PACKED_U8, R.PACKED_U8X4):
                px = list(c) + ([np.full_like(c[0], 7)] if format == R.PACKED_U8X4 else [])
                assert np.array_equal(got[i], np.stack(px, axis=2))
            elif format == R.PLANAR_U8:
                assert np.array_equal(got[i], np.stack(c))
            else:
                want = np.stack([R.half_bits(c[k], 1 / 255, 0) for k in range(3)])
                assert np.array_equal(got[i].view(np.uint16), want)
    # a raw table needs its count, a destination its shape
    with pytest.raises(ValueError):
        out.rgb(table.tensor.data_ptr())
    with pytest.raises(ValueError):
        out.rgb(table, dst=torch.zeros(4, dtype=torch.uint8, device="cuda"))
    del pool


# ------------------------------------------------------------------------------ 5. refusals
def test_refused_frames_are_skipped_and_reported(decs):
    """A kind outside 0..3 and a NULL plane the kind needs: the frame keeps its 0xA5, its neighbours are
    written, check() reports H264R_EDEVICE once, and the next good job passes.  The bad entries hold NULL
    or valid pointers only, and the kernel tests them before it uses any."""
    import torch
    dec = decs[1]
    W, H = 3, 2
    crop = OUT.Crop(1, 0, 0, 1)
    rng = np.random.default_rng(4)
    out = OUT.DeviceOutput(dec, W, H, crop)
    hfrm = _sources(OUT.OUT_FRAME, W, H, 1, 2, rng)
    hfld = _sources(OUT.OUT_FIELD_PAIR, W, H, 1, 1, rng)
    frm = tuple(torch.from_numpy(a).cuda() for a in hfrm[0])
    fld = [tuple(torch.from_numpy(a).cuda() for a in s) for s in hfld]
    for format, up in ((R.PACKED_U8, R.BILINEAR), (R.PLANAR_F16, R.REPLICATE)):
        rp = dict(format=format, up=up)
        fb = R.layout(*OUT.geometry(W, H, crop, 1).luma[2:], format, 0)[2]
        good_frame, good_pair = np.zeros(fb, np.uint8), np.zeros(fb, np.uint8)
        assert R.frame(OUT.OUT_FRAME, hfrm, W, H, crop, 1, good_frame, **rp) == fb
        R.frame(OUT.OUT_FIELD_PAIR, hfld, W, H, crop, 1, good_pair, **rp)
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
            out.rgb(out.frames_from(rows), dst=dst, format=format, chroma_up=up)
            with pytest.raises(h264r.H264RError) as e:
                dec.check()
            assert e.value.status == A.EDEVICE
            got = dst.cpu().numpy()
            for i, w in enumerate(wants):
                assert np.array_equal(got[i], w), f"frame {i} of {[r[0] for r in rows]}"
            # the error word is cleared by the report: a good job after it passes
            dst = torch.full((2, fb), FILL, dtype=torch.uint8, device="cuda")
            out.rgb(out.frames_from([(OUT.OUT_FIELD_PAIR, fld[0], fld[1]), (OUT.OUT_FRAME, frm)]), dst=dst, format=format,
                    chroma_up=up)
            dec.check()
            got = dst.cpu().numpy()
            assert np.array_equal(got[0], good_pair) and np.array_equal(got[1], good_frame)


def test_gbr_off_444_is_unsupported(decs):
    import torch
    y = torch.zeros(32 * 48, dtype=torch.uint8, device="cuda")
    for fmt in (0, 1, 2):
        out = OUT.DeviceOutput(decs[fmt], 3, 2)
        with pytest.raises(h264r.H264RError) as e:
            out.rgb(out.frames_from([(OUT.OUT_FRAME, (y, y, y))]), matrix=R.GBR)
        assert e.value.status == A.EUNSUPPORTED
        decs[fmt].check()


def test_400_context_never_reads_chroma(decs):
    """On a 4:0:0 context u / v are not even tested: NULL there is no refusal, and R = G = B."""
    import torch
    dec = decs[0]
    rng = np.random.default_rng(6)
    crop = OUT.Crop(3, 1, 2, 5)
    y = _content(32, 48, 1, 1, 0, 2, rng)
    out = OUT.DeviceOutput(dec, 3, 2, crop)
    got = out.rgb(out.frames_from([(OUT.OUT_FRAME, (torch.from_numpy(y).cuda(), None, None))]), format=R.PLANAR_U8,
                  chroma_up=R.BILINEAR, matrix=R.BT601)
    dec.check()
    got = got.cpu().numpy()[0]
    c = R.channels(*R.source_frame((y,), 3, 2, crop, 0), 0, R.BT601, 0, R.BILINEAR, 0)
    assert all(np.array_equal(got[k], c[k]) for k in range(3)) and np.array_equal(got[0], got[1]) and np.array_equal(got[1], got[2])


def test_host_argument_refusals(decs):
    import ctypes as C
    import torch
    dec = decs[1]
    out = OUT.DeviceOutput(dec, 3, 2)
    y = torch.zeros(32 * 48, dtype=torch.uint8, device="cuda")
    table = out.frames_from([(OUT.OUT_FRAME, (y, y, y))])
    call = lambda desc, tab, n, d, stride: dec._L.h264r_output_rgb(dec.handle, C.byref(desc) if desc is not None else None,
                                                                   tab, n, d, stride, None)
    tp = table.tensor.data_ptr()
    for format in FORMATS:
        desc = OUT.rgb_desc(out.desc, format=format)
        fb = OUT.rgb_geometry(desc, 1).frame_bytes
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
    bad = OUT.rgb_desc(OUT.OutDesc(3, 2, 0, 0, 0, 0, 1, OUT.SEMIPLANAR, 0, 0))
    assert call(bad, tp, 1, dp, fb) == A.EINVAL
    bad = OUT.rgb_desc(out.desc, alpha=256)
    assert call(bad, tp, 1, dp, fb) == A.EINVAL
    bad = OUT.rgb_desc(out.desc, scale=(float("nan"), 1, 1), format=R.PLANAR_F16)
    assert call(bad, tp, 1, dp, fb) == A.EINVAL
    dec.check()


# ------------------------------------------------------------------------------ 6. one committed stream end to end
GPU_DEC = os.path.join(S.ROOT, "arrow-h264_amd", "lib", "h264dec")


def test_stream_end_to_end(L, tmp_path):
    """hi422_cif_ibbp_slices (4:2:2, crop (1, 2, 3, 2)): the own parser through libh264r.so writes YUV
    frames at the reference's MD5s; those frames, put back into coded-size planes whose samples outside
    the crop are noise, go through one RGB job that must equal rgb_restate of the frames -- under
    bilinear too, where a sample outside the crop would show."""
    import torch
    name = "hi422_cif_ibbp_slices"
    cfg = S.STREAMS[name]
    assert os.path.exists(GPU_DEC), "arrow-h264_amd/lib/h264dec not built"
    yuv = tmp_path / "out.yuv"
    r = subprocess.run([GPU_DEC, "-i", S.stream_path(name), "-o", str(yuv)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-800:]
    assert OUT.digest_by_frames(str(yuv), cfg["frames"]) == GOLD[name]["frame_md5"]
    W, H, fmt, crop = cfg["width_mbs"], cfg["height_mbs"], cfg["chroma_format"], S.crop_of(cfg)
    assert (fmt, (crop.left, crop.right, crop.top, crop.bottom)) == (2, (1, 2, 3, 2))
    geom = OUT.geometry(W, H, crop, fmt)
    data = np.fromfile(str(yuv), np.uint8).reshape(cfg["frames"], geom.frame_bytes)
    rng = np.random.default_rng(8)
    cw, ch = A.chroma_mb(fmt)
    host = []
    for k in range(cfg["frames"]):
        planes = [rng.integers(0, 256, (16 * H, 16 * W), dtype=np.uint8), rng.integers(0, 256, (ch * H, cw * W), dtype=np.uint8),
                  rng.integers(0, 256, (ch * H, cw * W), dtype=np.uint8)]
        for p, part, (x0, y0, w, h) in zip(planes, _split_planar(data[k], W, H, crop, fmt), (geom.luma, geom.chroma, geom.chroma)):
            p[y0:y0 + h, x0:x0 + w] = part
        host.append([tuple(planes)])
    with h264r.Decoder(0, W, H, chroma_format=fmt) as dec:
        for j, (format, up) in enumerate([(R.PACKED_U8, R.BILINEAR), (R.PLANAR_F16, R.REPLICATE), (R.PACKED_U8X4, R.BILINEAR)]):
            _job(dec, fmt, W, H, crop, [OUT.OUT_FRAME] * len(host), host, 0, 0, (0, 64, 0)[j], format=format, chroma_up=up,
                 matrix=ROWS[j][0], full_range=ROWS[j][1], **IMAGENET)
