"""The device-side output stage on MI355X: h264r_output_frames (include/h264r_output.h, k_output.hip).

Expected bytes never come from the code under test: they are numpy's (h264r/output.py:frame_bytes and
geometry, pinned by tests/test_output.py, plus the weave rule of dpb_combine_field_yuv, picture.cc:578-622)
or the unmodified reference's per-frame MD5s of the committed streams (tests/golden/streams.json).
The unpaired-field kinds are pinned by the numpy definition alone (the other parity's rows are 128,
write_unpaired_field output.cc:229-263): the stream writer emits no unpaired field.
"""
import hashlib

import numpy as np
import pytest

import h264r
import streams as S
from h264r import _abi as A
from h264r import batch as B
from h264r import output as OUT
from h264r import synth

pytestmark = pytest.mark.gpu

GOLD = S.golden()["streams"]
FILL = 0xA5


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


# ------------------------------------------------------------------------------ numpy's output frame
def _woven(kind, srcs):
    """The coded-size frame planes of one output frame from its source pictures."""
    if kind == OUT.OUT_FRAME:
        return srcs[0]
    planes = []
    for k in range(len(srcs[0])):
        a = srcs[0][k]
        f = np.full((2 * a.shape[0], a.shape[1]), 128, np.uint8)
        if kind == OUT.OUT_FIELD_PAIR:
            f[0::2], f[1::2] = a, srcs[1][k]
        else:
            f[0 if kind == OUT.OUT_UNPAIRED_TOP else 1::2] = a
        planes.append(f)
    return tuple(planes)


def _rows(a, rect):
    x0, y0, w, h = rect
    return a[y0:y0 + h, x0:x0 + w]


def _expected_frame(planes, geom, fmt, layout, align, fake, out):
    """Write one frame into `out` (a uint8 vector prefilled by the caller) by the header's layout rule;
    returns frame_bytes.  Planar with contiguous rows is OUT.frame_bytes."""
    parts = [_rows(planes[0], geom.luma)]
    if fmt:
        cb, cr = _rows(planes[1], geom.chroma), _rows(planes[2], geom.chroma)
        if layout == OUT.SEMIPLANAR:
            parts.append(np.stack([cb, cr], axis=2).reshape(cb.shape[0], 2 * cb.shape[1]))
        else:
            parts += [cb, cr]
    elif fake and geom.fake_uv:
        run = np.full((1, geom.fake_uv), 128, np.uint8)
        parts += [np.concatenate([run, run], axis=1)] if layout == OUT.SEMIPLANAR else [run, run]
    off = 0
    for p in parts:
        h, w = p.shape
        pitch = w if align <= 1 else -(-w // align) * align
        view = out[off:off + pitch * h].reshape(h, pitch)
        view[:, :w] = p
        off += pitch * h
    return off


def _pattern(h, w, plane):
    y, x = np.mgrid[0:h, 0:w]
    return ((7 * x + 13 * y + plane) & 255).astype(np.uint8)


# ------------------------------------------------------------------------------ 1. directed small shapes
SIZES = [(1, 1), (1, 2), (3, 2), (11, 9)]
# (left, right): the cropped luma width mod 16 takes 0, 14, 2 (and 1, 15 where CropUnitX is 1), the
# source x offset mod 4 every value (luma where CropUnitX is 1, the chroma planes otherwise)
HCROPS = {2: [(0, 0), (1, 0), (3, 4), (2, 5)],
          1: [(0, 0), (3, 11), (2, 0), (1, 14), (0, 1), (1, 0)]}
VCROPS = [(0, 0, 1), (1, 0, 1), (0, 1, 0), (1, 1, 0)]                 # top, bottom, frame_mbs_only
KINDS = [OUT.OUT_FRAME, OUT.OUT_FIELD_PAIR, OUT.OUT_UNPAIRED_TOP, OUT.OUT_UNPAIRED_BOT]
CASES = [(1, False), (2, False), (3, False), (0, True), (0, False)]   # chroma_format_idc, fake_chroma


def _check_crop_coverage():
    for unit, crops in HCROPS.items():
        widths = {(16 - unit * (l + r)) % 16 for l, r in crops}
        assert widths >= ({0, 2, 14} | ({1, 15} if unit == 1 else set()))
        assert {l % 4 for l, r in crops} == {0, 1, 2, 3}
        assert all(16 - unit * (l + r) > 0 for l, r in crops)         # fits the 1-MB-wide frame


def _sources(kind, W, H, fmt, salt):
    """Host planes of the sources one frame of `kind` needs, pattern-filled, each plane with its own salt."""
    cw, ch = A.chroma_mb(fmt)
    fld = 0 if kind == OUT.OUT_FRAME else 1
    srcs = []
    for s in range(2 if kind == OUT.OUT_FIELD_PAIR else 1):
        shapes = [(16 * H >> fld, 16 * W)] + ([(ch * H >> fld, cw * W)] * 2 if fmt else [])
        srcs.append(tuple(_pattern(h, w, salt + 3 * s + p) for p, (h, w) in enumerate(shapes)))
    return srcs


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("fmt,fake", CASES, ids=["420", "422", "444", "400fake", "400"])
def test_directed_small_shapes(decs, fmt, fake, W, H):
    """Every output byte, and every byte that is not output (pitch padding, the gap between frames,
    the bytes around the buffer) still 0xA5."""
    import torch
    _check_crop_coverage()
    dec = decs[fmt]
    unit = 1 if fmt in (0, 3) else 2
    job = 0
    for layout in (OUT.PLANAR, OUT.SEMIPLANAR):
        for align in (0, 64, 256):
            for ci, (l, r) in enumerate(HCROPS[unit]):
                t, b, fmo = VCROPS[(ci + job) % len(VCROPS)]
                crop = OUT.Crop(l, r, t, b, frame_mbs_only=fmo)
                geom = OUT.geometry(W, H, crop, fmt)
                n = (1, 2, 5)[job % 3]
                kinds = [KINDS[(job + 3 * i) % 4] for i in range(n)]
                # sources laid out back to back in one device buffer, in the REVERSE of output order
                host = [_sources(k, W, H, fmt, 11 * i + job) for i, k in enumerate(kinds)]
                flat, where = [], {}
                for i in reversed(range(n)):
                    for s, planes in enumerate(host[i]):
                        for p, a in enumerate(planes):
                            where[(i, s, p)] = sum(x.size for x in flat)
                            flat.append(a.reshape(-1))
                pool = torch.from_numpy(np.concatenate(flat)).cuda()
                base = pool.data_ptr()
                rows = []
                for i, k in enumerate(kinds):
                    ent = [k]
                    for s in range(len(host[i])):
                        ent.append(tuple(base + where[(i, s, p)] if p < len(host[i][s]) else None for p in range(3)))
                    rows.append(tuple(ent))
                out = OUT.DeviceOutput(dec, W, H, crop, layout=layout, pitch_align=align, fake_chroma=fake)
                want_one = np.full(1 << 20, FILL, np.uint8)
                fb = _expected_frame(_woven(kinds[0], host[0]), geom, fmt, layout, align, fake, want_one)
                assert out.geom.frame_bytes == fb
                # frames 37 bytes apart beyond their size, the buffer 3 bytes off a 16-byte boundary
                stride, lead = fb + 37, 3 + (job % 13)
                total = lead + n * stride + 64
                want = np.full(total, FILL, np.uint8)
                for i, k in enumerate(kinds):
                    _expected_frame(_woven(k, host[i]), geom, fmt, layout, align, fake, want[lead + i * stride:])
                buf = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
                dst = buf[lead:lead + n * stride].view(n, stride)
                table = out.frames_from(rows)
                out.run(table, dst=dst)
                dec.check()
                got = buf.cpu().numpy()
                if not np.array_equal(got, want):
                    bad = np.flatnonzero(got != want)
                    pytest.fail(f"fmt {fmt} fake {fake} {W}x{H} layout {layout} align {align} crop {crop} kinds {kinds}: "
                                f"{len(bad)} bytes differ, first at {bad[0] - lead} of frame stride {stride} "
                                f"(got {got[bad[0]]}, want {want[bad[0]]})")
                if layout == OUT.PLANAR and align == 0 and kinds[0] == OUT.OUT_FRAME and (fmt or fake):
                    y, u, v = (host[0][0] + (None, None))[:3]               # the reference's bytes
                    assert bytes(got[lead:lead + fb]) == OUT.frame_bytes(y, u, v, geom)
                job += 1


# ------------------------------------------------------------------------------ 2. straight from the decoder
def _decode(L, dec, cfgs, n):
    """n pictures of every cfg as one batch; returns the DeviceBatch (its out planes stay on the device)."""
    pics = [synth.picture(L, cfg, i) for cfg in cfgs for i in range(n)]
    for s, (y, u, v) in enumerate(synth.refpics(L, cfgs[0])):
        dec.set_ref(s, y, u, v)
    db = B.to_device(B.pack(pics, h264r.quant_flat()), len(pics), None)
    dec.decode_batch(db.batch)
    return db


@pytest.mark.parametrize("fmt", [1, 2, 3, 0], ids=["420", "422", "444", "400"])
@pytest.mark.parametrize("layout", [OUT.PLANAR, OUT.SEMIPLANAR], ids=["planar", "semiplanar"])
def test_frame_batch_from_decoder(L, decs, fmt, layout):
    """A decoded frame batch goes through the output stage on the same stream with no host step in
    between: the job reads the batch's own out_y / out_u / out_v."""
    dec = decs[fmt]
    over = {} if fmt == 1 else dict(chroma_format={2: 2, 3: 3, 0: A.SYNTH_CHROMA_400}[fmt])
    db = _decode(L, dec, [synth.default_cfg(L, 3, 11, 9, **over)], 3)
    crop = OUT.Crop(1, 2, 1, 3)
    out = OUT.DeviceOutput(dec, 11, 9, crop, layout=layout, fake_chroma=fmt == 0)
    order = [2, 0, 1]
    t = db.tensors
    table = out.frames_from([(OUT.OUT_FRAME, (t["out_y"][i], t["out_u"][i] if fmt else None, t["out_v"][i] if fmt else None))
                             for i in order])
    got = out.run(table)
    dec.check()
    got = got.cpu().numpy()
    geom = OUT.geometry(11, 9, crop, fmt)
    for k, i in enumerate(order):
        want = np.zeros(out.geom.frame_bytes, np.uint8)
        assert _expected_frame(db.planes(i)[:3 if fmt else 1], geom, fmt, layout, 0, fmt == 0, want) == len(want)
        assert np.array_equal(got[k], want), f"frame {k} (picture {i})"
        if layout == OUT.PLANAR:
            assert bytes(got[k]) == OUT.frame_bytes(*db.planes(i), geom)


def test_field_batches_woven_pairwise(L, decs):
    """A batch of top fields and bottom fields (11 x 4 MBs each) woven pairwise into 11 x 8 frames."""
    dec = decs[1]
    top = synth.default_cfg(L, 3, 11, 4, structure=1, seed=0x51)
    bot = synth.default_cfg(L, 3, 11, 4, structure=2, seed=0x52)
    n = 3
    db = _decode(L, dec, [top, bot], n)
    crop = OUT.Crop(2, 1, 1, 1, frame_mbs_only=0)
    t = db.tensors
    pic = lambda i: (t["out_y"][i], t["out_u"][i], t["out_v"][i])
    spec = [(OUT.OUT_FIELD_PAIR, i, n + i) for i in (1, 2, 0)] + [(OUT.OUT_UNPAIRED_TOP, 0), (OUT.OUT_UNPAIRED_BOT, n)]
    rows = [(s[0],) + tuple(pic(i) for i in s[1:]) for s in spec]
    geom = OUT.geometry(11, 8, crop, 1)
    for layout in (OUT.PLANAR, OUT.SEMIPLANAR):
        out = OUT.DeviceOutput(dec, 11, 8, crop, layout=layout)
        got = out.run(out.frames_from(rows))
        dec.check()
        got = got.cpu().numpy()
        for k, s in enumerate(spec):
            planes = _woven(s[0], [db.planes(i) for i in s[1:]])
            want = np.zeros(out.geom.frame_bytes, np.uint8)
            _expected_frame(planes, geom, 1, layout, 0, False, want)
            assert np.array_equal(got[k], want), f"layout {layout} frame {k} kind {s[0]}"


# ------------------------------------------------------------------------------ 3. the reference's MD5s
MD5_NAMES = [n for n, c in S.STREAMS.items()
             if c.get("crop") or c.get("field") or c.get("mbaff") or c.get("chroma_format", 1) != 1] + ["bp_qcif_ippp"]


def test_md5_stream_set():
    assert 20 <= len(MD5_NAMES) <= 30 and len(set(MD5_NAMES)) == len(MD5_NAMES)
    kinds = [S.STREAMS[n] for n in MD5_NAMES]
    assert sum(1 for c in kinds if c.get("field")) == 8 and any(c.get("field") and c.get("crop") for c in kinds)
    assert {c.get("chroma_format", 1) for c in kinds if c.get("crop")} == {0, 1, 2, 3}


@pytest.mark.parametrize("name", MD5_NAMES)
def test_stream_frames_match_reference_md5(L, name):
    """A committed stream's captured pictures replayed through the streaming API, their planes put
    back on the device, and ONE output job for the whole stream -- frames and field pairs in output
    order, the SPS crop, planar, rows contiguous, 4:0:0 with the fake chroma: every frame_bytes slice
    has the MD5 the unmodified reference's output file has."""
    import torch
    cfg = S.STREAMS[name]
    fmt = cfg.get("chroma_format", 1)
    pics = S.load_capture(S.capture_path(name))
    W, H = cfg["width_mbs"], cfg["height_mbs"]
    with h264r.Decoder(0, W, H, chroma_format=fmt) as dec:
        dev = []
        for p in pics:
            dec.assign_quant_params(p["quant"])
            dec.init(p["W"], p["H"], p["pic"], p["slices"])
            for a, rec, lv, mv, ri in S.iter_mbs(p):
                dec.decode(a, rec, lv, mv, ri)
            planes = dec.deblock_filter(p["keep"])
            dev.append(tuple(torch.from_numpy(x).cuda() for x in planes[:3 if fmt else 1]) + ((None, None) if not fmt else ()))
        frames = OUT.pair_fields([S.structure(p) for p in pics], [int(p["pic"]["poc"][0]) for p in pics])
        assert len(frames) == cfg["frames"] and all(k in (OUT.OUT_FRAME, OUT.OUT_FIELD_PAIR) for k, _, _ in frames)
        out = OUT.DeviceOutput(dec, W, H, S.crop_of(cfg), fake_chroma=fmt == 0)
        table = out.frames_from([(k, dev[a]) + ((dev[b],) if b >= 0 else ()) for k, a, b in frames])
        got = out.run(table)
        dec.check()
        got = got.cpu().numpy()
    assert got.shape == (cfg["frames"], out.geom.frame_bytes)
    md5 = [hashlib.md5(got[i].tobytes()).hexdigest() for i in range(len(got))]
    bad = [i for i, (a, b) in enumerate(zip(md5, GOLD[name]["frame_md5"])) if a != b]
    assert not bad, f"{name}: output frames {bad} differ from the reference"


# ------------------------------------------------------------------------------ 4. refusals
def test_refused_frames_are_skipped_and_reported(decs):
    """A kind outside 0..3 and a field pair without its bottom luma plane: the frame is skipped (its
    bytes untouched), the other frames of the job are written, check() reports H264R_EDEVICE once, and
    the next good job passes.  The bad entries hold NULL or valid pointers only: nothing faults even if
    the kernel did read them."""
    import torch
    dec = decs[1]
    W, H = 3, 2
    crop = OUT.Crop(1, 0, 0, 1)
    geom = OUT.geometry(W, H, crop, 1)
    out = OUT.DeviceOutput(dec, W, H, crop)
    fb = out.geom.frame_bytes
    frm = tuple(torch.from_numpy(a).cuda() for a in _sources(OUT.OUT_FRAME, W, H, 1, 1)[0])
    fld = [tuple(torch.from_numpy(a).cuda() for a in s) for s in _sources(OUT.OUT_FIELD_PAIR, W, H, 1, 9)]
    host = lambda planes: tuple(x.cpu().numpy() for x in planes)
    good_frame, good_pair = np.zeros(fb, np.uint8), np.zeros(fb, np.uint8)
    _expected_frame(host(frm), geom, 1, OUT.PLANAR, 0, False, good_frame)
    _expected_frame(_woven(OUT.OUT_FIELD_PAIR, [host(fld[0]), host(fld[1])]), geom, 1, OUT.PLANAR, 0, False, good_pair)
    untouched = np.full(fb, FILL, np.uint8)
    jobs = [
        ([(OUT.OUT_FRAME, frm), (9, frm), (OUT.OUT_FIELD_PAIR, fld[0], fld[1])], [good_frame, untouched, good_pair]),
        ([(OUT.OUT_FIELD_PAIR, fld[0], (None, fld[1][1], fld[1][2])), (OUT.OUT_FRAME, frm)], [untouched, good_frame]),
        ([(-1, frm), (OUT.OUT_FRAME, (frm[0], None, frm[2]))], [untouched, untouched]),
    ]
    for rows, wants in jobs:
        dst = torch.full((len(rows), fb), FILL, dtype=torch.uint8, device="cuda")
        out.run(out.frames_from(rows), dst=dst)
        with pytest.raises(h264r.H264RError) as e:
            dec.check()
        assert e.value.status == A.EDEVICE
        got = dst.cpu().numpy()
        for i, w in enumerate(wants):
            assert np.array_equal(got[i], w), f"frame {i} of {[r[0] for r in rows]}"
        # the error word is cleared by the report: a good job after it passes
        dst = torch.full((2, fb), FILL, dtype=torch.uint8, device="cuda")
        out.run(out.frames_from([(OUT.OUT_FIELD_PAIR, fld[0], fld[1]), (OUT.OUT_FRAME, frm)]), dst=dst)
        dec.check()
        got = dst.cpu().numpy()
        assert np.array_equal(got[0], good_pair) and np.array_equal(got[1], good_frame)


def test_400_context_never_reads_chroma(decs):
    """On a 4:0:0 context u / v are not even tested: NULL there is no refusal."""
    import torch
    dec = decs[0]
    y = torch.from_numpy(_pattern(32, 48, 5)).cuda()
    out = OUT.DeviceOutput(dec, 3, 2, OUT.Crop(3, 1, 2, 5), fake_chroma=True)
    got = out.run(out.frames_from([(OUT.OUT_FRAME, (y, None, None))]))
    dec.check()
    assert bytes(got.cpu().numpy()[0]) == OUT.frame_bytes(y.cpu().numpy(), None, None, OUT.geometry(3, 2, OUT.Crop(3, 1, 2, 5), 0))


def test_host_argument_refusals(decs):
    import ctypes as C
    import torch
    dec = decs[1]
    out = OUT.DeviceOutput(dec, 3, 2)
    fb = out.geom.frame_bytes
    y = torch.zeros(fb, dtype=torch.uint8, device="cuda")
    table = out.frames_from([(OUT.OUT_FRAME, (y, y, y))])
    dst = torch.zeros((1, fb), dtype=torch.uint8, device="cuda")
    call = lambda desc, tab, n, d, stride: dec._L.h264r_output_frames(dec.handle, C.byref(desc), tab, n, d, stride, None)
    tp, dp = table.tensor.data_ptr(), dst.data_ptr()
    assert call(out.desc, tp, 1, dp, fb - 1) == A.EINVAL               # frames would overlap
    assert call(out.desc, None, 1, dp, fb) == A.EINVAL and call(out.desc, tp, 1, None, fb) == A.EINVAL
    assert call(out.desc, tp, -1, dp, fb) == A.EINVAL
    assert call(out.desc, tp, 0, dp, fb) == A.OK                        # nothing to do
    bad = OUT.OutDesc(3, 2, 0, 0, 0, 0, 1, OUT.PLANAR, 0, 1)
    assert call(bad, tp, 1, dp, fb) == A.EUNSUPPORTED                   # fake chroma off 4:0:0
    bad = OUT.OutDesc(3, 2, 0, 0, 0, 0, 1, 7, 0, 0)
    assert call(bad, tp, 1, dp, fb) == A.EINVAL
    assert call(out.desc, tp, 1, dp, fb) == A.OK
    dec.check()
