"""Deinterlaced frames on MI355X: h264r_deinterlace (include/h264r_deinterlace.h, k_deinterlace.hip).

Every comparison is byte-exact against tests/deint_restate.py, the definition restated from the header; no
expected byte comes from the library.  Destinations are prefilled with 0xA5 and compared whole, so a byte
written outside a plane's cropped rectangle (the rest of the coded-size plane, the gap between frames, the
bytes around the buffer) fails like a wrong sample.  Frames start a misaligned lead off the allocation and
lie a gap apart, as in tests/test_gpu_output_resample.py.  The shapes, tables and jobs are
deint_restate.CASES / case_table / case_jobs, whose coverage of the definition tests/test_deinterlace.py
holds on the CPU.
"""
import numpy as np
import pytest

import deint_restate as D
import h264r
import rgb_restate as R
from h264r import _abi as A
from h264r import batch as B
from h264r import output as OUT
from h264r import synth

pytestmark = pytest.mark.gpu

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


def _upload(table):
    """The sources of a host frame table back to back in one device buffer, in the REVERSE of table order;
    returns the pool (keep it alive) and frames_from's rows."""
    import torch
    flat, where, at = [], {}, 0
    for i in reversed(range(len(table))):
        for s, planes in enumerate(table[i][1]):
            for p, a in enumerate(planes):
                where[(i, s, p)] = at
                flat.append(a.reshape(-1))
                at += a.size
    pool = torch.from_numpy(np.concatenate(flat)).cuda()
    base = pool.data_ptr()
    rows = [(kind,) + tuple(tuple(base + where[(i, s, p)] if p < len(planes) else None for p in range(3))
                            for s, planes in enumerate(srcs)) for i, (kind, srcs) in enumerate(table)]
    return pool, rows


def _run(dec, fmt, W, H, crop, table, jobs, lead, gap, refused=(), rows=None):
    """One call into a 0xA5 buffer; every byte of the buffer against deint_restate (the jobs in `refused`
    keep their 0xA5).  Returns the destination tensor."""
    import torch
    pool, up = _upload(table)
    out = OUT.DeviceOutput(dec, W, H, crop)
    fb = D.layout(W, H, crop, fmt)[4]
    assert out.chroma_format == fmt and OUT.deint_geometry(out.desc, fmt).frame_bytes == fb
    n = len(jobs)
    stride = fb + gap
    total = lead + n * stride + 64
    want = np.full(total, FILL, np.uint8)
    for j, job in enumerate(jobs):
        if j not in refused:
            assert D.frame(job, table, W, H, crop, fmt, want[lead + j * stride:]) == fb
    buf = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    dst = buf[lead:lead + n * stride].view(n, stride)
    res = out.deinterlace(out.frames_from(up if rows is None else rows(up)), jobs, dst)
    if refused:
        with pytest.raises(h264r.H264RError) as e:
            dec.check()
        assert e.value.status == A.EDEVICE
    else:
        dec.check()
    got = buf.cpu().numpy()
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        j, o = divmod(int(bad[0]) - lead, stride)
        pytest.fail(f"fmt {fmt} {W}x{H} crop {crop} lead {lead} gap {gap}: {len(bad)} bytes differ, first in job {j} {jobs[j] if 0 <= j < n else None} "
                    f"at {o} of frame_bytes {fb} (got {got[bad[0]]}, want {want[bad[0]]})")
    del pool
    return res


# ------------------------------------------------------------------------------ 1. the directed cases
@pytest.mark.parametrize("k", range(len(D.CASES)), ids=[f"{'400 420 422 444'.split()[c[0]]}-{c[1]}x{c[2]}-{k}" for k, c in enumerate(D.CASES)])
def test_directed_cases(decs, k):
    """deint_restate.CASES: all four chroma formats; widths around H264R_DEINT_TILE_W, of more than two
    tiles and down to 2; heights of 2 and 4 and around H264R_DEINT_TILE_H; under every job of case_jobs():
    keep x second x mode, prev and / or next -1, prev == cur == next, FRAME and FIELD_PAIR namings of the same
    bytes, BOB from unpaired fields."""
    fmt, W, H, c = D.CASES[k]
    crop = OUT.Crop(*c[:4], frame_mbs_only=c[4])
    table, jobs = D.case_table(k), D.case_jobs()
    res = _run(decs[fmt], fmt, W, H, crop, table, jobs, (1, 5, 0, 16)[k % 4], (37, 0, 48)[k % 3])
    got = res.cpu().numpy()
    fb = D.layout(W, H, crop, fmt)[4]
    # the two namings of the same bytes: the same frames
    pairs = {jobs.index(a): jobs.index(b) for a, b in (((1, 0, 2, 0, 0, 1), (4, 5, 2, 0, 0, 1)), ((1, 0, 2, 1, 1, 1), (4, 0, 2, 1, 1, 1)),
                                                      ((1, 0, 2, 0, 0, 1), (1, 5, 2, 0, 0, 1)))}
    for a, b in pairs.items():
        assert np.array_equal(got[a, :fb], got[b, :fb])


def test_cases_are_what_they_claim():
    tw, th = OUT.DEINT_TILE_W, OUT.DEINT_TILE_H
    lw = {fmt: set() for fmt in range(4)}
    lh = {fmt: set() for fmt in range(4)}
    for fmt, W, H, c in D.CASES:
        assert 2 <= W <= 8 and 2 <= H <= 5
        r = D.layout(W, H, OUT.Crop(*c[:4], frame_mbs_only=c[4]), fmt)[0][0]
        lw[fmt].add(r[2]); lh[fmt].add(r[3])
    every_w, every_h = set().union(*lw.values()), set().union(*lh.values())
    assert {tw - 1, tw, tw + 1, 2} <= every_w and {tw - 2, tw, tw + 2} <= lw[1] | lw[2] and max(every_w) > 2 * tw
    assert {tw - 1, tw + 1} <= lw[3] | lw[0] and 2 in lw[1] and 2 in lw[3]
    assert all(4 in lh[f] for f in (1, 2, 3)) and 2 in lh[3] and 2 in lh[0]
    assert {th - 4, th - 2, th, th + 4} <= every_h


# ------------------------------------------------------------------------------ 2. refusals
@pytest.mark.parametrize("fmt", [1, 0], ids=["420", "400"])
def test_bad_jobs_among_good_ones(decs, fmt):
    """An index out of range, a bad mode, keep and second outside 0 / 1, a NULL plane, ADAPTIVE on an unpaired
    source (as cur, as prev), an unpaired parity that differs from keep: exactly those jobs keep their 0xA5,
    check() reports H264R_EDEVICE, the good jobs are exact -- among them BOB jobs whose prev / next name the
    refused sources, which BOB never dereferences.  The bad entries hold NULL or valid pointers only."""
    dec = decs[fmt]
    k = 3 if fmt else 15
    assert D.CASES[k][0] == fmt
    _, W, H, c = D.CASES[k]
    crop = OUT.Crop(*c[:4], frame_mbs_only=c[4])
    table = D.case_table(k)                                     # 0 .. 5 frames and pairs, 6 unpaired top, 7 unpaired bottom
    table += [table[1], table[0]]                               # 8: a pair without a plane, 9: a frame of a kind out of range
    n = len(table)

    def rows(up):
        up = list(up)
        kind, top, bot = up[8]
        up[8] = (kind, top, (bot[0], None, bot[2]) if fmt else (None, None, None))     # 4:0:0: y[1]; else u[1]
        up[9] = (9,) + up[9][1:]
        return up
    AD, BOB = OUT.DEINT_ADAPTIVE, OUT.DEINT_BOB
    jobs = [(1, 0, 2, 0, 0, AD),            # good
            (n, 0, 2, 0, 0, AD), (-1, 0, 2, 0, 0, BOB), (1, -2, 2, 0, 0, AD), (1, 0, n, 1, 0, BOB),       # 1 .. 4: indices
            (2, 1, 3, 1, 1, AD),            # good
            (1, 0, 2, 0, 0, 2), (1, 0, 2, 0, 0, -1), (1, 0, 2, 2, 0, AD), (1, 0, 2, 0, -1, BOB),           # 6 .. 9: mode, keep, second
            (8, 0, 2, 0, 0, AD), (8, -1, -1, 1, 0, BOB), (1, 8, 2, 0, 0, AD), (1, 0, 8, 1, 1, AD), (9, -1, -1, 0, 0, BOB),   # 10 .. 14
            (6, -1, -1, 0, 0, AD), (1, 6, 2, 0, 0, AD), (1, 0, 7, 1, 0, AD),                               # 15 .. 17: unpaired
            (6, -1, -1, 1, 0, BOB), (7, -1, -1, 0, 0, BOB),                                                # 18, 19: parity
            (6, 8, 9, 0, 0, BOB), (7, 9, 8, 1, 1, BOB), (1, 8, 6, 1, 0, BOB), (3, -1, -1, 0, 1, AD)]       # good
    refused = set(range(1, 5)) | set(range(6, 20))
    for j, job in enumerate(jobs):
        assert (OUT.deint_job_status(job, n) != A.OK) == (j in (1, 2, 3, 4, 6, 7, 8, 9))
    _run(dec, fmt, W, H, crop, table, jobs, 3, 16, refused=refused, rows=rows)
    # the error word is cleared by the report: a good call after it passes
    _run(dec, fmt, W, H, crop, table[:8], [jobs[0], jobs[5]], 0, 0)


def test_host_refusals_on_a_context(decs):
    import ctypes as C
    import torch
    dec = decs[1]
    out = OUT.DeviceOutput(dec, 3, 2, OUT.Crop(frame_mbs_only=0))
    y = torch.zeros(32 * 48, dtype=torch.uint8, device="cuda")
    table = out.frames_from([(OUT.OUT_FRAME, (y, y, y))])
    jobs = torch.from_numpy(OUT.deint_jobs(1, mode=OUT.DEINT_BOB).view(np.uint8).copy()).cuda()
    fb = OUT.deint_geometry(out.desc, 1).frame_bytes
    assert fb == 48 * 32 * 3 // 2
    dst = torch.full((fb + 16,), FILL, dtype=torch.uint8, device="cuda")
    tp, jp, dp, h = table.tensor.data_ptr(), jobs.data_ptr(), dst.data_ptr(), dec.handle
    call = lambda ctx, desc, tab, n, jb, nj, d, stride: dec._L.h264r_deinterlace(ctx, C.byref(desc) if desc is not None else None, tab, n,
                                                                                jb, nj, d, stride, None)
    d = out.desc
    assert call(None, d, tp, 1, jp, 1, dp, fb) == A.EINVAL and call(h, None, tp, 1, jp, 1, dp, fb) == A.EINVAL
    assert call(h, d, None, 1, jp, 1, dp, fb) == A.EINVAL and call(h, d, tp, 1, None, 1, dp, fb) == A.EINVAL
    assert call(h, d, tp, 1, jp, 1, None, fb) == A.EINVAL
    assert call(h, d, tp, -1, jp, 1, dp, fb) == A.EINVAL and call(h, d, tp, 1, jp, -1, dp, fb) == A.EINVAL
    assert call(h, d, tp, 1, jp, 1, dp, fb - 1) == A.EINVAL            # frames would overlap
    assert call(h, OUT._desc(3, 2, OUT.Crop(frame_mbs_only=0), OUT.SEMIPLANAR, 0, False), tp, 1, jp, 1, dp, fb) == A.EINVAL
    assert call(h, OUT._desc(3, 2, OUT.Crop(frame_mbs_only=0), OUT.PLANAR, 64, False), tp, 1, jp, 1, dp, fb) == A.EINVAL
    assert call(h, OUT._desc(3, 2, OUT.Crop(0, 0, 1, 0, frame_mbs_only=1), OUT.PLANAR, 0, False), tp, 1, jp, 1, dp, fb) == A.EUNSUPPORTED
    assert call(h, OUT._desc(3, 2, OUT.Crop(0, 0, 1, 0, frame_mbs_only=1), OUT.PLANAR, 0, False), tp, 1, jp, 1, dp, fb - 1) == A.EUNSUPPORTED
    assert call(h, d, tp, 1, jp, 0, dp, fb) == A.OK                    # nothing to do
    dec.check()
    assert bool((dst == FILL).all())
    assert call(h, d, tp, 1, jp, 1, dp + 1, fb) == A.OK                # any alignment
    dec.check()
    got = dst.cpu().numpy()
    assert got[0] == FILL and not got[1:1 + fb].any() and bool((got[1 + fb:] == FILL).all())
    with pytest.raises(ValueError):
        out.deinterlace(tp, OUT.deint_jobs(1))                         # a raw table needs its count
    with pytest.raises(ValueError):
        out.deinterlace(table, jp)                                     # a raw job table too


# ------------------------------------------------------------------------------ 3. from the decoder, and into the RGB stage
def _decode(L, dec, cfgs, n):
    """n pictures of every cfg as one batch; returns the DeviceBatch (its out planes stay on the device)."""
    pics = [synth.picture(L, cfg, i) for cfg in cfgs for i in range(n)]
    for s, (y, u, v) in enumerate(synth.refpics(L, cfgs[0])):
        dec.set_ref(s, y, u, v)
    db = B.to_device(B.pack(pics, h264r.quant_flat()), len(pics), None)
    dec.decode_batch(db.batch)
    return db


def test_field_pictures_from_the_decoder_on_another_stream(L, decs):
    """Top fields and bottom fields (11 x 4 MBs each) decoded on the context's stream, deinterlaced at field
    rate straight from the batch's out planes on a stream of the caller's, with no host synchronisation in
    between; compared with the restatement applied to the downloaded planes."""
    import torch
    dec = decs[1]
    n = 3
    W, H = 11, 8
    crop = OUT.Crop(2, 1, 1, 1, frame_mbs_only=0)
    out = OUT.DeviceOutput(dec, W, H, crop)
    fb = OUT.deint_geometry(out.desc, 1).frame_bytes
    jobs = np.concatenate([OUT.deint_jobs(n, tff=True, mode=OUT.DEINT_ADAPTIVE, field_rate=True),
                           OUT.deint_jobs(n, tff=False, mode=OUT.DEINT_BOB)])
    dst = torch.full((len(jobs), fb + 32), FILL, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    top = synth.default_cfg(L, 3, W, H // 2, structure=1, seed=0x51)
    bot = synth.default_cfg(L, 3, W, H // 2, structure=2, seed=0x52)
    db = _decode(L, dec, [top, bot], n)
    t = db.tensors
    pic = lambda i: (t["out_y"][i], t["out_u"][i], t["out_v"][i])
    table = out.frames_from([(OUT.OUT_FIELD_PAIR, pic(i), pic(n + i)) for i in range(n)])
    out.deinterlace(table, jobs, dst, stream=side.cuda_stream)
    side.synchronize()
    dec.check()
    host = [(OUT.OUT_FIELD_PAIR, [tuple(p.cpu().numpy().reshape(-1, w) for p, w in zip(pic(i), (16 * W, 8 * W, 8 * W))),
                                  tuple(p.cpu().numpy().reshape(-1, w) for p, w in zip(pic(n + i), (16 * W, 8 * W, 8 * W)))])
            for i in range(n)]
    assert host[0][1][0][0].shape == (16 * H // 2, 16 * W)
    assert any(not np.array_equal(host[i][1][0][0], host[i][1][1][0]) for i in range(n))
    want = np.full((len(jobs), fb + 32), FILL, np.uint8)
    for j, job in enumerate(jobs):
        D.frame(tuple(job), host, W, H, crop, 1, want[j])
    assert np.array_equal(dst.cpu().numpy(), want)


@pytest.mark.parametrize("fmt", [1, 2, 3, 0], ids=["420", "422", "444", "400"])
def test_result_named_as_a_frame_into_the_rgb_stage(decs, fmt):
    """Composition: the deinterlaced frames, named as H264R_OUT_FRAME sources by frames_of(), through
    h264r_output_rgb with the same descriptor: rgb_restate applied to the restated deinterlaced planes."""
    dec = decs[fmt]
    k = {1: 3, 2: 7, 3: 11, 0: 15}[fmt]
    assert D.CASES[k][0] == fmt
    _, W, H, c = D.CASES[k]
    crop = OUT.Crop(*c[:4], frame_mbs_only=c[4])
    table, jobs = D.case_table(k), [(1, 0, 2, 0, 0, OUT.DEINT_ADAPTIVE), (2, 1, 3, 1, 1, OUT.DEINT_ADAPTIVE), (6, -1, -1, 0, 0, OUT.DEINT_BOB)]
    pool, up = _upload(table)
    out = OUT.DeviceOutput(dec, W, H, crop)
    frames = out.deinterlace(out.frames_from(up), jobs)
    named = out.frames_of(frames)
    assert named.n == len(jobs)
    rects, off, pitch, rows, fb = D.layout(W, H, crop, fmt)
    for j, (format, up_mode) in enumerate(((R.PLANAR_U8, R.BILINEAR), (R.PACKED_U8, R.REPLICATE))):
        rgb = out.rgb(named, format=format, chroma_up=up_mode, matrix=R.BT601, full_range=j)
        dec.check()
        raw = rgb.cpu().numpy()
        for i, job in enumerate(jobs):
            planes = np.zeros(fb, np.uint8)
            D.frame(job, table, W, H, crop, fmt, planes)
            coded = tuple(planes[o:o + p * r].reshape(r, p) for o, p, r in zip(off, pitch, rows))
            ch = R.channels(*R.source_frame(coded, W, H, crop, fmt), fmt, R.BT601, j, up_mode, False)
            lw, lh = rects[0][2:]
            want = np.zeros(R.layout(lw, lh, format, 0)[2], np.uint8)
            R.write_frame(want, ch, format, 0)
            assert np.array_equal(np.ascontiguousarray(raw[i]).reshape(-1), want), (format, job)
    del pool
