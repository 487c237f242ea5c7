"""The slice-band exchange for every chroma format, and the halo of MBAFF frames, on the CPU.

* Host planes of chroma_format_idc 0, 2 and 3 through BandExchange in both implementations
  (gloo, world 2 and 3), by the method of test_dist.test_gloo_band_exchange: every row of the plan
  arrives, nothing else is written; the library's byte counts equal BandExchange.bytes_in(), and
  h264r_group_set_bands moves exactly what h264r_group_set_bands_fmt(.., 1, ..) moves.
* The argument errors of the format-aware entry points.
* dist.halo_mb_rows is sufficient, on the CPU oracle: a band decoded from references whose rows
  outside [band - h, band + h) are noise equals the band decoded from intact references -- MBAFF P
  and B pictures with mbaff=True (and NOT with the frame formula's h: a field MB reaches twice as
  far), 4:2:2 / 4:4:4 / 4:0:0 frame pictures with the frame formula.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _oracle as O
from h264r import _abi as A
from h264r import dist as D
from h264r import synth

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "arrow-h264_amd", "lib", "libh264r.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libh264r.so not built")
IMPLS = ["torch", pytest.param("abi", marks=needs_lib)]
FORMATS = (0, 2, 3)


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_row_bytes_per_mb_col():
    assert D.row_bytes_per_mb_col(1) == D.ROW_BYTES_PER_MB_COL == (256, 64, 64)
    assert D.row_bytes_per_mb_col() == (256, 64, 64)
    assert D.row_bytes_per_mb_col(0) == (256, 0, 0)
    assert D.row_bytes_per_mb_col(2) == (256, 128, 128)
    assert D.row_bytes_per_mb_col(3) == (256, 256, 256)
    for fmt in range(4):        # a chroma MB of A.chroma_mb samples, 16 rows of MBs wide
        cw, ch = A.chroma_mb(fmt)
        assert D.row_bytes_per_mb_col(fmt)[1] == cw * ch
    for bad in (-1, 4):
        with pytest.raises(ValueError):
            D.row_bytes_per_mb_col(bad)


def test_halo_rows_mbaff():
    # the frame formula is what it was (test_dist.test_halo_rows), with and without the keyword
    for m, want in ((0, 1), (52, 1), (53, 2), (131, 3)):
        assert D.halo_mb_rows(m) == D.halo_mb_rows(m, mbaff=False) == want
    # field MBs: 2 (ceil(m / 4) + 3) luma frame rows; chroma 4 (floor((m + 2) / 8) + 1)
    assert D.halo_mb_rows(0, mbaff=True) == 1            # 6 rows
    assert D.halo_mb_rows(20, mbaff=True) == 1           # 2 (5 + 3) = 16 rows
    assert D.halo_mb_rows(21, mbaff=True) == 2
    assert D.halo_mb_rows(35, mbaff=True) == 2           # 24 rows; the frame formula gives 1
    assert D.halo_mb_rows(99, mbaff=True) == 4           # 56 rows; the frame formula gives 2
    assert D.halo_mb_rows(35) == 1 and D.halo_mb_rows(99) == 2
    for m in range(0, 600):
        assert D.halo_mb_rows(m, mbaff=True) >= D.halo_mb_rows(m)


# ------------------------------------------------------------------ host planes through the group
def _fill(planes, rb, psz, nk, b0, b1, value):
    for pl in range(3):
        v = planes[pl][: nk * psz[pl]].view(nk, psz[pl])
        for k in range(nk):
            for r in range(b0, b1):
                v[k, r * rb[pl]:(r + 1) * rb[pl]] = value(k, pl, r)


def _fmt_worker(rank, world, port, q, impl):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ok = []
        W, H, nk, slack = 5, 11, 3, 64
        for fmt in FORMATS:
            rb = [c * W for c in D.row_bytes_per_mb_col(fmt)]
            psz = [r * H for r in rb]

            def value(k, pl, row):          # a byte per (picture, plane, MB row, offset)
                return ((torch.arange(rb[pl], dtype=torch.int64) * 3 + k * 101 + pl * 37 + row * 13) % 251).to(torch.uint8)
            for starts in ([0, 2, 3, 5], [0, 1, 4, 6], [0, 3]):
                bands = D.slice_bands(starts, H, world)
                b0, b1 = bands[rank]
                for mode, halo in (("halo", 1), ("halo", 2), ("allgather", 0)):
                    planes = [torch.full((nk * psz[pl] + slack,), 0xEE, dtype=torch.uint8) for pl in range(3)]
                    _fill(planes, rb, psz, nk, b0, b1, value)
                    X = D.BandExchange(bands, rank, W, H, nk, mode, halo, "cpu", impl=impl, chroma_format=fmt)
                    X.run(planes)
                    lo, hi = (0, H) if mode == "allgather" else (max(b0 - halo, 0), min(b1 + halo, H))
                    if b1 <= b0 and mode == "halo":
                        lo, hi = b0, b0
                    good = True
                    for pl in range(3):
                        v = planes[pl][: nk * psz[pl]].view(nk, psz[pl])
                        for k in range(nk):
                            for r in range(H):
                                seg = v[k, r * rb[pl]:(r + 1) * rb[pl]]
                                want = value(k, pl, r) if lo <= r < hi else torch.full_like(seg, 0xEE)
                                good &= bool(torch.equal(seg, want))
                        good &= bool((planes[pl][nk * psz[pl]:] == 0xEE).all())
                    # the format's bytes: what the plan names, in every plane
                    rows_in = sum(n1 - n0 for n0, n1 in X.need.values())
                    if impl == "abi":
                        good &= X.bytes_in() == nk * sum(rb) * rows_in
                        sent, recvd, transfers = X.grp.stats()
                        good &= recvd == X.bytes_in() and transfers == len(X.need) + len(X.give)
                        good &= sent == nk * sum(rb) * sum(g1 - g0 for g0, g1 in X.give.values())
                        X.grp.close()
                    else:
                        good &= X.bytes_in() >= nk * sum(rb) * rows_in
                    ok.append(good)
            if fmt == 0 and impl == "abi":
                # 4:0:0 takes planes of no rows: the chroma tensors above hold the slack alone
                ok.append(psz[1] == 0 and planes[1].numel() == slack)
        q.put((rank, all(ok), len(ok)))
    finally:
        dist.destroy_process_group()


def _spawn(target, world, *args):
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world, port, q) + args) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("world", [2, 3])
def test_gloo_band_exchange_formats(world, impl):
    """4:0:0, 4:2:2 and 4:4:4 host planes through BandExchange (both implementations)."""
    res = _spawn(_fmt_worker, world, impl)
    assert [r[1] for r in res] == [True] * world
    assert all(r[2] >= 27 for r in res)


def _compat_worker(rank, world, port, q):
    """h264r_group_set_bands against h264r_group_set_bands_fmt(.., 1, ..): the same planes through a
    group of each, the results and the byte counts compared."""
    import h264r
    from h264r import group as G
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        L = h264r.lib()
        ok = []
        W, H, nk, slack = 5, 11, 3, 64
        rb = [c * W for c in D.ROW_BYTES_PER_MB_COL]
        psz = [r * H for r in rb]
        value = lambda k, pl, row: ((torch.arange(rb[pl], dtype=torch.int64) * 5 + k * 71 + pl * 29 + row * 11) % 251
                                    ).to(torch.uint8)
        for starts in ([0, 2, 3, 5], [0, 3]):
            bands = D.slice_bands(starts, H, world)
            b0, b1 = bands[rank]
            barr = G._bands_array(bands)
            for mode, halo in (("halo", 2), ("allgather", 0)):
                out, stats = [], []
                for fmt_entry in (False, True):
                    planes = [torch.full((nk * psz[pl] + slack,), 0xEE, dtype=torch.uint8) for pl in range(3)]
                    _fill(planes, rb, psz, nk, b0, b1, value)
                    g = G.Group(world, rank, -1, "torch")
                    if fmt_entry:
                        st = L.h264r_group_set_bands_fmt(g._h, W, H, 1, barr.ctypes.data, G.MODES[mode], halo, nk)
                    else:
                        st = L.h264r_group_set_bands(g._h, W, H, barr.ctypes.data, G.MODES[mode], halo, nk)
                    ok.append(st == 0)
                    g.exchange(nk, planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), psz[0], psz[1])
                    out.append(planes)
                    stats.append(g.stats())
                    g.close()
                ok.append(stats[0] == stats[1] and (world == 1 or stats[0][1] > 0 or b1 <= b0))
                ok.append(all(bool(torch.equal(a, b)) for a, b in zip(*out)))
                need, _ = G.plan(bands, rank, mode, halo)
                ok.append(stats[0][1] == nk * 384 * W * sum(n1 - n0 for n0, n1 in need.values()))
        q.put((rank, all(ok), len(ok)))
    finally:
        dist.destroy_process_group()


@needs_lib
def test_set_bands_is_the_420_case():
    res = _spawn(_compat_worker, 2)
    assert [r[1] for r in res] == [True, True] and res[0][2] == 20


@needs_lib
def test_group_format_argument_errors():
    import ctypes as C
    import h264r
    from h264r import group as G
    W, H = 2, 3
    g = G.Group(1, 0, -1, "torch")
    try:
        for bad in (-1, 4):
            with pytest.raises(h264r.H264RError) as e:
                g.set_bands(W, H, [(0, H)], "halo", 1, 2, chroma_format=bad)
            assert e.value.status == A.EINVAL
        buf = (C.c_uint8 * (256 * W * H))()
        p = C.addressof(buf)
        # 4:2:2: chroma rows are 128 W bytes, so a 4:2:0 stride is too small; NULL chroma is refused
        g.set_bands(W, H, [(0, H)], "halo", 1, 2, chroma_format=2)
        g.exchange(1, p, p, p, 256 * W * H, 128 * W * H)
        for args in ((p, p, p, 256 * W * H, 64 * W * H), (p, p, p, 256 * W * H, 128 * W * H - 1),
                     (p, p, p, 256 * W * H - 1, 128 * W * H), (p, None, None, 256 * W * H, 128 * W * H),
                     (p, p, None, 256 * W * H, 128 * W * H)):
            with pytest.raises(h264r.H264RError) as e:
                g.exchange(1, *args)
            assert e.value.status == A.EINVAL
        # a refused format leaves the plan in place
        with pytest.raises(h264r.H264RError):
            g.set_bands(W, H, [(0, H)], "halo", 1, 2, chroma_format=4)
        g.exchange(1, p, p, p, 256 * W * H, 128 * W * H)
        # 4:4:4: 256 W bytes per chroma row
        g.set_bands(W, H, [(0, H)], "halo", 1, 2, chroma_format=3)
        g.exchange(1, p, p, p, 256 * W * H, 256 * W * H)
        with pytest.raises(h264r.H264RError):
            g.exchange(1, p, p, p, 256 * W * H, 128 * W * H)
        # 4:0:0: NULL chroma is accepted and stride_c ignored; given chroma planes are not looked at
        g.set_bands(W, H, [(0, H)], "halo", 1, 2, chroma_format=0)
        g.exchange(1, p, None, None, 256 * W * H, 0)
        g.exchange(1, p, None, None, 256 * W * H, -5)
        g.exchange(1, p, p, p, 256 * W * H, 0)
        with pytest.raises(h264r.H264RError):
            g.exchange(1, None, None, None, 256 * W * H, 0)
        # 4:2:0 through either entry point: NULL chroma stays refused
        for fmt in (None, 1):
            if fmt is None:
                b = G._bands_array([(0, H)])
                assert g._L.h264r_group_set_bands(g._h, W, H, b.ctypes.data, G.HALO, 1, 2) == A.OK
            else:
                g.set_bands(W, H, [(0, H)], "halo", 1, 2, chroma_format=fmt)
            g.exchange(1, p, p, p, 256 * W * H, 64 * W * H)
            with pytest.raises(h264r.H264RError):
                g.exchange(1, p, None, None, 256 * W * H, 64 * W * H)
            with pytest.raises(h264r.H264RError):
                g.exchange(1, p, p, p, 256 * W * H, 64 * W * H - 1)
    finally:
        g.close()


# ------------------------------------------------------------------ halo sufficiency (oracle only)
def _max_abs_mvy(p) -> int:
    """max |mv_y| (quarter samples) over the vectors the picture uses."""
    used = p.ref_idx >= 0
    if not used.any():
        return 0
    my = (p.mv >> 16).astype(np.uint16).view(np.int16).reshape(p.mv.shape)
    return int(np.abs(my[used].astype(np.int32)).max())


def _slice_bands(p):
    """[(row0, row1)] of the picture's slices (whole MB rows each)."""
    H, W = p.cfg.height_mbs, p.cfg.width_mbs
    s = p.mbs["slice"].reshape(H, W)
    assert (s == s[:, :1]).all()
    first = [0] + [r for r in range(1, H) if s[r, 0] != s[r - 1, 0]] + [H]
    return list(zip(first[:-1], first[1:]))


def _noisy_refs(refs, fmt, b0, b1, h, seed):
    """refs with every row outside MB rows [b0 - h, b1 + h) replaced by seeded noise."""
    rnd = np.random.default_rng(seed)
    ch = A.chroma_mb(fmt)[1]
    out = []
    for planes in refs:
        new = []
        for k, a in enumerate(planes):
            n = 16 if k == 0 else ch
            a = a.copy()
            lo, hi = max(b0 - h, 0) * n, min((b1 + h) * n, a.shape[0])
            noise = rnd.integers(0, 256, a.shape, dtype=np.uint8)
            a[:lo] = noise[:lo]
            a[hi:] = noise[hi:]
            new.append(a)
        out.append(tuple(new))
    return out


def _band_differs(p, refs, want, fmt, band, h, seed) -> bool:
    b0, b1 = band
    got = O.decode(p, _noisy_refs(refs, fmt, b0, b1, h, seed))
    ch = A.chroma_mb(fmt)[1]
    return any(not np.array_equal(got[k][b0 * n:b1 * n], want[k][b0 * n:b1 * n])
               for k, n in ((0, 16), (1, ch), (2, ch)) if n)


MBAFF_KINDS = {"P": (3, dict(num_refs=3)), "B": (4, dict(wp_mode=1, num_refs=2))}


@pytest.mark.parametrize("mv_range_y", [8, 24])
@pytest.mark.parametrize("kind", ["P", "B"])
def test_halo_is_sufficient_for_mbaff(kind, mv_range_y):
    """MBAFF pictures of 22 x 18 MBs, 3 slices, idc 2: halo_mb_rows(.., mbaff=True) rows of the
    references around a band are all the band reads; the frame formula's are not."""
    L = O.lib()
    cidx, over = MBAFF_KINDS[kind]
    cfg = synth.default_cfg(L, cidx, 22, 18, structure=A.MBAFF_FRAME, num_slices=3, deblock_idc=2,
                            mv_range_y=mv_range_y, **over)
    refs = synth.refpics(L, cfg)
    frame_h_fails = 0
    for index in (0, 1):
        p = synth.picture(L, cfg, index)
        f = p.mbs["flags"]
        assert ((f & A.MBF_FIELD) != 0).sum() >= 2, "the picture holds no field MBs"
        assert (((f & A.MBF_FIELD) != 0) & ((f & A.MBF_INTRA) == 0)).any(), "no inter field MB"
        bands = _slice_bands(p)
        assert bands == [(0, 6), (6, 12), (12, 18)]
        m = _max_abs_mvy(p)
        h, hf = D.halo_mb_rows(m, mbaff=True), D.halo_mb_rows(m)
        assert hf < h
        want = O.decode(p, refs)
        for i, band in enumerate(bands):
            assert not _band_differs(p, refs, want, 1, band, h, 100 * index + i), \
                f"picture {index} band {band}: max |mv_y| {m}, halo {h} MB rows is too small"
            frame_h_fails += _band_differs(p, refs, want, 1, band, hf, 100 * index + i)
    assert frame_h_fails >= 1, "the frame formula's halo was enough: the test shows nothing"


@pytest.mark.parametrize("cidx", [3, 4])
@pytest.mark.parametrize("fmt,synth_fmt", [(2, 2), (3, 3), (0, A.SYNTH_CHROMA_400)])
def test_halo_is_sufficient_for_chroma_formats(fmt, synth_fmt, cidx):
    """4:2:2 / 4:4:4 / 4:0:0 frame pictures need what the frame formula gives."""
    L = O.lib()
    for mv_range_y in (8, 24):
        over = dict(wp_mode=1) if cidx == 4 else {}
        cfg = synth.default_cfg(L, cidx, 22, 18, chroma_format=synth_fmt, num_slices=3, deblock_idc=2,
                                mv_range_y=mv_range_y, **over)
        refs = synth.refpics(L, cfg)
        for index in (0, 1):
            p = synth.picture(L, cfg, index)
            m = _max_abs_mvy(p)
            h = D.halo_mb_rows(m, mbaff=False)
            want = O.decode(p, refs)
            for i, band in enumerate(_slice_bands(p)):
                assert not _band_differs(p, refs, want, fmt, band, h, 100 * index + i), \
                    f"fmt {fmt} picture {index} band {band}: max |mv_y| {m}, halo {h} MB rows is too small"
