"""The format-aware band exchange (h264r_group_set_bands_fmt) and banded MBAFF decode on the GPU.

Two gloo ranks on the one GPU over the library's callback transport, as tests/test_gpu_group.py
(RCCL refuses two ranks on one device, so nothing here goes over RCCL):

* device planes of chroma_format_idc 0, 2 and 3 through k_band_copy with the format's row sizes:
  the rows of the plan arrive, nothing else is written, the slack after the planes is untouched;
* a chain rehearsal: each rank decodes its band of a dependent chain I -> P -> P of 22 x 18 MBs,
  one picture per step, and exchanges after each step; picture t + 1's only reference is picture
  t as the rank holds it after the exchange, rows it never received holding a marker.  MBAFF
  frames in halo mode with dist.halo_mb_rows(.., mbaff=True) and in all-gather mode, 4:2:2 frames
  in halo mode: each rank's band of every picture equals the oracle's chain of whole pictures.
"""
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MARK = 0xC3
FORMATS = (0, 2, 3)
# (name, chroma_format_idc, MBAFF, exchange mode)
CHAINS = (("mbaff halo", 1, True, "halo"), ("mbaff allgather", 1, True, "allgather"), ("4:2:2 halo", 2, False, "halo"))


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _planes_worker(rank, world, port, q):
    """test_gpu_group._worker's check for the other chroma formats."""
    import torch
    import torch.distributed as dist
    from h264r import dist as D
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        bad = []
        W, H, nk, slack = 5, 11, 3, 64
        for fmt in FORMATS:
            rb = [c * W for c in D.row_bytes_per_mb_col(fmt)]
            psz = [r * H for r in rb]
            for starts in ([0, 2, 5, 8], [0, 4, 6, 9], [0, 6]):
                bands = D.slice_bands(starts, H, world)
                for mode, halo in (("halo", 1), ("halo", 3), ("allgather", 0)):
                    val = lambda k, pl, r: ((torch.arange(rb[pl], dtype=torch.int64) * 7 + k * 89 + pl * 31 + r * 17) % 251
                                            ).to(torch.uint8)
                    host = [torch.full((nk * psz[pl] + slack,), 0xEE, dtype=torch.uint8) for pl in range(3)]
                    b0, b1 = bands[rank]
                    for pl in range(3):
                        hv = host[pl][: nk * psz[pl]].view(nk, psz[pl])
                        for k in range(nk):
                            for r in range(b0, b1):
                                hv[k, r * rb[pl]:(r + 1) * rb[pl]] = val(k, pl, r)
                    planes = [h.to("cuda:0") for h in host]
                    X = D.BandExchange(bands, rank, W, H, nk, mode, halo, "cuda:0", impl="abi", chroma_format=fmt)
                    side = torch.cuda.Stream()
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        X.run(planes)
                    torch.cuda.current_stream().wait_stream(side)
                    got = [p.cpu() for p in planes]
                    lo, hi = (0, H) if mode == "allgather" else (max(b0 - halo, 0), min(b1 + halo, H))
                    if b1 <= b0 and mode == "halo":
                        lo, hi = b0, b0
                    ok = True
                    for pl in range(3):
                        gv = got[pl][: nk * psz[pl]].view(nk, psz[pl])
                        for k in range(nk):
                            for r in range(H):
                                seg = gv[k, r * rb[pl]:(r + 1) * rb[pl]]
                                want = val(k, pl, r) if lo <= r < hi else torch.full_like(seg, 0xEE)
                                ok &= bool(torch.equal(seg, want))
                        ok &= bool((got[pl][nk * psz[pl]:] == 0xEE).all())
                    sent, recvd, transfers = X.grp.stats()
                    ok &= recvd == X.bytes_in() and transfers == len(X.need) + len(X.give)
                    ok &= X.bytes_in() == nk * sum(rb) * sum(n1 - n0 for n0, n1 in X.need.values())
                    X.grp.close()
                    if not ok:
                        bad.append((fmt, starts, mode, halo))
        q.put((rank, bad))
    finally:
        dist.destroy_process_group()


def _spawn(target, world=2):
    import torch.multiprocessing as mp
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=100) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


def test_gpu_group_device_planes_formats():
    res = _spawn(_planes_worker)
    assert [r[1] for r in res] == [[], []]


def _max_abs_mvy(p) -> int:
    used = p.ref_idx >= 0
    if not used.any():
        return 0
    my = (p.mv >> 16).astype(np.uint16).view(np.int16).reshape(p.mv.shape)
    return int(np.abs(my[used].astype(np.int32)).max())


def _chain_worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    import _oracle as O
    import h264r
    from h264r import _abi as A
    from h264r import batch as B
    from h264r import dist as D
    from h264r import synth
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        L = h264r.lib()
        W, H, slack = 22, 18, 64
        out = []
        for name, fmt, mbaff, mode in CHAINS:
            common = dict(num_slices=3, deblock_idc=2, seed=0x51CE + fmt)
            if mbaff:
                common["structure"] = A.MBAFF_FRAME
            if fmt != 1:
                common["chroma_format"] = fmt
            icfg = synth.default_cfg(L, 2, W, H, **common)
            pcfg = synth.default_cfg(L, 3, W, H, num_refs=1, mv_range_y=8, intra_permille=150, **common)
            chain = [synth.picture(L, icfg, 0), synth.picture(L, pcfg, 1), synth.picture(L, pcfg, 2)]
            for p in chain[1:]:
                assert (p.slices["ref_slot"][:, 0, 0] == 0).all()         # the one reference is DPB slot 0
                if mbaff:
                    assert (p.mbs["flags"] & A.MBF_FIELD).any()
            srow = chain[0].mbs["slice"].reshape(H, W)[:, 0]
            starts = [0] + [r for r in range(1, H) if srow[r] != srow[r - 1]]
            bands = D.slice_bands(starts, H, world)
            b0, b1 = bands[rank]
            m = max(_max_abs_mvy(p) for p in chain[1:])
            halo = D.halo_mb_rows(m, mbaff=mbaff) if mode == "halo" else 0
            # the oracle's chain of whole pictures
            want = [O.decode(chain[0], [])]
            for p in chain[1:]:
                want.append(O.decode(p, [want[-1]]))
            cw, ch = A.chroma_mb(fmt)
            psz = [256 * W * H, cw * ch * W * H, cw * ch * W * H]
            rows_pl = [16, ch, ch]
            X = D.BandExchange(bands, rank, W, H, 1, mode, halo, "cuda:0", impl="abi", chroma_format=fmt)
            dec = h264r.Decoder(0, 32, 32, chroma_format=fmt)
            ok, prev, keep = True, None, []
            lo, hi = (0, H) if mode == "allgather" else (max(b0 - halo, 0), min(b1 + halo, H))
            try:
                for t, p in enumerate(chain):
                    planes = [torch.full((psz[k] + slack,), MARK, dtype=torch.uint8, device="cuda:0") for k in range(3)]
                    tab = np.zeros(3 * A.MAX_SLOTS, np.int64)
                    if prev is not None:
                        tab[:3] = [x.data_ptr() for x in prev]
                    dtab = torch.from_numpy(tab).to("cuda:0")
                    db = B.to_device(B.pack([p], h264r.quant_flat()), 1, dtab.data_ptr())
                    db.batch.out_y, db.batch.out_u, db.batch.out_v = (x.data_ptr() for x in planes)
                    assert db.batch.mbaff == int(mbaff)
                    dec.decode_batch(db.batch, rows=(b0, b1))
                    dec.check()
                    X.run(planes)
                    torch.cuda.synchronize()
                    got = [x.cpu().numpy() for x in planes]
                    for k in range(3):
                        n = rows_pl[k]
                        if not n:
                            continue
                        g = got[k][:psz[k]].reshape(n * H, -1)
                        w = want[t][k]
                        ok &= bool(np.array_equal(g[b0 * n:b1 * n], w[b0 * n:b1 * n]))          # this rank's band
                        ok &= bool(np.array_equal(g[lo * n:hi * n], w[lo * n:hi * n]))          # and the rows received
                        ok &= bool((g[:lo * n] == MARK).all() and (g[hi * n:] == MARK).all())   # nothing else
                        ok &= bool((got[k][psz[k]:] == MARK).all())
                    keep.append((planes, dtab, db))
                    prev = planes
            finally:
                dec.close()
                X.grp.close()
            out.append((name, bool(ok), halo, m))
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_gpu_chain_rehearsal_two_ranks():
    from h264r import dist as D
    res = _spawn(_chain_worker)
    for rank, out in res:
        assert [o[0] for o in out] == [c[0] for c in CHAINS]
        for name, ok, halo, m in out:
            assert ok, f"rank {rank}, chain '{name}' (halo {halo} MB rows, max |mv_y| {m}) differs from the oracle's chain"
    # the MBAFF halo is the field MBs' reach, beyond the frame formula's for these vectors
    (_, _, halo, m) = res[0][1][0]
    assert halo == D.halo_mb_rows(m, mbaff=True) > D.halo_mb_rows(m)
