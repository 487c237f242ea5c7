"""k_inter4r's packed 16-bit residual with its 32-bit fallback, and the one-list deblocking records
(csrc/mb_inter4.h): synthetic pictures decoded in one batch, every plane byte-equal to the oracle's
decode (the method of test_gpu_parity._batch_vs_oracle).

The shapes are the smallest that reach every branch: 5 x 3 MBs is 15 MBs per picture, so the last
wave of a picture has one invalid group of lanes and the last 16-MB group is partial.  Which path a
wave takes depends on its data (sum |d| of each block's dequantised coefficients against
PK_RES_MAX = 32700), so test_guard_coverage works the test out on the host for the same pictures
and asserts that waves of both kinds are among them.
"""
import numpy as np
import pytest

import _oracle as O
import h264r
from h264r import _abi as A
from h264r import batch as B
from h264r import synth

PK_RES_MAX = 32700

# config 3 (P pictures, 4x4 transform) at 5 x 3 MBs, 6 pictures: the lower QP ranges take the packed
# path, the upper ones the fallback (single coefficients past int16), 38..46 mixes waves of both
QP_RANGES = [(0, 12), (20, 40), (38, 46), (44, 51), (51, 51)]
W3, H3, N3 = 5, 3, 6


@pytest.fixture(scope="module")
def L():
    h264r.build()
    return h264r.lib()


@pytest.fixture(scope="module")
def dec(L):
    d = h264r.Decoder(0, 16, 16)
    yield d
    d.close()


DEBLOCKS = (A.DBG_DEBLOCK_MB, A.DBG_DEBLOCK_ROWS, A.DBG_DEBLOCK_MB | A.DBG_DEBLOCK_GLOBAL, A.DBG_DEBLOCK_SPLIT)


def _first_diff(a, b, n):
    bad = np.argwhere(a != b)
    if not len(bad):
        return None
    y, x = bad[0]
    return f"{len(bad)} samples differ, first at (x={x}, y={y}) MB ({x // n}, {y // n}): gpu={a[y, x]} want={b[y, x]}"


def _batch_vs_oracle(L, dec, cidx, W, H, n, deblocks=(A.DBG_DEBLOCK_ROWS,), qm=None, **over):
    cfg = synth.default_cfg(L, cidx, W, H, **over)
    pics = [synth.picture(L, cfg, i) for i in range(n)]
    refs = synth.refpics(L, cfg)
    for s, (y, u, v) in enumerate(refs):
        dec.set_ref(s, y, u, v)
    lists = O.qmatrix(qm) if qm is not None else None
    host = B.pack(pics, h264r.quant_lists(*lists) if lists else h264r.quant_flat())
    want = [O.decode(p, refs, quant=O.quant_lists(*lists) if lists else None) for p in pics]
    for db_flag in deblocks:
        db = B.to_device(host, n, None)
        dec.set_debug(db_flag)
        try:
            dec.decode_batch(db.batch)
            dec.check()
        finally:
            dec.set_debug(0)
        for i in range(n):
            got = db.planes(i)
            for k in range(3):
                d = _first_diff(got[k], want[i][k], 16 if k == 0 else 8)
                assert d is None, f"deblock flag {db_flag} picture {i} plane {k}: {d}"


# ---------------------------------------------------------------- the guard, on the host
def _dq4(lev, scale, per):
    return ((int(lev) * int(scale) << per) + 8) >> 4


def _wave_paths(p, quant):
    """Per wave of k_inter4r (four consecutive MBs of the picture) which residual path its luma and
    its chroma take: 'packed', 'fallback' or None (no coded residual, or a path without the test).
    Mirrors luma_res_4x4 / inter4_chroma_residual: the lanes of intra, PCM and lossless MBs take no part in the test."""
    s4 = quant["scale4x4"]
    out = []
    nmb = len(p.mbs)
    for a0 in range(0, nmb, 4):
        luma_sums, chroma_sums, t8_any, luma_coded, chroma_coded = [], [], False, False, False
        for m in p.mbs[a0:a0 + 4]:
            flags, cbp = int(m["flags"]), int(m["cbp"])
            if flags & A.MBF_INTRA:
                continue
            cbpl, cbpc = cbp & 15, cbp >> 4
            luma_coded |= cbpl != 0
            chroma_coded |= cbpc != 0
            if flags & A.MBF_BYPASS:
                continue
            t8_any |= bool(flags & A.MBF_T8x8)
            lv = p.levels[int(m["coef_off"]):]
            off = 0
            qpl = int(m["qp_scaled"][0])
            for b8 in range(4):
                if not (cbpl >> b8) & 1:
                    continue
                if not flags & A.MBF_T8x8:
                    for k in range(4):
                        blk = lv[off + k * 16: off + k * 16 + 16]
                        luma_sums.append(sum(abs(_dq4(blk[i], s4[1][0][qpl % 6][i], qpl // 6)) for i in range(16)))
                off += 64
            cac = off if cbpc == 2 else -1
            off += 128 if cbpc == 2 else 0
            cdc = off                      # (an inter MB has no luma DC block)
            if cbpc:
                for cb in range(4):
                    quad = np.zeros((2, 4), np.int64)      # [plane][quadrant of the 4x4 block]
                    for pl in range(2):
                        qpc = int(m["qp_scaled"][1 + pl])
                        sc, per = s4[1][1 + pl][qpc % 6], qpc // 6
                        c = [int(x) for x in lv[cdc + pl * 4: cdc + pl * 4 + 4]]
                        f = (c[0] + c[1] + c[2] + c[3], c[0] - c[1] + c[2] - c[3],
                             c[0] + c[1] - c[2] - c[3], c[0] - c[1] - c[2] + c[3])[cb]
                        for pos in range(16):
                            if pos == 0:
                                v = ((f * int(sc[0])) << per) >> 5
                            elif cbpc == 2:
                                v = _dq4(lv[cac + pl * 64 + cb * 16 + pos], sc[pos], per)
                            else:
                                v = 0
                            quad[pl][(pos // 8) * 2 + (pos % 4) // 2] += abs(v)
                    # the kernel's measure: over the block's four lanes, the larger plane sum of each
                    chroma_sums.append(int(np.maximum(quad[0], quad[1]).sum()))

        def path(coded, sums, blocked):
            if not coded or blocked or not sums:
                return None
            return "packed" if max(sums) <= PK_RES_MAX else "fallback"
        out.append((path(luma_coded, luma_sums, t8_any), path(chroma_coded, chroma_sums, False)))
    return out


QM_RANGES = [(20, 40), (44, 51)]
QM_SEED = 21


def test_guard_coverage(L):
    """Among the config-3 pictures of test_gpu_p_qp_ranges and test_gpu_p_scaling_lists there are
    waves whose every block passes the range test (the packed transforms run) and waves with a
    failing block (the 32-bit code runs), for luma and for chroma: neither path can go untested
    silently.  No GPU needed."""
    flat, lists = h264r.quant_flat()[0], h264r.quant_lists(*O.qmatrix(QM_SEED))[0]
    count = {(pl, kind): 0 for pl in ("luma", "chroma") for kind in ("packed", "fallback")}
    per_case = {}
    for quant, ranges in ((flat, QP_RANGES), (lists, QM_RANGES)):
        for qp in ranges:
            cfg = synth.default_cfg(L, 3, W3, H3, qp_min=qp[0], qp_max=qp[1])
            n = {"packed": 0, "fallback": 0}
            for i in range(N3):
                for lu, ch in _wave_paths(synth.picture(L, cfg, i), quant):
                    for pl, kind in (("luma", lu), ("chroma", ch)):
                        if kind:
                            count[(pl, kind)] += 1
                            n[kind] += 1
            per_case[(quant is lists, qp)] = n
    print(count, per_case)
    assert all(v > 0 for v in count.values()), count
    # flat lists: below QP 12 no block can fail (16 coefficients of at most 8 * 29 * 4), and the
    # middle range has waves of both kinds
    assert per_case[(False, (0, 12))]["fallback"] == 0, per_case
    assert per_case[(False, (38, 46))]["packed"] > 0 and per_case[(False, (38, 46))]["fallback"] > 0, per_case


# ---------------------------------------------------------------- GPU parity
@pytest.mark.gpu
@pytest.mark.parametrize("qp", QP_RANGES, ids=lambda q: f"qp{q[0]}-{q[1]}")
def test_gpu_p_qp_ranges(L, dec, qp):
    _batch_vs_oracle(L, dec, 3, W3, H3, N3, qp_min=qp[0], qp_max=qp[1])


@pytest.mark.gpu
@pytest.mark.parametrize("qp", QM_RANGES, ids=lambda q: f"qp{q[0]}-{q[1]}")
def test_gpu_p_scaling_lists(L, dec, qp):
    """Explicit scaling lists: the scales are not flat, and larger."""
    _batch_vs_oracle(L, dec, 3, W3, H3, N3, qm=QM_SEED, qp_min=qp[0], qp_max=qp[1])


@pytest.mark.gpu
@pytest.mark.parametrize("wp_mode", [1, 2], ids=["explicit", "implicit"])
def test_gpu_b_mixed_transform(L, dec, wp_mode):
    """Config 4 at 6 x 4 MBs: B pictures (the two-list records, waves mixing one-list and two-list
    lanes), High 8x8 mixed with 4x4 (the 32-bit luma paths feeding the packed construction),
    weighted prediction; under all four deblocking schedules, since the records feed the walk."""
    _batch_vs_oracle(L, dec, 4, 6, 4, 4, deblocks=DEBLOCKS, wp_mode=wp_mode)


@pytest.mark.gpu
def test_gpu_p_lossless_pcm(L, dec):
    """Lossless and PCM MBs in the same waves as packed ones."""
    _batch_vs_oracle(L, dec, 3, W3, H3, N3, qp_min=0, qp_max=30, lossless_permille=300, pcm_permille=100,
                     intra_permille=300)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(9, 1), (1, 7)])
def test_gpu_p_no_neighbour(L, dec, W, H):
    """No upper MB in one, no left MB in the other: the edge-0 records' degenerate branches."""
    _batch_vs_oracle(L, dec, 3, W, H, N3)
