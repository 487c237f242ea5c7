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
from extremes import PK_RES_MAX, wave_paths

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
# (which path a wave takes: extremes.wave_paths, shared with the directed extreme-value cases of
# tests/extremes.py, which place blocks exactly at the bound)
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
                for lu, ch in wave_paths(synth.picture(L, cfg, i), quant):
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
