"""bench.py's roofline numerator: the per-kernel algorithmic bytes (kernel_bytes) partition
the SURVEY 8(d) total (h264r_synth_algo_bytes) with no byte counted twice: the MBs' R
between the inter and intra kernels, their W (384 B per MB) to deblocking."""
import os
import sys

import pytest

from h264r import synth
import h264r

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


@pytest.mark.parametrize("cidx", [2, 3, 4])
def test_kernel_bytes_partition_the_algorithmic_total(cidx):
    L = h264r.lib()
    cfg = synth.default_cfg(L, cidx, 11, 9)
    pics = [synth.picture(L, cfg, i) for i in range(3)]
    total = sum(sum(synth.algo_bytes(L, p)) for p in pics)
    inter, intra, deblock = bench.kernel_bytes(pics, 11 * 9)
    assert inter + intra + deblock == total
    assert deblock == 3 * 11 * 9 * 384
    assert (intra > 0) and (cidx == 2 or inter > 0)


def test_packed_chunks_are_the_whole_pack():
    """bench.py sets its batch up in chunks (packed_chunks): the chunks one after the other, each
    one's level-pool offsets moved by the levels before it (as chunks_to_device lays them out on the
    device), are byte for byte batch.pack of the whole list; the byte counts add up the same."""
    import numpy as np
    from h264r import batch as B
    L = h264r.lib()
    cfg = synth.default_cfg(L, 3, 11, 9)
    index = list(range(2 * bench.SETUP_CHUNK + 3))          # two whole chunks and a short one
    pics = [synth.picture(L, cfg, i) for i in index]
    whole = B.pack(pics, h264r.quant_flat())
    chunks = bench.packed_chunks(L, cfg, index, True)
    assert len(chunks) == 3
    off = 0
    for c in chunks:
        c["host"]["mbs"]["coef_off"] += off
        off += len(c["host"]["levels"])
    for k in ("mbs", "levels", "mv", "ref_idx", "slices", "pics", "quant"):
        got = np.concatenate([np.ascontiguousarray(c["host"][k]).view(np.uint8).reshape(-1) for c in chunks])
        assert np.array_equal(got, np.ascontiguousarray(whole[k]).view(np.uint8).reshape(-1)), k
    assert [sum(c["kbytes"][i] for c in chunks) for i in range(3)] == bench.kernel_bytes(pics, 11 * 9)
    assert sum(c["rd"] + c["wr"] for c in chunks) == sum(sum(synth.algo_bytes(L, p)) for p in pics)
