"""The host half of the deinterlacer (include/h264r_deinterlace.h): the exports, the layout of its
structures, h264r_deinterlace_geometry against h264r_output_geometry and its refusals in their order,
h264r_deint_job_status; and the restatement itself (tests/deint_restate.py): its two forms against each
other, its properties, what the GPU tests' inputs exercise, and the mutations they can tell apart.  No GPU
is needed.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import deint_restate as D
import h264r
from h264r import _abi as A
from h264r import output as OUT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _desc(W=11, H=8, crop=OUT.Crop(frame_mbs_only=0), layout=OUT.PLANAR, align=0, fake=False):
    return OUT._desc(W, H, crop, layout, align, fake)


def _status(desc, fmt=1):
    return h264r.lib().h264r_deinterlace_geometry(fmt, C.byref(desc) if desc is not None else None, C.byref(OUT.DeintGeom()))


# ------------------------------------------------------------------------------ the ABI
def test_library_exports_the_entry_points():
    L = h264r.lib()
    for name in ("h264r_deinterlace_geometry", "h264r_deint_job_status", "h264r_deinterlace"):
        assert hasattr(L, name), name


def test_struct_layout_and_constants_match_c():
    job = ["cur", "prev", "next", "keep", "second", "mode"]
    geom = ["rect", "plane_off", "plane_pitch", "frame_bytes"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "h264r_deinterlace.h"\nint main(void) {\n'
           '  printf("%zu %zu %d %d %d %d %d\\n", sizeof(h264r_deint_job), sizeof(h264r_deint_geom), H264R_DEINT_BOB, '
           'H264R_DEINT_ADAPTIVE, H264R_DEINT_TILE_W, H264R_DEINT_TILE_H, H264R_ABI_VERSION);\n'
           + "".join(f'  printf("%zu\\n", offsetof(h264r_deint_job, {n}));\n' for n in job)
           + "".join(f'  printf("%zu\\n", offsetof(h264r_deint_geom, {n}));\n' for n in geom) + "  return 0; }\n")
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "l.c")
        with open(c, "w") as f:
            f.write(src)
        exe = os.path.join(td, "l")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        v = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert v[:6] == [C.sizeof(OUT.DeintJob), C.sizeof(OUT.DeintGeom), OUT.DEINT_BOB, OUT.DEINT_ADAPTIVE, OUT.DEINT_TILE_W,
                     OUT.DEINT_TILE_H]
    assert v[0] == 24 == OUT.DEINT_JOB_DTYPE.itemsize and v[6] == A.ABI_VERSION
    assert v[7:13] == [getattr(OUT.DeintJob, n).offset for n in job] == [OUT.DEINT_JOB_DTYPE.fields[n][1] for n in job]
    assert v[13:] == [getattr(OUT.DeintGeom, n).offset for n in geom]
    assert (D.BOB, D.ADAPTIVE) == (OUT.DEINT_BOB, OUT.DEINT_ADAPTIVE)


# ------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_geometry_is_the_output_stages_rectangle_in_coded_size_planes(fmt):
    cw, ch = A.chroma_mb(fmt)
    for W, H, crop in [(11, 8, OUT.Crop(frame_mbs_only=0)), (120, 68, OUT.Crop(0, 0, 0, 2, frame_mbs_only=0)),
                       (3, 2, OUT.Crop(1, 2, 1, 1, frame_mbs_only=0)), (5, 4, OUT.Crop(3, 1, 2, 4, frame_mbs_only=1))]:
        g = OUT.deint_geometry(_desc(W, H, crop), fmt)
        og = OUT.device_geometry(W, H, crop, fmt)
        assert g.rect[0] == og.luma
        assert g.rect[1] == g.rect[2] == (og.chroma if fmt else (0, 0, 0, 0))
        sizes = [(16 * W, 16 * H)] + ([(cw * W, ch * H)] * 2 if fmt else [])
        off = 0
        for k in range(3):
            if k < len(sizes):
                assert (g.plane_off[k], g.plane_pitch[k]) == (off, sizes[k][0])
                off += sizes[k][0] * sizes[k][1]
            else:
                assert (g.plane_off[k], g.plane_pitch[k]) == (0, 0)
        assert g.frame_bytes == off
        rects, roff, rpitch, rrows, total = D.layout(W, H, crop, fmt)
        assert (list(g.rect[:len(rects)]), list(g.plane_off[:len(rects)]), list(g.plane_pitch[:len(rects)]), g.frame_bytes) == \
               ([tuple(r) for r in rects], roff, rpitch, total)


def test_host_statuses_in_their_order():
    ok = _desc()
    assert _status(ok) == A.OK
    # whatever h264r_output_geometry refuses
    assert _status(None) == A.EINVAL
    assert h264r.lib().h264r_deinterlace_geometry(1, C.byref(ok), None) == A.EINVAL
    assert _status(ok, 4) == A.EINVAL and _status(ok, -1) == A.EINVAL
    for bad in (_desc(0, 8), _desc(11, 0), _desc(1025, 8), _desc(11, 8, OUT.Crop(-1, 0, 0, 0, 0)), _desc(11, 8, OUT.Crop(88, 0, 0, 0, 0)),
                _desc(11, 8, OUT.Crop(0, 0, 0, 0, 2)), _desc(layout=7), _desc(align=3), _desc(align=-2), _desc(align=8192)):
        assert _status(bad) == A.EINVAL
        og = h264r.lib().h264r_output_geometry(1, C.byref(bad), C.byref(OUT.OutGeom()))
        assert og == A.EINVAL
    # and what the output stage accepts but this call does not
    for fmt in (0, 1, 2, 3):
        assert _status(_desc(layout=OUT.SEMIPLANAR), fmt) == A.EINVAL
        assert _status(_desc(align=2), fmt) == A.EINVAL and _status(_desc(align=64), fmt) == A.EINVAL
        assert _status(_desc(align=1), fmt) == A.OK
        assert _status(_desc(fake=True), fmt) == A.EINVAL          # the output stage: H264R_EUNSUPPORTED off 4:0:0
    # H264R_EUNSUPPORTED after those: frame_mbs_only 1 and an odd crop
    odd = OUT.Crop(0, 0, 1, 0, frame_mbs_only=1)
    assert _status(_desc(11, 8, odd), 1) == A.EUNSUPPORTED         # 4:2:0: chroma y0 = 1
    assert _status(_desc(11, 8, OUT.Crop(0, 0, 0, 1, frame_mbs_only=1)), 1) == A.EUNSUPPORTED   # chroma height 63
    assert _status(_desc(11, 8, OUT.Crop(0, 0, 2, 2, frame_mbs_only=1)), 1) == A.OK
    assert _status(_desc(11, 8, odd), 3) == A.EUNSUPPORTED and _status(_desc(11, 8, odd), 0) == A.EUNSUPPORTED
    assert _status(_desc(11, 8, OUT.Crop(0, 0, 1, 1, frame_mbs_only=1)), 3) == A.EUNSUPPORTED   # y0 odd, height even
    for layout, align, fake in ((OUT.SEMIPLANAR, 0, False), (OUT.PLANAR, 64, False), (OUT.PLANAR, 0, True), (OUT.PLANAR, 3, False)):
        assert _status(_desc(11, 8, odd, layout, align, fake), 1) == A.EINVAL                    # an argument error comes first
    assert _status(_desc(0, 8, odd), 1) == A.EINVAL
    # never with frame_mbs_only 0
    for fmt in (0, 1, 2, 3):
        for t, b in ((1, 0), (0, 1), (3, 2)):
            assert _status(_desc(11, 8, OUT.Crop(1, 1, t, b, frame_mbs_only=0)), fmt) == A.OK
    with pytest.raises(h264r.H264RError) as e:
        OUT.deint_geometry(_desc(11, 8, odd), 1)
    assert e.value.status == A.EUNSUPPORTED


def test_the_call_refuses_its_arguments_before_it_needs_a_device():
    """NULL pointers and negative counts are refused before the context is used at all."""
    L = h264r.lib()
    d = _desc()
    one = C.c_void_p(16)
    assert L.h264r_deinterlace(None, C.byref(d), one, 1, one, 1, one, 1 << 20, None) == A.EINVAL


def test_job_status_rules():
    st = lambda job, n=4: OUT.deint_job_status(job, n)
    assert st((0, -1, -1, 0, 0, OUT.DEINT_BOB)) == A.OK and st((3, 3, 3, 1, 1, OUT.DEINT_ADAPTIVE)) == A.OK
    assert st((2, 1, 3, 1, 0, OUT.DEINT_ADAPTIVE)) == A.OK
    assert st((4, -1, -1, 0, 0, 0)) == A.EINVAL and st((-1, -1, -1, 0, 0, 0)) == A.EINVAL       # cur
    assert st((0, -2, -1, 0, 0, 0)) == A.EINVAL and st((0, 4, -1, 0, 0, 0)) == A.EINVAL         # prev
    assert st((0, -1, -2, 0, 0, 0)) == A.EINVAL and st((0, -1, 4, 0, 0, 0)) == A.EINVAL         # next
    assert st((0, -1, -1, 2, 0, 0)) == A.EINVAL and st((0, -1, -1, -1, 0, 0)) == A.EINVAL       # keep
    assert st((0, -1, -1, 0, 2, 0)) == A.EINVAL and st((0, -1, -1, 0, -1, 0)) == A.EINVAL       # second
    assert st((0, -1, -1, 0, 0, 2)) == A.EINVAL and st((0, -1, -1, 0, 0, -1)) == A.EINVAL       # mode
    assert st((0, -1, -1, 0, 0, 0), 0) == A.EINVAL and st((0, -1, -1, 0, 0, 0), -1) == A.EINVAL
    assert h264r.lib().h264r_deint_job_status(None, 4) == A.EINVAL
    assert st(OUT.DeintJob(1, 0, 2, 1, 1, 1)) == A.OK and st(OUT.deint_jobs(4)[3]) == A.OK


def test_the_usual_job_lists():
    t = OUT.deint_jobs(3, tff=True, mode=OUT.DEINT_ADAPTIVE)
    assert [tuple(int(v) for v in r) for r in t] == [(0, -1, 1, 0, 0, 1), (1, 0, 2, 0, 0, 1), (2, 1, -1, 0, 0, 1)]
    t = OUT.deint_jobs(2, tff=False, mode=OUT.DEINT_BOB, field_rate=True)
    assert [tuple(int(v) for v in r) for r in t] == [(0, -1, 1, 1, 0, 0), (0, -1, 1, 0, 1, 0), (1, 0, -1, 1, 0, 0), (1, 0, -1, 0, 1, 0)]
    assert len(OUT.deint_jobs(0)) == 0
    for r in OUT.deint_jobs(5, field_rate=True):
        assert OUT.deint_job_status(r, 5) == A.OK
    assert np.array_equal(OUT.deint_job_table([tuple(int(v) for v in r) for r in t]), t)


# ------------------------------------------------------------------------------ the restatement
def _fields(rng, Hf, w):
    return tuple(rng.integers(0, 256, (Hf, w)).astype(np.int32) for _ in range(2))


@pytest.mark.parametrize("Hf,w", [(1, 1), (1, 2), (2, 5), (6, 22), (13, 43)])
def test_the_two_forms_agree(Hf, w):
    rng = np.random.default_rng(100 * Hf + w)
    C_, P, N = _fields(rng, Hf, w), _fields(rng, Hf, w), _fields(rng, Hf, w)
    for keep in (0, 1):
        for second in (0, 1):
            for mode in (D.BOB, D.ADAPTIVE):
                for PP, NN in ((P, N), (None, N), (P, None), (None, None), (C_, C_)):
                    a = D.plane(C_, PP, NN, keep, second, mode, D.interp_scalar)
                    b = D.plane(C_, PP, NN, keep, second, mode, D.interp_numpy)
                    assert np.array_equal(a, b), (keep, second, mode)


def test_kept_rows_are_copied_and_flat_frames_come_back():
    rng = np.random.default_rng(5)
    Hf, w = 7, 19
    C_, P, N = _fields(rng, Hf, w), _fields(rng, Hf, w), _fields(rng, Hf, w)
    for keep in (0, 1):
        for mode in (D.BOB, D.ADAPTIVE):
            out = D.plane(C_, P, N, keep, 0, mode)
            assert np.array_equal(out[keep::2], C_[keep])
    # a frame whose rows are all equal (and its neighbours in time, whatever they hold in BOB): unchanged
    row = rng.integers(0, 256, w).astype(np.int32)
    flat = (np.tile(row, (Hf, 1)), np.tile(row, (Hf, 1)))
    for keep in (0, 1):
        for second in (0, 1):
            assert np.array_equal(D.plane(flat, P, N, keep, second, D.BOB), np.tile(row, (2 * Hf, 1)))
            for PP, NN in ((flat, flat), (None, None), (None, flat)):
                assert np.array_equal(D.plane(flat, PP, NN, keep, second, D.ADAPTIVE), np.tile(row, (2 * Hf, 1)))


@pytest.mark.parametrize("k", range(len(D.CASES)))
def test_frame_and_field_pair_namings_agree(k):
    fmt, W, H, c = D.CASES[k]
    crop = OUT.Crop(*c[:4], frame_mbs_only=c[4])
    table = D.case_table(k)
    total = D.layout(W, H, crop, fmt)[4]
    for a, b in (((1, 0, 2, 0, 0, 1), (4, 5, 2, 0, 0, 1)), ((1, 0, 2, 1, 1, 1), (4, 0, 2, 1, 1, 1)), ((1, 0, 2, 0, 0, 1), (1, 5, 2, 0, 0, 1)),
                 ((1, -1, -1, 1, 0, 0), (4, -1, -1, 1, 0, 0))):
        x, y = np.full(total, 0xA5, np.uint8), np.full(total, 0xA5, np.uint8)
        assert D.frame(a, table, W, H, crop, fmt, x) == total == D.frame(b, table, W, H, crop, fmt, y)
        assert np.array_equal(x, y)
    # only the rectangle is written
    rects, off, pitch, rows, _ = D.layout(W, H, crop, fmt)
    inside = np.zeros(total, bool)
    for r, o, p, n in zip(rects, off, pitch, rows):
        inside[o:o + p * n].reshape(n, p)[r[1]:r[1] + r[3], r[0]:r[0] + r[2]] = True
    assert np.all(x[~inside] == 0xA5)


# ------------------------------------------------------------------------------ what the GPU tests' inputs exercise
def _case_stats(k, job):
    """Per plane of case k under an ADAPTIVE job: the stats of deint_restate.interp_numpy."""
    fmt, W, H, c = D.CASES[k]
    crop = OUT.Crop(*c[:4], frame_mbs_only=c[4])
    table = D.case_table(k)
    cur, prev, nxt, keep, second, mode = job
    res = []
    for p, rect in enumerate(D.layout(W, H, crop, fmt)[0]):
        both = lambda i: tuple(D.field(table[i][0], [s[p] for s in table[i][1]], f, rect) for f in (0, 1))
        st = {}
        D.plane(both(cur), both(prev) if prev >= 0 else None, both(nxt) if nxt >= 0 else None, keep, second, mode, stats=st)
        res.append(st)
    return res


def _shares(stats):
    n = sum(s["dir"].size for s in stats)
    out = {("dir", d): sum(int((s["dir"] == d).sum()) for s in stats) / n for d in (0, -1, -2, 1, 2)}
    out.update({("clamp", v): sum(int((s["clamp"] == v).sum()) for s in stats) / n for v in (-1, 0, 1)})
    out[("raised",)] = sum(int(s["raised"].sum()) for s in stats) / n
    return out, n


def test_noise_reaches_every_branch_of_the_definition():
    """Each of the five directions, each outcome of the last line and a diff raised by the mn / -mx line on
    at least 3 % of the interpolated samples: over all the GPU tests' planes together, and on each of their
    planes that has 200 samples or more.  Noise alone meets the floor: over all planes together the rarest
    outcomes are the +2 direction (8 %) and a raised diff (6 %)."""
    every = []
    for k in range(len(D.CASES)):
        for job in ((1, 0, 2, 0, 0, 1), (1, 0, 2, 1, 1, 1)):
            stats = _case_stats(k, job)
            every += stats
            for s in stats:
                if s["dir"].size >= 200:
                    shares, n = _shares([s])
                    assert min(shares.values()) >= 0.03, (k, job, n, shares)
    shares, n = _shares(every)
    print(n, shares)
    assert n > 20000 and min(shares.values()) >= 0.03, shares


@pytest.mark.parametrize("mutate", D.MUTATIONS)
def test_mutations_differ_on_the_same_inputs(mutate):
    """On the GPU tests' own tables and jobs every mutated restatement gives other bytes than the true one:
    in every case that is large enough to show it, and in the narrowest and lowest ones where the mutation
    is about an edge."""
    differ = 0
    for k, (fmt, W, H, c) in enumerate(D.CASES):
        crop = OUT.Crop(*c[:4], frame_mbs_only=c[4])
        table = D.case_table(k)
        lw, lh = D.layout(W, H, crop, fmt)[0][0][2:]
        total = D.layout(W, H, crop, fmt)[4]
        jobs = [j for j in D.case_jobs() if j[5] == D.ADAPTIVE and (mutate != "zeros" or j[1] < 0 or j[2] < 0)]
        for job in jobs:
            x, y = np.full(total, 0xA5, np.uint8), np.full(total, 0xA5, np.uint8)
            D.frame(job, table, W, H, crop, fmt, x)
            D.frame(job, table, W, H, crop, fmt, y, mutate=mutate)
            same = np.array_equal(x, y)
            differ += not same
            prev_is_cur = job[1] in (-1, job[0]) and job[2] in (-1, job[0])     # P = C = N: `second` names the same fields
            if lw >= 30 and lh >= 28 and not (mutate == "second" and prev_is_cur):
                assert not same, (mutate, k, job)
    assert differ >= len(D.CASES)
