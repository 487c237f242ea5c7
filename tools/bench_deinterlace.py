"""Bandwidth of the deinterlacer (include/h264r_deinterlace.h) against the output
stage's own copy, in one process: B interlaced frames of 120 x 68 MBs (1080i: frame_mbs_only 0,
frame_crop_bottom_offset 2 to 1080 rows) in 4:2:0, deinterlaced by h264r_deinterlace as ADAPTIVE at frame
rate (B jobs), ADAPTIVE at field rate (2 B jobs) and BOB (B jobs); and, as the yardstick, h264r_output_frames
writing the same table as woven planar frames, which moves 2 frames' bytes per frame.

A run is K back-to-back calls between two HIP events on one stream after W warm-up calls, nothing
synchronising inside; the figure of a measurement is the median of five runs, in ms per call.  The bytes/s
are over the ALGORITHMIC bytes, one frame being the cropped frame's bytes: 3.5 frames per ADAPTIVE job (five
fields read, one frame written), 1.5 per BOB job, 2 per frame of the yardstick.  The first and the last job
of each measurement are checked against tests/deint_restate.py first.

    python3 tools/bench_deinterlace.py [B] [K] [W]

One JSON line per measurement: {"what", "jobs", "ms", "ms_runs", "bytes", "gb_per_s"}, then a summary line
with each measurement's bytes/s relative to the yardstick's.  MEASUREMENT TOOL: off the headline metric
(bench.py does not run the output stage)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "arrow-h264_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import numpy as np
    import torch
    import h264r
    import deint_restate as D
    from h264r import output as OUT
    nframes = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    warm = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    W, H = 120, 68
    crop = OUT.Crop(0, 0, 0, 2, frame_mbs_only=0)
    h264r.lib()
    dec = h264r.Decoder(0, W, H)
    stream = torch.cuda.Stream()                              # a stream of its own: events and work on it alone
    torch.cuda.set_stream(stream)
    sp = stream.cuda_stream
    g = torch.Generator(device="cuda").manual_seed(1)
    y = torch.randint(0, 256, (nframes, 16 * H, 16 * W), dtype=torch.uint8, device="cuda", generator=g)
    u = torch.randint(0, 256, (nframes, 8 * H, 8 * W), dtype=torch.uint8, device="cuda", generator=g)
    v = torch.randint(0, 256, (nframes, 8 * H, 8 * W), dtype=torch.uint8, device="cuda", generator=g)
    out = OUT.DeviceOutput(dec, W, H, crop)
    table = out.frames_from([(OUT.OUT_FRAME, (y[i], u[i], v[i])) for i in range(nframes)])
    geom = OUT.geometry(W, H, crop)
    frame = geom.frame_bytes                                  # the cropped frame: 1920 x 1080 x 3 / 2
    assert geom.luma[2:] == (1920, 1080) and OUT.deint_geometry(out.desc).rect[0] == geom.luma
    host = {}

    def source(i):
        if i not in host:
            host[i] = (OUT.OUT_FRAME, [tuple(t[i].cpu().numpy() for t in (y, u, v))])
        return host[i]

    class Table:                                              # the frame table on the host, fetched as it is needed
        def __getitem__(self, i):
            return source(i)

    results = {}

    def timed(what, fn, njobs, nbytes):
        for _ in range(warm):
            fn()
        runs = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record(stream)
            for _ in range(steps):
                fn()
            b.record(stream)
            torch.cuda.synchronize()
            runs.append(a.elapsed_time(b) / steps)
        ms = statistics.median(runs)
        results[what] = nbytes / ms / 1e6
        print(json.dumps({"what": what, "jobs": njobs, "ms": ms, "ms_runs": runs, "bytes": nbytes, "gb_per_s": nbytes / ms / 1e6}),
              flush=True)

    cases = [("h264r_deinterlace adaptive, frame rate", OUT.deint_jobs(nframes, True, OUT.DEINT_ADAPTIVE), 3.5),
             ("h264r_deinterlace adaptive, field rate", OUT.deint_jobs(nframes, True, OUT.DEINT_ADAPTIVE, field_rate=True), 3.5),
             ("h264r_deinterlace bob", OUT.deint_jobs(nframes, True, OUT.DEINT_BOB), 1.5)]
    for what, jobs, per_job in cases:
        jt = torch.from_numpy(jobs.view(np.uint8).copy()).cuda()
        dst = out.deinterlace(table, jt, stream=sp)           # zero-filled: the 8 cropped rows stay 0
        dec.check()
        for j in (0, len(jobs) - 1):
            want = np.zeros(dst.shape[1], np.uint8)
            D.frame(tuple(jobs[j]), Table(), W, H, crop, 1, want)
            if not np.array_equal(dst[j].cpu().numpy(), want):
                raise SystemExit(f"bench_deinterlace: {what}: job {j} differs from tests/deint_restate.py")
        timed(what, lambda: out.deinterlace(table, jt, dst, stream=sp), len(jobs), int(per_job * frame * len(jobs)))
        del dst
    dst = torch.empty((nframes, frame), dtype=torch.uint8, device="cuda")
    timed("h264r_output_frames planar (yardstick)", lambda: out.run(table, dst=dst, stream=sp), nframes, 2 * frame * nframes)
    dec.check()
    base = results["h264r_output_frames planar (yardstick)"]
    print(json.dumps({"summary": "bytes/s over the algorithmic bytes, relative to h264r_output_frames in the same process",
                      **{k: v / base for k, v in results.items()}, "verified_vs_restatement": True}), flush=True)
    dec.close()


if __name__ == "__main__":
    main()
