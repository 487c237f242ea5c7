"""The Pillow-exact resampled RGB output stage (include/h264r_output.h: h264r_output_rgb_resampled,
DESIGN.md section 9d) against what a user does without it, by the method of tools/bench_output_rgb.py:
B pictures of 120 x 68 MBs (1080p) in 4:2:0, frame_crop_bottom_offset 4 to 1080 rows, BT.709 limited
range, replicate chroma, to 224 x 224 planar binary16 under each of the three filters.  Beside them, in
the same process:

    (a) h264r_output_rgb_scaled H264R_SCALE_AREA on the same job: the existing single-pass yardstick.
    (b) what a caller does today: h264r_output_rgb planar u8, then torch.nn.functional.interpolate
        (bicubic, antialiased) on the result, 128 pictures per call (converted with .float() first where
        torch has no 8-bit kernel for it; the label says which).  Its values are not compared with
        anything -- torch's bicubic is a = -0.75 and is not Pillow's -- only its time is taken.

HIP events on one stream around K back-to-back calls after W warm-up calls, nothing synchronising inside
the timed region; two runs (run 0, run 1), each going through all the candidates in turn; frames 0 and
B - 1 of every resampled variant are first checked against the restatement of the header
(tests/resample_restate.py).

    python3 tools/bench_output_resample.py [B] [K] [W]

One JSON line per measurement: {"what", "run", "pictures", "ms"}, then one summary line per run with the
ratios DESIGN.md section 9d quotes.
MEASUREMENT TOOL: off the headline metric (bench.py does not run the output stage)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "arrow-h264_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import numpy as np
    import torch
    import torch.nn.functional as F
    import h264r
    import resample_restate as RR
    import rgb_restate as R
    from h264r import output as OUT
    npics = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    warm = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    W, H = 120, 68
    crop = OUT.Crop.for_height(W, H, 1920, 1080)
    h264r.lib()
    dec = h264r.Decoder(0, W, H)
    stream = torch.cuda.Stream()                              # a stream of its own: events and work on it alone
    torch.cuda.set_stream(stream)
    sp = stream.cuda_stream
    g = torch.Generator(device="cuda").manual_seed(1)
    plane_bytes = npics * 384 * W * H
    planes = torch.randint(0, 256, (plane_bytes,), dtype=torch.uint8, device="cuda", generator=g)
    y = planes[:npics * 256 * W * H].view(npics, 256 * W * H)
    u = planes[npics * 256 * W * H:npics * 320 * W * H].view(npics, 64 * W * H)
    v = planes[npics * 320 * W * H:].view(npics, 64 * W * H)
    out = OUT.DeviceOutput(dec, W, H, crop)
    table = out.frames_from([(OUT.OUT_FRAME, (y[i], u[i], v[i])) for i in range(npics)])
    ow, oh = 224, 224
    filters = (("triangle", OUT.RESAMPLE_TRIANGLE), ("bicubic", OUT.RESAMPLE_BICUBIC), ("lanczos", OUT.RESAMPLE_LANCZOS))
    base = dict(matrix=OUT.CSC_BT709, full_range=False, chroma_up=OUT.UP_REPLICATE)
    format = OUT.RGB_PLANAR_F16

    def timed(what, run, fn):
        for _ in range(warm):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(stream)
        for _ in range(steps):
            fn()
        b.record(stream)
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / steps
        print(json.dumps({"what": what, "run": run, "pictures": npics, "ms": ms}), flush=True)
        return ms

    # the candidates, each with a destination of its own
    cands, plans = [], []
    for fname, filter in filters:
        plan = out.resample_plan(ow, oh, None, filter, format=format, **base)
        plans.append(plan)
        fb = plan.geom.frame_bytes
        dst = torch.full((npics, fb), 0xA5, dtype=torch.uint8, device="cuda")
        out.rgb_resampled(table, plan, dst=dst, stream=sp)
        dec.check()
        for i in (0, npics - 1):
            pl = [t[i].cpu().numpy() for t in (y, u, v)]
            pl = (pl[0].reshape(16 * H, 16 * W), pl[1].reshape(8 * H, 8 * W), pl[2].reshape(8 * H, 8 * W))
            want = np.zeros(fb, np.uint8)
            RR.frame(OUT.OUT_FRAME, [pl], W, H, crop, 1, want, ow, oh, filter=filter, matrix=R.BT709, format=format)
            if not np.array_equal(dst[i].cpu().numpy(), want):
                raise SystemExit(f"bench_output_resample: {fname} frame {i} differs from the restatement")
        cands.append((f"resampled {ow}x{oh} {fname} planar_f16",
                      lambda plan=plan, dst=dst: out.rgb_resampled(table, plan, dst=dst, stream=sp)))
    fb = OUT.scaled_geometry(OUT.scale_desc(OUT.rgb_desc(out.desc, format=format), ow, oh, None, OUT.SCALE_AREA), 1).frame_bytes
    area_dst = torch.empty((npics, fb), dtype=torch.uint8, device="cuda")
    cands.append((f"(a) scaled {ow}x{oh} area planar_f16",
                  lambda: out.rgb_scaled(table, ow, oh, filter=OUT.SCALE_AREA, format=format, dst=area_dst, stream=sp, **base)))
    full_u8 = torch.empty((npics, 3 * 1920 * 1080), dtype=torch.uint8, device="cuda")
    probe = torch.zeros((1, 3, 32, 32), dtype=torch.uint8, device="cuda")
    try:
        F.interpolate(probe, size=(8, 8), mode="bicubic", antialias=True, align_corners=False)
        as_input, how = (lambda t: t), "u8"
    except (RuntimeError, NotImplementedError):
        as_input, how = (lambda t: t.float()), "u8 -> .float()"
    torch.cuda.synchronize()

    def two_step():
        t = out.rgb(table, format=OUT.RGB_PLANAR_U8, dst=full_u8, stream=sp, **base)
        # slices of 128 pictures keep each call's tensor below 2^31 elements
        return [F.interpolate(as_input(t[k:k + 128]), size=(oh, ow), mode="bicubic", antialias=True, align_corners=False)
                for k in range(0, npics, 128)]
    cands.append((f"(b) h264r_output_rgb planar_u8 + interpolate bicubic antialias ({how}) {ow}x{oh}", two_step))
    cands.append(("(b1) h264r_output_rgb planar_u8 alone",
                  lambda: out.rgb(table, format=OUT.RGB_PLANAR_U8, dst=full_u8, stream=sp, **base)))

    results = [{}, {}]
    for run in (0, 1):
        for what, fn in cands:
            results[run][what] = timed(what, run, fn)
        dec.check()
    key = lambda r, head: next(r[k] for k in r if k.startswith(head))
    for run in (0, 1):
        r = results[run]
        s = {"summary": "ratios of times", "run": run}
        for fname, _ in filters:
            t = r[f"resampled {ow}x{oh} {fname} planar_f16"]
            s[f"{fname} / (a)"] = t / key(r, "(a)")
            s[f"{fname} / (b)"] = t / key(r, "(b) ")
        s["verified_vs_restatement"] = True
        print(json.dumps(s), flush=True)
    for plan in plans:
        plan.close()
    dec.close()


if __name__ == "__main__":
    main()
