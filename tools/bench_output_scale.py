"""The scaled RGB output stage (include/h264r_output.h: h264r_output_rgb_scaled)
against what a user does without it, by the method of tools/bench_output_rgb.py: B pictures of
120 x 68 MBs (1080p) in 4:2:0, frame_crop_bottom_offset 4 to 1080 rows, BT.709 limited range, replicate
chroma, scaled to 224 x 224 and to 960 x 540 with both filters as planar u8 and as planar binary16.
Beside them, in the same process:

    (a) h264r_output_rgb planar binary16 followed by torch.nn.functional.interpolate (bilinear,
        antialiased) on that tensor, 128 pictures per call, to 224 x 224 and to 960 x 540: the two-step
        path.  Its values are not compared with anything; only its time is taken.
    (b) h264r_output_rgb planar u8 alone, on the same table.
    (c) one device-to-device hipMemcpyAsync of the bytes the planes hold: the read roof.

HIP events on one stream around K back-to-back calls after W warm-up calls, nothing synchronising
inside the timed region; two runs (run 0, run 1), each going through all the candidates in turn; frames
0 and B - 1 of every scaled variant are first checked against the numpy restatement of the header
(tests/scale_restate.py).

    python3 tools/bench_output_scale.py [B] [K] [W]

One JSON line per measurement: {"what", "run", "pictures", "ms"}, then one summary line per run with the
ratios DESIGN.md section 9b quotes.
MEASUREMENT TOOL: off the headline metric (bench.py does not run the output stage)."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "arrow-h264_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _hip_runtime():
    """The HIP runtime this process already uses (torch's), for hipMemcpyAsync."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no libamdhip64 in this process")


def main():
    import numpy as np
    import torch
    import torch.nn.functional as F
    import h264r
    import rgb_restate as R
    import scale_restate as SR
    from h264r import output as OUT
    npics = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    warm = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    W, H = 120, 68
    crop = OUT.Crop.for_height(W, H, 1920, 1080)
    h264r.lib()
    hip = _hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    D2D = 3                                                   # hipMemcpyDeviceToDevice
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
    sizes = ((224, 224), (960, 540))
    filters = (("area", OUT.SCALE_AREA), ("bilinear", OUT.SCALE_BILINEAR))
    formats = (("planar_u8", OUT.RGB_PLANAR_U8), ("planar_f16", OUT.RGB_PLANAR_F16))
    base = dict(matrix=OUT.CSC_BT709, full_range=False, chroma_up=OUT.UP_REPLICATE)

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
    cands = []
    for ow, oh in sizes:
        for fname, filter in filters:
            for tname, format in formats:
                fb = OUT.scaled_geometry(OUT.scale_desc(OUT.rgb_desc(out.desc, format=format), ow, oh, None, filter), 1).frame_bytes
                dst = torch.full((npics, fb), 0xA5, dtype=torch.uint8, device="cuda")
                out.rgb_scaled(table, ow, oh, filter=filter, format=format, dst=dst, stream=sp, **base)
                dec.check()
                for i in (0, npics - 1):
                    pl = [t[i].cpu().numpy() for t in (y, u, v)]
                    pl = (pl[0].reshape(16 * H, 16 * W), pl[1].reshape(8 * H, 8 * W), pl[2].reshape(8 * H, 8 * W))
                    want = np.zeros(fb, np.uint8)
                    SR.frame(OUT.OUT_FRAME, [pl], W, H, crop, 1, want, ow, oh, filter=filter, matrix=R.BT709, format=format)
                    if not np.array_equal(dst[i].cpu().numpy(), want):
                        raise SystemExit(f"bench_output_scale: {ow}x{oh} {fname} {tname} frame {i} differs from numpy")
                cands.append((f"scaled {ow}x{oh} {fname} {tname}",
                              lambda ow=ow, oh=oh, filter=filter, format=format, dst=dst:
                              out.rgb_scaled(table, ow, oh, filter=filter, format=format, dst=dst, stream=sp, **base)))
    full_u8 = torch.empty((npics, 3 * 1920 * 1080), dtype=torch.uint8, device="cuda")
    cands.append(("(b) h264r_output_rgb planar_u8",
                  lambda: out.rgb(table, format=OUT.RGB_PLANAR_U8, dst=full_u8, stream=sp, **base)))
    full_f16 = torch.empty((npics, 6 * 1920 * 1080), dtype=torch.uint8, device="cuda")
    for ow, oh in sizes:
        def two_step(ow=ow, oh=oh):
            t = out.rgb(table, format=OUT.RGB_PLANAR_F16, dst=full_f16, stream=sp, **base)
            # slices of 128 pictures keep each call's tensor below 2^31 elements
            return [F.interpolate(t[k:k + 128], size=(oh, ow), mode="bilinear", antialias=True, align_corners=False)
                    for k in range(0, npics, 128)]
        cands.append((f"(a) h264r_output_rgb planar_f16 + interpolate {ow}x{oh}", two_step))
    copy_dst = torch.empty(plane_bytes, dtype=torch.uint8, device="cuda")

    def memcpy():
        if hip.hipMemcpyAsync(copy_dst.data_ptr(), planes.data_ptr(), plane_bytes, D2D, sp) != 0:
            raise SystemExit("hipMemcpyAsync failed")
    cands.append((f"(c) hipMemcpyAsync device to device, {plane_bytes} bytes of planes", memcpy))

    results = [{}, {}]
    for run in (0, 1):
        for what, fn in cands:
            results[run][what] = timed(what, run, fn)
        dec.check()
    key = lambda r, head: next(r[k] for k in r if k.startswith(head))
    for run in (0, 1):
        r = results[run]
        s = {"summary": "ratios of times", "run": run}
        for ow, oh in sizes:
            for tname in ("planar_u8", "planar_f16"):
                for fname in ("area", "bilinear"):
                    t = r[f"scaled {ow}x{oh} {fname} {tname}"]
                    s[f"{ow}x{oh} {fname} {tname} / (a)"] = t / key(r, f"(a) h264r_output_rgb planar_f16 + interpolate {ow}x{oh}")
                    s[f"{ow}x{oh} {fname} {tname} / (b)"] = t / key(r, "(b)")
                    s[f"{ow}x{oh} {fname} {tname} / (c)"] = t / key(r, "(c)")
        s["verified_vs_numpy"] = True
        print(json.dumps(s), flush=True)
    dec.close()


if __name__ == "__main__":
    main()
