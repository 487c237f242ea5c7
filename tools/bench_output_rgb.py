"""Bandwidth of the RGB output stage (include/h264r_output.h: h264r_output_rgb)
against a plain copy, by the method of tools/bench_output.py: B pictures of 120 x 68 MBs (1080p) in
4:2:0, frame_crop_bottom_offset 4 to 1080 rows, BT.709 limited range, written as each of the four
formats under replicate and under bilinear chroma, and the same number of OUTPUT bytes moved by one
device-to-device hipMemcpyAsync in the same process.  HIP events on one stream around K back-to-back
calls after W warm-up calls, nothing synchronising inside the timed region; everything is measured
twice (run 0, run 1); frames 0 and B - 1 of every variant are first checked against the numpy
restatement of the header (tests/rgb_restate.py).

    python3 tools/bench_output_rgb.py [B] [K] [W]

One JSON line per measurement: {"what", "run", "pictures", "bytes_out", "ms", "gb_per_s_out"}, then one
summary line per run with each variant's time relative to the copy of its own output bytes.
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
    import h264r
    import rgb_restate as R
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
    y = torch.randint(0, 256, (npics, 256 * W * H), dtype=torch.uint8, device="cuda", generator=g)
    u = torch.randint(0, 256, (npics, 64 * W * H), dtype=torch.uint8, device="cuda", generator=g)
    v = torch.randint(0, 256, (npics, 64 * W * H), dtype=torch.uint8, device="cuda", generator=g)
    out = OUT.DeviceOutput(dec, W, H, crop)
    table = out.frames_from([(OUT.OUT_FRAME, (y[i], u[i], v[i])) for i in range(npics)])
    formats = (("rgb24", OUT.RGB_PACKED_U8), ("rgbx", OUT.RGB_PACKED_U8X4), ("planar_u8", OUT.RGB_PLANAR_U8),
               ("planar_f16", OUT.RGB_PLANAR_F16))
    ups = (("replicate", OUT.UP_REPLICATE), ("bilinear", OUT.UP_BILINEAR))

    def timed(what, run, fn, nbytes):
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
        print(json.dumps({"what": what, "run": run, "pictures": npics, "bytes_out": nbytes, "ms": ms,
                          "gb_per_s_out": nbytes / ms / 1e6}), flush=True)
        return ms

    results = [{}, {}]
    for fname, format in formats:
        nbytes = npics * OUT.rgb_geometry(OUT.rgb_desc(out.desc, format=format), 1).frame_bytes
        dst = torch.empty((npics, nbytes // npics), dtype=torch.uint8, device="cuda")
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        for uname, up in ups:
            par = dict(matrix=OUT.CSC_BT709, full_range=False, chroma_up=up, format=format)
            dst.fill_(0xA5)
            out.rgb(table, dst=dst, stream=sp, **par)
            dec.check()
            for i in (0, npics - 1):
                planes = [t[i].cpu().numpy() for t in (y, u, v)]
                planes = (planes[0].reshape(16 * H, 16 * W), planes[1].reshape(8 * H, 8 * W), planes[2].reshape(8 * H, 8 * W))
                want = np.zeros(nbytes // npics, np.uint8)
                R.frame(OUT.OUT_FRAME, [planes], W, H, crop, 1, want, matrix=R.BT709, up=up, format=format)
                if not np.array_equal(dst[i].cpu().numpy(), want):
                    raise SystemExit(f"bench_output_rgb: {fname} {uname} frame {i} differs from numpy")

        def memcpy():
            if hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, D2D, sp) != 0:
                raise SystemExit("hipMemcpyAsync failed")
        for run in (0, 1):
            for uname, up in ups:
                par = dict(matrix=OUT.CSC_BT709, full_range=False, chroma_up=up, format=format)
                results[run][f"{fname} {uname}"] = timed(f"h264r_output_rgb {fname} {uname}", run,
                                                         lambda: out.rgb(table, dst=dst, stream=sp, **par), nbytes)
            results[run][f"{fname} copy"] = timed(f"hipMemcpyAsync device to device, bytes of {fname}", run, memcpy, nbytes)
        dec.check()
        del dst, src
    for run in (0, 1):
        r = results[run]
        print(json.dumps({"summary": "time relative to hipMemcpyAsync of the same output bytes", "run": run,
                          **{k: r[k] / r[k.split()[0] + " copy"] for k in r if not k.endswith(" copy")},
                          "verified_vs_numpy": True}), flush=True)
    dec.close()


if __name__ == "__main__":
    main()
