"""Bandwidth of the device-side output stage (include/h264r_output.h) against
a plain copy: B pictures of 120 x 68 MBs (1080p, the config-3 size) in 4:2:0, frame_crop_bottom_offset
4 to 1080 rows, written by h264r_output_frames as planar (the reference's bytes) and as NV12, and
the same number of output bytes moved by one device-to-device hipMemcpyAsync in the same process.
HIP events on one stream around K back-to-back calls after W warm-up calls, nothing synchronising
inside the timed region; frames 0 and B - 1 of each layout are checked against numpy first.

    python3 tools/bench_output.py [B] [K] [W]

One JSON line per measurement: {"what", "pictures", "bytes_out", "ms", "gb_per_s_out",
"gb_per_s_moved"} (moved = read + written: twice the output bytes), then a summary line with the
ratios.  MEASUREMENT TOOL: off the headline metric (bench.py does not run the output stage)."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "arrow-h264_amd"))


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
    from h264r import output as OUT
    npics = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    warm = int(sys.argv[3]) if len(sys.argv) > 3 else 3
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
    rows = [(OUT.OUT_FRAME, (y[i], u[i], v[i])) for i in range(npics)]
    geom = OUT.geometry(W, H, crop)
    results = {}

    def timed(what, fn, nbytes):
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
        results[what] = ms
        print(json.dumps({"what": what, "pictures": npics, "bytes_out": nbytes, "ms": ms,
                          "gb_per_s_out": nbytes / ms / 1e6, "gb_per_s_moved": 2 * nbytes / ms / 1e6}), flush=True)

    nbytes = 0
    for name, layout in (("planar", OUT.PLANAR), ("nv12", OUT.SEMIPLANAR)):
        out = OUT.DeviceOutput(dec, W, H, crop, layout=layout)
        table = out.frames_from(rows)
        dst = torch.empty((npics, out.geom.frame_bytes), dtype=torch.uint8, device="cuda")
        nbytes = dst.numel()
        out.run(table, dst=dst, stream=sp)
        dec.check()
        for i in (0, npics - 1):
            planes = [t[i].cpu().numpy() for t in (y, u, v)]
            planes = (planes[0].reshape(16 * H, 16 * W), planes[1].reshape(8 * H, 8 * W), planes[2].reshape(8 * H, 8 * W))
            want = np.frombuffer(OUT.frame_bytes(*planes, geom), np.uint8)
            if layout == OUT.SEMIPLANAR:
                ny, nc = geom.luma[2] * geom.luma[3], geom.chroma[2] * geom.chroma[3]
                want = np.concatenate([want[:ny], np.stack([want[ny:ny + nc], want[ny + nc:]], axis=1).reshape(-1)])
            if not np.array_equal(dst[i].cpu().numpy(), want):
                raise SystemExit(f"bench_output: {name} frame {i} differs from numpy")
        timed(f"h264r_output_frames {name}", lambda: out.run(table, dst=dst, stream=sp), nbytes)
        del dst
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def memcpy():
        if hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, D2D, sp) != 0:
            raise SystemExit("hipMemcpyAsync failed")
    timed("hipMemcpyAsync device to device", memcpy, nbytes)
    dec.check()
    base = results["hipMemcpyAsync device to device"]
    print(json.dumps({"summary": "time relative to hipMemcpyAsync of the same output bytes",
                      "planar": results["h264r_output_frames planar"] / base,
                      "nv12": results["h264r_output_frames nv12"] / base, "verified_vs_numpy": True}), flush=True)
    dec.close()


if __name__ == "__main__":
    main()
