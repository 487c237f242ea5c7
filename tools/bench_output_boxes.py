"""Boxes of scaled RGB from a device table (include/h264r_output.h: h264r_output_rgb_boxes, DESIGN.md
section 9c) against what a user does without it, by the method of tools/bench_output_scale.py: B pictures
of 120 x 68 MBs (1080p) in 4:2:0, frame_crop_bottom_offset 4 to 1080 rows, BT.709 limited range, replicate
chroma, planar binary16.  In one process:

    (A) crops: 8 boxes per picture from a seeded generator, sides 48 .. 400, each to 224 x 224, box i into
        image i, BILINEAR and AREA.  "boxes" is one h264r_output_rgb_boxes job for all 8 B of them;
        "calls" is 8 B h264r_output_rgb_scaled calls of one frame each (a one-entry frame table, the box's
        region) into the same places of a buffer of its own -- the library's C entry point straight from
        ctypes with descriptors made beforehand, so that what is timed is the library and the launches.
        The two buffers must be equal byte for byte.
    (B) letterbox: every picture whole to 640 x 360, centred in a 640 x 640 image (letterbox_boxes),
        BILINEAR and AREA.  "boxes" is one job of B boxes into prefilled images; "scaled" is
        h264r_output_rgb_scaled of the same table to 640 x 360 into a buffer of its own: the same pixels
        through the same window code.  The images' rows 140 .. 499 must equal the scaled frames.

HIP events on one stream around K back-to-back calls after W warm-up calls, nothing synchronising inside
the timed region; two runs (run 0, run 1), each going through all the candidates in turn.  One "call" of
(A) "calls" is all its 8 B library calls; it is timed over KC repetitions (default 10) after one warm-up,
because 200 of them are 1.6 million launches.  Box 0 and the last box of every job are first checked against
the numpy restatement (tests/boxes_restate.py).

    python3 tools/bench_output_boxes.py [B] [K] [W] [KC] [PARTS]

PARTS is AB (default), A or B: what to run, for a profiler that should see one of them alone.

One JSON line per measurement: {"what", "run", "pictures", "boxes", "ms"}, then one summary line per run with
the ratios DESIGN.md section 9c quotes.  The plan kernel's own time is not in here: a
`rocprofv3 --kernel-trace --stats` run of this tool gives it (k_output_boxes_plan).
MEASUREMENT TOOL: off the headline metric (bench.py does not run the output stage)."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "arrow-h264_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import numpy as np
    import torch
    import boxes_restate as BR
    import h264r
    import rgb_restate as R
    from h264r import _abi as A
    from h264r import output as OUT
    npics = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    warm = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    steps_calls = int(sys.argv[4]) if len(sys.argv) > 4 else 10
    parts = sys.argv[5] if len(sys.argv) > 5 else "AB"
    W, H = 120, 68
    crop = OUT.Crop.for_height(W, H, 1920, 1080)
    L = h264r.lib()
    dec = h264r.Decoder(0, W, H)
    stream = torch.cuda.Stream()                              # a stream of its own: events and work on it alone
    torch.cuda.set_stream(stream)
    sp = stream.cuda_stream
    g = torch.Generator(device="cuda").manual_seed(1)
    planes = torch.randint(0, 256, (npics * 384 * W * H,), dtype=torch.uint8, device="cuda", generator=g)
    y = planes[:npics * 256 * W * H].view(npics, 256 * W * H)
    u = planes[npics * 256 * W * H:npics * 320 * W * H].view(npics, 64 * W * H)
    v = planes[npics * 320 * W * H:].view(npics, 64 * W * H)
    out = OUT.DeviceOutput(dec, W, H, crop)
    table = out.frames_from([(OUT.OUT_FRAME, (y[i], u[i], v[i])) for i in range(npics)])
    tptr = table.tensor.data_ptr()
    filters = (("bilinear", OUT.SCALE_BILINEAR), ("area", OUT.SCALE_AREA))
    base = dict(matrix=OUT.CSC_BT709, full_range=False, chroma_up=OUT.UP_REPLICATE, format=OUT.RGB_PLANAR_F16)
    rgb = OUT.rgb_desc(out.desc, **base)

    def host_channels(i):
        pl = [t[i].cpu().numpy() for t in (y, u, v)]
        pl = (pl[0].reshape(16 * H, 16 * W), pl[1].reshape(8 * H, 8 * W), pl[2].reshape(8 * H, 8 * W))
        return BR.frame_channels(OUT.OUT_FRAME, [pl], W, H, crop, 1, R.BT709, 0, R.REPLICATE, 0)

    def check_boxes(what, dst, tab, idx, iw, ih, filter):
        """Boxes idx of the job against numpy, pixel for pixel of their own rectangle."""
        fb = dst.shape[1]
        for i in idx:
            b = {k: int(tab[i][k]) for k in BR.FIELDS}
            want = np.zeros(fb, np.uint8)
            BR.images(want, 0, [dict(b, image=0)], {b["frame"]: host_channels(b["frame"])}, iw, ih, filter=filter, format=R.PLANAR_F16)
            got = dst[b["image"]].cpu().numpy()
            rows = want.reshape(3, ih, 2 * iw)[:, b["dst_y"]:b["dst_y"] + b["out_h"], 2 * b["dst_x"]:2 * (b["dst_x"] + b["out_w"])]
            if not np.array_equal(got.reshape(3, ih, 2 * iw)[:, b["dst_y"]:b["dst_y"] + b["out_h"],
                                                            2 * b["dst_x"]:2 * (b["dst_x"] + b["out_w"])], rows):
                raise SystemExit(f"bench_output_boxes: {what} box {i} differs from numpy")

    def timed(what, run, fn, nboxes, k=steps, w=warm):
        for _ in range(w):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(stream)
        for _ in range(k):
            fn()
        b.record(stream)
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / k
        print(json.dumps({"what": what, "run": run, "pictures": npics, "boxes": nboxes, "ms": ms}), flush=True)
        return ms

    cands = []
    # ---------------------------------------------------------------- (A) crops to 224 x 224
    rng = np.random.default_rng(1)
    nb = 8 * npics
    side = 224
    crops = np.zeros(nb, OUT.OUT_BOX_DTYPE)
    crops["frame"] = np.arange(nb) // 8
    crops["image"] = np.arange(nb)
    crops["roi_w"], crops["roi_h"] = rng.integers(48, 401, nb), rng.integers(48, 401, nb)
    crops["roi_x"] = (rng.random(nb) * (1920 - crops["roi_w"] + 1)).astype(np.int32)
    crops["roi_y"] = (rng.random(nb) * (1080 - crops["roi_h"] + 1)).astype(np.int32)
    crops["out_w"] = crops["out_h"] = side
    crops_dev = torch.from_numpy(crops.view(np.uint8).reshape(-1).copy()).cuda()
    fb_a = OUT.boxes_geometry(OUT.boxes_desc(rgb, side, side), 1).frame_bytes
    for fname, filter in filters if "A" in parts else ():
        d = OUT.boxes_desc(rgb, side, side, None, filter)
        assert all(OUT.box_status(d, crops[i], npics, nb) == A.OK for i in range(0, nb, 97))
        one = torch.full((nb, fb_a), 0xA5, dtype=torch.uint8, device="cuda")
        many = torch.full((nb, fb_a), 0xA5, dtype=torch.uint8, device="cuda")

        def boxes_job(d=d, dst=one):
            st = L.h264r_output_rgb_boxes(dec.handle, C.byref(d), tptr, npics, crops_dev.data_ptr(), nb, dst.data_ptr(), fb_a, nb, sp)
            if st != A.OK:
                raise SystemExit(f"h264r_output_rgb_boxes: {st}")
        descs = [OUT.scale_desc(rgb, side, side, (int(b["roi_x"]), int(b["roi_y"]), int(b["roi_w"]), int(b["roi_h"])), filter) for b in crops]
        refs = [C.byref(s) for s in descs]
        entry = [tptr + 56 * int(f) for f in crops["frame"]]
        where = [many.data_ptr() + i * fb_a for i in range(nb)]
        scaled = L.h264r_output_rgb_scaled

        def calls_job(refs=refs, entry=entry, where=where):
            h = dec.handle
            for i in range(nb):
                if scaled(h, refs[i], entry[i], 1, where[i], fb_a, sp) != A.OK:
                    raise SystemExit("h264r_output_rgb_scaled failed")
        boxes_job()
        calls_job()
        dec.check()
        check_boxes(f"(A) {fname}", one, crops, (0, nb - 1), side, side, filter)
        if not torch.equal(one, many):
            raise SystemExit(f"bench_output_boxes: (A) {fname}: the job and the calls differ")
        del many                                              # the calls rewrite the job's buffer from here on: same bytes
        where[:] = [one.data_ptr() + i * fb_a for i in range(nb)]
        cands.append((f"(A) crops 224x224 {fname} boxes: 1 job", boxes_job, nb, steps, warm))
        cands.append((f"(A) crops 224x224 {fname} calls: {nb} h264r_output_rgb_scaled", calls_job, nb, steps_calls, 1))
    # ---------------------------------------------------------------- (B) letterbox into 640 x 640
    iw = ih = 640
    letter = OUT.letterbox_boxes(npics, 1920, 1080, iw, ih)
    ow, oh, dy = int(letter["out_w"][0]), int(letter["out_h"][0]), int(letter["dst_y"][0])
    assert (ow, oh, int(letter["dst_x"][0]), dy) == (640, 360, 0, 140)
    letter_dev = torch.from_numpy(letter.view(np.uint8).reshape(-1).copy()).cuda()
    fb_b = OUT.boxes_geometry(OUT.boxes_desc(rgb, iw, ih), 1).frame_bytes
    for fname, filter in filters if "B" in parts else ():
        d = OUT.boxes_desc(rgb, iw, ih, (ow, oh), filter)
        sd = OUT.scale_desc(rgb, ow, oh, None, filter)
        fb_s = OUT.scaled_geometry(sd, 1).frame_bytes
        img = torch.full((npics, fb_b), 0xA5, dtype=torch.uint8, device="cuda")
        frm = torch.full((npics, fb_s), 0xA5, dtype=torch.uint8, device="cuda")

        def boxes_job(d=d, dst=img):
            st = L.h264r_output_rgb_boxes(dec.handle, C.byref(d), tptr, npics, letter_dev.data_ptr(), npics, dst.data_ptr(), fb_b, npics, sp)
            if st != A.OK:
                raise SystemExit(f"h264r_output_rgb_boxes: {st}")

        def scaled_job(sd=sd, dst=frm):
            if L.h264r_output_rgb_scaled(dec.handle, C.byref(sd), tptr, npics, dst.data_ptr(), fb_s, sp) != A.OK:
                raise SystemExit("h264r_output_rgb_scaled failed")
        boxes_job()
        scaled_job()
        dec.check()
        check_boxes(f"(B) {fname}", img, letter, (0, npics - 1), iw, ih, filter)
        rows = img.view(npics, 3, ih, 2 * iw)
        if not torch.equal(rows[:, :, dy:dy + oh], frm.view(npics, 3, oh, 2 * ow)):
            raise SystemExit(f"bench_output_boxes: (B) {fname}: the images' rows and the scaled frames differ")
        if not bool((rows[:, :, :dy] == 0xA5).all()) or not bool((rows[:, :, dy + oh:] == 0xA5).all()):
            raise SystemExit(f"bench_output_boxes: (B) {fname}: the border was written")
        cands.append((f"(B) letterbox 640x360 in 640x640 {fname} boxes: 1 job", boxes_job, npics, steps, warm))
        cands.append((f"(B) letterbox 640x360 {fname} scaled: 1 h264r_output_rgb_scaled", scaled_job, npics, steps, warm))

    results = [{}, {}]
    for run in (0, 1):
        for what, fn, n, k, w in cands:
            results[run][what] = timed(what, run, fn, n, k, w)
        dec.check()
    key = lambda r, head: next(r[k] for k in r if k.startswith(head))
    for run in (0, 1):
        r = results[run]
        s = {"summary": "times and ratios", "run": run}
        for fname, _ in filters:
            if "A" in parts:
                s[f"(A) {fname} boxes / calls"] = key(r, f"(A) crops 224x224 {fname} boxes") / key(r, f"(A) crops 224x224 {fname} calls")
            if "B" in parts:
                s[f"(B) {fname} boxes - scaled ms"] = (key(r, f"(B) letterbox 640x360 in 640x640 {fname} boxes")
                                                       - key(r, f"(B) letterbox 640x360 {fname} scaled"))
        s["verified_vs_numpy"] = True
        print(json.dumps(s), flush=True)
    for fname, _ in filters if "B" in parts else ():
        a, b = (key(results[run], f"(B) letterbox 640x360 {fname} scaled") for run in (0, 1))
        print(json.dumps({"summary": f"(B) {fname} scaled: spread between the runs, ms", "ms": abs(a - b)}), flush=True)
    dec.close()


if __name__ == "__main__":
    main()
