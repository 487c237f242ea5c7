"""Output and compare step: the cropping YUV writer and the per-frame MD5 compare.

SURVEY §8(f) rank 3.  The reference writes every output picture as cropped
planar Y, Cb, Cr (`write_out_picture`, src/codec/h264/framebuf/output.cc:109-227)
and its test harness splits the decoded file into N equal frames, MD5s each and
compares count and digests with a `*.yuv.md5` list (`Executor.digest_by_frames`
/ `Executor.compare`, script/test/model/__init__.py:119-183).  This module does
the same on the planes the GPU path returns (`Decoder.deblock_filter`,
`DeviceBatch.planes`): 4:2:0, 8 bits per sample, frame coding -- the formats the
hot path reconstructs.

Host-side byte shuffling only (strided row copies); nothing here computes samples.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import io
import os
from dataclasses import dataclass
from typing import BinaryIO, Iterable, Sequence

import numpy as np


@dataclass(frozen=True)
class Crop:
    """SPS frame cropping, in the syntax's units (output.cc:147-157): offsets count
    chroma samples horizontally and chroma rows x (2 - frame_mbs_only_flag) vertically."""
    left: int = 0
    right: int = 0
    top: int = 0
    bottom: int = 0
    frame_mbs_only: int = 1

    @staticmethod
    def for_height(width_mbs: int, height_mbs: int, width: int, height: int) -> "Crop":
        """The crop an encoder signals for a width x height picture coded in whole MBs
        (1920x1080 in 120x68 MBs -> frame_crop_bottom_offset 4)."""
        dx, dy = 16 * width_mbs - width, 16 * height_mbs - height
        if dx < 0 or dy < 0 or dx % 2 or dy % 2:
            raise ValueError(f"{width}x{height} does not fit {width_mbs}x{height_mbs} MBs in 4:2:0 crop units")
        return Crop(right=dx // 2, bottom=dy // 2)


@dataclass(frozen=True)
class OutputGeometry:
    """Cropped output sizes (output.cc:135-165)."""
    luma: tuple[int, int, int, int]      # (x0, y0, width, height) inside the coded luma plane
    chroma: tuple[int, int, int, int]
    fake_uv: int = 0                     # 4:0:0: bytes of value 128 per chroma plane (output.cc:205-224)

    @property
    def frame_bytes(self) -> int:
        """iFrameSize (output.cc:164): one byte per sample at 8 bits."""
        return self.luma[2] * self.luma[3] + 2 * self.chroma[2] * self.chroma[3] + 2 * self.fake_uv


def geometry(width_mbs: int, height_mbs: int, crop: Crop = Crop(), chroma_format: int = 1) -> OutputGeometry:
    """output.cc:135-165: size_x_l = PicWidthInMbs*16, size_x_c = PicWidthInMbs*MbWidthC;
    crop_*_c from the SPS (vertical offsets x (2 - frame_mbs_only_flag)), crop_*_l =
    SubWidthC/SubHeightC x crop_*_c.  chroma_format 2 (4:2:2): SubHeightC 1; 3 (4:4:4): SubWidthC 1 too;
    0 (4:0:0): the cropped luma, then two planes of 128 of a quarter of its size (WriteUV,
    output.cc:205-224: the reference fakes a 4:2:0 file)."""
    if chroma_format == 0:                   # CropUnitX 1, CropUnitY 2 - frame_mbs_only_flag (7.4.2.1.1)
        uy = 2 - crop.frame_mbs_only
        lw, lh = 16 * width_mbs - (crop.left + crop.right), 16 * height_mbs - uy * (crop.top + crop.bottom)
        if min(crop.left, crop.right, crop.top, crop.bottom) < 0 or lw <= 0 or lh <= 0:
            raise ValueError(f"frame cropping {crop} leaves no picture of {width_mbs}x{height_mbs} MBs")
        return OutputGeometry((crop.left, uy * crop.top, lw, lh), (0, 0, 0, 0), (lw * lh) // 4)
    sub_w, sub_h = (1 if chroma_format == 3 else 2), (2 if chroma_format == 1 else 1)
    lc, rc = crop.left, crop.right
    tc, bc = crop.top * (2 - crop.frame_mbs_only), crop.bottom * (2 - crop.frame_mbs_only)
    size_x_l, size_y_l = 16 * width_mbs, 16 * height_mbs
    size_x_c, size_y_c = 16 // sub_w * width_mbs, 16 // sub_h * height_mbs
    lw, lh = size_x_l - sub_w * (lc + rc), size_y_l - sub_h * (tc + bc)
    cw, ch = size_x_c - (lc + rc), size_y_c - (tc + bc)
    if min(lc, rc, tc, bc) < 0 or lw <= 0 or lh <= 0 or cw <= 0 or ch <= 0:
        raise ValueError(f"frame cropping {crop} leaves no picture of {width_mbs}x{height_mbs} MBs")
    return OutputGeometry((sub_w * lc, sub_h * tc, lw, lh), (lc, tc, cw, ch))


def _plane_view(p: np.ndarray, rect: tuple[int, int, int, int], name: str) -> np.ndarray:
    x0, y0, w, h = rect
    if p.dtype != np.uint8 or p.ndim != 2 or p.shape[0] < y0 + h or p.shape[1] < x0 + w:
        raise ValueError(f"{name} plane {p.dtype}{p.shape} does not hold the crop window {rect}")
    return p[y0:y0 + h, x0:x0 + w]


def frame_bytes(y: np.ndarray, u: np.ndarray, v: np.ndarray, geom: OutputGeometry) -> bytes:
    """One output frame as written by write_out_picture (output.cc:186-201): the cropped
    Y rows, then Cb, then Cr, each row-contiguous (img2buf, output.cc:61-106)."""
    out = bytearray(geom.frame_bytes)
    mv = memoryview(out)
    off = 0
    planes = ((y, geom.luma, "Y"),) if geom.fake_uv else ((y, geom.luma, "Y"), (u, geom.chroma, "Cb"), (v, geom.chroma, "Cr"))
    for p, rect, name in planes:
        view = _plane_view(np.asarray(p), rect, name)
        n = view.size
        mv[off:off + n] = np.ascontiguousarray(view).reshape(-1).data
        off += n
    if geom.fake_uv:
        mv[off:] = b"\x80" * (2 * geom.fake_uv)
    return bytes(out)


class YuvWriter:
    """Appends cropped frames to a file (or any binary stream), like the reference's
    output file descriptor `p_out` (output.cc:109, write() per plane)."""

    def __init__(self, target: str | os.PathLike | BinaryIO, width_mbs: int, height_mbs: int,
                 crop: Crop = Crop()):
        self.geom = geometry(width_mbs, height_mbs, crop)
        self._own = not hasattr(target, "write")
        self._f: BinaryIO = open(target, "wb") if self._own else target   # type: ignore[assignment]
        self.frames = 0

    def write(self, y: np.ndarray, u: np.ndarray, v: np.ndarray) -> None:
        data = frame_bytes(y, u, v, self.geom)
        if self._f.write(data) not in (None, len(data)):
            raise IOError("write_out_picture: error writing to YUV file")
        self.frames += 1

    def close(self) -> None:
        if self._own and not self._f.closed:
            self._f.close()

    def __enter__(self) -> "YuvWriter":
        return self

    def __exit__(self, *exc) -> None:
        self.close()


def digest_by_frames(source: str | os.PathLike | bytes, frames: int) -> list[str]:
    """Executor.digest_by_frames (model/__init__.py:119-150): split the decoded YUV into
    `frames` equal chunks (size // frames; a remainder becomes one more chunk) and MD5
    each, lower-case hex."""
    if frames <= 0:
        raise ValueError(f"digest error: {frames} frames")
    data = source if isinstance(source, (bytes, bytearray)) else open(source, "rb").read()
    size = len(data) // frames
    if size <= 0:
        raise ValueError(f"digest error: {len(data)} bytes for {frames} frames")
    f = io.BytesIO(data)
    lines = []
    while True:
        chunk = f.read(size)
        if not chunk:
            break
        lines.append(hashlib.md5(chunk).hexdigest().lower())
    return lines


def read_digests(path: str | os.PathLike) -> list[str]:
    """A `*.yuv.md5` list: one digest per line (model/__init__.py:157-159)."""
    with open(path, "rt") as f:
        return [line.rstrip().lower() for line in f]


def write_digests(path: str | os.PathLike, lines: Iterable[str]) -> None:
    with open(path, "wt") as f:
        for line in lines:
            f.write(f"{line}\n")


class CompareError(Exception):
    pass


def compare(lines: Sequence[str], hashes: Sequence[str], name: str = "") -> list[str]:
    """Executor.compare (model/__init__.py:152-183): the frame counts must agree, then
    every digest; the first mismatch raises with its index."""
    lines = [x.rstrip().lower() for x in lines]
    hashes = [x.rstrip().lower() for x in hashes]
    if len(lines) != len(hashes):
        raise CompareError(f"decoded frames is different: {name}")
    for i, (line, h) in enumerate(zip(lines, hashes)):
        if line != h:
            raise CompareError(f"mismatch {i} {name}: {line} != {h}")
    return lines


def compare_yuv(source: str | os.PathLike | bytes, digest_file: str | os.PathLike, name: str = "") -> list[str]:
    """The harness's compare() for a decoded file against its `*.yuv.md5`."""
    hashes = read_digests(digest_file)
    return compare(digest_by_frames(source, len(hashes)), hashes, name)


# --------------------------------------------------------------------------------------------
# The device-side output stage (include/h264r_output.h): the same frames -- cropped, field pairs
# woven, 4:0:0 with the reference's 128 chroma, planar or semi-planar -- written by the GPU from
# planes that are already there.  ctypes mirror of the header, and DeviceOutput over torch tensors.
PLANAR, SEMIPLANAR = 0, 1                                         # h264r_out_desc.layout
OUT_FRAME, OUT_FIELD_PAIR, OUT_UNPAIRED_TOP, OUT_UNPAIRED_BOT = 0, 1, 2, 3   # h264r_out_frame.kind


class OutDesc(C.Structure):
    """h264r_out_desc"""
    _fields_ = [("width_mbs", C.c_int32), ("frame_height_mbs", C.c_int32),
                ("crop_left", C.c_int32), ("crop_right", C.c_int32), ("crop_top", C.c_int32),
                ("crop_bottom", C.c_int32), ("frame_mbs_only", C.c_int32), ("layout", C.c_int32),
                ("pitch_align", C.c_int32), ("fake_chroma", C.c_int32)]


class OutGeom(C.Structure):
    """h264r_out_geom"""
    _fields_ = [("luma", C.c_int32 * 4), ("chroma", C.c_int32 * 4), ("plane_off", C.c_int64 * 3),
                ("plane_pitch", C.c_int64 * 3), ("frame_bytes", C.c_int64)]


# h264r_out_frame: kind, pad, y[2], u[2], v[2]
OUT_FRAME_DTYPE = np.dtype([("kind", "<i4"), ("pad", "<i4"), ("y", "<u8", (2,)), ("u", "<u8", (2,)), ("v", "<u8", (2,))])
assert OUT_FRAME_DTYPE.itemsize == 56


# --------------------------------------------------------------------------------------------
# RGB frames (include/h264r_output.h, h264r_output_rgb): the enums, the ctypes mirrors, the geometry.
CSC_BT601, CSC_BT709, CSC_BT2020, CSC_GBR = 0, 1, 2, 3            # h264r_rgb_desc.matrix
UP_REPLICATE, UP_BILINEAR = 0, 1                                  # h264r_rgb_desc.chroma_up
RGB_PACKED_U8, RGB_PACKED_U8X4, RGB_PLANAR_U8, RGB_PLANAR_F16 = 0, 1, 2, 3   # h264r_rgb_desc.format


class RgbDesc(C.Structure):
    """h264r_rgb_desc"""
    _fields_ = [("src", OutDesc), ("matrix", C.c_int32), ("full_range", C.c_int32), ("chroma_up", C.c_int32),
                ("format", C.c_int32), ("bgr", C.c_int32), ("alpha", C.c_int32), ("scale", C.c_float * 3),
                ("bias", C.c_float * 3)]


class RgbGeom(C.Structure):
    """h264r_rgb_geom"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("plane_off", C.c_int64 * 3),
                ("plane_pitch", C.c_int64 * 3), ("frame_bytes", C.c_int64)]


@dataclass(frozen=True)
class RgbGeometry:
    """h264r_rgb_geom: the size and the layout of one RGB frame."""
    width: int
    height: int
    plane_off: tuple[int, int, int]
    plane_pitch: tuple[int, int, int]
    frame_bytes: int


def rgb_desc(src: OutDesc, matrix: int = CSC_BT709, full_range: bool = False, chroma_up: int = UP_REPLICATE,
             format: int = RGB_PLANAR_U8, bgr: bool = False, alpha: int = 255, scale=(1 / 255,) * 3,
             bias=(0,) * 3) -> RgbDesc:
    """An h264r_rgb_desc over a copy of `src` (an OutDesc: size, crop, frame_mbs_only, pitch_align)."""
    s = OutDesc.from_buffer_copy(src)
    return RgbDesc(s, int(matrix), int(full_range), int(chroma_up), int(format), int(bgr), int(alpha),
                   (C.c_float * 3)(*scale), (C.c_float * 3)(*bias))


def _rgb_geometry(fn: str, desc, chroma_format: int) -> RgbGeometry:
    """The h264r_rgb_geom that the library's `fn` fills for desc, as an RgbGeometry."""
    from . import _check, lib
    g = RgbGeom()
    _check(fn, getattr(lib(), fn)(chroma_format, C.byref(desc), C.byref(g)))
    return RgbGeometry(int(g.width), int(g.height), tuple(g.plane_off), tuple(g.plane_pitch), int(g.frame_bytes))


def rgb_geometry(desc: RgbDesc, chroma_format: int = 1) -> RgbGeometry:
    """h264r_output_rgb_geometry (host only, no GPU): raises H264RError with the library's status."""
    return _rgb_geometry("h264r_output_rgb_geometry", desc, chroma_format)


def rgb_view(buf, g: RgbGeometry, format: int):
    """The frames in `buf` (torch uint8 [n, stride >= frame_bytes]) as pixels: [n, H, W, 3 | 4] uint8
    (packed), [n, 3, H, W] uint8 or float16 (planar); rows keep their pitch, so the view is strided
    wherever a pitch_align pads them."""
    import torch
    n, stride = buf.shape[0], buf.stride(0)
    H, W, pitch = g.height, g.width, g.plane_pitch[0]
    if format in (RGB_PACKED_U8, RGB_PACKED_U8X4):
        ch = 3 if format == RGB_PACKED_U8 else 4
        return buf.as_strided((n, H, W, ch), (stride, pitch, ch, 1))
    if format == RGB_PLANAR_U8:
        return buf.as_strided((n, 3, H, W), (stride, pitch * H, pitch, 1))
    if stride % 2 or pitch % 2 or buf.data_ptr() % 2:
        raise ValueError("rgb_view: float16 frames need an even address, stride and pitch")
    half = buf[:, :g.frame_bytes].view(torch.float16)
    return half.as_strided((n, 3, H, W), (stride // 2, pitch * H // 2, pitch // 2, 1))


# --------------------------------------------------------------------------------------------
# Scaled RGB frames (include/h264r_output.h, h264r_output_rgb_scaled).
SCALE_BILINEAR, SCALE_AREA = 0, 1                                 # h264r_scale_desc.filter


class ScaleDesc(C.Structure):
    """h264r_scale_desc"""
    _fields_ = [("rgb", RgbDesc), ("roi_x", C.c_int32), ("roi_y", C.c_int32), ("roi_w", C.c_int32), ("roi_h", C.c_int32),
                ("out_w", C.c_int32), ("out_h", C.c_int32), ("filter", C.c_int32), ("pad", C.c_int32)]


def scale_desc(rgb: RgbDesc, out_w: int, out_h: int, roi=None, filter: int = SCALE_AREA) -> ScaleDesc:
    """An h264r_scale_desc over a copy of `rgb`; roi = (x, y, w, h) in luma samples of the cropped
    rectangle, None = all of it."""
    x, y, w, h = (0, 0, 0, 0) if roi is None else roi
    return ScaleDesc(RgbDesc.from_buffer_copy(rgb), int(x), int(y), int(w), int(h), int(out_w), int(out_h), int(filter), 0)


def scaled_geometry(desc: ScaleDesc, chroma_format: int = 1) -> RgbGeometry:
    """h264r_output_rgb_scaled_geometry (host only, no GPU): raises H264RError with the library's status."""
    return _rgb_geometry("h264r_output_rgb_scaled_geometry", desc, chroma_format)


# --------------------------------------------------------------------------------------------
# Resampled RGB frames (include/h264r_output.h, h264r_output_rgb_resampled): Pillow's 8-bit resize, exactly.
RESAMPLE_TRIANGLE, RESAMPLE_BICUBIC, RESAMPLE_LANCZOS = 0, 1, 2   # h264r_resample_desc.filter: Pillow BILINEAR, BICUBIC, LANCZOS
RESAMPLE_MAX_TAPS = 97                                            # H264R_RESAMPLE_MAX_TAPS
RESAMPLE_TILE_W, RESAMPLE_TILE_H = 16, 16                         # H264R_RESAMPLE_TILE_W / _H: the kernel's tile of output pixels


class ResampleDesc(C.Structure):
    """h264r_resample_desc"""
    _fields_ = [("rgb", RgbDesc), ("roi_x", C.c_int32), ("roi_y", C.c_int32), ("roi_w", C.c_int32), ("roi_h", C.c_int32),
                ("out_w", C.c_int32), ("out_h", C.c_int32), ("filter", C.c_int32), ("pad", C.c_int32)]


def resample_desc(rgb: RgbDesc, out_w: int, out_h: int, roi=None, filter: int = RESAMPLE_BICUBIC) -> ResampleDesc:
    """An h264r_resample_desc over a copy of `rgb`; roi = (x, y, w, h) in luma samples of the cropped
    rectangle (Pillow's box=(x, y, x + w, y + h)), None = all of it."""
    x, y, w, h = (0, 0, 0, 0) if roi is None else roi
    return ResampleDesc(RgbDesc.from_buffer_copy(rgb), int(x), int(y), int(w), int(h), int(out_w), int(out_h), int(filter), 0)


def resampled_geometry(desc: ResampleDesc, chroma_format: int = 1) -> RgbGeometry:
    """h264r_output_rgb_resampled_geometry (host only, no GPU): raises H264RError with the library's status."""
    return _rgb_geometry("h264r_output_rgb_resampled_geometry", desc, chroma_format)


def resample_axis(filter: int, in_size: int, in0: int, in1: int, out_size: int):
    """h264r_resample_axis (host only, no GPU): the table of one axis as numpy int32 arrays
    (xmin [out_size], count [out_size], kk [out_size, ksize]); raises H264RError with the library's status."""
    from . import _check, lib
    L = lib()
    ks = C.c_int32(0)
    _check("h264r_resample_axis", L.h264r_resample_axis(filter, in_size, in0, in1, out_size, None, None, None, C.byref(ks)))
    xmin, count = np.zeros(out_size, np.int32), np.zeros(out_size, np.int32)
    kk = np.zeros((out_size, ks.value), np.int32)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    _check("h264r_resample_axis", L.h264r_resample_axis(filter, in_size, in0, in1, out_size, ptr(xmin), ptr(count), ptr(kk),
                                                        C.byref(ks)))
    return xmin, count, kk


class ResamplePlan:
    """An h264r_resample_plan of one Decoder: destroyed by close(), at the end of a with block, or when
    the object goes -- after the launches that use it are done (Decoder.check())."""

    def __init__(self, decoder, desc: ResampleDesc, geom: RgbGeometry):
        from . import _check
        self.decoder, self.desc, self.geom = decoder, desc, geom
        self.format = int(desc.rgb.format)
        h = C.c_void_p()
        _check("h264r_resample_plan_create", decoder._L.h264r_resample_plan_create(decoder.handle, C.byref(desc), C.byref(h)))
        self.handle = h

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.decoder._L.h264r_resample_plan_destroy(self.handle)
            self.handle = None

    def __enter__(self) -> "ResamplePlan":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# --------------------------------------------------------------------------------------------
# Boxes of scaled RGB from a device table (include/h264r_output.h, h264r_output_rgb_boxes).
# h264r_out_box: frame, image, roi_x, roi_y, roi_w, roi_h, dst_x, dst_y, out_w, out_h, pad[2]
OUT_BOX_DTYPE = np.dtype([("frame", "<i4"), ("image", "<i4"), ("roi_x", "<i4"), ("roi_y", "<i4"), ("roi_w", "<i4"),
                          ("roi_h", "<i4"), ("dst_x", "<i4"), ("dst_y", "<i4"), ("out_w", "<i4"), ("out_h", "<i4"),
                          ("pad", "<i4", (2,))])
assert OUT_BOX_DTYPE.itemsize == 48


class OutBox(C.Structure):
    """h264r_out_box"""
    _fields_ = [("frame", C.c_int32), ("image", C.c_int32), ("roi_x", C.c_int32), ("roi_y", C.c_int32),
                ("roi_w", C.c_int32), ("roi_h", C.c_int32), ("dst_x", C.c_int32), ("dst_y", C.c_int32),
                ("out_w", C.c_int32), ("out_h", C.c_int32), ("pad", C.c_int32 * 2)]


class BoxesDesc(C.Structure):
    """h264r_boxes_desc"""
    _fields_ = [("rgb", RgbDesc), ("image_w", C.c_int32), ("image_h", C.c_int32), ("max_out_w", C.c_int32),
                ("max_out_h", C.c_int32), ("filter", C.c_int32), ("pad", C.c_int32)]


def boxes_desc(rgb: RgbDesc, image_w: int, image_h: int, max_out=None, filter: int = SCALE_AREA) -> BoxesDesc:
    """An h264r_boxes_desc over a copy of `rgb`; max_out = (w, h) bounds every box's output size, None =
    the image's size."""
    mw, mh = (image_w, image_h) if max_out is None else max_out
    return BoxesDesc(RgbDesc.from_buffer_copy(rgb), int(image_w), int(image_h), int(mw), int(mh), int(filter), 0)


def boxes_geometry(desc: BoxesDesc, chroma_format: int = 1) -> RgbGeometry:
    """h264r_output_rgb_boxes_geometry (host only, no GPU): the layout of one image; raises H264RError with
    the library's status."""
    return _rgb_geometry("h264r_output_rgb_boxes_geometry", desc, chroma_format)


def boxes_table(boxes) -> np.ndarray:
    """A host box table (OUT_BOX_DTYPE) of `boxes`: such an array already, or an iterable of boxes, each a
    mapping or a sequence (frame, image, roi_x, roi_y, roi_w, roi_h, dst_x, dst_y, out_w, out_h)."""
    if isinstance(boxes, np.ndarray) and boxes.dtype == OUT_BOX_DTYPE:
        return np.ascontiguousarray(boxes.reshape(-1))
    rows = list(boxes)
    tab = np.zeros(len(rows), OUT_BOX_DTYPE)
    names = OUT_BOX_DTYPE.names[:10]
    for i, row in enumerate(rows):
        if hasattr(row, "keys"):
            for k in row.keys():
                tab[i][k] = row[k]
        else:
            if len(row) != 10:
                raise ValueError("a box is (frame, image, roi_x, roi_y, roi_w, roi_h, dst_x, dst_y, out_w, out_h)")
            for k, v in zip(names, row):
                tab[i][k] = int(v)
    return tab


def box_status(desc: BoxesDesc, box, num_frames: int, num_images: int, chroma_format: int = 1) -> int:
    """h264r_out_box_status (host only, no GPU) of one box -- an OutBox, or one row of a box table: the
    library's status, H264R_OK for a box the device writes."""
    from . import lib
    if not isinstance(box, OutBox):
        box = OutBox.from_buffer_copy(np.asarray(box, OUT_BOX_DTYPE).reshape(1).tobytes())
    return int(lib().h264r_out_box_status(chroma_format, C.byref(desc), C.byref(box), num_frames, num_images))


def letterbox_boxes(n: int, lw: int, lh: int, image_w: int, image_h: int) -> np.ndarray:
    """The box table of a letterbox: frame i of n whole (lw x lh its cropped size) into image i, aspect
    kept, centred in image_w x image_h.  In integers: the axis that fills the image is the one the frame
    is longer in (lw * image_h <= lh * image_w: the height), the other is the nearest integer to the
    scaled size, 1 at the least; the border the caller has filled stays."""
    if min(n + 1, lw, lh, image_w, image_h) < 1:
        raise ValueError("letterbox_boxes: sizes must be positive")
    if lw * image_h <= lh * image_w:
        out_h = image_h
        out_w = max(1, (2 * lw * image_h + lh) // (2 * lh))
    else:
        out_w = image_w
        out_h = max(1, (2 * lh * image_w + lw) // (2 * lw))
    tab = np.zeros(n, OUT_BOX_DTYPE)
    tab["frame"] = tab["image"] = np.arange(n)
    tab["out_w"], tab["out_h"] = out_w, out_h
    tab["dst_x"], tab["dst_y"] = (image_w - out_w) // 2, (image_h - out_h) // 2
    return tab


# --------------------------------------------------------------------------------------------
# Deinterlaced frames (include/h264r_deinterlace.h, h264r_deinterlace).
DEINT_BOB, DEINT_ADAPTIVE = 0, 1                                  # h264r_deint_job.mode
DEINT_TILE_W, DEINT_TILE_H = 32, 64                               # H264R_DEINT_TILE_W / _H: the kernel's tile of samples

# h264r_deint_job: cur, prev, next, keep, second, mode
DEINT_JOB_DTYPE = np.dtype([("cur", "<i4"), ("prev", "<i4"), ("next", "<i4"), ("keep", "<i4"), ("second", "<i4"),
                            ("mode", "<i4")])
assert DEINT_JOB_DTYPE.itemsize == 24


class DeintJob(C.Structure):
    """h264r_deint_job"""
    _fields_ = [("cur", C.c_int32), ("prev", C.c_int32), ("next", C.c_int32), ("keep", C.c_int32), ("second", C.c_int32),
                ("mode", C.c_int32)]


class DeintGeom(C.Structure):
    """h264r_deint_geom"""
    _fields_ = [("rect", (C.c_int32 * 4) * 3), ("plane_off", C.c_int64 * 3), ("plane_pitch", C.c_int64 * 3),
                ("frame_bytes", C.c_int64)]


@dataclass(frozen=True)
class DeintGeometry:
    """h264r_deint_geom: the cropped rectangle inside each coded-size plane and the layout of one frame."""
    rect: tuple
    plane_off: tuple[int, int, int]
    plane_pitch: tuple[int, int, int]
    frame_bytes: int


def deint_geometry(desc: OutDesc, chroma_format: int = 1) -> DeintGeometry:
    """h264r_deinterlace_geometry (host only, no GPU): raises H264RError with the library's status."""
    from . import _check, lib
    g = DeintGeom()
    _check("h264r_deinterlace_geometry", lib().h264r_deinterlace_geometry(chroma_format, C.byref(desc), C.byref(g)))
    return DeintGeometry(tuple(tuple(r) for r in g.rect), tuple(g.plane_off), tuple(g.plane_pitch), int(g.frame_bytes))


def deint_job_table(jobs) -> np.ndarray:
    """A host job table (DEINT_JOB_DTYPE) of `jobs`: such an array already, or an iterable of jobs, each a
    mapping or a sequence (cur, prev, next, keep, second, mode)."""
    if isinstance(jobs, np.ndarray) and jobs.dtype == DEINT_JOB_DTYPE:
        return np.ascontiguousarray(jobs.reshape(-1))
    rows = list(jobs)
    tab = np.zeros(len(rows), DEINT_JOB_DTYPE)
    for i, row in enumerate(rows):
        if hasattr(row, "keys"):
            for k in row.keys():
                tab[i][k] = row[k]
        else:
            if len(row) != 6:
                raise ValueError("a job is (cur, prev, next, keep, second, mode)")
            for k, v in zip(DEINT_JOB_DTYPE.names, row):
                tab[i][k] = int(v)
    return tab


def deint_job_status(job, num_frames: int) -> int:
    """h264r_deint_job_status (host only, no GPU) of one job -- a DeintJob, or one row of a job table: the
    library's status, H264R_OK for a record the device accepts."""
    from . import lib
    if not isinstance(job, DeintJob):
        job = DeintJob.from_buffer_copy(deint_job_table([job] if not isinstance(job, np.ndarray) else job)[:1].tobytes())
    return int(lib().h264r_deint_job_status(C.byref(job), num_frames))


def deint_jobs(n_frames: int, tff: bool = True, mode: int = DEINT_ADAPTIVE, field_rate: bool = False) -> np.ndarray:
    """The usual job table for n_frames interlaced frames in display order, tff: the top field is the
    first in time.  At frame rate one job per frame, keeping its first field; at field rate two, the first
    field (second 0) and then the other (second 1).  prev is -1 at the start, next -1 at the end."""
    first = 0 if tff else 1
    per = 2 if field_rate else 1
    tab = np.zeros(n_frames * per, DEINT_JOB_DTYPE)
    for i in range(n_frames):
        for s in range(per):
            tab[i * per + s] = (i, i - 1 if i else -1, i + 1 if i + 1 < n_frames else -1, first ^ s, s, mode)
    return tab


def bind(L) -> None:
    """Declare the prototypes of include/h264r_output.h and include/h264r_deinterlace.h on the library
    (h264r.lib())."""
    P, I = C.c_void_p, C.c_int
    L.h264r_deinterlace_geometry.argtypes = [I, C.POINTER(OutDesc), C.POINTER(DeintGeom)]
    L.h264r_deinterlace_geometry.restype = I
    L.h264r_deint_job_status.argtypes = [C.POINTER(DeintJob), I]
    L.h264r_deint_job_status.restype = I
    L.h264r_deinterlace.argtypes = [P, C.POINTER(OutDesc), P, I, P, I, P, C.c_int64, P]
    L.h264r_deinterlace.restype = I
    L.h264r_output_geometry.argtypes = [I, C.POINTER(OutDesc), C.POINTER(OutGeom)]
    L.h264r_output_geometry.restype = I
    L.h264r_output_frames.argtypes = [P, C.POINTER(OutDesc), P, I, P, C.c_int64, P]
    L.h264r_output_frames.restype = I
    L.h264r_rgb_coefficients.argtypes = [I, I, C.POINTER(C.c_int32)]
    L.h264r_rgb_coefficients.restype = I
    L.h264r_output_rgb_geometry.argtypes = [I, C.POINTER(RgbDesc), C.POINTER(RgbGeom)]
    L.h264r_output_rgb_geometry.restype = I
    L.h264r_output_rgb.argtypes = [P, C.POINTER(RgbDesc), P, I, P, C.c_int64, P]
    L.h264r_output_rgb.restype = I
    L.h264r_output_rgb_scaled_geometry.argtypes = [I, C.POINTER(ScaleDesc), C.POINTER(RgbGeom)]
    L.h264r_output_rgb_scaled_geometry.restype = I
    L.h264r_output_rgb_scaled.argtypes = [P, C.POINTER(ScaleDesc), P, I, P, C.c_int64, P]
    L.h264r_output_rgb_scaled.restype = I
    L.h264r_output_rgb_boxes_geometry.argtypes = [I, C.POINTER(BoxesDesc), C.POINTER(RgbGeom)]
    L.h264r_output_rgb_boxes_geometry.restype = I
    L.h264r_out_box_status.argtypes = [I, C.POINTER(BoxesDesc), C.POINTER(OutBox), I, I]
    L.h264r_out_box_status.restype = I
    L.h264r_output_rgb_boxes.argtypes = [P, C.POINTER(BoxesDesc), P, I, P, I, P, C.c_int64, I, P]
    L.h264r_output_rgb_boxes.restype = I
    PI32 = C.POINTER(C.c_int32)
    L.h264r_output_rgb_resampled_geometry.argtypes = [I, C.POINTER(ResampleDesc), C.POINTER(RgbGeom)]
    L.h264r_output_rgb_resampled_geometry.restype = I
    L.h264r_resample_axis.argtypes = [I, I, I, I, I, PI32, PI32, PI32, PI32]
    L.h264r_resample_axis.restype = I
    L.h264r_resample_plan_create.argtypes = [P, C.POINTER(ResampleDesc), C.POINTER(P)]
    L.h264r_resample_plan_create.restype = I
    L.h264r_resample_plan_destroy.argtypes = [P]
    L.h264r_resample_plan_destroy.restype = None
    L.h264r_output_rgb_resampled.argtypes = [P, P, P, I, P, C.c_int64, P]
    L.h264r_output_rgb_resampled.restype = I


@dataclass(frozen=True)
class DeviceGeometry:
    """h264r_out_geom: the crop windows inside the coded planes and the layout of one output frame."""
    luma: tuple[int, int, int, int]
    chroma: tuple[int, int, int, int]
    plane_off: tuple[int, int, int]
    plane_pitch: tuple[int, int, int]
    frame_bytes: int


def _desc(width_mbs: int, frame_height_mbs: int, crop: Crop, layout: int, pitch_align: int, fake_chroma) -> OutDesc:
    return OutDesc(width_mbs, frame_height_mbs, crop.left, crop.right, crop.top, crop.bottom, crop.frame_mbs_only,
                   layout, pitch_align, int(fake_chroma))


def device_geometry(width_mbs: int, frame_height_mbs: int, crop: Crop = Crop(), chroma_format: int = 1,
                    layout: int = PLANAR, pitch_align: int = 0, fake_chroma: bool = False) -> DeviceGeometry:
    """h264r_output_geometry (host only, no GPU): raises H264RError with the library's status."""
    from . import _check, lib
    g = OutGeom()
    d = _desc(width_mbs, frame_height_mbs, crop, layout, pitch_align, fake_chroma)
    _check("h264r_output_geometry", lib().h264r_output_geometry(chroma_format, C.byref(d), C.byref(g)))
    return DeviceGeometry(tuple(g.luma), tuple(g.chroma), tuple(g.plane_off), tuple(g.plane_pitch), int(g.frame_bytes))


def pair_fields(structures: Sequence[int], pocs: Sequence[int]) -> list[tuple[int, int, int]]:
    """Decoded pictures (decoding order: h264r_pic.structure and POC of each) -> the output frames, in
    output order, as (kind, picture, second picture or -1).  Two consecutive field pictures of opposite
    parity make one H264R_OUT_FIELD_PAIR (top field first in the tuple, whichever was decoded first)
    with the smaller of their POCs; a field without its partner is an unpaired field; frames and MBAFF
    frames are H264R_OUT_FRAME.  Frames leave in POC order inside each IDR period, a new period at
    every POC 0 after the first frame -- the order the reference's DPB writes them (dpb.cc)."""
    TOP, BOTTOM = 1, 2                                   # H264R_TOP_FIELD, H264R_BOTTOM_FIELD
    frames, i, n = [], 0, len(structures)
    while i < n:
        st, poc = int(structures[i]), int(pocs[i])
        if st not in (TOP, BOTTOM):
            frames.append((poc, OUT_FRAME, i, -1))
            i += 1
        elif i + 1 < n and int(structures[i + 1]) == TOP + BOTTOM - st:
            top, bot = (i, i + 1) if st == TOP else (i + 1, i)
            frames.append((min(poc, int(pocs[i + 1])), OUT_FIELD_PAIR, top, bot))
            i += 2
        else:
            frames.append((poc, OUT_UNPAIRED_TOP if st == TOP else OUT_UNPAIRED_BOT, i, -1))
            i += 1
    keys, period = [], 0
    for k, f in enumerate(frames):
        if k and f[0] == 0:
            period += 1
        keys.append((period, f[0], k))
    return [frames[k][1:] for _, _, k in sorted(keys)]


@dataclass
class FrameTable:
    """A device array of h264r_out_frame and what keeps its sources alive."""
    tensor: object                  # torch uint8 [n * 56] on the device
    n: int
    keep: list


class DeviceOutput:
    """h264r_output_frames for one geometry on one Decoder (its chroma format and device).

        out = DeviceOutput(dec, W, H, Crop(bottom=4))
        table = out.frames_from([(OUT_FRAME, (y, u, v)), (OUT_FIELD_PAIR, (ty, tu, tv), (by, bu, bv))])
        frames = out.run(table)             # torch uint8 [n, frame_bytes] on the device
    """

    def __init__(self, decoder, width_mbs: int, frame_height_mbs: int, crop: Crop = Crop(), layout: int = PLANAR,
                 pitch_align: int = 0, fake_chroma: bool = False):
        self.decoder = decoder
        self.chroma_format = decoder._fmt
        self.desc = _desc(width_mbs, frame_height_mbs, crop, layout, pitch_align, fake_chroma)
        self.geom = device_geometry(width_mbs, frame_height_mbs, crop, self.chroma_format, layout, pitch_align,
                                    fake_chroma)

    @staticmethod
    def _addr(x) -> int:
        if x is None:
            return 0
        return int(x.data_ptr()) if hasattr(x, "data_ptr") else int(x)

    def frames_from(self, kinds_and_tensors, device: str = "cuda") -> FrameTable:
        """The device frame table of [(kind, (y, u, v)[, (y, u, v) of the bottom field])]: planes are
        torch tensors on the device or raw device addresses; None is a NULL pointer (u, v on 4:0:0)."""
        import torch
        rows = list(kinds_and_tensors)
        tab = np.zeros(len(rows), OUT_FRAME_DTYPE)
        keep = []
        for i, row in enumerate(rows):
            tab[i]["kind"] = int(row[0])
            for s, planes in enumerate(row[1:3]):
                if planes is None:
                    continue
                for name, p in zip(("y", "u", "v"), planes):
                    tab[i][name][s] = self._addr(p)
                    keep.append(p)
        t = torch.from_numpy(tab.view(np.uint8).reshape(-1).copy()).to(device)
        return FrameTable(t, len(rows), keep)

    def _call(self, who: str, fn: str, plan, table, n, dst, stream):
        """The call path of run, rgb and rgb_scaled: the library's `fn` on the frame table (a FrameTable, or
        a raw device address with n), the descriptor and the geometry that plan() returns, and dst: checked,
        or a new tensor of the geometry's frame_bytes per frame.  Returns (dst, n, geometry)."""
        import torch
        from . import _check
        if isinstance(table, FrameTable):
            n = table.n if n is None else n
            tptr = table.tensor.data_ptr()
        else:
            tptr = self._addr(table)
        if n is None:
            raise ValueError(f"{who}: n is needed with a raw frame table")
        d, g = plan()
        if dst is None:
            dst = torch.empty((n, g.frame_bytes), dtype=torch.uint8, device="cuda")
        if dst.dim() != 2 or dst.shape[0] < n or dst.stride(1) != 1 or dst.dtype != torch.uint8:
            raise ValueError(f"{who}: dst must be a uint8 tensor [n, dst_frame_stride] with contiguous rows")
        _check(fn, getattr(self.decoder._L, fn)(self.decoder.handle, C.byref(d), C.c_void_p(tptr), n,
                                                C.c_void_p(dst.data_ptr()), dst.stride(0), C.c_void_p(stream or 0)))
        return dst, n, g

    def run(self, table, n: int | None = None, dst=None, stream: int | None = None):
        """Write n frames (default: the whole table).  dst: a torch uint8 tensor [n, dst_frame_stride]
        on the device (written in place: padding and the bytes past frame_bytes keep what they hold) or
        None = a new [n, frame_bytes] tensor.  Asynchronous on `stream` (a hipStream_t address; None =
        the context's stream): Decoder.check() before the result is read on another stream."""
        return self._call("run", "h264r_output_frames", lambda: (self.desc, self.geom), table, n, dst, stream)[0]

    def rgb(self, table, n: int | None = None, *, matrix: int = CSC_BT709, full_range: bool = False,
            chroma_up: int = UP_REPLICATE, format: int = RGB_PLANAR_U8, bgr: bool = False, alpha: int = 255,
            scale=(1 / 255,) * 3, bias=(0,) * 3, dst=None, stream: int | None = None):
        """h264r_output_rgb on the same frame table: n RGB frames (default: the whole table) of this
        geometry (planar layout, no fake chroma), as a torch tensor that views the destination:
        [n, H, W, 3 | 4] uint8 for the packed formats, [n, 3, H, W] uint8 or float16 for the planar ones
        -- a strided view when pitch_align pads the rows.  dst: a torch uint8 tensor [n, dst_frame_stride]
        on the device, written in place (for PLANAR_F16 its address and stride must be even), or None =
        a new one of frame_bytes per frame.  Asynchronous on `stream`, as run()."""
        def plan():
            d = rgb_desc(self.desc, matrix, full_range, chroma_up, format, bgr, alpha, scale, bias)
            return d, rgb_geometry(d, self.chroma_format)
        dst, n, g = self._call("rgb", "h264r_output_rgb", plan, table, n, dst, stream)
        return rgb_view(dst[:n], g, format)

    def rgb_scaled(self, table, out_w: int, out_h: int, n: int | None = None, *, roi=None, filter: int = SCALE_AREA,
                   matrix: int = CSC_BT709, full_range: bool = False, chroma_up: int = UP_REPLICATE,
                   format: int = RGB_PLANAR_U8, bgr: bool = False, alpha: int = 255, scale=(1 / 255,) * 3, bias=(0,) * 3,
                   dst=None, stream: int | None = None):
        """h264r_output_rgb_scaled on the same frame table: the region `roi` = (x, y, w, h) of every RGB
        frame (luma samples of the cropped rectangle; None = all of it) resampled to out_w x out_h by
        `filter`, without the full-size frames.  The other keywords, dst and the tensor returned are
        those of rgb(), at the output size: [n, out_h, out_w, 3 | 4] or [n, 3, out_h, out_w]; this
        geometry's pitch_align pads the output rows."""
        def plan():
            d = scale_desc(rgb_desc(self.desc, matrix, full_range, chroma_up, format, bgr, alpha, scale, bias), out_w, out_h,
                           roi, filter)
            return d, scaled_geometry(d, self.chroma_format)
        dst, n, g = self._call("rgb_scaled", "h264r_output_rgb_scaled", plan, table, n, dst, stream)
        return rgb_view(dst[:n], g, format)

    def resample_plan(self, out_w: int, out_h: int, roi=None, filter: int = RESAMPLE_BICUBIC, *, matrix: int = CSC_BT709,
                      full_range: bool = False, chroma_up: int = UP_REPLICATE, format: int = RGB_PLANAR_U8, bgr: bool = False,
                      alpha: int = 255, scale=(1 / 255,) * 3, bias=(0,) * 3) -> ResamplePlan:
        """h264r_resample_plan_create for this geometry: the region `roi` = (x, y, w, h) of every RGB frame
        (Pillow's box; None = all of it) to out_w x out_h by `filter` (RESAMPLE_*), the other keywords those
        of rgb().  Synchronous: the tables are built on the host and uploaded.  One plan serves any number
        of rgb_resampled() calls; close() it (or leave a with block) after they are done."""
        d = resample_desc(rgb_desc(self.desc, matrix, full_range, chroma_up, format, bgr, alpha, scale, bias), out_w, out_h, roi,
                          filter)
        return ResamplePlan(self.decoder, d, resampled_geometry(d, self.chroma_format))

    def rgb_resampled(self, table, plan: ResamplePlan, n: int | None = None, dst=None, stream: int | None = None):
        """h264r_output_rgb_resampled on the same frame table: n frames (default: the whole table) resampled
        by `plan` exactly as Pillow's Image.resize would resample the RGB frames, without the full-size
        frames.  dst and the tensor returned are those of rgb_scaled(): [n, out_h, out_w, 3 | 4] or
        [n, 3, out_h, out_w]; this geometry's pitch_align pads the output rows.  Asynchronous on `stream`,
        as run()."""
        import torch
        from . import _check
        if isinstance(table, FrameTable):
            n = table.n if n is None else n
            tptr = table.tensor.data_ptr()
        else:
            tptr = self._addr(table)
        if n is None:
            raise ValueError("rgb_resampled: n is needed with a raw frame table")
        if not plan.handle:
            raise ValueError("rgb_resampled: the plan is closed")
        g = plan.geom
        if dst is None:
            dst = torch.empty((n, g.frame_bytes), dtype=torch.uint8, device="cuda")
        if dst.dim() != 2 or dst.shape[0] < n or dst.stride(1) != 1 or dst.dtype != torch.uint8:
            raise ValueError("rgb_resampled: dst must be a uint8 tensor [n, dst_frame_stride] with contiguous rows")
        _check("h264r_output_rgb_resampled",
               self.decoder._L.h264r_output_rgb_resampled(self.decoder.handle, plan.handle, C.c_void_p(tptr), n,
                                                          C.c_void_p(dst.data_ptr()), dst.stride(0), C.c_void_p(stream or 0)))
        return rgb_view(dst[:n], g, plan.format)

    def deinterlace(self, table, jobs, dst=None, stream: int | None = None, *, n: int | None = None,
                    num_jobs: int | None = None):
        """h264r_deinterlace on the same frame table: one progressive frame per job of `jobs` -- a host
        table (deint_job_table's input: a DEINT_JOB_DTYPE array such as deint_jobs() returns, or an iterable
        of jobs), uploaded here; or a torch uint8 tensor on the device that holds h264r_deint_job records;
        or a raw device address with num_jobs.  Needs this geometry planar, without pitch_align and
        fake_chroma.  Returns the torch uint8 tensor [num_jobs, frame_bytes] of coded-size planes (dst, if
        given: [num_jobs, dst_frame_stride], of which only the cropped rectangles are written; None = a new
        ZERO-FILLED one); frames_of() names its frames to the other calls.  Asynchronous on `stream`, as
        run()."""
        import torch
        from . import _check
        if isinstance(table, FrameTable):
            n = table.n if n is None else n
            tptr = table.tensor.data_ptr()
        else:
            tptr = self._addr(table)
        if n is None:
            raise ValueError("deinterlace: n is needed with a raw frame table")
        keep = None
        if hasattr(jobs, "data_ptr"):
            if jobs.dtype != torch.uint8 or not jobs.is_contiguous() or jobs.numel() % DEINT_JOB_DTYPE.itemsize:
                raise ValueError("deinterlace: a device job table is a contiguous uint8 tensor of 24-byte records")
            num_jobs = jobs.numel() // DEINT_JOB_DTYPE.itemsize if num_jobs is None else num_jobs
            jptr = jobs.data_ptr()
        elif isinstance(jobs, int):
            if num_jobs is None:
                raise ValueError("deinterlace: num_jobs is needed with a raw job table")
            jptr = jobs
        else:
            tab = deint_job_table(jobs)
            num_jobs = len(tab) if num_jobs is None else num_jobs
            # one record more than the table holds: an empty table still has an address
            raw = np.concatenate([tab.view(np.uint8).reshape(-1), np.zeros(DEINT_JOB_DTYPE.itemsize, np.uint8)])
            keep = torch.from_numpy(raw).to("cuda")
            jptr = keep.data_ptr()
        g = deint_geometry(self.desc, self.chroma_format)
        if dst is None:
            dst = torch.zeros((num_jobs, g.frame_bytes), dtype=torch.uint8, device="cuda")
        if dst.dim() != 2 or dst.shape[0] < num_jobs or dst.stride(1) != 1 or dst.dtype != torch.uint8:
            raise ValueError("deinterlace: dst must be a uint8 tensor [num_jobs, dst_frame_stride] with contiguous rows")
        _check("h264r_deinterlace",
               self.decoder._L.h264r_deinterlace(self.decoder.handle, C.byref(self.desc), C.c_void_p(tptr), n, C.c_void_p(jptr),
                                                 num_jobs, C.c_void_p(dst.data_ptr()), dst.stride(0), C.c_void_p(stream or 0)))
        if keep is not None:
            self._deint_tables = [keep]                     # alive until the next call replaces it
        return dst[:num_jobs]

    def frames_of(self, view) -> FrameTable:
        """The frame table that names the frames of deinterlace()'s result -- `view`, [n, stride] -- as
        H264R_OUT_FRAME sources for run(), rgb() and the other calls of this geometry."""
        g = deint_geometry(self.desc, self.chroma_format)
        if view.dim() != 2 or view.stride(1) != 1 or view.shape[1] < g.frame_bytes:
            raise ValueError("frames_of: view must be deinterlace()'s [n, dst_frame_stride] tensor")
        base, stride = view.data_ptr(), view.stride(0)
        rows = [(OUT_FRAME, tuple(base + i * stride + g.plane_off[k] if k == 0 or self.chroma_format else None for k in range(3)))
                for i in range(view.shape[0])]
        table = self.frames_from(rows)
        table.keep.append(view)
        return table

    def rgb_boxes(self, table, boxes, image_w: int, image_h: int, num_images: int, *, n: int | None = None,
                  num_boxes: int | None = None, max_out=None, filter: int = SCALE_AREA, matrix: int = CSC_BT709,
                  full_range: bool = False, chroma_up: int = UP_REPLICATE, format: int = RGB_PLANAR_U8, bgr: bool = False,
                  alpha: int = 255, scale=(1 / 255,) * 3, bias=(0,) * 3, dst=None, stream: int | None = None):
        """h264r_output_rgb_boxes: every box of `boxes` -- a region of a frame of the table, resampled by
        `filter` to the box's own size -- into its place in one of num_images images of image_w x image_h,
        in one job.  boxes: a host table (boxes_table's input: an OUT_BOX_DTYPE array or an iterable of
        boxes), uploaded here; or a torch uint8 tensor on the device that holds h264r_out_box records; or
        a raw device address with num_boxes.  max_out = (w, h) bounds every box's output size (None: the
        image's size; the launch is sized by it).  The other keywords and the tensor returned are those of
        rgb(), at the image size: [num_images, image_h, image_w, 3 | 4] or [num_images, 3, image_h,
        image_w]; this geometry's pitch_align pads the image rows.  dst: a torch uint8 tensor [num_images,
        dst_image_stride] on the device, of which only the boxes' pixels are written, or None = new
        ZERO-FILLED images.  Asynchronous on `stream`, as run()."""
        import torch
        from . import _check
        if isinstance(table, FrameTable):
            n = table.n if n is None else n
            tptr = table.tensor.data_ptr()
        else:
            tptr = self._addr(table)
        if n is None:
            raise ValueError("rgb_boxes: n is needed with a raw frame table")
        keep = None
        if hasattr(boxes, "data_ptr"):
            if boxes.dtype != torch.uint8 or not boxes.is_contiguous() or boxes.numel() % OUT_BOX_DTYPE.itemsize:
                raise ValueError("rgb_boxes: a device box table is a contiguous uint8 tensor of 48-byte records")
            num_boxes = boxes.numel() // OUT_BOX_DTYPE.itemsize if num_boxes is None else num_boxes
            bptr = boxes.data_ptr()
        elif isinstance(boxes, int):
            if num_boxes is None:
                raise ValueError("rgb_boxes: num_boxes is needed with a raw box table")
            bptr = boxes
        else:
            tab = boxes_table(boxes)
            num_boxes = len(tab) if num_boxes is None else num_boxes
            # one record more than the table holds: an empty table still has an address
            raw = np.concatenate([tab.view(np.uint8).reshape(-1), np.zeros(OUT_BOX_DTYPE.itemsize, np.uint8)])
            keep = torch.from_numpy(raw).to("cuda")
            bptr = keep.data_ptr()
        d = boxes_desc(rgb_desc(self.desc, matrix, full_range, chroma_up, format, bgr, alpha, scale, bias), image_w, image_h,
                       max_out, filter)
        g = boxes_geometry(d, self.chroma_format)
        if dst is None:
            dst = torch.zeros((num_images, g.frame_bytes), dtype=torch.uint8, device="cuda")
        if dst.dim() != 2 or dst.shape[0] < num_images or dst.stride(1) != 1 or dst.dtype != torch.uint8:
            raise ValueError("rgb_boxes: dst must be a uint8 tensor [num_images, dst_image_stride] with contiguous rows")
        _check("h264r_output_rgb_boxes",
               self.decoder._L.h264r_output_rgb_boxes(self.decoder.handle, C.byref(d), C.c_void_p(tptr), n, C.c_void_p(bptr),
                                                      num_boxes, C.c_void_p(dst.data_ptr()), dst.stride(0), num_images,
                                                      C.c_void_p(stream or 0)))
        if keep is not None:
            self._box_tables = [keep]                       # alive until the next job replaces it
        return rgb_view(dst[:num_images], g, format)
