"""Decoder output: 8-bit RGB / YUV frames and 10 / 12 / 16-bit planar YUV frames from the render loop, to host memory and to files
(host side of csrc/frames_out.hip).

``render_frames`` yields float32 ``[3, H, W]`` images in device memory; a player, ``ffmpeg`` or a quality tool takes 8-bit frames.
The reference converts on the host, one frame at a time (utils/report_utils.py:412-447: average the views, clamp, ``ToPILImage``,
``d{idx:05d}.png``).  Here the conversion is one HIP launch per render batch (``frames_to_u8``), the small result is copied to
pinned host memory on a stream of its own while the next batch composites (``render_frames_u8``), and ``write_video`` feeds a
sink — ``Y4MWriter``, ``RawWriter``, ``PNGWriter`` — from one background thread.

The conversion (include/gsvc_hip.h, gsvc_frames_to_u8): clamp to [0, 1] (NaN -> 0); ``rgb24`` interleaved ``[H, W, 3]``, or planar
Y, Cb, Cr (``yuv444p`` / ``yuv420p``, BT.709 or BT.601 weights, limited or full range; 4:2:0 chroma is the mean of the 2x2 block
taken in float: centre siting, Y4M's ``C420jpeg``); rounding ``trunc`` (what ``ToPILImage`` does; the default of ``rgb24``) or
``nearest`` (the default of the YUV layouts).

Deep frames (``FrameFormat(depth=10 | 12 | 16)``, ``yuv444p`` / ``yuv420p`` only; gsvc_frames_to_u16): every sample is one little-endian
16-bit word whose upper bits are zero — ffmpeg's ``yuv420p10le``, Y4M's ``C420p10``.  A frame still travels as a flat ``uint8`` buffer
of ``frame_bytes`` (twice the 8-bit count): the ``_u8`` in ``frames_to_u8`` / ``render_frames_u8`` means "a buffer of bytes", not
"8-bit samples", and the pinned double buffer, ``write_frames`` and the sinks carry deep frames as they carry 8-bit ones.

Importing this module needs neither a GPU nor the built library; ``frames_to_u8`` and what is built on it do (no CPU fallback).
"""
from __future__ import annotations

import os
import queue
import threading
import time
from dataclasses import dataclass

import numpy as np

from . import _lib

LAYOUTS = {"rgb24": 0, "yuv444p": 1, "yuv420p": 2}          # the GSVC_FRAMES_* enums of include/gsvc_hip.h
MATRICES = {"bt709": 0, "bt601": 1}
RANGES = {"limited": 0, "full": 1}
ROUNDINGS = {"trunc": 0, "nearest": 1}
DEPTHS = (8, 10, 12, 16)                                     # bits per sample; above 8: one little-endian 16-bit word per sample
MAX_BATCH = 16                                               # GSVC_FRAMES_MAX_BATCH: images per launch


@dataclass(frozen=True)
class FrameFormat:
    """What a frame looks like.  ``rounding=None`` takes the layout's default: ``trunc`` for ``rgb24`` (bit-equal to the
    reference's PNGs), ``nearest`` for YUV.  ``matrix`` and ``range`` do not apply to ``rgb24`` (always 255 c).  ``depth``: bits per
    sample, 8, or 10 / 12 / 16 for the planar YUV layouts (little-endian 16-bit words)."""
    layout: str = "yuv420p"
    matrix: str = "bt709"
    range: str = "limited"
    rounding: str | None = None
    depth: int = 8

    def __post_init__(self):
        for what, value, table in (("layout", self.layout, LAYOUTS), ("matrix", self.matrix, MATRICES), ("range", self.range, RANGES)):
            if value not in table:
                raise ValueError(f"FrameFormat: unknown {what} {value!r} (one of {', '.join(table)})")
        if self.rounding is not None and self.rounding not in ROUNDINGS:
            raise ValueError(f"FrameFormat: unknown rounding {self.rounding!r} (one of {', '.join(ROUNDINGS)} or None)")
        if isinstance(self.depth, bool) or self.depth not in DEPTHS:
            raise ValueError(f"FrameFormat: unknown depth {self.depth!r} (one of {', '.join(str(d) for d in DEPTHS)})")
        if self.layout == "rgb24" and self.depth != 8:
            raise ValueError(f"FrameFormat: rgb24 frames are 8-bit (got depth {self.depth})")

    @property
    def rounding_used(self) -> str:
        return self.rounding if self.rounding is not None else ("trunc" if self.layout == "rgb24" else "nearest")

    @property
    def name(self) -> str:
        """ffmpeg's spelling of layout and depth: ``yuv420p``, ``rgb24``, ``yuv444p10le``."""
        return self.layout if self.depth == 8 else f"{self.layout}{self.depth}le"

    @classmethod
    def from_name(cls, name: str, matrix: str = "bt709", range: str = "limited", rounding: str | None = None) -> "FrameFormat":
        """``yuv420p`` / ``yuv444p`` / ``rgb24``, or a deep spelling ``yuv4{20,44}p{10,12,16}[le]``."""
        text = str(name)
        if text in LAYOUTS:
            return cls(text, matrix, range, rounding)
        stem = text[:-2] if text.endswith("le") else text
        for layout in ("yuv420p", "yuv444p"):
            if stem.startswith(layout) and stem[len(layout):] in ("10", "12", "16"):
                return cls(layout, matrix, range, rounding, int(stem[len(layout):]))
        raise ValueError(f"FrameFormat: unknown format name {name!r} (yuv420p, yuv444p, rgb24 or yuv4{{20,44}}p{{10,12,16}}[le])")


def frame_bytes(H: int, W: int, fmt: FrameFormat = FrameFormat()) -> int:
    """Bytes of one frame: 3 H W (``rgb24``, ``yuv444p``) or H W 3 / 2 (``yuv420p``: one I420 frame; H and W even); twice that for
    a deep format (``fmt.depth`` above 8: two bytes per sample)."""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"frame_bytes: image size must be positive (got {H} x {W})")
    per = 2 if fmt.depth > 8 else 1
    if fmt.layout == "yuv420p":
        if H % 2 or W % 2:
            raise ValueError(f"frame_bytes: yuv420p needs even H and W (got {H} x {W})")
        return H * W * 3 // 2 * per
    return 3 * H * W * per


def planes(buf, H: int, W: int, fmt: FrameFormat = FrameFormat()):
    """Views into one flat uint8 frame (numpy array or tensor): ``(rgb [H, W, 3],)`` or ``(y [H, W], u, v)`` with u, v ``[H, W]``
    (``yuv444p``) or ``[H / 2, W / 2]`` (``yuv420p``).  Deep formats: the views are little-endian uint16 (``'<u2'`` / ``torch.uint16``)
    over the same bytes; the frame must then start at an even address."""
    n = frame_bytes(H, W, fmt)
    flat = buf.reshape(-1)
    if flat.shape[0] != n:
        raise ValueError(f"planes: a {fmt.name} frame of {H} x {W} has {n} bytes, got {flat.shape[0]}")
    if fmt.depth > 8:
        if isinstance(flat, np.ndarray):
            flat = flat.view("<u2")
        else:
            import torch
            flat = flat.view(torch.uint16)          # (this project runs on little-endian hosts only)
    if fmt.layout == "rgb24":
        return (flat.reshape(H, W, 3),)
    ch, cw = (H // 2, W // 2) if fmt.layout == "yuv420p" else (H, W)
    y, u, v = flat[:H * W], flat[H * W:H * W + ch * cw], flat[H * W + ch * cw:]
    return y.reshape(H, W), u.reshape(ch, cw), v.reshape(ch, cw)


def rgb24_to_image(frame, H: int, W: int):
    """A flat ``rgb24`` frame (uint8 tensor) as the float image ``[3, H, W]`` = u8 / 255 a metric takes."""
    return (planes(frame, H, W, FrameFormat("rgb24"))[0].permute(2, 0, 1).float() / 255.0).contiguous()


# ----------------------------------------------------------------------------------------------------------------------------
# device side
# ----------------------------------------------------------------------------------------------------------------------------
def frames_to_u8(images, fmt: FrameFormat = FrameFormat(), out=None):
    """float32 CUDA images ``[3, H, W]`` of one size (a sequence, or one ``[n, 3, H, W]`` tensor) -> uint8 ``[n, frame_bytes]`` on
    their device, one launch per 16 images on the current stream; nothing synchronises.  The ``_u8`` of the name means "a buffer of
    bytes": a deep format (``fmt.depth`` above 8) gives little-endian 16-bit samples in that buffer (``planes`` views them), and
    ``out`` must then start at an even address with an even row stride.  Images that are not contiguous are made
    so.  ``out``: a uint8 CUDA tensor ``[n, >= frame_bytes]`` whose rows are contiguous (bytes of a row past the frame are left
    alone); the return value is its ``[:, :frame_bytes]`` view."""
    import ctypes as C

    import torch
    images = list(images.unbind(0)) if isinstance(images, torch.Tensor) and images.dim() == 4 else list(images)
    if not images:
        raise ValueError("frames_to_u8: no images")
    first = images[0]
    for img in images:
        if not isinstance(img, torch.Tensor) or not img.is_cuda:
            raise _lib.GsvcError("frames_to_u8 runs on the HIP kernels of csrc/frames_out.hip; CPU tensors are not supported")
        if img.dtype != torch.float32 or img.dim() != 3 or img.shape[0] != 3:
            raise ValueError(f"frames_to_u8: images must be float32 [3, H, W] (got {img.dtype} {tuple(img.shape)})")
        if img.shape != first.shape or img.device != first.device:
            raise ValueError("frames_to_u8: the images of one call must have one size and one device")
    H, W = int(first.shape[1]), int(first.shape[2])
    nbytes = frame_bytes(H, W, fmt)
    n = len(images)
    if out is None:
        out = torch.empty((n, nbytes), dtype=torch.uint8, device=first.device)
    elif (out.dtype != torch.uint8 or out.device != first.device or out.dim() != 2 or out.shape[0] != n or out.shape[1] < nbytes
          or out.stride(1) != 1 or (n > 1 and out.stride(0) < nbytes)):
        raise ValueError(f"frames_to_u8: out must be uint8 [{n}, >= {nbytes}] with contiguous rows on {first.device}")
    L = _lib.lib()
    stride = int(out.stride(0)) if n > 1 else max(int(out.stride(0)), nbytes)
    if fmt.depth > 8 and n == 1:
        stride += stride & 1          # (one frame: the stride addresses nothing)
    with torch.cuda.device(first.device):
        stream = _lib.current_stream(first.device)
        for i in range(0, n, MAX_BATCH):
            chunk = [img.contiguous() for img in images[i:i + MAX_BATCH]]      # (alive until the launch is enqueued on their stream)
            ptrs = (C.c_void_p * len(chunk))(*[img.data_ptr() for img in chunk])
            if fmt.depth > 8:
                _lib.check(L.gsvc_frames_to_u16(ptrs, len(chunk), H, W, LAYOUTS[fmt.layout], MATRICES[fmt.matrix], RANGES[fmt.range],
                                                ROUNDINGS[fmt.rounding_used], fmt.depth, out.data_ptr() + i * stride, stride, stream),
                           "gsvc_frames_to_u16")
                continue
            _lib.check(L.gsvc_frames_to_u8(ptrs, len(chunk), H, W, LAYOUTS[fmt.layout], MATRICES[fmt.matrix], RANGES[fmt.range],
                                           ROUNDINGS[fmt.rounding_used], out.data_ptr() + i * stride, stride, stream),
                       "gsvc_frames_to_u8")
    return out[:, :nbytes]


def delivered_images(images, fmt: FrameFormat = FrameFormat(), chroma: str = "bilinear"):
    """The float pictures ``[n, 3, H, W]`` a viewer of the delivered frames sees: ``frames_from_u8(frames_to_u8(images, fmt), H, W, fmt,
    chroma)`` — quantised to ``fmt.depth`` bits, 4:2:0 chroma subsampled and upsampled again — or, for ``rgb24``, ``rgb24_to_image`` of
    every frame (bytes / 255).  What a codec's PSNR is taken on (``report.evaluate(delivered=fmt)``)."""
    import torch
    u8 = frames_to_u8(images, fmt)
    first = images[0]
    H, W = int(first.shape[-2]), int(first.shape[-1])
    if fmt.layout == "rgb24":
        return torch.stack([rgb24_to_image(fr, H, W) for fr in u8])
    from .frames_in import frames_from_u8
    return frames_from_u8(u8, H, W, fmt, chroma)


def render_frames_u8(frames, pc, pipe, bg_color, fmt: FrameFormat = FrameFormat(), batch: int = 8, to_host: bool = True,
                     scaling_modifier=1.0, mode=None, on_device_batch=None, grain=None, first_frame: int = 0, out_size=None):
    """The decoder's render loop with frames of bytes as output (8-bit samples, or little-endian 16-bit samples for a deep ``fmt``): a
    generator over ``render_frames`` that converts each render batch with one
    launch and yields one flat uint8 frame (``frame_bytes`` long; ``planes`` splits it) per video frame, in order.

    ``to_host=True``: a batch is copied into one of two pinned host buffers by a non-blocking copy on a stream of its own, ordered
    by events, and handed out one batch late, after its event — by then the next batch is generated, composited, converted and on
    its way into the other buffer.  A yielded frame is a CPU tensor that VIEWS the pinned buffer: it is valid until the generator is
    advanced again; a caller that keeps frames copies them (``frame.clone()``, ``frame.numpy().copy()``).
    ``to_host=False``: yields device tensors, rows of a per-batch tensor that is never written again.
    ``on_device_batch``: called with every batch's converted frames, uint8 ``[n, frame_bytes]`` in device memory, on the current stream
    before they are yielded or copied to the host (``bitstream.decode_video`` takes their picture hashes there); what it launches on
    that stream is ordered before the buffer is written again.
    ``grain`` (``grain.GrainParams``; YUV formats only): film grain is added to every batch in place on the device
    (``grain.apply_grain``), behind ``on_device_batch`` — the hook sees the ungrained pictures — and before the batch is yielded or
    copied; ``first_frame`` is the index of ``frames[0]`` in the whole clip, which the grain of a frame is a function of.  Without
    ``grain`` the launches and events are what they were.
    ``out_size=(H, W)`` (YUV formats only): behind ``on_device_batch`` — the hook sees the pictures at the size they were rendered at —
    every batch is resampled on the device to this size (``resample.resample_frames``) into a buffer of its own; the pinned host
    buffers and the yielded frames have that size, and ``grain`` is applied after the resample, at that size.  None: nothing changes."""
    import torch

    from .generate import GenerateMode
    from .ortho_gaussian_renderer import render_frames
    if mode is None:
        mode = GenerateMode.DECODING_AS_IS
    frames = list(frames)
    if not frames:
        return
    batch = int(batch)
    if batch < 1:
        raise ValueError("render_frames_u8: batch must be at least 1")
    if grain is not None:
        from .grain import apply_grain
        if fmt.layout == "rgb24":
            raise ValueError("render_frames_u8: rgb24 frames take no film grain (it lives in the delivered Y'CbCr domain)")
    if out_size is not None:
        from .resample import resample_frames
        if fmt.layout == "rgb24":
            raise ValueError("render_frames_u8: rgb24 frames are not resampled (the resampler works on planar Y'CbCr codes)")
        out_H, out_W = (int(v) for v in out_size)
    source = render_frames(frames, pc, pipe, bg_color, scaling_modifier=scaling_modifier, mode=mode, batch=batch)
    dev = pc._anchor.device
    ring = None           # to_host: two (device buffer, pinned buffer, copied event)
    copy_stream = None
    waiting = None        # the batch whose copy is in flight: (pinned rows, event)
    for j, i in enumerate(range(0, len(frames), batch)):
        images = [next(source) for _ in range(min(batch, len(frames) - i))]
        n = len(images)
        if not to_host:
            rows = frames_to_u8(images, fmt)
            if on_device_batch is not None:
                on_device_batch(rows)
            gH, gW = images[0].shape[1], images[0].shape[2]
            if out_size is not None:
                rows, gH, gW = resample_frames(rows, gH, gW, fmt, out_H, out_W), out_H, out_W
            if grain is not None:
                apply_grain(rows, gH, gW, fmt, grain, first_frame=int(first_frame) + i)
            yield from rows.unbind(0)
            continue
        if ring is None:
            rH, rW = images[0].shape[1], images[0].shape[2]
            nbytes = frame_bytes(rH, rW, fmt) if out_size is None else frame_bytes(out_H, out_W, fmt)
            ring = [(torch.empty((batch, nbytes), dtype=torch.uint8, device=dev),
                     torch.empty((batch, nbytes), dtype=torch.uint8, pin_memory=True), torch.cuda.Event()) for _ in range(2)]
            copy_stream = torch.cuda.Stream(dev)
            # out_size: ONE buffer at the rendered size; its writer (the conversion) and its readers (the hook, the resample) all
            # run on the current stream
            rendered = None if out_size is None else torch.empty((batch, frame_bytes(rH, rW, fmt)), dtype=torch.uint8, device=dev)
        on_dev, on_host, copied = ring[j % 2]
        cur = torch.cuda.current_stream(dev)
        if j >= 2:
            cur.wait_event(copied)              # the copy of batch j - 2 out of this device buffer
        converted = torch.cuda.Event()
        if out_size is not None:                # the hook reads the rendered pictures, the copy takes the resampled (and grained) ones
            frames_to_u8(images, fmt, out=rendered[:n])
            if on_device_batch is not None:
                on_device_batch(rendered[:n])
            resample_frames(rendered[:n], rH, rW, fmt, out_H, out_W, out=on_dev[:n])
            if grain is not None:
                apply_grain(on_dev[:n], out_H, out_W, fmt, grain, first_frame=int(first_frame) + i)
            converted.record(cur)
        elif grain is None:
            frames_to_u8(images, fmt, out=on_dev[:n])
            converted.record(cur)
            if on_device_batch is not None:
                on_device_batch(on_dev[:n])     # (behind the event: the copy does not wait for it)
        else:                                   # the hook reads the ungrained pictures, the copy takes the grained ones
            frames_to_u8(images, fmt, out=on_dev[:n])
            if on_device_batch is not None:
                on_device_batch(on_dev[:n])
            apply_grain(on_dev[:n], images[0].shape[1], images[0].shape[2], fmt, grain, first_frame=int(first_frame) + i)
            converted.record(cur)
        with torch.cuda.stream(copy_stream):
            copy_stream.wait_event(converted)
            on_host[:n].copy_(on_dev[:n], non_blocking=True)
            copied.record(copy_stream)
        del images
        if waiting is not None:
            rows, ev = waiting
            ev.synchronize()
            yield from rows.unbind(0)           # (the consumer is done with them before batch j + 1 overwrites their buffer)
        waiting = (on_host[:n], copied)
    if waiting is not None:
        rows, ev = waiting
        ev.synchronize()
        yield from rows.unbind(0)


# ----------------------------------------------------------------------------------------------------------------------------
# sinks
# ----------------------------------------------------------------------------------------------------------------------------
def _as_bytes_array(frame) -> np.ndarray:
    """A frame (CPU uint8 tensor or numpy array, any shape) as a flat contiguous uint8 numpy array, without a copy where possible."""
    if not isinstance(frame, np.ndarray):
        frame = frame.detach().cpu().numpy() if hasattr(frame, "detach") else np.asarray(frame)
    if frame.dtype != np.uint8:
        raise ValueError(f"a frame must be uint8 (got {frame.dtype})")
    return np.ascontiguousarray(frame).reshape(-1)


class _Sink:
    """``write(frame_u8)`` / ``close()``; usable as a context manager.  ``frames`` and ``bytes`` count what was written."""

    def __init__(self):
        self.frames = 0
        self.bytes = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self):
        pass


class RawWriter(_Sink):
    """Frame payloads back to back, nothing else (``.yuv`` / ``.rgb``: the reader has to know size and format), any layout."""

    def __init__(self, path):
        super().__init__()
        self.path = str(path)
        self._f = open(self.path, "wb")

    def write(self, frame_u8):
        a = _as_bytes_array(frame_u8)
        self._f.write(a.data)
        self.frames += 1
        self.bytes += a.shape[0]

    def close(self):
        if self._f is not None:
            self._f.close()
            self._f = None


class Y4MWriter(_Sink):
    """YUV4MPEG2 file: header ``YUV4MPEG2 W{W} H{H} F{n}:{d} Ip A1:1 C420jpeg XCOLORRANGE=LIMITED`` (``C444`` / ``FULL`` as the
    format says; ``C420p10``, ``C444p12``, ... for a deep format), then ``FRAME\\n`` + payload per frame.  Y4M has no field for the matrix: a BT.601 file and a BT.709 file have the
    same header, and most readers guess BT.601 below 720 lines and BT.709 from there — say which one was written next to the file."""

    def __init__(self, path, W: int, H: int, fps=(30, 1), fmt: FrameFormat = FrameFormat()):
        super().__init__()
        if fmt.layout not in ("yuv420p", "yuv444p"):
            raise ValueError(f"Y4MWriter: a Y4M file holds yuv420p or yuv444p frames, not {fmt.layout}")
        self.path, self.W, self.H, self.fmt = str(path), int(W), int(H), fmt
        self.frame_bytes = frame_bytes(H, W, fmt)
        self.header = y4m_header(W, H, fps, fmt)
        self._f = open(self.path, "wb")
        self._f.write(self.header)
        self.bytes = len(self.header)

    def write(self, frame_u8):
        a = _as_bytes_array(frame_u8)
        if a.shape[0] != self.frame_bytes:
            raise ValueError(f"Y4MWriter: a {self.fmt.name} frame of {self.H} x {self.W} has {self.frame_bytes} bytes, got {a.shape[0]}")
        self._f.write(b"FRAME\n")
        self._f.write(a.data)
        self.frames += 1
        self.bytes += 6 + a.shape[0]

    def close(self):
        if self._f is not None:
            self._f.close()
            self._f = None


def y4m_header(W: int, H: int, fps=(30, 1), fmt: FrameFormat = FrameFormat()) -> bytes:
    n, d = (int(fps[0]), int(fps[1])) if isinstance(fps, (tuple, list)) else (int(fps), 1)
    if n < 1 or d < 1:
        raise ValueError(f"y4m_header: bad frame rate {fps!r}")
    chroma = {"yuv420p": "420jpeg", "yuv444p": "444"}[fmt.layout]
    if fmt.depth > 8:
        chroma = f"{chroma[:3]}p{fmt.depth}"
    return f"YUV4MPEG2 W{int(W)} H{int(H)} F{n}:{d} Ip A1:1 C{chroma} XCOLORRANGE={fmt.range.upper()}\n".encode("ascii")


def read_y4m(path):
    """``(header, frames)`` of a Y4M file of 4:2:0 / 4:4:4 frames of 8 (``C420jpeg``, ``C444``, ...), 10, 12 or 16 bits (``C420p10``,
    ``C444p12``, ...; every 4:2:0 tag is read as centre sited): header = {"W", "H", "fps": (n, d), "interlace", "aspect", "chroma",
    "range" (None when the file does not say), "layout", "depth", "frame_bytes"}; frames = uint8 numpy ``[T, frame_bytes]``, a fresh
    array (every frame starts at an even address)."""
    data = open(path, "rb").read()
    end = data.index(b"\n")
    fields = data[:end].decode("ascii").split(" ")
    if fields[0] != "YUV4MPEG2":
        raise ValueError(f"{path}: not a YUV4MPEG2 file")
    hdr = {"W": None, "H": None, "fps": None, "interlace": None, "aspect": None, "chroma": "420jpeg", "range": None}
    for f in fields[1:]:
        if not f:
            continue
        tag, val = f[0], f[1:]
        if tag == "W":
            hdr["W"] = int(val)
        elif tag == "H":
            hdr["H"] = int(val)
        elif tag == "F":
            hdr["fps"] = tuple(int(x) for x in val.split(":"))
        elif tag == "I":
            hdr["interlace"] = val
        elif tag == "A":
            hdr["aspect"] = val
        elif tag == "C":
            hdr["chroma"] = val
        elif f.startswith("XCOLORRANGE="):
            hdr["range"] = f.split("=", 1)[1].lower()
    deep = {f"{c}p{d}": ("yuv" + c + "p", d) for c in ("420", "444") for d in (10, 12, 16)}
    if hdr["chroma"] in ("420jpeg", "420", "420mpeg2", "420paldv"):
        hdr["layout"], hdr["depth"] = "yuv420p", 8
    elif hdr["chroma"] == "444":
        hdr["layout"], hdr["depth"] = "yuv444p", 8
    elif hdr["chroma"] in deep:
        hdr["layout"], hdr["depth"] = deep[hdr["chroma"]]
    else:
        raise ValueError(f"{path}: chroma format C{hdr['chroma']} is not 4:2:0 / 4:4:4 of 8, 10, 12 or 16 bits")
    nbytes = frame_bytes(hdr["H"], hdr["W"], FrameFormat(hdr["layout"], depth=hdr["depth"]))
    hdr["frame_bytes"] = nbytes
    out, pos = [], end + 1
    while pos < len(data):
        nl = data.index(b"\n", pos)
        if not data[pos:nl].startswith(b"FRAME"):
            raise ValueError(f"{path}: expected FRAME at byte {pos}")
        if nl + 1 + nbytes > len(data):
            raise ValueError(f"{path}: truncated frame at byte {pos}")
        out.append(np.frombuffer(data, np.uint8, nbytes, nl + 1))
        pos = nl + 1 + nbytes
    return hdr, (np.stack(out) if out else np.zeros((0, nbytes), np.uint8))


class PNGWriter(_Sink):
    """One PNG per frame under ``directory``, named as the reference names them (``d{idx:05d}.png``, utils/report_utils.py:445).
    ``rgb24`` frames only: ``[H, W, 3]`` arrays, or flat frames when ``W`` and ``H`` are given.  ``bytes`` counts the files' sizes."""

    def __init__(self, directory, W: int | None = None, H: int | None = None, start: int = 0):
        super().__init__()
        self.directory, self.W, self.H, self.index = str(directory), W, H, int(start)
        os.makedirs(self.directory, exist_ok=True)

    def write(self, frame_u8):
        from PIL import Image
        a = frame_u8 if isinstance(frame_u8, np.ndarray) else _as_bytes_array(frame_u8).reshape(tuple(frame_u8.shape))
        if a.ndim != 3:
            if self.W is None or self.H is None:
                raise ValueError("PNGWriter: a flat frame needs PNGWriter(directory, W, H)")
            a = planes(_as_bytes_array(a), self.H, self.W, FrameFormat("rgb24"))[0]
        if a.dtype != np.uint8 or a.shape[2] != 3:
            raise ValueError(f"PNGWriter takes rgb24 frames [H, W, 3] (got {a.dtype} {a.shape})")
        path = os.path.join(self.directory, f"d{self.index:05d}.png")
        Image.fromarray(np.ascontiguousarray(a), "RGB").save(path)
        self.index += 1
        self.frames += 1
        self.bytes += os.path.getsize(path)


def write_frames(frames_u8, sink, queue_frames: int = 16) -> dict:
    """Feed an iterable of uint8 frames to ``sink`` from ONE background thread behind a bounded queue (``queue_frames`` copied
    frames: a slow sink — the PNG encoder — holds the producer back instead of growing memory) and close the sink.  An exception
    of the sink is raised here, in the caller.  Returns {"frames", "bytes", "seconds", "fps"}: the clock runs until the sink is
    closed."""
    q: queue.Queue = queue.Queue(maxsize=max(int(queue_frames), 1))
    failed = []

    def work():
        while True:
            item = q.get()
            if item is None:
                return
            if failed:
                continue              # keep draining, so that the producer never blocks on a full queue
            try:
                sink.write(item)
            except BaseException as e:  # noqa: BLE001
                failed.append(e)

    t0 = time.perf_counter()
    th = threading.Thread(target=work, name="gsvc-frame-writer", daemon=True)
    th.start()
    count = 0
    try:
        for fr in frames_u8:
            if failed:
                break
            q.put(_as_bytes_array(fr).copy() if not (isinstance(fr, np.ndarray) and fr.ndim == 3) else fr.copy())
            count += 1
    finally:
        q.put(None)
        th.join()
        try:
            sink.close()
        except BaseException as e:  # noqa: BLE001
            failed.append(e)
    if failed:
        raise failed[0]
    seconds = time.perf_counter() - t0
    return {"frames": count, "bytes": int(getattr(sink, "bytes", 0)), "seconds": seconds,
            "fps": count / seconds if seconds > 0 else float("inf")}


def write_video(frames, pc, pipe, bg_color, sink, fmt: FrameFormat = FrameFormat(), batch: int = 8, scaling_modifier=1.0, mode=None,
                queue_frames: int = 16) -> dict:
    """Render ``frames`` with ``render_frames_u8(..., to_host=True)`` into ``sink`` (``write_frames``)."""
    return write_frames(render_frames_u8(frames, pc, pipe, bg_color, fmt=fmt, batch=batch, to_host=True,
                                         scaling_modifier=scaling_modifier, mode=mode), sink, queue_frames=queue_frames)


def open_sink(path, W: int, H: int, fps=(30, 1), fmt: FrameFormat | None = None):
    """``(sink, format)`` for a path: ``.y4m`` -> Y4MWriter, ``.yuv`` / ``.rgb`` -> RawWriter, anything else -> a directory of PNGs.
    ``fmt`` None: yuv420p for ``.y4m`` / ``.yuv``, rgb24 for ``.rgb`` and PNGs.  A deep ``fmt`` (``depth`` 10 / 12 / 16) is carried as it
    is: the Y4M header says ``C420p10``, a raw file holds two bytes per sample."""
    ext = os.path.splitext(str(path))[1].lower()
    if ext == ".y4m":
        fmt = fmt or FrameFormat("yuv420p")
        return Y4MWriter(path, W, H, fps, fmt), fmt
    if ext in (".yuv", ".rgb"):
        fmt = fmt or FrameFormat("yuv420p" if ext == ".yuv" else "rgb24")
        return RawWriter(path), fmt
    fmt = fmt or FrameFormat("rgb24")
    if fmt.layout != "rgb24":
        raise ValueError("a directory of PNGs takes rgb24 frames")
    return PNGWriter(path, W, H), fmt
