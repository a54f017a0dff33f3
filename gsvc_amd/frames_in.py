"""Encoder input: 8-bit RGB / YUV and 10 / 12 / 16-bit planar YUV video files to float frames on the GPU (host side of
csrc/frames_in.hip), the mirror image of ``frames_out``.

A fit reads float32 ``[3, H, W]`` pictures; a video file holds 8 bits per sample.  ``io.FrameCubeDataset`` opens one PNG per frame
with PIL and divides by 255 on the host; here ``open_video`` hands out the bytes of a ``.y4m`` / ``.yuv`` / ``.rgb`` file,
``frames_from_u8`` converts up to 16 uploaded frames with one HIP launch, and ``VideoFileCube`` is the dataset a ``Trainer`` or
``report.evaluate`` takes: the file's frames either converted once and kept as float (``resident="float"``) or kept in device memory
as they are in the file and converted one frame per fetch (``resident="u8"``: 3.1 MB instead of 24.9 MB per 1080p 4:2:0 frame).

The conversion (include/gsvc_hip.h, gsvc_frames_from_u8): ``rgb24`` is ``b / 255`` (bit-equal to ``io.load_image``); the YUV layouts
invert the BT.709 / BT.601 matrix of ``frames_out`` for limited or full range codes and clamp to [0, 1]; 4:2:0 chroma is centre
sited (Y4M ``C420jpeg``, what ``Y4MWriter`` writes) and upsampled on the codes, ``chroma="bilinear"`` (the default; weights 9/16,
3/16, 3/16, 1/16) or ``"nearest"``.  Deep frames (``fmt.depth`` 10 / 12 / 16: little-endian 16-bit samples in the same flat ``uint8``
buffers, twice the bytes; gsvc_frames_from_u16) go through the same formulas with the constants of their depth.

Importing this module needs neither a GPU nor the built library; ``frames_from_u8`` and ``VideoFileCube`` do (no CPU fallback).
"""
from __future__ import annotations

import os
import weakref

import numpy as np

from . import _lib
from .frames_out import LAYOUTS, MATRICES, MAX_BATCH, RANGES, FrameFormat, frame_bytes, read_y4m

CHROMAS = {"nearest": 0, "bilinear": 1}                      # the GSVC_FRAMES_CHROMA_* enums of include/gsvc_hip.h


def _chroma_id(chroma: str) -> int:
    if chroma not in CHROMAS:
        raise ValueError(f"unknown chroma mode {chroma!r} (one of {', '.join(CHROMAS)})")
    return CHROMAS[chroma]


# ----------------------------------------------------------------------------------------------------------------------------
# device side
# ----------------------------------------------------------------------------------------------------------------------------
def frames_from_u8(frames_u8, H: int, W: int, fmt: FrameFormat = FrameFormat(), chroma: str = "bilinear", out=None):
    """uint8 CUDA frames ``[n, >= frame_bytes]`` with contiguous rows (or one flat frame) -> float32 ``[n, 3, H, W]`` RGB on their
    device, one launch per 16 frames on the current stream; nothing synchronises.  The ``_u8`` of the name means "a buffer of bytes":
    a deep format (``fmt.depth`` above 8) reads little-endian 16-bit samples from it; the frames must then start at even addresses
    (an even base and row stride).  Bytes of a row past the frame are not read;
    ``fmt.rounding`` is ignored.  ``out``: a float32 CUDA tensor ``[n, 3, H, W]`` whose images are contiguous (it is returned)."""
    import ctypes as C

    import torch
    cid = _chroma_id(chroma)
    if not isinstance(frames_u8, torch.Tensor):
        raise ValueError(f"frames_from_u8: frames must be a uint8 tensor (got {type(frames_u8).__name__})")
    if not frames_u8.is_cuda:
        raise _lib.GsvcError("frames_from_u8 runs on the HIP kernels of csrc/frames_in.hip; CPU tensors are not supported")
    H, W = int(H), int(W)
    nbytes = frame_bytes(H, W, fmt)
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() not in (1, 2):
        raise ValueError(f"frames_from_u8: frames must be uint8 [n, >= {nbytes}] or one flat frame (got {frames_u8.dtype} "
                         f"{tuple(frames_u8.shape)})")
    if frames_u8.dim() == 1:
        frames_u8 = frames_u8.unsqueeze(0)
    n = int(frames_u8.shape[0])
    if n < 1 or frames_u8.shape[1] < nbytes or frames_u8.stride(1) != 1 or (n > 1 and frames_u8.stride(0) < nbytes):
        raise ValueError(f"frames_from_u8: a {fmt.name} frame of {H} x {W} has {nbytes} bytes; frames must be [n >= 1, >= {nbytes}] "
                         f"with contiguous rows (got {tuple(frames_u8.shape)}, strides {tuple(frames_u8.stride())})")
    dev = frames_u8.device
    if out is None:
        out = torch.empty((n, 3, H, W), dtype=torch.float32, device=dev)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != dev or tuple(out.shape) != (n, 3, H, W)
          or not out[0].is_contiguous()):
        raise ValueError(f"frames_from_u8: out must be float32 [{n}, 3, {H}, {W}] on {dev} with contiguous images")
    L = _lib.lib()
    stride = int(frames_u8.stride(0)) if n > 1 else max(int(frames_u8.stride(0)), nbytes)
    if fmt.depth > 8 and n == 1:
        stride += stride & 1          # (one frame: the stride addresses nothing)
    base, obase, ostride = frames_u8.data_ptr(), out.data_ptr(), int(out.stride(0)) * 4
    with torch.cuda.device(dev):
        stream = _lib.current_stream(dev)
        for i in range(0, n, MAX_BATCH):
            m = min(MAX_BATCH, n - i)
            ptrs = (C.c_void_p * m)(*[obase + (i + k) * ostride for k in range(m)])
            if fmt.depth > 8:
                _lib.check(L.gsvc_frames_from_u16(base + i * stride, stride, m, H, W, LAYOUTS[fmt.layout], MATRICES[fmt.matrix],
                                                  RANGES[fmt.range], cid, fmt.depth, ptrs, stream), "gsvc_frames_from_u16")
                continue
            _lib.check(L.gsvc_frames_from_u8(base + i * stride, stride, m, H, W, LAYOUTS[fmt.layout], MATRICES[fmt.matrix],
                                             RANGES[fmt.range], cid, ptrs, stream), "gsvc_frames_from_u8")
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# files
# ----------------------------------------------------------------------------------------------------------------------------
def open_video(path, W: int | None = None, H: int | None = None, fmt: FrameFormat | None = None):
    """``(header, frames)`` of a video file of 8-bit or deep (10 / 12 / 16-bit, two bytes per sample) frames; frames = uint8 array
    ``[T, frame_bytes]``, header = {"W", "H", "frames", "frame_bytes", "depth", "fmt": the FrameFormat of the payload, ...}.  The depth
    of a ``.y4m`` file comes from the file (``C420p10``, ...), that of a raw file from ``fmt``.

    ``.y4m``: read with ``frames_out.read_y4m`` (its header's fields are kept); the file's size, layout, depth and ``XCOLORRANGE`` win over
    ``W``, ``H`` and ``fmt``, which supplies the matrix (Y4M has no field for it) and the range of a file that does not state one.
    ``.yuv`` / ``.rgb``: frame payloads back to back (``RawWriter``), memory-mapped; ``W`` and ``H`` are required and a file whose
    size is not a whole number of frames is refused.  ``fmt`` None: what ``open_sink`` uses for the extension — yuv420p (BT.709,
    limited range) for ``.y4m`` / ``.yuv``, rgb24 for ``.rgb``."""
    path = str(path)
    ext = os.path.splitext(path)[1].lower()
    if ext == ".y4m":
        hdr, frames = read_y4m(path)
        base = fmt or FrameFormat("yuv420p")
        if hdr["range"] not in (None, "limited", "full"):
            raise ValueError(f"{path}: unknown XCOLORRANGE={hdr['range']}")
        used = FrameFormat(hdr["layout"], base.matrix, hdr["range"] or base.range, base.rounding, hdr["depth"])
        hdr = dict(hdr, frames=int(frames.shape[0]), fmt=used)
        return hdr, frames
    if ext in (".yuv", ".rgb"):
        if W is None or H is None:
            raise ValueError(f"{path}: a raw {ext} file does not say its size: open_video(path, W, H)")
        used = fmt or FrameFormat("yuv420p" if ext == ".yuv" else "rgb24")
        nbytes = frame_bytes(H, W, used)
        size = os.path.getsize(path)
        if size == 0 or size % nbytes:
            raise ValueError(f"{path}: {size} bytes are not a whole number of {used.name} frames of {int(W)} x {int(H)} "
                             f"({nbytes} bytes each)")
        frames = np.memmap(path, dtype=np.uint8, mode="r", shape=(size // nbytes, nbytes))
        return {"W": int(W), "H": int(H), "layout": used.layout, "range": used.range, "depth": used.depth, "frame_bytes": nbytes,
                "frames": size // nbytes, "fmt": used}, frames
    raise ValueError(f"{path}: open_video reads .y4m, .yuv and .rgb files")


class VideoFileCube:
    """The frames of a video file as the dataset of a fit, addressed like ``io.FrameCubeDataset`` and ``frame.SyntheticFrameCube``
    (``dataset[i]`` is frame i with its picture kept transposed ``[3, W, H]`` and its camera at ``z = (i - T/2) / scale``;
    ``get_optical_flow(i)`` the flow between frames i and i + 1, from ``optical_flow_dir`` through ``io.load_flow``).

    The frames (8-bit, or deep: ``resident="u8"`` then means "as the file's bytes", 6.2 MB per 1080p 4:2:0 frame) are uploaded in chunks of up to 16 through one pinned staging buffer and converted on the device
    (``frames_from_u8``); no float arithmetic on pixels runs on the host.
      ``resident="float"``  every frame is converted once and kept as float32: fetching a frame launches nothing.
      ``resident="u8"``     the video stays in device memory as it is in the file; ``get_z_frame`` converts the one frame it hands
                            out with one launch on the current stream, into a tensor of its own that nothing writes again.  A reader on
                            ANOTHER stream calls ``ready(i)`` first (``Trainer`` does, for its two frames, before the image losses):
                            the current stream then waits for the conversions of frame i that are still held by a ``Frame``, and
                            their tensors are recorded on it, so that the allocator does not hand their memory out under the reader.
                            Two limits: a conversion is remembered through the tensor its ``Frame`` carries — a reader that keeps
                            only another view of the picture must order itself —, and every fetch converts and allocates 12 H W
                            bytes, also one whose picture is never read (a batched ``Trainer`` step fetches its pair twice: four
                            conversions per step where two are read).

    ``frame_range=(first, stop)``: the cube of the file's frames ``first .. stop - 1`` alone (one group of pictures of a long clip,
    gsvc_amd/scene.py): only those frames are uploaded, frame i of the cube is file frame ``first + i``, and ``len``, ``scale``,
    ``x_min``, ``y_min`` and ``z_min`` are those of a clip of ``stop - first`` frames; the flow files used are those of the pairs
    inside the range.  None: all frames.

    ``frames``: a uint8 array ``[len, frame_bytes]`` that stands in for the payload of the file's frames (those of ``frame_range``): a
    prefiltered source (gsvc_amd/tfilter.py).  The file still supplies size, format and count.  None: the file's own.

    ``frame_size=(W, H)`` (with ``frames`` only): the payload has this size instead of the file's — a resampled source
    (gsvc_amd/resample.py) — and the cube's ``width``, ``height``, ``scale``, ``x_min`` and ``y_min`` are those of ``frame_size``; the
    file still supplies format and count.  ``yuv_planes`` and ``luma_detail`` then read the payload given, which is kept on the host (the
    file's own frames have another size).  None: the payload has the file's size."""

    def __init__(self, path, optical_flow_dir=None, W: int | None = None, H: int | None = None, fmt: FrameFormat | None = None,
                 chroma: str = "bilinear", device="cuda", resident: str = "float", frame_range=None, frames=None, frame_size=None):
        import pathlib

        import torch
        if resident not in ("float", "u8"):
            raise ValueError(f"VideoFileCube: resident must be 'float' or 'u8' (got {resident!r})")
        _chroma_id(chroma)
        self.path, self.chroma, self.resident = str(path), chroma, resident
        given = frames
        self.header, frames = open_video(path, W, H, fmt)
        self.fmt = self.header["fmt"]
        self.height, self.width, self.len = int(self.header["H"]), int(self.header["W"]), int(frames.shape[0])
        if self.len < 1:
            raise ValueError(f"{self.path}: no frames")
        self.frame_range = None
        if frame_range is not None:
            try:
                first, stop = (int(v) for v in frame_range)
            except (TypeError, ValueError):
                raise ValueError(f"VideoFileCube: frame_range must be (first, stop) (got {frame_range!r})") from None
            if not 0 <= first < stop <= self.len:
                raise ValueError(f"VideoFileCube: frame_range ({first}, {stop}) is not a non-empty range inside the {self.len} frames of "
                                 f"{self.path}")
            self.frame_range = (first, stop)
            frames, self.len = frames[first:stop], stop - first
        self.frame_bytes = int(self.header["frame_bytes"])          # of the payload: the file's, or that of ``frame_size``
        self._payload = None
        if frame_size is not None:
            if given is None:
                raise ValueError("VideoFileCube: frame_size describes a payload given with frames=")
            try:
                self.width, self.height = (int(v) for v in frame_size)
            except (TypeError, ValueError):
                raise ValueError(f"VideoFileCube: frame_size must be (W, H) (got {frame_size!r})") from None
            self.frame_bytes = frame_bytes(self.height, self.width, self.fmt)
        if given is not None:
            given = np.asarray(given)
            if given.dtype != np.uint8 or given.shape != (self.len, self.frame_bytes):
                raise ValueError(f"VideoFileCube: frames must be uint8 [{self.len}, {self.frame_bytes}] (got {given.dtype} "
                                 f"{given.shape})")
            frames = given
            if frame_size is not None:
                self._payload = given
        self.scale = max(self.height, self.width, self.len) / 2
        self.x_min = -self.width / 2 / self.scale
        self.y_min = -self.height / 2 / self.scale
        self.z_min = -self.len / 2 / self.scale
        self.optical_flow_paths = sorted(pathlib.Path(optical_flow_dir).iterdir()) if optical_flow_dir is not None else []
        if self.frame_range is not None:
            self.optical_flow_paths = self.optical_flow_paths[self.frame_range[0]:self.frame_range[1] - 1]
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.GsvcError("VideoFileCube converts its frames with the HIP kernels of csrc/frames_in.hip; it needs a CUDA device")
        self._views, self._fetched = {}, {}
        self._planes = None          # resident="float": the plane buffers of every frame, from the first yuv_planes() on
        self._upload(frames)
        from .io import load_flow
        self.prefetched_of = [load_flow(p).to(self.device) for p in self.optical_flow_paths]

    def _upload(self, frames):
        import torch
        T, H, W, nbytes = self.len, self.height, self.width, self.frame_bytes
        chunk = min(MAX_BATCH, T)
        staging = torch.empty((chunk, nbytes), dtype=torch.uint8, pin_memory=True)
        host = staging.numpy()
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            if self.resident == "u8":
                self._u8, self._images = torch.empty((T, nbytes), dtype=torch.uint8, device=self.device), None
                on_dev = None
            else:
                self._u8, self._images = None, torch.empty((T, 3, H, W), dtype=torch.float32, device=self.device)
                on_dev = torch.empty((chunk, nbytes), dtype=torch.uint8, device=self.device)
            for i in range(0, T, chunk):
                m = min(chunk, T - i)
                np.copyto(host[:m], frames[i:i + m])
                dst = self._u8[i:i + m] if on_dev is None else on_dev[:m]
                dst.copy_(staging[:m], non_blocking=True)
                if on_dev is not None:
                    frames_from_u8(dst, H, W, self.fmt, self.chroma, out=self._images[i:i + m])
                stream.synchronize()          # the staging buffer is free again; after the last chunk: every stream may read the video

    def __len__(self):
        return self.len

    @property
    def len_z_frames(self):
        return self.len

    @property
    def frame_num(self):
        return self.len

    @property
    def frame_height(self):
        return self.height

    @property
    def frame_width(self):
        return self.width

    def _picture(self, image_id):
        if self._images is not None:
            return self._images[image_id].permute(0, 2, 1)
        import torch
        img = frames_from_u8(self._u8[image_id:image_id + 1], self.height, self.width, self.fmt, self.chroma)[0].permute(0, 2, 1)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(self.device))
        live = [(r, ev) for r, ev in self._fetched.get(image_id, ()) if r() is not None]
        self._fetched[image_id] = live + [(weakref.ref(img), done)]
        return img

    def yuv_planes(self, image_id):
        """The float32 plane buffer ``[Y: H W | Cb | Cr]`` of frame ``image_id`` straight from the file's sample codes, in the file's
        own layout (``yuv_loss.frame_planes``: no matrix, no chroma upsampling; ``yuv_loss.split_planes`` views it as Y and C) — the
        ground truth of a fit with ``loss_domain = "yuv420"`` / ``"yuv444"``.  A Y'CbCr file only.
          ``resident="u8"``     one launch per call on the current stream, reading the resident bytes (complete before the
                                constructor returned: nothing to order across streams), into a tensor of its own.
          ``resident="float"``  all frames are converted on first use, in chunks of 16 on the current stream, and kept: 4 bytes per
                                sample, 6 H W bytes per 4:2:0 frame.  Readers on other streams order themselves behind that first call."""
        from .yuv_loss import frame_planes
        if self.fmt.layout not in ("yuv420p", "yuv444p"):
            raise ValueError(f"{self.path}: {self.fmt.layout} frames hold no Y'CbCr planes")
        image_id = int(image_id)
        if not 0 <= image_id < self.len:
            raise IndexError(f"frame {image_id} of {self.len}")
        if self._u8 is not None:
            return frame_planes(self._u8[image_id:image_id + 1], self.height, self.width, self.fmt)[0]
        if self._planes is None:
            self._planes = self._convert_planes()
        return self._planes[image_id]

    def _host_frames(self):
        """The host bytes of the cube's frames for a second upload: the file's frames of ``frame_range``, or the payload of
        ``frame_size``."""
        if self._payload is not None:
            return self._payload
        _, frames = open_video(self.path, self.width, self.height, self.fmt)
        if self.frame_range is not None:
            frames = frames[self.frame_range[0]:self.frame_range[1]]
        return frames

    def _convert_planes(self):
        """Every frame's plane buffer, for ``resident="float"``: the file's bytes are uploaded again in chunks of up to 16 frames
        through one pinned staging buffer (the float pictures cannot give the un-interpolated chroma back)."""
        import torch

        from .yuv_loss import frame_planes
        frames = self._host_frames()
        T, nbytes = self.len, self.frame_bytes
        chunk = min(MAX_BATCH, T)
        staging = torch.empty((chunk, nbytes), dtype=torch.uint8, pin_memory=True)
        host = staging.numpy()
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            on_dev = torch.empty((chunk, nbytes), dtype=torch.uint8, device=self.device)
            planes = torch.empty((T, nbytes // (2 if self.fmt.depth > 8 else 1)), dtype=torch.float32, device=self.device)
            for i in range(0, T, chunk):
                m = min(chunk, T - i)
                np.copyto(host[:m], frames[i:i + m])
                on_dev[:m].copy_(staging[:m], non_blocking=True)
                frame_planes(on_dev[:m], self.height, self.width, self.fmt, out=planes[i:i + m])
                stream.synchronize()          # the staging buffer is free again
        return planes

    def luma_detail(self, cell: int = 8):
        """The detail map of the cube's frames from the file's luma codes (gsvc_amd/detail.py) -> uint32 ``[T, Hc, Wc]``: what a fit
        with ``init="detail"`` draws its anchors from.  A Y'CbCr file only.  The same bits in either residency:
          ``resident="u8"``     one launch on the resident bytes.
          ``resident="float"``  the file's bytes are uploaded again in chunks of 16 frames plus one overlapping frame, as
                                ``_convert_planes`` does (the float pictures cannot give the codes back).
        A ``frame_range`` cube reads its own frames only: its last frame looks back, never past the range."""
        from . import detail
        if self.fmt.layout not in ("yuv420p", "yuv444p"):
            raise ValueError(f"{self.path}: {self.fmt.layout} frames hold no luma plane")
        if self._u8 is not None:
            return detail.luma_detail(self._u8, self.height, self.width, self.fmt, cell)
        frames = self._host_frames()
        return detail.file_detail(frames, self.height, self.width, self.fmt, cell, self.device)

    def ready(self, image_id):
        """Order the current stream behind the conversions of frame ``image_id`` whose pictures are still in use, and tell the
        allocator that this stream reads them.  Nothing to do for ``resident="float"``: those pictures were complete before the
        constructor returned."""
        if self._images is not None:
            return
        import torch
        cur = torch.cuda.current_stream(self.device)
        live = []
        for r, ev in self._fetched.get(image_id, ()):
            img = r()
            if img is not None:
                cur.wait_event(ev)
                img.record_stream(cur)
                live.append((r, ev))
        self._fetched[image_id] = live

    def get_z_frame(self, image_id, load_image=True):
        from .frame import Frame, make_view_matrix
        image_id = int(image_id)
        if not 0 <= image_id < self.len:
            raise IndexError(f"frame {image_id} of {self.len}")
        z = (image_id - self.len / 2) / self.scale
        if image_id not in self._views:
            self._views[image_id] = make_view_matrix(z=z, plane="xy")
        vm, vms, cam = self._views[image_id]
        img = self._picture(image_id) if load_image else None
        return Frame(image_id=image_id, plane="xy", image=img, x_min=self.x_min, y_min=self.y_min, z=z, image_width=self.width,
                     image_height=self.height, view_matrix=vm, view_matrix_s=vms, scale=self.scale, cam_pos=cam)

    def get_dummy_frame(self, image_id):
        return self.get_z_frame(image_id, load_image=False)

    def __getitem__(self, idx):
        return self.get_z_frame(idx)

    def get_optical_flow(self, idx):
        if not self.prefetched_of:
            raise RuntimeError(f"{self.path}: a video file holds no optical flow: the fit needs optical_lambda = 0, or flow files "
                               "(VideoFileCube(path, optical_flow_dir=...))")
        return self.prefetched_of[idx]
