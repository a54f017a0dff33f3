"""The bitstream file: ONE ``.gsvc`` file from which another process rebuilds the model and renders the video with nothing else
(DESIGN.md section 8g).  Little-endian, written with ``struct``:

    b"GSVC" | uint16 version (1) | uint16 sections | sections x (4-byte tag, uint64 length, uint32 CRC-32 of the payload) | payloads

The payloads follow the table in its order.  A reader skips tags it does not know, so a later version can add sections; a newer
VERSION is refused.  Sections of version 1:

    HEAD   everything a decoder must know before it can allocate, as typed fields (``pack_fields``): the picture (W, H, frames, frame
           rate), the cube geometry and render settings, the model's shape, the anchor quantiser's bounds and the scalars of StreamPack.
           Floats are float32 bit patterns — every one of them is a float32 where it is used (the kernels take them by value as floats,
           the bounds and the anchor grid are float32 tensors) — never text.
    MLPS   the bytes of ``mlp_codec.encode_mlp`` (8-bit weights, Huffman-coded)
    ANCH   StreamPack.anchor_stream (occupancy octree + rANS)
    MASK   StreamPack.masks          HASH   StreamPack.hash
    SLAB   per z-slab the feature, scaling and offsets streams, each behind a uint64 length
    PHSH   optional: the name of the FrameFormat the hashes were taken in (+ matrix, range, rounding) and uint64 [frames, 3] picture
           hashes (``metrics.picture_hash``: include/gsvc_hip.h, gsvc_picture_hash)
    GRAN   optional: the film-grain parameters (``grain.GrainParams.pack``, 122 bytes) a decoder synthesises grain from on the delivered
           frames, AFTER their picture hashes are taken: PHSH stays the hash of the ungrained picture.  A
           decoder that does not know the tag skips it and delivers the ungrained pictures.
    DISP   optional: typed fields display_W, display_H and filter (1: the Lanczos-3 of gsvc_amd/resample.py).  HEAD's W x H is the
           CODED size, the size the model renders at; a file with DISP was fitted to a resampled source and its decoder resamples
           every decoded picture to display_W x display_H, AFTER its picture hash is taken: PHSH stays the hash of the coded-size
           picture, which does not depend on the resampler's tables.  An unknown filter id is refused.  A
           decoder that does not know the tag skips it and delivers the coded size.

A clip of several groups of pictures is a sequence file of such file images: gsvc_amd/sequence.py.

``write_bitstream`` / ``read_bitstream`` need neither a GPU nor the built library; ``Bitstream.build_model`` and ``decode_video`` do.
Nothing here reads the source video or the trainer.
"""
from __future__ import annotations

import struct
import zlib
from dataclasses import dataclass, field

import numpy as np

MAGIC = b"GSVC"
VERSION = 1
_PREFIX = struct.Struct("<4sHH")           # magic, version, number of sections
_ENTRY = struct.Struct("<4sQI")            # tag, payload length, CRC-32 of the payload
KNOWN_TAGS = (b"HEAD", b"MLPS", b"ANCH", b"MASK", b"HASH", b"SLAB", b"PHSH", b"DISP", b"GRAN")          # (a set: sections are found by tag, in any file order)
REQUIRED_TAGS = KNOWN_TAGS[:6]


class BitstreamError(ValueError):
    """A file that is not a bitstream of this library, or a damaged one; ``section`` names where (a tag, ``"magic"``, ``"version"`` or
    ``"table"``)."""

    def __init__(self, section: str, message: str):
        super().__init__(f"bitstream section {section}: {message}")
        self.section = section


# ----------------------------------------------------------------------------------------------------------------------------
# framing
# ----------------------------------------------------------------------------------------------------------------------------
def pack_sections(sections) -> bytes:
    """[(tag, payload)] -> the bytes of a file."""
    sections = [(t.encode("ascii") if isinstance(t, str) else bytes(t), bytes(p)) for t, p in sections]
    for tag, _ in sections:
        if len(tag) != 4:
            raise ValueError(f"a section tag has 4 characters (got {tag!r})")
    out = [_PREFIX.pack(MAGIC, VERSION, len(sections))]
    out += [_ENTRY.pack(tag, len(p), zlib.crc32(p) & 0xFFFFFFFF) for tag, p in sections]
    out += [p for _, p in sections]
    return b"".join(out)


def unpack_sections(blob: bytes, known=None) -> list:
    """The bytes of a file -> [(tag, payload)] in file order, every CRC checked (unknown sections too: a damaged file is damaged).
    ``known``: keep only these tags."""
    blob = bytes(blob)
    if len(blob) < len(MAGIC) or blob[:4] != MAGIC:
        raise BitstreamError("magic", "not a GSVC bitstream file" if len(blob) >= 4 else "truncated inside the magic")
    if len(blob) < _PREFIX.size:
        raise BitstreamError("version", "truncated inside the file prefix")
    _, version, count = _PREFIX.unpack_from(blob, 0)
    if version > VERSION or version < 1:
        raise BitstreamError("version", f"version {version} is not readable by this decoder (it reads up to {VERSION})")
    at = _PREFIX.size
    if len(blob) < at + count * _ENTRY.size:
        raise BitstreamError("table", f"truncated inside the section table ({count} sections)")
    table = [_ENTRY.unpack_from(blob, at + i * _ENTRY.size) for i in range(count)]
    at += count * _ENTRY.size
    out = []
    for tag, length, crc in table:
        name = tag.decode("ascii", "replace")
        if at + length > len(blob):
            raise BitstreamError(name, f"truncated: {length} bytes declared, {max(len(blob) - at, 0)} present")
        payload = blob[at:at + length]
        if zlib.crc32(payload) & 0xFFFFFFFF != crc:
            raise BitstreamError(name, "CRC mismatch")
        at += length
        if known is None or tag in known:
            out.append((tag, payload))
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# typed fields (HEAD, and the text part of PHSH)
# ----------------------------------------------------------------------------------------------------------------------------
def _f32(v) -> bytes:
    return np.float32(v).tobytes()


def pack_fields(fields: dict) -> bytes:
    """{name: value} -> bytes.  bool, int (int64), float (its float32 bit pattern), str (UTF-8), a list / tuple / array of ints
    (int64 each) or of floats (float32 each; an empty list is a list of ints)."""
    out = [struct.pack("<H", len(fields))]
    for name, v in fields.items():
        key = name.encode("ascii")
        out.append(struct.pack("<B", len(key)) + key)
        if isinstance(v, (bool, np.bool_)):
            out.append(b"b" + struct.pack("<B", int(v)))
        elif isinstance(v, (int, np.integer)):
            out.append(b"i" + struct.pack("<q", int(v)))
        elif isinstance(v, (float, np.floating)):
            out.append(b"f" + _f32(v))
        elif isinstance(v, str):
            text = v.encode("utf-8")
            out.append(b"s" + struct.pack("<I", len(text)) + text)
        elif isinstance(v, (list, tuple, np.ndarray)):
            a = np.asarray(v).reshape(-1)
            if a.size and a.dtype.kind == "f":
                out.append(b"F" + struct.pack("<I", a.size) + a.astype("<f4").tobytes())
            elif a.size == 0 or a.dtype.kind in "iub":
                out.append(b"I" + struct.pack("<I", a.size) + a.astype("<i8").tobytes())
            else:
                raise TypeError(f"pack_fields: {name}: a list holds ints or floats (got {a.dtype})")
        else:
            raise TypeError(f"pack_fields: {name}: unsupported type {type(v).__name__}")
    return b"".join(out)


def unpack_fields(payload: bytes, section: str = "HEAD") -> dict:
    """The inverse of ``pack_fields``: floats come back as ``numpy.float32`` (the stored bits), lists as tuples."""
    buf, at = bytes(payload), 0

    def take(n):
        nonlocal at
        if at + n > len(buf):
            raise BitstreamError(section, "the fields run past the end of the section")
        at += n
        return buf[at - n:at]

    out = {}
    (count,) = struct.unpack("<H", take(2))
    for _ in range(count):
        name = take(take(1)[0]).decode("ascii")
        kind = take(1)
        if kind == b"b":
            out[name] = bool(take(1)[0])
        elif kind == b"i":
            out[name] = struct.unpack("<q", take(8))[0]
        elif kind == b"f":
            out[name] = np.frombuffer(take(4), "<f4")[0]
        elif kind == b"s":
            out[name] = take(struct.unpack("<I", take(4))[0]).decode("utf-8")
        elif kind == b"F":
            n = struct.unpack("<I", take(4))[0]
            out[name] = tuple(np.frombuffer(take(4 * n), "<f4"))
        elif kind == b"I":
            n = struct.unpack("<I", take(4))[0]
            out[name] = tuple(int(v) for v in np.frombuffer(take(8 * n), "<i8"))
        else:
            raise BitstreamError(section, f"unknown field type {kind!r} of {name}")
    if at != len(buf):
        raise BitstreamError(section, "bytes behind the last field")
    return out


def _pack_slabs(pack) -> bytes:
    out = []
    for s in range(len(pack.slabs)):
        for stream in (pack.feat[s], pack.scaling[s], pack.offsets[s]):
            out.append(struct.pack("<Q", len(stream)) + bytes(stream))
    return b"".join(out)


def _unpack_slabs(payload: bytes, n_slabs: int):
    streams, at = [], 0
    for _ in range(3 * n_slabs):
        if at + 8 > len(payload):
            raise BitstreamError("SLAB", "fewer streams than the header's slabs need")
        (n,) = struct.unpack_from("<Q", payload, at)
        at += 8
        if at + n > len(payload):
            raise BitstreamError("SLAB", "a stream runs past the end of the section")
        streams.append(payload[at:at + n])
        at += n
    if at != len(payload):
        raise BitstreamError("SLAB", "bytes behind the last stream")
    return streams[0::3], streams[1::3], streams[2::3]


def _pack_hashes(fmt, hashes) -> bytes:
    h = np.ascontiguousarray(np.asarray(hashes)).view(np.uint64) if np.asarray(hashes).dtype == np.int64 else np.asarray(hashes, np.uint64)
    if h.ndim != 2 or h.shape[1] != 3:
        raise ValueError(f"picture hashes are [frames, 3] (got {h.shape})")
    text = pack_fields({"format": fmt.name, "matrix": fmt.matrix, "range": fmt.range, "rounding": fmt.rounding_used, "frames": int(h.shape[0])})
    return struct.pack("<I", len(text)) + text + h.astype("<u8").tobytes()


def _unpack_hashes(payload: bytes):
    if len(payload) < 4:
        raise BitstreamError("PHSH", "truncated")
    (n,) = struct.unpack_from("<I", payload, 0)
    if 4 + n > len(payload):
        raise BitstreamError("PHSH", "the format fields run past the end of the section")
    f = unpack_fields(payload[4:4 + n], "PHSH")
    body = payload[4 + n:]
    if len(body) != 24 * f["frames"]:
        raise BitstreamError("PHSH", f"{f['frames']} frames need {24 * f['frames']} bytes of hashes, {len(body)} present")
    return f, np.frombuffer(body, "<u8").reshape(-1, 3).copy()


# ----------------------------------------------------------------------------------------------------------------------------
# the header
# ----------------------------------------------------------------------------------------------------------------------------
@dataclass
class CubeGeometry:
    """What a decoder needs of the frame cube (``VideoFileCube`` / ``SyntheticFrameCube`` derive it from the video's size) and of the
    render configuration."""
    W: int
    H: int
    frames: int
    scale: float
    x_min: float
    y_min: float
    z_min: float
    threshold: float                       # ModelParams.threshold as the fit used it
    background: tuple = (0.0, 0.0, 0.0)
    fps: tuple = (30, 1)
    sh_degree: int = 0
    raster_flags: int = 0
    raster_low_pass: float = 0.0

    @classmethod
    def of(cls, cube, model_params, pipe=None, background=(0.0, 0.0, 0.0), fps=None):
        """``fps`` None: the frame rate a video file's header states (``VideoFileCube.header``), else 30."""
        if fps is None:
            fps = (getattr(cube, "header", None) or {}).get("fps") or (30, 1)
        return cls(W=int(cube.width), H=int(cube.height), frames=int(cube.len_z_frames), scale=float(cube.scale), x_min=float(cube.x_min),
                   y_min=float(cube.y_min), z_min=float(cube.z_min), threshold=float(model_params.threshold),
                   background=tuple(float(v) for v in background), fps=(int(fps[0]), int(fps[1])), sh_degree=int(model_params.sh_degree),
                   raster_flags=int(getattr(pipe, "raster_flags", 0) or 0), raster_low_pass=float(getattr(pipe, "raster_low_pass", 0.0) or 0.0))


def make_header(pc, pack, geometry: CubeGeometry) -> dict:
    """The fields of HEAD from the encoder's model, its StreamPack and the cube's geometry."""
    mc = pc.model_config
    g = geometry
    return {
        # picture
        "W": g.W, "H": g.H, "frames": g.frames, "fps_num": g.fps[0], "fps_den": g.fps[1],
        # cube geometry and render settings
        "scale": g.scale, "x_min": g.x_min, "y_min": g.y_min, "z_min": g.z_min, "threshold": g.threshold, "background": list(g.background),
        "sh_degree": g.sh_degree, "raster_flags": g.raster_flags, "raster_low_pass": g.raster_low_pass,
        # model shape (the arguments of GaussianModel)
        "feat_dim": int(pc.feat_dim), "n_offsets": int(pc.n_offsets), "voxel_size": float(pc.voxel_size),
        "update_depth": int(pc.update_depth), "update_init_factor": int(pc.update_init_factor),
        "update_hierarchy_factor": int(pc.update_hierachy_factor),
        "n_features_per_level": int(pc.n_features_per_level), "log2_hashmap_size": int(pc.log2_hashmap_size),
        "log2_hashmap_size_2D": int(pc.log2_hashmap_size_2D), "resolutions_list": [int(v) for v in pc.resolutions_list],
        "resolutions_list_2D": [int(v) for v in pc.resolutions_list_2D], "use_2D": bool(pc.use_2D), "ste_binary": bool(pc.ste_binary),
        "ste_multistep": bool(pc.ste_multistep), "add_noise": bool(pc.add_noise), "Q": float(pc.Q),
        "time_multi_res": int(mc.time_multi_res), "offset_multi_res": int(mc.offset_multi_res),
        # quantisation of the anchors
        "x_bound_min": pc.x_bound_min.detach().reshape(-1).cpu().numpy().astype(np.float32),
        "x_bound_max": pc.x_bound_max.detach().reshape(-1).cpu().numpy().astype(np.float32),
        # StreamPack
        "n_full": int(pack.n_full), "n": int(pack.n), "prob_masks": float(pack.prob_masks), "prob_hash": float(pack.prob_hash),
        "anchor_interval": np.asarray(pack.anchor_interval, np.float32).reshape(-1), "anchor_min": np.asarray(pack.anchor_min, np.float32).reshape(-1),
        "slabs": [int(v) for s in pack.slabs for v in s],
    }


_HEAD_FIELDS = ("W", "H", "frames", "fps_num", "fps_den", "scale", "x_min", "y_min", "z_min", "threshold", "background", "sh_degree",
                "raster_flags", "raster_low_pass", "feat_dim", "n_offsets", "voxel_size", "update_depth", "update_init_factor",
                "update_hierarchy_factor", "n_features_per_level", "log2_hashmap_size", "log2_hashmap_size_2D", "resolutions_list",
                "resolutions_list_2D", "use_2D", "ste_binary", "ste_multistep", "add_noise", "Q", "time_multi_res", "offset_multi_res",
                "x_bound_min", "x_bound_max", "n_full", "n", "prob_masks", "prob_hash", "anchor_interval", "anchor_min", "slabs")


# ----------------------------------------------------------------------------------------------------------------------------
# the file
# ----------------------------------------------------------------------------------------------------------------------------
def bitstream_bytes(pc, pack, cube_geometry: CubeGeometry, mlp_bytes: bytes, hashes=None, grain=None) -> bytes:
    """The bytes ``write_bitstream`` writes.  ``hashes``: None, or ``(FrameFormat, uint64 / int64 [frames, 3])``; ``grain``: None, or
    the ``grain.GrainParams`` of section GRAN."""
    from . import anchor_codec
    head = make_header(pc, pack, cube_geometry)
    for name in ("prob_masks", "prob_hash"):
        if float(np.float32(head[name])) != head[name]:          # (a ratio of float32 tensors: a decoder with another value could not decode)
            raise ValueError(f"write_bitstream: {name} = {head[name]!r} is not a float32")
    anchor_stream = pack.anchor_stream if pack.anchor_stream else anchor_codec.encode_anchors(pack.anchors_q)
    sections = [(b"HEAD", pack_fields(head)), (b"MLPS", bytes(mlp_bytes)), (b"ANCH", anchor_stream), (b"MASK", pack.masks),
                (b"HASH", pack.hash), (b"SLAB", _pack_slabs(pack))]
    if hashes is not None:
        sections.append((b"PHSH", _pack_hashes(*hashes)))
    if grain is not None:
        sections.append((b"GRAN", grain.pack()))
    return pack_sections(sections)


def write_bitstream(path, pc, pack, cube_geometry: CubeGeometry, mlp_bytes: bytes, hashes=None) -> dict:
    """Write the file; returns {"bytes": the file's size, "sections": {tag: payload bytes}}."""
    blob = bitstream_bytes(pc, pack, cube_geometry, mlp_bytes, hashes)
    with open(path, "wb") as f:
        f.write(blob)
    return {"bytes": len(blob), "sections": {t.decode("ascii"): len(p) for t, p in unpack_sections(blob)}}


def with_hashes(blob: bytes, fmt, hashes) -> bytes:
    """The bytes of a file with its PHSH section set to these picture hashes (``hashes`` None: removed); every other section, known
    or not, is kept as it is."""
    sections = [(t, p) for t, p in unpack_sections(blob) if t != b"PHSH"]
    if hashes is not None:
        sections.append((b"PHSH", _pack_hashes(fmt, hashes)))
    return pack_sections(sections)


def with_grain(blob: bytes, params) -> bytes:
    """The bytes of a file with its GRAN section set to these film-grain parameters (``grain.GrainParams``; None: removed); every other
    section, known or not, is kept as it is."""
    sections = [(t, p) for t, p in unpack_sections(blob) if t != b"GRAN"]
    if params is not None:
        sections.append((b"GRAN", params.pack()))
    return pack_sections(sections)


def pack_display(W: int, H: int, filter_id: int = 1) -> bytes:
    """The payload of a DISP section."""
    return pack_fields({"display_W": int(W), "display_H": int(H), "filter": int(filter_id)})


def unpack_display(payload: bytes) -> tuple:
    """A DISP payload -> ``(W, H)``; a missing field, a size below 2 or an unknown filter id is a ``BitstreamError("DISP", ...)``."""
    from .resample import FILTER_IDS
    f = unpack_fields(payload, "DISP")
    for name in ("display_W", "display_H", "filter"):
        if not isinstance(f.get(name), int) or isinstance(f.get(name), bool):
            raise BitstreamError("DISP", f"field {name} is missing or not an integer")
    if f["filter"] not in FILTER_IDS:
        raise BitstreamError("DISP", f"unknown filter id {f['filter']} (this decoder knows {sorted(FILTER_IDS)})")
    if f["display_W"] < 2 or f["display_H"] < 2:
        raise BitstreamError("DISP", f"the display size {f['display_W']} x {f['display_H']} is not a picture size")
    return f["display_W"], f["display_H"]


def with_display(blob: bytes, size) -> bytes:
    """The bytes of a file with its DISP section set to the display size ``(W, H)`` (None: removed); every other section, known or not,
    is kept as it is."""
    sections = [(t, p) for t, p in unpack_sections(blob) if t != b"DISP"]
    if size is not None:
        sections.append((b"DISP", pack_display(size[0], size[1])))
    return pack_sections(sections)


@dataclass
class Bitstream:
    header: dict
    pack: object                              # StreamPack; ``anchors_q`` is decoded by ``build_model`` (on the device when there is one)
    mlp_bytes: bytes
    hash_format: object = None                # FrameFormat of PHSH, or None
    hashes: object = None                     # uint64 [frames, 3], or None
    grain: object = None                      # grain.GrainParams of GRAN, or None
    display: object = None                    # (W, H) of DISP, or None
    section_bytes: dict = field(default_factory=dict)
    file_bytes: int = 0

    @property
    def geometry(self) -> CubeGeometry:
        h = self.header
        return CubeGeometry(W=h["W"], H=h["H"], frames=h["frames"], scale=float(h["scale"]), x_min=float(h["x_min"]), y_min=float(h["y_min"]),
                            z_min=float(h["z_min"]), threshold=float(h["threshold"]), background=tuple(float(v) for v in h["background"]),
                            fps=(h["fps_num"], h["fps_den"]), sh_degree=h["sh_degree"], raster_flags=h["raster_flags"],
                            raster_low_pass=float(h["raster_low_pass"]))

    @property
    def coded_size(self) -> tuple:
        """``(W, H)`` of HEAD: the size the model renders at."""
        return int(self.header["W"]), int(self.header["H"])

    @property
    def display_size(self) -> tuple:
        """``(W, H)`` a decode delivers by default: DISP's where the file has one, else the coded size."""
        return self.display if self.display is not None else self.coded_size

    def frames(self):
        """The T frames a renderer takes (``Frame`` without a picture), from the header's geometry: what ``get_dummy_frame`` builds."""
        from .frame import Frame, make_view_matrix
        g = self.geometry
        out = []
        for i in range(g.frames):
            z = (i - g.frames / 2) / g.scale
            vm, vms, cam = make_view_matrix(z=z, plane="xy")
            out.append(Frame(image_id=i, plane="xy", image=None, x_min=g.x_min, y_min=g.y_min, z=z, image_width=g.W, image_height=g.H,
                             view_matrix=vm, view_matrix_s=vms, scale=g.scale, cam_pos=cam))
        return out

    def build_model(self, device="cuda"):
        """A fresh ``GaussianModel`` from HEAD alone, its networks from MLPS, everything else through ``conduct_stream_decoding`` ->
        ``(pc, frames, pipe, bg)``, what ``render_frames`` / ``render_frames_u8`` take.  Raises (nothing partial is returned) when a
        stream does not decode."""
        import torch

        from . import anchor_codec, io, mlp_codec
        from .arguments import ModelParams, PipelineParams
        from .model import GaussianModel
        from .stream_codec import conduct_stream_decoding
        h, dev = self.header, torch.device(device)
        mp_ = ModelParams(sh_degree=h["sh_degree"], threshold=float(h["threshold"]), anchor_feature_dim=h["feat_dim"], n_offsets=h["n_offsets"],
                          voxel_size=float(h["voxel_size"]), update_depth=h["update_depth"], update_init_factor=h["update_init_factor"],
                          update_hierarchy_factor=h["update_hierarchy_factor"], time_multi_res=h["time_multi_res"],
                          offset_multi_res=h["offset_multi_res"], log2=h["log2_hashmap_size"], log2_2D=h["log2_hashmap_size_2D"],
                          grid_feature_dim=h["n_features_per_level"], white_background=all(float(v) == 1.0 for v in h["background"]))
        q = float(h["Q"])
        pc = GaussianModel(mp_, h["feat_dim"], h["n_offsets"], float(h["voxel_size"]), h["update_depth"], h["update_init_factor"],
                           h["update_hierarchy_factor"], False, n_features_per_level=h["n_features_per_level"],
                           log2_hashmap_size=h["log2_hashmap_size"], log2_hashmap_size_2D=h["log2_hashmap_size_2D"],
                           resolutions_list=tuple(h["resolutions_list"]), resolutions_list_2D=tuple(h["resolutions_list_2D"]),
                           ste_binary=h["ste_binary"], ste_multistep=h["ste_multistep"], add_noise=h["add_noise"],
                           Q=int(q) if q == int(q) else q, use_2D=h["use_2D"], device=dev)
        lo, hi = np.asarray(h["x_bound_min"], np.float32), np.asarray(h["x_bound_max"], np.float32)
        pc.x_bound_min, pc.x_bound_max = torch.from_numpy(lo.copy()).view(1, 3).to(dev), torch.from_numpy(hi.copy()).view(1, 3).to(dev)
        pc.bound_min_host, pc.bound_max_host = tuple(float(v) for v in lo), tuple(float(v) for v in hi)
        io.init_anchor_params(pc, int(h["n_full"]))          # the per-anchor tensors at the size the decoder fills
        with torch.no_grad():
            pc._rotation[:, 0] = 1.0                         # anchors are axis-aligned in GSVC: the identity, as create_from_points sets it
            sd = pc.state_dict()
            try:
                weights = mlp_codec.decode_mlp_bytes(self.mlp_bytes)
            except Exception as e:  # noqa: BLE001
                raise BitstreamError("MLPS", f"the MLP stream does not decode ({e})") from e
            for k, v in weights.items():
                if k not in sd or tuple(sd[k].shape) != tuple(v.shape):
                    raise BitstreamError("MLPS", f"tensor {k} {tuple(v.shape)} does not fit the model HEAD describes")
                sd[k].copy_(v.to(sd[k].device))
        pack = self.pack
        if pack.anchors_q is None:
            try:
                if dev.type == "cuda":
                    pack.anchors_q_dev = anchor_codec.decode_anchors_gpu(pack.anchor_stream, dev)
                    pack.anchors_q = pack.anchors_q_dev.cpu().numpy().astype(np.uint16)
                else:
                    pack.anchors_q = anchor_codec.decode_anchors(pack.anchor_stream)
            except Exception as e:  # noqa: BLE001
                raise BitstreamError("ANCH", f"the anchor stream does not decode ({e})") from e
        if int(pack.anchors_q.shape[0]) != int(pack.n):
            raise BitstreamError("ANCH", f"{pack.anchors_q.shape[0]} anchors decoded, HEAD says {pack.n}")
        conduct_stream_decoding(pc, pack)
        pipe = PipelineParams(raster_flags=h["raster_flags"], raster_low_pass=float(h["raster_low_pass"]))
        bg = torch.tensor([float(v) for v in h["background"]], dtype=torch.float32)      # host tensor: the kernels take it by value
        return pc, self.frames(), pipe, bg


def parse_bitstream(blob: bytes) -> Bitstream:
    """``read_bitstream`` of the file's bytes."""
    from .frames_out import FrameFormat
    from .stream_codec import StreamPack
    found = {}
    for tag, payload in unpack_sections(blob, known=KNOWN_TAGS):
        if tag in found:
            raise BitstreamError(tag.decode("ascii"), "the section appears twice")
        found[tag] = payload
    for tag in REQUIRED_TAGS:
        if tag not in found:
            raise BitstreamError(tag.decode("ascii"), "the section is missing")
    h = unpack_fields(found[b"HEAD"], "HEAD")
    for name in _HEAD_FIELDS:
        if name not in h:
            raise BitstreamError("HEAD", f"field {name} is missing")
    slabs = [(h["slabs"][i], h["slabs"][i + 1]) for i in range(0, len(h["slabs"]) - 1, 2)]
    feat, scaling, offsets = _unpack_slabs(found[b"SLAB"], len(slabs))
    pack = StreamPack(n_full=h["n_full"], n=h["n"], anchor_interval=np.asarray(h["anchor_interval"], np.float32),
                      anchor_min=np.asarray(h["anchor_min"], np.float32), anchors_q=None, prob_masks=float(h["prob_masks"]),
                      prob_hash=float(h["prob_hash"]), slabs=slabs, feat=feat, scaling=scaling, offsets=offsets, masks=found[b"MASK"],
                      hash=found[b"HASH"], bit_mlp_encoded=8 * len(found[b"MLPS"]), anchor_stream=found[b"ANCH"])
    bs = Bitstream(header=h, pack=pack, mlp_bytes=found[b"MLPS"], section_bytes={t.decode("ascii"): len(p) for t, p in found.items()},
                   file_bytes=len(blob))
    if b"PHSH" in found:
        f, hashes = _unpack_hashes(found[b"PHSH"])
        if hashes.shape[0] != h["frames"]:
            raise BitstreamError("PHSH", f"hashes of {hashes.shape[0]} frames in a file of {h['frames']}")
        try:
            bs.hash_format = FrameFormat.from_name(f["format"], f["matrix"], f["range"], f["rounding"])
        except (ValueError, KeyError) as e:
            raise BitstreamError("PHSH", f"unknown frame format ({e})") from e
        bs.hashes = hashes
    if b"GRAN" in found:
        from .grain import GrainParams
        bs.grain = GrainParams.unpack(found[b"GRAN"])
    if b"DISP" in found:
        bs.display = unpack_display(found[b"DISP"])
    return bs


def read_bitstream(path) -> Bitstream:
    """Read and check a ``.gsvc`` file (magic, version, every section's length and CRC) -> ``Bitstream``.  ``BitstreamError`` names the
    section that is damaged; nothing partial is returned."""
    with open(path, "rb") as f:
        return parse_bitstream(f.read())


# ----------------------------------------------------------------------------------------------------------------------------
# decoding to frames
# ----------------------------------------------------------------------------------------------------------------------------
class NullSink:
    """A sink that drops its frames (the encoder's verification pass)."""

    def __init__(self):
        self.frames = 0
        self.bytes = 0

    def write(self, frame_u8):
        self.frames += 1

    def close(self):
        pass


def _same_format(a, b) -> bool:
    return (a.layout, a.depth, a.matrix, a.range, a.rounding_used) == (b.layout, b.depth, b.matrix, b.range, b.rounding_used)


def hashed_frames(frames, pc, pipe, bg, H: int, W: int, fmt, batch: int, hashes_out, grain=None, first_frame: int = 0, out_size=None):
    """``render_frames_u8(..., to_host=True)`` with the picture hash of every batch taken ON THE DEVICE, before the host copy: yields the
    frames as host tensors and appends one int64 ``[n, 3]`` device tensor per batch to ``hashes_out`` (None: no hashes are taken).
    ``grain`` (``grain.GrainParams``): film grain is added to every batch behind its hashes; ``first_frame``: the index of ``frames[0]``
    in the whole clip.  ``out_size=(H, W)``: every batch is resampled to this size behind its hashes (and before its grain)."""
    from .frames_out import render_frames_u8
    from .metrics import picture_hash
    hook = None if hashes_out is None else (lambda rows: hashes_out.append(picture_hash(rows, H, W, fmt)))
    return render_frames_u8(frames, pc, pipe, bg, fmt=fmt, batch=batch, to_host=True, on_device_batch=hook, grain=grain,
                            first_frame=first_frame, out_size=out_size)


def grain_to_apply(bs, fmt, film_grain: bool):
    """The ``GrainParams`` a decode of ``bs`` into ``fmt`` applies: the file's, unless it has none, ``film_grain`` is off or ``fmt`` is
    ``rgb24`` (grain lives in the delivered Y'CbCr domain)."""
    return bs.grain if film_grain and bs.grain is not None and fmt.layout != "rgb24" else None


def delivered_size(coded, display, size, fmt, what: str) -> tuple:
    """``(W, H)`` a decode into ``fmt`` delivers for ``size`` = "display" (``display``, the size of DISP, when the file has one), "coded"
    or ``(W, H)``.  An ``rgb24`` decode delivers the coded size whatever was asked (the resampler works on Y'CbCr codes; the convention
    of film grain); otherwise a size other than the coded one must be one the resampler takes (``resample.check_sizes``)."""
    from .resample import check_sizes
    coded = (int(coded[0]), int(coded[1]))
    if isinstance(size, str):
        if size not in ("display", "coded"):
            raise ValueError(f"{what}: size is 'display', 'coded' or (W, H) (got {size!r})")
        want = coded if size == "coded" or display is None else (int(display[0]), int(display[1]))
    else:
        try:
            want = tuple(int(v) for v in size)
        except (TypeError, ValueError):
            want = ()
        if len(want) != 2:
            raise ValueError(f"{what}: size is 'display', 'coded' or (W, H) (got {size!r})")
    if fmt.layout == "rgb24" or want == coded:
        return coded
    check_sizes(coded[1], coded[0], want[1], want[0], fmt, what)
    return want


def decode_video(bitstream_or_path, sink, fmt=None, batch: int = 8, verify: bool = True, strict: bool = False, device="cuda",
                 film_grain: bool = True, size="display") -> dict:
    """Decode a bitstream file to frames of ``fmt`` (default: the file's PHSH format, else yuv420p) into ``sink`` (``write`` / ``close``:
    ``frames_out.open_sink``, ``NullSink``).  With ``verify`` the picture hash of every frame is taken on the device before the host
    copy and, where the file carries PHSH in the same format, compared.  Returns {"frames", "bytes", "seconds", "fps", "format",
    "hashes" (uint64 [frames, 3], with ``verify``), "verified" (bool), "frames_verified", "frames_mismatched", "mismatched" (indices),
    "verify_skipped" (why nothing was compared, or None), "film_grain" (whether grain was added)}.  ``strict``: a mismatch raises
    ``BitstreamError`` (after the frames were written), and so does a file without comparable hashes.  ``film_grain``: a file with a GRAN
    section has its grain synthesised on the delivered frames (``grain.apply_grain``) behind the picture hashes, which stay those of
    the ungrained pictures; False, a file without GRAN or an ``rgb24`` decode deliver the pictures as they are.  ``size``: "display" (the
    default: the size of the file's DISP section when it has one, else the coded size), "coded" (HEAD's size, as the model renders), or
    ``(W, H)``: any size within the resampler's ratio limit, for any file (a preview decode).  A delivered size other than the coded one
    is reached by ``resample.resample_frames`` on the device behind the picture hashes — PHSH and ``strict`` speak of the coded-size
    pictures — and before the grain.  An ``rgb24`` decode delivers the coded-size pictures.  The result has "W", "H" (of the frames
    delivered) and "resampled" (whether they were resampled)."""
    import torch

    from .frames_out import FrameFormat, write_frames
    bs = bitstream_or_path if isinstance(bitstream_or_path, Bitstream) else read_bitstream(bitstream_or_path)
    if fmt is None:
        fmt = bs.hash_format or FrameFormat("yuv420p")
    H, W = bs.header["H"], bs.header["W"]
    out_W, out_H = delivered_size((W, H), bs.display, size, fmt, "decode_video")          # (a size that cannot be had: before the model is built)
    out_size = None if (out_W, out_H) == (W, H) else (out_H, out_W)
    pc, frames, pipe, bg = bs.build_model(device)
    per_batch = [] if verify else None
    grain = grain_to_apply(bs, fmt, film_grain)
    with torch.no_grad():
        res = write_frames(hashed_frames(frames, pc, pipe, bg, H, W, fmt, int(batch), per_batch, grain=grain, out_size=out_size), sink)
    res["format"] = fmt.name
    res["film_grain"] = grain is not None
    res.update(W=out_W, H=out_H, resampled=out_size is not None)
    res.update(verified=False, frames_verified=0, frames_mismatched=0, mismatched=[], verify_skipped=None)
    if not verify:
        res["verify_skipped"] = "verification was turned off"
    else:
        got = torch.cat(per_batch).cpu().numpy().view(np.uint64)
        res["hashes"] = got
        if bs.hashes is None:
            res["verify_skipped"] = "the file carries no picture hashes (PHSH)"
        elif not _same_format(fmt, bs.hash_format):
            res["verify_skipped"] = (f"the file's picture hashes are of {bs.hash_format.name} ({bs.hash_format.matrix}, {bs.hash_format.range}, "
                                     f"{bs.hash_format.rounding_used}) frames, not of the {fmt.name} ({fmt.matrix}, {fmt.range}, "
                                     f"{fmt.rounding_used}) frames decoded")
        else:
            bad = np.nonzero((got != bs.hashes).any(axis=1))[0].tolist()
            res.update(verified=True, frames_verified=int(got.shape[0]) - len(bad), frames_mismatched=len(bad), mismatched=bad)
    if strict and res["frames_mismatched"]:
        raise BitstreamError("PHSH", f"picture hash mismatch in {res['frames_mismatched']} of {len(frames)} frames: {res['mismatched']}")
    if strict and not res["verified"]:
        raise BitstreamError("PHSH", f"nothing was verified: {res['verify_skipped']}")
    return res
