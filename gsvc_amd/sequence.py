"""The sequence file: several groups of pictures (GOPs) in ONE ``.gsvs`` file, each of them a complete bitstream file image of
gsvc_amd/bitstream.py, so that a decoder can start at any GOP and holds one GOP's model at a time.  The section
framing is that of the bitstream file under another magic:

    b"GSVS" | uint16 version (1) | uint16 sections | sections x (4-byte tag, uint64 length, uint32 CRC-32 of the payload) | payloads

    SEQH   typed fields (``bitstream.pack_fields``): W, H, fps_num, fps_den, frames, and per GOP gop_first, gop_frames and gop_cut (1 where
           the GOP starts at a detected scene cut)
    GOPU   one per GOP, in order: a COMPLETE ``GSVC`` version-1 file image — its own table, CRCs and picture hashes (PHSH)

SEQH's W x H is the CODED size, that of every GOP's HEAD; a sequence coded at a reduced size carries its display size in every GOP's DISP
section, the same in all of them (``Sequence.display_size``; ``decode_sequence`` refuses a file whose GOPs disagree).

A reader skips tags it does not know; a newer version is refused.  ``open_sequence`` reads the prefix, the table and SEQH only; a GOP's
bytes are read when ``Sequence.gop(k)`` asks for them.  A plain ``GSVC`` file opens as a sequence of one GOP.

``write_sequence`` / ``open_sequence`` need neither a GPU nor the built library; ``decode_sequence`` does.
"""
from __future__ import annotations

import os
import struct
import time
import zlib
from dataclasses import dataclass, field

import numpy as np

from .bitstream import (_ENTRY, _PREFIX, MAGIC, VERSION, Bitstream, BitstreamError, CubeGeometry, _same_format, delivered_size, grain_to_apply,
                        hashed_frames, pack_fields, parse_bitstream, unpack_fields)

SEQ_MAGIC = b"GSVS"
SEQ_VERSION = 1
_SEQH_FIELDS = ("W", "H", "fps_num", "fps_den", "frames", "gop_first", "gop_frames", "gop_cut")


def sequence_bytes(gop_blobs, W: int, H: int, fps, cut_flags=None) -> bytes:
    """The bytes ``write_sequence`` writes.  The index is taken from the GOPs themselves: GOP k starts where GOP k - 1 ends."""
    blobs = [bytes(b) for b in gop_blobs]
    if not blobs:
        raise ValueError("write_sequence: a sequence holds at least one GOP")
    if len(blobs) > 65534:
        raise ValueError(f"write_sequence: at most 65534 GOPs fit one file (got {len(blobs)})")
    cut_flags = [0] * len(blobs) if cut_flags is None else [int(bool(c)) for c in cut_flags]
    if len(cut_flags) != len(blobs):
        raise ValueError(f"write_sequence: {len(cut_flags)} cut flags for {len(blobs)} GOPs")
    counts = [_head_of(b, "GOPU[%d]" % k)["frames"] for k, b in enumerate(blobs)]
    firsts = [int(v) for v in np.cumsum([0] + counts[:-1])]
    seqh = pack_fields({"W": int(W), "H": int(H), "fps_num": int(fps[0]), "fps_den": int(fps[1]), "frames": int(sum(counts)),
                        "gop_first": firsts, "gop_frames": counts, "gop_cut": cut_flags})
    sections = [(b"SEQH", seqh)] + [(b"GOPU", b) for b in blobs]
    out = [_PREFIX.pack(SEQ_MAGIC, SEQ_VERSION, len(sections))]
    out += [_ENTRY.pack(tag, len(p), zlib.crc32(p) & 0xFFFFFFFF) for tag, p in sections]
    out += [p for _, p in sections]
    return b"".join(out)


def write_sequence(path, gop_blobs, W: int, H: int, fps, cut_flags=None) -> dict:
    """Write the GOPs' file images (``bitstream.bitstream_bytes`` / ``with_hashes``) as one sequence file; returns {"bytes", "gops"}."""
    gop_blobs = list(gop_blobs)
    blob = sequence_bytes(gop_blobs, W, H, fps, cut_flags)
    with open(path, "wb") as f:
        f.write(blob)
    return {"bytes": len(blob), "gops": len(gop_blobs)}


def _table_of(f, size: int, magic: bytes, newest: int):
    """The prefix and the section table of an open file -> [(tag, offset, length, crc)]."""
    head = f.read(_PREFIX.size)
    if len(head) < 4 or head[:4] != magic:
        raise BitstreamError("magic", f"not a {magic.decode()} file" if len(head) >= 4 else "truncated inside the magic")
    if len(head) < _PREFIX.size:
        raise BitstreamError("version", "truncated inside the file prefix")
    _, version, count = _PREFIX.unpack(head)
    if version > newest or version < 1:
        raise BitstreamError("version", f"version {version} is not readable by this decoder (it reads up to {newest})")
    raw = f.read(count * _ENTRY.size)
    if len(raw) < count * _ENTRY.size:
        raise BitstreamError("table", f"truncated inside the section table ({count} sections)")
    at, table = _PREFIX.size + count * _ENTRY.size, []
    for i in range(count):
        tag, length, crc = _ENTRY.unpack_from(raw, i * _ENTRY.size)
        table.append((tag, at, length, crc))
        at += length
    return table


def _payload(f, size: int, entry, name: str) -> bytes:
    _, offset, length, crc = entry
    if offset + length > size:
        raise BitstreamError(name, f"truncated: {length} bytes declared, {max(size - offset, 0)} present")
    f.seek(offset)
    payload = f.read(length)
    if len(payload) != length:
        raise BitstreamError(name, f"truncated: {length} bytes declared, {len(payload)} present")
    if zlib.crc32(payload) & 0xFFFFFFFF != crc:
        raise BitstreamError(name, "CRC mismatch")
    return payload


def _head_of(blob: bytes, name: str) -> dict:
    """The HEAD fields of a GSVC file image (its table is read, only HEAD's CRC is checked)."""
    import io
    try:
        f = io.BytesIO(blob)
        for entry in _table_of(f, len(blob), MAGIC, VERSION):
            if entry[0] == b"HEAD":
                return unpack_fields(_payload(f, len(blob), entry, "HEAD"), "HEAD")
        raise BitstreamError("HEAD", "the section is missing")
    except BitstreamError as e:
        raise ValueError(f"write_sequence: {name} is not a bitstream file image ({e})") from e


@dataclass
class Sequence:
    """An opened sequence file: the picture, the GOP index and where each GOP's bytes lie.  ``gop(k)`` reads and checks one GOP."""
    path: str
    magic: bytes
    W: int
    H: int
    fps: tuple
    frames: int
    gops: list                                 # [(first, count)], tiling [0, frames)
    cuts: list                                 # per GOP: 1 where it starts at a detected scene cut
    file_bytes: int = 0
    _entries: list = field(default_factory=list, repr=False)

    @property
    def geometry(self) -> CubeGeometry:
        """The picture's size, frame count and rate (the cube geometry proper belongs to each GOP: ``gop(k).geometry``)."""
        return CubeGeometry(W=self.W, H=self.H, frames=self.frames, scale=max(self.H, self.W, self.frames) / 2, x_min=0.0, y_min=0.0, z_min=0.0,
                            threshold=0.0, fps=tuple(self.fps))

    def gop_bytes(self, k: int) -> int:
        return int(self._entries[k][2])

    def gop_image(self, k: int) -> bytes:
        """The bytes of GOP ``k``, a complete bitstream file image, read from the file and checked against the table's CRC."""
        k = int(k)
        if not 0 <= k < len(self.gops):
            raise IndexError(f"GOP {k} of {len(self.gops)}")
        with open(self.path, "rb") as f:
            if self.magic == MAGIC:
                return f.read()
            return _payload(f, self.file_bytes, self._entries[k], f"GOPU[{k}]")

    def gop(self, k: int) -> Bitstream:
        """Seek to GOP ``k``, check its CRC and parse it.  ``BitstreamError.section`` is ``"GOPU[k]"``; an error inside the GOP keeps its
        own section in the message.  A GOP whose W, H, frame rate or frame count disagrees with the index is refused."""
        k = int(k)
        if not 0 <= k < len(self.gops):
            raise IndexError(f"GOP {k} of {len(self.gops)}")
        name = f"GOPU[{k}]"
        payload = self.gop_image(k)
        if self.magic == MAGIC:
            return parse_bitstream(payload)                        # a plain bitstream file: its errors are its own
        try:
            bs = parse_bitstream(payload)
        except BitstreamError as e:
            raise BitstreamError(name, f"section {e.section}: {str(e).split(': ', 1)[-1]}") from e
        h = bs.header
        for key, want in (("W", self.W), ("H", self.H), ("fps_num", self.fps[0]), ("fps_den", self.fps[1]), ("frames", self.gops[k][1])):
            if h[key] != want:
                raise BitstreamError(name, f"section HEAD: {key} = {h[key]} disagrees with the sequence header ({want})")
        return bs

    @property
    def hash_format(self):
        """The format of the first GOP's picture hashes, or None."""
        return self.gop(0).hash_format

    @property
    def display(self):
        """``(W, H)`` of the first GOP's DISP section, or None: what every GOP of the file must say."""
        return self.gop(0).display

    @property
    def display_size(self) -> tuple:
        """``(W, H)`` a decode delivers by default: the first GOP's DISP where it has one, else the coded size of SEQH."""
        return self.display or (int(self.W), int(self.H))


def open_sequence(path) -> Sequence:
    """Open a ``.gsvs`` sequence file, or a plain ``.gsvc`` bitstream file as a sequence of one GOP: the prefix, the section table and
    the header (SEQH; HEAD of a plain file) are read and checked, no GOP is.  ``BitstreamError.section``: ``"magic"``, ``"version"``,
    ``"table"`` or ``"SEQH"`` here, ``"GOPU[k]"`` from ``Sequence.gop(k)``."""
    path = str(path)
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        magic = f.read(4)
        f.seek(0)
        if magic == MAGIC:
            table = _table_of(f, size, MAGIC, VERSION)
            heads = [e for e in table if e[0] == b"HEAD"]
            if not heads:
                raise BitstreamError("HEAD", "the section is missing")
            h = unpack_fields(_payload(f, size, heads[0], "HEAD"), "HEAD")
            for name in ("W", "H", "fps_num", "fps_den", "frames"):
                if name not in h:
                    raise BitstreamError("HEAD", f"field {name} is missing")
            return Sequence(path=path, magic=MAGIC, W=h["W"], H=h["H"], fps=(h["fps_num"], h["fps_den"]), frames=h["frames"],
                            gops=[(0, h["frames"])], cuts=[0], file_bytes=size, _entries=[(b"GOPU", 0, size, 0)])
        if len(magic) == 4 and magic != SEQ_MAGIC:
            raise BitstreamError("magic", "neither a GSVS sequence file nor a GSVC bitstream file")
        table = _table_of(f, size, SEQ_MAGIC, SEQ_VERSION)
        seqh = [e for e in table if e[0] == b"SEQH"]
        if len(seqh) != 1:
            raise BitstreamError("SEQH", "the section is missing" if not seqh else "the section appears twice")
        h = unpack_fields(_payload(f, size, seqh[0], "SEQH"), "SEQH")
    for name in _SEQH_FIELDS:
        if name not in h:
            raise BitstreamError("SEQH", f"field {name} is missing")
    entries = [e for e in table if e[0] == b"GOPU"]
    firsts, counts, cuts = h["gop_first"], h["gop_frames"], h["gop_cut"]
    if not (len(firsts) == len(counts) == len(cuts) == len(entries)) or not entries:
        raise BitstreamError("SEQH", f"the index lists {len(firsts)} / {len(counts)} / {len(cuts)} GOPs, the file holds {len(entries)}")
    at = 0
    for k, (first, count) in enumerate(zip(firsts, counts)):
        if first != at or count < 1:
            raise BitstreamError("SEQH", f"the index does not tile the frames: GOP {k} is ({first}, {count}), frame {at} comes next")
        at += count
    if at != h["frames"]:
        raise BitstreamError("SEQH", f"the index does not tile the frames: it ends at frame {at} of {h['frames']}")
    return Sequence(path=path, magic=SEQ_MAGIC, W=h["W"], H=h["H"], fps=(h["fps_num"], h["fps_den"]), frames=h["frames"],
                    gops=list(zip(firsts, counts)), cuts=[int(c) for c in cuts], file_bytes=size, _entries=entries)


def decode_sequence(path_or_seq, sink, fmt=None, batch: int = 8, verify: bool = True, strict: bool = False, device="cuda", frames=None,
                    film_grain: bool = True, size="display") -> dict:
    """``bitstream.decode_video`` of a sequence file, GOP by GOP into the ONE ``sink``: a GOP's bytes are read, its model built, its
    frames rendered, hashed on the device, compared with the GOP's PHSH and written; the model is dropped before the next GOP is
    built, so the peak device memory is one GOP's.  ``frames=(a, b)``: only the GOPs that overlap ``[a, b)`` are read and built and,
    within them, only those frames are compared and written; they are rendered in the render batches of a decode of the whole GOP (up
    to ``batch - 1`` frames more on either side), so that a frame has the bits it has there.  Returns the keys of ``decode_video`` with
    ``mismatched`` as indices into the whole sequence and ``hashes`` of the frames decoded, plus ``"gops"``: per GOP decoded {"gop",
    "first", "frames" (of the GOP), "decoded", "rendered", "bytes", "seconds", "frames_verified", "film_grain"}.  ``strict`` as in
    ``decode_video``.  ``film_grain``: a GOP with a GRAN section has ITS grain synthesised on its frames (behind the picture hashes), every
    frame under its index in the WHOLE clip, so that ``frames=(a, b)`` yields the bytes the same frames have in a full decode;
    ``"film_grain"`` of the result says whether any GOP decoded had grain added.  ``size``: as in ``decode_video`` ("display": the DISP
    size of the file's GOPs, else the coded size; "coded"; or ``(W, H)``); a GOP whose DISP section differs from the first GOP's is a
    ``BitstreamError`` whatever ``size`` says, and the result has "W", "H" and "resampled"."""
    import gc

    import torch

    from .frames_out import FrameFormat, write_frames
    seq = path_or_seq if isinstance(path_or_seq, Sequence) else open_sequence(path_or_seq)
    a, b = (0, seq.frames) if frames is None else (int(frames[0]), int(frames[1]))
    if not 0 <= a < b <= seq.frames:
        raise ValueError(f"decode_sequence: frames ({a}, {b}) is not a non-empty range inside the {seq.frames} frames of the file")
    todo = [(k, first, count) for k, (first, count) in enumerate(seq.gops) if first < b and first + count > a]
    state = {"fmt": fmt, "got": [], "skipped": None, "bad": [], "verified": 0, "compared": 0, "gops": [], "size": None}
    display = seq.display
    step = int(batch)
    if step < 1:
        raise ValueError("decode_sequence: batch must be at least 1")

    def run():
        for k, first, count in todo:
            t0 = time.perf_counter()
            bs = seq.gop(k)
            if state["fmt"] is None:
                state["fmt"] = bs.hash_format or FrameFormat("yuv420p")
            used = state["fmt"]
            if bs.display != display:
                raise BitstreamError(f"GOPU[{k}]", f"section DISP: the display size {bs.display} disagrees with that of GOP 0 ({display})")
            if state["size"] is None:
                state["size"] = delivered_size((seq.W, seq.H), display, size, used, "decode_sequence")
            out_W, out_H = state["size"]
            out_size = None if (out_W, out_H) == (seq.W, seq.H) else (out_H, out_W)
            lo, hi = max(a, first) - first, min(b, first + count) - first
            # rendered in the batches a decode of the whole GOP renders — [r0, r1) is [lo, hi) widened to multiples of ``batch`` —: the last
            # bit of a picture can depend on which frames share its generation batch; handed on and compared: [lo, hi)
            r0, r1 = lo // step * step, min(-(-hi // step) * step, count)
            pc, cams, pipe, bg = bs.build_model(device)
            per_batch = [] if verify else None
            grain = grain_to_apply(bs, used, film_grain)
            with torch.no_grad():
                for j, picture in enumerate(hashed_frames(cams[r0:r1], pc, pipe, bg, seq.H, seq.W, used, step, per_batch, grain=grain,
                                                          first_frame=first + r0, out_size=out_size)):
                    if lo <= r0 + j < hi:
                        yield picture
            ok = 0
            if verify:
                got = torch.cat(per_batch)[lo - r0:hi - r0].cpu().numpy().view(np.uint64)
                state["got"].append(got)
                if bs.hashes is None:
                    state["skipped"] = state["skipped"] or f"GOP {k} carries no picture hashes (PHSH)"
                elif not _same_format(used, bs.hash_format):
                    hf = bs.hash_format
                    state["skipped"] = state["skipped"] or (f"the picture hashes of GOP {k} are of {hf.name} ({hf.matrix}, {hf.range}, "
                                                            f"{hf.rounding_used}) frames, not of the {used.name} ({used.matrix}, {used.range}, "
                                                            f"{used.rounding_used}) frames decoded")
                else:
                    bad = np.nonzero((got != bs.hashes[lo:hi]).any(axis=1))[0]
                    state["bad"] += [int(first + lo + i) for i in bad]
                    ok = (hi - lo) - len(bad)
                    state["verified"] += ok
                    state["compared"] += 1
            del pc, cams, pipe, bg, bs, per_batch
            gc.collect()
            state["gops"].append({"gop": k, "first": first, "frames": count, "decoded": hi - lo, "rendered": r1 - r0, "bytes": seq.gop_bytes(k),
                                  "seconds": time.perf_counter() - t0, "frames_verified": ok, "film_grain": grain is not None})

    res = write_frames(run(), sink)
    used = state["fmt"]
    res["format"] = used.name
    res.update(verified=False, frames_verified=0, frames_mismatched=0, mismatched=[], verify_skipped=None, gops=state["gops"],
               film_grain=any(g["film_grain"] for g in state["gops"]))
    res.update(W=state["size"][0], H=state["size"][1], resampled=tuple(state["size"]) != (int(seq.W), int(seq.H)))
    if not verify:
        res["verify_skipped"] = "verification was turned off"
    else:
        res["hashes"] = np.concatenate(state["got"])
        if state["skipped"]:
            res["verify_skipped"] = state["skipped"]
        res.update(verified=state["skipped"] is None and state["compared"] == len(todo), frames_verified=state["verified"],
                   frames_mismatched=len(state["bad"]), mismatched=state["bad"])
    if strict and res["frames_mismatched"]:
        raise BitstreamError("PHSH", f"picture hash mismatch in {res['frames_mismatched']} of {res['frames']} frames: {res['mismatched']}")
    if strict and not res["verified"]:
        raise BitstreamError("PHSH", f"nothing was verified: {res['verify_skipped']}")
    return res
