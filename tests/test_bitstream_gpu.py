"""GPU tests of the bitstream file end to end (gsvc_amd/bitstream.py, tools/gsvc_decode.py): a tiny fit (8 frames of 64 x 48, 3 000
initial anchors, 60 steps through all four phases — the shared set-up of gsvc_amd/fit_setup.py, so that the model has been through what a
real one has; the untrained helper of tests/test_codec_gpu.py fixes a 256 x 256 x 64 cube) is stream-encoded and written as ONE file.  Every
reference to the encoder's model and cube is dropped; a model rebuilt from the file alone must then deliver, as yuv420p codes, exactly the
frames the encoder side renders from ``conduct_stream_decoding(deepcopy(q), pack_q, mlp_file)`` — the container adds nothing and loses
nothing — in this process and in a fresh one; damage is reported by section, a changed picture hash by frame."""
import copy
import gc
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gsvc_amd import bitstream as B
from gsvc_amd.frames_out import FrameFormat, frame_bytes, read_y4m

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, T = 48, 64, 8
FMT = FrameFormat("yuv420p")


class _Keep:
    """A sink that keeps its frames."""

    def __init__(self):
        self.rows, self.bytes = [], 0

    def write(self, frame_u8):
        self.rows.append(np.array(frame_u8, copy=True))

    def close(self):
        pass


@pytest.fixture(scope="module")
def encoded(tmp_path_factory):
    """{"plain": the file without hashes, "hashed": with PHSH (yuv420p), "want": uint8 [T, frame_bytes], the encoder side's frames}."""
    from gsvc_amd.arguments import cfg_20240919
    from gsvc_amd.fit_setup import configure_fit, new_fit
    from gsvc_amd.frame import SyntheticFrameCube
    from gsvc_amd.frames_out import render_frames_u8
    from gsvc_amd.stream_codec import conduct_stream_decoding, conduct_stream_encoding
    tmp = tmp_path_factory.mktemp("bitstream")
    dev = torch.device("cuda", 0)
    mp_, opt, pipe = cfg_20240919()
    cube = SyntheticFrameCube(H, W, T, seed=1234, device=dev).materialize()
    steps = 60
    configure_fit(mp_, opt, cube, steps, 0.004, 8.0, 2e-5)
    q, trainer = new_fit(cube, mp_, opt, pipe, 3000, dev)
    bg = trainer.background
    for it in range(1, steps + 1):
        trainer.step(it)
    torch.cuda.synchronize()
    trainer.close()
    mlp_file = str(tmp / "mlp.bin")
    with torch.no_grad():
        pack_q = conduct_stream_encoding(q, mlp_file=mlp_file)
        dec_q = conduct_stream_decoding(copy.deepcopy(q), pack_q, mlp_file=mlp_file)
        frames = [cube.get_dummy_frame(i) for i in range(T)]
        want = torch.stack(list(render_frames_u8(frames, dec_q, pipe, bg, fmt=FMT, batch=8, to_host=False))).cpu().numpy()
    assert want.shape == (T, frame_bytes(H, W, FMT)) and len(np.unique(want)) > 8          # (pictures, not a constant)
    plain = str(tmp / "clip.gsvc")
    with open(mlp_file, "rb") as f:
        written = B.write_bitstream(plain, q, pack_q, B.CubeGeometry.of(cube, mp_, pipe, bg.tolist()), f.read())
    assert written["bytes"] == os.path.getsize(plain) and set(written["sections"]) == {"HEAD", "MLPS", "ANCH", "MASK", "HASH", "SLAB"}
    n_coded = int(pack_q.n)
    # nothing of the encoder survives this line: the model, its copy, the pack, the cube, the trainer
    del q, dec_q, pack_q, cube, trainer, frames, mp_, opt, pipe, bg
    gc.collect()
    torch.cuda.empty_cache()
    # the encoder's last step (tools/gsvc_encode.py): the decoder's own path on the file gives the hashes the file then carries
    res = B.decode_video(plain, B.NullSink(), fmt=FMT, batch=8, verify=True)
    assert res["frames"] == T and res["verified"] is False and "no picture hashes" in res["verify_skipped"]
    hashed = str(tmp / "clip_hashed.gsvc")
    with open(plain, "rb") as f, open(hashed, "wb") as g:
        g.write(B.with_hashes(f.read(), FMT, res["hashes"]))
    return {"plain": plain, "hashed": hashed, "want": want, "anchors": n_coded, "tmp": tmp}


def test_the_file_alone_rebuilds_the_encoder_sides_frames(encoded):
    from gsvc_amd.frames_out import render_frames_u8
    bs = B.read_bitstream(encoded["plain"])
    assert (bs.header["W"], bs.header["H"], bs.header["frames"]) == (W, H, T) and bs.pack.n == encoded["anchors"]
    assert bs.file_bytes == os.path.getsize(encoded["plain"])
    pc, frames, pipe, bg = bs.build_model("cuda")
    assert pc.decoded_version and len(frames) == T and int(pc._anchor.shape[0]) == bs.pack.n_full
    with torch.no_grad():
        got = torch.stack(list(render_frames_u8(frames, pc, pipe, bg, fmt=FMT, batch=8, to_host=False))).cpu().numpy()
    assert np.array_equal(got, encoded["want"]), int((got != encoded["want"]).sum())
    # and through decode_video's own loop (hash on the device, then the host copy), batches that do not divide the frame count
    sink = _Keep()
    res = B.decode_video(encoded["plain"], sink, fmt=FMT, batch=3, verify=False)
    assert res["frames"] == T and res["verify_skipped"] == "verification was turned off" and "hashes" not in res
    assert np.array_equal(np.stack(sink.rows), encoded["want"])


def test_decode_video_verifies_every_frame_here_and_in_a_fresh_process(encoded):
    from tests import _picture_hash_ref as ref
    bs = B.read_bitstream(encoded["hashed"])
    assert bs.hash_format == FrameFormat("yuv420p", rounding="nearest") and bs.hashes.shape == (T, 3)
    assert np.array_equal(bs.hashes, ref.picture_hash_ref(encoded["want"], H, W, "yuv420p", 8))          # the hashes ARE those of the frames
    res = B.decode_video(bs, B.NullSink(), fmt=FMT, batch=8, strict=True)
    assert res["verified"] and res["frames_verified"] == T and res["frames_mismatched"] == 0 and res["mismatched"] == []
    out = str(encoded["tmp"] / "out.y4m")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gsvc_decode.py"), encoded["hashed"], "-o", out, "--strict"], cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-2500:])
    line = json.loads(run.stdout.strip().splitlines()[-1])
    assert line["frames"] == T and line["frames_verified"] == T and line["frames_mismatched"] == 0 and line["format"] == "yuv420p"
    hdr, frames = read_y4m(out)
    assert (hdr["W"], hdr["H"], hdr["layout"], hdr["depth"]) == (W, H, "yuv420p", 8)
    assert np.array_equal(frames, encoded["want"])


def test_a_flipped_slab_byte_is_a_crc_error(encoded, tmp_path):
    blob = bytearray(open(encoded["hashed"], "rb").read())
    sections = B.unpack_sections(bytes(blob))
    at = 8 + 16 * len(sections)
    for tag, payload in sections:
        if tag == b"SLAB":
            break
        at += len(payload)
    blob[at + len(payload) // 2] ^= 0x01
    bad = tmp_path / "bad.gsvc"
    bad.write_bytes(bytes(blob))
    with pytest.raises(B.BitstreamError, match="CRC") as e:
        B.read_bitstream(bad)
    assert e.value.section == "SLAB"
    with pytest.raises(B.BitstreamError):
        B.decode_video(str(bad), B.NullSink())


def test_an_edited_picture_hash_is_reported_for_exactly_that_frame(encoded, tmp_path):
    blob = open(encoded["hashed"], "rb").read()
    bs = B.read_bitstream(encoded["hashed"])
    hashes = bs.hashes.copy()
    hashes[5, 1] ^= np.uint64(1)          # one bit of the U plane's hash of frame 5; with_hashes writes the section's new CRC
    edited = tmp_path / "edited.gsvc"
    edited.write_bytes(B.with_hashes(blob, bs.hash_format, hashes))
    res = B.decode_video(str(edited), B.NullSink(), fmt=FMT)
    assert res["verified"] and res["frames_mismatched"] == 1 and res["mismatched"] == [5] and res["frames_verified"] == T - 1
    with pytest.raises(B.BitstreamError, match=r"\[5\]") as e:
        B.decode_video(str(edited), B.NullSink(), fmt=FMT, strict=True)
    assert e.value.section == "PHSH"
    out = str(tmp_path / "out.y4m")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gsvc_decode.py"), str(edited), "-o", out, "--strict"], cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode != 0 and "[5]" in run.stderr, (run.returncode, run.stdout[-1500:], run.stderr[-2500:])


def test_another_format_skips_verification_and_says_so(encoded):
    for fmt in (FrameFormat("yuv444p"), FrameFormat("yuv420p", depth=10), FrameFormat("yuv420p", range="full")):
        sink = _Keep()
        res = B.decode_video(encoded["hashed"], sink, fmt=fmt)
        assert res["verified"] is False and res["frames_verified"] == 0 and res["frames_mismatched"] == 0
        assert "yuv420p" in res["verify_skipped"] and fmt.name in res["verify_skipped"]
        assert len(sink.rows) == T and sink.rows[0].shape == (frame_bytes(H, W, fmt),) and res["hashes"].shape == (T, 3)


def test_encode_tool_then_decode_tool_in_another_process(tmp_path):
    """tools/gsvc_encode.py on a small Y4M clip, then tools/gsvc_decode.py --strict in a fresh process that sees nothing but the file: it
    writes the video, every frame verified; the bpp the encoder prints is the size of that one file."""
    from gsvc_amd.frame import SyntheticFrameCube
    from gsvc_amd.frames_out import Y4MWriter, frames_to_u8
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gsvc_encode
    cube = SyntheticFrameCube(H, W, T, seed=7, device="cuda")
    clip, out, coded = str(tmp_path / "clip.y4m"), str(tmp_path / "out.y4m"), str(tmp_path / "clip.gsvc")
    with Y4MWriter(clip, W, H, (25, 1), FMT) as sink:
        for fr in frames_to_u8([cube._image(t) for t in range(T)], FMT).cpu():
            sink.write(fr)
    del cube
    log = gsvc_encode.main([clip, "-o", coded, "--steps", "40", "--anchors", "2000", "--slab-frames", "8", "--densify-grad-threshold", "2e-5"])
    size = os.path.getsize(coded)
    assert log["total_bytes"] == size and log["bpp"] == 8.0 * size / (H * W * T) and log["hash_format"] == "yuv420p"
    assert set(log["sections"]) == {"HEAD", "MLPS", "ANCH", "MASK", "HASH", "SLAB", "PHSH"} and sum(log["sections"].values()) + 8 + 16 * 7 == size
    assert B.read_bitstream(coded).geometry.fps == (25, 1)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gsvc_decode.py"), coded, "-o", out, "--strict"], cwd=str(tmp_path),
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-2500:])
    line = json.loads(run.stdout.strip().splitlines()[-1])
    assert line["frames_verified"] == T and line["frames_mismatched"] == 0
    hdr, frames = read_y4m(out)
    assert (hdr["W"], hdr["H"], hdr["fps"], frames.shape) == (W, H, (25, 1), (T, frame_bytes(H, W, FMT)))
