"""GPU tests of the group-of-pictures path end to end: a 16-frame 64 x 48 clip with one scene change goes through
the cut detector (``scene.video_histograms``, the kernel of csrc/scene.hip), tools/gsvc_encode.py with --gop-frames / --scene-cuts (two
tiny fits, as tests/test_bitstream_gpu.py's), the sequence file (gsvc_amd/sequence.py) and tools/gsvc_decode.py in a fresh process:
the index, every frame verified, random access to frames 10 .. 12 building one GOP, damage named by GOP and by global frame.

The clip: ``SyntheticFrameCube(48, 64, 16, seed=7)`` as yuv420p, its luma codes remapped on the host into two disjoint ranges,
16 + (c - 16) * 94 // 219 (16 .. 110) for frames 0 - 7 and 141 + (c - 16) * 94 // 219 (141 .. 235) for frames 8 - 15; chroma is
untouched.  The reference distance (tests/_scene_ref.py) is then exactly 1.0 at the cut and, computed on the CPU for this clip, at most
0.135 elsewhere at 256 bins: the fixture asserts 1.0 and < 0.25 before anything else, the detector runs at its default 0.5."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gsvc_amd import bitstream as B
from gsvc_amd import scene
from gsvc_amd import sequence as S
from gsvc_amd.frames_out import FrameFormat, Y4MWriter, frame_bytes, read_y4m
from tests import _scene_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, T, CUT = 48, 64, 16, 8
FMT = FrameFormat("yuv420p")
NB = frame_bytes(H, W, FMT)
FIT = ["--steps", "40", "--anchors", "2000", "--slab-frames", "8", "--densify-grad-threshold", "2e-5"]
sys.path.insert(0, os.path.join(ROOT, "tools"))


class _Keep:
    """A sink that keeps its frames."""

    def __init__(self):
        self.rows, self.bytes = [], 0

    def write(self, frame_u8):
        self.rows.append(np.array(frame_u8, copy=True))

    def close(self):
        pass


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """{"path": the Y4M file, "frames": uint8 [T, NB], "hist": the reference histograms, "tmp"}."""
    from gsvc_amd.frame import SyntheticFrameCube
    from gsvc_amd.frames_out import frames_to_u8
    tmp = tmp_path_factory.mktemp("sequence")
    cube = SyntheticFrameCube(H, W, T, seed=7, device="cuda")
    frames = frames_to_u8([cube._image(t) for t in range(T)], FMT).cpu().numpy().copy()
    del cube
    luma = frames[:, :H * W].astype(np.int64)
    assert luma.min() >= 16 and luma.max() <= 235          # limited-range codes: the two remapped ranges are 16 .. 110 and 141 .. 235
    frames[:CUT, :H * W] = (16 + (luma[:CUT] - 16) * 94 // 219).astype(np.uint8)
    frames[CUT:, :H * W] = (141 + (luma[CUT:] - 16) * 94 // 219).astype(np.uint8)
    hist = ref.histogram_ref(frames, H, W, "yuv420p", 8)
    for bins in (256, 64):
        d_ref = ref.distance_ref(hist, bins=bins)
        assert d_ref[CUT - 1] == 1.0 and max(d for t, d in enumerate(d_ref) if t != CUT - 1) < 0.25, d_ref
    path = str(tmp / "clip.y4m")
    with Y4MWriter(path, W, H, (25, 1), FMT) as sink:
        for fr in frames:
            sink.write(torch.from_numpy(fr))
    return {"path": path, "frames": frames, "hist": hist, "tmp": tmp}


@pytest.fixture(scope="module")
def encoded(clip):
    """The clip encoded with scene cuts: {"file", "log"}."""
    import gsvc_encode
    coded = str(clip["tmp"] / "clip.gsvs")
    log = gsvc_encode.main([clip["path"], "-o", coded, "--gop-frames", "12", "--scene-cuts", "--min-gop", "4"] + FIT)
    return {"file": coded, "log": log}


@pytest.fixture(scope="module")
def whole(encoded):
    """``decode_sequence`` of the whole file in this process: {"frames": uint8 [T, NB], "res"}."""
    sink = _Keep()
    res = S.decode_sequence(encoded["file"], sink, strict=True)
    return {"frames": np.stack(sink.rows), "res": res}


def test_video_histograms_are_the_reference_and_the_cut_is_found(clip):
    got = scene.video_histograms(clip["path"], "cuda")
    assert got.dtype == np.int32 and got.shape == (T, 3, 256) and np.array_equal(got.astype(np.int64), clip["hist"])
    assert np.array_equal(scene.video_histograms(clip["path"], "cuda", chunk=5), got)          # chunks that do not divide the clip
    d = scene.histogram_distance(got)
    assert d.tolist() == ref.distance_ref(clip["hist"]) and d[CUT - 1] == 1.0
    assert scene.scene_cuts(d) == [CUT]
    cuts, d2 = scene.detect_cuts(clip["path"], "cuda")
    assert cuts == [CUT] and d2.tolist() == d.tolist()


def test_a_frame_range_is_a_cube_of_its_own(clip):
    from gsvc_amd.frames_in import VideoFileCube
    full = VideoFileCube(clip["path"], device="cuda")
    part = VideoFileCube(clip["path"], device="cuda", frame_range=(CUT, T))
    assert len(part) == part.len_z_frames == T - CUT and part.frame_range == (CUT, T) and full.frame_range is None and len(full) == T
    assert part.scale == max(H, W, T - CUT) / 2 and part.z_min == -(T - CUT) / 2 / part.scale and part.x_min == -W / 2 / part.scale
    for i in (0, 3, T - CUT - 1):
        assert torch.equal(part[i].image, full[CUT + i].image) and part[i].z == (i - (T - CUT) / 2) / part.scale
    with pytest.raises(IndexError):
        part.get_z_frame(T - CUT)
    g = B.CubeGeometry.of(part, type("M", (), {"threshold": 0.1, "sh_degree": 0}))
    assert (g.frames, g.fps, g.z_min) == (T - CUT, (25, 1), part.z_min)
    # the flow estimator takes it as it takes any cube: one field per pair INSIDE the range
    from gsvc_amd.flow import EstimatedFlowCube
    flows = EstimatedFlowCube(part)
    assert len(flows) == T - CUT and flows.scale == part.scale and tuple(flows.get_optical_flow(T - CUT - 2).shape) == (2, H, W)
    with pytest.raises(IndexError):
        flows.get_optical_flow(T - CUT - 1)


def test_encode_with_scene_cuts_writes_a_sequence_file(encoded):
    log, size = encoded["log"], os.path.getsize(encoded["file"])
    with open(encoded["file"], "rb") as f:
        assert f.read(4) == b"GSVS"
    seq = S.open_sequence(encoded["file"])
    assert seq.gops == [(0, CUT), (CUT, T - CUT)] and seq.cuts == [0, 1] and (seq.W, seq.H, seq.frames, seq.fps) == (W, H, T, (25, 1))
    assert log["total_bytes"] == size == seq.file_bytes and log["bpp"] == 8.0 * size / (H * W * T) and log["scene_cuts"] == [CUT]
    assert [(g["first"], g["frames"], g["cut"]) for g in log["gops"]] == [(0, CUT, 0), (CUT, T - CUT, 1)]
    total = 0
    for k, g in enumerate(log["gops"]):
        image = seq.gop_image(k)
        bs = B.parse_bitstream(image)                  # each GOPU is a complete bitstream file of its own
        assert bs.hashes is not None and bs.hashes.shape == (g["frames"], 3) and bs.hash_format == FrameFormat("yuv420p", rounding="nearest")
        assert (bs.header["W"], bs.header["H"], bs.header["frames"]) == (W, H, g["frames"]) and bs.geometry.scale == max(H, W, g["frames"]) / 2
        assert g["bytes"] == len(image) == seq.gop_bytes(k) and g["bpp"] == 8.0 * len(image) / (H * W * g["frames"]) and g["fit_seconds"] > 0
        assert set(g["sections"]) == {"HEAD", "MLPS", "ANCH", "MASK", "HASH", "SLAB", "PHSH"}
        total += len(image)
    assert size > total                                # the file's bpp counts the container too


def test_decode_in_a_fresh_process_verifies_every_frame(encoded, whole):
    out = str(os.path.join(os.path.dirname(encoded["file"]), "out.y4m"))
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gsvc_decode.py"), encoded["file"], "-o", out, "--strict"], cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-2500:])
    line = json.loads(run.stdout.strip().splitlines()[-1])
    assert line["frames"] == T and line["frames_verified"] == T and line["frames_mismatched"] == 0 and line["verified"] is True
    assert [(g["gop"], g["first"], g["frames"], g["frames_verified"]) for g in line["gops"]] == [(0, 0, CUT, CUT), (1, CUT, T - CUT, T - CUT)]
    hdr, frames = read_y4m(out)
    assert (hdr["W"], hdr["H"], hdr["fps"], frames.shape) == (W, H, (25, 1), (T, NB))
    # this process delivers the same bytes
    res = whole["res"]
    assert res["frames"] == T and res["verified"] and res["frames_verified"] == T and res["mismatched"] == [] and res["hashes"].shape == (T, 3)
    assert np.array_equal(whole["frames"], frames)
    # and frames 8 .. 15 are GOP 1 decoded on its own, as the bitstream file it is
    alone = _Keep()
    one = B.decode_video(S.open_sequence(encoded["file"]).gop(1), alone, fmt=FMT, strict=True)
    assert one["frames_verified"] == T - CUT and np.array_equal(np.stack(alone.rows), frames[CUT:])
    assert np.array_equal(res["hashes"][CUT:], one["hashes"])


def test_random_access_decodes_three_frames_and_builds_one_gop(encoded, whole, capsys):
    import gsvc_decode
    out = str(os.path.join(os.path.dirname(encoded["file"]), "part.y4m"))
    capsys.readouterr()
    assert gsvc_decode.main([encoded["file"], "-o", out, "--strict", "--frames", "10:13"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["frames"] == 3 and line["frames_verified"] == 3 and line["frames_mismatched"] == 0 and line["verified"] is True
    assert [(g["gop"], g["first"], g["decoded"]) for g in line["gops"]] == [(1, CUT, 3)]          # GOP 0 was never read or built
    frames = read_y4m(out)[1]
    assert frames.shape == (3, NB) and np.array_equal(frames, whole["frames"][10:13])
    # a range over the boundary takes both GOPs and hands on only those frames of each.  Frame 8 is the case that matters: rendered
    # as a batch of ONE, the first frame of GOP 1 differs from its render inside the batch of eight in the last bits of thousands of
    # float samples (measured; now and then one 8-bit code flips), so a part of a GOP is rendered in the whole decode's batches
    sink = _Keep()
    res = S.decode_sequence(encoded["file"], sink, frames=(6, 9), strict=True)
    assert [(g["gop"], g["decoded"], g["rendered"]) for g in res["gops"]] == [(0, 2, 8), (1, 1, 8)] and res["frames_verified"] == 3
    assert np.array_equal(np.stack(sink.rows), whole["frames"][6:9])
    sink = _Keep()
    res = S.decode_sequence(encoded["file"], sink, frames=(10, 13), batch=2, verify=False)          # the caller's batch is the caller's choice
    assert [(g["gop"], g["decoded"], g["rendered"]) for g in res["gops"]] == [(1, 3, 4)] and len(sink.rows) == 3
    with pytest.raises(ValueError, match="frames"):
        S.decode_sequence(encoded["file"], _Keep(), frames=(9, 17))


def test_damage_is_named_by_gop_and_by_global_frame(encoded, tmp_path, capsys):
    import gsvc_decode
    seq = S.open_sequence(encoded["file"])
    blob = bytearray(open(encoded["file"], "rb").read())
    offset = seq._entries[1][1]
    assert bytes(blob[offset:offset + 4]) == b"GSVC"
    blob[offset + seq.gop_bytes(1) // 2] ^= 0x01
    bad = tmp_path / "bad.gsvs"
    bad.write_bytes(bytes(blob))
    capsys.readouterr()
    assert gsvc_decode.main([str(bad), "-o", str(tmp_path / "bad.y4m"), "--strict"]) != 0
    assert "GOPU[1]" in capsys.readouterr().err
    with pytest.raises(B.BitstreamError) as e:
        S.decode_sequence(str(bad), B.NullSink())
    assert e.value.section == "GOPU[1]"
    # an edited picture hash of global frame 13 = frame 5 of GOP 1 (with_hashes writes the section's CRC, write_sequence the GOP's)
    images = [seq.gop_image(0), seq.gop_image(1)]
    bs = B.parse_bitstream(images[1])
    hashes = bs.hashes.copy()
    hashes[13 - CUT, 1] ^= np.uint64(1)
    edited = tmp_path / "edited.gsvs"
    S.write_sequence(edited, [images[0], B.with_hashes(images[1], bs.hash_format, hashes)], W, H, (25, 1), seq.cuts)
    res = S.decode_sequence(str(edited), B.NullSink())
    assert res["verified"] and res["frames_mismatched"] == 1 and res["mismatched"] == [13] and res["frames_verified"] == T - 1
    assert [g["frames_verified"] for g in res["gops"]] == [CUT, T - CUT - 1]
    with pytest.raises(B.BitstreamError, match=r"\[13\]") as e:
        S.decode_sequence(str(edited), B.NullSink(), strict=True)
    assert e.value.section == "PHSH"
    assert gsvc_decode.main([str(edited), "-o", str(tmp_path / "edited.y4m"), "--strict"]) != 0
    assert "[13]" in capsys.readouterr().err


def test_fixed_gop_length_and_the_plain_file(clip, encoded):
    import gsvc_encode
    fixed = str(clip["tmp"] / "fixed.gsvs")
    log = gsvc_encode.main([clip["path"], "-o", fixed, "--gop-frames", "8"] + FIT)
    seq = S.open_sequence(fixed)
    assert seq.gops == [(0, 8), (8, 8)] == S.open_sequence(encoded["file"]).gops and seq.cuts == [0, 0] and log["scene_cuts"] is None
    assert [g["cut"] for g in log["gops"]] == [0, 0] and all(seq.gop(k).hashes is not None for k in range(2))
    # without --gop-frames: today's file, which also opens as a sequence of one
    plain = str(clip["tmp"] / "plain.gsvc")
    log = gsvc_encode.main([clip["path"], "-o", plain] + FIT)
    assert open(plain, "rb").read(4) == b"GSVC" and "gops" not in log and log["total_bytes"] == os.path.getsize(plain)
    assert B.read_bitstream(plain).header["frames"] == T
    one = S.open_sequence(plain)
    assert one.gops == [(0, T)] and one.gop_bytes(0) == os.path.getsize(plain)
    res = S.decode_sequence(plain, B.NullSink(), strict=True)
    assert res["frames_verified"] == T and [g["gop"] for g in res["gops"]] == [0]
