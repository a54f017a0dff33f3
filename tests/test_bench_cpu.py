"""bench.py's host-side pieces: the result line (bench.result_line), the --dump-outputs writer (bench.dump_outputs) and its options."""
import json
import os

import numpy as np

import bench


def test_dump_outputs_budget_dtypes_and_fixed_sample(tmp_path):
    rng = np.random.default_rng(1)
    arrays = {"loss": np.float32(0.5), "frame_idx": 7, "radii": rng.integers(0, 9, 500_000).astype(np.int32), "mask": np.ones(3, bool),
              "small64": rng.random((4, 4)), **{f"image{i}": rng.random((3, 1080, 1920), dtype=np.float32) for i in range(4)}}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(n + ".npy" for n in arrays)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_BYTES <= 64_000_000
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), f
    # what fits is written whole and exact: integers and booleans as float64, float64 stays float64
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "radii.npy"), arrays["radii"].astype(np.float64))
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "small64.npy"), arrays["small64"])
    assert np.load(tmp_path / "a" / "frame_idx.npy") == 7.0 and np.load(tmp_path / "a" / "loss.npy").dtype == np.float32
    # 4 x 25 MB of images do not fit: each keeps an equal share, at the sorted positions numpy.random.default_rng(0) draws
    img = np.load(tmp_path / "a" / "image0.npy")
    assert img.ndim == 1 and 1_000_000 < img.size < arrays["image0"].size
    idx = np.sort(np.random.default_rng(0).choice(arrays["image0"].size, img.size, replace=False))
    np.testing.assert_array_equal(img, arrays["image0"].reshape(-1)[idx])


def test_result_line_is_one_line_with_every_number_and_no_notes():
    res = {"metric": "m", "value": 1.5, "ms_per_step": 6.5, "steps": 20, "note": "x" * 500, "render_fps_note": "y" * 500,
           "config": {"workload": "w", "instances_note": "z", "active_per_render": 3.0},
           "flips": [{"step": 8, "note": "n"}], "side": {"error": "E: e", "kernels": {"k_blend": {"avg_us": 2.0}}}}
    line = bench.result_line(res)
    assert "\n" not in line and "note" not in line
    assert json.loads(line) == {"metric": "m", "value": 1.5, "ms_per_step": 6.5, "steps": 20, "config": {"workload": "w", "active_per_render": 3.0},
                                "flips": [{"step": 8}], "side": {"error": "E: e", "kernels": {"k_blend": {"avg_us": 2.0}}}}


def test_a_plain_run_is_lean_and_full_is_an_option():
    assert not bench.parse(["--gpus", "1", "--steps", "20", "--warmup", "5"]).full
    assert bench.parse(["--full"]).full
