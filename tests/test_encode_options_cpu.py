"""CPU tests of the encoder's options record (gsvc_amd/encode_options.py): its defaults, what ``encode_gop`` refuses before any file is
touched, that tools/gsvc_encode.py and tools/fit_synthetic.py read a command line into the same record, and that every rule between
options the two parsers share ends both with exit code 2."""
import dataclasses
import os
import sys

import pytest

from gsvc_amd.encode_options import EncodeOptions, options_from_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# the keywords of encode_gop behind frame_range and their defaults, as its signature had them before the record existed (28 of them)
DEFAULTS = dict(steps=2000, lmbda=0.004, anchors=100_000, slab_frames=16.0, densify_grad_threshold=None, estimate_flow=False, flow_dir=None,
                video_size=(None, None), video_format=None, hash_format=None, loss_domain="rgb", init="uniform", init_cell=8, init_mix=0.25,
                distortion="ssim", film_grain=False, grain_gain=1.0, grain_seed=None, grain_flat_threshold=None, grain_max_residual=None,
                denoise=None, denoise_gain=1.0, coded_size=None, weighting=None, weight_strength=0.5, weight_cell=None, roi=None,
                weight_file=None)
BASE = {"gsvc_encode": ["clip.y4m", "-o", "clip.gsvc"], "fit_synthetic": ["--video", "clip.y4m"]}
SHARED = [name for name in DEFAULTS if name not in ("hash_format", "coded_size", "grain_gain", "grain_seed")]          # (what both tools can set)


def test_defaults_are_those_of_the_old_signature():
    got = {f.name: f.default for f in dataclasses.fields(EncodeOptions)}
    assert got == DEFAULTS and list(got) == list(DEFAULTS)
    assert all(type(got[k]) is type(v) for k, v in DEFAULTS.items())
    assert not EncodeOptions().weighted and EncodeOptions(roi=[(0, 0, 8, 8, 2.0)]).weighted and not EncodeOptions(roi=[]).weighted
    assert EncodeOptions(weight_file="w.npy").weighted and EncodeOptions(weighting="activity").weighted
    with pytest.raises(dataclasses.FrozenInstanceError):
        EncodeOptions().steps = 1


def test_encode_gop_refuses_before_any_file_is_touched():
    from gsvc_amd.fit_setup import encode_gop
    for kw, what in ((dict(coded_size=(48,)), r"coded_size must be \(W, H\)"), (dict(coded_size=(48, 32), flow_dir="f"), "with coded_size use estimate_flow"),
                     (dict(coded_size=(48, 32), film_grain=True), "film_grain with coded_size is not supported")):
        with pytest.raises(ValueError, match=what):
            encode_gop("no_such_file.y4m", "cpu", **kw)
    with pytest.raises(TypeError, match="no_such_option"):
        encode_gop("no_such_file.y4m", "cpu", no_such_option=1)
    with pytest.raises(TypeError, match="not both"):
        encode_gop("no_such_file.y4m", "cpu", options=EncodeOptions(), steps=40)
    # weights go with the rgb domain and the single-scale SSIM only: the messages of loss_utils.StepDistortion, before the video is read
    with pytest.raises(ValueError, match="loss_domain must be 'rgb'"):
        encode_gop("no_such_file.y4m", "cpu", roi=[(0, 0, 16, 16, 2.0)], loss_domain="yuv420")
    with pytest.raises(ValueError, match="weighted MS-SSIM does not exist"):
        encode_gop("no_such_file.y4m", "cpu", weighting="activity", distortion="ms_ssim")


def test_the_two_tools_read_the_same_options():
    import fit_synthetic
    import gsvc_encode
    given = ["--init", "detail", "--weighting", "activity", "--roi", "0,0,16,16:2", "--denoise", "2.5", "--loss-domain", "rgb"]
    enc = options_from_args(gsvc_encode.parse_args(BASE["gsvc_encode"] + given))
    fit = options_from_args(fit_synthetic.parse_args(BASE["fit_synthetic"] + given))
    for name in SHARED:
        assert getattr(enc, name) == getattr(fit, name), name
    assert (enc.init, enc.weighting, enc.roi, enc.denoise, enc.loss_domain) == ("detail", "activity", [(0, 0, 16, 16, 2.0)], 2.5, "rgb")
    assert (enc.init_cell, enc.init_mix, enc.weight_strength, enc.denoise_gain) == (8, 0.25, 0.5, 1.0) and enc.weighted and fit.weighted
    assert fit.new_fit_keywords() == dict(init="detail", init_cell=8, init_mix=0.25, weighting="activity", weight_strength=0.5, weight_cell=None,
                                          roi=[(0, 0, 16, 16, 2.0)], weight_file=None, roi_base_hw=None)
    assert fit.init_log() == {"init": "detail", "init_cell": 8, "init_mix": 0.25} and EncodeOptions().init_log() == {"init": "uniform"}
    # nothing optional given: the record's own defaults (the encoder names its hash format, which is the default one)
    enc = options_from_args(gsvc_encode.parse_args(BASE["gsvc_encode"]))
    fit = options_from_args(fit_synthetic.parse_args([]))
    for name in SHARED:
        assert getattr(enc, name) == getattr(fit, name) == DEFAULTS[name], name
    assert fit == EncodeOptions() and enc.hash_format.name == "yuv420p" and dataclasses.replace(enc, hash_format=None) == EncodeOptions()
    # the options whose names differ from their fields, and the sizes
    enc = options_from_args(gsvc_encode.parse_args(BASE["gsvc_encode"] + ["--film-grain", "--film-grain-gain", "2", "--film-grain-seed", "7", "--weight-map", "w.npy",
                                                                         "--video-size", "64x48", "--video-format", "yuv420p10le"]))
    assert (enc.film_grain, enc.grain_gain, enc.grain_seed, enc.weight_file, enc.video_size) == (True, 2.0, 7, "w.npy", (64, 48))
    assert enc.video_format.depth == 10 and options_from_args(gsvc_encode.parse_args(BASE["gsvc_encode"] + ["--coded-size", "48x32"])).frame_size == (48, 32)


RULES = (["--weight-strength", "0.5"], ["--weight-cell", "8"], ["--weighting", "activity", "--loss-domain", "yuv420"],
         ["--roi", "0,0,16,16:2", "--distortion", "ms_ssim"], ["--weight-map", "w.npy", "--loss-domain", "yuv444"], ["--denoise-gain", "2"],
         ["--init-cell", "4"], ["--init-mix", "0.5"], ["--init", "uniform", "--init-cell", "8"], ["--init", "detail", "--init-mix", "1.5"],
         ["--init", "detail", "--init-mix", "-0.1"], ["--video-size", "64"], ["--video-size", "0x48"])


@pytest.mark.parametrize("tool", ["gsvc_encode", "fit_synthetic"])
def test_rules_between_options_end_both_tools_with_code_2(tool, capsys):
    mod = __import__(tool)
    for extra in RULES:
        with pytest.raises(SystemExit) as e:
            mod.parse_args(BASE[tool] + extra)
        assert e.value.code == 2, extra
        assert extra[0] in capsys.readouterr().err or extra[0] in ("--weighting", "--roi", "--weight-map"), extra
    assert mod.parse_args(BASE[tool] + ["--init", "detail", "--init-mix", "1.0", "--weighting", "activity", "--weight-cell", "16"]).weighted
