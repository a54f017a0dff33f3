"""What an encode is asked to do, stated once: ``EncodeOptions``, the record ``fit_setup.encode_gop`` takes, and what tools/gsvc_encode.py
and tools/fit_synthetic.py share of their command lines (``add_fit_arguments``, ``check_fit_arguments``, ``options_from_args``,
``parse_frame_format``).  A default lives in the record alone: the parsers leave a dependent option None when it was not given, and
``options_from_args`` then does not pass the field.  Importing this module needs neither torch nor the built library."""
from __future__ import annotations

import dataclasses


@dataclasses.dataclass(frozen=True)
class EncodeOptions:
    """The keywords of ``fit_setup.encode_gop``.  The rules that need no file are checked when the record is made (``ValueError``)."""
    steps: int = 2000                      # iterations of the fit; the reference's 40 000-iteration schedule is scaled to them
    lmbda: float = 0.004                   # weight of the rate in the loss
    anchors: int = 100_000                 # initial points, before the voxel merge of ``create_from_points``
    slab_frames: float = 16.0              # z-slab of a render in frames (2 x threshold x scale)
    densify_grad_threshold: float = None   # None: the reference's 5e-4
    estimate_flow: bool = False            # estimate the optical flow from the frames the fit sees (``flow.EstimatedFlowCube``)
    flow_dir: str = None                   # optical-flow files, one per frame pair, at the source's size; neither: optical_lambda = 0
    video_size: tuple = (None, None)       # (W, H) of a raw video file
    video_format: object = None            # FrameFormat of a raw video file (a .y4m file's own layout, depth and range win)
    hash_format: object = None             # FrameFormat whose picture hashes the file carries (PHSH); None: yuv420p
    loss_domain: str = "rgb"               # where the fit takes its distortion (``OptimizationParams.loss_domain``); the file is the same
    init: str = "uniform"                  # where the first anchors are drawn: "uniform" in the cube, "detail" where the luma has detail
    init_cell: int = 8                     # init="detail": the cell of the detail map in pixels (a starting value, not measured)
    init_mix: float = 0.25                 # init="detail": the share of the points still drawn uniformly (likewise)
    distortion: str = "ssim"               # the structural term: "ssim" or "ms_ssim" (``OptimizationParams.distortion``)
    film_grain: bool = False               # measure the grain the fit removed against the ORIGINAL source and ship it (section GRAN)
    grain_gain: float = 1.0                # scales the fitted grain strengths (``grain.fit_grain``)
    grain_seed: int = None                 # the 64-bit grain seed; None: derived from the file image as it stands when the grain is fitted
    grain_flat_threshold: int = None       # the two rejection thresholds of ``grain.grain_stats``; None: its defaults
    grain_max_residual: int = None
    denoise: object = None                 # "auto" or a noise sigma in codes: fit the motion-compensated temporally filtered frames
    denoise_gain: float = 1.0              # scales the prefilter's strength (``tfilter.denoise_range``)
    coded_size: tuple = None               # (Wc, Hc): fit the source resampled to this size (after ``denoise``); the file says DISP
    weighting: str = None                  # "activity": weight the distortion per cell by the activity of the frames the fit sees
    weight_strength: float = 0.5           # of the activity map: > 0 moves weight to flat cells (a starting value, not measured)
    weight_cell: int = None                # the cell of the weight maps in pixels; None: 8
    roi: list = None                       # [(x, y, w, h, weight), ...] in the SOURCE's pixels, over a base of 1
    weight_file: str = None                # a .npy of weights [Hc, Wc] or [frames, Hc, Wc] of the frames the fit sees

    def __post_init__(self):
        if self.coded_size is not None:
            try:
                pair = len(self.frame_size) == 2
            except (TypeError, ValueError):
                pair = False
            if not pair:
                raise ValueError(f"encode_gop: coded_size must be (W, H) (got {self.coded_size!r})")
            if self.flow_dir is not None:
                raise ValueError("encode_gop: the flows of flow_dir are at the source's size; with coded_size use estimate_flow")
            if self.film_grain:
                raise ValueError("encode_gop: film_grain with coded_size is not supported (the grain would be measured at one size and "
                                 "synthesised at another)")
        if self.weighted and self.loss_domain != "rgb":          # (what ``loss_utils.StepDistortion`` refuses, before a file is read)
            raise ValueError(f"weight maps are taken on RGB pictures only: loss_domain must be 'rgb' (got {self.loss_domain!r}); the "
                             f"weighted plane terms of the yuv domains do not exist")
        if self.weighted and self.distortion != "ssim":
            raise ValueError(f"weight maps go with distortion 'ssim' only (got {self.distortion!r}): a weighted MS-SSIM does not exist")

    @property
    def weighted(self) -> bool:
        """Whether anything asks for a spatially weighted distortion."""
        return self.weighting is not None or bool(self.roi) or self.weight_file is not None

    @property
    def frame_size(self):
        """``coded_size`` as two ints; None without."""
        return None if self.coded_size is None else tuple(int(v) for v in self.coded_size)

    def init_log(self) -> dict:
        """What a log says of the first anchors: "init", and with init="detail" "init_cell" and "init_mix"."""
        return {"init": self.init, **({"init_cell": int(self.init_cell), "init_mix": float(self.init_mix)} if self.init == "detail" else {})}

    def new_fit_keywords(self, roi_base_hw=None) -> dict:
        """The keywords of ``fit_setup.new_fit`` that are options; ``roi_base_hw``: the size the rectangles of ``roi`` are given in."""
        names = ("init", "init_cell", "init_mix", "weighting", "weight_strength", "weight_cell", "roi", "weight_file")
        return dict({k: getattr(self, k) for k in names}, roi_base_hw=roi_base_hw)


def parse_frame_format(text):
    """LAYOUT[,MATRIX[,RANGE]] -> FrameFormat; LAYOUT in ffmpeg's spelling (yuv420p, yuv444p10le, rgb24, ...)."""
    from .frames_out import FrameFormat
    name, *rest = text.split(",")
    if len(rest) > 2:
        raise SystemExit(f"a frame format is LAYOUT[,MATRIX[,RANGE]] (got {text!r})")
    return FrameFormat.from_name(name, **dict(zip(("matrix", "range"), rest)))


def add_fit_arguments(ap):
    """Declare the options tools/gsvc_encode.py and tools/fit_synthetic.py share.  A dependent option (one that needs another) defaults
    to None = not given; ``check_fit_arguments`` holds the rules between them."""
    from .resample import parse_size          # (the one reader of a WxH option; like the next two it needs neither torch nor the library)
    from .tfilter import parse_sigma          # ({auto,SIGMA})
    from .wdist import parse_roi              # (X,Y,W,H:WEIGHT)
    D = EncodeOptions
    ap.add_argument("--steps", type=int, default=D.steps)
    ap.add_argument("--lmbda", type=float, default=D.lmbda)
    ap.add_argument("--anchors", type=int, default=D.anchors)
    ap.add_argument("--slab-frames", type=float, default=D.slab_frames, help="z-slab of a render in frames (2 x threshold x scale)")
    ap.add_argument("--densify-grad-threshold", type=float, default=None, help="default: the reference's 5e-4")
    ap.add_argument("--video-size", type=parse_size, default=None, metavar="WxH", help="frame size of a raw video file")
    ap.add_argument("--video-format", default=None, metavar="LAYOUT[,MATRIX[,RANGE]]",
                    help="e.g. yuv420p,bt601,full or yuv420p10le (default: yuv420p,bt709,limited; rgb24 for .rgb; a .y4m file's own layout, "
                         "depth and range win)")
    ap.add_argument("--estimate-flow", action="store_true", help="estimate the optical flow from the frames (gsvc_amd.flow.EstimatedFlowCube)")
    ap.add_argument("--flow-dir", default=None, metavar="DIR", help="optical-flow files of the video, one per frame pair (none: optical_lambda = 0)")
    ap.add_argument("--loss-domain", choices=("rgb", "yuv420", "yuv444"), default=D.loss_domain,
                    help="where the fit takes its distortion: float RGB, or Y'CbCr planes (gsvc_amd/yuv_loss.py): those of a Y'CbCr video "
                         "file's sample codes, else the transform of the RGB pictures")
    ap.add_argument("--distortion", choices=("ssim", "ms_ssim"), default=D.distortion,
                    help="the structural term of the fit's distortion: single-scale SSIM, or MS-SSIM as the metrics report it (rgb "
                         "domain, sides above 160 pixels)")
    ap.add_argument("--init", choices=("uniform", "detail"), default=D.init,
                    help="where the first anchors are drawn: uniformly in the cube, or where the luma has detail (gsvc_amd/detail.py)")
    ap.add_argument("--init-cell", type=int, choices=(4, 8, 16), default=None, help="with --init detail: the cell of the detail map in pixels (default 8)")
    ap.add_argument("--init-mix", type=float, default=None, metavar="X",
                    help="with --init detail: the share of the points that is still drawn uniformly, 0 .. 1 (default 0.25)")
    ap.add_argument("--denoise", type=parse_sigma, default=None, metavar="{auto,SIGMA}",
                    help="fit a motion-compensated temporally filtered video file (gsvc_amd/tfilter.py): 'auto' estimates the noise (per GOP), "
                         "a number gives its sigma in codes; YUV sources only.  Grain and metrics are still taken against the original source")
    ap.add_argument("--denoise-gain", type=float, default=None, metavar="X", help="with --denoise: scale the filter's strength (default 1.0)")
    ap.add_argument("--weighting", choices=("activity",), default=None,
                    help="weight the fit's distortion per cell by the clip's activity (gsvc_amd/wdist.py; per GOP); rgb loss domain and "
                         "--distortion ssim only, YUV sources only")
    ap.add_argument("--weight-strength", type=float, default=None, metavar="S",
                    help="with --weighting activity: > 0 moves weight to flat cells, < 0 to detail (default 0.5: a starting value, not measured)")
    ap.add_argument("--weight-cell", type=int, choices=(4, 8, 16), default=None, help="the cell of the weight maps in pixels (default 8)")
    ap.add_argument("--roi", action="append", type=parse_roi, default=None, metavar="X,Y,W,H:WEIGHT",
                    help="a rectangle in the source's pixels with this weight over a base of 1 (repeatable; later ones override earlier ones)")
    ap.add_argument("--weight-map", default=None, metavar="FILE.npy",
                    help="weights [Hc, Wc] or [frames, Hc, Wc] at --weight-cell of the frames the fit sees; multiplies with the other sources")
    ap.add_argument("--film-grain", action="store_true",
                    help="with a Y'CbCr video file: measure the grain the fit removed against the file's codes and ship its parameters "
                         "(section GRAN; gsvc_amd/grain.py)")


def check_fit_arguments(ap, args):
    """The rules between the options of ``add_fit_arguments`` (``ap.error``: exit code 2); sets ``args.weighted``."""
    args.weighted = args.weighting is not None or bool(args.roi) or args.weight_map is not None
    if args.weight_strength is not None and args.weighting is None:
        ap.error("--weight-strength needs --weighting activity")
    if args.weight_cell is not None and not args.weighted:
        ap.error("--weight-cell needs --weighting, --roi or --weight-map")
    if args.weighted and (args.loss_domain != "rgb" or args.distortion != "ssim"):
        ap.error("weighted distortion needs --loss-domain rgb and --distortion ssim")
    if args.denoise is None and args.denoise_gain is not None:
        ap.error("--denoise-gain needs --denoise")
    if args.init != "detail" and (args.init_cell is not None or args.init_mix is not None):
        ap.error("--init-cell and --init-mix need --init detail")
    if args.init_mix is not None and not 0.0 <= args.init_mix <= 1.0:
        ap.error("--init-mix must lie in 0 .. 1")


RENAMED = {"grain_gain": "film_grain_gain", "grain_seed": "film_grain_seed", "weight_file": "weight_map"}          # field: option


def options_from_args(args) -> EncodeOptions:
    """The record of a parsed command line.  A field whose option the tool does not have, or that was not given (None), is not passed:
    its default is the record's."""
    given = {f.name: getattr(args, RENAMED.get(f.name, f.name), None) for f in dataclasses.fields(EncodeOptions)}
    for name in ("video_format", "hash_format"):
        given[name] = given[name] and parse_frame_format(given[name])
    return EncodeOptions(**{k: v for k, v in given.items() if v is not None})
