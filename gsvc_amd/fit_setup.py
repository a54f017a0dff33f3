"""The set-up of a fit that tools/fit_synthetic.py and tools/gsvc_encode.py share: the reference's 40 000-iteration schedule scaled to
a run's length, and the model, its initial anchors and the Trainer on a frame cube.

The reference's schedule (pipeline/train.py:325-583: 10 k full precision / 5 k quantised / 20 k entropy-constrained / 5 k
straight-through; statistics from 500, densification 1 500 .. 25 000 every 100, paused 1 000 iterations at the first phase change) is
scaled to ``steps`` iterations with the same proportions.
"""
from __future__ import annotations

import numpy as np
import torch


def configure_fit(mp_, opt, cube, steps: int, lmbda: float, slab_frames: float, densify_grad_threshold=None):
    """Set the render slab (``mp_.threshold``: ``slab_frames`` frames thick) and scale the schedule of ``opt`` to ``steps`` iterations,
    in place."""
    N = int(steps)
    mp_.threshold = slab_frames / 2.0 / cube.scale
    s = N / 40_000.0
    opt.iterations, opt.lmbda = N, lmbda
    opt.full_precision_training_total, opt.quantized_training_total = int(10_000 * s), int(5_000 * s)
    opt.entropy_constrained_train_total = int(20_000 * s)
    opt.ste_entropy_constrained_train_total = N - int(35_000 * s)
    opt.start_stat, opt.update_from, opt.update_until = int(500 * s), int(1_500 * s), int(25_000 * s)
    opt.update_interval = max(20, int(100 * s))
    opt.pause_densification = int(1_000 * s)
    if densify_grad_threshold is not None:
        opt.densify_grad_threshold = densify_grad_threshold
    for name in dir(opt):                        # the learning-rate schedules decay over the run's length
        if name.endswith("_max_steps"):
            setattr(opt, name, N)


def new_fit(cube, mp_, opt, pipe, anchors: int, device):
    """Seed the generators, build the model of configuration ``mp_`` with ``anchors`` uniformly drawn initial points inside the cube
    (reference frame_cube/utils.py:6-15, init_point_cloud, bleed 0.1) and its Trainer -> ``(pc, trainer)``."""
    from . import dist as gdist
    from .model import GaussianModel
    from .train import Trainer
    torch.manual_seed(0)
    np.random.seed(0)
    pc = GaussianModel(mp_, mp_.anchor_feature_dim, mp_.n_offsets, mp_.voxel_size, mp_.update_depth, mp_.update_init_factor,
                       mp_.update_hierarchy_factor, mp_.use_feat_bank, n_features_per_level=mp_.grid_feature_dim,
                       log2_hashmap_size=mp_.log2, log2_hashmap_size_2D=mp_.log2_2D, device=device)
    lim = np.array([cube.x_min, cube.y_min, cube.z_min]) * 1.1
    pc.create_from_points(np.random.default_rng(0).uniform(lim, -lim, (anchors, 3)), spatial_lr_scale=1.0)
    pc.update_anchor_bound(cube.x_min, cube.y_min, cube.z_min)
    pc.training_setup(opt)
    gdist.broadcast_parameters(pc)
    trainer = Trainer(pc, cube, opt, pipe, mp_, seed=0)
    return pc, trainer
