"""Flag + YAML surface of the sampling path.

Mirrors the reference's ``utils/config.py:8-49``: the same flags, the same
``type=bool`` quirk (any non-empty string is True), YAML read from
``./config/<name>.yml`` relative to the cwd, and ``CONFIG_NAME`` attached.
``sys.argv`` and the cwd are part of the API there (constructors re-parse);
``parse_config_args(argv)`` additionally accepts an explicit argv so tests and
the bench need not mutate ``sys.argv``.
"""
import argparse
import os
from types import SimpleNamespace

import yaml

_CONFIG_DIRS = ["./config", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config")]


def load_config(config_name):
    for d in _CONFIG_DIRS:
        path = os.path.join(d, config_name + ".yml")
        if os.path.exists(path):
            break
    else:
        raise FileNotFoundError(os.path.join("./config", config_name + ".yml"))
    with open(path, "r") as stream:
        data = yaml.safe_load(stream)
    cfg = SimpleNamespace(**data)
    cfg.CONFIG_NAME = config_name
    return cfg


def remove_config_index(config_name):
    if config_name[-1].isdigit():
        config_name = config_name[:config_name.rfind("_")]
    return config_name


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--dataset", type=str, required=True)
    p.add_argument("--save_best", type=bool, default=False)
    p.add_argument("--folder", type=str, default=None)
    p.add_argument("--config", type=str, required=True)
    p.add_argument("--resume", type=bool, default=False)
    p.add_argument("--debug", type=bool, default=False)
    p.add_argument("--flip", type=bool, default=False)
    p.add_argument("--pred_frames", type=int, default=1)
    p.add_argument("--show", type=bool, default=False)
    p.add_argument("--old_name", type=str, default="old_name_default")
    p.add_argument("--fullscreen", type=bool, default=False)
    p.add_argument("--save_output", type=bool, default=False)
    p.add_argument("--index", type=int, default=0)
    p.add_argument("--denoise", type=bool, default=False)
    p.add_argument("--mode", type=str, default="")
    p.add_argument("--denoise_start_step", type=int, default=40)
    # the denoising loop's sampler and schedule length (num_inference_steps, hard-coded to 50 in the reference's predict loop)
    p.add_argument("--sampler", type=str, default="ddim", choices=("ddim", "dpmpp_2m"))
    p.add_argument("--denoise_steps", type=int, default=50)
    # prediction.predict: hold each clip's last --pred_frames frames out as targets and report PSNR / SSIM per predicted step
    p.add_argument("--eval_holdout", type=bool, default=False)
    # the trainer's optimizer step (all off by default: the reference's optim.Adam(lr) on every batch)
    p.add_argument("--grad_accum", type=int, default=1)              # batches whose gradients are summed per optimizer step
    p.add_argument("--clip_grad_norm", type=float, default=0.0)      # global gradient 2-norm bound, 0: no clipping
    p.add_argument("--weight_decay", type=float, default=0.0)
    p.add_argument("--optimizer", type=str, default="adam", choices=("adam", "adamw"))
    # the run around the optimizer (all off by default): learning-rate schedule, averaged weights, the training-state file
    p.add_argument("--lr_schedule", type=str, default="none", choices=("none", "linear", "cosine"))
    p.add_argument("--warmup_steps", type=int, default=0)            # optimizer steps of linear warm-up from 0
    p.add_argument("--ema_decay", type=float, default=0.0)           # 0: no averaged weights; else <stem>_ema.pt beside <stem>_test.pt
    p.add_argument("--save_state", type=bool, default=False)         # <stem>_state.pt after every epoch: what --old_state continues from
    p.add_argument("--old_state", type=str, default=None)            # with --resume True --old_name: ./checkpoints/<old_state>.pt
    return p


_OVERRIDE = None


def set_args(argv):
    """Pin the argv every later ``parse_config_args()`` sees (None = sys.argv)."""
    global _OVERRIDE
    _OVERRIDE = list(argv) if argv is not None else None


def parse_config_args(argv=None):
    if argv is None:
        argv = _OVERRIDE
    args = build_parser().parse_args(argv)
    if args.old_state and not args.resume:
        raise ValueError("--old_state continues a run whose weights --resume True --old_name NAME loads: it needs --resume True")
    return load_config(args.config), args
