#!/usr/bin/env python3
"""Device-event timings of the optimizer tail of the training step at the `bench.py --train` shape (the config's own batch):

    python tools/train_optim_bench.py [--config 1_16_kitti_L1_64] [--reps 30] [--rounds 3] [--ema] [--out FILE]

  adam            svg_transformer_adam_step (adam_kernel: 7 streams of 4 bytes per parameter)
  optim_plain     svg_transformer_optim_step without decay / clipping / scaling (adamw_kernel alone, the same 7 streams)
  adamw           ... with weight decay 0.01 (decoupled)
  adamw_clip      ... and max_grad_norm: the norm pass (4 bytes per parameter, read only) + its finish + the update
  grad_norm       svg_transformer_grad_norm, events around the call (norm pass + finish + the 8-byte copy back)
  loss_bw1 / 2    one svg_transformer_loss call with backward = 1 / SVG_BACKWARD_ACCUMULATE
  step_accum1 / 4 optimizer step over 1 / 4 micro-batches (loss calls + update), per micro-batch
  --ema adds, in the same process and the same rounds:
  adam_ema / adamw_ema / adamw_clip_ema   the same three steps with svg_transformer_ema_configure(0.999): the kernels' EMA
                  instantiation, 9 streams of 4 bytes per parameter
  lerp_pass       what an unfused EMA would add to a step: e.lerp_(p, 1 - decay) over one flat f32 tensor of the model's size
                  (torch's element-wise kernel: 3 streams of 4 bytes per parameter, no chunk table)

Every figure is the mean over `reps` enqueue-only calls between two events on the capturable side stream (the loss calls replay
their hipGraph there), after a warm-up of each shape; the rounds alternate all measurements so that the spread is visible."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="1_16_kitti_L1_64")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ema", action="store_true", help="also time the optimizer steps with averaged weights on, and a stand-alone lerp pass")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    from sd_video_gen_amd import _lib, config as svg_config
    from sd_video_gen_amd.transformer import Transformer
    svg_config.set_args(["--dataset", "synthetic-ball", "--config", args.config])
    cfg = svg_config.load_config(args.config)
    first = lambda v: v[0] if isinstance(v, (list, tuple)) else v
    torch.manual_seed(0)
    model = Transformer(num_tokens=0, dim_model=first(cfg.DIM_MODEL), num_heads=first(cfg.NUM_HEADS), num_encoder_layers=first(cfg.NUM_ENCODER_LAYERS),
                        num_decoder_layers=first(cfg.NUM_DECODER_LAYERS), dropout_p=first(cfg.DROPOUT_P)).train()
    n_par = sum(p.numel() for p in model.parameters())
    B, F = first(cfg.BATCH_SIZE), first(cfg.FRAMES_TO_PREDICT)
    T = first(cfg.FRAMES_PER_CLIP) + F + 1
    feat = cfg.FRAME_SIZE // 8
    D = 4 * feat * feat
    g = torch.Generator().manual_seed(1)
    nb = torch.cat([2.0 * torch.ones(B, 1, D), 0.8 * torch.randn(B, T - 1, D, generator=g)], dim=1).cuda()
    tc = _lib.TrainCfg(frames_to_predict=F, feat_h=feat, feat_w=feat, w_mse=float(bool(first(getattr(cfg, "USE_MSE", False)))),
                       w_l1=float(bool(first(getattr(cfg, "USE_L1", False)))),
                       w_gdl=float(bool(first(getattr(cfg, "USE_GDL", False)))) * float(first(getattr(cfg, "LAMBDA_GDL", 1))),
                       gdl_alpha=float(first(getattr(cfg, "ALPHA", 1))), w_contrastive=0.0, temperature=0.07, dropout_p=float(first(cfg.DROPOUT_P)), seed=0)
    lr = float(first(cfg.LR))
    side = torch.cuda.Stream()
    seed = [0]

    def loss(mode):
        seed[0] += 1
        tc.seed = seed[0]
        model.training_loss(tc, nb, backward=mode, read_losses=False)

    def accum(k):
        loss(1)
        for _ in range(k - 1):
            loss(2)
        if k == 1:
            model.adam_step(lr)
        else:
            model.optim_step(lr, weight_decay=0.0, grad_scale=1.0 / k)

    work = {
        "adam": (lambda: model.adam_step(lr), 1),
        "optim_plain": (lambda: model.optim_step(lr, weight_decay=0.0), 1),
        "adamw": (lambda: model.optim_step(lr, weight_decay=0.01), 1),
        "adamw_clip": (lambda: model.optim_step(lr, weight_decay=0.01, max_grad_norm=1.0), 1),
        "grad_norm": (lambda: model.grad_norm(), 1),
        "loss_bw1": (lambda: loss(1), 1),
        "loss_bw2": (lambda: loss(2), 1),
        "step_accum1": (lambda: accum(1), 1),
        "step_accum4": (lambda: accum(4), 4),
    }

    work_ema = {}
    if args.ema:
        decay = 0.999
        flat_p, flat_e = torch.randn(n_par, device="cuda"), torch.randn(n_par, device="cuda")
        work["lerp_pass"] = (lambda: flat_e.lerp_(flat_p, 1.0 - decay), 1)
        work_ema = {"adam_ema": work["adam"], "adamw_ema": work["adamw"], "adamw_clip_ema": work["adamw_clip"]}

    def ema_on(on):
        side.synchronize()
        model.ema_configure(decay if on else 0.0)       # (synchronises the device; the first call allocates the averaged weights)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):
            e0.record(side)
            for _ in range(reps):
                fn()
            e1.record(side)
        side.synchronize()
        return e0.elapsed_time(e1) / reps

    with torch.cuda.stream(side):
        loss(1)                                     # the training state and its first gradients
        for fn, _ in work.values():                 # every shape once: graph captures, code objects
            for _ in range(3):
                fn()
    side.synchronize()
    if work_ema:
        ema_on(True)
        with torch.cuda.stream(side):
            for fn, _ in work_ema.values():
                for _ in range(3):
                    fn()
        ema_on(False)
    ms = {k: [] for k in list(work) + list(work_ema)}
    for _ in range(args.rounds):
        for k, (fn, per) in work.items():
            ms[k].append(timed(fn, max(3, args.reps // per)) / per)
        if work_ema:
            ema_on(True)
            for k, (fn, per) in work_ema.items():
                ms[k].append(timed(fn, max(3, args.reps // per)) / per)
            ema_on(False)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    gb = n_par * 4 / 1e9
    rec = {"config": args.config, "parameters": n_par, "batch": [B, T], "reps": args.reps, "library": _lib.source_hash(),
           "ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "median_ms": {k: round(v, 4) for k, v in med.items()},
           "gradient_bytes_GB": gb,
           "adam_TBps": 7 * gb / med["adam"], "optim_plain_TBps": 7 * gb / med["optim_plain"], "adamw_TBps": 7 * gb / med["adamw"],
           "norm_pass_ms_by_difference": med["adamw_clip"] - med["adamw"], "norm_pass_TBps_by_difference": gb / max(med["adamw_clip"] - med["adamw"], 1e-9),
           "grad_norm_call_TBps": gb / med["grad_norm"],
           "accumulate_extra_ms": med["loss_bw2"] - med["loss_bw1"]}
    if args.ema:
        spread = lambda k: (max(ms[k]) - min(ms[k])) / med[k]
        rec.update({"ema_decay": decay, "adam_ema_TBps": 9 * gb / med["adam_ema"], "adamw_ema_TBps": 9 * gb / med["adamw_ema"],
                    "lerp_pass_TBps": 3 * gb / med["lerp_pass"],
                    "fused_ema_extra_ms": {"adam": med["adam_ema"] - med["adam"], "adamw": med["adamw_ema"] - med["adamw"]},
                    "unfused_sum_ms": {"adam": med["adam"] + med["lerp_pass"], "adamw": med["adamw"] + med["lerp_pass"]},
                    "fused_not_slower_than_unfused": {"adam": med["adam_ema"] <= med["adam"] + med["lerp_pass"],
                                                      "adamw": med["adamw_ema"] <= med["adamw"] + med["lerp_pass"]},
                    "round_spread_rel": {k: round(spread(k), 4) for k in ("adam", "adamw", "adam_ema", "adamw_ema", "lerp_pass")}})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
