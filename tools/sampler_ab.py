"""DPM++(2M) against DDIM on the GPU: the per-step time of the denoising loop at the headline shape (28 clips, 64x64
latents, guidance 0 and 7.5), and sample_clips(denoise=True, start_step=0) frames/s at 20 DPM++ against 50 DDIM steps.  The two
samplers alternate in one process; prints one JSON line per measurement.  usage (repository root): python3 tools/sampler_ab.py"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from sd_video_gen_amd import config as svg_config  # noqa: E402
from sd_video_gen_amd.sd_utils import SDUtils  # noqa: E402
from sd_video_gen_amd.transformer import Transformer  # noqa: E402
from sd_video_gen_amd.predict import sample_clips, bouncing_ball_clips  # noqa: E402

cfgname = "1_16_kitti_L1_64"
svg_config.set_args(["--dataset", "synthetic-ball", "--config", cfgname, "--denoise", "True"])
cfg = svg_config.load_config(cfgname)
torch.manual_seed(0)
sdu = SDUtils(weights="synthetic", seed=0, verbose=False, dtype="fp16")
ctx = sdu.ctx
C = 28
g = torch.Generator(device="cuda").manual_seed(1)
z = torch.randn(C, 4, 64, 64, generator=g, device="cuda") * 0.5
noise = torch.randn(C, 4, 64, 64, generator=g, device="cuda")
e1 = sdu.encode_text([""])
emb = torch.cat([e1[:1].repeat(C, 1, 1), e1[1:].repeat(C, 1, 1)])
side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
res = {"loop_per_step_ms": {}, "sample_clips": {}}
S0, NS = 40, 50          # 10 steps per timed loop (the 2nd is captured, 3..10 replay)
with torch.cuda.stream(side):
    for gd in (0.0, 7.5):
        for smp in ("ddim", "dpmpp_2m"):      # warm-up + planning
            ctx.sample_loop(z, emb, sampler=smp, num_steps=NS, start_step=S0, guidance=gd, noise=noise)
        side.synchronize()
        t = {"ddim": [], "dpmpp_2m": []}
        for rep in range(6):
            for smp in (("ddim", "dpmpp_2m") if rep % 2 == 0 else ("dpmpp_2m", "ddim")):
                side.synchronize()
                t0 = time.perf_counter()
                ctx.sample_loop(z, emb, sampler=smp, num_steps=NS, start_step=S0, guidance=gd, noise=noise)
                side.synchronize()
                t[smp].append((time.perf_counter() - t0) * 1e3 / (NS - S0))
        res["loop_per_step_ms"]["guidance_%g" % gd] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}
                                                       for k, v in t.items()}
        print(json.dumps(res["loop_per_step_ms"]["guidance_%g" % gd]), flush=True)
    # frames/s of sample_clips(denoise, start_step 0): 20 DPM++ steps vs 50 DDIM steps, one stream group of the headline (28 clips)
    torch.manual_seed(0)
    model = Transformer(num_tokens=0, dim_model=cfg.DIM_MODEL[0], num_heads=cfg.NUM_HEADS[0], num_encoder_layers=cfg.NUM_ENCODER_LAYERS[0],
                        num_decoder_layers=cfg.NUM_DECODER_LAYERS[0], dropout_p=cfg.DROPOUT_P[0]).eval()
    clips = bouncing_ball_clips(C, cfg.FRAME_SIZE, 5, seed=0, device="cuda")
    seeds = list(range(C))
    runs = {"ddim_50": dict(sampler="ddim", num_inference_steps=50), "dpmpp_2m_20": dict(sampler="dpmpp_2m", num_inference_steps=20)}
    for k, kw in runs.items():
        sample_clips(model, sdu, clips, 1, denoise=True, start_step=0, seeds=seeds, text_embeddings=e1, **kw)
    side.synchronize()
    t = {k: [] for k in runs}
    for rep in range(3):
        for k in (list(runs) if rep % 2 == 0 else list(runs)[::-1]):
            side.synchronize()
            t0 = time.perf_counter()
            sample_clips(model, sdu, clips, 1, denoise=True, start_step=0, seeds=seeds, text_embeddings=e1, **runs[k])
            side.synchronize()
            t[k].append(C / (time.perf_counter() - t0))
    res["sample_clips"] = {k: {"frames_per_s_median": statistics.median(v), "min": min(v), "max": max(v), "all": v} for k, v in t.items()}
    res["sample_clips"]["shape"] = "%d clips, F=%d, 1 predicted frame, 512x512 denoise, guidance 0, start_step 0, one stream" % (C, cfg.FRAME_SIZE)
print(json.dumps(res["sample_clips"]), flush=True)
