"""The LMS text-to-image loop in the library against the host loop it replaces: ms per step of
SDUtils.denoise_img_latents at 50 steps, 64x64 latents, guidance 7.5, full-size seeded weights, N latents in one call.
Host loop = in_library=False (torch arithmetic + scipy quadrature per step), library loop = in_library=True (svg_sample_loop with
SVG_SAMPLER_LMS: fused kernels, the step captured as a graph).  The two alternate in one process; prints one JSON line.
usage (repository root): python3 tools/lms_ab.py <N>     (N = 1 and N = 8 for the DESIGN figures, one process each)"""
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

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1
STEPS, REPS = 50, 3
svg_config.set_args(["--dataset", "synthetic-ball", "--config", "1_16_kitti_L1_64", "--denoise", "True"])
torch.manual_seed(0)
sdu = SDUtils(weights="synthetic", seed=0, verbose=False, dtype="fp16")
e1 = sdu.encode_text([""])
emb = torch.cat([e1[:1].repeat(N, 1, 1), e1[1:].repeat(N, 1, 1)])
lat = torch.randn(N, 4, 64, 64, generator=torch.Generator().manual_seed(1))
side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
t = {"host": [], "library": []}
with torch.cuda.stream(side):
    for mode in t:                                 # warm-up + planning
        sdu.denoise_img_latents(emb, num_inference_steps=STEPS, guidance_scale=7.5, latents=lat.clone(), in_library=mode == "library")
    side.synchronize()
    for rep in range(REPS):
        for mode in (("host", "library") if rep % 2 == 0 else ("library", "host")):
            side.synchronize()
            t0 = time.perf_counter()
            out = sdu.denoise_img_latents(emb, num_inference_steps=STEPS, guidance_scale=7.5, latents=lat.clone(), in_library=mode == "library")
            side.synchronize()
            t[mode].append((time.perf_counter() - t0) * 1e3 / STEPS)
            assert torch.isfinite(out).all()
res = {"N": N, "steps": STEPS, "latents": "64x64", "guidance": 7.5, "device": torch.cuda.get_device_name(0),
       "ms_per_step": {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v} for k, v in t.items()}}
res["host_over_library"] = res["ms_per_step"]["host"]["median"] / res["ms_per_step"]["library"]["median"]
print(json.dumps(res), flush=True)
