"""GPU: svg_frame_metrics (csrc/metrics.hip) against the fp64 judge of frame_metrics_judge.py, element by element, and the hold-out
protocol built on it (metrics.evaluate_holdout, `prediction.predict --eval_holdout`).

Per input kind, over the shapes of frame_metrics_judge.SHAPES — one valid position (11x11), a 363-byte image stride (3x11x11), 39-byte rows
(12x13), exactly one 32x32 tile (42x42), one column over a tile (27x43), 43x75, the project's frame sizes 64^2 and 128^2, a non-square
several-tile image (96x160): the squared error equals numpy's integer sum exactly; every element of the SSIM map is within MAP_TOL = 1e-3
and every image mean within MEAN_TOL = 8e-5 of the judge (where the bounds come from: frame_metrics_judge.py and
test_frame_metrics_cpu.py); the call without a map, a repeated call, and an image alone instead of inside its batch give the same bits.

Measured on MI355X (gfx950), worst over the shapes — map element / image mean:
  uniform 1.8e-7 / 4.7e-8      identical 3.6e-7 / 4.0e-8     pm1 5.6e-7 / 1.4e-7       const255 0 / 0
  const0_255 1.7e-9 / 1.7e-9   ramp 2.7e-5 / 1.1e-5          ball 5.7e-5 / 2.2e-7
(the ramp's mean is the single-position 11x11 image, the ball's map the 128x128 frames); each figure goes to parity_margins.json.
"""
import math

import numpy as np
import pytest
import torch

import frame_metrics_judge as J
from conftest import margin

pytestmark = pytest.mark.gpu

_REF = {}


def reference(kind, N, H, W):
    """(a, b, sse, ssim, map) of one case: the inputs and the judge's answer, computed once and never written to"""
    key = (kind, N, H, W)
    if key not in _REF:
        a, b = J.make_pair(kind, N, H, W)
        _REF[key] = (a, b) + J.judge(a, b)
        for x in _REF[key]:
            x.setflags(write=False)
    return _REF[key]


def bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


@pytest.mark.parametrize("kind", J.KINDS)
def test_kernel_against_fp64_judge(ctx, kind):
    from sd_video_gen_amd import metrics
    worst_map, worst_mean = 0.0, 0.0
    for (N, H, W) in J.SHAPES:
        if kind == "ball" and (H != W or H not in (64, 128)):
            continue
        a, b, sse_ref, ssim_ref, map_ref = reference(kind, N, H, W)
        ta, tb = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(b.copy()).cuda()
        sse, ssim, smap = ctx.frame_metrics(ta, tb, return_map=True)
        what = "%s %dx%dx%d" % (kind, N, H, W)
        assert sse.dtype == torch.int64 and ssim.dtype == torch.float64 and smap.dtype == torch.float32
        assert smap.shape == (N, H - 10, W - 10, 3)
        assert np.array_equal(sse.cpu().numpy(), sse_ref), what                                        # exact integer arithmetic
        e_map = float(np.abs(smap.cpu().numpy().astype(np.float64) - map_ref).max())                   # every element, none excluded
        e_mean = float(np.abs(ssim.cpu().numpy() - ssim_ref).max())
        print("[frame-metrics] %-24s map %.3e  mean %.3e" % (what, e_map, e_mean))
        assert e_map < J.MAP_TOL, what
        assert e_mean < J.MEAN_TOL, what
        worst_map, worst_mean = max(worst_map, e_map), max(worst_mean, e_mean)
        # without the map, and again: the same bits
        sse2, ssim2 = ctx.frame_metrics(ta, tb)
        assert torch.equal(sse2, sse) and torch.equal(bits(ssim2), bits(ssim)), what
        sse3, ssim3, smap3 = ctx.frame_metrics(ta, tb, return_map=True)
        assert torch.equal(sse3, sse) and torch.equal(bits(ssim3), bits(ssim)) and torch.equal(smap3.view(torch.int32), smap.view(torch.int32)), what
        # image n alone (its own allocation: another base address) instead of inside the batch
        for n in range(N if N > 1 else 0):
            s1, m1, p1 = ctx.frame_metrics(ta[n:n + 1].clone(), tb[n:n + 1].clone(), return_map=True)
            assert torch.equal(s1, sse[n:n + 1]) and torch.equal(bits(m1), bits(ssim[n:n + 1])), what
            assert torch.equal(p1.view(torch.int32), smap[n:n + 1].view(torch.int32)), what
        # the Python surface on top: mse and psnr are host arithmetic on the exact integer
        res = metrics.frame_metrics(ta, tb, ctx=ctx)
        assert torch.equal(res["sse"], sse) and torch.equal(bits(res["ssim"]), bits(ssim))
        np.testing.assert_allclose(res["mse"].cpu().numpy(), sse_ref / float(H * W * 3), rtol=1e-15)
        if kind in ("identical", "const255"):
            assert (sse == 0).all() and torch.isinf(res["psnr"]).all() and (res["psnr"] > 0).all(), what
            assert float((ssim - 1.0).abs().max()) < J.MEAN_TOL, what
        else:
            want = 10.0 * np.log10(255.0 ** 2 / (sse_ref / float(H * W * 3)))
            np.testing.assert_allclose(res["psnr"].cpu().numpy(), want, rtol=1e-12, atol=1e-12)      # (0 dB for 0 against 255)
    margin("frame_metrics %s: worst SSIM map element vs fp64" % kind, worst_map, J.MAP_TOL, unit="max-abs")
    margin("frame_metrics %s: worst image-mean SSIM vs fp64" % kind, worst_mean, J.MEAN_TOL, unit="max-abs")


def test_odd_base_address_and_leading_dimensions(ctx):
    """a stack that starts at an odd byte address, and (C, P, H, W, 3) leading dimensions through metrics.frame_metrics"""
    from sd_video_gen_amd import metrics
    a, b, sse_ref, ssim_ref, map_ref = reference("uniform", 2, 27, 43)
    n = a.size
    for off in (1, 2, 3):
        bufa, bufb = torch.zeros(n + 8, dtype=torch.uint8, device="cuda"), torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
        ta, tb = bufa[off:off + n].view(a.shape), bufb[off + 1:off + 1 + n].view(b.shape)
        ta.copy_(torch.from_numpy(a.copy()))
        tb.copy_(torch.from_numpy(b.copy()))
        assert ta.data_ptr() % 4 == off and ta.is_contiguous()
        sse, ssim, smap = ctx.frame_metrics(ta, tb, return_map=True)
        assert np.array_equal(sse.cpu().numpy(), sse_ref)
        assert np.abs(smap.cpu().numpy().astype(np.float64) - map_ref).max() < J.MAP_TOL
        assert np.abs(ssim.cpu().numpy() - ssim_ref).max() < J.MEAN_TOL
    res = metrics.frame_metrics(a.copy().reshape(2, 1, 27, 43, 3), b.copy().reshape(2, 1, 27, 43, 3), ctx=ctx, return_map=True)
    assert res["sse"].shape == (2, 1) and res["ssim"].shape == (2, 1) and res["psnr"].shape == (2, 1) and res["mse"].shape == (2, 1)
    assert res["ssim_map"].shape == (2, 1, 17, 33, 3)
    assert np.array_equal(res["sse"].cpu().numpy().reshape(2), sse_ref)


def test_workspace_is_planned_and_a_second_call_grows_nothing():
    from sd_video_gen_amd import _lib
    c = _lib.Context(0)
    try:
        a = torch.randint(0, 256, (3, 96, 160, 3), dtype=torch.uint8, device="cuda")
        b = torch.randint(0, 256, (3, 96, 160, 3), dtype=torch.uint8, device="cuda")
        g0 = c.workspace_growths()
        first = c.frame_metrics(a, b)
        g1 = c.workspace_growths()
        assert g1 == g0 + 1 and c.workspace_bytes() >= 3 * 3 * 5 * 12          # the [N][tiles] partials came from the arena
        second = c.frame_metrics(a, b)
        assert c.workspace_growths() == g1
        assert torch.equal(first[0], second[0]) and torch.equal(bits(first[1]), bits(second[1]))
        # the call takes part in svg_plan_begin .. svg_plan_end: a batch whose partials (12 bytes per image and tile) exceed the arena is
        # only measured there — nothing is launched, so the outputs keep their values — and the arena is sized once when the plan ends
        sse = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        ssim = torch.full((1,), -7.0, dtype=torch.float64, device="cuda")
        n_big = 400000
        assert n_big * 12 > c.workspace_bytes()
        with c.planning() as plan:
            c.check(c.lib.svg_frame_metrics(c.h, a.data_ptr(), b.data_ptr(), n_big, 42, 42, sse.data_ptr(), ssim.data_ptr(), None,
                                            torch.cuda.current_stream().cuda_stream), "svg_frame_metrics")
            assert c.workspace_growths() == g1
        torch.cuda.synchronize()
        assert int(sse[0]) == -7 and float(ssim[0]) == -7.0
        assert plan.bytes >= n_big * 12 and c.workspace_bytes() >= plan.bytes and c.workspace_growths() == g1 + 1
        third = c.frame_metrics(a, b)
        assert c.workspace_growths() == g1 + 1
        assert torch.equal(first[0], third[0]) and torch.equal(bits(first[1]), bits(third[1]))
    finally:
        c.close()


def test_library_rejects_bad_sizes_and_null_pointers(ctx):
    from sd_video_gen_amd import _lib
    ok = torch.zeros((1, 11, 11, 3), dtype=torch.uint8, device="cuda")
    for shape in ((1, 10, 16, 3), (1, 16, 10, 3), (0, 16, 16, 3)):
        bad = torch.zeros(shape, dtype=torch.uint8, device="cuda")
        with pytest.raises(ValueError, match="frame_metrics"):
            ctx.frame_metrics(bad, bad)
    sse = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    ssim = torch.full((1,), -7.0, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    f = ctx.lib.svg_frame_metrics
    p = lambda t: t.data_ptr()      # noqa: E731
    assert f(ctx.h, None, p(ok), 1, 11, 11, p(sse), p(ssim), None, s) == _lib.SVG_ERR_INVALID
    assert f(ctx.h, p(ok), None, 1, 11, 11, p(sse), p(ssim), None, s) == _lib.SVG_ERR_INVALID
    assert f(ctx.h, p(ok), p(ok), 1, 11, 11, None, p(ssim), None, s) == _lib.SVG_ERR_INVALID
    assert f(ctx.h, p(ok), p(ok), 1, 11, 11, p(sse), None, None, s) == _lib.SVG_ERR_INVALID
    assert f(None, p(ok), p(ok), 1, 11, 11, p(sse), p(ssim), None, s) == _lib.SVG_ERR_INVALID
    assert f(ctx.h, p(ok), p(ok), 1, 16385, 11, p(sse), p(ssim), None, s) == _lib.SVG_ERR_INVALID      # the stated size bound
    assert f(ctx.h, p(ok), p(ok), 1, 11, 16385, p(sse), p(ssim), None, s) == _lib.SVG_ERR_INVALID
    torch.cuda.synchronize()
    assert int(sse[0]) == -7 and float(ssim[0]) == -7.0                      # nothing was launched
    # the context is usable afterwards
    out = ctx.frame_metrics(ok, ok)
    assert int(out[0][0]) == 0 and abs(float(out[1][0]) - 1.0) < J.MEAN_TOL


VCFG = dict(block_out=(64, 128, 128, 128), layers=1, groups=32, latent=4)
UCFG = dict(block_out=(64, 128), layers=1, heads=4, ctx_dim=768, groups=32, in_ch=4, out_ch=4, attn=(1, 0))


def test_evaluate_holdout_end_to_end(ctx):
    """the wiring, not the networks: reduced networks with seeded weights, no denoise; the returned metrics are the judge applied on the
    host to the returned frames and the clips"""
    from oracle import sd_oracle as SO
    from sd_video_gen_amd import config as svg_config, metrics
    from sd_video_gen_amd.predict import bouncing_ball_clips
    from sd_video_gen_amd.sd_utils import SDUtils
    from sd_video_gen_amd.transformer import Transformer
    svg_config.set_args(["--dataset", "synthetic-ball", "--config", "model_10_26"])
    vsd = SO.seeded_weights(SO.vae_shapes(VCFG), 3)
    usd = SO.seeded_weights(SO.unet_shapes(UCFG), 4)
    sdu = SDUtils(weights={"vae": vsd, "unet": usd, "text_encoder": "synthetic"}, arch={"vae": VCFG, "unet": UCFG}, verbose=False)
    torch.manual_seed(3)
    m = Transformer(dim_model=64, num_heads=4, num_encoder_layers=1, num_decoder_layers=2).eval()
    clips = bouncing_ball_clips(2, 64, 7, seed=5)
    res = metrics.evaluate_holdout(m, sdu, clips, 5, seeds=[11, 12])
    assert res["frames"].shape == (2, 6, 64, 64, 3) and res["latents"].shape == (2, 6, 256) and res["clips"] == 2
    frames, cl = res["frames"].cpu().numpy(), clips.numpy()
    n = 64 * 64 * 3
    for prefix, got in (("", frames[:, 4:6]), ("copy_last_", np.broadcast_to(cl[:, 4:5], cl[:, 5:7].shape))):
        sse_ref, ssim_ref, _ = J.judge(np.ascontiguousarray(got), cl[:, 5:7])
        assert res[prefix + "psnr"].shape == (2, 2)
        np.testing.assert_allclose(res[prefix + "mse"], sse_ref / float(n), rtol=1e-15)                # the squared error is exact
        want_psnr = np.where(sse_ref == 0, np.inf, 10.0 * np.log10(255.0 ** 2 / np.maximum(sse_ref / float(n), 1e-300)))
        np.testing.assert_allclose(res[prefix + "psnr"], want_psnr, rtol=1e-12, atol=1e-12)
        assert np.abs(res[prefix + "ssim"] - ssim_ref).max() < J.MEAN_TOL
    assert np.isfinite(res["copy_last_psnr"]).all()                          # the ball moves between frames
    np.testing.assert_allclose(res["mean"]["ssim"], res["ssim"].mean(axis=0), rtol=1e-15)
    assert list(res["mean"]["psnr_infinite"]) == [0, 0]


def test_main_prints_one_row_per_predicted_step(monkeypatch, capsys, tmp_path):
    """`python -m prediction.predict --eval_holdout 1 --pred_frames 2`: two metric rows under the header; without the flag the command
    prints what it printed before the flag existed, and both runs sample the same latents (the conditioning frames are the same)"""
    from sd_video_gen_amd import predict as P
    monkeypatch.setenv("SVG_ALLOW_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.delenv("SVG_SD_WEIGHTS", raising=False)
    monkeypatch.chdir(tmp_path)
    argv = ["--dataset", "synthetic-ball", "--config", "model_10_26", "--pred_frames", "2"]
    torch.manual_seed(3)
    lat_plain = P.main(argv)
    plain = capsys.readouterr().out.strip().splitlines()
    torch.manual_seed(3)
    lat_hold = P.main(argv + ["--eval_holdout", "1"])
    held = capsys.readouterr().out.strip().splitlines()
    n = len(plain)
    assert all(line.startswith("[sd-video-gen] ") for line in plain[:-1]) and plain[-1] == "all_latents shape:  (8, 6, 256)"
    assert held[:n] == plain and len(held) == n + 1 + 2
    assert held[n].split()[:4] == ["step", "PSNR", "SSIM", "MSE"] and "copy-last" in held[n] and held[n].split()[-1] == "clips"
    for k, row in enumerate(held[n + 1:]):
        cols = row.split()
        assert len(cols) == 7 and int(cols[0]) == k + 1 and int(cols[-1]) == 8
        assert all(math.isfinite(float(c)) for c in cols[1:6])
        assert -1.0 <= float(cols[2]) <= 1.0 and -1.0 <= float(cols[5]) <= 1.0
    assert torch.equal(lat_plain, lat_hold)
    assert not (tmp_path / "outputs").exists()


def test_main_holds_out_frames_of_png_clip_folders_and_writes_the_json(monkeypatch, capsys, tmp_path):
    """`--dataset ball --folder <dir> --eval_holdout 1 --pred_frames 2 --save_output True`: the crawler hands out 7-frame clips, the
    first 5 condition, and outputs/metrics_<config>_<index>_<mode>.json holds what evaluate_holdout gives for the same clips"""
    import json
    import os
    from PIL import Image
    from sd_video_gen_amd import predict as P, config as svg_config, metrics
    from sd_video_gen_amd.sd_utils import SDUtils
    from sd_video_gen_amd.transformer import Transformer
    monkeypatch.setenv("SVG_ALLOW_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.delenv("SVG_SD_WEIGHTS", raising=False)
    monkeypatch.chdir(tmp_path)
    clips = P.bouncing_ball_clips(3, 64, 7, seed=7)
    for c in range(3):
        d = tmp_path / "data" / "test" / ("%04d" % (c + 1))
        os.makedirs(d)
        for t in range(7):
            Image.fromarray(clips[c, t].numpy()).save(d / ("frame_%03d.png" % t))
    argv = ["--dataset", "ball", "--folder", str(tmp_path / "data"), "--config", "model_10_26", "--pred_frames", "2", "--eval_holdout", "1",
            "--save_output", "True", "--index", "3", "--mode", "test"]
    torch.manual_seed(3)
    lat = P.main(argv)
    out = capsys.readouterr().out.strip().splitlines()
    assert lat.shape == (3, 6, 256) and out[-3].split()[0] == "step" and [r.split()[-1] for r in out[-2:]] == ["3", "3"]
    with open(os.path.join("outputs", "metrics_model_10_26_3_test.json")) as f:
        saved = json.load(f)
    svg_config.set_args(argv)
    torch.manual_seed(3)
    sdu = SDUtils(verbose=False)
    m = Transformer(num_tokens=0, dim_model=256, num_heads=8, num_encoder_layers=6, num_decoder_layers=6, dropout_p=0.1).eval()
    res = metrics.evaluate_holdout(m, sdu, clips, 5, seeds=[0, 1, 2])
    assert torch.equal(res["latents"], lat)
    assert saved == json.loads(json.dumps(metrics.to_json(res))) and saved["clips"] == 3
    assert np.array(saved["psnr"]).shape == (3, 2) and len(saved["mean"]["ssim"]) == 2 and len(saved["copy_last_mean"]["psnr"]) == 2
