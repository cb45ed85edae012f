"""No GPU: the fp64 judge of svg_frame_metrics against an independent formulation and closed forms, the float32 emulation that
justifies the GPU tolerances, the host arithmetic of PSNR / MSE, the argument checks, the hold-out index bookkeeping and the flag.

Measured here (float32 emulation of the kernel's arithmetic against the judge, over the whole input set of frame_metrics_judge.cases()):
worst map element 5.7e-5 (128x128 ball), worst image mean 1.99e-5 (the single-position 11x11 ramp); without the 128 shift 2.6e-4 and 4.7e-6."""
import math

import numpy as np
import pytest
import torch

import frame_metrics_judge as J


def test_judge_matches_scipy_formulation():
    """skimage's formulation: scipy.ndimage.gaussian_filter(sigma 1.5, truncate 3.5, reflect) on the whole image, cropped by 5"""
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(7)
    a, b = rng.integers(0, 256, (27, 43, 3), dtype=np.uint8), rng.integers(0, 256, (27, 43, 3), dtype=np.uint8)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    G = lambda x: np.stack([ndi.gaussian_filter(x[..., c], 1.5, truncate=3.5, mode="reflect") for c in range(3)], -1)      # noqa: E731
    mu_a, mu_b = G(a64), G(b64)
    var_a, var_b, cov = G(a64 * a64) - mu_a * mu_a, G(b64 * b64) - mu_b * mu_b, G(a64 * b64) - mu_a * mu_b
    m = (((2 * mu_a * mu_b + J.C1) * (2 * cov + J.C2)) / ((mu_a ** 2 + mu_b ** 2 + J.C1) * (var_a + var_b + J.C2)))[5:-5, 5:-5]
    sse, ssim, jm = J.judge(a, b)
    assert jm.shape == (17, 33, 3) and m.shape == jm.shape
    assert np.abs(jm - m).max() < 1e-12
    assert abs(ssim - m.mean()) < 1e-12
    assert sse == ((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum()


def test_judge_closed_forms():
    z, w = np.zeros((1, 14, 17, 3), np.uint8), np.full((1, 14, 17, 3), 255, np.uint8)
    sse, ssim, m = J.judge(z, w)
    want = J.C1 / (255.0 ** 2 + J.C1)
    assert np.abs(m - want).max() < 1e-13 and abs(ssim[0] - want) < 1e-13
    assert sse[0] == 14 * 17 * 3 * 255 ** 2
    a = np.random.default_rng(3).integers(0, 256, (2, 13, 12, 3), dtype=np.uint8)
    sse, ssim, m = J.judge(a, a.copy())
    assert (m == 1.0).all() and (ssim == 1.0).all() and (sse == 0).all()
    assert abs(J.taps().sum() - 1.0) < 1e-15 and len(J.taps()) == 11
    assert abs(J.C1 - 6.5025) < 1e-12 and abs(J.C2 - 58.5225) < 1e-12


def test_f32_emulation_stays_within_a_quarter_of_the_gpu_tolerances():
    """the tolerances of the GPU test rest on this, not on what the kernel gives: float32 arithmetic in the kernel's order (pixels minus
    128, separable sequential accumulation) over the GPU test's whole input set"""
    worst_map, worst_mean = (0.0, ""), (0.0, "")
    for cid, N, H, W, kind in J.cases():
        a, b = J.make_pair(kind, N, H, W)
        _, ssim, m = J.judge(a, b)
        e_ssim, e_m = J.emulate_f32(a, b)
        worst_map = max(worst_map, (float(np.abs(e_m - m).max()), cid))
        worst_mean = max(worst_mean, (float(np.abs(e_ssim - ssim).max()), cid))
    print("f32 emulation vs fp64 judge: worst map element %.3e (%s), worst image mean %.3e (%s)" % (worst_map + worst_mean))
    assert worst_map[0] <= J.MAP_TOL / 4, worst_map
    assert worst_mean[0] <= J.MEAN_TOL / 4, worst_mean


def test_psnr_and_mse_from_sse():
    from sd_video_gen_amd.metrics import psnr_from_sse
    n = 64 * 64 * 3
    sse = torch.tensor([[0, n], [n * 255 ** 2, 7]], dtype=torch.int64)
    mse, psnr = psnr_from_sse(sse, n)
    assert mse.dtype == torch.float64 and psnr.dtype == torch.float64 and mse.shape == (2, 2)
    assert mse[0, 0] == 0.0 and math.isinf(psnr[0, 0]) and psnr[0, 0] > 0
    assert mse[0, 1] == 1.0 and abs(float(psnr[0, 1]) - 10 * math.log10(255.0 ** 2)) < 1e-12
    assert mse[1, 0] == 255.0 ** 2 and abs(float(psnr[1, 0])) < 1e-12
    assert abs(float(mse[1, 1]) - 7.0 / n) < 1e-18 and abs(float(psnr[1, 1]) - 10 * math.log10(255.0 ** 2 * n / 7.0)) < 1e-10


class _NoContext:
    def __getattr__(self, name):
        raise AssertionError("frame_metrics touched the context (%s) before rejecting its arguments" % name)


@pytest.mark.parametrize("a_shape,b_shape,a_dtype,b_dtype", [
    ((2, 16, 16, 3), (2, 16, 17, 3), np.uint8, np.uint8),        # unequal shapes
    ((2, 16, 16, 3), (2, 16, 16, 3), np.float32, np.uint8),      # not uint8
    ((2, 16, 16, 3), (2, 16, 16, 3), np.uint8, np.int16),
    ((2, 16, 16, 4), (2, 16, 16, 4), np.uint8, np.uint8),        # last dimension
    ((16, 3), (16, 3), np.uint8, np.uint8),
    ((2, 10, 16, 3), (2, 10, 16, 3), np.uint8, np.uint8),        # H below the window
    ((2, 16, 10, 3), (2, 16, 10, 3), np.uint8, np.uint8),        # W below the window
])
def test_frame_metrics_rejects_bad_arguments_before_the_context(a_shape, b_shape, a_dtype, b_dtype):
    from sd_video_gen_amd.metrics import frame_metrics
    with pytest.raises(ValueError):
        frame_metrics(np.zeros(a_shape, a_dtype), np.zeros(b_shape, b_dtype), ctx=_NoContext())
    with pytest.raises(ValueError):
        frame_metrics(torch.zeros(a_shape, dtype=torch.from_numpy(np.zeros(1, a_dtype)).dtype),
                      torch.zeros(b_shape, dtype=torch.from_numpy(np.zeros(1, b_dtype)).dtype), ctx=_NoContext())


def test_holdout_indices_baseline_and_step_means(monkeypatch):
    """frames are tagged by (clip, index) in their first byte: prediction k (frame cond - 1 + k of the emitted clip) must meet
    clips[:, cond + k], the baseline must be clips[:, cond - 1], and a step's mean PSNR skips and counts the infinite values"""
    from sd_video_gen_amd import metrics, predict
    C, cond, P, F = 3, 5, 2, 11
    clips = torch.zeros((C, cond + P, F, F, 3), dtype=torch.uint8)
    for c in range(C):
        for t in range(cond + P):
            clips[c, t] = 10 * c + t                                  # ground-truth frame t of clip c carries 10 c + t
    seen = {}

    def fake_sample_clips(model, sd_utils, clips_u8, pred_frames, return_frames=False, **kw):
        seen["args"] = (model, tuple(clips_u8.shape), pred_frames, return_frames, kw)
        assert torch.equal(clips_u8, clips[:, :cond])                 # conditioning: the first cond frames only
        n_out = cond - 1 + pred_frames                                # the emitted clip drops the last conditioning frame
        frames = torch.zeros((C, n_out, F, F, 3), dtype=torch.uint8)
        for c in range(C):
            for i in range(n_out):
                frames[c, i] = 100 + 10 * c + i                       # emitted frame i of clip c carries 100 + 10 c + i
        return torch.zeros((C, n_out, 4)), frames

    calls = []

    def fake_metrics(pred, true):
        pt, tt = pred[..., 0, 0, 0].to(torch.float64), true[..., 0, 0, 0].to(torch.float64)
        calls.append((pt.clone(), tt.clone()))
        psnr = pt.clone()
        if len(calls) == 1:
            psnr[0, 0] = math.inf                                     # clip 0, step 0 of the prediction: identical frames
            psnr[1, 1] = math.inf
            psnr[0, 1] = math.inf
            psnr[2, 1] = math.inf                                     # step 1: no finite value at all
        return {"psnr": psnr, "ssim": tt / 100.0, "mse": pt - tt, "sse": torch.zeros_like(pt, dtype=torch.int64)}

    monkeypatch.setattr(predict, "sample_clips", fake_sample_clips)

    class FakeSD:
        device = torch.device("cpu")

    res = metrics.evaluate_holdout("model", FakeSD(), clips, cond, metrics_fn=fake_metrics, seeds=[4, 5, 6], denoise=False)
    assert seen["args"][0] == "model" and seen["args"][2] == P and seen["args"][3] is True
    assert seen["args"][4] == {"seeds": [4, 5, 6], "denoise": False}
    assert len(calls) == 2
    want_pred = torch.tensor([[100.0 + 10 * c + cond - 1 + k for k in range(P)] for c in range(C)], dtype=torch.float64)
    want_true = torch.tensor([[10.0 * c + cond + k for k in range(P)] for c in range(C)], dtype=torch.float64)
    want_last = torch.tensor([[10.0 * c + cond - 1] * P for c in range(C)], dtype=torch.float64)
    assert torch.equal(calls[0][0], want_pred) and torch.equal(calls[0][1], want_true)
    assert torch.equal(calls[1][0], want_last) and torch.equal(calls[1][1], want_true)
    for k in ("psnr", "ssim", "mse", "copy_last_psnr", "copy_last_ssim", "copy_last_mse"):
        assert res[k].shape == (C, P) and res[k].dtype == np.float64
    np.testing.assert_array_equal(res["mse"], (want_pred - want_true).numpy())
    np.testing.assert_array_equal(res["copy_last_psnr"], want_last.numpy())
    np.testing.assert_array_equal(res["copy_last_ssim"], (want_true / 100.0).numpy())
    # step 0: clips 1 and 2 are finite, clip 0 is not; step 1: nothing finite
    m = res["mean"]
    assert m["psnr"][0] == (want_pred[1, 0] + want_pred[2, 0]) / 2 and m["psnr_infinite"][0] == 1
    assert math.isnan(m["psnr"][1]) and m["psnr_infinite"][1] == 3
    np.testing.assert_allclose(m["ssim"], (want_true / 100.0).numpy().mean(axis=0), rtol=1e-15)
    np.testing.assert_allclose(m["mse"], (want_pred - want_true).numpy().mean(axis=0), rtol=1e-15)
    b = res["copy_last_mean"]
    assert list(b["psnr_infinite"]) == [0, 0] and b["psnr"][0] == want_last[:, 0].mean()
    assert res["clips"] == C and res["frames"].shape == (C, cond - 1 + P, F, F, 3) and res["latents"].shape == (C, cond - 1 + P, 4)
    rows = metrics.format_table(res)
    assert len(rows) == 1 + P
    import json
    json.dumps(metrics.to_json(res))
    with pytest.raises(ValueError):
        metrics.evaluate_holdout("model", FakeSD(), clips[:, :cond], cond, metrics_fn=fake_metrics)


def test_eval_holdout_flag_defaults_to_false_and_leaves_the_existing_command_lines_alone():
    from sd_video_gen_amd import config as svg_config
    lines = [["--dataset", "synthetic-ball", "--config", "model_10_26"],
             ["--dataset", "synthetic-ball", "--config", "model_10_26", "--denoise", "1", "--pred_frames", "4"],
             ["--dataset", "ball", "--config", "1_19_ball_complex_L1_64", "--folder", "x", "--save_output", "True", "--sampler", "dpmpp_2m"]]
    for argv in lines:
        cfg, args = svg_config.parse_config_args(argv)
        assert args.eval_holdout is False
        d = dict(vars(args))
        d.pop("eval_holdout")
        # everything else is what the parser gave before the flag existed: the defaults and the given values
        assert d["dataset"] == argv[1] and d["config"] == argv[3] and cfg.CONFIG_NAME == argv[3]
        assert d["pred_frames"] == (4 if "--pred_frames" in argv else 1) and d["denoise"] is ("--denoise" in argv)
        assert d["sampler"] == ("dpmpp_2m" if "--sampler" in argv else "ddim") and d["save_output"] is ("--save_output" in argv)
        assert d["denoise_steps"] == 50 and d["denoise_start_step"] == 40 and d["index"] == 0 and d["mode"] == ""
        assert len(d) == 27
    _, args = svg_config.parse_config_args(lines[0] + ["--eval_holdout", "True", "--pred_frames", "4"])
    assert args.eval_holdout is True and args.pred_frames == 4
