"""Per-frame quality of predicted frames against held-out ground truth: PSNR and SSIM per predicted step, next to FVD.

``frame_metrics`` compares two uint8 frame stacks on the device (``svg_frame_metrics``: the exact integer sum of squared
differences and the mean 11x11-Gaussian SSIM of Wang et al. 2004, valid positions only); MSE and PSNR are host arithmetic on the
exact integer.  ``evaluate_holdout`` is the protocol: condition on the first frames of longer clips, predict the rest, compare
each predicted step with the frame that was held out, and with the copy-last-frame baseline (the baseline the reference's
``predict_naive_fvd.py`` compares against).  The reference itself has no per-frame measure.
"""
import math

import numpy as np
import torch

from . import _lib

WINDOW = 11           # the SSIM window: frames smaller than this have no valid position


def psnr_from_sse(sse, n_values):
    """sse (integer tensor), values per image -> (mse, psnr) float64 tensors: mse = sse / n_values, psnr = 10 log10(255^2 / mse), inf where
    sse == 0"""
    sse = torch.as_tensor(sse)
    mse = sse.to(torch.float64) / float(n_values)
    psnr = torch.where(sse == 0, torch.full_like(mse, math.inf), 10.0 * torch.log10(255.0 ** 2 / mse.clamp_min(1e-300)))
    return mse, psnr


def _check_pair(pred_u8, true_u8):
    a, b = torch.as_tensor(pred_u8), torch.as_tensor(true_u8)
    if a.dtype != torch.uint8 or b.dtype != torch.uint8:
        raise ValueError("frame_metrics takes uint8 frames, got %s and %s" % (a.dtype, b.dtype))
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError("frame_metrics takes two stacks of one shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    if a.dim() < 3 or a.shape[-1] != 3:
        raise ValueError("frame_metrics takes (..., H, W, 3) frames, got %s" % (tuple(a.shape),))
    if a.shape[-3] < WINDOW or a.shape[-2] < WINDOW:
        raise ValueError("frame_metrics needs frames of at least %d x %d (the SSIM window), got %d x %d"
                         % (WINDOW, WINDOW, a.shape[-3], a.shape[-2]))
    return a, b


def frame_metrics(pred_u8, true_u8, ctx=None, return_map=False):
    """uint8 tensors or arrays (..., H, W, 3) of equal shape -> dict of tensors shaped like the leading dimensions: ``sse`` (int64, exact),
    ``mse`` (float64, sse / (H W 3)), ``psnr`` (float64, 10 log10(255^2 / mse), inf where sse == 0), ``ssim`` (float64) and, with
    ``return_map``, ``ssim_map`` (float32, (..., H - 10, W - 10, 3)).  ValueError for unequal shapes, a dtype other than uint8, a last
    dimension other than 3 or H / W below 11 (before any context is touched).  ``ctx``: the library context (default: the process's)."""
    a, b = _check_pair(pred_u8, true_u8)
    lead = tuple(a.shape[:-3])
    H, W = int(a.shape[-3]), int(a.shape[-2])
    if ctx is None:
        ctx = _lib.default_context()
    out = ctx.frame_metrics(a.reshape(-1, H, W, 3), b.reshape(-1, H, W, 3), return_map=return_map)
    sse = out[0].reshape(lead)
    mse, psnr = psnr_from_sse(sse, H * W * 3)
    res = {"sse": sse, "mse": mse, "psnr": psnr, "ssim": out[1].reshape(lead)}
    if return_map:
        res["ssim_map"] = out[2].reshape(lead + (H - 10, W - 10, 3))
    return res


def step_means(psnr, ssim, mse):
    """(C, P) arrays -> per-step means over clips: a step's mean PSNR is taken over its finite values (nan when it has none) and the
    count of infinite ones (identical frames) is reported beside it"""
    psnr, ssim, mse = (np.asarray(x, dtype=np.float64) for x in (psnr, ssim, mse))
    finite = np.isfinite(psnr)
    n_fin = finite.sum(axis=0)
    mean_psnr = np.where(n_fin > 0, np.where(finite, psnr, 0.0).sum(axis=0) / np.maximum(n_fin, 1), np.nan)
    return {"psnr": mean_psnr, "psnr_infinite": (~finite).sum(axis=0), "ssim": ssim.mean(axis=0), "mse": mse.mean(axis=0)}


def holdout_metrics(frames_u8, clips_u8, cond_frames, metrics_fn=frame_metrics):
    """The comparison half of ``evaluate_holdout``: ``frames_u8`` (C, cond_frames - 1 + P, F, F, 3) as sample_clips returns them for the
    first ``cond_frames`` frames of ``clips_u8`` (C, cond_frames + P, F, F, 3).  The emitted clip drops the last conditioning frame
    (SURVEY §9.3), so prediction k is frame cond_frames - 1 + k and its target is clips[:, cond_frames + k]; the baseline repeats
    clips[:, cond_frames - 1]."""
    clips_u8 = torch.as_tensor(clips_u8)
    P = clips_u8.shape[1] - cond_frames
    if P < 1 or cond_frames < 1:
        raise ValueError("hold-out evaluation needs clips of cond_frames + P frames, P >= 1: got %d frames for cond_frames %d"
                         % (clips_u8.shape[1], cond_frames))
    if frames_u8.shape[1] != cond_frames - 1 + P:
        raise ValueError("expected %d emitted frames (%d conditioning - 1 + %d predicted), got %d" % (cond_frames - 1 + P, cond_frames, P, frames_u8.shape[1]))
    target = clips_u8[:, cond_frames:].to(frames_u8.device)
    pred = frames_u8[:, cond_frames - 1:]
    last = clips_u8[:, cond_frames - 1:cond_frames].to(frames_u8.device).expand_as(target)
    out = {}
    for prefix, got in (("", pred), ("copy_last_", last)):
        m = metrics_fn(got.contiguous(), target.contiguous())
        for k in ("psnr", "ssim", "mse"):
            out[prefix + k] = torch.as_tensor(m[k]).detach().cpu().numpy().astype(np.float64)
    out["mean"] = step_means(out["psnr"], out["ssim"], out["mse"])
    out["copy_last_mean"] = step_means(out["copy_last_psnr"], out["copy_last_ssim"], out["copy_last_mse"])
    out["clips"] = int(clips_u8.shape[0])
    return out


def evaluate_holdout(model, sd_utils, clips_u8, cond_frames, metrics_fn=frame_metrics, **sample_kw):
    """``clips_u8`` (C, cond_frames + P, F, F, 3): sample P frames from the first ``cond_frames`` (``sample_clips(..., return_frames=True,
    **sample_kw)``) and compare prediction k with the held-out frame clips[:, cond_frames + k].  Returns a dict: ``psnr``, ``ssim``,
    ``mse`` (C, P) float64 arrays; ``copy_last_psnr`` / ``_ssim`` / ``_mse``, the same for clips[:, cond_frames - 1] against every target;
    ``mean`` and ``copy_last_mean``, the per-step means over clips (``step_means``); ``clips``; ``latents`` and ``frames`` as sample_clips
    returns them."""
    from . import predict
    clips_u8 = torch.as_tensor(clips_u8)
    P = clips_u8.shape[1] - cond_frames
    if P < 1:
        raise ValueError("hold-out evaluation needs clips of cond_frames + P frames, P >= 1: got %d frames for cond_frames %d"
                         % (clips_u8.shape[1], cond_frames))
    dev = sd_utils.device
    lat, frames = predict.sample_clips(model, sd_utils, clips_u8[:, :cond_frames].to(dev), P, return_frames=True, **sample_kw)
    out = holdout_metrics(frames, clips_u8, cond_frames, metrics_fn=metrics_fn)
    out["latents"], out["frames"] = lat, frames
    return out


def format_table(res):
    """the per-step table of a hold-out result, one row per predicted step"""
    m, b = res["mean"], res["copy_last_mean"]
    rows = ["step    PSNR     SSIM        MSE   copy-last PSNR   copy-last SSIM   clips"]
    for k in range(len(m["ssim"])):
        rows.append("%4d  %6.2f  %7.4f  %9.2f   %14.2f   %14.4f   %5d" % (k + 1, m["psnr"][k], m["ssim"][k], m["mse"][k], b["psnr"][k], b["ssim"][k],
                                                                         res["clips"]))
    return rows


def to_json(res):
    """a hold-out result without its tensors, as plain lists (infinite PSNRs become the string 'inf')"""
    def plain(x):
        if isinstance(x, dict):
            return {k: plain(v) for k, v in x.items()}
        if isinstance(x, np.ndarray):
            return [plain(v) for v in x.tolist()]
        if isinstance(x, list):
            return [plain(v) for v in x]
        if isinstance(x, float) and not math.isfinite(x):
            return "nan" if math.isnan(x) else ("inf" if x > 0 else "-inf")
        return x
    return plain({k: v for k, v in res.items() if k not in ("latents", "frames")})
