"""GPU: the VAE's opt-in f32 residual stream (VAE key stream_f32, SDUtils(vae_residual='f32')).

The reference runs its VAE in fp32 (utils/sd_utils.py:140,162).  In f32-stream mode the tensors a block hands to the next — conv_in's
output, every resnet's conv2 + residual, the mid-block attention's proj_attn + residual, the up / down-sampler outputs — are summed and
stored in f32; GroupNorm / conv1 / shortcut outputs and every matrix operand stay 16-bit (the "f32 residual stream everywhere" variant of
tests/analysis_vae_decoder_storage.py).  Checked here, bottom up:
  * the f32-output epilogue of the halo conv (both channel-tile widths, stride 1 and the fused upsample) and of the implicit GEMM,
    bit for bit on integer data, and which kernel ran;
  * GroupNorm on the f32 stream, from the epilogue's column sums and from its own statistics pass;
  * the full-size decoder and encoder against the fp32 oracle, default mode and f32 mode side by side;
  * sample_clips in f32 mode against the CPU loop oracle, the workspace planned once, and two contexts at once bit-reproducible.
"""
import os
import sys
import threading

import pytest
import torch
import torch.nn.functional as F

from conftest import margin, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden_sd as GG, loop_oracle, sd_oracle as SO  # noqa: E402
from sd_video_gen_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden", "sd_cfg2_stages_autocast.pt")
STORAGE = {"bf16": (torch.bfloat16, "", 8), "fp16": (torch.float16, "_f16", 11)}     # dtype, op suffix, significand bits


@pytest.fixture(params=["bf16", "fp16"])
def storage(request):
    return STORAGE[request.param]


@pytest.fixture
def halo_min(monkeypatch):
    """let the halo kernel take test-sized convs (it needs >= 192 workgroups by default), as the existing parity tests do"""
    monkeypatch.setenv("SVG_HALO_MIN", "1")
    _lib.env_refresh()
    yield
    monkeypatch.delenv("SVG_HALO_MIN")
    _lib.env_refresh()


def _conv_f32s(ctx, st, x, w, residual=None, residual_f32=None, mode=0, gn=None):
    """svg_op_conv3x3_f32s: returns (f32 out, gn_out or None, halo width, used_epilogue_stats)"""
    dt, suffix, _ = st
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    Ho, Wo = (H, W) if mode == 0 else ((H // 2, W // 2) if mode == 2 else (2 * H, 2 * W))
    out = torch.empty(B, Ho, Wo, Cout, device="cuda", dtype=torch.float32)
    hw, used = _lib.C.c_int(-1), _lib.C.c_int(-1)
    gamma = beta = gn_out = None
    if gn is not None:
        gamma, beta = gn
        gn_out = torch.empty(B, Ho, Wo, Cout, device="cuda", dtype=dt)
    ptr = lambda t: t.data_ptr() if t is not None else None
    fn = getattr(ctx.lib, "svg_op_conv3x3_f32s" + suffix)
    ctx.check(fn(ctx.h, ptr(x), ptr(w), None, ptr(residual), ptr(residual_f32), ptr(out), ptr(gamma), ptr(beta), ptr(gn_out),
                 B, H, W, Cin, Cout, mode, 32, 1e-6, 1, _lib.C.byref(hw), _lib.C.byref(used), None), "conv3x3_f32s")
    torch.cuda.synchronize()
    return out, gn_out, hw.value, used.value


def _conv_ref_i64(x, w, mode):
    """3x3 conv of integer-valued tensors, exact: every partial sum is an integer below 9 * Cin <= 2^24, so the f32 CPU conv is exact in
    any summation order; returned as int64 NHWC"""
    xc = x.float().cpu().permute(0, 3, 1, 2)
    if mode == 2:
        y = F.conv2d(F.pad(xc, (0, 1, 0, 1)), w.cpu(), stride=2)
    elif mode == 3:
        y = F.conv2d(F.interpolate(xc, scale_factor=2.0, mode="nearest"), w.cpu(), padding=1)
    else:
        y = F.conv2d(xc, w.cpu(), padding=1)
    return y.permute(0, 2, 3, 1).round().to(torch.int64)


# (B, H, W, Cin, Cout, mode, expected halo width (0 = implicit GEMM), SVG_HALO_MIN=1)
CASES = [
    (1, 32, 32, 64, 128, 0, 128, True),          # halo, stride 1, 128-channel tiles
    (1, 192, 192, 64, 160, 0, 160, True),        # halo, stride 1, 160-channel tiles (fewer serial rounds than 2 x 128)
    (1, 16, 16, 64, 128, 3, 128, True),          # halo, nearest-2x upsample in front
    (1, 96, 96, 64, 160, 3, 160, True),          # halo, upsample, 160-channel tiles
    (2, 88, 88, 64, 256, 0, 0, False),           # implicit GEMM (88 % 16 != 0), no split-K
    (1, 8, 8, 64, 320, 0, 0, False),             # implicit GEMM with split-K (the f32-stream reduce), 160-column tiles
    (1, 64, 64, 8, 128, 0, 0, False),            # implicit GEMM, 8-channel input (conv_in)
    (1, 64, 64, 128, 128, 2, 0, False),          # implicit GEMM, stride 2 (the encoder's downsamplers)
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%d_%d-%d_m%d_w%d" % c[:7])
@pytest.mark.parametrize("res_kind", ["f32", "h16"])
def test_f32_stream_conv_is_exact_and_takes_the_expected_kernel(ctx, storage, case, res_kind, monkeypatch):
    """x, w in {-1, 0, 1}: the conv sums are exact in f32.  The f32 residual holds odd integers in [4097, 8191], which neither fp16 nor
    bf16 can represent: the output is exact only if the residual is read, added and stored in f32.  (The 16-bit residual: small integers.)"""
    B, H, W, Cin, Cout, mode, width, force = case
    if force:
        monkeypatch.setenv("SVG_HALO_MIN", "1")
    _lib.env_refresh()
    try:
        dt = storage[0]
        g = torch.Generator(device="cuda").manual_seed(B * H + Cin + Cout + mode)
        x = torch.randint(-1, 2, (B, H, W, Cin), device="cuda", generator=g).to(dt)
        w = torch.randint(-1, 2, (Cout, Cin, 3, 3), device="cuda", generator=g).float()
        want = _conv_ref_i64(x, w, mode)
        if res_kind == "f32":
            r = (torch.randint(2048, 4096, want.shape, device="cuda", generator=g) * 2 + 1).float()
            out, _, hw, _ = _conv_f32s(ctx, storage, x, w, residual_f32=r, mode=mode)
        else:
            r = torch.randint(-64, 65, want.shape, device="cuda", generator=g).to(dt)
            out, _, hw, _ = _conv_f32s(ctx, storage, x, w, residual=r, mode=mode)
        want = want + r.cpu().to(torch.int64)
    finally:
        monkeypatch.delenv("SVG_HALO_MIN", raising=False)
        _lib.env_refresh()
    assert hw == width, "kernel: halo width %d, expected %d" % (hw, width)
    assert torch.equal(out.cpu(), want.to(torch.float32)), case


def _gn64(y, gamma, beta, groups=32, eps=1e-6, silu=True):
    t = F.group_norm(y.double().permute(0, 3, 1, 2), groups, gamma.double(), beta.double(), eps)
    if silu:
        t = F.silu(t)
    return t.permute(0, 2, 3, 1)


def _close_to_rounding(got, ref, bits, what):
    """got (16-bit) equals ref (float64) up to one rounding to `bits` significant bits, plus the f32 statistics' own error"""
    err = (got.double().cpu() - ref.cpu()).abs()
    tol = ref.cpu().abs() * 2.0 ** (-bits) + 2e-4
    bad = (err > tol).sum().item()
    print("[f32 stream] %s: max |err| %.3e, %d of %d beyond one rounding" % (what, err.max().item(), bad, err.numel()))
    assert bad == 0, what


@pytest.mark.parametrize("path", ["halo", "igemm"])
def test_f32_stream_groupnorm_from_epilogue_sums(ctx, storage, path, halo_min):
    """conv (f32 stream) -> GroupNorm + SiLU from the epilogue's column sums of the STORED f32 values, at H = W >= 32"""
    dt, _, bits = storage
    g = torch.Generator(device="cuda").manual_seed(5)
    if path == "halo":
        x = torch.randn(1, 32, 32, 128, device="cuda", generator=g).to(dt)
        w = torch.randn(256, 128, 3, 3, device="cuda", generator=g) * 0.03
    else:                                        # 8-channel input: the implicit GEMM without split-K (K = 72)
        x = torch.randn(1, 64, 64, 8, device="cuda", generator=g).to(dt)
        w = torch.randn(128, 8, 3, 3, device="cuda", generator=g) * 0.2
    Cout = w.shape[0]
    r = torch.randn(*x.shape[:3], Cout, device="cuda", generator=g) * 2 + 0.5
    gamma = torch.rand(Cout, device="cuda", generator=g) + 0.5
    beta = torch.randn(Cout, device="cuda", generator=g) * 0.1
    out, gn_out, hw, used = _conv_f32s(ctx, storage, x, w, residual_f32=r, gn=(gamma, beta))
    assert (hw > 0) == (path == "halo")
    assert used == 1, "the GroupNorm ran its own statistics pass"
    _close_to_rounding(gn_out, _gn64(out, gamma, beta), bits, "GroupNorm from %s epilogue sums" % path)


@pytest.mark.parametrize("hw", [16, 64], ids=["small_hw", "stats_pass"])
def test_groupnorm_on_f32_input(ctx, storage, hw):
    """the f32-input GroupNorm (+SiLU) op: single-launch small-HW kernel (16 x 16) and statistics pass + apply (64 x 64)"""
    dt, suffix, bits = storage
    g = torch.Generator(device="cuda").manual_seed(hw)
    B, C = 2, 128
    x = torch.randn(B, hw, hw, C, device="cuda", generator=g) * 3 + 1.5
    gamma = torch.rand(C, device="cuda", generator=g) + 0.5
    beta = torch.randn(C, device="cuda", generator=g) * 0.1
    out = torch.empty(B, hw, hw, C, device="cuda", dtype=dt)
    fn = getattr(ctx.lib, "svg_op_groupnorm_f32" + suffix)
    ctx.check(fn(ctx.h, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), B, hw * hw, C, 32, 1e-6, 1, None), "groupnorm_f32")
    torch.cuda.synchronize()
    _close_to_rounding(out, _gn64(x, gamma, beta), bits, "GroupNorm f32 input %dx%d" % (hw, hw))


# ---- full-size VAE against the fp32 oracle ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLD, weights_only=False)


@pytest.fixture(scope="module")
def vsd():
    return SO.seeded_weights(SO.vae_shapes(), GG.VAE_SEED)


@pytest.fixture(scope="module", autouse=True)
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    yield
    torch.set_num_threads(n)


def _vae(ctx, vsd, stream_f32):
    c = SO.SD_VAE
    ctx.configure(_lib.SVG_VAE, block_out=list(c["block_out"]), layers=2, groups=32, latent=4, f16=1, stream_f32=int(stream_f32))
    ctx.load_state_dict(_lib.SVG_VAE, vsd)
    assert ctx.finalize(_lib.SVG_VAE) == 83_653_863


def test_decode_512_closer_to_the_fp32_oracle(ctx, gold, vsd):
    """the fixture's denoised latent decoded at 512 x 512 in default mode and in f32-stream mode (same context, reconfigured), against
    the fp32 oracle: uint8 pixels changed at 512^2 and after the nearest resize to F = 64, max diff, float-image rel-L2.  The bars are the
    CPU replay's prediction (profiles/r05_vae_decoder_storage.txt: 7.53 % -> 6.10 %, 2.27e-3 -> 1.85e-3) with slack."""
    z = gold["den"].reshape(1, 4, 64, 64)
    with torch.no_grad():
        ref_img, ref_fl = SO.decode_img_latents(vsd, z, return_float=True)
    ref_img = torch.as_tensor(ref_img) if not torch.is_tensor(ref_img) else ref_img
    rows = {}
    for mode in (False, True):
        _vae(ctx, vsd, mode)
        img, fl = ctx.vae_decode(z.cuda(), return_float=True)
        img, fl = img.cpu(), fl.cpu()
        d = (img.int() - ref_img.int()).abs()
        rows[mode] = dict(flips=float((d > 0).float().mean()), flips_F=float((img[:, ::8, ::8] != ref_img[:, ::8, ::8]).float().mean()),
                          maxd=int(d.max()), rel=rel_l2(fl, ref_fl))
        print("[f32 stream] decode@512 %-8s uint8 changed %.2f %% @512^2, %.2f %% at F, max diff %d, image rel-L2 %.3e"
              % ("f32" if mode else "default", 100 * rows[mode]["flips"], 100 * rows[mode]["flips_F"], rows[mode]["maxd"], rows[mode]["rel"]))
    d16, d32 = rows[False], rows[True]
    margin("f32 stream decode@512: uint8 pixels changed @512^2", d32["flips"], 0.066, unit="share")
    margin("f32 stream decode@512: points fewer changed than default mode (>= 0.8)", 0.8 / max(100 * (d16["flips"] - d32["flips"]), 1e-9), 1.0,
           unit="ratio")
    margin("f32 stream decode@512: uint8 pixels changed at F", d32["flips_F"], 0.069, unit="share")
    assert d32["maxd"] <= 1
    margin("f32 stream decode@512: image rel-L2 relative to default mode", d32["rel"] / d16["rel"], 0.92, unit="ratio")


def test_encode_512_no_worse_than_default(ctx, vsd):
    """encoder moments @512 (inputs as test_vae_fp16_512) against SO.vae_encode_moments: f32-stream mode is no worse than default"""
    g = torch.Generator().manual_seed(12)
    img = torch.randint(0, 256, (1, 512, 512, 3), dtype=torch.uint8, generator=g)
    eps = torch.randn(1, 4, 64, 64, generator=g)
    x = 2 * ((img / 255.0).float().permute(0, 3, 1, 2) - 0.5)
    with torch.no_grad():
        ref = SO.vae_encode_moments(vsd, x)
    err = {}
    for mode in (False, True):
        _vae(ctx, vsd, mode)
        _, mom = ctx.vae_encode(img.cuda(), eps=eps.cuda(), return_moments=True)
        err[mode] = rel_l2(mom.cpu(), ref)
        print("[f32 stream] encode@512 %-8s moments rel-L2 %.3e" % ("f32" if mode else "default", err[mode]))
    margin("f32 stream encode@512: moments rel-L2 relative to default mode", err[True] / err[False], 1.0 + 1e-9, unit="ratio")


# ---- through SDUtils ---------------------------------------------------------------------------------------------------------------
VCFG = dict(block_out=(64, 128, 128, 128), layers=1, groups=32, latent=4)
UCFG = dict(block_out=(64, 128), layers=1, heads=4, ctx_dim=768, groups=32, in_ch=4, out_ch=4, attn=(1, 0))


def _set_cfg():
    from sd_video_gen_amd import config as svg_config
    svg_config.set_args(["--dataset", "synthetic-ball", "--config", "model_10_26", "--denoise", "1"])


def _small_nets(seed=3):
    return SO.seeded_weights(SO.vae_shapes(VCFG), seed), SO.seeded_weights(SO.unet_shapes(UCFG), seed + 1)


def _worker(vsd, usd, **kw):
    from sd_video_gen_amd.sd_utils import SDUtils
    from sd_video_gen_amd.transformer import Transformer
    c = _lib.Context(0)
    sdu = SDUtils(weights={"vae": vsd, "unet": usd, "text_encoder": "synthetic"}, arch={"vae": VCFG, "unet": UCFG}, verbose=False, ctx=c, **kw)
    torch.manual_seed(3)
    m = Transformer(dim_model=64, num_heads=4, num_encoder_layers=1, num_decoder_layers=2).eval().use_context(c)
    return m, sdu


def _clip_noise_cpu(seed, res, F_, pred_frames, start_step):
    g = torch.Generator(device="cuda").manual_seed(seed)
    L = F_ // 8
    n = {"cond": torch.randn((5, 4, L, L), generator=g, device="cuda").cpu(), "e512": [], "add": [], "eF": []}
    for _ in range(pred_frames):
        n["e512"].append(torch.randn((4, res // 8, res // 8), generator=g, device="cuda").cpu())
        if start_step > 0:
            n["add"].append(torch.randn((4, res // 8, res // 8), generator=g, device="cuda").cpu())
        n["eF"].append(torch.randn((4, L, L), generator=g, device="cuda").cpu())
    return n


def test_sample_clips_f32_stream_against_the_loop_oracle(monkeypatch):
    """reduced width, denoise round trip at 128 x 128: sample_clips with vae_residual='f32' against the CPU loop oracle (error no more than
    1.05 x default mode's), the workspace planned once (no growth from the second call on), and $SVG_VAE_RESIDUAL=f32 == the argument"""
    from sd_video_gen_amd.predict import sample_clips, bouncing_ball_clips
    _set_cfg()
    vsd, usd = _small_nets()
    clips = bouncing_ball_clips(2, 64, 5, seed=9)
    seeds, S = [21, 22], 47
    lat = {}
    for mode in ("fp16", "f32"):
        m, sdu = _worker(vsd, usd, vae_residual=mode)
        assert sdu.vae_residual == mode
        emb = sdu.encode_text([""])
        kw = dict(denoise=True, start_step=S, text_embeddings=emb, res=128)
        lat[mode] = sample_clips(m, sdu, clips.cuda(), 2, seeds=seeds, **kw)
        torch.cuda.synchronize()
        g1 = sdu.ctx.workspace_growths()
        again = sample_clips(m, sdu, clips.cuda(), 2, seeds=seeds, **kw)
        torch.cuda.synchronize()
        assert sdu.ctx.workspace_growths() == g1, "steady state allocated"
        assert torch.equal(again, lat[mode])
    xsd = {k: v.cpu() for k, v in m.state_dict().items()}
    err = {"fp16": [], "f32": []}
    for c in range(2):
        noise = _clip_noise_cpu(seeds[c], 128, 64, 2, S)
        ref = loop_oracle.sample_clip(xsd, 4, vsd, clips[c], 2, noise, denoise=True, start_step=S, unet_sd=usd, text_emb=emb.cpu(),
                                      vae_cfg=VCFG, unet_cfg=UCFG, res=128)
        for mode in err:
            err[mode].append(rel_l2(lat[mode][c:c + 1].cpu(), ref))
    print("[f32 stream] sample_clips vs loop oracle: default %s, f32 %s" % (err["fp16"], err["f32"]))
    margin("f32 stream sample_clips vs loop oracle, relative to default mode", sum(err["f32"]) / sum(err["fp16"]), 1.05, unit="ratio")
    monkeypatch.setenv("SVG_VAE_RESIDUAL", "f32")
    m2, sdu2 = _worker(vsd, usd)
    assert sdu2.vae_residual == "f32"
    lat_env = sample_clips(m2, sdu2, clips.cuda(), 2, seeds=seeds, denoise=True, start_step=S, text_embeddings=sdu2.encode_text([""]), res=128)
    assert torch.equal(lat_env, lat["f32"])


def test_two_contexts_f32_stream_bit_reproducible():
    """as test_two_contexts_at_once_are_bit_reproducible, in f32-stream mode: paired decodes and encodes from two threads equal the quiet
    single-context result (the f32-stream epilogues publish their GroupNorm sums through LDS too)"""
    _set_cfg()
    vsd, usd = _small_nets()
    W = [_worker(vsd, usd, vae_residual="f32")[1] for _ in range(2)]
    st = [torch.cuda.Stream() for _ in range(2)]
    g = torch.Generator(device="cuda").manual_seed(1)
    z = [torch.randn(2, 4, 16, 16, device="cuda", generator=g) * 0.2 for _ in range(2)]
    img = [torch.randint(0, 256, (2, 128, 128, 3), dtype=torch.uint8, device="cuda", generator=g) for _ in range(2)]
    eps = [torch.randn(2, 4, 16, 16, device="cuda", generator=g) for _ in range(2)]

    def calls(t):
        c = W[t].ctx
        return [c.vae_decode(z[t], out_hw=(64, 64), return_float=True)[1], c.vae_encode(img[t], eps=eps[t])]
    ref = []
    for t in range(2):
        with torch.cuda.stream(st[t]):
            ref.append([o.clone() for o in calls(t)])
            st[t].synchronize()
    bad = [0, 0]
    for _ in range(20):
        outs = [None, None]

        def run(t):
            with torch.cuda.stream(st[t]):
                outs[t] = calls(t)
                st[t].synchronize()
        ths = [threading.Thread(target=run, args=(t,)) for t in range(2)]
        [x.start() for x in ths]
        [x.join() for x in ths]
        for t in range(2):
            bad[t] += int(any(not torch.equal(o, r) for o, r in zip(outs[t], ref[t])))
    assert bad == [0, 0], "paired calls that differ from the quiet reference, per context: %s of 20" % bad


def test_vae_residual_is_validated():
    from sd_video_gen_amd.sd_utils import SDUtils
    _set_cfg()
    with pytest.raises(ValueError, match="vae_residual"):
        SDUtils(weights={"vae": "synthetic", "unet": "synthetic", "text_encoder": "synthetic"}, verbose=False, vae_residual="f64")
