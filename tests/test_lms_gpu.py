"""GPU: the LMS text-to-image sampler inside the library's sample loop (svg_sample_loop(SVG_SAMPLER_LMS), svg_lms_step) against
an f64 restatement of the update, the oracle's denoise_img_latents, its own direct-launch path, and the host loop it replaces.

Tolerances: one update is five f32 products and sums on f32-rounded coefficients: per element 16 * 2^-24 * (|x| + sum_k |c_k d_{i-k}|).
Loops through the seeded UNet use NET_TOL, the bound test_sd_gpu.py sets for this very loop; the library loop differs from the
host loop only in f32 rounding of the update, so its error may not exceed 1.5x the host loop's."""
import os
import sys

import pytest
import torch

from conftest import margin, rel_l2
from test_sd_gpu import NET_TOL, TINY_UNET, load_unet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import sd_oracle as SO  # noqa: E402
from sd_video_gen_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

# the reduced networks of test_sd_gpu.py::test_lms_text_to_image_sampler
VCFG = dict(block_out=(64, 128, 128, 128), layers=1, groups=32, latent=4)
UCFG = dict(block_out=(64, 128), layers=1, heads=4, ctx_dim=768, groups=32, in_ch=4, out_ch=4, attn=(1, 0))


@pytest.fixture(scope="module")
def nets():
    """(SDUtils on the reduced networks, UNet state dict, [uncond x2; text x2] embeddings, unit-normal draws (2,4,16,16))"""
    from sd_video_gen_amd import config as svg_config
    from sd_video_gen_amd.sd_utils import SDUtils
    svg_config.set_args(["--dataset", "synthetic-ball", "--config", "model_10_26", "--denoise", "1"])
    vsd, usd = SO.seeded_weights(SO.vae_shapes(VCFG), 3), SO.seeded_weights(SO.unet_shapes(UCFG), 4)
    g = torch.Generator().manual_seed(5)
    emb = torch.randn(4, 77, 768, generator=g)
    lat0 = torch.randn(2, 4, 16, 16, generator=g)
    # prompt_to_img takes its embeddings from the constructor: one prompt, [uncond; text]
    sdu = SDUtils(weights={"vae": vsd, "unet": usd}, arch={"vae": VCFG, "unet": UCFG}, verbose=False, text_embeddings=emb[::2].clone())
    return sdu, usd, emb, lat0


_ORACLE = {}


def oracle_latents(usd, emb, lat0, steps, guidance):
    """SO.denoise_img_latents, computed once per case and never written to"""
    key = (steps, guidance)
    if key not in _ORACLE:
        _ORACLE[key] = SO.denoise_img_latents(usd, emb, lat0.clone(), steps, guidance, cfg=UCFG)
    return _ORACLE[key]


@pytest.mark.parametrize("n,offset", [(2 * 4 * 8 * 8, 0), (1001, 0), (2 * 4 * 8 * 8, 1)])
@pytest.mark.parametrize("alias", [False, True])
def test_lms_step_matches_f64_oracle(ctx, n, offset, alias):
    """steps 0 ... 8 of a 9-step schedule: every order and two wraps of the ring.  n = 512 takes the 16-byte accesses, n = 1001
    (not a multiple of 4) and a latent 4 bytes off a 16-byte boundary the scalar form."""
    steps = 9
    g = torch.Generator().manual_seed(n + offset)
    bufs = [(torch.randn(n + offset, generator=g) * 14.6).cuda(), torch.empty(n + offset, device="cuda")]
    x, spare = bufs[0][offset:], bufs[1][offset:]             # offset 1: both 4 bytes past a 16-byte boundary
    ring = torch.full((4, n), float("nan"), device="cuda")
    want_ring = torch.full((4, n), float("nan"), dtype=torch.float64)
    for i in range(steps):
        _, _, _, order, c = _lib.lms_coefs(steps, i)
        eps = torch.randn(n, generator=g)
        # the oracle: same ring, coefficients from svg_lms_coefs, f64
        want_ring[i & 3] = eps.double()
        terms = [c[k] * want_ring[(i - k) & 3] for k in range(order)]
        want = x.cpu().double() + sum(terms)
        bound = 16 * 2.0 ** -24 * (x.cpu().double().abs() + sum(t.abs() for t in terms))
        assert x.data_ptr() % 16 == 4 * offset
        before = ring.clone()
        xin = x.cpu().double()
        got = ctx.lms_step(x, eps.cuda(), ring, steps, i, out=x if alias else spare)
        err = (got.cpu().double() - want).abs()
        print("n %d offset %d alias %d step %d order %d: max err / bound = %.3f" % (n, offset, alias, i, order, float((err / bound).max())))
        assert bool((err <= bound).all()), (i, float((err / bound).max()))
        # the ring: slot i & 3 holds this step's eps, the other three are untouched (NaN where never written)
        assert torch.equal(ring[i & 3].cpu(), eps)
        for k in range(1, 4):
            s = (i - k) & 3
            assert torch.equal(ring[s].isnan(), before[s].isnan()) and torch.equal(ring[s].nan_to_num(), before[s].nan_to_num())
        if not alias:
            assert torch.equal(x.cpu().double(), xin)           # the input is left alone
            x, spare = got, x
    with pytest.raises(ValueError):
        ctx.lms_step(x, eps.cuda(), ring, steps, steps)


@pytest.mark.parametrize("steps", [6, 9])
@pytest.mark.parametrize("guidance", [7.5, 0.0])
def test_lms_loop_matches_oracle_and_host_loop(nets, steps, guidance):
    sdu, usd, emb, lat0 = nets
    want = oracle_latents(usd, emb, lat0, steps, guidance)
    kw = dict(height=128, width=128, num_inference_steps=steps, guidance_scale=guidance)
    lib = sdu.denoise_img_latents(emb, latents=lat0.clone(), in_library=True, **kw).cpu()
    host = sdu.denoise_img_latents(emb, latents=lat0.clone(), in_library=False, **kw).cpu()
    e_lib, e_host = rel_l2(lib, want), rel_l2(host, want)
    print("LMS %d steps, guidance %g: library loop rel-L2 %.3e, host loop rel-L2 %.3e" % (steps, guidance, e_lib, e_host))
    assert torch.isfinite(lib).all()
    # measured (fp16 UNet), library / host: 6 steps 2.018e-3 / 2.022e-3 guided, 2.955e-4 / 2.955e-4 unguided; 9 steps 1.604e-3 / 1.623e-3
    # guided, 2.496e-4 / 2.492e-4 unguided
    margin("LMS in the library, %d steps at guidance %g (tiny UNet)" % (steps, guidance), e_lib, NET_TOL)
    assert e_lib <= 1.5 * e_host, (e_lib, e_host)
    # the same call through the context, and the history of the direct-launch path: scaled draws first, the result last
    c = sdu.unet.ctx
    hist = c.sample_loop(lat0.cuda(), emb.cuda(), sampler="lms", num_steps=steps, guidance=guidance, return_hist=True).cpu()
    assert hist.shape == ((steps + 1) * 2, 4, 16, 16)
    assert rel_l2(hist[:2], lat0 * _lib.lms_coefs(steps, 0)[1]) < 1e-6
    assert torch.equal(hist[-2:], lib)


@pytest.mark.parametrize("guidance,N", [(7.5, 2), (0.0, 3), (7.5, 3), (0.0, 2)])
def test_lms_graph_replay_equals_direct_launches(ctx, monkeypatch, guidance, N):
    """the captured LMS step (input scale, ring slot, order and coefficients through the device counter) replays to the bits of
    the direct launches; the history of the direct path ends in the same bits"""
    cfg = TINY_UNET
    load_unet(ctx, cfg, 29)
    g = torch.Generator().manual_seed(7)
    h, L = 16, 9
    lat = torch.randn(N, 4, h, h, generator=g).cuda()
    emb = torch.randn(2 * N, L, cfg["ctx_dim"], generator=g).cuda()
    kw = dict(sampler="lms", num_steps=9, guidance=guidance)
    ref = ctx.sample_loop(lat, emb, **kw)                  # null stream: direct launches
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    outs = {}
    for mode in ("1", "0", "1"):
        monkeypatch.setenv("SVG_DDIM_GRAPH", mode)
        _lib.env_refresh()
        with torch.cuda.stream(side):
            outs.setdefault(mode, []).append(ctx.sample_loop(lat, emb, **kw))
        side.synchronize()
    assert torch.equal(outs["1"][0], outs["0"][0]) and torch.equal(outs["1"][1], outs["0"][0])
    assert torch.equal(outs["1"][0], ref)
    assert torch.isfinite(ref).all()
    with torch.cuda.stream(side):
        hist = ctx.sample_loop(lat, emb, return_hist=True, **kw)
    side.synchronize()
    assert torch.equal(hist[-N:], ref)


def test_lms_workspace_is_planned_and_planning_launches_nothing(nets):
    sdu, usd, emb, lat0 = nets
    c = sdu.unet.ctx
    kw = dict(height=128, width=128, num_inference_steps=9, guidance_scale=7.5, in_library=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                           # a capturable stream: the graph path
        a = sdu.denoise_img_latents(emb, latents=lat0.clone(), **kw)
        side.synchronize()
        g1, b1 = c.workspace_growths(), c.workspace_bytes()
        b = sdu.denoise_img_latents(emb, latents=lat0.clone(), **kw)
        side.synchronize()
    assert c.workspace_growths() == g1 and c.workspace_bytes() == b1
    assert torch.isfinite(a).all() and torch.equal(a, b)
    # a loop inside a planning window records its need and launches nothing
    z = lat0.cuda()
    with c.planning():
        out = c.sample_loop(z, emb.cuda(), sampler="lms", num_steps=9, guidance=7.5)   # a copy of z, unwritten
    torch.cuda.synchronize()
    assert torch.equal(out, z)


def test_lms_default_is_untouched(nets, monkeypatch):
    sdu, usd, emb, lat0 = nets
    kw = dict(height=128, width=128, num_inference_steps=6, guidance_scale=7.5)
    # SVG_LMS_LOOP unset: the host loop, bit for bit; it is read at each call
    monkeypatch.delenv("SVG_LMS_LOOP", raising=False)
    host = sdu.denoise_img_latents(emb, latents=lat0.clone(), in_library=False, **kw)
    assert torch.equal(sdu.denoise_img_latents(emb, latents=lat0.clone(), **kw), host)
    lib = sdu.denoise_img_latents(emb, latents=lat0.clone(), in_library=True, **kw)
    monkeypatch.setenv("SVG_LMS_LOOP", "1")
    assert torch.equal(sdu.denoise_img_latents(emb, latents=lat0.clone(), **kw), lib)
    monkeypatch.setenv("SVG_LMS_LOOP", "0")
    assert torch.equal(sdu.denoise_img_latents(emb, latents=lat0.clone(), **kw), host)
    assert not torch.equal(lib, host)
    # the other samplers share the table, the counter and the K / V^T cache with an LMS call on the same context: same bits around it
    c = sdu.unet.ctx
    z, e = (lat0 * 0.5).cuda(), emb.cuda()
    noise = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(9)).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())

    def others():
        with torch.cuda.stream(side):                       # a capturable stream: the graph path
            r = [c.sample_loop(z, e, sampler=s, num_steps=50, start_step=45, guidance=gd, noise=noise)
                 for s in ("ddim", "dpmpp_2m") for gd in (7.5, 0.0)]
        side.synchronize()
        return r
    before = others()
    with torch.cuda.stream(side):
        c.sample_loop(lat0.cuda(), e, sampler="lms", num_steps=9, guidance=7.5)
    side.synchronize()
    after = others()
    assert all(torch.equal(a, b) for a, b in zip(before, after))


def test_lms_bad_arguments_leave_the_context_usable(nets):
    sdu, usd, emb, lat0 = nets
    c = sdu.unet.ctx
    good = c.sample_loop(lat0.cuda(), emb.cuda(), sampler="lms", num_steps=6, guidance=7.5)
    with pytest.raises(ValueError, match="start_step"):
        c.sample_loop(lat0.cuda(), emb.cuda(), sampler="lms", num_steps=6, start_step=1, guidance=7.5, noise=lat0.cuda())
    with pytest.raises(ValueError):
        sdu.gen_i2i_latents(emb, 128, 128, 6, 7.5, lat0, start_step=0, sampler="lms")
    assert torch.equal(c.sample_loop(lat0.cuda(), emb.cuda(), sampler="lms", num_steps=6, guidance=7.5), good)


def test_lms_public_surface(nets):
    sdu, usd, emb, lat0 = nets
    imgs = sdu.prompt_to_img(["a photo"], height=128, width=128, num_inference_steps=3, latents=lat0[:1].clone(), in_library=True)
    assert imgs.shape == (1, 128, 128, 3) and imgs.dtype.name == "uint8"
    host = sdu.prompt_to_img(["a photo"], height=128, width=128, num_inference_steps=3, latents=lat0[:1].clone(), in_library=False)
    assert host.shape == imgs.shape
