"""What the frame-metrics tests share (no test in here): the fp64 judge of svg_frame_metrics, a float32 emulation of the kernel's
arithmetic order, the input set, and the two tolerances.

Tolerances.  The error of an f32 SSIM map comes from the cancellation in G*a^2 - mu^2 against C2 = 58.5.  Float32 emulations measured on
the CPU against the judge over exactly the input set below: plain f32 2.6e-4 worst map element (the ramp at 64^2 and 128^2) and 4.4e-6
worst image mean; f32 on pixels shifted by 128 (what the kernel does) 6.3e-5 and 2.0e-5 (the single-position 11x11 ramp).  The bounds are
4x the worse figure of each column — the factor allows for the kernel's different summation order and FMA contraction:
MAP_TOL = 1e-3 absolute per map element, MEAN_TOL = 8e-5 absolute per image mean.  A wrong tap, a halo off by one or a transposed tile
moves the map of a random pair (spread over about [-0.5, 0.5]) by 1e-2 or more."""
import numpy as np

MAP_TOL = 1e-3
MEAN_TOL = 8e-5
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2          # 6.5025, 58.5225


def taps():
    x = np.arange(-5, 6, dtype=np.float64)
    g = np.exp(-x * x / (2 * 1.5 * 1.5))
    return g / g.sum()


def _valid_filter(x, g, axis):
    """11-tap valid correlation along `axis` (the window is symmetric: correlation == convolution), sequential accumulation in x.dtype"""
    n = x.shape[axis] - 10
    acc = np.zeros_like(np.take(x, range(n), axis=axis))
    for k in range(11):
        acc = acc + g[k] * np.take(x, range(k, k + n), axis=axis)
    return acc


def judge(a, b):
    """a, b uint8 (..., H, W, 3) -> (sse int64 (...), ssim float64 (...), map float64 (..., H-10, W-10, 3)): the definition, in fp64"""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    g = taps()
    G = lambda x: _valid_filter(_valid_filter(x, g, -2), g, -3)      # noqa: E731  (W, then H)
    mu_a, mu_b = G(a64), G(b64)
    var_a, var_b, cov = G(a64 * a64) - mu_a * mu_a, G(b64 * b64) - mu_b * mu_b, G(a64 * b64) - mu_a * mu_b
    m = ((2 * mu_a * mu_b + C1) * (2 * cov + C2)) / ((mu_a * mu_a + mu_b * mu_b + C1) * (var_a + var_b + C2))
    d = a.astype(np.int64) - b.astype(np.int64)
    return (d * d).sum(axis=(-3, -2, -1)), m.mean(axis=(-3, -2, -1)), m


def emulate_f32(a, b, shift=128):
    """the kernel's arithmetic in numpy float32: pixels minus `shift`, the horizontal then the vertical 11-tap pass of a, b, a^2, b^2, ab by
    sequential accumulation, the map value in f32 (every operation rounds, where the GPU contracts some into FMAs), its sum in double"""
    f = np.float32
    u, v = (a.astype(np.int32) - shift).astype(f), (b.astype(np.int32) - shift).astype(f)
    g = taps().astype(f)
    G = lambda x: _valid_filter(_valid_filter(x, g, -2), g, -3)      # noqa: E731
    s0, s1, s2, s3, s4 = G(u), G(v), G(u * u), G(v * v), G(u * v)
    var_a, var_b, cov = s2 - s0 * s0, s3 - s1 * s1, s4 - s0 * s1
    ma, mb = s0 + f(shift), s1 + f(shift)
    m = ((f(2) * ma * mb + f(C1)) * (f(2) * cov + f(C2))) / ((ma * ma + mb * mb + f(C1)) * (var_a + var_b + f(C2)))
    assert m.dtype == np.float32
    return m.astype(np.float64).mean(axis=(-3, -2, -1)), m


SHAPES = [(1, 11, 11), (3, 11, 11), (2, 12, 13), (1, 42, 42), (2, 27, 43), (1, 43, 75), (2, 64, 64), (1, 128, 128), (1, 96, 160)]
KINDS = ["uniform", "identical", "pm1", "const255", "const0_255", "ramp", "ball"]


def make_pair(kind, N, H, W, seed=0):
    """one input pair (a, b) uint8 (N, H, W, 3); None where the kind does not exist at the shape (ball: the 64^2 and 128^2 frames)"""
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8), rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    if kind == "identical":
        a = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
        return a, a.copy()
    if kind == "pm1":
        a = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
        return a, np.clip(a.astype(np.int32) + rng.integers(-1, 2, a.shape), 0, 255).astype(np.uint8)
    if kind == "const255":
        return np.full((N, H, W, 3), 255, np.uint8), np.full((N, H, W, 3), 255, np.uint8)
    if kind == "const0_255":
        return np.zeros((N, H, W, 3), np.uint8), np.full((N, H, W, 3), 255, np.uint8)
    if kind == "ramp":
        y, x = np.mgrid[0:H, 0:W]
        a = np.broadcast_to((((3 * x + 2 * y) % 256).astype(np.uint8))[None, :, :, None], (N, H, W, 3)).copy()
        return a, np.roll(a, 1, axis=2)
    if kind == "ball":
        if H != W or H not in (64, 128):
            return None
        from sd_video_gen_amd.predict import bouncing_ball_clips
        clips = bouncing_ball_clips(N, H, 2, seed=seed).numpy()
        return np.ascontiguousarray(clips[:, 0]), np.ascontiguousarray(clips[:, 1])
    raise ValueError(kind)


def cases():
    """[(id, N, H, W, kind)] of the whole input set"""
    out = []
    for (N, H, W) in SHAPES:
        for kind in KINDS:
            if kind == "ball" and (H != W or H not in (64, 128)):
                continue
            out.append(("%dx%dx%d-%s" % (N, H, W, kind), N, H, W, kind))
    return out
