"""CPU helpers of the matcher error-bound tests (a plain module, not a conftest): the float64 window statistics the fast
NCC path's listing rule is stated in, a classifier of every NCC output against that rule, and trap frames that put
windows next to each of its thresholds (and cost-volume / photometric pairs next to the census-SAD sign decision).

Listing rule (ncc_prepass.hip: ncc_prepass_kernel; constants in ctd_prepass.h).  For every window of every image (frame
f, channel c; pattern channel c) with n = bs^2 samples, mean m and sum of squared deviations V:
    cval   = f32( f64 sum of the window centred at (H/2, W/2), clamped / n )      one constant per image
    F - 1  = n (m - cval)^2 / V
    listed = F - 1 > kFlagRatio / C   or   sqrt(V) < kDevFloor   or   kFlatRatio n m^2 > V   ("flat", kFlatRatio = 4e-7)
A listed window's outputs are recomputed in the reference's order; every other output of the fast volume is trusted to
|fast - exact| <= 1e-5 |exact| + 1e-6 (C > 1: 1e-5 sum_c |exact_c| + C 1e-6), from the error model
|fast - exact| <~ 7 * 2^-24 * sum_c sqrt(Fa Fb).
Windows follow the reference's clamp rules (ext.h:145-160): rows clamp, and a pattern window's columns are shifted by
the disparity BEFORE they clamp, so the pattern side is indexed by the unclamped column x = w - d; every x at or left
of -(bs - 1 - bs/2) is the same fully clamped window (the left-border run).

The pre-pass decides in f32 (block 9) or from f64 sums, so an output whose windows sit within GUARD (relative) of a
threshold may go either way: the classifier calls it "guard"."""
import numpy as np
import torch
import torch.nn.functional as F

K_FLAG_RATIO = 1.39         # ctd_prepass.h kFlagRatio
K_DEV_FLOOR = 7e-2          # ctd_prepass.h kDevFloor
K_FLAT = 4e-7               # ctd_prepass.h kFlatRatio: flat when kFlatRatio n mean^2 > V
GUARD = 0.015

UNLISTED, GUARDED, LISTED = 0, 1, 2


# ---------------------------------------------------------------------------------------------------------------------
# window statistics and the classifier
# ---------------------------------------------------------------------------------------------------------------------
def _unfold(img, bs, left, right):
    """img [B,H,W] (any float) -> f64 windows [B, n, H, W + left + right - (bs - 1)]: replicate rows, columns padded by
    replicate `left` / `right` (the clamp of an unclamped column)"""
    h = bs // 2
    x = torch.as_tensor(np.ascontiguousarray(img)).to(torch.float64)[:, None]
    x = F.pad(x, (left, right, h, bs - 1 - h), mode="replicate")
    B, _, Hp, Wp = x.shape
    return F.unfold(x, bs).view(B, bs * bs, Hp - bs + 1, Wp - bs + 1)


def centring_constant(img, bs):
    """cval of ncc_prepass_kernel for img [H,W]: the f64 mean of the clamped window at (H/2, W/2), rounded to f32"""
    H, W = img.shape
    h = bs // 2
    rows = np.clip(H // 2 + np.arange(bs) - h, 0, H - 1)
    cols = np.clip(W // 2 + np.arange(bs) - h, 0, W - 1)
    return float(np.float32(np.asarray(img, np.float64)[np.ix_(rows, cols)].sum() / (bs * bs)))


def window_stats(img, bs, left=None, right=None):
    """Per-window f64 statistics of images img [B,H,W] (two-pass: mean, then the sum of squared deviations).
    Default padding: the frame side (columns w = 0 .. W-1).  Returns a dict of [B, H, Wout] arrays: mean, V (sum of
    squared deviations), dev = sqrt(V), f1 = F - 1 relative to each image's cval, flat (kFlatRatio n mean^2 / V, > 1 means
    flat), and cval [B]."""
    h = bs // 2
    left = h if left is None else left
    right = bs - 1 - h if right is None else right
    img = np.asarray(img, np.float32)
    win = _unfold(img, bs, left, right)
    n = bs * bs
    mean = win.mean(1)
    V = ((win - mean[:, None]) ** 2).sum(1)
    cval = torch.tensor([centring_constant(im, bs) for im in img], dtype=torch.float64).view(-1, 1, 1)
    Vs = torch.where(V > 0, V, torch.full_like(V, 1e-300))
    f1 = n * (mean - cval) ** 2 / Vs
    flat = K_FLAT * n * mean ** 2 / Vs
    return {"mean": mean.numpy(), "V": V.numpy(), "dev": V.sqrt().numpy(), "f1": f1.numpy(), "flat": flat.numpy(),
            "cval": cval.view(-1).numpy()}


def pattern_stats(pattern, bs, D):
    """window_stats of the pattern images [C,H,W] over the unclamped columns x = -(D-1) .. W-1 (index x + D - 1)"""
    h = bs // 2
    return window_stats(pattern, bs, left=D - 1 + h, right=bs - 1 - h)


def window_class(st, flag_ratio, guard=GUARD):
    """LISTED / GUARDED / UNLISTED per window of a window_stats dict, against the listing rule with flag_ratio =
    kFlagRatio / C: LISTED when some test is crossed by more than `guard` (relative), UNLISTED when every test is
    passed by more than `guard`, GUARDED otherwise"""
    f1, dev, flat = st["f1"], st["dev"], st["flat"]
    listed = (f1 > flag_ratio * (1 + guard)) | (dev < K_DEV_FLOOR * (1 - guard)) | (flat > 1 + guard)
    safe = (f1 < flag_ratio * (1 - guard)) & (dev > K_DEV_FLOOR * (1 + guard)) & (flat < 1 - guard)
    return np.where(listed, LISTED, np.where(safe, UNLISTED, GUARDED)).astype(np.int8)


def classify(frames, pattern, D, bs, guard=GUARD):
    """frames [N,C,H,W], pattern [C,H,W] -> (cls int8 [N,D,H,W], sqrtF f64 [N,D,H,W], floor f64 [N,C,D,H,W]).
    cls: the largest window class of the 2C windows an output (f, d, h, w) reads (frame f, channel c at column w;
    pattern channel c at column x = w - d).  sqrtF: sum over channels of sqrt(Fa Fb), the error model's factor.  floor:
    per channel, 1e-8 / (sa sb), the relative change of that channel's NCC by the reference denominator's 1e-8
    (ctd_prepass.h: kDevFloor keeps it <= 2.1e-6 on unlisted windows)."""
    frames = np.asarray(frames, np.float32)
    pattern = np.asarray(pattern, np.float32)
    N, C, H, W = frames.shape
    ratio = K_FLAG_RATIO / C
    sa = window_stats(frames.reshape(N * C, H, W), bs, None, None)
    sb = pattern_stats(pattern, bs, D)
    ca = window_class(sa, ratio, guard).reshape(N, C, H, W)
    cb = window_class(sb, ratio, guard)                                # [C, H, W + D - 1]
    fa = np.sqrt(1 + sa["f1"]).reshape(N, C, H, W)
    fb = np.sqrt(1 + sb["f1"])
    # column x = w - d of the pattern planes sits at index w - d + D - 1
    j = (np.arange(W)[None, :] - np.arange(D)[:, None]) + D - 1       # [D, W]
    cbd = cb[:, :, j].transpose(0, 2, 1, 3)                            # [C, D, H, W]
    fbd = fb[:, :, j].transpose(0, 2, 1, 3)
    cls = np.maximum(ca[:, :, None], cbd[None]).max(1)                 # [N, D, H, W]
    sqrtF = (fa[:, :, None] * fbd[None]).sum(1)
    da = np.maximum(sa["dev"], 1e-30).reshape(N, C, H, W)
    db = np.maximum(sb["dev"], 1e-30)[:, :, j].transpose(0, 2, 1, 3)
    floor = 1e-8 / (da[:, :, None] * db[None])                         # [N, C, D, H, W]
    return cls.astype(np.int8), sqrtF, floor


# ---------------------------------------------------------------------------------------------------------------------
# NCC trap frames.  Every generator: gen(seed, N, C, H, W, bs) -> (frames [N,C,H,W] f32, pattern [C,H,W] f32).
# ---------------------------------------------------------------------------------------------------------------------
def _tile(rs, bs, H, W, dev=1.0):
    """a bs x bs random tile repeated over [H,W]: every window away from the clamped borders holds one full period, so
    every such window has the same mean (~0) and the same sum of squared deviations dev^2"""
    t = rs.randn(bs, bs)
    t -= t.mean()
    t *= dev / np.sqrt((t ** 2).sum())
    return np.tile(t, (H // bs + 1, W // bs + 1))[:H, :W]


def _bands(W, width, k):
    """band index (0 .. k-1, cycling) of every column, bands `width` wide"""
    return (np.arange(W) // width) % k


def _shifted(pattern, rs, disp_max, noise):
    """a frame seen at a random disparity per row band: frame[h, w] = pattern[h, w - d(h)] + noise"""
    C, H, W = pattern.shape
    out = np.empty_like(pattern)
    d = rs.randint(0, disp_max, size=H // 8 + 1)
    for h in range(H):
        cols = np.clip(np.arange(W) - d[h // 8], 0, W - 1)
        out[:, h] = pattern[:, h, cols]
    return out + noise * rs.randn(*out.shape)


RATIOS = (0.9, 0.98, 1.02, 1.1)

# (block size, H, W, D) of the GPU suite: block 9 (the f32 pre-pass and the specialised kernels) at W = 516 with
# D = 256, and the generic block sizes at widths that are not multiples of 4
NCC_SHAPES = [(9, 20, 516, 256), (5, 17, 301, 96), (7, 13, 203, 61)]


def trap_seed(bs, H, C):
    """the seed the GPU suite draws a generator's frames with at a shape"""
    return bs * 1000 + H + C


def _staircase_image(rs, H, W, bs, C):
    """DC steps over the tiled texture: band levels put interior windows at F - 1 = kFlagRatio / C * r for r in RATIOS,
    both signs, relative to the level of the centre band (which is 0: cval is then the tile's mean).  Bands are 2 bs
    wide and the centre band is centred on column W / 2, so the centring window lies inside it."""
    img = _tile(rs, bs, H, W, 1.0)
    width = 2 * bs
    levels = [0.0] + [s * np.sqrt(K_FLAG_RATIO / C * r / (bs * bs)) for r in RATIOS for s in (1, -1)]
    band = ((np.arange(W) - (W // 2 - bs)) // width) % len(levels)     # band 0: columns W/2 - bs .. W/2 + bs - 1
    return (img + np.asarray(levels)[band][None, :]).astype(np.float32)


def gen_staircase(seed, N, C, H, W, bs):
    rs = np.random.RandomState(seed)
    pat = np.stack([_staircase_image(rs, H, W, bs, C) for _ in range(C)])
    frames = np.stack([np.stack([_staircase_image(rs, H, W, bs, C) for _ in range(C)]) for _ in range(N)])
    return frames.astype(np.float32), pat.astype(np.float32)


def _devfloor_image(rs, H, W, bs):
    """bands of the tiled texture with window deviation kDevFloor * r, r in RATIOS, on one DC level"""
    width = 2 * bs
    band = _bands(W, width, len(RATIOS))
    img = np.zeros((H, W))
    for k, r in enumerate(RATIOS):
        img[:, band == k] = _tile(rs, bs, H, W, K_DEV_FLOOR * r)[:, band == k]
    return (img + 0.25).astype(np.float32)


def gen_devfloor(seed, N, C, H, W, bs):
    rs = np.random.RandomState(seed)
    pat = np.stack([_devfloor_image(rs, H, W, bs) for _ in range(C)])
    frames = np.stack([np.stack([_devfloor_image(rs, H, W, bs) for _ in range(C)]) for _ in range(N)])
    return frames, pat


def _flat_image(rs, H, W, bs, level=200.0):
    """a large mean with a tiny variance: bands with V = kFlatRatio n level^2 / r (kFlatRatio n mean^2 / V = r), r in RATIOS; the
    deviation stays above kDevFloor and every band has the same mean (F - 1 ~ 0): only the flat test decides"""
    n = bs * bs
    width = 2 * bs
    band = _bands(W, width, len(RATIOS))
    img = np.zeros((H, W))
    for k, r in enumerate(RATIOS):
        img[:, band == k] = _tile(rs, bs, H, W, np.sqrt(K_FLAT * n * level ** 2 / r))[:, band == k]
    return (img + level).astype(np.float32)


def gen_flat(seed, N, C, H, W, bs, level=200.0):
    rs = np.random.RandomState(seed)
    pat = np.stack([_flat_image(rs, H, W, bs, level) for _ in range(C)])
    frames = np.stack([np.stack([_flat_image(rs, H, W, bs, level) for _ in range(C)]) for _ in range(N)])
    return frames, pat


# the flat clause exists for the rounding of the window mean, ulp(mean) / mean, which runs from 2^-23 just above a power
# of two down to 2^-24 just below the next: levels across the binade [128, 256)
FLAT_LEVELS = {"flat": 200.0, "flat128": 128.25, "flat181": 181.0, "flat255": 255.0}


def _flat_gen(level):
    def g(seed, N, C, H, W, bs):
        return gen_flat(seed, N, C, H, W, bs, level)
    return g


def _ramp(rs, H, W, axis):
    """texture under an illumination ramp along `axis` (1: columns, 0: rows): gain 0.05 .. 2, offset 0 .. 40"""
    tex = rs.rand(H, W)
    t = np.linspace(0, 1, W)[None, :] if axis == 1 else np.linspace(0, 1, H)[:, None]
    return ((0.05 + 1.95 * t) * tex + 40 * t).astype(np.float32)


def gen_ramp_h(seed, N, C, H, W, bs):
    rs = np.random.RandomState(seed)
    pat = np.stack([_ramp(rs, H, W, 1) for _ in range(C)])
    frames = np.stack([_shifted(pat, rs, 64, 1e-2) * 1.1 + 0.5 for _ in range(N)])
    return frames.astype(np.float32), pat


def gen_ramp_v(seed, N, C, H, W, bs):
    rs = np.random.RandomState(seed)
    pat = np.stack([_ramp(rs, H, W, 0) for _ in range(C)])
    frames = np.stack([_shifted(pat, rs, 64, 1e-2) for _ in range(N)])
    return frames.astype(np.float32), pat


def gen_dots(seed, N, C, H, W, bs):
    """dots on black (10 % of the pixels 1, the rest 0) with sensor noise: dot-free windows hold noise only"""
    rs = np.random.RandomState(seed)
    pat = (rs.rand(C, H, W) < 0.1).astype(np.float64)
    frames = np.stack([_shifted(pat, rs, 64, 1e-3) for _ in range(N)])
    return frames.astype(np.float32), pat.astype(np.float32)


def _clipped(rs, H, W, top):
    """a smooth field plus texture, clipped to [0, top]: plateaus of exact 0 and exact `top`"""
    y, x = np.mgrid[0:H, 0:W]
    field = np.sin(x / 23.0 + rs.rand() * 6) * np.cos(y / 17.0 + rs.rand() * 6) * 1.6 + 0.5
    return np.clip((field + 0.3 * rs.rand(H, W)) * top, 0, top)


def gen_clipped(seed, N, C, H, W, bs, top=1.0):
    rs = np.random.RandomState(seed)
    pat = np.stack([_clipped(rs, H, W, top) for _ in range(C)])
    frames = np.stack([np.clip(_shifted(pat, rs, 64, 0), 0, top) for _ in range(N)])
    return frames.astype(np.float32), pat.astype(np.float32)


def gen_clipped255(seed, N, C, H, W, bs):
    return gen_clipped(seed, N, C, H, W, bs, top=255.0)


def gen_scaled(seed, N, C, H, W, bs, k=0):
    """one uniform texture (and its shifted, noisy view) scaled by 10^k"""
    rs = np.random.RandomState(seed)
    pat = rs.rand(C, H, W)
    frames = np.stack([_shifted(pat, rs, 64, 0.05) for _ in range(N)])
    s = 10.0 ** k
    return (frames * s).astype(np.float32), (pat * s).astype(np.float32)


def gen_chan_scale(seed, N, C, H, W, bs):
    """channels of the same scene whose scales differ by 1e3 each"""
    rs = np.random.RandomState(seed)
    pat = rs.rand(C, H, W) * (1e3 ** np.arange(C))[:, None, None]
    frames = np.stack([_shifted(pat, rs, 64, 0) * (1 + 0.05 * rs.randn(C, H, W)) for _ in range(N)])
    return frames.astype(np.float32), pat.astype(np.float32)


def gen_chan_cancel(seed, N, C, H, W, bs):
    """per-channel NCCs that nearly cancel: the frame's channels are one texture, the pattern's are +texture, -texture
    (and +texture again for C = 3, the third against a texture of its own) -- their sum leaves ~ the 1e-6 term"""
    rs = np.random.RandomState(seed)
    tex = rs.rand(H, W)
    sign = np.array([1.0, -1.0, 1.0][:C])[:, None, None]
    pat = sign * tex[None] + 1e-4 * rs.randn(C, H, W)
    if C == 3:
        pat[2] = rs.rand(H, W)
    frames = []
    for _ in range(N):
        f = _shifted(tex[None], rs, 64, 0)[0]
        frames.append(np.stack([f + 1e-4 * rs.randn(H, W) for _ in range(C)]))
    return np.stack(frames).astype(np.float32), pat.astype(np.float32)


def _scale_gen(k):
    def g(seed, N, C, H, W, bs):
        return gen_scaled(seed, N, C, H, W, bs, k)
    return g


NCC_GENERATORS = {
    "staircase": gen_staircase, "devfloor": gen_devfloor, "ramp_h": gen_ramp_h, "ramp_v": gen_ramp_v,
    "dots": gen_dots, "clipped": gen_clipped, "clipped255": gen_clipped255,
}
NCC_GENERATORS.update({name: _flat_gen(level) for name, level in FLAT_LEVELS.items()})
NCC_GENERATORS.update({"scale%+d" % k: _scale_gen(k) for k in range(-3, 4)})
# staircase with C channels: its levels sit at the per-channel threshold kFlagRatio / C
MULTICHANNEL_GENERATORS = {"staircase": gen_staircase, "chan_scale": gen_chan_scale, "chan_cancel": gen_chan_cancel}


# ---------------------------------------------------------------------------------------------------------------------
# cost-volume / photometric traps: gen(seed, N, H, W) -> (im [N,H,W] f32, pattern [H,W] f32)
# ---------------------------------------------------------------------------------------------------------------------
def perturb(rs, x, density=1.0):
    """x (f32) moved per pixel by one of: 0, +-1 ulp, +-1e-6 (1 +- 0.1); a pixel is left alone with probability
    1 - density"""
    x = np.asarray(x, np.float32)
    k = np.where(rs.rand(*x.shape) < density, rs.randint(0, 7, size=x.shape), 0)
    up, dn = np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))
    step = np.choose(np.clip(k - 3, 0, 3), [0.0, 0.9e-6, 1e-6, 1.1e-6]) * rs.choice([-1.0, 1.0], size=x.shape)
    out = np.where(k == 0, x, np.where(k == 1, up, np.where(k == 2, dn, x + step)))
    return out.astype(np.float32)


def cv_ulp(seed, N, H, W, scale=1.0):
    """frames that are the pattern at a disparity, up to 0, +-1 ulp and +-1e-6 (1 +- 0.1) per pixel"""
    rs = np.random.RandomState(seed)
    pat = (rs.rand(H, W) * scale).astype(np.float32)
    ims = np.stack([perturb(rs, _shifted(pat[None], rs, 32, 0)[0]) for _ in range(N)])
    return ims, pat


def cv_dc(seed, N, H, W):
    """texture on DC offsets up to 1e3 (per row band) that differ between the frame and the pattern by < 1"""
    rs = np.random.RandomState(seed)
    dc = np.repeat(10.0 ** rs.uniform(0, 3, size=H // 4 + 1), 4)[:H, None]
    pat = (rs.rand(H, W) + dc).astype(np.float32)
    ims = np.stack([(_shifted(pat[None], rs, 32, 1e-3)[0] + rs.uniform(-0.5, 0.5)).astype(np.float32)
                    for _ in range(N)])
    return ims, pat


COST_GENERATORS = {"ulp": cv_ulp, "ulp_small": lambda s, N, H, W: cv_ulp(s, N, H, W, 1e-2), "dc": cv_dc}


def sign_trap_pair(seed, B, H, W, bs, scale=1.0):
    """(es, ta) [B,1,H,W] with ta = es perturbed by 0, +-1 ulp, +-1e-6 (1 +- 0.1) at a density of 1 / bs^2: census
    differences at or next to zero (every pair with a perturbed end), where the sign of the census-SAD gradient is
    decided, sparse enough that most pixels' gradients take no pair within one ulp of zero"""
    rs = np.random.RandomState(seed)
    es = (rs.rand(B, 1, H, W) * scale).astype(np.float32)
    return es, perturb(rs, es, 1.0 / (bs * bs))
