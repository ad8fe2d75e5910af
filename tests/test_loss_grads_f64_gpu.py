"""Training-loss kernels, values and every gradient, elementwise against float64 stock-torch references
(tests/f64_refs.py) at the shapes the 64 x 4 tiles of losses.hip and the 64 x 8 tiles (9-wide halo) of
photometric_fast.hip and pattern_loss.hip meet in training, including their ragged edges.

Tolerance rule (the same for every case; nothing is tuned per case):
  * every element outside the mask: |hip - f64| <= r |f64| + a max|f64| + p, with r = 1e-5, a = 2e-5;
  * p = 0 except where an f32 sampling coordinate conditions the result: then p = delta_pos * L, delta_pos the
    rounding distance of the f32 coordinate (derived at POS_ULPS below) and L the f64 Lipschitz constant of the
    checked output under a shift of all sampling positions, measured by finite differences of the f64 reference;
  * the HIP maximum error (unmasked elements) is at most 1.25 x the error of the same composition run in stock-torch
    f32, + 4e-7 max|f64| (the self-calibration of tests/test_f64_arbitration_gpu.py);
  * values: the same rule on the scalar (a = 0);
  * no fraction-of-bad-elements and no mean-only bounds.
A mask excludes only elements whose gradient is discontinuous within rounding distance of the inputs; it is computed
from the f64 intermediates (never from the comparison), its size is printed and capped per case, and masked elements
must still be finite.  The discontinuities: a census / SAD pair difference at 0 (sign), an unnormalised sampling
coordinate at an integer or at the clip borders 0 / W-1 (bilinear cell, clip), a geometric |d - sample| at the clamp
or d - sample at 0, pdf at the 1e-4 clamp, g at 1 (no-edge clamp), and depth pixels receiving bilinear scatter from a
masked source."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import f64_refs as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24                 # unit roundoff of f32
RT, AT = 1e-5, 2e-5
CAP = 1e-3                       # default cap of the masked fraction
# rounding distance of the f32 sampling coordinates, in units of EPS * max(W, H):
#  geometric: depth * ray, two 3x3 rotations, K, the divide and the 4-step normalisation, ~12 roundings at magnitudes
#  up to W (emulating the kernel's chain in numpy f32 gives at most 3.9 at 480 x 640): 6;
#  pattern warp: x - disp, / (W-1), - 0.5, * 2, + 1, * W, - 1, / 2, each at magnitude <= W (measured <= 2.1): 3
POS_ULPS_GEO, POS_ULPS_PAT = 6.0, 3.0
# census_sad: a pixel's gradient sums the signs of the 80 pairs it centres and the 80 it is the tap of; each pair lies
# within its rounding distance (~0.71 * 2 * 1e-4 at 512 wide) of 0 with probability ~1e-3, so ~15 % of the pixels
# touch such a pair at 432 x 512, and a few % at 40 wide (printed per case)
CENSUS_CAP = 0.3


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def te():
    from connecting_the_dots_amd import torchext
    return torchext


def check(what, hip, f64, f32=None, mask=None, pos=0.0, cap=CAP, a=AT, extra_masked=0, cal=0.0):
    """the module docstring's rule for one output; pos: the derived conditioning term (absolute, scalar or per
    element); extra_masked: elements one masked source may mask beyond the fraction `cap`; cal: added to the f32
    cross-check's floor where the two sides sum in different orders (float atomics)"""
    hip = hip.detach().double()
    f64 = f64.detach().double().to(hip.device)
    assert hip.shape == f64.shape, (what, hip.shape, f64.shape)
    assert torch.isfinite(hip).all(), what
    keep = torch.ones_like(f64, dtype=torch.bool) if mask is None else ~mask.to(hip.device)
    n, n_masked = f64.numel(), int((~keep).sum())
    scale = float(f64[keep].abs().max()) if bool(keep.any()) else 0.0
    err = (hip - f64).abs()
    pos = pos.to(hip.device) if torch.is_tensor(pos) else pos
    bound = RT * f64.abs() + a * scale + pos
    pmax = float(pos.max()) if torch.is_tensor(pos) else pos
    worst = float(((err - bound)[keep]).max()) if bool(keep.any()) else -1.0
    eh = float(err[keep].max()) if bool(keep.any()) else 0.0
    ef = float((f32.detach().double().to(hip.device) - f64).abs()[keep].max()) if f32 is not None and bool(keep.any()) else None
    print("%-58s n=%-9d masked=%-6d (cap %d)  max err %.3e  scale %.3e  pos %.2e  f32 err %s" % (
        what, n, n_masked, math.ceil(cap * n) + extra_masked, eh, scale, pmax, "%.3e" % ef if ef is not None else "-"))
    assert n_masked <= math.ceil(cap * n) + extra_masked, (what, "masked", n_masked, n)
    if worst > 0:
        i = int(torch.argmax(torch.where(keep, err - bound, torch.full_like(err, -1e300))))
        idx = np.unravel_index(i, tuple(f64.shape))
        raise AssertionError("%s: max |hip - f64| %.3e over the bound at %s: hip %.9e f64 %.9e bound %.3e" % (
            what, eh, idx, float(hip.flatten()[i]), float(f64.flatten()[i]), float(bound.flatten()[i])))
    if ef is not None and n >= 64:      # (the maximum of fewer elements is a single rounding draw on either side)
        assert eh <= 1.25 * ef + 4e-7 * scale + cal, (what, "HIP error above 1.25 x stock-torch f32's", eh, ef)


def check_value(what, hip, f64, f32=None, pos=0.0):
    pos = float(pos)
    check(what, torch.as_tensor(float(hip)).view(1), torch.as_tensor(float(f64)).view(1),
          None if f32 is None else torch.as_tensor(float(f32)).view(1), pos=pos, a=0.0)


def dilate(mask, k):
    """pixels within the k x k window (k odd) of a masked pixel, [B,1,H,W]"""
    return F.max_pool2d(mask.double(), k, stride=1, padding=k // 2) > 0


def near_integer(x, delta):
    return (x - torch.round(x)).abs() <= delta


# ------------------------------------------------------------------------------------------------------------------
# DispToDepth
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 1, 3, 5), (2, 1, 37, 70), (8, 1, 480, 640)])
def test_disp_to_depth_vs_f64(te, shape):
    g = torch.Generator().manual_seed(shape[2] * 7 + shape[3])
    disp = torch.rand(shape, generator=g) * 200 - 20          # ~10 % at or below 0: the relu gate
    disp.view(-1)[0] = 0.0
    go = torch.randn(shape, generator=g)
    d = disp.cuda().requires_grad_(True)
    depth = te.DispToDepth(567.6, 0.075)(d)
    depth.backward(go.cuda())
    bf = 567.6 * 0.075
    ref = R.disp_to_depth(disp, bf, go)
    f32 = R.disp_to_depth(disp, bf, go, dtype=torch.float32)
    # the relu gate: 1e12 * bf where disp <= 0; elementwise relative check there and everywhere else
    check("d2d depth %s" % (shape,), depth, ref.value, f32.value, a=0.0)
    check("d2d grad %s" % (shape,), d.grad, ref.grads["disp"], f32.grads["disp"], a=0.0)


# ------------------------------------------------------------------------------------------------------------------
# Sobel + DisparityLoss
# ------------------------------------------------------------------------------------------------------------------
DL_SHAPES = [(1, 1, 1), (1, 2, 3), (2, 3, 5), (1, 4, 64), (1, 5, 65), (2, 9, 63), (3, 37, 70), (2, 60, 80),
             (2, 120, 160), (8, 480, 640)]


def disparity_input(B, H, W, seed):
    """disparities with steep ramps (|grad| ~ 20 per pixel: pdf below the 1e-4 clamp, g > 1), flat patches (g on its
    sqrt(1e-8) floor) and gentle noise, bounded by ~200 so the f32 Sobel sums round at <= ulp(256)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W)
    y = torch.arange(H, dtype=torch.float64).view(1, 1, H, 1)
    tri = 20.0 * (x % 10 - 5).abs()                                  # steep sawtooth, slope 20
    smooth = 5 + 3 * torch.sin(x / 7.0) + 2 * torch.cos(y / 5.0)    # slopes < 1
    disp = torch.where((x // 10 + y // 6) % 3 == 0, tri, smooth).expand(B, 1, H, W).clone()
    disp += 0.05 * torch.rand(B, 1, H, W, generator=g, dtype=torch.float64)
    flat = ((x // 8 + y // 8) % 4 == 1).expand(B, 1, H, W)
    disp[flat] = 7.0                                                  # exactly flat patches
    return disp.float(), torch.rand(B, 1, H, W, generator=g), torch.randn(B, 1, H, W, generator=g) * 3


def disparity_masks(ref, edge):
    """(grad_disp mask, grad_edge mask): pdf within rounding distance of the clamp / g of 1, and for grad_disp the
    5 x 5 window of such pixels (the transposed Sobel gathers ggx, ggy of the neighbours).  delta_g: 25 f32 fmas over
    terms bounded by sum |k| |disp|, <= 16 EPS (sum |k| |disp| + g) at the sqrt."""
    inter = ref.inter
    dg = 16 * EPS * (inter["sobel_abs"] + inter["g"])
    if edge:
        # d log pdf / d g <= 1 / B0; log, exp, the mixture: 16 EPS
        bad = (torch.log(inter["pdf"] / R.PDF_MIN)).abs() <= dg / R.B0 + 16 * EPS
    else:
        bad = (inter["g"] - 1).abs() <= dg
    return dilate(bad, 5), bad


@pytest.mark.parametrize("shape", DL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", ["edge", "noedge", "logits"])
def test_disparity_loss_vs_f64(te, shape, mode):
    B, H, W = shape
    disp, edge, logits = disparity_input(B, H, W, seed=B * 1000 + H * 10 + W)
    d = disp.cuda().requires_grad_(True)
    kw, kw32 = {}, {}
    if mode == "edge":
        e = edge.cuda().requires_grad_(True)
        val = te.disparity_loss(d, e)
        kw = {"edge": edge}
    elif mode == "logits":
        lg = logits.cuda().requires_grad_(True)
        e = 1 - torch.sigmoid(lg)                       # the trainer's edge (train.py)
        e.retain_grad()
        val = te.disparity_loss(d, e)
        # the kernel's input is the f32 edge; 1 - sigmoid in f32 is torch's (its rounding is not the kernel's)
        kw = {"edge": e.detach().cpu()}
    else:
        val = te.disparity_loss(d)
    (val * 1.5).backward()                              # a non-unit upstream gradient
    ref = R.disparity_loss(disp, **kw)
    f32 = R.disparity_loss(disp.cuda(), **{k: v.cuda() for k, v in kw.items()}, dtype=torch.float32)
    tag = "disparity %s %dx%dx%d" % (mode, B, H, W)
    mdisp, medge = disparity_masks(ref, mode != "noedge")
    # f32 conditioning: the Sobel sums of the f32 disparities round at delta_g = 16 EPS (sum |k| |disp| + g); the
    # value moves by sum |dL/dg| delta_g, and the direction gx / g of d/d gx by delta_g / g (large where g sits near
    # its 1e-4 floor), which the transposed filter (sum |kx| + |ky| = 1.4) gathers from the 5 x 5 neighbours
    dg = 16 * EPS * (ref.inter["sobel_abs"] + ref.inter["g"])
    pv = float((ref.inter["dLdg"].abs() * dg).sum())
    pggx = ref.inter["dLdg"].abs() * dg / ref.inter["g"]
    pd = 1.4 * F.max_pool2d(pggx, 5, stride=1, padding=2)
    check_value(tag + " value", val, ref.value, f32.value, pos=pv)
    # (a pixel at a kink masks its 5 x 5 neighbours)
    check(tag + " d/d disp", d.grad, 1.5 * ref.grads["disp"], 1.5 * f32.grads["disp"], mdisp, pos=1.5 * pd,
          cap=25 * CAP)
    if mode == "edge":
        check(tag + " d/d edge", e.grad, 1.5 * ref.grads["edge"], 1.5 * f32.grads["edge"], medge)
    elif mode == "logits":
        check(tag + " d/d edge", e.grad, 1.5 * ref.grads["edge"], 1.5 * f32.grads["edge"], medge)


# ------------------------------------------------------------------------------------------------------------------
# Geometric loss (symmetric forward in one launch, the two backward launches)
# ------------------------------------------------------------------------------------------------------------------
def camera(H, W):
    K = np.array([[0.9 * W, 0, W / 2.0 - 0.3], [0, 0.92 * W, H / 2.0 + 0.2], [0, 0, 1]], np.float32)
    return K, np.linalg.inv(K.astype(np.float64)).astype(np.float32)


def pose(B, rs, kind):
    R0 = np.stack([np.eye(3, dtype=np.float32)] * B)
    R1 = R0.copy()
    R1[:, 0, 1], R1[:, 1, 0] = 0.01, -0.01
    t0 = (rs.randn(B, 3) * 0.02).astype(np.float32)
    t1 = (rs.randn(B, 3) * 0.02).astype(np.float32)
    if kind == "out":                     # a sideways translation: >= 20 % of the points leave the frame
        t1[:, 0] += 0.6
        t1[:, 1] -= 0.3
    elif kind == "behind":                # a step along the axis past the near patch of depth0: d <= 0 there
        t1[:, 2] -= 1.0
    return R0, t0, R1, t1


def geometric_masks(ref, H, W, clamp, mag):
    """(mask depth0, mask depth1, fraction of sources masked).  A source (pixel of one direction) is masked where
    ix / iy lie within delta_pos of an integer (bilinear cell; the clip borders 0 and W-1 are integers), where d -
    sample lies within delta_e of 0 (sign) or |d - sample| within delta_e of the clamp; delta_e: d and the sample are
    8-rounding f32 values, 16 EPS (|d| + |sample|), plus the sample's shift under delta_pos (depth slope <= the
    largest neighbour difference of the sampled depth map, max_slope).  Its own depth pixel and every depth pixel of
    the other map its bilinear scatter may reach (cells floor(ix +- delta)) are masked."""
    delta = POS_ULPS_GEO * EPS * max(W, H)
    masks = {0: None, 1: None}
    frac = []
    for dname, own, other in (("fwd", 0, 1), ("rev", 1, 0)):
        it = ref.inter[dname]
        ix, iy, e = it["ix"], it["iy"], it["e"]
        inside_x = (ix > -delta) & (ix < W - 1 + delta)
        inside_y = (iy > -delta) & (iy < H - 1 + delta)
        src = (near_integer(ix, delta) & inside_x) | (near_integer(iy, delta) & inside_y)
        # d is a sum of terms of magnitude <= mag and carries ~4 EPS mag; u = uvd / d inherits 4 EPS mag |u| / |d|,
        # inside delta (measured) while |d| is within a few x of mag, but not once d has cancelled to below mag / 16
        # near the camera plane: there the cell is not fixed by the f32 inputs
        src |= (it["d"].abs() < mag / 16) & (inside_x | inside_y)
        x0 = ix.clamp(0, W - 1).round().long()
        y0 = iy.clamp(0, H - 1).round().long()
        bi = torch.arange(ix.shape[0], device=ix.device).view(-1, 1, 1, 1).expand_as(x0)
        de = 16 * EPS * (it["d"].abs() + it["sample"].abs()) + delta * it["slope"][bi, 0, y0, x0]
        src |= e.abs() <= de
        if clamp > 0:
            src |= (it["diff"] - clamp).abs() <= de
        frac.append(float(src.double().mean()))
        own_m = src.clone()
        tgt = torch.zeros_like(src)
        b, _, hh, ww = torch.nonzero(src, as_tuple=True)
        if b.numel():
            cx = ix[src].clamp(0, W - 1)
            cy = iy[src].clamp(0, H - 1)
            for ox in (-delta, delta):
                for oy in (-delta, delta):
                    x0 = torch.floor((cx + ox).clamp(0, W - 1)).long()
                    y0 = torch.floor((cy + oy).clamp(0, H - 1)).long()
                    for sx in (0, 1):
                        for sy in (0, 1):
                            tgt[b, 0, (y0 + sy).clamp(max=H - 1), (x0 + sx).clamp(max=W - 1)] = True
        masks[own] = own_m if masks[own] is None else masks[own] | own_m
        masks[other] = tgt if masks[other] is None else masks[other] | tgt
    return masks[0], masks[1], max(frac)


def depth_slope(depth):
    """per pixel of a depth map: largest |x| plus largest |y| neighbour difference of the 3 x 3 cells around it"""
    return pattern_slope(depth)


def geometric_case(te, B, H, W, kind, clamp, seed):
    rs = np.random.RandomState(seed)
    K, Ki = camera(H, W)
    R0, t0, R1, t1 = pose(B, rs, kind)
    depth0 = (1.0 + rs.rand(B, 1, H, W) * 2.0).astype(np.float32)
    if kind == "behind":
        depth0 += 1.0
        depth0[:, :, H // 4: H // 2 + 1, W // 4: W // 2 + 1] = 0.5 + 0.45 * rs.rand(B, 1, H // 2 - H // 4 + 1,
                                                                                    W // 2 - W // 4 + 1)
    depth1 = (depth0 + rs.randn(B, 1, H, W).astype(np.float32) * 0.08).astype(np.float32)   # diffs straddle 0.1
    mod = te.ProjectionDepthSimilarityLoss(torch.from_numpy(K), torch.from_numpy(Ki), H, W, clamp=clamp)
    ray = mod.ray.clone()
    a, b = cuda(depth0).requires_grad_(True), cuda(depth1).requires_grad_(True)
    val = mod(a, b, cuda(R0), cuda(t0), cuda(R1), cuda(t1))
    (val * 0.75).backward()
    args = [cuda(x) for x in (depth0, depth1, K)] + [ray.cuda()] + [cuda(x) for x in (R0, t0, R1, t1)]
    ref = R.geometric_loss(*args, clamp)
    f32 = R.geometric_loss(*args, clamp, dtype=torch.float32)
    ref.inter["fwd"]["slope"] = depth_slope(args[1].double())
    ref.inter["rev"]["slope"] = depth_slope(args[0].double())
    tag = "geometric %s c=%g %dx%dx%d" % (kind, clamp, B, H, W)
    mag = max(float(args[0].abs().max()), float(args[1].abs().max())) + float(args[5].abs().max()) + \
        float(args[7].abs().max())
    m0, m1, frac = geometric_masks(ref, H, W, clamp, mag)
    fi = ref.inter["fwd"]
    out = float(((fi["ix"] < 0) | (fi["ix"] > W - 1) | (fi["iy"] < 0) | (fi["iy"] > H - 1)).double().mean())
    # position conditioning: each source's sample moves by <= delta_pos * slope; the gradients are piecewise linear in
    # the sampling position with slope (f64, finite difference of the reference under a shift of K's principal point)
    delta = POS_ULPS_GEO * EPS * max(W, H)
    # (a step h = delta / 4 < delta crosses no unmasked kink)
    h = delta / 4
    Ks = args[2].double().clone()
    Ks[0, 2] += h
    Ks[1, 2] += h
    shifted = R.geometric_loss(args[0], args[1], Ks, *args[3:], clamp)
    pos = {}
    for name, m in (("depth0", m0), ("depth1", m1)):
        lip = ((shifted.grads[name] - ref.grads[name]).abs()[~m].max() / h) if bool((~m).any()) else 0.0
        pos[name] = float(lip) * delta
    # a coordinate lies within delta of an integer with probability 2 delta (x and y), the sign / clamp kinks add
    # delta_e times the density of d - sample (~1 % at 480 x 640 with the rough depth maps here), and a masked source
    # masks itself and <= 9 pixels of the other map (one source at most: extra_masked)
    cap = 0.03
    # float atomics: the scatter into a depth pixel that n sources reach is summed in another order than torch's;
    # orders differ by <= n EPS sum |addend| <= n EPS max|grad| (n from the f64 coordinates)
    # (recursive summation: (n - 1) EPS sum |addend|; the pile-ups are the clipped sources of one side of the frame,
    # whose addends share a sign, so sum |addend| = |f64 gradient| there)
    piles = {}
    for name, it in (("depth1", ref.inter["fwd"]), ("depth0", ref.inter["rev"])):
        x0 = it["ix"].clamp(0, W - 1).floor().long()
        y0 = it["iy"].clamp(0, H - 1).floor().long()
        bi = torch.arange(B, device=x0.device).view(-1, 1, 1, 1).expand_as(x0)
        cnt = torch.zeros(B * H * W, dtype=torch.float64, device=x0.device)
        for sx in (0, 1):
            for sy in (0, 1):
                idx = (bi * H + (y0 + sy).clamp(max=H - 1)) * W + (x0 + sx).clamp(max=W - 1)
                cnt += torch.bincount(idx.reshape(-1), minlength=B * H * W).double()
        piles[name] = cnt.view(B, 1, H, W)
    check_value(tag + " value", val * 0.75, 0.75 * ref.value, 0.75 * f32.value)
    # d carries ~4 EPS mag absolute (above), and the own-source gradient scales as up to 1 / d^2 (the perspective
    # divide): relative 2 * 4 EPS mag / |d|, x 4 for margin
    for name, grad, m in (("depth0", a.grad, m0), ("depth1", b.grad, m1)):
        d_own = ref.inter["fwd" if name == "depth0" else "rev"]["d"].abs()
        pile = piles[name] * EPS * 0.75 * ref.grads[name].abs()
        pile = pile + 32 * EPS * mag / d_own.clamp(min=1e-30) * 0.75 * ref.grads[name].abs()
        check(tag + " d/d " + name, grad, 0.75 * ref.grads[name], 0.75 * f32.grads[name], m, pos=0.75 * pos[name] + pile,
              cap=cap, extra_masked=10, cal=float(pile.max()))
    return out, int((fi["d"] <= 0).sum())


GEO_SHAPES = [(1, 2, 2), (1, 4, 65), (2, 9, 63), (3, 33, 130), (15, 432, 512), (8, 480, 640), (8, 60, 80)]


@pytest.mark.parametrize("clamp", [0.1, -1.0])
@pytest.mark.parametrize("shape", GEO_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_geometric_loss_vs_f64(te, shape, clamp):
    B, H, W = shape
    for k, kind in enumerate(("small", "out", "behind")):
        out, behind = geometric_case(te, B, H, W, kind, clamp, seed=B * 100 + H + W + k)
        if kind == "out" and H * W >= 64:
            assert out >= 0.2, ("the out-of-frame pose must send >= 20 % of the points out", out)
        if kind == "behind":
            assert behind > 0, "no point behind the camera"


# ------------------------------------------------------------------------------------------------------------------
# Pattern similarity loss, single level (fused 'fast' and ATen warp + exact block loss)
# ------------------------------------------------------------------------------------------------------------------
def pattern_slope(pat):
    """per pixel of the pattern map: largest |x| plus largest |y| neighbour difference of the 3 x 3 cells around it"""
    p = pat.double()
    sx = F.pad((p[..., 1:] - p[..., :-1]).abs(), (0, 1, 0, 0))
    sy = F.pad((p[..., 1:, :] - p[..., :-1, :]).abs(), (0, 0, 0, 1))
    return F.max_pool2d(sx, 3, 1, 1) + F.max_pool2d(sy, 3, 1, 1)


def pattern_masks(ref, type, H, W, pslope):
    """grad mask: ix within delta_pos of an integer (bilinear cell; 0 and W-1 the clip), and for sad / census_sad the
    pixels of every pair whose difference lies within delta_pair of 0 (the tap pixel; for census also the centre).
    delta_pair: the warped values carry delta_pos * local slope + 4 EPS |value|; census differences of two soft steps
    whose slope is <= 0.5 / sqrt(eps) = 0.71 (eps 0.5), plus 8 EPS for the soft steps' own rounding."""
    delta = POS_ULPS_PAT * EPS * max(W, H)
    ix = ref.inter["ix"]
    bad = near_integer(ix, delta) & (ix > -delta) & (ix < W - 1 + delta)
    if type in ("sad", "census_sad"):
        near = ref.inter["pair_near"]                                   # [B,81,H,W]
        B = near.shape[0]
        hit = torch.zeros(B, H * W, dtype=torch.bool, device=near.device)
        ys = torch.arange(H, device=near.device).view(H, 1)
        xs = torch.arange(W, device=near.device).view(1, W)
        centre = torch.zeros(B, H * W, dtype=torch.bool, device=near.device)
        p = (ys * W + xs).view(-1)
        for t in range(81):
            dy, dx = t // 9 - 4, t % 9 - 4
            r = ((ys + dy).clamp(0, H - 1) * W + (xs + dx).clamp(0, W - 1)).view(-1)
            sel = near[:, t].reshape(B, -1)
            if type == "census_sad":
                sel = sel & (r != p)     # a tap clamped onto the centre pairs 0 with 0 identically: gradient 0
                centre |= sel
            for b in range(B):
                if bool(sel[b].any()):
                    hit[b, r[sel[b]]] = True
        bad |= hit.view(B, 1, H, W) | centre.view(B, 1, H, W)
    return bad


def pair_tolerance(ref, pslope, type, delta, H, W):
    """per warped pixel: delta_pos * local pattern slope + 4 EPS |value|; census pairs are differences of soft steps
    of slope <= 0.5 / sqrt(eps) = 0.71 (eps 0.5) over tap and centre, + 8 EPS for the steps' rounding; sad pairs
    carry the tap's distance (the image is exact)"""
    x0 = ref.inter["ix"].clamp(0, W - 1).round().long()
    y0 = ref.inter["iy"].clamp(0, H - 1).round().long().expand_as(x0)
    vtol = delta * pslope[0, 0][y0, x0] + 4 * EPS * ref.value[1].abs()
    return (vtol, 0.71, 8 * EPS) if type == "census_sad" else (vtol, 1.0, 0.0)


def pattern_case(te, B, H, W, algo, type, use_mask, with_gp, seed):
    g = torch.Generator().manual_seed(seed)
    pattern = torch.randn(1, 1, H, W, generator=g)
    im = torch.randn(B, 1, H, W, generator=g)
    std = 0.05 + torch.rand(B, 1, H, W, generator=g)
    # disparities up to W / 8 plus a band that pushes u - disp below 0 and a band above W - 1 (negative disparity)
    disp = torch.rand(B, 1, H, W, generator=g) * (W / 8.0)
    disp[..., : max(1, W // 6)] += 3.0
    disp[..., -max(1, W // 6):] -= 2.0 + W / 8.0
    gp = torch.randn(B, 1, H, W, generator=g) * 1e-3 if with_gp else None
    mod = te.RectifiedPatternSimilarityLoss(H, W, pattern.cuda(), loss_type=type, loss_eps=0.5, algo=algo)
    d = disp.cuda().requires_grad_(True)
    val, proj = mod(d, im.cuda(), std.cuda() if use_mask else None)
    if gp is not None:
        torch.autograd.backward((val, proj), (torch.ones_like(val), gp.cuda()))
    else:
        val.backward()
    args = (disp.cuda(), im.cuda(), pattern.cuda(), std.cuda() if use_mask else None, type, 0.5,
            None if gp is None else gp.cuda())
    pslope = pattern_slope(pattern.cuda())
    delta = POS_ULPS_PAT * EPS * max(W, H)
    ref = R.pattern_loss(*args)
    if type in ("sad", "census_sad"):
        ref.inter["pair_near"] = R.pattern_loss(*args, pair_tol=pair_tolerance(ref, pslope, type, delta, H, W)).inter["pair_near"]
    f32 = R.pattern_loss(*args, dtype=torch.float32)
    tag = "pattern %s %s mask=%d gp=%d %dx%dx%d" % (algo, type, use_mask, with_gp, B, H, W)
    # warped values: the sample moves by <= delta_pos * local slope (x: W-based, y: H-based coordinate)
    x0 = ref.inter["ix"].clamp(0, W - 1).round().long()
    y0 = ref.inter["iy"].clamp(0, H - 1).round().long().expand_as(x0)
    loc = pslope[0, 0][y0, x0]
    check(tag + " pattern_proj", proj, ref.value[1], f32.value[1], pos=delta * loc + 4 * EPS * ref.value[1].abs())
    check_value(tag + " value", val, ref.value[0], f32.value[0])
    mask = pattern_masks(ref, type, H, W, pslope)
    # gradient: piecewise smooth in the sampling positions; Lipschitz constant by a finite difference of the f64
    # reference under a shift of every disparity by h
    h = delta / 4                                    # crosses no unmasked kink
    sh = R.pattern_loss(args[0].double() + h, *args[1:])
    keep = ~mask
    lip = float((sh.grads["disp"] - ref.grads["disp"]).abs()[keep].max() / h) if bool(keep.any()) else 0.0
    cap = CAP + 2 * 2 * delta + (CENSUS_CAP if type == "census_sad" else 0.0)
    # + the iy weights: d proj / d disp = (p01 - p00) wy0 + (p11 - p10) wy1 moves by <= delta * 2 * local slope when
    # iy carries its rounding delta; it multiplies the gradient arriving at pattern_proj (f64 gproj, grad_proj included)
    piy = ref.inter["gproj"].abs() * delta * 2 * loc * W / (W - 1)
    # algo='exact' runs the block-loss backward in the reference extension's own f32 order (bit for bit,
    # tests/test_photometric_gpu.py); that order's rounding, up to ~1e-6 of the scale, is the reference's, not the port's
    check(tag + " d/d disp", d.grad, ref.grads["disp"], f32.grads["disp"], mask, pos=lip * delta * W / (W - 1) + piy,
          cap=cap, cal=1e-6 * float(ref.grads["disp"].abs().max()) if algo == "exact" else 0.0)


PAT_SHAPES = [(1, 2, 2), (1, 8, 64), (1, 9, 65), (2, 17, 130), (2, 24, 40)]


@pytest.mark.parametrize("algo", ["fast", "exact"])
@pytest.mark.parametrize("shape", PAT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pattern_loss_vs_f64(te, shape, algo):
    B, H, W = shape
    k = 0
    for type in R.PHOTO_TYPES:
        for use_mask in (True, False):
            for with_gp in (False, True):
                pattern_case(te, B, H, W, algo, type, use_mask, with_gp, seed=1000 * H + W + k)
                k += 1


@pytest.mark.parametrize("algo", ["fast", "exact"])
@pytest.mark.parametrize("type", ["census_sad", "mse"])
def test_pattern_loss_vs_f64_training_size(te, algo, type):
    """16 x 432 x 512 (config 3): the elementwise check next to test_pattern_loss_gpu.py's statistical one"""
    pattern_case(te, 16, 432, 512, algo, type, True, type == "mse", seed=5)


# ------------------------------------------------------------------------------------------------------------------
# Multi-level pattern loss (config-5 pyramid), each level against its own f64 reference
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("type", ["census_sad", "mse"])
def test_pattern_loss_multi_vs_f64(te, type):
    B = 8
    g = torch.Generator().manual_seed(9)
    disps, ims, stds, pats = [], [], [], []
    for s in range(4):
        H, W = 480 >> s, 640 >> s
        pats.append(torch.randn(1, 1, H, W, generator=g))
        ims.append(torch.randn(B, 1, H, W, generator=g))
        stds.append(None if s == 3 else 0.05 + torch.rand(B, 1, H, W, generator=g))
        disps.append(torch.rand(B, 1, H, W, generator=g) * (60 >> s) - 2.0)
    da = [d.cuda().requires_grad_(True) for d in disps]
    vals, _, projs = te.pattern_loss_multi(da, [i.cuda() for i in ims], [None if m is None else m.cuda() for m in stds],
                                           [p.cuda() for p in pats], type, 0.5)
    w = torch.tensor([1.0, 0.5, 0.25, 2.0], device="cuda")
    (vals * w).sum().backward()
    for s in range(4):
        H, W = 480 >> s, 640 >> s
        args = (disps[s].cuda(), ims[s].cuda(), pats[s].cuda(), None if stds[s] is None else stds[s].cuda(), type, 0.5)
        ref = R.pattern_loss(*args)
        f32 = R.pattern_loss(*args, dtype=torch.float32)
        delta = POS_ULPS_PAT * EPS * max(W, H)
        pslope = pattern_slope(pats[s].cuda())
        if type == "census_sad":
            ref.inter["pair_near"] = R.pattern_loss(*args, pair_tol=pair_tolerance(ref, pslope, type, delta, H, W)).inter["pair_near"]
        tag = "pattern multi %s level %d %dx%dx%d" % (type, s, B, H, W)
        x0 = ref.inter["ix"].clamp(0, W - 1).round().long()
        y0 = ref.inter["iy"].clamp(0, H - 1).round().long().expand_as(x0)
        check(tag + " pattern_proj", projs[s], ref.value[1], f32.value[1],
              pos=delta * pslope[0, 0][y0, x0] + 4 * EPS * ref.value[1].abs())
        check_value(tag + " value", vals[s], ref.value[0], f32.value[0])
        mask = pattern_masks(ref, type, H, W, pslope)
        h = delta / 4
        sh = R.pattern_loss(args[0].double() + h, *args[1:])
        lip = float((sh.grads["disp"] - ref.grads["disp"]).abs()[~mask].max() / h)
        cap = CAP + 2 * 2 * delta + (CENSUS_CAP if type == "census_sad" else 0.0)
        piy = ref.inter["gproj"].abs() * delta * 2 * pslope[0, 0][y0, x0] * W / (W - 1)
        check(tag + " d/d disp", da[s].grad, w[s] * ref.grads["disp"], w[s] * f32.grads["disp"], mask,
              pos=float(w[s]) * (lip * delta * W / (W - 1) + piy), cap=cap)


# ------------------------------------------------------------------------------------------------------------------
# The clip border exactly: ix == 0 and ix == W - 1
# ------------------------------------------------------------------------------------------------------------------
def _f32_scan(start, chain, target, n=4096):
    """the f32 neighbour of `start` (scanning outwards) whose f32 chain gives exactly `target`"""
    x = np.float32(start)
    up, dn = x, x
    for _ in range(n):
        for c in (up, dn):
            if chain(c) == np.float32(target):
                return c
        up, dn = np.nextafter(up, np.float32(np.inf)), np.nextafter(dn, np.float32(-np.inf))
    raise AssertionError("no f32 input maps exactly onto %r" % target)


@pytest.mark.parametrize("edge", ["lo", "hi"])
def test_geometric_position_gradient_at_exact_clip_border(te, edge):
    """K = I, R = I, t0 = 0, t1 = (tx, 0, 0), depth0 = 1: u = ray[0] + tx in f32 (the kernel is built with
    -ffp-contract=off, so its f32 chain ray[0] -> ix is the numpy f32 chain below).  With t1 = 0 the depth0 gradient
    would not see the position term at all (scaling depth0 moves the point along its ray: u stays put); tx != 0 makes
    d u / d depth0 = -tx.  At ix == 0 or W - 1 exactly, border padding clips the coordinate and
    ATen's clip_coordinates_set_grad zeroes the position gradient ("borders are considered out of bounds"): the depth0
    gradient of that pixel must be what stock-torch f32 autograd gives."""
    from connecting_the_dots_amd import _lib
    L = _lib.lib()
    f = np.float32
    B, H, W = 1, 4, 8

    tx = f(0.25)

    def chain(r):
        u = f(r) + tx
        un = f(2) * (u / f(W - 1) - f(0.5))
        return ((un + f(1)) * f(W) - f(1)) * f(0.5)

    target = 0.0 if edge == "lo" else float(W - 1)
    u_star = _f32_scan((target + 0.5) / W * (W - 1) - tx, chain, target)
    assert chain(u_star) == f(target)
    ray = np.zeros((H * W, 3), np.float32)
    ray[:, 0] = 3.3                                  # every other pixel samples inside the frame
    ray[:, 1] = 1.6
    ray[:, 2] = 1.0
    px = 1 * W + 2
    ray[px, 0] = u_star
    eye = np.eye(3, dtype=np.float32)
    depth0 = np.ones((B, 1, H, W), np.float32)
    depth1 = (2.0 + 0.37 * np.arange(W, dtype=np.float32)[None, None, None, :] +
              0.11 * np.arange(H, dtype=np.float32)[None, None, :, None]).astype(np.float32)
    depth1 = np.ascontiguousarray(np.broadcast_to(depth1, (B, 1, H, W)))
    t1 = np.array([[tx, 0, 0]], np.float32)
    t = {n: cuda(x) for n, x in (("d0", depth0), ("d1", depth1), ("ray", ray), ("K", eye), ("R", eye[None]),
                                 ("t", np.zeros((1, 3), np.float32)), ("t1", t1))}
    gl = torch.ones(1, device="cuda")
    g0 = torch.zeros(B, 1, H, W, device="cuda")
    g1 = torch.zeros(B, 1, H, W, device="cuda")
    p = lambda x: x.data_ptr()
    s = torch.cuda.current_stream().cuda_stream
    assert L.ctd_geometric_bwd_f32(p(t["d0"]), p(t["d1"]), p(t["ray"]), p(t["K"]), p(t["R"]), p(t["t"]), p(t["R"]),
                                   p(t["t1"]), p(gl), p(g0), 0, p(g1), B, H, W, -1.0, 0, s) == 0
    torch.cuda.synchronize()
    a = torch.from_numpy(depth0).requires_grad_(True)
    b = torch.from_numpy(depth1).requires_grad_(True)
    T = torch.from_numpy
    v, inter = R.geometric_dir(a, b, T(eye), T(ray), T(eye[None]), T(np.zeros((1, 3), np.float32)), T(eye[None]),
                               T(t1), -1.0)
    v.backward()
    assert float(inter["ix"].view(-1)[px]) == target              # torch's f32 chain lands on the border too
    got, want = float(g0.view(-1)[px]), float(a.grad.view(-1)[px])
    print("geometric clip %s: ix == %g, hip d/d depth0 %.9e, stock-torch f32 %.9e" % (edge, target, got, want))
    assert abs(got - want) <= 1e-5 * abs(want) + 1e-12, (edge, got, want)
    # the sampled value did not change: depth1's gradient equals torch's everywhere
    assert torch.allclose(g1.cpu(), b.grad, rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("edge", ["lo", "hi"])
def test_pattern_position_gradient_at_exact_clip_border(te, edge):
    """the same for the fused pattern warp: a disparity that puts ix exactly on 0 / W - 1 (f32 scan of the kernel's
    chain); the gradient there is ATen's, 0"""
    f = np.float32
    B, H, W = 1, 8, 64
    x, y = 20, 3

    def chain(disp):
        u1 = f(x) - f(disp)
        gx = f(2) * (u1 / f(W - 1) - f(0.5))
        return ((gx + f(1)) * f(W) - f(1)) / f(2)

    target = 0.0 if edge == "lo" else float(W - 1)
    d_star = _f32_scan(x - (target + 0.5) / W * (W - 1), chain, target)
    g = torch.Generator().manual_seed(4)
    pattern = torch.randn(1, 1, H, W, generator=g)
    im = torch.randn(B, 1, H, W, generator=g)
    disp = torch.rand(B, 1, H, W, generator=g) * 5
    disp[0, 0, y, x] = float(d_star)
    d = disp.cuda().requires_grad_(True)
    mod = te.RectifiedPatternSimilarityLoss(H, W, pattern.cuda(), algo="fast")
    val, _ = mod(d, im.cuda(), None)
    val.backward()
    f32 = R.pattern_loss(disp, im, pattern, None, "census_sad", 0.5, dtype=torch.float32)
    assert float(f32.inter["ix"][0, 0, y, x]) == target
    got, want = float(d.grad[0, 0, y, x]), float(f32.grads["disp"][0, 0, y, x])
    print("pattern clip %s: hip %.9e stock-torch f32 %.9e" % (edge, got, want))
    assert want == 0.0 and got == 0.0
