"""Stock-torch restatements of the training losses and of LCN (model/networks.py of the reference), for the float64
tests.  Not a conftest: a plain helper module that tests import.

Every reference takes the f32 tensors the HIP kernels take, promotes them to `dtype` (float64 by default; float32 gives
the stock-torch f32 composition the tests calibrate against), differentiates with autograd and returns a `Ref`:
`value` (scalar), `grads` (name -> gradient, same shape as the input) and `inter` (name -> intermediate values the
tests build their discontinuity masks from).  Nothing here calls a HIP kernel; tests/test_f64_refs.py pins these
formulas to the vectors captured from the reference modules (tests/golden)."""
from collections import namedtuple

import torch
import torch.nn.functional as F

Ref = namedtuple("Ref", "value grads inter")

SOBEL_KX = [[-5, -4, 0, 4, 5], [-8, -10, 0, 10, 8], [-10, -20, 0, 20, 10], [-8, -10, 0, 10, 8], [-5, -4, 0, 4, 5]]
B0, B1 = 0.0503428816795, 1.07274045944          # DisparityLoss's Laplace scales (networks.py:389-390)
PDF_MIN = 1e-4                                   # clamp(min=1e-4) of the mixture density
PHOTO_TYPES = ("mse", "sad", "census_mse", "census_sad")


def _leaf(x, dtype):
    return x.detach().to(dtype).requires_grad_(True)


def disp_to_depth(disp, baseline_focal, grad_out, dtype=torch.float64):
    """DispToDepth (networks.py:313-321): depth = bf / (relu(disp) + 1e-12); grads['disp'] for upstream grad_out"""
    d = _leaf(disp, dtype)
    depth = (1.0 / (F.relu(d) + 1e-12)) * baseline_focal
    (g,) = torch.autograd.grad(depth, d, grad_out.to(dtype))
    return Ref(depth.detach(), {"disp": g}, {})


def sobel(disp):
    """SobelFilter(norm=False) (networks.py:537-565): replicate pad 2, the 5x5 kx / 240 and ky = kx^T; (gx, gy)"""
    kx = torch.tensor(SOBEL_KX, dtype=disp.dtype, device=disp.device) / 240.0
    dp = F.pad(disp, (2, 2, 2, 2), mode="replicate")
    return F.conv2d(dp, kx.view(1, 1, 5, 5)), F.conv2d(dp, kx.t().contiguous().view(1, 1, 5, 5))


def disparity_loss(disp, edge=None, logits=None, dtype=torch.float64):
    """Sobel + DisparityLoss (networks.py:395-412).  `edge` is the edge probability; with `logits` instead, edge =
    1 - sigmoid(logits) as the trainer builds it and grads['logits'] is returned in place of grads['edge'].
    inter: g (gradient magnitude), dLdg (d value / d g), pdf (None without edge), sobel_abs (sum |k| |disp| over the 5x5 window: the
    magnitude the f32 Sobel sums round at)."""
    d = _leaf(disp, dtype)
    leaves, names = [d], ["disp"]
    e = None
    if logits is not None:
        lg = _leaf(logits, dtype)
        e = 1 - torch.sigmoid(lg)
        leaves.append(lg)
        names.append("logits")
    elif edge is not None:
        e = _leaf(edge, dtype)
        leaves.append(e)
        names.append("edge")
    gx, gy = sobel(d)
    g = torch.sqrt(gx * gx + gy * gy + 1e-8)
    pdf = None
    if e is None:
        val = g.clamp(0, 1).mean()
    else:
        pdf = (1 - e) / B0 * torch.exp(-g / B0) + e / B1 * torch.exp(-g / B1)
        val = (-torch.log(pdf.clamp(min=PDF_MIN))).mean()
    *grads, dldg = torch.autograd.grad(val, leaves + [g])
    with torch.no_grad():
        kabs = torch.tensor(SOBEL_KX, dtype=dtype, device=d.device).abs() / 240.0
        sabs = F.conv2d(F.pad(d.abs(), (2, 2, 2, 2), mode="replicate"), kabs.view(1, 1, 5, 5))
    return Ref(val.detach(), dict(zip(names, grads)),
               {"g": g.detach(), "dLdg": dldg, "pdf": None if pdf is None else pdf.detach(), "sobel_abs": sabs})


def geometric_dir(depth0, depth1, K, ray, R0, t0, R1, t1, clamp):
    """One direction of ProjectionDepthSimilarityLoss (networks.py:483-498) on tensors already of the working dtype:
    (mean, intermediates).  ray [H*W,3] is the module's ray."""
    B, _, H, W = depth0.shape
    xyz = depth0.reshape(B, -1, 1) * ray.unsqueeze(0)
    xyz = torch.bmm(xyz - t0.reshape(B, 1, 3), R0)
    xyz = torch.bmm(xyz, R1.transpose(1, 2)) + t1.reshape(B, 1, 3)
    uvd = xyz @ K.T
    d = uvd[:, :, 2:3]
    uv = uvd[:, :, :2] / (F.relu(d) + 1e-12)
    gx = 2 * (uv[:, :, 0] / (W - 1) - 0.5)
    gy = 2 * (uv[:, :, 1] / (H - 1) - 0.5)
    grid = torch.stack((gx, gy), dim=2).view(B, H, W, 2)
    sample = F.grid_sample(depth1, grid, padding_mode="border", align_corners=False)
    e = d.view(B, 1, H, W) - sample
    diff = torch.abs(e)
    term = torch.clamp(diff, 0, clamp) if clamp > 0 else diff
    with torch.no_grad():
        inter = {"ix": (((gx + 1) * W - 1) / 2).view(B, 1, H, W), "iy": (((gy + 1) * H - 1) / 2).view(B, 1, H, W),
                 "d": d.detach().view(B, 1, H, W), "sample": sample.detach(), "e": e.detach(), "diff": diff.detach()}
    return term.mean(), inter


def geometric_loss(depth0, depth1, K, ray, R0, t0, R1, t1, clamp, dtype=torch.float64):
    """The symmetric loss the module returns: fwd(depth0 -> view 1) + fwd(depth1 -> view 0).  grads 'depth0',
    'depth1'; inter 'fwd' and 'rev' hold the two directions' intermediates (ix and iy before clipping, d, sample, e =
    d - sample, diff = |e|)."""
    a, b = _leaf(depth0, dtype), _leaf(depth1, dtype)
    K, ray, R0, t0, R1, t1 = (x.detach().to(dtype) for x in (K, ray, R0, t0, R1, t1))
    v0, i0 = geometric_dir(a, b, K, ray, R0, t0, R1, t1, clamp)
    v1, i1 = geometric_dir(b, a, K, ray, R1, t1, R0, t0, clamp)
    val = v0 + v1
    g0, g1 = torch.autograd.grad(val, (a, b))
    return Ref(val.detach(), {"depth0": g0, "depth1": g1}, {"fwd": i0, "rev": i1})


def block_loss(es, ta, block_size, type, eps):
    """The block photometric loss (PhotometricLossForward of the reference's ext, as functions.py:120-147 restates it
    with replicate pad + unfold) of one-channel images: (per-pixel loss [B,1,H,W], pair differences [B,bs*bs,H,W]).
    A pair difference is the value the loss squares or takes the absolute value of: es - ta at the tap for
    mse / sad, soft(es_tap - es_centre) - soft(ta_tap - ta_centre) for the census types."""
    p = block_size // 2
    B, C, H, W = es.shape

    def windows(x):
        xp = F.pad(x, (p, p, p, p), mode="replicate")
        return F.unfold(xp, kernel_size=block_size).view(B, block_size * block_size, H, W)

    ew, tw = windows(es), windows(ta)
    if type in ("mse", "sad"):
        diff = ew - tw
    else:
        def soft(x):
            return 0.5 * (1 + x / torch.sqrt(x * x + eps))
        diff = soft(ew - es) - soft(tw - ta)
    term = diff * diff if type.endswith("mse") else diff.abs()
    return term.sum(dim=1, keepdim=True) / block_size ** 2, diff


def warp_grid(disp, H, W):
    """RectifiedPatternSimilarityLoss's sampling grid (networks.py:362-369) for disp [B,1,H,W]: (grid, ix, iy) with
    ix, iy the unnormalised (align_corners=False) coordinates before clipping"""
    B = disp.shape[0]
    u = torch.arange(W, dtype=disp.dtype, device=disp.device).view(1, 1, -1).expand(1, H, -1)
    v = torch.arange(H, dtype=disp.dtype, device=disp.device).view(1, -1, 1).expand(1, -1, W)
    gx = 2 * ((u - disp.view(B, H, W)) / (W - 1) - 0.5)
    gy = (2 * (v / (H - 1) - 0.5)).expand(B, -1, -1)
    grid = torch.stack((gx, gy), dim=3)
    return grid, (((gx + 1) * W - 1) / 2).unsqueeze(1), (((gy + 1) * H - 1) / 2).unsqueeze(1)


def pattern_loss(disp, im, pattern, mask, type, eps=0.5, grad_proj=None, dtype=torch.float64, pair_tol=None):
    # pair_tol: None, or (vtol, c, floor) -- vtol [B,1,H,W] the rounding distance of each warped value; a pair is
    # near 0 when |pair| <= c (vtol at the tap + vtol at the centre) + floor
    """RectifiedPatternSimilarityLoss.tforward (networks.py:358-378): pattern = channel mean, pattern_proj =
    grid_sample(bilinear, border, align_corners=False), diff = block loss (block 9), val = sum(mask * diff) /
    sum(mask) (mask = ones when None).  d val / d disp (+ grad_proj . d pattern_proj / d disp when grad_proj is
    given, the upstream gradient at the returned pattern_proj) in grads['disp'].  One frame at a time: the 81-tap
    windows of a 432 x 512 batch would not fit; the frames' gradients share only the denominator sum(mask).
    value is (val, pattern_proj); inter: ix, iy (unnormalised, before clipping), gproj (the gradient arriving at
    pattern_proj) and pair (the pair differences,
    [B,81,H,W]) -- or, with pair_tol given, pair_near (bool, an eighth of the memory)."""
    B, _, H, W = disp.shape
    pat = pattern.detach().to(dtype).mean(dim=1, keepdim=True)
    den = mask.detach().to(dtype).sum() if mask is not None else torch.tensor(float(B * H * W), dtype=dtype,
                                                                              device=disp.device)
    num = torch.zeros((), dtype=dtype, device=disp.device)
    grads, projs, ixs, iys, pairs, gprojs = [], [], [], [], [], []
    for b in range(B):
        d = _leaf(disp[b:b + 1], dtype)
        grid, ix, iy = warp_grid(d, H, W)
        proj = F.grid_sample(pat, grid, padding_mode="border", align_corners=False)
        diff, pair = block_loss(proj, im[b:b + 1].detach().to(dtype), 9, type, eps)
        m = mask[b:b + 1].detach().to(dtype) if mask is not None else torch.ones_like(diff)
        nb = (m * diff).sum()
        out = nb / den
        if grad_proj is not None:
            out = out + (proj * grad_proj[b:b + 1].to(dtype)).sum()
        g, gpj = torch.autograd.grad(out, (d, proj))
        num = num + nb.detach()
        grads.append(g)
        gprojs.append(gpj)
        projs.append(proj.detach())
        ixs.append(ix.detach())
        iys.append(iy.detach())
        if pair_tol is None:
            pairs.append(pair.detach())
        else:
            vt, c, fl = pair_tol
            vb = vt[b:b + 1].to(dtype)
            vw = F.unfold(F.pad(vb, (4, 4, 4, 4), mode="replicate"), kernel_size=9).view(1, 81, H, W)
            pairs.append(pair.detach().abs() <= c * (vw + vb) + fl)
    return Ref((num / den, torch.cat(projs)), {"disp": torch.cat(grads)},
               {"ix": torch.cat(ixs), "iy": torch.cat(iys), "gproj": torch.cat(gprojs), ("pair" if pair_tol is None else "pair_near"): torch.cat(pairs)})


def lcn(x, radius, eps, dtype=torch.float64):
    """LCN.tforward (networks.py:507-533): ReflectionPad2d(radius), two all-ones (2r+1)^2 conv2d (of x and of x**2),
    avg = box / n, std = sqrt(box(x**2) / n - avg**2 + 1e-6) + eps, y = (x - avg) / std.  x [N,1,H,W] (any float
    dtype, promoted to `dtype`; float32 is the stock-torch f32 yardstick).  Returns a Ref: value (y, std), no grads, inter 'avg',
    'ex2' (box(x**2) / n), 'var' (ex2 - avg**2 + 1e-6, the argument of the square root).  x**2 is squared in `dtype`:
    at float64 it is exact for f32 samples, so it equals the square of the f32 tensor the module squares, to within
    that tensor's one rounding (at most 2^-24 relative, which the tests' tolerance covers)."""
    d = x.detach().to(dtype)
    n = float((2 * radius + 1) ** 2)
    k = torch.ones(1, 1, 2 * radius + 1, 2 * radius + 1, dtype=dtype, device=d.device)
    pad = torch.nn.ReflectionPad2d(radius)
    box = F.conv2d(pad(d), k)
    avg = box / n
    ex2 = F.conv2d(pad(d ** 2), k) / n
    var = ex2 - avg ** 2 + 1e-6
    std = torch.sqrt(var) + eps
    return Ref(((d - avg) / std, std), {}, {"avg": avg, "ex2": ex2, "var": var})


def _xcorr_windows(x, bs, left, right):
    """x [B,C,H,W] -> centred windows [B,C,n,H,Wout] and their sums of squared deviations [B,C,H,Wout]: replicate rows,
    columns padded by replicate `left` / `right` (the clamp of an unclamped column), two-pass mean and deviation"""
    B, C, H, W = x.shape
    h = bs // 2
    xp = F.pad(x.reshape(B * C, 1, H, W), (left, right, h, bs - 1 - h), mode="replicate")
    win = F.unfold(xp, bs).view(B, C, bs * bs, H, -1)
    win = win - win.mean(2, keepdim=True)
    return win, (win * win).sum(2)


def xcorrvol(in0, in1, n_disps, block_size, dtype=torch.float64, budget=1 << 25):
    """XCorrVolFunctor (ext.h:120-191) as stock torch ops on in0's device: in0 [C,H,W] or [N,C,H,W], in1 [C,H,W] ->
    [D,H,W] or [N,D,H,W], out[d,h,w] = sum_c dot / (sqrt(s0 s1) + 1e-8) over the bs x bs windows centred at (h, w) of
    in0 and (h, w - d) of in1.  Rows clamp; the pattern's columns are shifted by d BEFORE they clamp (ext.h:152), so
    its windows are taken over the unclamped columns x = -(D-1) .. W-1.  Disparities are processed in chunks of at most
    `budget` window elements."""
    squeeze = in0.dim() == 3
    a = (in0.unsqueeze(0) if squeeze else in0).to(dtype)
    b = in1.to(device=a.device, dtype=dtype).unsqueeze(0)
    N, C, H, W = a.shape
    D, bs = int(n_disps), int(block_size)
    h = bs // 2
    wa, sa = _xcorr_windows(a, bs, h, bs - 1 - h)              # [N,C,n,H,W], [N,C,H,W]
    wb, sb = _xcorr_windows(b, bs, D - 1 + h, bs - 1 - h)               # [1,C,n,H,W+D-1]: column x at index x + D - 1
    # offset j = D - 1 - d of the W-wide view starting at index j is the pattern at x = w - d
    vb, vs = wb.unfold(-1, W, 1), sb.unfold(-1, W, 1)         # [1,C,n,H,D,W], [1,C,H,D,W]
    out = torch.empty((N, D, H, W), dtype=dtype, device=a.device)
    chunk = max(1, budget // max(1, N * C * bs * bs * H * W))
    for d0 in range(0, D, chunk):
        d1 = min(D, d0 + chunk)
        js = slice(D - d1, D - d0)                             # offsets of d = d1-1 .. d0
        dot = (wa.unsqueeze(-2) * vb[..., js, :]).sum(2)       # [N,C,H,dc,W]
        den = torch.sqrt(sa.unsqueeze(-2) * vs[..., js, :]) + 1e-8
        val = (dot / den).sum(1).flip(-2)                      # [N,H,dc,W], d ascending
        out[:, d0:d1] = val.permute(0, 2, 1, 3)
    return out[0] if squeeze else out


def costvol(im, pattern, n_disps, block_size, type, eps, dtype=torch.float64, chunk=32):
    """The SAD / MSE / soft-census cost volume by composition, as oracle.costvol builds it from the reference's loss:
    cost[f,d] = block_loss(P_d, im[f]) with P_d[h,x] = P[h, clamp(x-d)].  im [H,W] | [N,H,W], pattern [H,W] | [N,H,W]
    -> [D,H,W] | [N,D,H,W], in `dtype` on im's device."""
    squeeze = im.dim() == 2
    a = (im.unsqueeze(0) if squeeze else im).to(dtype)
    N, H, W = a.shape
    p = pattern.to(device=a.device, dtype=dtype)
    p = p.expand(N, H, W) if p.dim() == 2 else p
    D = int(n_disps)
    out = torch.empty((N, D, H, W), dtype=dtype, device=a.device)
    cols = torch.arange(W, device=a.device)
    for f in range(N):
        for d0 in range(0, D, chunk):
            ds = torch.arange(d0, min(D, d0 + chunk), device=a.device)
            idx = (cols[None, :] - ds[:, None]).clamp(0, W - 1)          # [dc, W]
            pd = p[f][:, idx].permute(1, 0, 2).unsqueeze(1)            # [dc,1,H,W]
            ta = a[f].expand(len(ds), 1, H, W)
            out[f, d0:d0 + len(ds)] = block_loss(pd, ta, block_size, type, eps)[0][:, 0]
    return out[0] if squeeze else out
