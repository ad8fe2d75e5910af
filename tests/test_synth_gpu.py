"""Training-sample finishing and augmentation on the MI355X (connecting_the_dots_amd.synth): the finishing kernel bit
for bit against a numpy f32 restatement in the order include/ctd_hip.h states (pre -> grad through the CPU oracle's
datagen LCN), |Sobel| against float64, the augmentation against the reference's own augment_image outputs
(tests/golden/synth_augment.npz), salt-and-pepper precedence, the device-generator path without a host sync, and a
rendered track through TrackTrainer."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from connecting_the_dots_amd import synth
from tests import workloads

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "synth_augment.npz")
KD = np.array([-1, -2, 0, 2, 1], np.float32)
KS = np.array([1, 4, 6, 4, 1], np.float32)


def reflect101(i, n):
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i < n, i, p - i)


def sep5(a, kr, kc, dt):
    """row pass with taps kr, then column pass with kc, BORDER_REFLECT_101, s = 0; s += k[j] * v[j] in dtype dt"""
    H, W = a.shape
    a = a.astype(dt)
    ap = a[:, reflect101(np.arange(-2, W + 2), W)]
    h = np.zeros((H, W), dt)
    for j in range(5):
        h = h + dt(kr[j]) * ap[:, j:j + W]
    hp = h[reflect101(np.arange(-2, H + 2), H)]
    v = np.zeros((H, W), dt)
    for j in range(5):
        v = v + dt(kc[j]) * hp[j:j + H]
    return v


def sobel_mag(amb, dt):
    gx = sep5(amb, KD, KS, dt)
    gy = sep5(amb, KS, KD, dt)
    return np.sqrt(gx * gx + gy * gy), gx, gy


def finish_ref(oracle, depth, color, normal, b, bf, thr=0.8, ks=5, eps=0.1):
    c, n = color, normal
    imc = ((c[..., 0] + c[..., 1]) + c[..., 2]) / np.float32(3.0)
    amb = ((n[..., 0] + n[..., 1]) + n[..., 2]) / np.float32(3.0)
    im = np.float32(b) * imc + np.float32(1.0 - b) * amb
    with np.errstate(divide="ignore"):
        disp = np.float32(bf) / depth
    mask = (depth > 0).astype(np.float32)
    grad = np.empty_like(amb)
    for f in range(amb.shape[0]):
        g, _, _ = sobel_mag(amb[f], np.float32)
        pre = np.maximum(g - np.float32(thr), np.float32(0.0))
        grad[f] = np.clip(oracle.lcn_datagen(pre, ks, eps)[0], 0.0, 1.0)
    return dict(im=im, ambient=amb, grad=grad, disp=disp, mask=mask)


def finish_case(seed, N, H, W):
    rs = np.random.RandomState(seed)
    depth = rs.uniform(0.5, 4.0, size=(N, H, W)).astype(np.float32)
    depth[rs.uniform(size=depth.shape) < 0.05] = 0.0                 # inf disparity
    depth[rs.uniform(size=depth.shape) < 0.05] = -1.0                # nothing hit (the renderer's -1)
    color = rs.uniform(0, 1, size=(N, H, W, 3)).astype(np.float32)
    normal = rs.uniform(0, 1, size=(N, H, W, 3)).astype(np.float32)
    normal[:, : H // 3, : W // 2] = 0.4                              # a flat region: pre == 0, LCN on the variance floor
    normal[:, H // 2:, W // 3:] *= rs.uniform(0, 3, size=(N, 1, 1, 1)).astype(np.float32)   # strong edges
    normal[depth < 0] = 0.0
    return depth, color, normal


@pytest.mark.parametrize("N,H,W", [(2, 37, 53), (1, 96, 128), (3, 9, 40), (1, 40, 10), (1, 1, 1), (2, 3, 70),
                                   (1, 11, 11), (1, 130, 67)])
def test_finish_render_bit_exact(oracle, N, H, W):
    depth, color, normal = finish_case(N * 1000 + H * 7 + W, N, H, W)
    b, bf = 0.6 + 0.0137, 0.075 * 567.599975586 / 2
    up = lambda a: torch.from_numpy(a).cuda()
    out = synth.finish_render(up(depth), up(color), up(normal), b, 0.075, 567.599975586 / 2)
    ref = finish_ref(oracle, depth, color, normal, b, bf)
    for k in ("im", "ambient", "grad", "disp", "mask"):
        got = out[k].cpu().numpy()
        assert np.array_equal(got, ref[k]), "%s differs in %d of %d pixels" % (k, (got != ref[k]).sum(), got.size)
    g = ref["grad"]
    assert (g >= 0).all() and (g <= 1).all()
    if H > 10 and W > 10:
        assert (g[:, :5] == 0).all() and (g[:, -5:] == 0).all() and (g[:, :, :5] == 0).all() and (g[:, :, -5:] == 0).all()
        if H > 30 and W > 30:
            assert (g[:, 5:-5, 5:-5] > 0).any() and (g[:, 5:-5, 5:-5] < 1).any()
    else:
        assert (g == 0).all()
    # optional outputs
    out2 = synth.finish_render(up(depth), up(color), up(normal), [b] * N, 0.075, 567.599975586 / 2, with_disp=False,
                               with_mask=False)
    assert out2["disp"] is None and torch.equal(out2["grad"], out["grad"])


def test_finish_render_grad_equals_lcn_datagen_of_pre(oracle):
    """the fused LCN is ctd_lcn_datagen_f32's bits: run the library's datagen LCN on the host-restated pre"""
    from connecting_the_dots_amd import _lib
    depth, color, normal = finish_case(5, 2, 64, 80)
    up = lambda a: torch.from_numpy(a).cuda()
    out = synth.finish_render(up(depth), up(color), up(normal), 0.55, 0.075, 283.8, lcn_clip=False)
    amb = ((normal[..., 0] + normal[..., 1]) + normal[..., 2]) / np.float32(3.0)
    pre = np.stack([np.maximum(sobel_mag(a, np.float32)[0] - np.float32(0.8), np.float32(0)) for a in amb])
    x = up(pre)
    y, s = torch.empty_like(x), torch.empty_like(x)
    _lib.check(_lib.lib().ctd_lcn_datagen_f32(x.data_ptr(), y.data_ptr(), s.data_ptr(), 2, 64, 80, 5, 0.1, 0,
                                              torch.cuda.current_stream().cuda_stream), "lcn_datagen")
    assert torch.equal(out["grad"], y)
    assert (y.cpu().numpy() > 1).any() or (y.cpu().numpy() < 0).any()   # lcn_clip=False really left it unclipped


def test_sobel_magnitude_against_float64():
    """the stated f32 order is within 16 eps32 of the absolute tap sums of a float64 evaluation"""
    rs = np.random.RandomState(11)
    for H, W in ((37, 53), (5, 3), (64, 64)):
        amb = (rs.uniform(0, 1, size=(H, W)) * rs.uniform(0, 4)).astype(np.float32)
        g32, _, _ = sobel_mag(amb, np.float32)
        g64, _, _ = sobel_mag(amb.astype(np.float64), np.float64)
        ax = sep5(np.abs(amb.astype(np.float64)), np.abs(KD), KS, np.float64)
        ay = sep5(np.abs(amb.astype(np.float64)), KS, np.abs(KD), np.float64)
        bound = 16 * 2.0 ** -24 * (ax + ay)
        assert (np.abs(g32.astype(np.float64) - g64) <= bound).all()


def _golden_cases():
    z = np.load(GOLDEN)
    c = 0
    while "c%d_meta" % c in z:
        seed, n = (int(v) for v in z["c%d_meta" % c])
        yield z, c, seed, n, float(z["c%d_max_sp_noise" % c])
        c += 1


def _params(blur, sigma, scale=1.0):
    p = np.zeros(len(blur), synth.AUGMENT_PARAMS)
    for i in range(len(blur)):
        p[i]["blur"] = int(blur[i])
        p[i]["taps"] = synth.gaussian_taps(sigma[i]) if blur[i] else 0.0
        p[i]["noise_scale"] = scale
    return torch.from_numpy(p.view(np.uint8)).cuda()


def _blur_ref(img, sigma, dt):
    k = synth.gaussian_taps(sigma)
    if dt is np.float64:
        x = np.arange(-2, 3, dtype=np.float64)
        e = np.exp(-x * x / (2 * sigma * sigma))
        k = e / e.sum()
    return sep5(img, k, k, dt)


def _augment_ref(img, d):
    """the stated order: f32 blur, + f64 noise term, salt then pepper, clip in f64, one rounding"""
    x = _blur_ref(img, d["sigma"], np.float32) if d["blur"] else img
    v = x.astype(np.float64) + d["noise"]
    f = v.reshape(-1)
    f[d["salt"]] = img.max()
    f[d["pepper"]] = img.min()
    return np.clip(v, 0.0, 1.0).astype(np.float32)


def test_augment_reproduces_the_reference_fixture():
    """the fixture's own draws through the kernels: bit for bit the reference output where the blur coin is off, bit
    for bit the stated f32 blur where it is on (the fixture's stand-in GaussianBlur returned its input)"""
    n_off = n_on = 0
    for z, c, seed, n, sp in _golden_cases():
        for i in range(n):
            k = "c%d_%d_" % (c, i)
            img = z[k + "img"]
            H, W = img.shape
            d = dict(blur=bool(z[k + "blur"]), sigma=float(z[k + "sigma"]), noise=z[k + "noise"], salt=z[k + "salt"],
                     pepper=z[k + "pepper"])
            kk = len(d["salt"])
            idx = lambda a: torch.from_numpy(np.asarray(a, np.int64).reshape(1, -1) if kk else np.zeros((1, 1), np.int64)).cuda()
            out, minmax = synth._augment_launch(torch.from_numpy(img[None, None]).cuda(),
                                                torch.from_numpy(d["noise"][None]).cuda(), 1,
                                                _params([d["blur"]], [d["sigma"]]),
                                                torch.tensor([kk], dtype=torch.int32).cuda(), idx(d["salt"]),
                                                idx(d["pepper"]), kk)
            got = out[0, 0].cpu().numpy()
            mn, mx = synth.decode_minmax(minmax.cpu().numpy())
            assert mn[0] == img.min() and mx[0] == img.max()
            if not d["blur"]:
                assert np.array_equal(got, z[k + "out"]), k
                n_off += 1
            else:
                assert np.array_equal(got, _augment_ref(img, d)), k
                n_on += 1
    assert n_off >= 4 and n_on >= 4


def test_blur_against_float64():
    """bit for bit the stated f32 order; against a float64 blur with the exact taps, within the forward-error bound of
    that order, 14 * 2^-24 * blur(|x|) (f32 taps: 2 roundings per tap pair, 2 products, 4 + 4 sums, with margin).  A
    bound of 2 ulp of the result does not hold for this order: up to 3.6 ulp occur (5.6 * 2^-24 * blur(|x|))."""
    rs = np.random.RandomState(4)
    for H, W, sigma in ((24, 40, 0.21), (7, 9, 0.5), (70, 130, 0.37), (1, 5, 0.3), (3, 2, 0.45)):
        img = rs.uniform(0, 1, size=(2, 1, H, W)).astype(np.float32)
        out, _ = synth._augment_launch(torch.from_numpy(img).cuda(), torch.zeros((2, H, W), device="cuda"), 0,
                                       _params([1, 1], [sigma, sigma]), None, None, None, 0)
        got = out.cpu().numpy()
        for f in range(2):
            r32 = _blur_ref(img[f, 0], sigma, np.float32)
            r64 = _blur_ref(img[f, 0], sigma, np.float64)
            assert np.array_equal(got[f, 0], r32)
            a64 = _blur_ref(np.abs(img[f, 0]), sigma, np.float64)
            assert (np.abs(got[f, 0] - r64) <= 14 * 2.0 ** -24 * a64).all()


def test_rng_path_matches_the_fixture():
    """synth.augment(rng=...) end to end: same draws as augment_image, same outputs (blur off), same restatement (on)"""
    for z, c, seed, n, sp in _golden_cases():
        rng = np.random.RandomState(seed)
        groups = [list(range(0, 3)), [3]]                   # three 24x40 images, then the 7x9 one
        for g in groups:
            img = np.stack([z["c%d_%d_img" % (c, i)] for i in g])[:, None]
            out, draws = synth.augment(torch.from_numpy(img).cuda(), rng=rng, max_sp_noise=sp, return_draws=True)
            out = out.cpu().numpy()
            for j, i in enumerate(g):
                k = "c%d_%d_" % (c, i)
                if not bool(z[k + "blur"]):
                    assert np.array_equal(out[j, 0], z[k + "out"])
                else:
                    assert np.array_equal(out[j, 0], _augment_ref(img[j, 0], draws[j]))


def test_pepper_wins_where_indices_collide():
    img = torch.linspace(0.1, 0.9, 64, device="cuda").reshape(1, 1, 8, 8).contiguous()
    salt = torch.tensor([[5, 9, 5, 63]], device="cuda")
    pepper = torch.tensor([[5, 1, 9, 70]], device="cuda")            # 70 is outside the image: skipped
    out, _ = synth._augment_launch(img, torch.zeros((1, 8, 8), device="cuda"), 0, _params([0], [0]),
                                   torch.tensor([4], dtype=torch.int32, device="cuda"), salt, pepper, 4)
    o = out.reshape(-1).cpu()
    lo, hi = float(img.min()), float(img.max())
    assert o[5] == lo and o[9] == lo and o[1] == lo and o[63] == hi
    keep = [i for i in range(64) if i not in (1, 5, 9, 63)]
    assert torch.equal(o[keep], img.reshape(-1).cpu()[keep])


def test_generator_path_is_sync_free_and_sane():
    N, H, W = 16, 128, 160
    img = torch.full((N, 1, H, W), 0.5, device="cuda")
    g = torch.Generator(device="cuda")
    g.manual_seed(123)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out, d = synth.augment(img, generator=g, max_noise=20.0, max_sp_noise=0.001, return_draws=True)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    kmax = int(H * W * 0.001)
    counts = d["counts"].cpu().numpy()
    assert (counts >= 0).all() and (counts <= kmax).all()
    sp = d["sp"].cpu().numpy()
    assert (counts[~sp] == 0).all()
    assert np.array_equal(counts[sp], (d["ratio"].cpu().numpy()[sp] * H * W).astype(np.int32))
    sig = d["sigma"].cpu().numpy()
    assert (sig >= 0.2).all() and (sig <= 0.5).all()
    assert 0 < d["blur"].sum() < N and 0 < sp.sum() < N
    scale = d["scale"].cpu().numpy()
    assert (scale >= 0).all() and (scale <= 20.0 / 255).all()
    noise = d["noise"]
    assert abs(float(noise.std()) - 1.0) < 0.01 and abs(float(noise.mean())) < 0.01
    # a flat image blurs to a flat image: the two f32 tap sums of 0.5 (the stated order), then the noise and the clip
    taps = d["taps"]
    h = torch.zeros(N, device="cuda")
    for j in range(5):
        h = h + taps[:, j] * 0.5
    v = torch.zeros(N, device="cuda")
    for j in range(5):
        v = v + taps[:, j] * h
    base = torch.where(d["blur"], v, torch.full_like(v, 0.5)).double().view(-1, 1, 1)
    exp = (base + noise.double() * d["scale"].view(-1, 1, 1)).clamp(0, 1).float()
    o = out[:, 0].clone()
    for n in range(N):
        if counts[n]:
            touched = torch.cat([d["salt"][n, :counts[n]], d["pepper"][n, :counts[n]]])
            o[n].view(-1)[touched] = exp[n].view(-1)[touched]
    assert torch.equal(o, exp)
    dev_std = (out[:, 0] - 0.5).std(dim=(1, 2)).cpu().numpy()
    assert np.allclose(dev_std, scale, rtol=0.05, atol=2e-3)


class TinyNet(torch.nn.Module):
    """DispEdgeNet's output contract (4 disparity scales, 3 edge-logit scales) at test size"""

    def __init__(self, max_disp):
        super().__init__()
        self.body = torch.nn.Sequential(torch.nn.Conv2d(2, 8, 3, padding=1), torch.nn.ReLU())
        self.disp_heads = torch.nn.ModuleList(torch.nn.Conv2d(8, 1, 3, padding=1) for _ in range(4))
        self.edge_heads = torch.nn.ModuleList(torch.nn.Conv2d(8, 1, 3, padding=1) for _ in range(3))
        self.max_disp = max_disp

    def forward(self, x):
        feats = [self.body(x)]
        for _ in range(3):
            feats.append(F.avg_pool2d(feats[-1], 2))
        return ([torch.sigmoid(h(feats[s])) * (self.max_disp / 2 ** s) for s, h in enumerate(self.disp_heads)],
                [h(feats[s]) for s, h in enumerate(self.edge_heads)])


def test_render_track_sample_trains():
    from connecting_the_dots_amd import torchext as te
    from connecting_the_dots_amd.train import TrackTrainer
    H, W, TL = 96, 128, 2
    sc = workloads.render_scene(3, H=H, W=W)
    K = sc["cam"][0]
    pat = workloads.syn_dot_pattern(H, W)
    pat3 = torch.from_numpy(np.ascontiguousarray(np.stack([pat] * 3, axis=2))).cuda()
    sizes = [(H >> s, W >> s) for s in range(4)]
    pats = [p.contiguous() for p in synth.scale_patterns(pat3, sizes)]
    rng = np.random.RandomState(0)
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    samples = [synth.render_track_sample(sc, pats, K, rng, track_length=TL, sample_id=0),
               synth.render_track_sample(sc, pats, K, rng, track_length=TL, generator=g, sample_id=1)]
    for smp in samples:
        for s in range(4):
            for key in ("im", "ambient", "grad"):
                assert tuple(smp["%s%d" % (key, s)].shape) == (TL, 1) + sizes[s]
            gr = smp["grad%d" % s]
            assert (gr >= 0).all() and (gr <= 1).all()
            if min(sizes[s]) > 10:
                assert (gr[..., :5, :] == 0).all() and (gr[..., :, -5:] == 0).all()
            im = smp["im%d" % s]
            assert (im >= 0).all() and (im <= 1).all()
        assert (smp["grad0"] > 0).any()
        assert torch.isfinite(smp["disp0"][smp["disp0"] > 0]).all()
    batch = synth.collate_tracks(samples)
    assert tuple(batch["im0"].shape) == (TL, 2, 1, H, W) and tuple(batch["R"].shape) == (TL, 2, 3, 3)
    assert tuple(batch["t"].shape) == (TL, 2, 3) and tuple(batch["id"].shape) == (2,)
    lpats = [te.lcn(p[..., 0][None, None].contiguous(), 5, 0.05)[0] for p in pats]
    Kt = torch.from_numpy(K).cuda()
    torch.manual_seed(0)
    tr = TrackTrainer(TinyNet(64).cuda(), lpats, Kt, 0.075, [float(K[0, 0]) / 2 ** s for s in range(4)], train_edge=-1)
    vals = tr.train_step(batch)
    assert len(vals) > 0 and all(np.isfinite(v) for v in vals)
