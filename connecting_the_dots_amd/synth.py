"""Training-sample finishing of the synthetic data path, on the device.

The reference turns a rendered frame into a training sample in two places, both built on OpenCV:
data/create_syn_data.py:152-188 (blend of the reflected pattern with the ambient image, disparity, mask, and the edge
target `grad = clip(lcn.normalize(max(|Sobel5(ambient)| - 0.8, 0), 5, 0.1), 0, 1)`) and data/commons.py:46-107
`augment_image`, applied per scale by data/dataset.py:99-131.  Here:

    finish_render(depth, color, normal, blend, baseline, focal)   -> dict(im, ambient, grad, disp, mask)   (one launch)
    augment(img, rng=... | generator=...)                         -> blurred, noisy, salt-and-peppered copy
    scale_patterns(pattern, imsizes)                              -> the pattern pyramid of commons.get_patterns
    sample_track_poses(rng)                                       -> camera / projector poses of one track
    render_track_sample(mesh, patterns, K, rng)                   -> one sample with the keys of TrackSynDataset
    collate_tracks(samples)                                       -> the [tl, B, 1, H_s, W_s] batch of TrackTrainer

The kernels are ctd_syn_finish_f32, ctd_augment_f32 and ctd_salt_pepper_f32 (include/ctd_hip.h states their operation
orders and exactness claims).  There is no CPU path: a missing library is an error.
"""
import numpy as np
import torch

from . import _lib
from .renderer import MeshBVH, PyCamera, PyShader, render_mesh_proj

# ctd_augment_params of include/ctd_hip.h (32 bytes per image)
AUGMENT_PARAMS = np.dtype([("blur", "<i4"), ("taps", "<f4", (5,)), ("noise_scale", "<f8")])
assert AUGMENT_PARAMS.itemsize == 32

# data/dataset.py:50-53: the augmentation the training set uses
DATASET_AUGMENT = dict(max_shift=0, max_blur=0.5, max_noise=3.0, max_sp_noise=0.0005)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _need(t, name, dtype, ndim=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == dtype):
        raise RuntimeError("%s must be a contiguous CUDA tensor of dtype %s" % (name, dtype))
    if ndim is not None and t.dim() != ndim:
        raise ValueError("%s must have %d dimensions, got shape %s" % (name, ndim, tuple(t.shape)))


def gaussian_taps(sigma):
    """The 5 taps of cv2.GaussianBlur(ksize=5, sigma) as the kernels take them: e_j = exp(-(j-2)^2 / (2 sigma^2)),
    k_j = (float)(e_j / sum(e)), formed in double.  sigma: scalar or array -> f32 [..., 5]."""
    s = np.asarray(sigma, np.float64)[..., None]
    x = np.arange(5, dtype=np.float64) - 2.0
    e = np.exp(-(x * x) / (2.0 * s * s))
    return (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)


def finish_render(depth, color, normal, blend, baseline, focal, grad_threshold=0.8, lcn_radius=5, lcn_eps=0.1,
                  lcn_clip=True, with_disp=True, with_mask=True):
    """create_syn_data.py:163-188 for N frames of one size, in one launch.

    depth [N,H,W], color [N,H,W,3], normal [N,H,W,3] (the ambient image; zero where nothing was hit, as
    render_mesh_proj leaves it): f32 CUDA tensors.  blend: the per-sample `blend_im_rnd`, a float or one value per
    frame (kept in double, as the reference's np.float64).  disp = (baseline * focal) / depth with baseline * focal
    formed in double (focal of this scale: K[0,0] / 2^s).  Returns dict of [N,H,W] f32 tensors: im (blended IR frame),
    ambient, grad (edge target), disp and mask (None when not asked for)."""
    _need(depth, "depth", torch.float32, 3)
    _need(color, "color", torch.float32, 4)
    _need(normal, "normal", torch.float32, 4)
    N, H, W = depth.shape
    if tuple(color.shape) != (N, H, W, 3) or tuple(normal.shape) != (N, H, W, 3):
        raise ValueError("color and normal must be [N,H,W,3] with depth's N, H, W")
    dev = depth.device
    if isinstance(blend, torch.Tensor):
        b = blend.to(device=dev, dtype=torch.float64).reshape(-1)
    else:
        b = torch.as_tensor(np.asarray(blend, np.float64).reshape(-1), device=dev)
    if b.numel() == 1:
        b = b.expand(N)
    if b.numel() != N:
        raise ValueError("blend must be a scalar or have one value per frame")
    b = b.contiguous()
    new = lambda: torch.empty((N, H, W), dtype=torch.float32, device=dev)
    im, amb, grad = new(), new(), new()
    disp = new() if with_disp else None
    mask = new() if with_mask else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    st = _lib.lib().ctd_syn_finish_f32(depth.data_ptr(), color.data_ptr(), normal.data_ptr(), b.data_ptr(),
                                       float(baseline) * float(focal), float(grad_threshold), int(lcn_radius),
                                       float(lcn_eps), int(bool(lcn_clip)), im.data_ptr(), amb.data_ptr(),
                                       grad.data_ptr(), ptr(disp), ptr(mask), N, H, W, dev.index, _stream(dev))
    _lib.check(st, "syn_finish")
    return dict(im=im, ambient=amb, grad=grad, disp=disp, mask=mask)


def draw_augment(rng, n, H, W, max_blur=0.5, max_noise=3.0, max_sp_noise=0.0005, max_shift=0):
    """The draws of commons.augment_image for n images of H x W, from a numpy RandomState, in the reference's order
    (image after image: blur coin, sigma if blurring, randn(H,W), the noise uniform, the s&p coin, and if applying
    salt and pepper the ratio and the two `choice` calls).  Host only.  Returns one dict per image: blur (bool),
    sigma, u (noise uniform), noise (the f64 term randn * u / 255 of the reference), sp (bool), ratio, salt, pepper
    (int64 flat indices)."""
    if max_shift > 1:
        raise NotImplementedError("max_shift > 1 needs cv2.warpAffine shear / shift; the training set uses 0")
    draws = []
    for _ in range(n):
        d = {}
        d["blur"] = bool(rng.uniform(0, 1) < 0.5)
        d["sigma"] = rng.uniform(0.2, max_blur) if d["blur"] else float("nan")
        r = rng.randn(H, W)
        d["u"] = rng.uniform(0.0, max_noise)
        d["noise"] = r * d["u"] / 255.0                     # the reference's expression, evaluated left to right
        d["sp"] = bool(rng.uniform(0, 1) < 0.5)
        d["ratio"], d["salt"], d["pepper"] = 0.0, np.zeros(0, np.int64), np.zeros(0, np.int64)
        if d["sp"]:
            d["ratio"] = rng.uniform(0.0, max_sp_noise)
            k = int(H * W * d["ratio"])
            d["salt"] = rng.choice(H * W, k).astype(np.int64)
            d["pepper"] = rng.choice(H * W, k).astype(np.int64)
        draws.append(d)
    return draws


def _augment_launch(img, noise, noise_f64, params, counts, salt, pepper, kmax):
    N, _, H, W = img.shape
    dev = img.device
    out = torch.empty_like(img)
    minmax = torch.empty((N, 2), dtype=torch.int32, device=dev)
    L = _lib.lib()
    st = L.ctd_augment_f32(img.data_ptr(), noise.data_ptr() if noise is not None else None, int(noise_f64),
                           params.data_ptr(), out.data_ptr(), minmax.data_ptr(), N, H, W, dev.index, _stream(dev))
    _lib.check(st, "augment")
    if kmax > 0:
        st = L.ctd_salt_pepper_f32(out.data_ptr(), minmax.data_ptr(), counts.data_ptr(), salt.data_ptr(),
                                   pepper.data_ptr(), int(kmax), N, H, W, dev.index, _stream(dev))
        _lib.check(st, "salt_pepper")
    return out, minmax


def augment(img, rng=None, generator=None, max_blur=0.5, max_noise=3.0, max_sp_noise=0.0005, max_shift=0,
            return_draws=False):
    """commons.augment_image on every image of img [N,1,H,W] (f32 CUDA) -> new [N,1,H,W] tensor.

    rng (numpy RandomState): the reference's stream draw for draw (draw_augment), the noise drawn on the host in
    float64 -- the output is then bit-identical to augment_image wherever the blur coin is off.  Otherwise the draws
    come from `generator` (a CUDA torch.Generator, or None for the device's default): the same distributions drawn
    with torch on the device, no host synchronisation; salt / pepper index buffers hold int(H*W*max_sp_noise) entries
    per image beside a per-image count.  return_draws: also return the draws (host dicts, or device tensors)."""
    if max_shift > 1:
        raise NotImplementedError("max_shift > 1 needs cv2.warpAffine shear / shift; the training set uses 0")
    _need(img, "img", torch.float32, 4)
    if img.shape[1] != 1:
        raise ValueError("img must be [N,1,H,W]")
    N, _, H, W = img.shape
    dev = img.device
    if N == 0:
        return (img.clone(), None) if return_draws else img.clone()
    if rng is not None:
        draws = draw_augment(rng, N, H, W, max_blur, max_noise, max_sp_noise, max_shift)
        p = np.zeros(N, AUGMENT_PARAMS)
        for i, d in enumerate(draws):
            p[i]["blur"] = int(d["blur"])
            p[i]["taps"] = gaussian_taps(d["sigma"]) if d["blur"] else 0.0
            p[i]["noise_scale"] = 1.0                        # the f64 plane is the whole term
        kmax = max(len(d["salt"]) for d in draws)
        counts = np.array([len(d["salt"]) for d in draws], np.int32)
        salt = np.zeros((N, max(kmax, 1)), np.int64)
        pepper = np.zeros((N, max(kmax, 1)), np.int64)
        for i, d in enumerate(draws):
            salt[i, :len(d["salt"])] = d["salt"]
            pepper[i, :len(d["pepper"])] = d["pepper"]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        noise = up(np.stack([d["noise"] for d in draws]))
        out, _ = _augment_launch(img, noise, 1, up(p.view(np.uint8)), up(counts), up(salt), up(pepper), kmax)
        return (out, draws) if return_draws else out
    g = generator
    f64 = dict(device=dev, dtype=torch.float64, generator=g)
    blur = torch.rand(N, **f64) < 0.5
    sigma = 0.2 + (max_blur - 0.2) * torch.rand(N, **f64)
    x = torch.arange(5, device=dev, dtype=torch.float64) - 2.0
    e = torch.exp(-(x * x) / (2.0 * sigma[:, None] * sigma[:, None]))
    taps = (e / e.sum(dim=1, keepdim=True)).to(torch.float32)
    noise = torch.randn((N, H, W), device=dev, dtype=torch.float32, generator=g)
    scale = torch.rand(N, **f64) * max_noise / 255.0
    sp = torch.rand(N, **f64) < 0.5
    ratio = torch.rand(N, **f64) * max_sp_noise
    kmax = int(H * W * max_sp_noise)
    counts = torch.where(sp, (ratio * float(H * W)).to(torch.int32), torch.zeros_like(ratio, dtype=torch.int32))
    salt = torch.randint(0, H * W, (N, max(kmax, 1)), device=dev, dtype=torch.int64, generator=g)
    pepper = torch.randint(0, H * W, (N, max(kmax, 1)), device=dev, dtype=torch.int64, generator=g)
    params = torch.cat([blur.to(torch.int32)[:, None].view(torch.uint8), taps.view(torch.uint8),
                        scale[:, None].view(torch.uint8)], dim=1).contiguous()
    out, minmax = _augment_launch(img, noise, 0, params, counts, salt, pepper, kmax)
    if return_draws:
        return out, dict(blur=blur, sigma=sigma, taps=taps, noise=noise, scale=scale, sp=sp, ratio=ratio, counts=counts,
                         salt=salt[:, :kmax], pepper=pepper[:, :kmax], minmax=minmax)
    return out


def decode_minmax(words):
    """The [N,2] minmax words of ctd_augment_f32 -> (min, max) f32 numpy arrays (host)."""
    w = np.ascontiguousarray(np.asarray(words).view(np.uint32).reshape(-1, 2))

    def val(k):
        u = np.where(k & 0x80000000, k & 0x7fffffff, ~k).astype(np.uint32)
        return u.view(np.float32)
    return val(~w[:, 0]), val(w[:, 1])


def scale_patterns(pattern, imsizes):
    """commons.get_patterns:27-29: every level is cv2.resize(pattern, (w_s, h_s), INTER_LINEAR) of the FULL-resolution
    pattern.  For a factor f = 2^s that samples the source at f*d + (f-1)/2, i.e. the mean of the centre 2x2 of each
    f x f block (rows / columns f*d + f/2 - 1 and f*d + f/2), formed as cv2 does: the two row interpolations, then the
    column one, weights 0.5 (exact).  At level 1 that is the mean of each 2x2 block.
    pattern: [H,W] or [H,W,C] tensor; imsizes: [(H,W), (H/2,W/2), ...] successive exact halvings."""
    p = pattern if isinstance(pattern, torch.Tensor) else torch.as_tensor(np.asarray(pattern))
    if p.dim() not in (2, 3):
        raise ValueError("pattern must be [H,W] or [H,W,C]")
    sizes = [tuple(int(v) for v in s) for s in imsizes]
    if not sizes or sizes[0] != tuple(p.shape[:2]):
        raise ValueError("imsizes[0] must be the pattern's size %s" % (tuple(p.shape[:2]),))
    for a, b in zip(sizes, sizes[1:]):
        if a[0] % 2 or a[1] % 2 or b != (a[0] // 2, a[1] // 2):
            raise ValueError("imsizes must be successive exact halvings, got %s" % (sizes,))
    out = [p]
    for s in range(1, len(sizes)):
        f = 2 ** s
        h, w = sizes[s]
        r0 = torch.arange(h, device=p.device) * f + f // 2 - 1
        c0 = torch.arange(w, device=p.device) * f + f // 2 - 1
        a, b = p[r0][:, c0], p[r0][:, c0 + 1]
        c, d = p[r0 + 1][:, c0], p[r0 + 1][:, c0 + 1]
        out.append(0.5 * (0.5 * (a + b)) + 0.5 * (0.5 * (c + d)))
    return out


def get_rotation_matrix(v0, v1):
    """commons.get_rotation_matrix: Rodrigues' rotation taking v0 to v1.  The reference builds the cross-product matrix
    from a string ('{}'.format of the f32 components, parsed back as double by np.matrix); this does the same."""
    v0 = v0 / np.linalg.norm(v0)
    v1 = v1 / np.linalg.norm(v1)
    v = np.cross(v0, v1)
    c = np.dot(v0, v1)
    s = np.linalg.norm(v)
    q = [float("{}".format(x)) for x in v]
    k = np.array([[0, -q[2], q[1]], [q[2], 0, -q[0]], [-q[1], q[0], 0]], np.float64)
    r = np.eye(3) + k + k @ k * ((1 - c) / (s ** 2))
    return r.astype(np.float32)


def sample_track_poses(rng, track_length=4, baseline=0.075, blend_im=0.6):
    """create_syn_data.py:98-135 without the scene: consumes `rng` in the reference's order (cam_x_, cam_y_, cam_z_,
    blend_im_rnd, then 3 uniforms per track frame).  Cameras look at (0,0,3); the projector sits at t + [-baseline,0,0]
    with the camera's rotation.  Returns dict(R [tl,3,3], t [tl,3], R_proj, t_proj: f32 numpy, blend_im: float)."""
    center = np.array([0, 0, 3], dtype=np.float32)
    basevec = np.array([-baseline, 0, 0], dtype=np.float32)
    cam_x_ = rng.uniform(-0.2, 0.2)
    cam_y_ = rng.uniform(-0.2, 0.2)
    cam_z_ = rng.uniform(-0.2, 0.2)
    blend_im_rnd = float(np.clip(blend_im + rng.uniform(-0.1, 0.1), 0, 1))
    R, t, Rp, tp = [], [], [], []
    for _ in range(track_length):
        cam_x = cam_x_ + rng.uniform(-0.1, 0.1)
        cam_y = cam_y_ + rng.uniform(-0.1, 0.1)
        cam_z = cam_z_ + rng.uniform(-0.1, 0.1)
        tcam = np.array([cam_x, cam_y, cam_z], dtype=np.float32)
        if np.linalg.norm(tcam[0:2]) < 1e-9:
            Rcam = np.eye(3, dtype=np.float32)
        else:
            Rcam = get_rotation_matrix(center, center - tcam)
        R.append(Rcam)
        t.append(tcam)
        Rp.append(Rcam)
        tp.append(tcam + basevec)
    return dict(R=np.stack(R), t=np.stack(t), R_proj=np.stack(Rp), t_proj=np.stack(tp), blend_im=blend_im_rnd)


def render_track_sample(mesh, patterns, K, rng, track_length=4, blend_im=0.6, baseline=0.075, data_aug=True,
                        generator=None, sample_id=0, aug_params=None, bvh=None):
    """One track of one static scene, on the device: create_syn_data.create_data's per-frame, per-scale loop
    (render_mesh_proj with the reference's shader and decay, then finish_render) followed by TrackSynDataset's
    augmentation (data_aug: every scale's `im`, the draws of dataset.py's settings; with max_shift = 0 disp and grad
    are unchanged).

    mesh: dict(verts [n,3] f32, colors [n,3] f32, faces [m,3] int32) -- numpy or CUDA tensors; patterns: one
    [H_s,W_s,3] f32 CUDA tensor per scale (scale_patterns); K [3,3] intrinsics of scale 0.  `rng` (numpy RandomState)
    draws the poses and -- unless `generator` is given -- the augmentation.
    Returns the keys of data/dataset.py:57-137 as CUDA tensors: im{s}, ambient{s}, grad{s} [tl,1,H_s,W_s], disp0
    [tl,1,H,W], R [tl,3,3], t [tl,3], blend_im (f32 scalar), id.
    bvh: None (brute-force ray casting), a renderer.MeshBVH of this mesh, or 'auto' (one tree built here and used for
    all track_length x scales renders); the result is the same, bit for bit."""
    dev = patterns[0].device
    up = lambda a, dt: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))).to(dev, dt).contiguous()
    verts, colors, faces = up(mesh["verts"], torch.float32), up(mesh["colors"], torch.float32), up(mesh["faces"],
                                                                                                    torch.int32)
    if isinstance(bvh, str):
        if bvh != 'auto':
            raise ValueError("bvh must be None, 'auto' or a MeshBVH")
        bvh = MeshBVH(verts, faces, device=dev)
    elif bvh is not None and not (bvh.verts.shape == verts.shape and bvh.faces.shape == faces.shape and
                                  torch.equal(bvh.verts, verts) and torch.equal(bvh.faces, faces)):
        raise RuntimeError("bvh was built from another mesh")
    if bvh is not None:
        verts, faces = bvh.verts, bvh.faces
    K = np.asarray(K.cpu() if isinstance(K, torch.Tensor) else K, np.float32)
    poses = sample_track_poses(rng, track_length, baseline, blend_im)
    shader = PyShader(0.5, 1.5, 0.0, 10)                               # create_syn_data.py:155
    n_s = len(patterns)
    frames = [[] for _ in range(n_s)]
    for ind in range(track_length):
        for s in range(n_s):
            scale = 1.0 / 2 ** s
            h, w = patterns[s].shape[:2]
            fx, fy, px, py = (float(K[0, 0]) * scale, float(K[1, 1]) * scale, float(K[0, 2]) * scale,
                              float(K[1, 2]) * scale)
            cam = PyCamera(fx, fy, px, py, poses["R"][ind], poses["t"][ind], w, h)
            proj = PyCamera(fx, fy, px, py, poses["R_proj"][ind], poses["t_proj"][ind], w, h)
            frames[s].append(render_mesh_proj(verts, colors, faces, cam, proj, shader, patterns[s], d_alpha=0.0,
                                              d_beta=0.35, bvh=bvh))
    out = {}
    for s in range(n_s):
        depth, color, normal = (torch.stack([f[k] for f in frames[s]]) for k in range(3))
        r = finish_render(depth, color, normal, poses["blend_im"], baseline, float(K[0, 0]) / 2 ** s,
                          with_disp=(s == 0), with_mask=False)
        out["im%d" % s] = r["im"][:, None]
        out["ambient%d" % s] = r["ambient"][:, None]
        out["grad%d" % s] = r["grad"][:, None]
        if s == 0:
            out["disp0"] = r["disp"][:, None]
    if data_aug:
        kw = dict(DATASET_AUGMENT if aug_params is None else aug_params)
        for s in range(n_s):
            src = dict(generator=generator) if generator is not None else dict(rng=rng)
            out["im%d" % s] = augment(out["im%d" % s], **src, **kw)
    out["R"] = torch.from_numpy(poses["R"]).to(dev)
    out["t"] = torch.from_numpy(poses["t"]).to(dev)
    out["blend_im"] = torch.tensor(poses["blend_im"], dtype=torch.float32, device=dev)
    out["id"] = torch.tensor(sample_id, dtype=torch.int64, device=dev)
    return out


def collate_tracks(samples):
    """Stacks render_track_sample outputs into TrackTrainer's batch: image-like keys [tl,B,...] (the track axis first,
    as exp_synphge.Worker.copy_data leaves them), R [tl,B,3,3], t [tl,B,3], blend_im [B], id [B]."""
    if not samples:
        raise ValueError("collate_tracks needs at least one sample")
    out = {}
    for k in samples[0]:
        vals = [smp[k] for smp in samples]
        out[k] = torch.stack(vals, dim=0) if k in ("id", "blend_im") else torch.stack(vals, dim=1).contiguous()
    return out
