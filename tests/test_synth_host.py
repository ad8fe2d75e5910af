"""CPU checks of connecting_the_dots_amd.synth: the numpy draw stream of the augmentation against the draws the
reference's own augment_image made (tests/golden/synth_augment.npz), the Gaussian taps, the track poses, the pattern
pyramid and argument errors."""
import os

import numpy as np
import pytest
import torch

from connecting_the_dots_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "synth_augment.npz")


def _cases():
    z = np.load(GOLDEN)
    c = 0
    while "c%d_meta" % c in z:
        seed, n = (int(v) for v in z["c%d_meta" % c])
        yield z, c, seed, n, float(z["c%d_max_sp_noise" % c])
        c += 1


def test_rng_draws_equal_the_reference_stream():
    n_sp = 0
    for z, c, seed, n, sp in _cases():
        rng = np.random.RandomState(seed)
        for i in range(n):
            k = "c%d_%d_" % (c, i)
            H, W = z[k + "img"].shape
            d = synth.draw_augment(rng, 1, H, W, max_blur=0.5, max_noise=3.0, max_sp_noise=sp)[0]
            assert d["blur"] == bool(z[k + "blur"])
            if d["blur"]:
                assert d["sigma"] == float(z[k + "sigma"])
            assert d["u"] == float(z[k + "u"])
            assert np.array_equal(d["noise"], z[k + "noise"])
            assert d["sp"] == bool(z[k + "sp"])
            assert d["ratio"] == float(z[k + "ratio"])
            assert np.array_equal(d["salt"], z[k + "salt"]) and np.array_equal(d["pepper"], z[k + "pepper"])
            n_sp += len(d["salt"])
    assert n_sp > 0                                       # the fixture exercises salt and pepper


def test_rng_path_without_blur_or_sp_reproduces_the_fixture_on_the_host():
    """the draws alone rebuild the reference output where neither blur nor s&p applies (x + noise, clip, f32)"""
    seen = 0
    for z, c, seed, n, sp in _cases():
        for i in range(n):
            k = "c%d_%d_" % (c, i)
            if bool(z[k + "blur"]) or len(z[k + "salt"]):
                continue
            v = np.clip(z[k + "img"].astype(np.float64) + z[k + "noise"], 0.0, 1.0).astype(np.float32)
            assert np.array_equal(v, z[k + "out"])
            seen += 1
    assert seen > 0


def test_gaussian_taps_match_their_float64_definition():
    for sigma in (0.2, 0.3371, 0.5, 1.5):
        x = np.arange(-2, 3, dtype=np.float64)
        e = np.exp(-x * x / (2 * sigma * sigma))
        ref = (e / e.sum()).astype(np.float32)
        k = synth.gaussian_taps(sigma)
        assert k.dtype == np.float32 and np.array_equal(k, ref)
        assert abs(float(k.astype(np.float64).sum()) - 1.0) < 1e-6
        assert np.array_equal(k, k[::-1])
    assert synth.gaussian_taps([0.3, 0.4]).shape == (2, 5)


def test_sample_track_poses():
    rng = np.random.RandomState(7)
    p = synth.sample_track_poses(rng, track_length=4, baseline=0.075, blend_im=0.6)
    assert p["R"].shape == (4, 3, 3) and p["t"].shape == (4, 3) and p["R"].dtype == np.float32
    assert 0.5 <= p["blend_im"] <= 0.7
    center = np.array([0, 0, 3.0])
    for R, t, Rp, tp in zip(p["R"], p["t"], p["R_proj"], p["t_proj"]):
        R64 = R.astype(np.float64)
        assert np.abs(R64 @ R64.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R64) - 1) < 1e-6
        # get_rotation_matrix(center, center - t) takes the direction of the centre to that of centre - t
        a = center / np.linalg.norm(center)
        b = (center - t) / np.linalg.norm(center - t)
        assert np.abs(R64 @ a - b).max() < 1e-6
        assert np.array_equal(Rp, R) and np.allclose(tp, t + np.array([-0.075, 0, 0], np.float32), atol=0)
        assert np.all(np.abs(t) <= 0.3 + 1e-7)
    # the reference's order: 3 + 1 + 3 per frame uniforms
    rng2 = np.random.RandomState(7)
    u = rng2.uniform(size=3 + 1 + 3 * 4)
    assert rng.uniform() == rng2.uniform()
    assert p["t"][0][0] == np.float32((u[0] * 0.4 - 0.2) + (u[4] * 0.2 - 0.1))


def test_scale_patterns_is_cv2_linear_resize_of_the_full_pattern():
    rs = np.random.RandomState(3)
    pat = (rs.uniform(size=(48, 64, 3)) < 0.3).astype(np.float32) * rs.uniform(size=(48, 64, 3)).astype(np.float32)
    sizes = [(48, 64), (24, 32), (12, 16), (6, 8)]
    lv = synth.scale_patterns(torch.from_numpy(pat), sizes)
    assert [tuple(l.shape[:2]) for l in lv] == sizes
    assert torch.equal(lv[0], torch.from_numpy(pat))
    # level 1: the mean of each 2x2 block
    m = pat.reshape(24, 2, 32, 2, 3)
    ref1 = 0.5 * (0.5 * (m[:, 0, :, 0] + m[:, 0, :, 1])) + 0.5 * (0.5 * (m[:, 1, :, 0] + m[:, 1, :, 1]))
    assert np.array_equal(lv[1].numpy(), ref1)
    assert np.allclose(lv[1].numpy(), m.mean(axis=(1, 3)), rtol=0, atol=1e-7)
    # deeper levels: bilinear samples at f*d + (f-1)/2 of the full-resolution pattern (centre 2x2 of each block)
    for s in (2, 3):
        f = 2 ** s
        h, w = sizes[s]
        ref = np.zeros((h, w, 3), np.float64)
        for y in range(h):
            for x in range(w):
                sy, sx = f * y + (f - 1) / 2, f * x + (f - 1) / 2
                y0, x0 = int(np.floor(sy)), int(np.floor(sx))
                wy, wx = sy - y0, sx - x0
                ref[y, x] = ((1 - wy) * ((1 - wx) * pat[y0, x0] + wx * pat[y0, x0 + 1]) +
                             wy * ((1 - wx) * pat[y0 + 1, x0] + wx * pat[y0 + 1, x0 + 1]))
        assert np.allclose(lv[s].numpy(), ref, rtol=0, atol=1e-7)
    assert len(synth.scale_patterns(torch.from_numpy(pat[..., 0]), sizes[:2])) == 2


def test_argument_errors():
    with pytest.raises(ValueError):
        synth.scale_patterns(torch.zeros(48, 64), [(48, 64), (24, 30)])
    with pytest.raises(ValueError):
        synth.scale_patterns(torch.zeros(48, 64), [(40, 64)])
    with pytest.raises(ValueError):
        synth.scale_patterns(torch.zeros(6, 6), [(6, 6), (3, 3), (1, 1)])          # 3 is not halved exactly
    with pytest.raises(NotImplementedError):
        synth.draw_augment(np.random.RandomState(0), 1, 8, 8, max_shift=64)
    with pytest.raises(NotImplementedError):
        synth.augment(torch.zeros(1, 1, 8, 8), rng=np.random.RandomState(0), max_shift=2)
    with pytest.raises(RuntimeError):                                               # CPU tensors are refused
        synth.augment(torch.zeros(1, 1, 8, 8), rng=np.random.RandomState(0))
    with pytest.raises(RuntimeError):
        synth.finish_render(torch.zeros(1, 8, 8), torch.zeros(1, 8, 8, 3), torch.zeros(1, 8, 8, 3), 0.6, 0.075, 500.0)
    with pytest.raises(ValueError):
        synth.collate_tracks([])


def test_c_abi_validates_before_touching_the_device():
    from connecting_the_dots_amd import _lib
    L = _lib.lib()
    assert L.ctd_syn_finish_f32(None, None, None, None, 1.0, 0.8, 5, 0.1, 1, None, None, None, None, None, 1, 0, 8, -1,
                                None) == 1
    assert L.ctd_syn_finish_f32(None, None, None, None, 1.0, 0.8, -1, 0.1, 1, None, None, None, None, None, 1, 8, 8, -1,
                                None) == 1
    assert L.ctd_syn_finish_f32(None, None, None, None, 1.0, 0.8, 5, 0.1, 1, None, None, None, None, None, 1, 8, 8, -1,
                                None) == 1                                          # null pointers
    assert L.ctd_syn_finish_f32(None, None, None, None, 1.0, 0.8, 5, 0.1, 1, None, None, None, None, None, 0, 8, 8, -1,
                                None) == 0                                          # nothing to do
    assert L.ctd_augment_f32(None, None, 2, None, None, None, 1, 8, 8, -1, None) == 1
    assert L.ctd_augment_f32(None, None, 0, None, None, None, 1, 8, 8, -1, None) == 1
    assert L.ctd_augment_f32(None, None, 0, None, None, None, 1, 65536, 65536, -1, None) == 1
    assert L.ctd_salt_pepper_f32(None, None, None, None, None, -1, 1, 8, 8, -1, None) == 1
    assert L.ctd_salt_pepper_f32(None, None, None, None, None, 4, 1, 8, 8, -1, None) == 1
    assert L.ctd_salt_pepper_f32(None, None, None, None, None, 0, 1, 8, 8, -1, None) == 0
    assert np.dtype(synth.AUGMENT_PARAMS).itemsize == 32
