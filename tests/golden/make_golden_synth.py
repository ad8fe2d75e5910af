"""Generate tests/golden/synth_augment.npz by running the reference's own `data/commons.augment_image`.

    python tests/golden/make_golden_synth.py <reference checkout>

cv2 is not needed: a stand-in module whose GaussianBlur records its sigma and returns its input is installed first
(with max_shift = 0 nothing else of cv2 is reached).  The RandomState handed to augment_image is wrapped so that every
draw it makes is recorded as it happens; the fixture stores, per case, the input images, the recorded sigmas, the
draws (blur and s&p coins, the noise term randn * u / 255 in float64 and u, the s&p ratio and index lists) and the
output cast to float32 as data/dataset.py:116 does.  Only this data is written; no reference source is stored.
"""
import os
import sys
import types

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "synth_augment.npz")

# (seed, image shapes, max_sp_noise): dataset settings, and a larger s&p ratio so that the small images get indices
CASES = [(0, [(24, 40)] * 3 + [(7, 9)], 0.0005), (1, [(24, 40)] * 3 + [(7, 9)], 0.05),
         (2, [(24, 40)] * 3 + [(7, 9)], 0.05), (3, [(24, 40)] * 3 + [(7, 9)], 0.2)]


class Recorder:
    """Passes uniform / randn / choice through to a RandomState and records each result in call order."""

    def __init__(self, rng):
        self.rng, self.log = rng, []

    def uniform(self, *a, **k):
        v = self.rng.uniform(*a, **k)
        self.log.append(("uniform", v))
        return v

    def randn(self, *a):
        v = self.rng.randn(*a)
        self.log.append(("randn", v))
        return v

    def choice(self, *a, **k):
        v = self.rng.choice(*a, **k)
        self.log.append(("choice", v))
        return v


def images(rs, shapes):
    out = []
    for H, W in shapes:
        im = rs.uniform(0.2, 0.6, size=(H, W)).astype(np.float32)
        im[rs.randint(H), rs.randint(W)] = 0.97          # an outlying bright pixel: salt takes its value
        im[rs.randint(H), rs.randint(W)] = 0.05
        out.append(im)
    return out


def main(ref):
    sys.path.insert(0, ref)
    sys.path.insert(0, os.path.join(ref, "data"))
    sigmas = []
    cv2 = types.ModuleType("cv2")

    def gaussian_blur(img, ksize, sigma):
        assert tuple(ksize) == (5, 5)
        sigmas.append(sigma)
        return img
    cv2.GaussianBlur = gaussian_blur
    sys.modules["cv2"] = cv2
    import commons                                       # the reference's data/commons.py

    data = {}
    for ci, (seed, shapes, sp) in enumerate(CASES):
        ims = images(np.random.RandomState(1000 + seed), shapes)
        rec = Recorder(np.random.RandomState(seed))
        for i, im in enumerate(ims):
            del sigmas[:]
            n0 = len(rec.log)
            out, _, _ = commons.augment_image(im, rec, max_shift=0, max_blur=0.5, max_noise=3.0, max_sp_noise=sp)
            log = rec.log[n0:]
            names = [n for n, _ in log]
            assert names[0] == "uniform"
            blur = bool(log[0][1] < 0.5)
            j = 2 if blur else 1
            assert names[j] == "randn" and names[j + 1] == "uniform" and names[j + 2] == "uniform"
            r, u = log[j][1], log[j + 1][1]
            s_p = bool(log[j + 2][1] < 0.5)
            ratio, salt, pepper = 0.0, np.zeros(0, np.int64), np.zeros(0, np.int64)
            if s_p:
                ratio, salt, pepper = log[j + 3][1], log[j + 4][1], log[j + 5][1]
            assert len(sigmas) == int(blur)
            key = "c%d_%d_" % (ci, i)
            data[key + "img"] = im
            data[key + "out"] = np.asarray(out).astype(np.float32)
            data[key + "blur"] = np.array(blur)
            data[key + "sigma"] = np.array(sigmas[0] if blur else np.nan, np.float64)
            data[key + "u"] = np.array(u, np.float64)
            data[key + "noise"] = r * u / 255.0              # the reference's f64 noise term
            data[key + "sp"] = np.array(s_p)
            data[key + "ratio"] = np.array(ratio, np.float64)
            data[key + "salt"] = np.asarray(salt, np.int64)
            data[key + "pepper"] = np.asarray(pepper, np.int64)
        data["c%d_meta" % ci] = np.array([seed, len(shapes)], np.int64)
        data["c%d_max_sp_noise" % ci] = np.array(sp, np.float64)
    np.savez_compressed(OUT, **data)
    print("wrote", OUT, "(%d arrays)" % len(data))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
