"""Generate tests/golden/hyperdepth_train.npz: the reference HyperDepth trainer's held-out quality (build machine only).

    python tests/golden/make_golden_hyperdepth_train.py <reference checkout> [runs]

The reference's hyperdepth/hyperdepth.pyx is compiled the way tests/golden/make_golden_hyperdepth.py does it
(cythonized into a temporary directory, g++ -O3 -fopenmp against the checkout's headers); nothing of it is copied.

The data is a small procedural structured-light set: one seeded dot pattern, blurred, seen through piecewise-planar
disparities (2 or 3 planes per frame, split by a random line), with sensor noise; 12 training and 4 held-out frames of
48 x 128.  The reference's `train_forest` seeds itself from std::random_device, so every run gives other forests: it is
run `runs` times (default 5) at the pyx defaults (n_disp_bins 10, depth_switch 0), each run's forests are evaluated on
the held-out frames by the reference's own `eval_forest`, and the fixture records per run
    [share of valid pixels with |error| < 1, share with |error| < 0.5, mean |error| of the pixels with |error| < 1]
(valid: a held-out pixel whose disparity gives a training class, the sample rule of ctd_hyperdepth_train_f32) and the
trainer's wall time (48 rows, 4 OpenMP threads, this machine's CPU).
"""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hyperdepth_train.npz")

from tests.golden.make_golden_hyperdepth import build_reference  # noqa: E402

N_TRAIN, N_TEST, H, W = 12, 4, 48, 128
N_DISP_BINS, DEPTH_SWITCH = 10, 0


def make_data(seed=2024):
    """ims u8 [16, H, W] and disps f32 [16, H, W]; frames 0..11 train, 12..15 held out."""
    rs = np.random.RandomState(seed)
    Wp = W + 8
    dots = (rs.rand(H, Wp) < 0.3).astype(np.float64) * 255.0
    pat = dots.copy()                                       # 1-2-1 blur along the rows
    pat[:, 1:-1] = 0.25 * dots[:, :-2] + 0.5 * dots[:, 1:-1] + 0.25 * dots[:, 2:]
    n = N_TRAIN + N_TEST
    ims = np.empty((n, H, W), np.uint8)
    disps = np.empty((n, H, W), np.float32)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    for f in range(n):
        k = rs.randint(2, 4)
        # region label: which side of up to two random lines the pixel lies on
        label = np.zeros((H, W), np.int64)
        for j in range(k - 1):
            ang = rs.uniform(0, np.pi)
            cx, cy = rs.uniform(0.2, 0.8) * W, rs.uniform(0.2, 0.8) * H
            label += ((xx - cx) * np.cos(ang) + (yy - cy) * np.sin(ang) > 0).astype(np.int64)
        d = np.empty((H, W))
        for j in range(k):
            a, b, c = rs.uniform(4, 20), rs.uniform(-3, 3), rs.uniform(-3, 3)
            d = np.where(label == j, a + b * xx / W + c * yy / H, d)
        d = np.clip(d, 0.5, None)
        proj = xx - d
        x0 = np.floor(proj).astype(np.int64)
        t = proj - x0
        x0c, x1c = np.clip(x0, 0, Wp - 1), np.clip(x0 + 1, 0, Wp - 1)
        rows = np.arange(H)[:, None]
        v = (1 - t) * pat[rows, x0c] + t * pat[rows, x1c] + rs.randn(H, W) * 8.0
        ims[f] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
        disps[f] = d.astype(np.float32)
    return ims, disps


def metrics(est, disps):
    """[< 1 px share, < 0.5 px share, inlier MAE] over the valid pixels (the training sample rule)."""
    col = np.arange(disps.shape[2], dtype=np.float32)[None, None]
    with np.errstate(invalid="ignore"):
        p = (col - disps) * np.float32(N_DISP_BINS)
        valid = (disps >= 0) & (p > -1)
    err = np.abs(est[..., 0] - disps)[valid]
    inl = err < 1
    return np.array([inl.mean(), (err < 0.5).mean(), err[inl].mean() if inl.any() else np.nan])


def main():
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    runs = int(sys.argv[2]) if len(sys.argv) == 3 else 5
    hdm = build_reference(os.path.abspath(sys.argv[1]))
    ims, disps = make_data()
    tr_i, tr_d = np.ascontiguousarray(ims[:N_TRAIN]), np.ascontiguousarray(disps[:N_TRAIN])
    te_i, te_d = np.ascontiguousarray(ims[N_TRAIN:]), np.ascontiguousarray(disps[N_TRAIN:])
    res, secs = [], []
    for r in range(runs):
        tmp = tempfile.mkdtemp(prefix="ctd_hd_train_ref_")
        prefix = os.path.join(tmp, "fr")
        t0 = time.perf_counter()
        hdm.train_forest(hdm.TrainParams(), tr_i, tr_d, n_disp_bins=N_DISP_BINS, depth_switch=DEPTH_SWITCH,
                         n_threads=4, forest_prefix=prefix)
        secs.append(time.perf_counter() - t0)
        est = hdm.eval_forest(te_i, te_d, n_disp_bins=N_DISP_BINS, depth_switch=DEPTH_SWITCH, n_threads=4,
                              forest_prefix=prefix)
        res.append(metrics(est, te_d))
        print("run %d: %.2f s, metrics %s" % (r, secs[-1], res[-1]), flush=True)
    np.savez_compressed(OUT, ims=ims, disps=disps, n_train=N_TRAIN, n_disp_bins=N_DISP_BINS,
                        depth_switch=DEPTH_SWITCH, ref_metrics=np.asarray(res), ref_seconds=np.asarray(secs))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
