"""Times the match-validity ops (csrc/match_validity.hip):
  (a) the scan of a materialised volume (match_validity = scan + flag kernel) against argmax_disp on the same volume,
      both of which read the volume once;
  (b) the whole xcorrvol_validity call (fast and exact) against xcorrvol_argmax(return_volume=True);
  (c) the share of pixels and pattern columns the fast path settles by exact re-scoring;
at BASELINE config 2 (16 x 432 x 512, D 128, block 9, the bench's LCN'd synthetic frames against the LCN'd dot pattern)
and on one config-4 frame (1024 x 1024, D 256; NCC, and the census_sad / sad costs).
    python tools/time_match_validity.py [--reps 30]
Device time from HIP events around each call, after warm-up launches; median / min / max over the repetitions."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from connecting_the_dots_amd import torchext as te  # noqa: E402
from tests import workloads  # noqa: E402

MIN_GAP = 0.05
FMT = "%-62s %.4f / %.4f / %.4f ms"


def median_ms(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def ncc_block(x, p, D, BS, reps):
    P = x.shape[0] * x.shape[2] * x.shape[3]
    idx, _, vol = te.xcorrvol_argmax(x, p, D, BS, return_volume=True)
    arg = median_ms(lambda: te.argmax_disp(vol), reps)
    scan = median_ms(lambda: te.match_validity(vol, idx, True, 1, MIN_GAP), reps)
    print(FMT % (("(a) argmax_disp on the volume",) + arg))
    print(FMT % (("(a) match_validity on the volume (scan + flag kernel)",) + scan))
    print("%-62s %.2f x" % ("    ratio of the medians", scan[0] / arg[0]))
    del vol
    base = median_ms(lambda: te.xcorrvol_argmax(x, p, D, BS, return_volume=True), reps)
    fast = median_ms(lambda: te.xcorrvol_validity(x, p, idx, D, BS, 1, MIN_GAP, algo="fast"), reps)
    print(FMT % (("(b) xcorrvol_argmax(return_volume=True)",) + base))
    print(FMT % (("(b) xcorrvol_validity algo=fast",) + fast))
    exact = median_ms(lambda: te.xcorrvol_validity(x, p, idx, D, BS, 1, MIN_GAP, algo="exact"), max(3, reps // 5), 2)
    print(FMT % (("(b) xcorrvol_validity algo=exact",) + exact))
    out = te.xcorrvol_validity(x, p, idx, D, BS, 1, MIN_GAP, algo="fast", return_rescored=True)
    valid = int((out[0] == 7).sum())
    print("(c) re-scored: %d pixels (%.4f %%), %d pattern columns (%.4f %%) of %d; valid %.1f %% (min_gap %g, lr_tol 1)"
          % (out[3].numel(), 100.0 * out[3].numel() / P, out[4].numel(), 100.0 * out[4].numel() / P, P, 100.0 * valid / P,
             MIN_GAP), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()

    N, H, W, D, BS = 16, 432, 512, 128, 9
    rs = np.random.RandomState(2)
    pat = workloads.syn_dot_pattern(H, W, seed=42)
    raw = torch.from_numpy(np.stack([workloads.synth_ir(pat, rs, D)[0] for _ in range(N)])[:, None]).cuda()
    x = te.lcn(raw, 5, 0.05)[0]
    p = te.lcn(torch.from_numpy(pat[None, None]).cuda(), 5, 0.05)[0][0].contiguous()
    print("config 2: %d x %dx%d, D %d, block %d, median / min / max of %d launches (device time, HIP events)"
          % (N, W, H, D, BS, args.reps))
    ncc_block(x, p, D, BS, args.reps)
    del x, raw

    H = W = 1024
    D = 256
    pat = workloads.syn_dot_pattern(H, W, seed=42)
    raw = torch.from_numpy(workloads.synth_ir(pat, rs, D)[0][None, None]).cuda()
    xc = te.lcn(raw, 5, 0.05)[0]
    pc = te.lcn(torch.from_numpy(pat[None, None]).cuda(), 5, 0.05)[0][0].contiguous()
    print("config 4, one frame: %dx%d, D %d, block %d" % (W, H, D, BS))
    ncc_block(xc, pc, D, BS, args.reps)
    im, pt = xc[:, 0].contiguous(), pc[0].contiguous()
    for kind in ("census_sad", "sad"):
        ci = te.costvol_argmin(im, pt, D, BS, kind, 0.5)[0]
        t = median_ms(lambda: te.costvol_validity(im, pt, ci, D, BS, kind, 0.5, 1, 0.0, algo="fast"), args.reps)
        out = te.costvol_validity(im, pt, ci, D, BS, kind, 0.5, 1, 0.0, algo="fast", return_rescored=True)
        print(FMT % (("costvol_validity %s algo=fast (min_gap 0)" % kind,) + t))
        print("    re-scored: %d pixels, %d pattern columns of %d" % (out[3].numel(), out[4].numel(), H * W), flush=True)


if __name__ == "__main__":
    main()
