"""Times the volume-free cost argmin (torchext.costvol_argmin) at BASELINE config 4 (1024 x 1024 x 256, block 9, eps 0.5,
the bench's LCN'd uniform frame against the LCN'd dot pattern) for census_sad and sad, against the unfused pair
costvol(algo="fast") + torch.argmin, and reports the work-list length (pixels re-scored in the reference order):
    python tools/time_costvol_argmin.py [--reps 50]
Device time from HIP events around each call, after warm-up launches; the median over the repetitions is reported."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from connecting_the_dots_amd import torchext as te  # noqa: E402
from tests import workloads  # noqa: E402


def median_ms(fn, reps, warmup=10):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    H = W = 1024
    D, BS = 256, 9
    x, _ = te.lcn(torch.from_numpy(workloads.uniform_frame(77, H, W)[None]).cuda(), 5, 0.05)
    p, _ = te.lcn(torch.from_numpy(workloads.syn_dot_pattern(H, W, seed=42)[None, None]).cuda(), 5, 0.05)
    x, p = x[0].contiguous(), p[0, 0].contiguous()
    print("config 4: %dx%dx%d, block %d, median / min / max of %d launches (device time, HIP events)" % (W, H, D, BS, args.reps))
    for kind in ("census_sad", "sad"):
        _, _, rescored = te.costvol_argmin(x, p, D, BS, kind, 0.5, return_rescored=True)
        fused = median_ms(lambda: te.costvol_argmin(x, p, D, BS, kind, 0.5), args.reps)
        plain = median_ms(lambda: te.costvol_argmin(x, p, D, BS, kind, 0.5, rerank_rel=-1), args.reps)
        unfused = median_ms(lambda: te.costvol(x, p, D, BS, kind, 0.5, algo="fast").argmin(1), args.reps)
        print("%-10s costvol_argmin %.3f / %.3f / %.3f ms (work list %d of %d pixels)  rerank_rel=-1 %.3f ms  "
              "costvol(fast) + argmin %.3f / %.3f / %.3f ms" % (kind, *fused, rescored.numel(), H * W, plain[0], *unfused),
              flush=True)


if __name__ == "__main__":
    main()
