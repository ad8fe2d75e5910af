"""Times the sub-pixel refinement alone and end to end:
  - xcorrvol_subpixel (parabola) at BASELINE config 2 (16 x 432 x 512, D 128, block 9, the bench's LCN'd synthetic frames
    against the LCN'd dot pattern), without and with a prepared pattern (pattern planes kept between calls);
  - costvol_subpixel (equiangular) for census_sad and sad at config 4 (1024 x 1024 x 256, block 9, eps 0.5);
  - xcorrvol_argmax at config 2 with subpixel=None and subpixel="parabola".
    python tools/time_subpixel.py [--reps 50]
Device time from HIP events around each call, after warm-up launches; median / min / max over the repetitions."""
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
    fmt = "%-58s %.4f / %.4f / %.4f ms"

    N, H, W, D, BS = 16, 432, 512, 128, 9
    rs = np.random.RandomState(2)
    pat = workloads.syn_dot_pattern(H, W, seed=42)
    raw = torch.from_numpy(np.stack([workloads.synth_ir(pat, rs, D)[0] for _ in range(N)])[:, None]).cuda()
    x = te.lcn(raw, 5, 0.05)[0]
    p = te.lcn(torch.from_numpy(pat[None, None]).cuda(), 5, 0.05)[0][0].contiguous()
    idx = te.xcorrvol_argmax(x, p, D, BS)[0]
    print("config 2: %d x %dx%d, D %d, block %d, median / min / max of %d launches (device time, HIP events)"
          % (N, W, H, D, BS, args.reps))
    print(fmt % (("xcorrvol_subpixel parabola",) + median_ms(lambda: te.xcorrvol_subpixel(x, p, idx, D, BS), args.reps)))
    h = te.prepare_pattern(p, N, D, BS)
    print(fmt % (("xcorrvol_subpixel parabola, prepared pattern",)
                 + median_ms(lambda: te.xcorrvol_subpixel(x, p, idx, D, BS, prepared=h), args.reps)))
    plain = median_ms(lambda: te.xcorrvol_argmax(x, p, D, BS), args.reps)
    refined = median_ms(lambda: te.xcorrvol_argmax(x, p, D, BS, subpixel="parabola"), args.reps)
    print(fmt % (("xcorrvol_argmax", ) + plain))
    print(fmt % (("xcorrvol_argmax subpixel=parabola", ) + refined))
    print("%-58s %.4f ms" % ("  difference of the medians", refined[0] - plain[0]), flush=True)

    H = W = 1024
    D = 256
    xc, _ = te.lcn(torch.from_numpy(workloads.uniform_frame(77, H, W)[None]).cuda(), 5, 0.05)
    pc, _ = te.lcn(torch.from_numpy(workloads.syn_dot_pattern(H, W, seed=42)[None, None]).cuda(), 5, 0.05)
    xc, pc = xc[0].contiguous(), pc[0, 0].contiguous()
    print("config 4: %dx%dx%d, block %d" % (W, H, D, BS))
    for kind in ("census_sad", "sad"):
        ci = te.costvol_argmin(xc, pc, D, BS, kind, 0.5)[0]
        print(fmt % (("costvol_subpixel equiangular %s" % kind,)
                     + median_ms(lambda: te.costvol_subpixel(xc, pc, ci, D, BS, kind, 0.5), args.reps)), flush=True)


if __name__ == "__main__":
    main()
