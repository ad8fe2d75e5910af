"""Times the semi-global aggregation (csrc/sgm.hip) at BASELINE config 2 (16 x 432 x 512, D 128; the block-9 SAD volume
of the bench's LCN'd synthetic frames against the LCN'd dot pattern), for 4 and 8 paths:
  (a) sgm_aggregate: device time, the bytes the algorithm moves (3 V per path: the first direction reads C and stores
      S, every other one reads C and S and stores S, the argmin reads S) and the implied fraction of the 6.29 TB/s a
      float4 copy reaches on this card;
  (b) costvol (the volume's own price), for scale;
  (c) the same recurrence restated in plain torch ops on the same card: slab-wise tensor ops, one step per row or
      column.  Its indices are compared with (a)'s.
    python tools/time_sgm.py [--reps 10] [--out profiles/sgm.txt]
Device time from HIP events around each call, after warm-up launches; median / min / max over the repetitions
(10; the torch restatement: 2 after one warm-up).  Exits non-zero if the HIP path is not faster than the torch restatement."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from connecting_the_dots_amd import torchext as te  # noqa: E402
from tests import sgm_ref, workloads  # noqa: E402

COPY_RATE = 6.29e12                    # bytes / s, float4 copy on an MI355X
P1, P2 = 0.02, 0.16
FMT = "%-58s %.3f / %.3f / %.3f ms"


def median_ms(fn, reps, warmup=3):
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


def torch_step(Cp, Lq, p1, p2):
    """Cp, Lq [N, D, n]"""
    m = Lq.amin(1, keepdim=True)
    t = torch.minimum(Lq, m + p2)
    t[:, 1:] = torch.minimum(t[:, 1:], Lq[:, :-1] + p1)
    t[:, :-1] = torch.minimum(t[:, :-1], Lq[:, 1:] + p1)
    return Cp + (t - m)


def torch_path(C, dy, dx, p1, p2):
    N, D, H, W = C.shape
    L = C.clone()
    if dy == 0:
        for x in (range(1, W) if dx > 0 else range(W - 2, -1, -1)):
            L[..., x] = torch_step(C[..., x], L[..., x - dx], p1, p2)
        return L
    lo, hi = max(dx, 0), W + min(dx, 0)                      # columns whose predecessor is inside the image
    for y in (range(1, H) if dy > 0 else range(H - 2, -1, -1)):
        L[:, :, y, lo:hi] = torch_step(C[:, :, y, lo:hi], L[:, :, y - dy, lo - dx:hi - dx], p1, p2)
    return L


def torch_sgm(C, p1, p2, paths):
    S = None
    for dy, dx in sgm_ref.directions(paths):
        L = torch_path(C, dy, dx, p1, p2)
        S = L if S is None else S.add_(L)
    best, idx = S.min(1)
    return idx, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgm.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_sgm.py needs a GPU"

    N, H, W, D, BS = 16, 432, 512, 128, 9
    rs = np.random.RandomState(2)
    pat = workloads.syn_dot_pattern(H, W, seed=42)
    raw = torch.from_numpy(np.stack([workloads.synth_ir(pat, rs, D)[0] for _ in range(N)])[:, None]).cuda()
    im = te.lcn(raw, 5, 0.05)[0][:, 0].contiguous()
    pt = te.lcn(torch.from_numpy(pat[None, None]).cuda(), 5, 0.05)[0][0, 0].contiguous()
    vol = te.costvol(im, pt, D, BS, "sad", 0.5)
    V = 4 * vol.numel()

    lines = ["config 2: %d x %dx%d, D %d, block-%d SAD volume (V = %.3f GB), P1 %g, P2 %g; median / min / max of %d "
             "launches (device time, HIP events)" % (N, W, H, D, BS, V / 1e9, P1, P2, args.reps)]
    lines.append(FMT % (("(b) costvol sad (default algo), for scale",) + median_ms(
        lambda: te.costvol(im, pt, D, BS, "sad", 0.5), args.reps)))
    ok = True
    for paths in (4, 8):
        hip = median_ms(lambda: te.sgm_aggregate(vol, P1, P2, paths), args.reps)
        moved = 3 * paths * V
        lines.append(FMT % (("(a) sgm_aggregate paths=%d" % paths,) + hip))
        lines.append("    bytes moved by the algorithm %.2f GB (%d V) -> %.2f TB/s = %.1f %% of the %.2f TB/s copy rate" % (
            moved / 1e9, 3 * paths, moved / hip[0] / 1e9, 100.0 * moved / (hip[0] * 1e-3) / COPY_RATE, COPY_RATE / 1e12))
        ref = median_ms(lambda: torch_sgm(vol, P1, P2, paths), args.torch_reps, 1)
        lines.append(FMT % (("(c) torch-ops restatement paths=%d (%d launches)" % (paths, args.torch_reps),) + ref))
        idx = te.sgm_aggregate(vol, P1, P2, paths)[0]
        differ = int((idx != torch_sgm(vol, P1, P2, paths)[0]).sum())
        lines.append("    torch / HIP = %.1f x; indices differing between the two: %d of %d" % (
            ref[0] / hip[0], differ, idx.numel()))
        ok = ok and hip[0] < ref[0]
        print("\n".join(lines[-4:]), flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    if not ok:
        sys.exit("the HIP path is not faster than the torch restatement")


if __name__ == "__main__":
    main()
