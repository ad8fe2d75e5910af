"""Times the disparity post-filters (csrc/disp_filter.hip) at BASELINE config 2 (16 x 432 x 512, D 128) on the int64
indices of `xcorrvol_argmax` for LCN'd synthetic frames with added noise, and on the serpentine frame (one
one-pixel-wide component that covers the frame: the worst case for label propagation across tiles):
  (a) disp_components, disp_speckle, disp_median at windows 3 and 5, disparity_filter (max_diff 1, max_size 20,
      connectivity 4, window 3);
  (b) a device-to-device copy of the same input and output bytes (the rate denominator of each op);
  (c) the same partition by plain torch ops on the device: minimum-label propagation to a fixpoint, its labels compared
      with (a)'s;
  (d) xcorrvol_argmax, the matcher call the filter follows, at the same shape.
    python tools/time_disp_filter.py [--reps 30] [--out profiles/disp_filter.txt]
Device time from HIP events around each call, after warm-up launches; median / min / max over the repetitions (30; the
torch restatement: 3 after one warm-up on the matcher indices, a single run of one frame on the serpentine).  The
int64 -> f32 conversion of the indices is inside the timed calls."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from connecting_the_dots_amd import torchext as te  # noqa: E402
from tests import dispfilter_ref, workloads  # noqa: E402

FMT = "%-64s %.3f / %.3f / %.3f ms"


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


def torch_labels(d, max_diff):
    """4-connected minimum-label propagation to a fixpoint; d f32 [N,H,W] (NaN = dead) -> (labels int32, sweeps)"""
    N, H, W = d.shape
    live = torch.isfinite(d)
    big = H * W
    lab = torch.arange(H * W, device=d.device, dtype=torch.int32).view(1, H, W).expand(N, H, W).clone()
    lab[~live] = big
    lh = live[:, :, 1:] & live[:, :, :-1] & ((d[:, :, 1:] - d[:, :, :-1]).abs() <= max_diff)
    lv = live[:, 1:] & live[:, :-1] & ((d[:, 1:] - d[:, :-1]).abs() <= max_diff)
    bigt = torch.full((), big, dtype=torch.int32, device=d.device)
    sweeps = 0
    while True:
        new = lab.clone()
        new[:, :, 1:] = torch.minimum(new[:, :, 1:], torch.where(lh, lab[:, :, :-1], bigt))
        new[:, :, :-1] = torch.minimum(new[:, :, :-1], torch.where(lh, lab[:, :, 1:], bigt))
        new[:, 1:] = torch.minimum(new[:, 1:], torch.where(lv, lab[:, :-1], bigt))
        new[:, :-1] = torch.minimum(new[:, :-1], torch.where(lv, lab[:, 1:], bigt))
        sweeps += 1
        if torch.equal(new, lab):                                # (a host synchronisation per sweep)
            break
        lab = new
    lab[~live] = -1
    return lab, sweeps


def copy_ms(n_in, n_out, reps, device):
    """a device-to-device copy that reads n_in and writes n_out bytes (the larger of the two is copied, the rest read or
    written on its own)"""
    n = max(n_in, n_out)
    src = torch.empty(n, dtype=torch.uint8, device=device)
    dst = torch.empty(n, dtype=torch.uint8, device=device)
    return median_ms(lambda: dst[:n_out].copy_(src[:n_out]) if n_out >= n_in else dst[:n_in].copy_(src[:n_in]), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--torch-frames", type=int, default=1, help="frames of the serpentine batch given to the torch restatement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "disp_filter.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_disp_filter.py needs a GPU"

    N, H, W, D, BS = 16, 432, 512, 128, 9
    rs = np.random.RandomState(2)
    pat = workloads.syn_dot_pattern(H, W, seed=42)
    raw = np.stack([workloads.synth_ir(pat, rs, D)[0] for _ in range(N)])
    raw = (raw + rs.normal(0, 0.15, raw.shape)).astype(np.float32)
    x = te.lcn(torch.from_numpy(raw[:, None]).cuda(), 5, 0.05)[0]
    p = te.lcn(torch.from_numpy(pat[None, None]).cuda(), 5, 0.05)[0][0].contiguous()
    idx = te.xcorrvol_argmax(x, p, D, BS)[0]
    serp = torch.from_numpy(np.where(dispfilter_ref.serpentine(H, W), np.float32(7), np.float32(np.nan))).cuda()
    serp = serp.unsqueeze(0).expand(N, H, W).contiguous()
    pix = N * H * W

    lines = ["config 2: %d x %dx%d, D %d; median / min / max of %d launches (device time, HIP events)" % (
        N, W, H, D, args.reps)]
    matcher = median_ms(lambda: te.xcorrvol_argmax(x, p, D, BS), args.reps)
    lines.append(FMT % (("(d) xcorrvol_argmax block %d (the matcher call before the filter)" % BS,) + matcher))
    print(lines[-1], flush=True)

    for name, d, in_bytes in (("matcher idx (int64)", idx, 8), ("serpentine (f32)", serp, 4)):
        label, size = te.disp_components(d, None, 1.0, 4)
        n_comp = int((label == torch.arange(H * W, device="cuda", dtype=torch.int32).view(1, H, W)).sum())
        lines.append("-- %s: %d components over %d pixels, the largest %d pixels" % (name, n_comp, pix, int(size.max())))
        ops = [("disp_components", lambda: te.disp_components(d, None, 1.0, 4), 8),
               ("disp_speckle max_size 20", lambda: te.disp_speckle(d, None, 1.0, 20, 4), 1),
               ("disp_median window 3", lambda: te.disp_median(d, None, 3, 0), 5),
               ("disp_median window 5", lambda: te.disp_median(d, None, 5, 0), 5),
               ("disparity_filter (speckle 20 + median 3)", lambda: te.disparity_filter(d, None, 1.0, 20, 4, 3, 0), 5)]
        for what, fn, out_bytes in ops:
            t = median_ms(fn, args.reps)
            c = copy_ms(in_bytes * pix, out_bytes * pix, args.reps, "cuda")
            lines.append(FMT % (("(a) " + what,) + t))
            lines.append("    (b) copy of %d B in + %d B out per pixel %.3f ms -> op / copy = %.1f x; op / matcher = %.3f" % (
                in_bytes, out_bytes, c[0], t[0] / c[0], t[0] / matcher[0]))
            print("\n".join(lines[-2:]), flush=True)
        nf = N if d is idx else args.torch_frames
        df = d[:nf].to(torch.float32)
        treps, twarm = (args.torch_reps, 1) if d is idx else (1, 0)      # (the serpentine needs ~ H * W / 2 sweeps: once)
        ref = median_ms(lambda: torch_labels(df, 1.0), treps, twarm)
        tl, sweeps = torch_labels(df, 1.0)
        hip = median_ms(lambda: te.disp_components(df, None, 1.0, 4), args.reps)
        differ = int((tl != te.disp_components(df, None, 1.0, 4)[0]).sum())
        lines.append(FMT % (("(c) torch min-label propagation, %d frame(s), %d sweeps (%d launches)" % (
            nf, sweeps, treps),) + ref))
        lines.append("    disp_components on the same %d frame(s) %.3f ms: torch / HIP = %.1f x; labels differing: %d of %d" % (
            nf, hip[0], ref[0] / hip[0], differ, tl.numel()))
        print("\n".join(lines[-2:]), flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
