"""Times the multi-view depth consistency check and the point fusion (csrc/depth_fusion.hip) on one track of 4 views of
640 x 480 (the noisy scene of tests/fusion_ref.py: both planes, depth noise, 10 % gross outliers, holes):
    python tools/time_depth_fusion.py [--reps 30] [--kernel-stats DIR_OR_CSV] [--out profiles/depth_fusion.txt]
      HIP-event medians of single calls of depth_consistency and depth_fuse_points (dedupe off / on), the compulsory
      bytes of each kernel computed from the shape and the counts, and -- with --kernel-stats -- each kernel's time from
      a rocprofv3 kernel trace of the run below, beside those bytes;
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_depth_fusion.py --trace-calls 20
      the traced run: 3 untimed and 20 traced calls of depth_fuse_points (dedupe on), nothing else.
Compulsory bytes = every array a kernel has to read or write once (the gathers into the source views and the rays of
the pixels they hit fall on arrays that are already counted).
The scene comes from the tests' generator (tests/fusion_ref.py), on purpose: the timed input is the one the parity tests
check, and both travel with the tree."""
import argparse
import csv
import glob
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from connecting_the_dots_amd import torchext as te  # noqa: E402
from tests import fusion_ref  # noqa: E402

SHAPE = (1, 4, 480, 640)                                       # B, V, H, W


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


def kernel_stats(path):
    """rocprofv3's kernel_stats.csv (or the newest one under a directory) -> {name: (calls, avg, min, max in us)}"""
    if os.path.isdir(path):
        path = sorted(glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)[-1]
    return {r["Name"]: (int(r["Calls"]), float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3)
            for r in csv.DictReader(open(path))}


def compulsory_bytes(shape, n_points):
    """[(kernel, bytes, what)] of one depth_fuse_points call with dedupe that emits n_points points"""
    B, V, H, W = shape
    n, plane = B * V * H * W, H * W
    blocks = B * V * ((plane + 255) // 256)
    ray_b = 12 * plane
    return [("depth_consistency_kernel", 5 * n + ray_b + 6 * n, "depth + valid, rays once; count, keep, fused"),
            ("fuse_count_kernel", 2 * n + 5 * n + ray_b + 4 * blocks, "keep, emit flags; depth + valid, rays (dedupe); counts"),
            ("fuse_scan_kernel", 8 * blocks + 8 * B, "workgroup counts in and out"),
            ("fuse_scatter_kernel", n + 4 * blocks + n_points * (4 + 12 + 20),
             "emit flags, offsets; per point fused + ray in, point + src out")]


def kernel_lines(shape, n_points, stats):
    """the per-kernel lines of the report; stats = kernel_stats(...) or None (times not measured)"""
    n = int(np.prod(shape))
    lines = ["compulsory bytes per kernel (dedupe on)%s" % (
        "" if stats else "; kernel times: NOT MEASURED (no --kernel-stats given)")]
    for name, nbytes, what in compulsory_bytes(shape, n_points):
        hit = [v for k, v in (stats or {}).items() if name in k]
        t = "calls %d avg %.1f us (min %.1f, max %.1f) = %.2f TB/s" % (hit[0] + (nbytes / hit[0][1] / 1e6,)) if hit else "-"
        lines.append("  %-26s %10d B = %5.2f B/pixel (%s): %s" % (name, nbytes, nbytes / n, what, t))
    return lines


def scene_tensors(shape):
    sc = fusion_ref.make_scene("noisy", *shape, 1)
    return [torch.from_numpy(np.ascontiguousarray(sc[k])).cuda() for k in ("depth", "ray", "K", "R", "t", "valid")]


def report(shape, reps, stats=None):
    """the text of profiles/depth_fusion.txt for one shape: event timings of the three calls, then kernel_lines()"""
    B, V, H, W = shape
    t_in = scene_tensors(shape)
    pts, src, _, count, keep, _ = te.depth_fuse_points(*t_in, return_maps=True)
    m1, m0, kept = int(src.numel()), int(te.depth_fuse_points(*t_in, dedupe=False)[1].numel()), int(keep.sum())
    lines = ["%d track(s) x %d views x %dx%d, max_px 1, max_rel 0.01, min_views 1: %d pixels, %d kept, %d points without "
             "dedupe, %d with; counts %s" % (B, V, W, H, B * V * H * W, kept, m0, m1,
                                             np.bincount(count.cpu().numpy().ravel()).tolist()),
             "median / min / max of %d single calls (device time, HIP events; the fusion includes its one read-back)" % reps]
    for what, fn in (("depth_consistency", lambda: te.depth_consistency(*t_in)),
                     ("depth_fuse_points dedupe off", lambda: te.depth_fuse_points(*t_in, dedupe=False)),
                     ("depth_fuse_points dedupe on", lambda: te.depth_fuse_points(*t_in))):
        lines.append("%-48s %.3f / %.3f / %.3f ms" % ((what,) + median_ms(fn, reps)))
        print(lines[-1], flush=True)
    return "\n".join(lines + kernel_lines(shape, m1, stats)) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_fusion.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_depth_fusion.py needs a GPU"
    if args.trace_calls:
        t_in = scene_tensors(SHAPE)
        for _ in range(3 + args.trace_calls):
            te.depth_fuse_points(*t_in)
        torch.cuda.synchronize()
        return
    text = report(SHAPE, args.reps, kernel_stats(args.kernel_stats) if args.kernel_stats else None)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
