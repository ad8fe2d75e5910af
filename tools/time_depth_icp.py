"""Times the depth-map normals and the point-to-plane ICP (csrc/depth_icp.hip) and writes profiles/depth_icp.txt:
depth_normals, depth_icp_system (with and without residual / assoc), depth_icp_update and a 10-round depth_icp at
4 tracks x 4 views x 432 x 512 (the corner scene of tests/icp_ref.py, views 1 and 2 of every track perturbed by 1 degree /
1 cm and 2 degrees / 3 cm), beside depth_consistency at the same shape, whose gathers into the other views are comparable
traffic.  Each call's compulsory bytes (every array it has to read or write once; the gathers fall on arrays already
counted) are computed from the shape, and with them bytes per pixel, the achieved rate and its share of the 8 TB/s HBM peak.
    python tools/time_depth_icp.py [--reps 30] [--shape 4 4 432 512] [--out profiles/depth_icp.txt]
Device time from HIP events around each call, after warm-up calls; median / min / max over the repetitions.  The scene
comes from the tests' generator on purpose: the timed input is the one the parity tests check."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from connecting_the_dots_amd import torchext as te  # noqa: E402
from tests import icp_ref  # noqa: E402

SHAPE = (4, 4, 432, 512)                                       # B, V, H, W
HBM_PEAK = 8.0e12                                              # bytes / s
ITERS = 10


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


def compulsory_bytes(shape):
    """{call: (bytes, what)} from the shape alone; target=None, so only view 0 of a track is gathered from"""
    B, V, H, W = shape
    n, plane, views = B * V * H * W, H * W, B * V
    chunks = (plane + 1023) // 1024
    ray_b, partial_b = 12 * plane, 2 * 232 * views * chunks + 232 * views
    system = 5 * n + ray_b + 12 * B * plane + partial_b
    return {
        "depth_normals": (5 * n + ray_b + 12 * n, "depth + valid, rays once; normals"),
        "depth_icp_system": (system, "depth + valid, rays once, the normals of view 0; partials out and in, systems"),
        "depth_icp_system + maps": (system + 12 * n, "the same + residual and assoc"),
        "depth_icp_update": ((232 + 2 * 48 + 1) * views, "system, pose in and out, ok"),
        "depth_consistency": (5 * n + ray_b + 6 * n, "depth + valid, rays once; count, keep, fused"),
    }


def report(shape, reps, warmup=10):
    """the text of profiles/depth_icp.txt for one shape"""
    B, V, H, W = shape
    n = B * V * H * W
    sc = icp_ref.make_corner(B, V, H, W, 1)
    depth, ray, K, R0, t0, valid = [torch.from_numpy(np.ascontiguousarray(sc[k])).cuda()
                                    for k in ("depth", "ray", "K", "R0", "t0", "valid")]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s.rstrip())

    say("depth-map normals and point-to-plane ICP: %d tracks x %d views x %dx%d = %d pixels (corner scene of tests/icp_ref.py, "
        "views 1 and 2 perturbed by 1 degree / 1 cm and 2 degrees / 3 cm)" % (B, V, W, H, n))
    say("device %s; median / min / max of %d calls (device time, HIP events), after %d warm-up calls"
        % (torch.cuda.get_device_name(0), reps, warmup))
    say("compulsory bytes from the shape; rate = bytes / median; share of the %.1f TB/s HBM peak" % (HBM_PEAK / 1e12))
    say()
    normal = te.depth_normals(depth, ray, valid)
    system = te.depth_icp_system(depth, normal, ray, K, R0, t0, valid)
    calls = [("depth_normals", lambda: te.depth_normals(depth, ray, valid)),
             ("depth_icp_system", lambda: te.depth_icp_system(depth, normal, ray, K, R0, t0, valid)),
             ("depth_icp_system + maps", lambda: te.depth_icp_system(depth, normal, ray, K, R0, t0, valid, return_maps=True)),
             ("depth_icp_update", lambda: te.depth_icp_update(system, R0, t0)),
             ("depth_consistency", lambda: te.depth_consistency(depth, ray, K, R0, t0, valid, max_px=1.0, max_rel=0.002))]
    nbytes = compulsory_bytes(shape)
    fmt = "%-26s %8.4f / %8.4f / %8.4f ms  %12d B = %6.2f B/pixel  %6.3f TB/s = %5.1f %% of peak  (%s)"
    for name, fn in calls:
        t = median_ms(fn, reps, warmup)
        b, what = nbytes[name]
        rate = b / (t[0] * 1e-3)
        say(fmt % ((name,) + t + (b, b / n, rate / 1e12, 100.0 * rate / HBM_PEAK, what)))
    say()
    t = median_ms(lambda: te.depth_icp(depth, ray, K, R0, t0, valid, iters=ITERS), reps, warmup)
    b = nbytes["depth_normals"][0] + ITERS * (nbytes["depth_icp_system"][0] + nbytes["depth_icp_update"][0])
    say("depth_icp, %d rounds (normals once, then system + update per round, no host synchronisation)" % ITERS)
    say("%-26s %8.4f / %8.4f / %8.4f ms  %12d B  %6.3f TB/s = %5.1f %% of peak; %.4f ms per round" % (
        ("depth_icp",) + t + (b, b / t[0] / 1e9, 100.0 * b / (t[0] * 1e-3) / HBM_PEAK, t[0] / ITERS)))
    R, tt, info = te.depth_icp(depth, ray, K, R0, t0, valid, iters=ITERS)
    rot0, tr0 = icp_ref.pose_errors(sc["R0"], sc["t0"], sc["R"], sc["t"])
    rot1, tr1 = icp_ref.pose_errors(R.cpu().numpy(), tt.cpu().numpy(), sc["R"], sc["t"])
    say("what it did: translation error %.2e .. %.2e -> at most %.2e, rotation error %.2f .. %.2f -> at most %.2e degrees; "
        "ok %s; count per view %d .. %d of %d; rmse %.2e -> %.2e" % (
            tr0[:, 1:3].min(), tr0[:, 1:3].max(), tr1.max(), rot0[:, 1:3].min(), rot0[:, 1:3].max(), rot1.max(),
            info["ok"].cpu().numpy().tolist(), int(info["count"][-1, :, 1:].min()), int(info["count"][-1, :, 1:].max()), H * W,
            float(info["rmse"][0, :, 1:].max()), float(info["rmse"][-1, :, 1:].max())))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--shape", type=int, nargs=4, default=list(SHAPE))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_icp.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_depth_icp.py needs a GPU"
    text = report(tuple(args.shape), args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
