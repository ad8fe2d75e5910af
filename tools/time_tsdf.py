"""Times the truncated signed distance volumes (csrc/tsdf.hip) and writes profiles/tsdf.txt: tsdf_integrate,
tsdf_surface_points (the count call and the fill call of the wrapper, and the wrapper with its synchronisation) and
tsdf_raycast at 4 tracks x 4 views x 432 x 512 into 256^3 voxels per track (the corner scene of tests/icp_ref.py at its
true poses, every pixel valid), and, for what the single launch buys in volume traffic, one tsdf_integrate over the 4
views beside four calls of the same kernel over one view each.  Each call's compulsory bytes (every array it has to read
or write once; the gathers fall on arrays already counted) are computed from the shape and from what the scene touches,
and with them the achieved rate and its share of the 8 TB/s HBM peak.
    python tools/time_tsdf.py [--reps 30] [--shape 4 4 432 512] [--grid 256] [--out profiles/tsdf.txt]
Device time from HIP events around each call, after warm-up calls; median / min / max over the repetitions.  The scene
comes from the tests' generator on purpose: the timed input is the one the parity tests check."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from connecting_the_dots_amd import _lib  # noqa: E402
from connecting_the_dots_amd import torchext as te  # noqa: E402
from tests import icp_ref  # noqa: E402

SHAPE = (4, 4, 432, 512)                                       # B, V, H, W
GRID = 256                                                     # voxels along each axis
EXTENT, CENTRE = 2.4, (0.0, 0.0, 2.3)                          # the cube's edge and centre: the corner is 2.1 .. 2.7 away
HBM_PEAK = 8.0e12                                              # bytes / s
CAST = dict(d_min=1.9, n_steps=96)                             # the step is 1.5 voxels: 1.9 .. 3.25 at 256 voxels, past every wall


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


def report(shape, n, reps, warmup=10):
    """the text of profiles/tsdf.txt for one shape and grid"""
    B, V, H, W = shape
    pixels, voxels = B * V * H * W, B * n ** 3
    sc = icp_ref.make_corner(B, V, H, W, 1)
    depth, ray, K, R, t = [torch.from_numpy(np.ascontiguousarray(sc[k])).cuda() for k in ("depth", "ray", "K", "R", "t")]
    voxel = EXTENT / n
    origin = torch.tensor([[c - 0.5 * voxel * (n - 1) for c in CENTRE]] * B, dtype=torch.float32, device="cuda")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s.rstrip())

    say("truncated signed distance volumes: %d tracks x %d views x %dx%d = %d pixels into %d^3 = %d voxels per track of %.5f "
        "(corner scene of tests/icp_ref.py, true poses, every pixel valid, trunc = 4 voxels)" % (B, V, W, H, pixels, n, n ** 3,
                                                                                                 voxel))
    say("device %s; median / min / max of %d calls (device time, HIP events), after %d warm-up calls"
        % (torch.cuda.get_device_name(0), reps, warmup))
    say("compulsory bytes from the shape and the scene; rate = bytes / median; share of the %.1f TB/s HBM peak" % (HBM_PEAK / 1e12))
    say()
    fmt = "%-34s %8.4f / %8.4f / %8.4f ms  %12d B  %6.3f TB/s = %5.1f %% of peak  (%s)"

    def line(name, tm, nbytes, what):
        rate = nbytes / (tm[0] * 1e-3)
        say(fmt % ((name,) + tm + (nbytes, rate / 1e12, 100.0 * rate / HBM_PEAK, what)))

    # the volume all four views made, and what it touched
    T, w = te.tsdf_volume(B, n, n, n)
    te.tsdf_integrate(T, w, origin, voxel, depth, ray, K, R, t)
    touched = int((w > 0).sum())
    image_b = 4 * pixels + 12 * H * W                              # depth, and the rays once (valid is NULL here)

    # integrate: every call starts from the fresh volume again (the copies are outside the timed region's cost only in
    # that they are two device copies of the volume; they are timed alone and subtracted)
    T0, w0 = te.tsdf_volume(B, n, n, n)
    Tw, ww = torch.empty_like(T0), torch.empty_like(w0)

    def reset():
        Tw.copy_(T0)
        ww.copy_(w0)

    def one_call():
        reset()
        te.tsdf_integrate(Tw, ww, origin, voxel, depth, ray, K, R, t)

    views = [(depth[:, v:v + 1].contiguous(), R[:, v:v + 1].contiguous(), t[:, v:v + 1].contiguous()) for v in range(V)]

    def per_view_calls():
        reset()
        for dv, Rv, tv in views:
            te.tsdf_integrate(Tw, ww, origin, voxel, dv, ray, K, Rv, tv)

    t_reset = median_ms(reset, reps, warmup)
    t_one = median_ms(one_call, reps, warmup)
    t_per = median_ms(per_view_calls, reps, warmup)
    assert torch.equal(Tw, T) and torch.equal(ww, w)               # four calls over one view each: the same bits
    one = tuple(x - t_reset[0] for x in t_one)
    per = tuple(x - t_reset[0] for x in t_per)
    b_one = 4 * voxels + 8 * touched + image_b                     # weight read; tsdf and weight written where touched
    seen = [int(x) for x in _touched_per_view(T0, w0, Tw, ww, origin, voxel, views, ray, K)]
    b_per = V * 4 * voxels + sum(8 * s for s in seen) + sum(4 * s for s in _already(seen, touched)) + image_b
    say("resetting the volume (two device copies, subtracted below)      %8.4f ms" % t_reset[0])
    line("tsdf_integrate, %d views, 1 call" % V, one, b_one, "weight read, %d voxels touched: tsdf + weight written; depth, rays once" % touched)
    line("tsdf_integrate, %d calls of 1 view" % V, per, b_per,
         "weight read %d times; per call the voxels it touches written, and read where already weighted" % V)
    say("the single launch: %.2f x the time and %.2f x the compulsory bytes of the per-view calls" % (one[0] / per[0], b_one / b_per))
    say()

    # surface points
    L = _lib.lib()
    ws = torch.empty(L.ctd_tsdf_surface_workspace_bytes(B, n, n, n), dtype=torch.uint8, device="cuda")
    n_per_track = torch.zeros(B, dtype=torch.int64, device="cuda")
    points, src, counts, normals = te.tsdf_surface_points(T, w, origin, voxel, return_normals=True)
    m = points.shape[0]
    stream = torch.cuda.current_stream().cuda_stream

    def c_call(p, nr, s, cap):
        st = L.ctd_tsdf_surface_points_f32(T.data_ptr(), w.data_ptr(), origin.data_ptr(), voxel, 1.0, p, nr, s,
                                           n_per_track.data_ptr(), cap, B, n, n, n, ws.data_ptr(), ws.numel(), 0, stream)
        _lib.check(st, "ctd_tsdf_surface_points_f32")

    usable = int(((w >= 1) & (T.abs() < 1)).sum())
    chunks = B * ((n ** 3 + 255) // 256)
    b_count = 4 * voxels + 4 * touched + voxels + 2 * 4 * chunks   # weight; tsdf behind the weight; flags; counts out and in
    b_fill = b_count + voxels + 4 * chunks + m * (16 + 12 + 8)     # the flags and offsets again; per point 2 tsdf + origin, point, src
    line("surface points: count call", median_ms(lambda: c_call(None, None, None, 0), reps, warmup), b_count,
         "weight, tsdf of %d weighted voxels (%d usable), flags written, counts scanned" % (touched, usable))
    line("surface points: fill call", median_ms(lambda: c_call(points.data_ptr(), None, src.data_ptr(), m), reps, warmup), b_fill,
         "the count pass again, flags read, %d points and src written" % m)
    line("surface points: fill + normals", median_ms(lambda: c_call(points.data_ptr(), normals.data_ptr(), src.data_ptr(), m), reps,
                                                    warmup), b_fill + m * (48 + 12),
         "the same + six neighbours read and a normal written per point")
    line("tsdf_surface_points (wrapper)", median_ms(lambda: te.tsdf_surface_points(T, w, origin, voxel, return_normals=True), reps,
                                                   warmup), b_count + b_fill + m * (48 + 12),
         "count, one synchronisation, allocation, fill + normals")
    say("%d points, %d with a normal; per track %s" % (m, int(torch.isfinite(normals).all(1).sum()), counts.cpu().numpy().tolist()))
    say()

    # ray cast, at the integrated poses
    step = 1.5 * voxel
    cast = te.tsdf_raycast(T, w, origin, voxel, ray, R, t, H, W, CAST["d_min"], step, CAST["n_steps"])
    hit = torch.isfinite(cast)
    b_cast = 4 * pixels + 12 * H * W + 8 * touched                 # depth out, rays once, the weighted voxels once
    line("tsdf_raycast, %d steps of 1.5 voxels" % CAST["n_steps"],
         median_ms(lambda: te.tsdf_raycast(T, w, origin, voxel, ray, R, t, H, W, CAST["d_min"], step, CAST["n_steps"]), reps, warmup),
         b_cast, "depth written, rays once, tsdf + weight of the weighted voxels once: a floor, the march reads them many times")
    err = (cast - depth).abs()[hit]
    say("what it did: %.2f %% of the pixels hit; median |depth - truth| %.3e = %.4f voxel, largest %.3e" % (
        100.0 * float(hit.float().mean()), float(err.median()), float(err.median()) / voxel, float(err.max())))
    return "\n".join(lines) + "\n"


def _touched_per_view(T0, w0, Tw, ww, origin, voxel, views, ray, K):
    """the number of voxels each one-view call touches (each from the fresh volume)"""
    out = []
    for dv, Rv, tv in views:
        Tw.copy_(T0)
        ww.copy_(w0)
        te.tsdf_integrate(Tw, ww, origin, voxel, dv, ray, K, Rv, tv)
        out.append((ww > 0).sum().item())
    return out


def _already(seen, union):
    """a lower bound of the voxels each call finds already weighted: the calls after the first re-read tsdf where an
    earlier call was; with touch counts s_v and a union u, at least sum(s_v) - u re-reads in all"""
    return [max(sum(seen) - union, 0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--shape", type=int, nargs=4, default=list(SHAPE))
    ap.add_argument("--grid", type=int, default=GRID)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_tsdf.py needs a GPU"
    text = report(tuple(args.shape), args.grid, args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
