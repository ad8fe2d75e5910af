"""Build time of the device BVH and per-frame render_mesh_proj time with and without it, on data-generator-like
scenes (tests/bvh_scenes.get_mesh_like: the 1000-unit board plus four procedural objects) at 480x640 and its
three halvings.  Every BVH frame is also checked bit for bit against the brute-force frame.

    python tools/time_render_bvh.py [--faces 50000 250000 1000000] [--reps 3] [--out profiles/render_bvh.txt]

The brute-force frame at 1 M faces takes seconds: run each size as its own step under a time limit."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, nargs="+", default=[50000, 250000, 1000000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--brute-reps", type=int, default=1)
    ap.add_argument("--out", default=None, help="append the table to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    from connecting_the_dots_amd import renderer
    from tests import bvh_scenes

    dev = torch.device("cuda", 0)

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return out, min(ts) * 1e3

    lines = []
    for n in args.faces:
        v, c, f = bvh_scenes.get_mesh_like(n, 0)
        vt, ct, ft = (torch.from_numpy(a).to(dev) for a in (v, c, f))
        bvh, t_build = timed(lambda: renderer.MeshBVH(vt, ft), args.reps)
        lines.append("scene %d faces: build %.2f ms, depth %d, %.1f MB%s" % (
            len(f), t_build, bvh.depth, bvh.nbytes / 2 ** 20, "" if bvh.usable else " (refused: too deep)"))
        sh = renderer.PyShader(0.5, 1.5, 0.0, 10)
        for s in range(4):
            H, W = 480 >> s, 640 >> s
            cam = renderer.PyCamera(*(lambda K, R, t, W_, H_: (K[0, 0], K[1, 1], K[0, 2], K[1, 2], R, t, W_, H_))(
                *bvh_scenes.camera(H, W)))
            proj = renderer.PyCamera(*(lambda K, R, t, W_, H_: (K[0, 0], K[1, 1], K[0, 2], K[1, 2], R, t, W_, H_))(
                *bvh_scenes.camera(H, W, t=(0.075, 0, 0))))
            pat = torch.from_numpy(bvh_scenes.pattern(H, W)).to(dev)
            a, tb = timed(lambda: renderer.render_mesh_proj(vt, ct, ft, cam, proj, sh, pat, 0.0, 0.35, bvh=bvh),
                          args.reps)
            r, tr = timed(lambda: renderer.render_mesh_proj(vt, ct, ft, cam, proj, sh, pat, 0.0, 0.35),
                          args.brute_reps)
            same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, r))
            lines.append("  %4dx%-4d mesh_proj  brute %9.2f ms   bvh %8.3f ms   speed-up %7.1fx   bit-exact %s" % (
                H, W, tr, tb, tr / tb, same))
        print("\n".join(lines[-5:]), flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
