"""Time of mesheval.point_mesh_distance by brute force and through the device BVH, tree build excluded and reported
separately, on data-generator-like scenes (tests/bvh_scenes.get_mesh_like: the 1000-unit board plus four procedural
objects) with 10^5 query points: near the surface (vertices of the objects, drawn with replacement, + 1e-3 noise: the
evaluation case) and uniform in the objects' bounding box.  Every BVH answer is also checked bit for bit against the
brute-force answer.  The last column is what `bvh='auto'` decides on: brute force against build + traversal.

    python tools/time_point_mesh.py [--faces 300 1000 2000 4000 10000 30000 100000 1000000] [--points 100000] [--reps 5]
                                    [--out profiles/point_mesh.txt]

Times are device-event times of the kernel calls (torch.sqrt and the output allocation included), the minimum and the
median over --reps after one warm-up call.  Brute force at 10^6 faces takes a large fraction of a second per call: it gets
--brute-reps."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def query_points(v, n, seed):
    """(near the surface, uniform in the objects' box), f32 [n,3] each; the board's six corners come first in v"""
    import numpy as np
    rs = np.random.RandomState(seed)
    obj = v[6:]
    near = obj[rs.randint(0, len(obj), n)] + rs.normal(size=(n, 3)) * 1e-3
    box = rs.uniform(obj.min(0), obj.max(0), size=(n, 3))
    return near.astype(np.float32), box.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, nargs="+", default=[300, 1000, 2000, 4000, 10000, 30000, 100000, 1000000])
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--brute-reps", type=int, default=2)
    ap.add_argument("--out", default=None, help="append the table to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    from connecting_the_dots_amd import mesheval, renderer
    from tests import bvh_scenes

    if not torch.cuda.is_available():
        raise SystemExit("time_point_mesh.py measures on the GPU; there is none here")
    dev = torch.device("cuda", 0)

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return out, min(ts), float(np.median(ts))

    lines = ["%d query points, reps %d (brute force %d); times in ms, min / median" % (args.points, args.reps, args.brute_reps)]
    for n in args.faces:
        v, _, f = bvh_scenes.get_mesh_like(n, 0)
        vt, ft = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
        bvh, t_build, t_build_med = timed(lambda: renderer.MeshBVH(vt, ft), args.reps)
        lines.append("scene %d faces: build %.3f / %.3f ms (host clock included: the build synchronises), depth %d, %.1f MB%s"
                     % (len(f), t_build, t_build_med, bvh.depth, bvh.nbytes / 2 ** 20,
                        "" if bvh.usable else " (refused: too deep)"))
        for name, pts in zip(("near-surface", "box-uniform"), query_points(v, args.points, 1)):
            p = torch.from_numpy(pts).to(dev)
            a, tb, tb_med = timed(lambda: mesheval.point_mesh_distance(p, vt, ft, bvh=bvh, return_closest=True), args.reps)
            r, tr, tr_med = timed(lambda: mesheval.point_mesh_distance(p, vt, ft, return_closest=True), args.brute_reps)
            same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, r))
            lines.append("  %-12s brute %10.3f / %10.3f   bvh %8.3f / %8.3f   speed-up %8.1fx   bit-exact %s   "
                         "brute / (build + bvh) %7.2f" % (name, tr, tr_med, tb, tb_med, tr / tb, same, tr / (t_build + tb)))
        print("\n".join(lines[-3:]), flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
