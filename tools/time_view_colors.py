"""Times the view colours (csrc/mesh_color.hip: ctd_mesh_view_colors_f32 through meshcolor.view_colors) by brute force
and through the device BVH, the tree build reported separately, and writes profiles/view_colors.txt: 10^5 near-surface
points (vertices of the objects, drawn with replacement, + 1e-3 noise, as in tools/time_point_mesh.py) coloured from
V = 4 views of 480 x 640 against data-generator-like scenes (tests/bvh_scenes.get_mesh_like: the 1000-unit board plus
four procedural objects), among them the 71 K-face and the 987 K-face scene of profiles/point_mesh.txt.  The last column
is what `bvh='auto'` decides on: brute force against build + traversal.

    python tools/time_view_colors.py [--faces 300 1000 2000 4000 10000 30000 100000 1000000] [--points 100000] [--reps 5]
                                     [--brute-reps 2] [--out profiles/view_colors.txt]

Times are device-event times of the calls (output allocation included), the minimum and the median over --reps after one
warm-up call.  Every BVH answer is also checked bit for bit against the brute-force answer, on all four outputs.  The
cameras sit within 0.3 of the origin and look along +z, where get_mesh_like puts its objects; margin 0.01, mode 'mean',
with the points' normals (towards the first camera, noisy) and without."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, V, C = 480, 640, 4, 3
MARGIN = 0.01


def views(seed):
    """K f32 [3,3], R f32 [V,3,3], t f32 [V,3]: f = 0.9 W, small rotations about +z-looking cameras near the origin"""
    import numpy as np
    rs = np.random.RandomState(seed)
    K = np.array([[0.9 * W, 0, W / 2 - 0.5], [0, 0.9 * W, H / 2 - 0.5], [0, 0, 1]], np.float32)
    R, t = [], []
    for v in range(V):
        w = rs.normal(size=3) * 0.05
        th = np.linalg.norm(w)
        k = w / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        Rv = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
        R.append(Rv)
        t.append(-Rv @ rs.uniform(-0.3, 0.3, size=3))
    return K, np.stack(R).astype(np.float32), np.stack(t).astype(np.float32)


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
    from connecting_the_dots_amd import meshcolor, renderer
    from tests import bvh_scenes
    from tools.time_point_mesh import query_points

    if not torch.cuda.is_available():
        raise SystemExit("time_view_colors.py measures on the GPU; there is none here")
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

    K, R, t = (torch.from_numpy(a).to(dev) for a in views(0))
    images = torch.rand((V, C, H, W), dtype=torch.float32, device=dev, generator=torch.Generator(dev).manual_seed(0))
    lines = ["# tools/time_view_colors.py, %s: meshcolor.view_colors, brute force against the BVH traversal"
             % torch.cuda.get_device_name(0),
             "%d near-surface points, %d views of %dx%d, %d channels, margin %g, mode 'mean'; reps %d (brute force %d); "
             "times in ms, min / median" % (args.points, V, H, W, C, MARGIN, args.reps, args.brute_reps)]
    print("\n".join(lines), flush=True)
    for n in args.faces:
        v, _, f = bvh_scenes.get_mesh_like(n, 0)
        vt, ft = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
        bvh, t_build, t_build_med = timed(lambda: renderer.MeshBVH(vt, ft), args.reps)
        lines.append("scene %d faces: build %.3f / %.3f ms (host clock included: the build synchronises), depth %d, %.1f MB%s"
                     % (len(f), t_build, t_build_med, bvh.depth, bvh.nbytes / 2 ** 20,
                        "" if bvh.usable else " (refused: too deep)"))
        near, _ = query_points(v, args.points, 1)
        p = torch.from_numpy(near).to(dev)
        nrm = -p + 0.5 * torch.randn(p.shape, dtype=torch.float32, device=dev, generator=torch.Generator(dev).manual_seed(1))
        for name, normals in (("no normals", None), ("normals", nrm.contiguous())):
            def call(tree, normals=normals):
                return meshcolor.view_colors(p, images, K, R, t, MARGIN, vt, ft, normals=normals, bvh=tree, return_flags=True)

            a, tb, tb_med = timed(lambda: call(bvh), args.reps)
            r, tr, tr_med = timed(lambda: call(None), args.brute_reps)
            same = all(torch.equal(getattr(a, k).view(torch.uint8), getattr(r, k).view(torch.uint8)) or
                       (k == "color" and torch.equal(torch.nan_to_num(a.color, nan=-1.0), torch.nan_to_num(r.color, nan=-1.0)))
                       for k in ("color", "weight", "n_views", "flags"))
            used = float((a.flags == meshcolor.USED).float().mean())
            occluded = float((a.flags == (meshcolor.IN_IMAGE | meshcolor.FACING)).float().mean())
            lines.append("  %-10s brute %10.3f / %10.3f   bvh %8.3f / %8.3f   speed-up %8.1fx   bit-exact %s   "
                         "brute / (build + bvh) %7.2f   pairs used %4.1f %%, occluded %4.1f %%"
                         % (name, tr, tr_med, tb, tb_med, tr / tb, same, tr / (t_build + tb), 100 * used, 100 * occluded))
        print("\n".join(lines[-3:]), flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
