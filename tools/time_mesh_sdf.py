"""Time of meshsdf.point_mesh_signed_distance against mesheval.point_mesh_distance in the same run, of the cutoff, and of
meshsdf.mesh_to_tsdf, on the scenes and points of tools/time_point_mesh.py (tests/bvh_scenes.get_mesh_like: the 1000-unit
board plus four procedural objects; 10^5 query points near the surface and uniform in the objects' bounding box), all
through the device BVH.  The adjacency and the tree are built once per scene and their builds are listed separately.

    python tools/time_mesh_sdf.py [--faces 100000 1000000] [--points 100000] [--grids 128 256] [--reps 5]
                                  [--out profiles/mesh_sdf.txt]

Times are device-event times around the Python calls (torch.sqrt, the sign product and the output allocation included),
the minimum and the median over --reps after one warm-up call.  The split of the signed call into its two launches comes
from torch.profiler's kernel records where they are available (the device time of the traversal kernel and of
mesh_sdf_sign_kernel, summed over the profiled call); the line says so when they are not, and the difference between the
signed and the unsigned call then stands for the sign pass.  Every signed answer is checked bit for bit against the
unsigned one (distance, face, closest), and the cut-off answer against the uncut one restricted to max_dist."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--grids", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the table to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    from connecting_the_dots_amd import mesheval, meshsdf, meshsmooth, renderer
    from tests import bvh_scenes
    from tools.time_point_mesh import query_points

    if not torch.cuda.is_available():
        raise SystemExit("time_mesh_sdf.py measures on the GPU; there is none here")
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

    def kernel_split(fn):
        """(nearest ms, sign ms) of one call from the profiler's kernel records, or None"""
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            near = sign = 0.0
            for ev in prof.events():
                t = getattr(ev, "device_time", None)
                t = getattr(ev, "cuda_time", 0.0) if t is None else t
                if "mesh_sdf_sign_kernel" in ev.name:
                    sign += t
                elif "point_mesh_bvh_kernel" in ev.name or "point_mesh_brute_kernel" in ev.name:
                    near += t
            return (near / 1e3, sign / 1e3) if near > 0 and sign > 0 else None
        except Exception:                                      # noqa: BLE001  a measurement aid: its absence is reported
            return None

    def bits(x, y):
        return torch.equal(x.view(torch.int32), y.view(torch.int32))

    lines = ["%d query points, reps %d; times in ms, min / median" % (args.points, args.reps)]
    for n in args.faces:
        v, _, f = bvh_scenes.get_mesh_like(n, 0)
        vt, ft = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
        bvh, t_build, t_build_med = timed(lambda: renderer.MeshBVH(vt, ft), args.reps)
        adj, t_adj, t_adj_med = timed(lambda: meshsmooth.MeshAdjacency(ft, len(v)), args.reps)
        obj = v[6:].astype(np.float64)
        a, b, c = (obj[f[2:, k] - 6] for k in range(3))
        edge = float(np.mean([np.linalg.norm(b - a, axis=1).mean(), np.linalg.norm(c - b, axis=1).mean(),
                              np.linalg.norm(a - c, axis=1).mean()]))
        lines.append("scene %d faces: tree build %.3f / %.3f ms, adjacency build %.3f / %.3f ms (host clock included: both "
                     "synchronise), depth %d, max incident %d, mean edge %.5f"
                     % (len(f), t_build, t_build_med, t_adj, t_adj_med, bvh.depth, adj.max_incident, edge))
        for name, pts in zip(("near-surface", "box-uniform"), query_points(v, args.points, 1)):
            p = torch.from_numpy(pts).to(dev)
            u, tu, tu_med = timed(lambda: mesheval.point_mesh_distance(p, vt, ft, bvh=bvh, return_closest=True), args.reps)
            s, ts, ts_med = timed(lambda: meshsdf.point_mesh_signed_distance(p, vt, ft, bvh=bvh, adjacency=adj, return_closest=True,
                                                                             return_feature=True), args.reps)
            same = bits(s[0].abs(), u[0]) and torch.equal(s[1], u[1]) and bits(s[2], u[2])
            split = kernel_split(lambda: meshsdf.point_mesh_signed_distance(p, vt, ft, bvh=bvh, adjacency=adj, return_closest=True,
                                                                            return_feature=True))
            how = ("nearest kernel %.3f, sign kernel %.3f (profiler)" % split if split else
                   "no kernel records: sign pass by difference %.3f" % (ts - tu))
            feat = torch.bincount(s[3].long().clamp(min=0), minlength=7).tolist()
            lines.append("  %-12s unsigned %8.3f / %8.3f   signed %8.3f / %8.3f   ratio %.3f   %s   bit-exact %s   features "
                         "v/e/f %d/%d/%d   negative %.3f" % (name, tu, tu_med, ts, ts_med, ts / tu, how, same, sum(feat[:3]),
                                                            sum(feat[3:6]), feat[6], float((s[4] < 0).float().mean())))
            if name == "box-uniform":
                md = 4 * edge
                c4, tc, tc_med = timed(lambda: meshsdf.point_mesh_signed_distance(p, vt, ft, bvh=bvh, adjacency=adj, max_dist=md),
                                       args.reps)
                hit = c4[1] >= 0
                lim = torch.sqrt(torch.tensor(meshsdf._max_d2(md, "t"), device=dev))      # (sqrt is monotone, not strictly)
                ok = bool((s[0].abs()[hit] <= lim).all()) and bool((s[0].abs()[~hit] >= lim).all()) and \
                    bits(c4[0][hit], s[0][hit]) and torch.equal(c4[1][hit], s[1][hit])
                lines.append("  %-12s max_dist 4 mean edges = %.5f: %8.3f / %8.3f against %8.3f without   speed-up %.2fx   "
                             "%.1f %% of the points qualify   restriction of the uncut answer %s"
                             % ("", md, tc, tc_med, ts, ts / tc, 100 * float(hit.float().mean()), ok))
        lo, hi = v[6:].min(0).astype(np.float64), v[6:].max(0).astype(np.float64)
        for g in args.grids:
            voxel = float((hi - lo).max() / (g - 1))
            origin = torch.tensor((lo + hi) / 2 - voxel * (g - 1) / 2, dtype=torch.float32, device=dev)
            (tsdf, weight), tg, tg_med = timed(lambda: meshsdf.mesh_to_tsdf(vt, ft, origin, voxel, (g, g, g), 4 * voxel, bvh=bvh,
                                                                           adjacency=adj), max(2, args.reps // 2))
            lines.append("  mesh_to_tsdf %d^3, voxel %.5f, trunc 4 voxels: %9.3f / %9.3f ms   %.2f %% of the voxels within "
                         "trunc, %.2f %% negative" % (g, voxel, tg, tg_med, 100 * float(weight.mean()),
                                                     100 * float((tsdf < 0).float().mean())))
        print("\n".join(lines[-(4 + len(args.grids)):]), flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
