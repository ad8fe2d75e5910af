"""Time of one round of meshrobust.robust_icp_system and of a 10-round meshrobust.robust_mesh_icp next to the plain
meshreg.mesh_icp_system and meshreg.mesh_icp in the same process, on the two large scenes of tools/time_mesh_register.py
(tests/bvh_scenes.get_mesh_like at 10^5 and 10^6 target faces: 70 724 and 986 500 faces) with 10^5 near-surface points
(tools/time_point_mesh.query_points), through a prebuilt tree.

One round, at the pose P1 = a rotation of --degrees about the points' centroid, after a round at the identity P0, hinted
(with the faces of the round at P0) and unhinted, every map asked for:
  plain      mesh_icp_system(points, P1)
  robust     robust_icp_system(points, P1, kernel='tukey', scale = robust_scale of the round at P0, rim = the mesh's face_rim,
             normals = the unit normals of the faces the points were nearest to at P0, min_cos 0.5): every gate on
  weights    robust_icp_system(points, P1, kernel='tukey', scale) alone: no rim, no normals
The six are timed in turn inside one loop, so that a drift of the clocks touches all alike; device-event times, the
minimum and the median over --reps after a warm-up of each.  face_rim (once per mesh, with its adjacency prebuilt) is
timed on its own.  Then 10 rounds of the plane metric from the identity on the points as P1 left them: mesh_icp,
robust_mesh_icp with scale='mad' and Tukey weights, and the same with rim and normals, each with the hint loop.

    python tools/time_mesh_robust.py [--faces 100000 1000000] [--points 100000] [--reps 20] [--out profiles/mesh_robust.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--degrees", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="append the table to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    from connecting_the_dots_amd import meshreg, meshrobust, meshsmooth, renderer
    from tests import bvh_scenes
    from tests import meshreg_ref as mr
    from tools.time_point_mesh import query_points

    if not torch.cuda.is_available():
        raise SystemExit("time_mesh_robust.py measures on the GPU; there is none here")
    dev = torch.device("cuda", 0)

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return out, a.elapsed_time(b)

    def timed_in_turn(fns, reps):
        """{name: fn} -> {name: (last result, min ms, median ms)}, one of each per pass"""
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        ts, out = {k: [] for k in fns}, {}
        for _ in range(reps):
            for k, fn in fns.items():
                out[k], ms = event_ms(fn)
                ts[k].append(ms)
        return {k: (out[k], min(v), float(np.median(v))) for k, v in ts.items()}

    lines = ["%d near-surface points, a move of %g degrees, reps %d; times in ms, min / median" % (args.points, args.degrees,
                                                                                                 args.reps)]
    for n in args.faces:
        v, _, f = bvh_scenes.get_mesh_like(n, 0)
        vt, ft = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
        tree = renderer.MeshBVH(vt, ft)
        adj = meshsmooth.MeshAdjacency(ft, vt.shape[0])
        rim = meshrobust.face_rim(ft, vt.shape[0], adjacency=adj)
        r = timed_in_turn({"rim": lambda: meshrobust.face_rim(ft, vt.shape[0], adjacency=adj)}, args.reps)
        pts = query_points(v, args.points, 1)[0]
        c = pts.astype(np.float64).mean(0)
        Q = mr.rotation([1.0, -2.0, 0.5], args.degrees)
        p = torch.from_numpy(pts).to(dev)
        R0, t0 = torch.eye(3, device=dev), torch.zeros(3, device=dev)
        R1 = torch.from_numpy(Q.astype(np.float32)).to(dev)
        t1 = torch.from_numpy((c - Q @ c).astype(np.float32)).to(dev)
        lines.append("scene %d faces (tree depth %d), %d boundary edges; face_rim %7.3f / %7.3f, %.1f %% of the faces touch the "
                     "rim" % (len(f), tree.depth, adj.n_boundary_edges, r["rim"][1], r["rim"][2],
                              100.0 * float((rim != 0).float().mean())))
        for metric in ("plane", "point"):
            _, prev, res0, _, _, _ = meshrobust.robust_icp_system(p, vt, ft, R0, t0, metric=metric, kernel="none", bvh=tree,
                                                                  return_maps=True)
            scale = meshrobust.robust_scale(res0, "tukey").reshape(1)
            normals = meshrobust._face_unit_normals(vt, ft, prev.clamp(min=0).long())
            every = dict(metric=metric, kernel="tukey", scale=scale, rim=rim, normals=normals, min_cos=0.5, bvh=tree,
                         return_maps=True)
            weights = dict(metric=metric, kernel="tukey", scale=scale, bvh=tree, return_maps=True)
            plain = dict(metric=metric, bvh=tree, return_maps=True)
            r = timed_in_turn({
                "plain": lambda: meshreg.mesh_icp_system(p, vt, ft, R1, t1, **plain),
                "plain hinted": lambda: meshreg.mesh_icp_system(p, vt, ft, R1, t1, hint=prev, **plain),
                "robust": lambda: meshrobust.robust_icp_system(p, vt, ft, R1, t1, **every),
                "robust hinted": lambda: meshrobust.robust_icp_system(p, vt, ft, R1, t1, hint=prev, **every),
                "weights": lambda: meshrobust.robust_icp_system(p, vt, ft, R1, t1, **weights),
                "weights hinted": lambda: meshrobust.robust_icp_system(p, vt, ft, R1, t1, hint=prev, **weights)}, args.reps)
            used = [float(r[k][0][0][28]) for k in ("robust", "weights", "plain")]
            as_bits = lambda x: x.view({torch.float32: torch.int32, torch.float64: torch.int64}.get(x.dtype, x.dtype))
            same = all(torch.equal(as_bits(x), as_bits(y)) for x, y in zip(r["robust"][0], r["robust hinted"][0]))
            lines.append("  %-5s unhinted: plain %7.3f / %7.3f   every gate %7.3f / %7.3f (%.3f of plain)   weights alone %7.3f / "
                         "%7.3f (%.3f)" % (metric, r["plain"][1], r["plain"][2], r["robust"][1], r["robust"][2],
                                           r["robust"][2] / r["plain"][2], r["weights"][1], r["weights"][2],
                                           r["weights"][2] / r["plain"][2]))
            lines.append("        hinted:   plain %7.3f / %7.3f   every gate %7.3f / %7.3f (%.3f of plain)   weights alone %7.3f / "
                         "%7.3f (%.3f)   points used %d / %d / %d   hinted bits equal %s" % (
                             r["plain hinted"][1], r["plain hinted"][2], r["robust hinted"][1], r["robust hinted"][2],
                             r["robust hinted"][2] / r["plain hinted"][2], r["weights hinted"][1], r["weights hinted"][2],
                             r["weights hinted"][2] / r["plain hinted"][2], used[0], used[1], used[2], same))
        # ten rounds, end to end, on the points as P1 left them
        S = meshreg.transform_points(p, R1, t1).contiguous()
        normals = meshrobust._face_unit_normals(vt, ft, prev.clamp(min=0).long())
        normals = meshreg.transform_points(normals, R1, torch.zeros(3, device=dev)).contiguous()
        r = timed_in_turn({
            "plain": lambda: meshreg.mesh_icp(S, vt, ft, iters=10, bvh=tree),
            "tukey": lambda: meshrobust.robust_mesh_icp(S, vt, ft, iters=10, kernel="tukey", bvh=tree),
            "every": lambda: meshrobust.robust_mesh_icp(S, vt, ft, iters=10, kernel="tukey", rim=rim, normals=normals, min_cos=0.5,
                                                        bvh=tree)}, max(3, args.reps // 4))
        errs = {k: mr.pose_error(r[k][0][0].cpu().numpy(), r[k][0][1].cpu().numpy(), Q.T, c - Q.T @ c) for k in r}
        lines.append("  10 rounds, plane, hint loop: mesh_icp %7.3f / %7.3f   robust_mesh_icp tukey %7.3f / %7.3f (%.3f)   tukey, rim "
                     "and normals %7.3f / %7.3f (%.3f)   pose error in degrees %.2e / %.2e / %.2e   last used %d / %d" % (
                         r["plain"][1], r["plain"][2], r["tukey"][1], r["tukey"][2], r["tukey"][2] / r["plain"][2], r["every"][1],
                         r["every"][2], r["every"][2] / r["plain"][2], errs["plain"][0], errs["tukey"][0], errs["every"][0],
                         int(r["tukey"][0][2]["used"][-1]), int(r["every"][0][2]["used"][-1])))
        print("\n".join(lines[-6:]), flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
