"""Time of one round of meshreg.mesh_icp_system and of a 10-round meshreg.mesh_icp on the two large scenes of
profiles/point_mesh.txt (tests/bvh_scenes.get_mesh_like at 10^5 and 10^6 target faces: 70 724 and 986 500 faces) with 10^5
near-surface points (tools/time_point_mesh.query_points), through a prebuilt tree.

One round, at the pose P1 = a rotation of --degrees about the points' centroid, after a round at the identity P0:
  unhinted   mesh_icp_system(points, P1)
  hinted     mesh_icp_system(points, P1, hint = the faces of the round at P0)
  yardstick  mesheval.point_mesh_distance(transform_points(points, P1), return_closest=True): the nearest-face query that
             stood before, on the same posed points (the posing itself is outside the timed window)
The three are timed in turn inside one loop, so that a drift of the clocks touches all alike; device-event times, the
minimum and the median over --reps after a warm-up of each.  The hinted and unhinted maps are compared bit for bit.
Then mesh_icp, 10 rounds of the plane metric from the identity on the points as P1 left them, with and without the hint
loop (the tree prebuilt), and with bvh='auto' (the build inside); the poses of the first two are compared bit for bit.

    python tools/time_mesh_register.py [--faces 100000 1000000] [--points 100000] [--reps 20] [--out profiles/mesh_register.txt]
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
    from connecting_the_dots_amd import mesheval, meshreg, renderer
    from tests import bvh_scenes
    from tests import meshreg_ref as mr
    from tools.time_point_mesh import query_points

    if not torch.cuda.is_available():
        raise SystemExit("time_mesh_register.py measures on the GPU; there is none here")
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
        pts = query_points(v, args.points, 1)[0]
        c = pts.astype(np.float64).mean(0)
        Q = mr.rotation([1.0, -2.0, 0.5], args.degrees)
        p = torch.from_numpy(pts).to(dev)
        R0, t0 = torch.eye(3, device=dev), torch.zeros(3, device=dev)
        R1 = torch.from_numpy(Q.astype(np.float32)).to(dev)
        t1 = torch.from_numpy((c - Q @ c).astype(np.float32)).to(dev)
        lines.append("scene %d faces (tree depth %d, %.1f MB)" % (len(f), tree.depth, tree.nbytes / 2 ** 20))
        for metric in ("plane", "point"):
            prev = meshreg.mesh_icp_system(p, vt, ft, R0, t0, metric=metric, bvh=tree, return_maps=True)[1]
            S = meshreg.transform_points(p, R1, t1).contiguous()
            moved = float((S - p).norm(dim=1).mean())
            r = timed_in_turn({
                "unhinted": lambda: meshreg.mesh_icp_system(p, vt, ft, R1, t1, metric=metric, bvh=tree, return_maps=True),
                "hinted": lambda: meshreg.mesh_icp_system(p, vt, ft, R1, t1, metric=metric, bvh=tree, hint=prev,
                                                          return_maps=True),
                "no maps": lambda: meshreg.mesh_icp_system(p, vt, ft, R1, t1, metric=metric, bvh=tree, hint=prev),
                "yardstick": lambda: mesheval.point_mesh_distance(S, vt, ft, bvh=tree, return_closest=True)}, args.reps)
            same = all(torch.equal(x.view(torch.int64 if x.dtype == torch.float64 else torch.int32),
                                   y.view(torch.int64 if y.dtype == torch.float64 else torch.int32))
                       for x, y in zip(r["unhinted"][0], r["hinted"][0]))
            kept = float((r["hinted"][0][1] == prev).float().mean())
            lines.append("  %-5s mean move %.3g; system unhinted %7.3f / %7.3f   hinted %7.3f / %7.3f   hinted, no maps %7.3f / "
                         "%7.3f   point_mesh_distance %7.3f / %7.3f   unhinted / yardstick %.2f   hinted / unhinted %.2f   "
                         "same bits %s   faces kept %.3f" % (
                             metric, moved, r["unhinted"][1], r["unhinted"][2], r["hinted"][1], r["hinted"][2],
                             r["no maps"][1], r["no maps"][2], r["yardstick"][1], r["yardstick"][2],
                             r["unhinted"][2] / r["yardstick"][2], r["hinted"][2] / r["unhinted"][2], same, kept))
        # ten rounds, end to end, on the points as P1 left them
        S = meshreg.transform_points(p, R1, t1).contiguous()
        r = timed_in_turn({
            "hint": lambda: meshreg.mesh_icp(S, vt, ft, iters=10, bvh=tree),
            "no hint": lambda: meshreg.mesh_icp(S, vt, ft, iters=10, bvh=tree, use_hint=False),
            "auto": lambda: meshreg.mesh_icp(S, vt, ft, iters=10, bvh="auto")}, max(3, args.reps // 4))
        (Ra, ta, info), _, _ = r["hint"]
        same = torch.equal(Ra, r["no hint"][0][0]) and torch.equal(ta, r["no hint"][0][1])
        rot, tr = mr.pose_error(Ra.cpu().numpy(), ta.cpu().numpy(), Q.T, c - Q.T @ c)
        lines.append("  mesh_icp, 10 rounds, plane: hint loop %7.3f / %7.3f   without %7.3f / %7.3f   bvh='auto' (build inside) "
                     "%7.3f / %7.3f   same poses %s   rms %.3g -> %.3g   pose error %.2e degrees, %.2e" % (
                         r["hint"][1], r["hint"][2], r["no hint"][1], r["no hint"][2], r["auto"][1], r["auto"][2], same,
                         float(info["rms"][0]), float(info["rms"][-1]), rot, tr))
        print("\n".join(lines[-4:]), flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
