"""Time of meshglobal's parts and of the whole global_mesh_icp call, next to the route a caller had without it: the same
poses pushed through meshreg.mesh_icp_system 64 at a time.

The scenes are those of tools/time_mesh_register.py (tests/bvh_scenes.get_mesh_like at 10^5 and 10^6 target faces) WITHOUT
the board's two triangles, which are 1000 units wide where the four objects measure about 1: the volume is laid around the
objects.  10^5 near-surface points (tools/time_point_mesh.query_points), moved by --degrees about their centroid and by
--shift.  Per scene, for volumes of 64^3 and 128^3 (default_box, pad 6, trunc 6 voxels) and 2048 and 8192 scoring points,
--rotations x 27 poses:
  levels     distance_levels through a prebuilt tree
  score      pose_scores on the points in the caller's order (order=None) and on the same points already sorted along the
             Morton curve (order=None again: the kernel alone), and morton_order with the gather on its own
  refine     mesh_icp of all the points from the 8 best starts, 40 point-metric rounds, the hint loop
  whole      global_mesh_icp with these levels handed in (scoring, starts, refinement, final ranking), and the pose error
             it ends with
  yardstick  one unhinted mesh_icp_system call of 64 of the poses on the scoring points, times rotations * 27 / 64
Device-event times, the minimum and the median over --reps after a warm-up of each.

    python tools/time_mesh_global.py [--faces 100000 1000000] [--points 100000] [--reps 10] [--out profiles/mesh_global.txt]
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
    ap.add_argument("--rotations", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--degrees", type=float, default=140.0)
    ap.add_argument("--shift", type=float, default=0.5)
    ap.add_argument("--out", default=None, help="append the table to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    from connecting_the_dots_amd import meshglobal as mgl
    from connecting_the_dots_amd import meshreg, renderer
    from tests import bvh_scenes
    from tests import meshreg_ref as mr
    from tools.time_point_mesh import query_points

    if not torch.cuda.is_available():
        raise SystemExit("time_mesh_global.py measures on the GPU; there is none here")
    dev = torch.device("cuda", 0)

    def timed(fn, reps):
        """-> (last result, min ms, median ms)"""
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

    lines = ["%d near-surface points moved by %g degrees and %g; %d rotations x 27 offsets; reps %d; times in ms, min / median" % (
        args.points, args.degrees, args.shift, args.rotations, args.reps)]
    shown = 0
    for n in args.faces:
        v, _, f = bvh_scenes.get_mesh_like(n, 0)
        f = np.ascontiguousarray(f[2:])                                   # without the board
        vt, ft = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
        tree = renderer.MeshBVH(vt, ft)
        pts = query_points(v, args.points, 1)[0].astype(np.float64)
        Q = mr.rotation([1.0, -2.0, 0.5], args.degrees)
        c = pts.mean(0)
        d = np.array([0.6, 0.0, 0.8]) * args.shift
        moved = (pts - c) @ Q.T + c + d
        R_true, t_true = Q.T, c - Q.T @ (c + d)
        p = torch.from_numpy(np.ascontiguousarray(moved.astype(np.float32))).to(dev)
        Rg = mgl.rotation_grid(args.rotations, dev)
        c_points, c_mesh = mgl._centroids(p, vt, ft, "time_mesh_global")
        base = (c_mesh[None, :] - Rg.double() @ c_points).to(torch.float32).contiguous()
        gap = float(torch.linalg.norm(torch.from_numpy(c).to(dev) - c_mesh))
        lines.append("scene %d faces (tree depth %d); the points' centroid lies %.2f from the area-weighted centroid of the mesh "
                     "(the points are drawn per vertex, not per area)" % (len(f), tree.depth, gap))
        coarse = None
        for res in (64, 128):
            origin, voxel, dims = mgl.default_box(vt[6:], resolution=res, pad=6)
            levels, lo, md = timed(lambda: mgl.distance_levels(vt, ft, origin, voxel, dims, 6 * voxel, bvh=tree), max(2, args.reps // 3))
            offsets = mgl.offset_grid(3, 2 * voxel, dev)
            coarse = coarse or (levels, origin, voxel)
            lines.append("  volume %d x %d x %d, voxel %.4f: distance_levels %8.3f / %8.3f, %.1f %% of the voxels within trunc" % (
                dims + (voxel, lo, md, 100.0 * float((levels != 255).float().mean()))))
            for n_score in (2048, 8192):
                sub = p[::-(-p.shape[0] // n_score)].contiguous()
                perm, s_lo, s_md = timed(lambda: sub[mgl.morton_order(sub)].contiguous(), args.reps)
                plain = timed(lambda: mgl.pose_scores(sub, Rg, base, offsets, levels, origin, voxel, order=None), args.reps)
                morton = timed(lambda: mgl.pose_scores(perm, Rg, base, offsets, levels, origin, voxel, order=None), args.reps)
                same = torch.equal(plain[0], morton[0])
                R0, t0, s0, m0 = mgl.best_starts(plain[0], Rg, base, offsets, 8)
                yard = timed(lambda: meshreg.mesh_icp_system(sub, vt, ft, Rg[:64].contiguous(), base[:64].contiguous(),
                                                             metric="point", bvh=tree), max(2, args.reps // 3))
                batches = args.rotations * 27 / 64.0
                poses = args.rotations * 27 * sub.shape[0]
                lines.append("    %5d scoring points: pose_scores caller's order %8.3f / %8.3f   Morton order %8.3f / %8.3f (%.2f of it; "
                             "%.1f G pose-points/s)   the sort %6.3f / %6.3f   same bits %s   mesh_icp_system, 64 poses unhinted %8.3f / "
                             "%8.3f, x %.0f batches = %.0f ms: %.0f times the scoring" % (
                                 sub.shape[0], plain[1], plain[2], morton[1], morton[2], morton[2] / plain[2], poses / morton[2] * 1e-6,
                                 s_lo, s_md, same, yard[1], yard[2], batches, yard[2] * batches,
                                 yard[2] * batches / (morton[2] + s_md)))
                refine = timed(lambda: meshreg.mesh_icp(p, vt, ft, R0, t0, iters=40, metric="point", bvh=tree), max(2, args.reps // 3))
                whole = timed(lambda: mgl.global_mesh_icp(p, vt, ft, n_rotations=args.rotations, n_score=n_score,
                                                          levels=levels, origin=origin, voxel=voxel, bvh=tree), max(2, args.reps // 3))
                R, t, info = whole[0]
                rot, tr = mr.pose_error(R.cpu().numpy(), t.cpu().numpy(), R_true, t_true)
                starts = [mr.pose_error(info["start_R"][k].cpu().numpy(), info["start_t"][k].cpu().numpy(), R_true, t_true)[0]
                          for k in range(8)]
                lines.append("          refinement (8 starts, 40 rounds, all points) %8.3f / %8.3f   global_mesh_icp with these levels %8.3f / "
                             "%8.3f   the yardstick's scoring alone is %.0f times the whole call   pose error %.2e degrees, %.2e   "
                             "starts %s degrees off, ok %s" % (refine[1], refine[2], whole[1], whole[2], yard[2] * batches / whole[2], rot,
                                                               tr, " ".join("%.0f" % s for s in starts), info["ok"].tolist()))
            print("\n".join(lines[shown:]), flush=True)
            shown = len(lines)
        # the same call with offsets that reach the gap between the centroids: 9^3 offsets of 4 voxels, the first volume
        levels, origin, voxel = coarse
        wide = timed(lambda: mgl.global_mesh_icp(p, vt, ft, n_rotations=args.rotations, t_steps=9, t_step=4 * voxel, n_score=2048,
                                                 levels=levels, origin=origin, voxel=voxel, bvh=tree), 2)
        R, t, info = wide[0]
        rot, tr = mr.pose_error(R.cpu().numpy(), t.cpu().numpy(), R_true, t_true)
        sub = p[::-(-p.shape[0] // 2048)].contiguous()
        off9 = mgl.offset_grid(9, 4 * voxel, dev)
        sc9 = timed(lambda: mgl.pose_scores(sub, Rg, base, off9, levels, origin, voxel), args.reps)
        lines.append("  729 offsets of 4 voxels (reach %.2f), first volume, %d scoring points: pose_scores with the sort %8.3f / %8.3f   "
                     "global_mesh_icp %8.3f / %8.3f   pose error %.2e degrees, %.2e   final %s" % (
                         4 * 4 * voxel, sub.shape[0], sc9[1], sc9[2], wide[1], wide[2], rot, tr,
                         " ".join("%.3g" % x for x in info["final"].tolist())))
        print(lines[-1], flush=True)
        shown = len(lines)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
