"""Soak of the BVH ray caster: seeded random scenes (triangle soups from millimetre to metre scale, random poses,
cameras inside and outside the mesh), each rendered by brute force and through a fresh MeshBVH; every output buffer
must match bit for bit.  The pytest suite runs 100 such cases (tests/test_render_bvh_gpu.py::test_fuzz).

    python tools/fuzz_render_bvh.py [--cases 2000] [--seed 0]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import numpy as np
    from tests import bvh_scenes
    from tests.test_render_bvh_gpu import both
    for case in range(args.cases):
        rs = np.random.RandomState(args.seed * 1000003 + case)
        n = int(rs.choice([1, 3, 17, 100, 1000, 5000]))
        scale = 10.0 ** rs.uniform(-4, 1.5)
        verts = (rs.normal(size=3) * [1, 1, 2] + rs.normal(size=(3 * n, 3)) * scale).astype(np.float32)
        faces = rs.randint(0, 3 * n, size=(n, 3)) if rs.rand() < 0.3 else np.arange(3 * n).reshape(-1, 3)
        colors = rs.uniform(0, 1, verts.shape).astype(np.float32)
        H, W = int(rs.randint(3, 64)), int(rs.randint(3, 64))
        R = bvh_scenes.rand_rot(rs) if rs.rand() < 0.5 else np.eye(3)
        both(verts, colors, faces, bvh_scenes.camera(H, W, t=rs.normal(size=3) * 0.3, R=R, f=rs.uniform(2, 60)),
             bvh_scenes.camera(H + 1, W + 2, t=rs.normal(size=3) * 0.3, f=rs.uniform(2, 60)))
        if case % 100 == 99:
            print("%d cases bit-exact" % (case + 1), flush=True)
    print("fuzz_render_bvh: %d cases bit-exact" % args.cases)


if __name__ == "__main__":
    main()
