#!/usr/bin/env python3
"""Reference-style synthetic training tracks on the device, then a few training steps on them.

    python examples/make_synthetic_tracks.py [--batch 4] [--track-length 2] [--steps 5] [--height 480] [--width 640]

For each track: the poses of data/create_syn_data.py (cameras around the origin looking at (0,0,3), the projector one
baseline to the side), the structured-light ray caster at four scales, the finishing step (blend, disparity, and the
reference's edge target: the data-generation LCN of the ambient image's Sobel magnitude) and the training set's
augmentation (data/dataset.py: blur, noise, salt and pepper).  The tracks are collated into TrackTrainer's layout and
trained on for a few steps with the full-size disparity / edge network.  ShapeNet does not ship offline: the scene is
tests/workloads.render_scene (a slanted wall and a few boxes).  Prints the time of every stage.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--track-length", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--bvh", action="store_true", 
                    help="ray-cast through a per-sample BVH (same output, faster on large meshes)")
    args = ap.parse_args()

    import numpy as np
    import torch
    from connecting_the_dots_amd import synth
    from connecting_the_dots_amd import torchext as te
    from connecting_the_dots_amd.nets import DispEdgeNet
    from connecting_the_dots_amd.train import TrackTrainer
    from tests import workloads

    H, W, TL = args.height, args.width, args.track_length
    dev = torch.device("cuda", 0)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    sc = workloads.render_scene(args.seed, H=H, W=W)
    K = sc["cam"][0]
    pat = workloads.syn_dot_pattern(H, W)
    sizes = [(H >> s, W >> s) for s in range(4)]
    pats = [p.contiguous() for p in synth.scale_patterns(torch.from_numpy(np.stack([pat] * 3, axis=2)).to(dev), sizes)]
    rng = np.random.RandomState(args.seed)
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    bvh = "auto" if args.bvh else None
    synth.render_track_sample(sc, pats, K, rng, track_length=TL, generator=g, bvh=bvh)          # warm-up (code objects)
    samples, ms = clock(lambda: [synth.render_track_sample(sc, pats, K, rng, track_length=TL, generator=g, sample_id=b, bvh=bvh)
                                 for b in range(args.batch)])
    print("render + finish + augment: %d tracks x %d frames x 4 scales at %dx%d: %.1f ms" % (args.batch, TL, H, W, ms))
    batch, ms = clock(lambda: synth.collate_tracks(samples))
    print("collate: %.2f ms" % ms)
    for s in range(3):
        gr = batch["grad%d" % s]
        print("grad%d (ambient Sobel -> datagen LCN edge target): mean %.4f, %.2f%% of pixels >= 0.2" %
              (s, float(gr.mean()), 100 * float((gr >= 0.2).float().mean())))
    lpats = [te.lcn(p[..., 0][None, None].contiguous(), 5, 0.05)[0] for p in pats]
    torch.manual_seed(0)
    tr = TrackTrainer(DispEdgeNet(2, 128), lpats, torch.from_numpy(K).to(dev), 0.075,
                      [float(K[0, 0]) / 2 ** s for s in range(4)], train_edge=-1)
    for step in range(args.steps):
        vals, ms = clock(lambda: tr.train_step(batch))
        print("train step %d: %.1f ms%s, loss %.5f (%d terms, all finite: %s)" %
              (step, ms, " (includes MIOpen's first-use kernel builds)" if step == 0 else "", sum(vals), len(vals),
               all(np.isfinite(v) for v in vals)))


if __name__ == "__main__":
    main()
