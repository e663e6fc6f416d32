"""What --refine_pose costs per step: pose_refine.PoseRefiner's fixed schedule (one pyramid launch, one mask launch, begin,
2 launches per iteration, end) next to the stream step it runs in front of.

    python tools/bench_pose_refine.py [--out profiles/pose_refine.txt] [--rounds 9] [--calls 20] [--window 0.3] [--no_stream]

Method (that of tools/bench_consistency.py): ``calls`` refiner steps are captured into a hipGraph, so the host's enqueue time is
out of the picture; a timed window is as many replays of that graph as fill ``window`` seconds, between two device events, after
a warm-up replay; reported are the median over the rounds and the spread of the time per step.  That time includes the gaps the
graph executor leaves between dependent kernel nodes, and every launch of a refiner step depends on the one before it.  In the
driver the refiner's launches are eager (in front of the graph replay), so there the host's enqueue time comes on top where the
device is not already behind.

The stream step's own time is ``network.GraphedStream`` replayed on the same shapes (6 levels, seeded weights) between device
events: code this change does not touch.  Needs a GPU: there is no fallback.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(1, 384, 384), (8, 384, 384), (8, 384, 512)]              # (batch, H, W)


def main(argv=None):
    import torch
    from m4depth_amd import M4Depth, synthetic
    from m4depth_amd._lib import build_info, lib
    from m4depth_amd.network import GraphedStream
    from m4depth_amd.pose_refine import DEFAULTS, PoseRefiner
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_refine.txt"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20, help="refiner steps per captured graph")
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--no_stream", action="store_true", help="skip the stream step's own time")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_refine needs a GPU")
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream(device=dev)

    def stats(v):
        return f"median {np.median(v):8.2f} us  (min {np.min(v):8.2f} .. max {np.max(v):8.2f})"

    n_iter = len(DEFAULTS["strides"]) * DEFAULTS["iters"]
    lines = [f"# tools/bench_pose_refine.py -- {build_info()}", f"# device: {torch.cuda.get_device_name(0)}",
             f"# defaults (untuned): strides {DEFAULTS['strides']} x {DEFAULTS['iters']} iterations = {n_iter} iterations per step",
             f"# {args.rounds} windows per figure; a refiner window = replays of a hipGraph of {args.calls} steps between device events",
             ""]
    model = None
    for b, h, w in CASES:
        rng = np.random.default_rng(b * 1000 + w)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        img = np.stack([0.5 + 0.4 * np.sin(xx / (17 + 5 * c) + yy / 23) for c in range(3)], -1)[None].repeat(b, 0)
        cur, prev = t(img + rng.normal(0, 0.01, img.shape)), t(np.roll(img, 2, axis=2) + rng.normal(0, 0.01, img.shape))
        est = t(8.0 + 2.0 * np.sin(xx / 60)[None, ..., None].repeat(b, 0))
        aa = rng.normal(0.0, 0.01, (b, 3))
        ang = np.linalg.norm(aa, axis=1, keepdims=True)
        rot = t(np.concatenate([np.cos(ang / 2), aa / np.maximum(ang, 1e-12) * np.sin(ang / 2)], axis=1))
        trans = t(rng.normal([0.3, 0.05, 0.1], 0.03, (b, 3)))
        camera = {"f": t(np.tile([[0.5 * w, 0.5 * h]], (b, 1))), "c": t(np.tile([[0.5 * w, 0.5 * h]], (b, 1)))}
        zeros, ones = torch.zeros(b, dtype=torch.uint8, device=dev), torch.ones(b, dtype=torch.uint8, device=dev)
        rows = torch.empty((b, 8), device=dev)
        frames = [{"RGB_im": prev, "rot": rot, "trans": trans, "camera": camera, "new_traj": zeros},
                  {"RGB_im": cur, "rot": rot, "trans": trans, "camera": camera, "new_traj": zeros}]
        refiner = PoseRefiner(copy_estimate=False)

        def step(k):
            refiner.step(frames[k % 2], zeros, ones, rows)
            refiner.keep(frames[k % 2], est)

        with torch.cuda.stream(side):
            step(0)                                                # passes through: builds the first pyramid
            step(1)                                                # the first full step: loads the code objects, sizes the workspace
            n1 = lib.m4d_launch_count()
            step(2)
            per_step = lib.m4d_launch_count() - n1
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for k in range(args.calls):
                step(3 + k)
        g.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.replay()
        torch.cuda.synchronize()
        replays = max(3, int(args.window / max(time.perf_counter() - t0, 1e-5)))
        t_r = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(replays):
                g.replay()
            e1.record()
            e1.synchronize()
            t_r.append(e0.elapsed_time(e1) * 1e3 / (replays * args.calls))
        r = rows.cpu().numpy()
        lines.append(f"batch {b}, {h}x{w}  ({per_step} library launches per step + 1 mask launch; applied {int(r[:, 6].sum())}/{b}, "
                     f"cover {r[:, 2].mean():.3f})")
        lines.append(f"  PoseRefiner.step                     {stats(t_r)}")
        if not args.no_stream:
            if model is None:
                model = M4Depth(nbre_levels=6)
                model.load_numpy_weights(synthetic.init_weights(6, seed=42), dev)
            model.reset_state()
            runner = GraphedStream(model, frames[0])
            for _ in range(4):
                runner(frames[1])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            runner(frames[1])
            torch.cuda.synchronize()
            reps = max(4, int(args.window / max(time.perf_counter() - t0, 1e-5)))
            t_s = []
            for _ in range(args.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    runner(frames[1])
                e1.record()
                e1.synchronize()
                t_s.append(e0.elapsed_time(e1) * 1e3 / reps)
            lines.append(f"  GraphedStream replay (6 levels)      {stats(t_s)}  refiner / stream step = "
                         f"{np.median(t_r) / np.median(t_s):.3f}")
            del runner
        lines.append("")
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:                            # after every case: a later failure keeps the earlier figures
            fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
