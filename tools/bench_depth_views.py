"""What the multi-view depth check costs: m4d_depth_views for K = 1, 4, 8 earlier frames beside m4d_depth_cloud's two passes on the
same frames, and the predict loop
(--stream --graph --save_dir --save_cloud) with and without --cloud_views 4.

    python tools/bench_depth_views.py [--out profiles/depth_views.txt] [--rounds 9] [--calls 500] [--window 0.3] [--no_driver]

Method (that of tools/bench_consistency.py): ``calls`` launches of ONE variant at fixed arguments are captured into a hipGraph
(the entry points are plain launches), so the host's enqueue time is out of the picture; a timed window is as many replays of
that graph as fill ``window`` seconds, between two device events, after a warm-up replay.  The variants alternate inside a round
so a drift of the machine hits all of them; reported are the median over the rounds and the spread (min .. max) of the time per
call, which includes the gap the graph executor leaves between dependent kernel nodes (one per call for the check, two for the
cloud).  At fixed arguments every replay writes the same ring slot; the ring is filled from a moving camera over a tilted plane
(tests/depth_views_ref.py's scene at full size), so every view tests and confirms most pixels: the expensive case.

The end-to-end figure is the loop of tools/bench_cloud_export.py (profiles/cloud_export.txt): GraphedStream replays on synthetic
frames, export.PredictionWriter with clouds at stride 2, the host clock from the first timed step to the end of close(); the two
forms alternate.  Needs a GPU: there is no fallback.
"""
import argparse
import ctypes
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = [(1, 384, 384), (8, 384, 384), (8, 384, 512)]              # (batch, H, W)
VIEWS = (1, 4, 8)


def plane_scene(b, h, w, n):
    """n frames of a tilted plane from a camera that moves and turns a little every frame: (maps [n,b,h,w,1] float32,
    poses [n,b,7] float64, f, c [b,2] float32)."""
    f = np.tile(np.array([[0.5 * w, 0.5 * h]], np.float32), (b, 1))
    c = np.tile(np.array([[0.5 * w - 0.3, 0.5 * h + 0.4]], np.float32), (b, 1))
    normal = np.array([0.12, -0.2, 1.0]) / np.linalg.norm([0.12, -0.2, 1.0])
    axis = np.array([0.3, -0.8, 0.52]) / np.linalg.norm([0.3, -0.8, 0.52])
    rows, cols = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    x, y = ((cols + 0.5) - float(c[0, 0])) / float(f[0, 0]), ((rows + 0.5) - float(c[0, 1])) / float(f[0, 1])
    maps, poses = np.empty((n, b, h, w, 1), np.float32), np.empty((n, b, 7))
    for k in range(n):
        ang = np.deg2rad(0.4 * k)
        qw, (qx, qy, qz) = np.cos(ang / 2), axis * np.sin(ang / 2)
        rot = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                        [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                        [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])
        t = np.array([0.08, -0.04, 0.06]) * k
        den = sum(normal[i] * (rot[i, 0] * x + rot[i, 1] * y + rot[i, 2]) for i in range(3))
        maps[k] = ((9.0 - normal @ t) / den).astype(np.float32)[None, :, :, None]
        poses[k] = [qw, qx, qy, qz, *t]
    return maps, poses, f, c


def main(argv=None):
    import torch
    from m4depth_amd import network_ops as nops
    from m4depth_amd._lib import lib, check, stream_ptr, build_info
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_views.txt"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=500, help="launches per captured graph")
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--no_driver", action="store_true", help="skip the main.py --stream --graph runs")
    ap.add_argument("--driver_rounds", type=int, default=3)
    ap.add_argument("--driver_steps", type=int, default=200, help="timed steps per run of the predict loop")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth_views needs a GPU")
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream(device=dev)
    windows = []

    def graph_of(fn):
        torch.cuda.synchronize()                                   # what fn reads was written on the default stream
        with torch.cuda.stream(side):
            fn()                                                   # first launch outside the capture: loads the code object
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(args.calls):
                fn()
        g.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.replay()
        torch.cuda.synchronize()
        # fn travels with its graph: its default arguments own the tensors whose addresses the graph holds.  Dropped, they would
        # be freed when the next variant rebinds the names, and the next capture's empty_cache() would unmap them under this graph
        return g, max(3, int(args.window / max(time.perf_counter() - t0, 1e-5))), fn

    def timed(item):
        g, replays, _ = item
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(replays):
            g.replay()
        end.record()
        end.synchronize()
        windows.append(start.elapsed_time(end) * 1e-3)
        return start.elapsed_time(end) * 1e3 / (replays * args.calls)      # microseconds per call

    def stats(v):
        return f"median {np.median(v):8.2f} us  (min {np.min(v):8.2f} .. max {np.max(v):8.2f})"

    lines = [f"# tools/bench_depth_views.py -- {build_info()}", f"# device: {torch.cuda.get_device_name(0)}",
             f"# {args.rounds} rounds per variant; a window = replays of a hipGraph of {args.calls} calls between device events; "
             "the variants alternate within a round", ""]
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    for b, h, w in CASES:
        maps, poses, f, c = plane_scene(b, h, w, max(VIEWS) + 1)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        cam_f, cam_c = t(f), t(c)
        rgb = torch.rand((b, h, w, 3), device=dev)
        variants, shares = {}, {}
        for K in VIEWS:
            state = nops.depth_views_state(b, h, w, K, dev)
            for k in range(K):                                     # fill the ring through the wrapper: frames 0 .. K-1
                nops.depth_views(t(maps[k]), cam_f, cam_c, t(poses[k]), state, force_all=(k == 0))
            depth, pose = t(maps[K]), t(poses[K])
            n_views = torch.empty((b, h, w), dtype=torch.uint8, device=dev)
            depth_f = torch.empty((b, h, w, 1), device=dev)
            age_in, age_out = state["age"]
            head, mv = state["head"], min(2, K)

            def check_call(depth=depth, pose=pose, state=state, K=K, head=head, age_in=age_in, age_out=age_out, mv=mv,
                           n_views=n_views, depth_f=depth_f, cam_f=cam_f, cam_c=cam_c):
                check(lib.m4d_depth_views(p(depth), h * w, p(cam_f), p(cam_c), p(pose), None, 0, b, h, w, K, head,
                                          p(state["ring_depth"]), p(state["ring_pose"]), p(age_in), p(age_out), 1.0, 0.01, mv,
                                          p(n_views), p(depth_f), stream_ptr()), "m4d_depth_views")

            variants[f"views{K}"] = graph_of(check_call)
            torch.cuda.synchronize()
            shares[K] = (float((n_views == K).float().mean()), float(torch.isfinite(depth_f).float().mean()))
        for step in (1, 2):
            cap = nops.cloud_capacity(h, w, step)
            vertices = torch.empty((b, cap, 16), dtype=torch.uint8, device=dev)
            counts = torch.empty(b, dtype=torch.int32, device=dev)
            ws = torch.empty(max(int(lib.m4d_depth_cloud_workspace_ints(b, h, w, step)), 1), dtype=torch.int32, device=dev)
            depth, pose = t(maps[1]), t(poses[1])

            def cloud_call(step=step, vertices=vertices, counts=counts, ws=ws, depth=depth, pose=pose, rgb=rgb, cam_f=cam_f,
                           cam_c=cam_c):
                check(lib.m4d_depth_cloud(p(depth), h * w, p(rgb), 3 * h * w, p(cam_f), p(cam_c), p(pose), b, h, w, step, 1.0, 80.0,
                                          p(vertices), p(counts), p(ws), stream_ptr()), "m4d_depth_cloud")

            variants[f"cloud{step}"] = graph_of(cloud_call)
        times = {name: [] for name in variants}
        names = list(variants)
        for k in range(args.rounds):
            for name in (names if k % 2 == 0 else names[::-1]):
                times[name].append(timed(variants[name]))
        lines.append(f"batch {b}, {h}x{w}")
        for K in VIEWS:
            lines.append(f"  m4d_depth_views, K = {K} (1 launch)          {stats(times[f'views{K}'])}  "
                         f"per frame {np.median(times[f'views{K}']) / b:7.2f} us   ({100 * shares[K][0]:.1f} % of the pixels confirmed by "
                         f"all {K}, {100 * shares[K][1]:.1f} % kept)")
        for step in (1, 2):
            lines.append(f"  m4d_depth_cloud, stride {step} (2 launches)     {stats(times[f'cloud{step}'])}  "
                         f"per frame {np.median(times[f'cloud{step}']) / b:7.2f} us")
        lines.append("")
    lines.insert(3, f"# timed windows: {min(windows):.2f} .. {max(windows):.2f} s")

    if not args.no_driver:
        import shutil
        import m4depth_amd as M
        from m4depth_amd import main as MAIN, network as net, synthetic as S
        from m4depth_amd.export import PredictionWriter, FrameNamer
        size, levels, warmup, steps = 384, 6, 10, args.driver_steps
        lines.append(f"predict loop as tools/bench_cloud_export.py runs it: --stream --graph, synthetic {size}x{size}, {levels} levels "
                     f"(random weights); {steps} steps per run after {warmup} warm-up steps, {args.driver_rounds} runs per form, "
                     "alternating; frames/s (steps x batch) by the host clock, close() included; writer: 4 slots, 8 threads, kitti16, "
                     f"--save_range 1 80, clouds at stride 2; {os.cpu_count()} CPUs visible, "
                     f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}")
        tmp = tempfile.mkdtemp(prefix="m4d_views_bench_")
        try:
            for b in (1, 8):
                samples, cam = S.make_sequence(b, 8, size, size, seed=7, motion="lateral")
                cam_d = {k: torch.from_numpy(v).to(dev) for k, v in cam.items()}
                frames = [{"RGB_im": torch.from_numpy(x["RGB_im"]).to(dev), "depth": torch.from_numpy(x["depth"]).to(dev),
                           "rot": torch.from_numpy(x["rot"]).to(dev), "trans": torch.from_numpy(x["trans"]).to(dev),
                           "new_traj": torch.zeros(b, dtype=torch.bool), "camera": cam_d} for x in samples]
                model = M.M4Depth(nbre_levels=levels)
                model.load_numpy_weights(S.init_weights(levels, seed=42), dev)
                runner = net.GraphedStream(model, MAIN._stream_frame(dict(frames[0], new_traj=torch.ones(b, dtype=torch.bool)), dev))
                share = {}

                def run(views):
                    out = os.path.join(tmp, f"v{views}_{b}")
                    writer = PredictionWriter(out, "kitti16", cloud=True, cloud_step=2, cloud_views=views)
                    namer = FrameNamer(b)
                    t0 = None
                    for i in range(warmup + steps):
                        if i == warmup:
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                        f = frames[i % 8]
                        est = runner(MAIN._stream_frame(f, dev))["depth"]
                        writer.submit(est, namer(f["new_traj"]), rgb=f["RGB_im"], rot=f["rot"], trans=f["trans"], camera=f["camera"],
                                      reset=f["new_traj"])
                    writer.close()
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    share[views] = (writer.cloud_kept, writer.cloud_cap)
                    shutil.rmtree(out, ignore_errors=True)
                    return steps * b / dt

                fps = {0: [], 4: []}
                for k in range(args.driver_rounds):
                    for views in ((0, 4) if k % 2 == 0 else (4, 0)):
                        fps[views].append(run(views))
                        print(f"batch {b} cloud_views {views}: {fps[views][-1]:.1f} frames/s", flush=True)
                lines += ["", f"batch {b}"]
                for views, label in ((0, "--save_dir --save_cloud"), (4, "--save_dir --save_cloud --cloud_views 4")):
                    x = fps[views]
                    lines.append(f"  {label:42s} runs {', '.join(f'{y:7.1f}' for y in x)}   median {np.median(x):7.1f}   "
                                 f"(clouds hold {share[views][0]} of {share[views][1]} possible vertices)")
                lines.append(f"  with / without = {np.median(fps[4]) / np.median(fps[0]):.3f}; spread of the form without: "
                             f"{min(fps[0]) / np.median(fps[0]):.3f} .. {max(fps[0]) / np.median(fps[0]):.3f} of its median")
                del runner, model
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
