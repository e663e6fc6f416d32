"""What the voxel maps cost: m4d_voxel_map_integrate per frame beside m4d_depth_cloud's two passes on the same frames, with and
without the in-wave combining of equal keys; one extract and one clear at 2^21 slots; and the predict loop
(--stream --graph --save_dir --save_cloud) with and without --save_map 0.05.

    M4D_LIB_FLAVOUR=experiments python tools/bench_voxel_map.py [--out profiles/voxel_map.txt] [--rounds 9] [--calls 200]
                                                                [--window 0.3] [--no_driver]

Method (that of tools/bench_depth_views.py): ``calls`` launches of ONE variant at fixed arguments are captured into a hipGraph, so
the host's enqueue time is out of the picture; a timed window is as many replays of that graph as fill ``window`` seconds,
between two device events, after a warm-up replay.  The variants alternate inside a round; reported are the median over the
rounds and the spread (min .. max) of the time per call.  The scene is bench_depth_views' tilted plane 9 m away seen from a
moving camera; frames 0..4 are integrated first under stamps 1..5, the timed call integrates frame 5 under stamp 6 over and over:
the steady state of a map, in which most voxels of a frame exist already (the sums grow, which costs nothing; the statistics
printed beside each figure say what the table held).  The form without combining exists in the experiments build of the library
only (make EXPERIMENTS=1, M4D_LIB_FLAVOUR=experiments); without it that column is left out.

The end-to-end figure is the loop of tools/bench_cloud_export.py (profiles/cloud_export.txt): GraphedStream replays on synthetic
frames (random weights: the estimates are noise, every vertex opens a voxel of its own -- the worst case for the table),
export.PredictionWriter with clouds at stride 2, the host clock from the first timed step to the last submit and to the end of
close(), which with --save_map extracts, sorts, copies and writes one map per slot; the two forms alternate.  Needs a GPU.
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

SIZE, SLOTS_LOG2, PRIMED = 384, 21, 5
BATCHES, STRIDES, VOXELS = (1, 8), (1, 2), (0.05, 0.2)


def main(argv=None):
    import torch
    from bench_depth_views import plane_scene
    from m4depth_amd import network_ops as nops
    from m4depth_amd._lib import lib, check, stream_ptr, build_info, has_experiments
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_map.txt"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200, help="launches per captured graph")
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--no_driver", action="store_true", help="skip the predict loops")
    ap.add_argument("--driver_rounds", type=int, default=3)
    ap.add_argument("--driver_steps", type=int, default=200, help="timed steps per run of the predict loop")
    ap.add_argument("--driver_slots_log2", type=int, default=24)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_voxel_map needs a GPU")
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream(device=dev)
    windows = []

    def graph_of(fn):
        torch.cuda.synchronize()
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
        return g, max(3, int(args.window / max(time.perf_counter() - t0, 1e-5))), fn     # fn owns the graph's tensors

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

    lines = [f"# tools/bench_voxel_map.py -- {build_info()}", f"# device: {torch.cuda.get_device_name(0)}",
             f"# {args.rounds} rounds per variant; a window = replays of a hipGraph of {args.calls} calls between device events; "
             "the variants alternate within a round", ""]
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    forms = [("combined", lib.m4d_voxel_map_integrate)]
    if has_experiments:
        forms.append(("uncombined", lib.m4d_voxel_map_integrate_uncombined))
    for b in BATCHES:
        maps, poses, f, c = plane_scene(b, SIZE, SIZE, PRIMED + 1)
        cam_f, cam_c = t(f), t(c)
        rgb = torch.rand((b, SIZE, SIZE, 3), device=dev)
        variants, notes = {}, {}
        for step in STRIDES:
            cap = nops.cloud_capacity(SIZE, SIZE, step)
            clouds = [nops.depth_cloud(t(maps[k]), rgb, cam_f, cam_c, step=step, pose=t(poses[k])) for k in range(PRIMED + 1)]
            vertices, counts = clouds[PRIMED]
            ws = torch.empty(max(int(lib.m4d_depth_cloud_workspace_ints(b, SIZE, SIZE, step)), 1), dtype=torch.int32, device=dev)
            depth, pose = t(maps[PRIMED]), t(poses[PRIMED])

            def cloud_call(step=step, vertices=vertices, counts=counts, ws=ws, depth=depth, pose=pose):
                check(lib.m4d_depth_cloud(p(depth), SIZE * SIZE, p(rgb), 3 * SIZE * SIZE, p(cam_f), p(cam_c), p(pose), b, SIZE, SIZE,
                                          step, 1.0, 80.0, p(vertices), p(counts), p(ws), stream_ptr()), "m4d_depth_cloud")

            variants[f"cloud s{step}"] = graph_of(cloud_call)
            for voxel in VOXELS:
                for name, entry in forms:
                    state = nops.voxel_map_state(b, SLOTS_LOG2, dev)
                    for k in range(PRIMED):
                        nops.voxel_map_integrate(*clouds[k], voxel, k + 1, state)
                    torch.cuda.synchronize()
                    before = state["stats"][0].cpu().tolist()

                    def call(entry=entry, vertices=vertices, counts=counts, cap=cap, voxel=voxel, state=state):
                        check(entry(p(vertices), p(counts), b, cap, voxel, PRIMED + 1, p(state["words"]), SLOTS_LOG2, stream_ptr()),
                              "m4d_voxel_map_integrate")

                    key = f"integrate s{step} v{voxel} {name}"
                    variants[key] = graph_of(call)
                    torch.cuda.synchronize()
                    after = state["stats"][0].cpu().tolist()
                    notes[key] = (f"{int(counts[0])} vertices per sample; sample 0 held {before[3]} voxels before, {after[3]} after, "
                                  f"dropped_full {after[2]}")
        times = {name: [] for name in variants}
        names = list(variants)
        for k in range(args.rounds):
            for name in (names if k % 2 == 0 else names[::-1]):
                times[name].append(timed(variants[name]))
        lines.append(f"batch {b}, {SIZE}x{SIZE}, 2^{SLOTS_LOG2} slots per sample")
        for name in names:
            lines.append(f"  {name:36s} {stats(times[name])}  per frame {np.median(times[name]) / b:7.2f} us"
                         + (f"   ({notes[name]})" if name in notes else "   (2 launches)"))
        lines.append("")
        del variants, clouds
        torch.cuda.empty_cache()
    lines.insert(3, f"# timed windows: {min(windows):.2f} .. {max(windows):.2f} s")

    # one extract and one clear at 2^21 slots, batch 1: device events around the launch, and the host clock around the wrapper
    maps, poses, f, c = plane_scene(1, SIZE, SIZE, PRIMED + 1)
    state = nops.voxel_map_state(1, SLOTS_LOG2, dev)
    rgb = torch.rand((1, SIZE, SIZE, 3), device=dev)
    for k in range(PRIMED + 1):
        v, n = nops.depth_cloud(t(maps[k]), rgb, t(f), t(c), step=1, pose=t(poses[k]))
        nops.voxel_map_integrate(v, n, 0.05, k + 1, state)
    nops.voxel_map_extract(state, 0, 2, 0.05)                          # allocates the scratch, loads the code object
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    keys, _, st = nops.voxel_map_extract(state, 0, 2, 0.05)
    torch.cuda.synchronize()
    wrapper_ms = (time.perf_counter() - t0) * 1e3
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    state["count"].zero_()
    torch.cuda.synchronize()
    e0.record()
    check(lib.m4d_voxel_map_extract(p(state["words"]), 1, SLOTS_LOG2, 0, 2, 0.05, p(state["keys_out"]), p(state["vertices_out"]),
                                    1 << SLOTS_LOG2, p(state["count"]), stream_ptr()), "m4d_voxel_map_extract")
    e1.record()
    nops.voxel_map_clear(state)
    e2.record()
    e2.synchronize()
    lines += [f"once each, batch 1, 2^{SLOTS_LOG2} slots (168 MB), a map of {st['occupied']} voxels of which {len(keys)} seen by >= 2 frames:",
              f"  m4d_voxel_map_extract (1 launch, device events)       {e0.elapsed_time(e1) * 1e3:9.1f} us",
              f"  network_ops.voxel_map_extract (launch, wait, torch.sort, gather; host clock) {wrapper_ms:7.2f} ms",
              f"  m4d_voxel_map_clear (1 launch, device events)         {e1.elapsed_time(e2) * 1e3:9.1f} us", ""]
    del state
    torch.cuda.empty_cache()

    if not args.no_driver:
        import shutil
        import m4depth_amd as M
        from m4depth_amd import main as MAIN, network as net, synthetic as S
        from m4depth_amd.export import PredictionWriter, FrameNamer
        levels, warmup, steps = 6, 10, args.driver_steps
        lines.append(f"predict loop as tools/bench_cloud_export.py runs it: --stream --graph, synthetic {SIZE}x{SIZE}, {levels} levels "
                     f"(random weights); {steps} steps per run after {warmup} warm-up steps, {args.driver_rounds} runs per form, "
                     "alternating; frames/s (steps x batch) by the host clock up to the last submit | close() included; writer: 4 "
                     f"slots, 8 threads, kitti16, --save_range 1 80, clouds at stride 2, --save_map 0.05 with 2^{args.driver_slots_log2} "
                     f"slots per sample; one trajectory per slot, so close() writes every map; {os.cpu_count()} CPUs visible, "
                     f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}")
        tmp = tempfile.mkdtemp(prefix="m4d_map_bench_")
        try:
            for b in BATCHES:
                samples, cam = S.make_sequence(b, 8, SIZE, SIZE, seed=7, motion="lateral")
                cam_d = {k: torch.from_numpy(v).to(dev) for k, v in cam.items()}
                frames = [{"RGB_im": torch.from_numpy(x["RGB_im"]).to(dev), "depth": torch.from_numpy(x["depth"]).to(dev),
                           "rot": torch.from_numpy(x["rot"]).to(dev), "trans": torch.from_numpy(x["trans"]).to(dev),
                           "new_traj": torch.zeros(b, dtype=torch.bool), "camera": cam_d} for x in samples]
                model = M.M4Depth(nbre_levels=levels)
                model.load_numpy_weights(S.init_weights(levels, seed=42), dev)
                runner = net.GraphedStream(model, MAIN._stream_frame(dict(frames[0], new_traj=torch.ones(b, dtype=torch.bool)), dev))
                note = {}

                def run(with_map):
                    out = os.path.join(tmp, f"m{int(with_map)}_{b}")
                    writer = PredictionWriter(out, "kitti16", cloud=True, cloud_step=2, save_map=0.05 if with_map else None,
                                              map_slots_log2=args.driver_slots_log2)
                    namer = FrameNamer(b)
                    t0 = None
                    for i in range(warmup + steps):
                        if i == warmup:
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                        fr = frames[i % 8]
                        est = runner(MAIN._stream_frame(fr, dev))["depth"]
                        writer.submit(est, namer(fr["new_traj"]), rgb=fr["RGB_im"], rot=fr["rot"], trans=fr["trans"],
                                      camera=fr["camera"], reset=fr["new_traj"])
                    t1 = time.perf_counter()
                    writer.close()
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    note[with_map] = (writer.maps, writer.map_voxels, writer.map_dropped_range, writer.map_dropped_full)
                    shutil.rmtree(out, ignore_errors=True)
                    return steps * b / (t1 - t0), steps * b / (t2 - t0)

                fps = {False: [], True: []}
                for k in range(args.driver_rounds):
                    for with_map in ((False, True) if k % 2 == 0 else (True, False)):
                        fps[with_map].append(run(with_map))
                        print(f"batch {b} save_map {with_map}: {fps[with_map][-1][0]:.1f} | {fps[with_map][-1][1]:.1f} frames/s", flush=True)
                lines += ["", f"batch {b}"]
                for with_map, label in ((False, "--save_dir --save_cloud"), (True, "--save_dir --save_cloud --save_map 0.05")):
                    for col, what in ((0, "to the last submit"), (1, "close() included ")):
                        x = [r[col] for r in fps[with_map]]
                        lines.append(f"  {label:40s} {what}  runs {', '.join(f'{y:7.1f}' for y in x)}   median {np.median(x):7.1f}")
                m = note[True]
                lines.append(f"  (the last run with maps: {m[0]} maps, {m[1]} voxels written, {m[2]} vertices dropped out of range, "
                             f"{m[3]} by full tables)")
                for col, what in ((0, "to the last submit"), (1, "close() included")):
                    base = [r[col] for r in fps[False]]
                    lines.append(f"  {what}: with / without = {np.median([r[col] for r in fps[True]]) / np.median(base):.3f}; spread of "
                                 f"the form without: {min(base) / np.median(base):.3f} .. {max(base) / np.median(base):.3f} of its median")
                del runner, model
                torch.cuda.empty_cache()
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
