"""What the TSDF meshes cost: m4d_tsdf_allocate (with and without the per-thread skip of a repeated key) and m4d_tsdf_integrate
per frame, beside m4d_voxel_map_integrate and m4d_depth_cloud on the same frames; one extraction and one clear at 2^22 slots, split
into launches and sort/search; and the predict loop (--stream --graph --save_dir --save_cloud) with and without --save_mesh 0.05.

    M4D_LIB_FLAVOUR=experiments python tools/bench_tsdf_mesh.py [--out profiles/tsdf_mesh.txt] [--rounds 9] [--calls 100]
                                                                [--window 0.3] [--no_driver]

Method (that of tools/bench_voxel_map.py): ``calls`` launches of ONE variant at fixed arguments are captured into a hipGraph, so
the host's enqueue time is out of the picture; a timed window is as many replays of that graph as fill ``window`` seconds,
between two device events, after a warm-up replay.  The variants alternate inside a round; reported are the median over the
rounds and the spread (min .. max) of the time per call.  The scene is bench_depth_views' tilted plane 9 m away seen from a
moving camera; frames 0..4 are fused first, the timed calls work on frame 5 over and over: the steady state of a volume, in
which the voxels of a frame exist already (allocate finds its keys, integrate's sums grow, which costs nothing).  The form of
allocate without the skip exists in the experiments build of the library only; without it that row is left out.

The end-to-end figure is the loop of tools/bench_cloud_export.py (profiles/cloud_export.txt): GraphedStream replays on synthetic
frames (random weights: the estimates are noise, every ray opens voxels of its own -- the worst case for the table),
export.PredictionWriter with clouds at stride 2, the host clock from the first timed step to the last submit and to the end of
close(), which with --save_mesh extracts, sorts, copies and writes one mesh per slot; the two forms alternate.  Needs a GPU.
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

SIZE, SLOTS_LOG2, MAP_SLOTS_LOG2, PRIMED, TRUNC = 384, 22, 21, 5, 4
BATCHES, VOXELS = (1, 8), (0.05, 0.2)


def bars_lines():
    """The distance bars of tests/test_tsdf_mesh_ref.py: what the float64 variant of the numpy restatement measures against the
    analytic surfaces, doubled for float32 rounding and the per-sample cameras.  Runs on the CPU."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tsdf_mesh_ref as T
    S, P = T.SPHERE, T.PLANE
    lines = ["distance bars of tests/test_tsdf_mesh_ref.py (numpy restatement; the bars are twice what its float64 variant measures):"]
    for exact in (True, False):
        m = T.fuse(T.sphere_frames(), S["f"], S["c"], S["voxel"], S["trunc"], S["near"], S["far"], exact=exact).extract(1)
        r = np.linalg.norm(m["xyz"].astype(np.float64), axis=1)
        lines.append(f"  unit sphere, 26 views at 48x48, voxel {S['voxel']} m, K = {S['trunc']}, {'float64' if exact else 'float32'}: "
                     f"{len(m['keys'])} vertices, {len(m['quads'])} quads, radii {r.min():.5f} .. {r.max():.5f} m"
                     + (f"  -> band {1 - 2 * (1 - r.min()):.5f} .. {1 + 2 * (r.max() - 1):.5f} m" if exact else ""))
    for exact in (True, False):
        m = T.fuse(T.plane_frames(), T.PLANE_F, T.PLANE_C, P["voxel"], P["trunc"], P["near"], P["far"], exact=exact).extract(2)
        d = np.abs(m["xyz"].astype(np.float64) @ T.PLANE_NORMAL - T.PLANE_OFFSET) / P["voxel"]
        lines.append(f"  tilted plane at 3 m, 4 views at 24x32, voxel {P['voxel']} m, K = {P['trunc']}, {'float64' if exact else 'float32'}: "
                     f"{len(m['keys'])} vertices, largest distance {d.max():.5f} voxel" + (f"  -> bar {2 * d.max():.5f} voxel" if exact else ""))
    return lines


def main(argv=None):
    import torch
    from bench_depth_views import plane_scene
    from m4depth_amd import network_ops as nops
    from m4depth_amd._lib import lib, check, stream_ptr, build_info, has_experiments
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_mesh.txt"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=100, help="launches per captured graph")
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--no_driver", action="store_true", help="skip the predict loops")
    ap.add_argument("--driver_rounds", type=int, default=3)
    ap.add_argument("--driver_steps", type=int, default=200, help="timed steps per run of the predict loop")
    ap.add_argument("--driver_slots_log2", type=int, default=24)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf_mesh needs a GPU")
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

    lines = [f"# tools/bench_tsdf_mesh.py -- {build_info()}", f"# device: {torch.cuda.get_device_name(0)}",
             f"# {args.rounds} rounds per variant; a window = replays of a hipGraph of {args.calls} calls between device events; "
             "the variants alternate within a round", ""]
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    forms = [("allocate", lib.m4d_tsdf_allocate)]
    if has_experiments:
        forms.append(("allocate, no key skip", lib.m4d_tsdf_allocate_plain))
    px = SIZE * SIZE
    for b in BATCHES:
        maps, poses, f, c = plane_scene(b, SIZE, SIZE, PRIMED + 1)
        cam_f, cam_c = t(f), t(c)
        rgb = torch.rand((b, SIZE, SIZE, 3), device=dev)
        depths, pose_d = [t(maps[k]) for k in range(PRIMED + 1)], [t(poses[k]) for k in range(PRIMED + 1)]
        depth, pose = depths[PRIMED], pose_d[PRIMED]
        variants, notes = {}, {}
        clouds = [nops.depth_cloud(depths[k], rgb, cam_f, cam_c, step=1, pose=pose_d[k]) for k in range(PRIMED + 1)]
        vertices, counts = clouds[PRIMED]
        ws = torch.empty(max(int(lib.m4d_depth_cloud_workspace_ints(b, SIZE, SIZE, 1)), 1), dtype=torch.int32, device=dev)

        def cloud_call(vertices=vertices, counts=counts, ws=ws, depth=depth, pose=pose, rgb=rgb, cam_f=cam_f, cam_c=cam_c, b=b):
            check(lib.m4d_depth_cloud(p(depth), px, p(rgb), 3 * px, p(cam_f), p(cam_c), p(pose), b, SIZE, SIZE, 1, 1.0, 80.0,
                                      p(vertices), p(counts), p(ws), stream_ptr()), "m4d_depth_cloud")

        variants["m4d_depth_cloud, stride 1 (2 launches)"] = graph_of(cloud_call)
        for voxel in VOXELS:
            state = nops.tsdf_state(b, SLOTS_LOG2, dev)
            for k in range(PRIMED + 1):                                # frame 5 too: the timed allocate claims nothing
                nops.tsdf_integrate(depths[k], rgb, cam_f, cam_c, pose_d[k], voxel, TRUNC, state)
            torch.cuda.synchronize()
            st = dict(zip(nops.TSDF_STATS, state["stats"][0].cpu().tolist()))
            held = f"sample 0 holds {st['occupied']} voxels, dropped_full {st['dropped_full']}"
            for name, entry in forms:
                def call(entry=entry, voxel=voxel, state=state, depth=depth, pose=pose, cam_f=cam_f, cam_c=cam_c, b=b):
                    check(entry(p(depth), px, p(cam_f), p(cam_c), p(pose), b, SIZE, SIZE, 1.0, 80.0, voxel, TRUNC, p(state["words"]),
                                SLOTS_LOG2, stream_ptr()), "m4d_tsdf_allocate")
                variants[f"{name} v{voxel}"] = graph_of(call)
                notes[f"{name} v{voxel}"] = held

            def integrate_call(voxel=voxel, state=state, depth=depth, pose=pose, rgb=rgb, cam_f=cam_f, cam_c=cam_c, b=b):
                check(lib.m4d_tsdf_integrate(p(depth), px, p(rgb), 3 * px, p(cam_f), p(cam_c), p(pose), b, SIZE, SIZE, 1.0, 80.0, voxel,
                                             TRUNC, p(state["words"]), SLOTS_LOG2, stream_ptr()), "m4d_tsdf_integrate")
            before = int(state["stats"][0, 3])
            variants[f"integrate v{voxel}"] = graph_of(integrate_call)
            torch.cuda.synchronize()
            per_call = (int(state["stats"][0, 3]) - before) // (2 * args.calls + 1)
            notes[f"integrate v{voxel}"] = f"{held}; {per_call} records updated per call; the pass streams {8 << SLOTS_LOG2} bytes of keys"

            vm = nops.voxel_map_state(b, MAP_SLOTS_LOG2, dev)
            for k in range(PRIMED):
                nops.voxel_map_integrate(*clouds[k], voxel, k + 1, vm)

            def vm_call(voxel=voxel, vm=vm, vertices=vertices, counts=counts, b=b):
                check(lib.m4d_voxel_map_integrate(p(vertices), p(counts), b, px, voxel, PRIMED + 1, p(vm["words"]), MAP_SLOTS_LOG2,
                                                  stream_ptr()), "m4d_voxel_map_integrate")
            variants[f"m4d_voxel_map_integrate v{voxel}"] = graph_of(vm_call)
            torch.cuda.synchronize()
            notes[f"m4d_voxel_map_integrate v{voxel}"] = f"stride 1, 2^{MAP_SLOTS_LOG2} slots, sample 0 holds {int(vm['stats'][0, 3])} voxels"
        times = {name: [] for name in variants}
        names = list(variants)
        for k in range(args.rounds):
            for name in (names if k % 2 == 0 else names[::-1]):
                times[name].append(timed(variants[name]))
        lines.append(f"batch {b}, {SIZE}x{SIZE}, K = {TRUNC}, 2^{SLOTS_LOG2} slots per sample")
        for name in names:
            lines.append(f"  {name:40s} {stats(times[name])}  per frame {np.median(times[name]) / b:8.2f} us"
                         + (f"   ({notes[name]})" if name in notes else ""))
        lines.append("")
        del variants, clouds, state, vm
        torch.cuda.empty_cache()
    lines.insert(3, f"# timed windows: {min(windows):.2f} .. {max(windows):.2f} s")

    # one extraction and one clear at 2^22 slots, batch 1
    maps, poses, f, c = plane_scene(1, SIZE, SIZE, PRIMED + 1)
    rgb = torch.rand((1, SIZE, SIZE, 3), device=dev)
    for voxel in VOXELS:
        state = nops.tsdf_state(1, SLOTS_LOG2, dev)
        for k in range(PRIMED + 1):
            nops.tsdf_integrate(t(maps[k]), rgb, t(f), t(c), t(poses[k]), voxel, TRUNC, state)
        nops.tsdf_extract(state, 0, 2, voxel)                              # loads the code objects, warms the allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keys, _, tri, st = nops.tsdf_extract(state, 0, 2, voxel)
        torch.cuda.synchronize()
        wrapper_ms = (time.perf_counter() - t0) * 1e3
        occ = st["occupied"]
        out = (torch.empty(occ, dtype=torch.int64, device=dev), torch.empty((occ, 16), dtype=torch.uint8, device=dev),
               torch.empty((3 * occ, 5), dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev))
        words = p(state["words"])
        e = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        torch.cuda.synchronize()
        e[0].record()
        check(lib.m4d_tsdf_extract_vertices(words, 1, SLOTS_LOG2, 0, 2, voxel, p(out[0]), p(out[1]), occ, p(out[3][0:1]), stream_ptr()),
              "m4d_tsdf_extract_vertices")
        e[1].record()
        check(lib.m4d_tsdf_extract_faces(words, 1, SLOTS_LOG2, 0, 2, p(out[2]), 3 * occ, p(out[3][1:2]), stream_ptr()),
              "m4d_tsdf_extract_faces")
        e[2].record()
        torch.cuda.synchronize()
        n_v, n_q = out[3].cpu().tolist()
        t0 = time.perf_counter()
        nops.tsdf_order(out[0][:n_v], out[1][:n_v], out[2][:n_q])
        torch.cuda.synchronize()
        order_ms = (time.perf_counter() - t0) * 1e3
        e[3].record()
        nops.tsdf_clear(state)
        e[4].record()
        e[4].synchronize()
        us = lambda i, j: e[i].elapsed_time(e[j]) * 1e3
        lines += [f"once each, batch 1, 2^{SLOTS_LOG2} slots (134 MB), voxel {voxel} m: a volume of {occ} voxels, a mesh of {len(keys)} "
                  f"vertices and {len(tri)} triangles ({st['quads_dropped']} quads dropped at the rim):",
                  f"  m4d_tsdf_extract_vertices (1 launch, device events)                   {us(0, 1):9.1f} us",
                  f"  m4d_tsdf_extract_faces (1 launch, device events)                      {us(1, 2):9.1f} us",
                  f"  network_ops.tsdf_order (two sorts, searchsorted, gathers; host clock) {order_ms:9.2f} ms",
                  f"  network_ops.tsdf_extract (all of it with its two waits; host clock)   {wrapper_ms:9.2f} ms",
                  f"  m4d_tsdf_clear (1 launch, device events)                              {us(3, 4):9.1f} us", ""]
        del state, out
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
                     f"slots, 8 threads, kitti16, --save_range 1 80, clouds at stride 2, --save_mesh 0.05 (K = 4) with "
                     f"2^{args.driver_slots_log2} slots per sample; one trajectory per slot, so close() writes every mesh; "
                     f"{os.cpu_count()} CPUs visible, OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}")
        tmp = tempfile.mkdtemp(prefix="m4d_mesh_bench_")
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

                def run(with_mesh):
                    out = os.path.join(tmp, f"m{int(with_mesh)}_{b}")
                    writer = PredictionWriter(out, "kitti16", cloud=True, cloud_step=2, save_mesh=0.05 if with_mesh else None,
                                              mesh_slots_log2=args.driver_slots_log2)
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
                    note[with_mesh] = (writer.meshes, writer.mesh_vertices, writer.mesh_triangles, writer.mesh_dropped_range,
                                       writer.mesh_dropped_full)
                    shutil.rmtree(out, ignore_errors=True)
                    del writer
                    torch.cuda.empty_cache()
                    return steps * b / (t1 - t0), steps * b / (t2 - t0)

                fps = {False: [], True: []}
                for k in range(args.driver_rounds):
                    for with_mesh in ((False, True) if k % 2 == 0 else (True, False)):
                        fps[with_mesh].append(run(with_mesh))
                        print(f"batch {b} save_mesh {with_mesh}: {fps[with_mesh][-1][0]:.1f} | {fps[with_mesh][-1][1]:.1f} frames/s", flush=True)
                lines += ["", f"batch {b}"]
                for with_mesh, label in ((False, "--save_dir --save_cloud"), (True, "--save_dir --save_cloud --save_mesh 0.05")):
                    for col, what in ((0, "to the last submit"), (1, "close() included ")):
                        x = [r[col] for r in fps[with_mesh]]
                        lines.append(f"  {label:40s} {what}  runs {', '.join(f'{y:7.1f}' for y in x)}   median {np.median(x):7.1f}")
                m = note[True]
                lines.append(f"  (the last run with meshes: {m[0]} meshes, {m[1]} vertices, {m[2]} triangles, {m[3]} samples dropped out of "
                             f"range, {m[4]} by full tables)")
                for col, what in ((0, "to the last submit"), (1, "close() included")):
                    base = [r[col] for r in fps[False]]
                    lines.append(f"  {what}: with / without = {np.median([r[col] for r in fps[True]]) / np.median(base):.3f}; spread of "
                                 f"the form without: {min(base) / np.median(base):.3f} .. {max(base) / np.median(base):.3f} of its median")
                del runner, model
                torch.cuda.empty_cache()
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    lines += [""] + bars_lines()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
