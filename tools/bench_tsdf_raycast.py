"""What the fused depth per frame costs: m4d_tsdf_raycast (whole-range march and window = 2) beside m4d_tsdf_allocate and
m4d_tsdf_integrate of the same run, and against the forms its two choices were measured against (m4d_tsdf_raycast_plain: row-major
waves, no key reuse); the predict loop (--stream --graph --save_dir --save_cloud --save_mesh 0.05) with and without --save_fused;
and main.py --eval_streams 8 --graph with and without --fused 0.05.

    M4D_LIB_FLAVOUR=experiments python tools/bench_tsdf_raycast.py [--out profiles/tsdf_raycast.txt] [--rounds 9] [--calls 100]
                                                                   [--window 0.3] [--no_driver] [--no_eval] [--render]
                                                                   [--parent_lib SO]

--render adds m4d_tsdf_render to the same rounds (profiles/tsdf_render.txt): nearest and trilinear sampling beside
m4d_tsdf_raycast, each without and with the normal, colour and view outputs, and the forms the trilinear march's two devices were
measured against (m4d_tsdf_render_plain: the eight corners probed one by one, no corners kept).  --parent_lib SO times the
m4d_tsdf_raycast of another build of the library -- the parent commit's -- in the same rounds, and prints the ratio next to the
spread of the rounds.

Method and scene: those of tools/bench_tsdf_mesh.py -- ``calls`` launches of ONE variant at fixed arguments captured into a
hipGraph, a timed window = as many replays as fill ``window`` seconds between two device events after a warm-up replay, the
variants alternating inside a round, median and spread (min .. max) over the rounds.  The tilted plane 9 m away seen from a moving
camera: frames 0..5 are fused, frame 5's camera is rendered over and over (its own depth map is the guide of the windowed march).
The plain forms exist in the experiments build of the library only; without it those rows are left out.

End to end: the loop of tools/bench_tsdf_mesh.py (GraphedStream replays on synthetic frames with random weights -- the estimates
are noise, the worst case for the table and for the march, which finds a surface late or never) with --save_mesh 0.05, with and
without --save_fused, alternating; and main.py --mode=eval --eval_streams 8 --graph on the Mid-Air-format set of
tools/bench_stream_eval.py, in child processes, with and without --fused 0.05 (whole range and --fused_window 2).  Needs a GPU.
"""
import argparse
import ctypes
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SIZE, SLOTS_LOG2, PRIMED, TRUNC, MIN_FRAMES = 384, 22, 5, 4, 2
BATCHES, VOXELS = (1, 8), (0.05, 0.2)
PLAIN_FORMS = ((0, "row-major waves, every sample probes (plain)"), (1, "8x8 tiles, every sample probes"),
               (2, "row-major waves, key reuse"))
RENDER_NAMES = ("nearest", "trilinear")
RENDER_FORMS = ((0, "corners one by one, every sample probes (plain)"), (1, "corners together, every sample probes"),
                (2, "corners one by one, kept while the base cell stays"))


def main(argv=None):
    import torch
    from bench_depth_views import plane_scene
    from m4depth_amd import network_ops as nops
    from m4depth_amd._lib import lib, check, stream_ptr, build_info, has_experiments
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default profiles/tsdf_raycast.txt, with --render profiles/tsdf_render.txt")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=100, help="launches per captured graph")
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--render", action="store_true",
                    help="also time m4d_tsdf_render: nearest and trilinear sampling, with and without its three optional outputs, and "
                         "(experiments build) the forms its two devices were measured against")
    ap.add_argument("--parent_lib", default=None, metavar="SO",
                    help="another build of the library (the parent commit's libm4depth_hip.so): its m4d_tsdf_raycast is timed in the "
                         "same rounds")
    ap.add_argument("--no_driver", action="store_true", help="skip the predict loops")
    ap.add_argument("--no_eval", action="store_true", help="skip the --eval_streams children")
    ap.add_argument("--driver_rounds", type=int, default=3)
    ap.add_argument("--driver_steps", type=int, default=200, help="timed steps per run of the predict loop")
    ap.add_argument("--driver_slots_log2", type=int, default=24)
    ap.add_argument("--eval_traj", type=int, default=8)
    ap.add_argument("--eval_len", type=int, nargs=2, default=(30, 60))
    ap.add_argument("--eval_limit", type=int, default=240, help="time limit of one --eval_streams child, seconds")
    args = ap.parse_args(argv)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "tsdf_render.txt" if args.render else "tsdf_raycast.txt")
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf_raycast needs a GPU")
    dev = torch.device("cuda:0")
    parent = None
    if args.parent_lib:
        from m4depth_amd._lib import SIGNATURES
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        parent.m4d_tsdf_raycast.restype, parent.m4d_tsdf_raycast.argtypes = SIGNATURES["m4d_tsdf_raycast"][:2]
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

    lines = [f"# tools/bench_tsdf_raycast.py -- {build_info()}", f"# device: {torch.cuda.get_device_name(0)}",
             f"# {args.rounds} rounds per variant; a window = replays of a hipGraph of {args.calls} calls between device events; "
             "the variants alternate within a round", ""]
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    px = SIZE * SIZE
    for b in BATCHES:
        maps, poses, f, c = plane_scene(b, SIZE, SIZE, PRIMED + 1)
        cam_f, cam_c = t(f), t(c)
        rgb = torch.rand((b, SIZE, SIZE, 3), device=dev)
        depths, pose_d = [t(maps[k]) for k in range(PRIMED + 1)], [t(poses[k]) for k in range(PRIMED + 1)]
        depth, pose = depths[PRIMED], pose_d[PRIMED]
        out = torch.empty((b, SIZE, SIZE, 1), dtype=torch.float32, device=dev)
        extra = (torch.empty((b, SIZE, SIZE, 3), device=dev), torch.empty((b, SIZE, SIZE, 3), device=dev),
                 torch.empty((b, SIZE, SIZE, 3), dtype=torch.uint8, device=dev))       # normal, colour, view
        variants, notes = {}, {}
        for voxel in VOXELS:
            state = nops.tsdf_state(b, SLOTS_LOG2, dev)
            for k in range(PRIMED + 1):
                nops.tsdf_integrate(depths[k], rgb, cam_f, cam_c, pose_d[k], voxel, TRUNC, state)
            torch.cuda.synchronize()
            st = dict(zip(nops.TSDF_STATS, state["stats"][0].cpu().tolist()))
            held = f"sample 0 holds {st['occupied']} voxels, dropped_full {st['dropped_full']}"

            def allocate_call(voxel=voxel, state=state, depth=depth, pose=pose, cam_f=cam_f, cam_c=cam_c, b=b):
                check(lib.m4d_tsdf_allocate(p(depth), px, p(cam_f), p(cam_c), p(pose), b, SIZE, SIZE, 1.0, 80.0, voxel, TRUNC,
                                            p(state["words"]), SLOTS_LOG2, stream_ptr()), "m4d_tsdf_allocate")

            def integrate_call(voxel=voxel, state=state, depth=depth, pose=pose, rgb=rgb, cam_f=cam_f, cam_c=cam_c, b=b):
                check(lib.m4d_tsdf_integrate(p(depth), px, p(rgb), 3 * px, p(cam_f), p(cam_c), p(pose), b, SIZE, SIZE, 1.0, 80.0, voxel,
                                             TRUNC, p(state["words"]), SLOTS_LOG2, stream_ptr()), "m4d_tsdf_integrate")
            variants[f"m4d_tsdf_allocate v{voxel}"] = graph_of(allocate_call)
            variants[f"m4d_tsdf_integrate v{voxel}"] = graph_of(integrate_call)
            notes[f"m4d_tsdf_allocate v{voxel}"] = held
            for window in (None, 2):
                hits = torch.zeros(b, dtype=torch.int64, device=dev)
                nops.tsdf_raycast(state, cam_f, cam_c, pose, SIZE, SIZE, voxel, TRUNC, MIN_FRAMES, guide=depth if window else None,
                                  window=window, out=out, hits=hits)
                torch.cuda.synchronize()
                share = float(hits.sum()) / (b * px)
                label = "whole range 1..80 m" if window is None else f"window {window}"
                tail = (p(depth) if window else None, px if window else 0, window or 0, None, 0, p(out), px, None)

                def product(voxel=voxel, state=state, pose=pose, cam_f=cam_f, cam_c=cam_c, b=b, tail=tail):
                    check(lib.m4d_tsdf_raycast(p(state["words"]), b, SLOTS_LOG2, p(cam_f), p(cam_c), p(pose), SIZE, SIZE, 1.0, 80.0, voxel,
                                               TRUNC, MIN_FRAMES, *tail, stream_ptr()), "m4d_tsdf_raycast")
                variants[f"m4d_tsdf_raycast v{voxel}, {label}"] = graph_of(product)
                notes[f"m4d_tsdf_raycast v{voxel}, {label}"] = f"{100 * share:.1f} % of the pixels rendered; 8x8 tiles, key reuse"
                for variant, what in (PLAIN_FORMS if has_experiments else ()):
                    def plain(variant=variant, voxel=voxel, state=state, pose=pose, cam_f=cam_f, cam_c=cam_c, b=b, tail=tail):
                        check(lib.m4d_tsdf_raycast_plain(variant, p(state["words"]), b, SLOTS_LOG2, p(cam_f), p(cam_c), p(pose), SIZE, SIZE,
                                                         1.0, 80.0, voxel, TRUNC, MIN_FRAMES, *tail, stream_ptr()),
                              "m4d_tsdf_raycast_plain")
                    variants[f"  {what} v{voxel}, {label}"] = graph_of(plain)
                if parent is not None:
                    def before(voxel=voxel, state=state, pose=pose, cam_f=cam_f, cam_c=cam_c, b=b, tail=tail):
                        check(parent.m4d_tsdf_raycast(p(state["words"]), b, SLOTS_LOG2, p(cam_f), p(cam_c), p(pose), SIZE, SIZE, 1.0, 80.0,
                                                      voxel, TRUNC, MIN_FRAMES, *tail, stream_ptr()), "m4d_tsdf_raycast (--parent_lib)")
                    variants[f"  m4d_tsdf_raycast of --parent_lib v{voxel}, {label}"] = graph_of(before)
                if not args.render:
                    continue
                # m4d_tsdf_render: both samplings without and with the three optional outputs, then the forms its two devices
                # were measured against (trilinear, no optional output)
                for interp, outputs in ((0, False), (1, False), (0, True), (1, True)):
                    looks = [x for t3, s3 in zip(extra, (3 * px,) * 3) for x in ((p(t3), s3) if outputs else (None, 0))]

                    def render(voxel=voxel, state=state, pose=pose, cam_f=cam_f, cam_c=cam_c, b=b, tail=tail, interp=interp, looks=looks):
                        check(lib.m4d_tsdf_render(p(state["words"]), b, SLOTS_LOG2, p(cam_f), p(cam_c), p(pose), SIZE, SIZE, 1.0, 80.0, voxel,
                                                  TRUNC, MIN_FRAMES, *tail[:5], interp, *tail[5:7], *looks, tail[7], stream_ptr()),
                              "m4d_tsdf_render")
                    name = f"m4d_tsdf_render {RENDER_NAMES[interp]}{' + normal, colour, view' if outputs else ''} v{voxel}, {label}"
                    variants[name] = graph_of(render)
                    if interp and not outputs:
                        hits.zero_()
                        nops.tsdf_render(state, cam_f, cam_c, pose, SIZE, SIZE, voxel, TRUNC, MIN_FRAMES, guide=depth if window else None,
                                         window=window, interp="trilinear", out=out, hits=hits)
                        torch.cuda.synchronize()
                        notes[name] = f"{100 * float(hits.sum()) / (b * px):.1f} % of the pixels rendered; corners together, kept"
                for variant, what in (RENDER_FORMS if has_experiments else ()):
                    def plain_render(variant=variant, voxel=voxel, state=state, pose=pose, cam_f=cam_f, cam_c=cam_c, b=b, tail=tail):
                        check(lib.m4d_tsdf_render_plain(variant, p(state["words"]), b, SLOTS_LOG2, p(cam_f), p(cam_c), p(pose), SIZE, SIZE,
                                                        1.0, 80.0, voxel, TRUNC, MIN_FRAMES, *tail[:5], 1, *tail[5:7], None, 0, None, 0,
                                                        None, 0, tail[7], stream_ptr()), "m4d_tsdf_render_plain")
                    variants[f"  trilinear, {what} v{voxel}, {label}"] = graph_of(plain_render)
        times = {name: [] for name in variants}
        names = list(variants)
        for k in range(args.rounds):
            for name in (names if k % 2 == 0 else names[::-1]):
                times[name].append(timed(variants[name]))
            print(f"batch {b}: round {k + 1} of {args.rounds}, {len(names)} variants", flush=True)
        lines.append(f"batch {b}, {SIZE}x{SIZE}, K = {TRUNC}, min_frames {MIN_FRAMES}, 2^{SLOTS_LOG2} slots per sample")
        width = max(66, max(len(name) for name in names))
        for name in names:
            lines.append(f"  {name:{width}s} {stats(times[name])}  per frame {np.median(times[name]) / b:8.2f} us"
                         + (f"   ({notes[name]})" if name in notes else ""))
        for name in names:                                     # this build's raycast against --parent_lib's, and the spread of its rounds
            other = "  m4d_tsdf_raycast of --parent_lib" + name[len("m4d_tsdf_raycast"):]
            if name.startswith("m4d_tsdf_raycast v") and other in times:
                mine, theirs = np.array(times[name]), np.array(times[other])
                lines.append(f"  {name}: this build / --parent_lib = {np.median(mine) / np.median(theirs):.4f}; rounds of this build "
                             f"{mine.min() / np.median(mine):.4f} .. {mine.max() / np.median(mine):.4f} of their median, of the other "
                             f"{theirs.min() / np.median(theirs):.4f} .. {theirs.max() / np.median(theirs):.4f}")
        lines.append("")
        del variants, state
        torch.cuda.empty_cache()
    lines.insert(3, f"# timed windows: {min(windows):.2f} .. {max(windows):.2f} s")

    if not args.no_driver:
        import m4depth_amd as M
        from m4depth_amd import main as MAIN, network as net, synthetic as S
        from m4depth_amd.export import PredictionWriter, FrameNamer
        levels, warmup, steps = 6, 10, args.driver_steps
        lines.append(f"predict loop as tools/bench_tsdf_mesh.py runs it: --stream --graph, synthetic {SIZE}x{SIZE}, {levels} levels "
                     f"(random weights); {steps} steps per run after {warmup} warm-up steps, {args.driver_rounds} runs per form, "
                     "alternating; frames/s (steps x batch) by the host clock up to the last submit | close() included; writer: 4 "
                     f"slots, 8 threads, kitti16, --save_range 1 80, clouds at stride 2, --save_mesh 0.05 (K = 4) with "
                     f"2^{args.driver_slots_log2} slots per sample; {os.cpu_count()} CPUs visible, "
                     f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}")
        tmp = tempfile.mkdtemp(prefix="m4d_raycast_bench_")
        forms = (("--save_mesh 0.05", {}), ("--save_mesh 0.05 --save_fused", dict(save_fused=True)),
                 ("--save_mesh 0.05 --save_fused --fused_window 2", dict(save_fused=True, fused_window=2)))
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

                def run(label, kw):
                    out_dir = os.path.join(tmp, f"f{len(kw)}_{b}")
                    writer = PredictionWriter(out_dir, "kitti16", cloud=True, cloud_step=2, save_mesh=0.05,
                                              mesh_slots_log2=args.driver_slots_log2, **kw)
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
                    note[label] = (writer.fused_pixels, writer.fused_cap, writer.mesh_dropped_full)
                    shutil.rmtree(out_dir, ignore_errors=True)
                    del writer
                    torch.cuda.empty_cache()
                    return steps * b / (t1 - t0), steps * b / (t2 - t0)

                fps = {label: [] for label, _ in forms}
                for k in range(args.driver_rounds):
                    for label, kw in (forms if k % 2 == 0 else forms[::-1]):
                        fps[label].append(run(label, kw))
                        print(f"batch {b} {label}: {fps[label][-1][0]:.1f} | {fps[label][-1][1]:.1f} frames/s", flush=True)
                lines += ["", f"batch {b}"]
                for label, _ in forms:
                    for col, what in ((0, "to the last submit"), (1, "close() included ")):
                        x = [r[col] for r in fps[label]]
                        lines.append(f"  {label:48s} {what}  runs {', '.join(f'{y:7.1f}' for y in x)}   median {np.median(x):7.1f}")
                    fp, cap, full = note[label]
                    if cap:
                        lines.append(f"    (the last run: {100.0 * fp / cap:.1f} % of the pixels rendered, {full} samples dropped by full tables)")
                base = [r[0] for r in fps[forms[0][0]]]
                for label, _ in forms[1:]:
                    lines.append(f"  to the last submit: {label} / without = {np.median([r[0] for r in fps[label]]) / np.median(base):.3f}")
                lines.append(f"  spread of the form without: {min(base) / np.median(base):.3f} .. {max(base) / np.median(base):.3f} of its median")
                del runner, model
                torch.cuda.empty_cache()
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        lines.append("")

    if not args.no_eval:
        from bench_stream_eval import write_dataset
        data = tempfile.mkdtemp(prefix="m4d_raycast_eval_")
        try:
            t0 = time.perf_counter()
            cfg, rec, lengths = write_dataset(data, args.eval_traj, args.eval_len[0], args.eval_len[1], (SIZE, SIZE))
            lines.append(f"main.py --mode=eval --dataset=midair --eval_streams 8 --graph, child processes, alternating: "
                         f"{args.eval_traj} Mid-Air-format trajectories, {sum(lengths)} frames of {SIZE}x{SIZE} (written in "
                         f"{time.perf_counter() - t0:.1f} s), 6 levels, random weights (the estimates are noise); the loop's own "
                         "sample-frames/s, the first step excluded")
            base = [sys.executable, "-m", "m4depth_amd.main", "--mode=eval", "--dataset=midair", "--db_path_config", cfg, "--records_path",
                    rec, "--arch_depth", "6", "--height", str(SIZE), "--width", str(SIZE), "--eval_streams", "8", "--graph"]
            forms = (("without --fused", []), ("--fused 0.05", ["--fused", "0.05"]),
                     ("--fused 0.05 --fused_window 2", ["--fused", "0.05", "--fused_window", "2"]))
            rates, said = {label: [] for label, _ in forms}, {}
            for k in range(2):
                for label, extra in (forms if k % 2 == 0 else forms[::-1]):
                    r = subprocess.run(["timeout", "-k", "10", str(args.eval_limit)] + base + extra
                                       + ["--ckpt_dir", os.path.join(data, f"ck_{len(extra)}_{k}")], cwd=ROOT, capture_output=True, text=True)
                    if r.returncode != 0:
                        raise SystemExit(f"child failed with exit status {r.returncode}: {label}\n{(r.stdout + r.stderr)[-3000:]}")
                    rates[label].append(float(re.search(r"([0-9.]+) sample-frames/s", r.stdout).group(1)))
                    said[label] = [l for l in r.stdout.splitlines() if l.startswith("fused depth at")]
                    print(f"{label}: {rates[label][-1]:.1f} sample-frames/s", flush=True)
            for label, _ in forms:
                lines.append(f"  {label:32s} runs {', '.join(f'{y:7.1f}' for y in rates[label])}   median {np.median(rates[label]):7.1f}"
                             f"   = {np.median(rates[label]) / np.median(rates[forms[0][0]]):.3f} of the loop without")
                lines += ["    " + l for l in said[label]]
        finally:
            shutil.rmtree(data, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
