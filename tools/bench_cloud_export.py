"""What --save_cloud costs the predict loop: main.py --mode=predict --stream --graph on synthetic Mid-Air-sized frames (384x384,
6 levels), batch 1 and batch 8, three forms of the loop body, ``--runs`` runs of ``--frames`` steps each, interleaved --

  (a) save   : export.PredictionWriter, depth PNGs (--save_dir alone)
  (b) cloud2 : the same + clouds at stride 2 (--save_cloud, the default stride)
  (c) cloud1 : the same + clouds at stride 1

-- timed with the host clock from the first timed step to the end of ``close()``, after ``--warmup`` steps; ``--dry`` runs the
forms with ``encode=False`` (kernels, copies and ring, no file written) to tell the copy of the ``cap`` region from the file
writes.  Writes the table to ``--out``.

    python tools/bench_cloud_export.py --out profiles/cloud_export.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_cloud_export.py --kernel-only 200   # a run of its own
    python tools/bench_cloud_export.py --kernel-stats DIR/.../*_kernel_stats.csv --out profiles/cloud_export.txt      # appends
"""
import argparse
import csv
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KERNELS = ("pose_accumulate_kernel", "cloud_count_kernel", "cloud_write_kernel")
FORMS = {"save": None, "cloud2": 2, "cloud1": 1}


def kernel_stats(path):
    lines = []
    for r in csv.DictReader(open(path)):
        name = next((k for k in KERNELS if k in r["Name"]), None)
        if name is not None:
            lines.append(f"{name}: {r['Calls']} calls, average {float(r['AverageNs']) / 1e3:.2f} us, min "
                         f"{float(r['MinNs']) / 1e3:.2f} us, max {float(r['MaxNs']) / 1e3:.2f} us")
    return lines or ["no cloud kernel found in " + path]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200, help="timed steps per run")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--levels", type=int, default=6)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--dry", action="store_true", help="also time every form with encode=False")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", type=int, default=0, metavar="N",
                    help="launch the pose step and the cloud kernels (batch 1, stride 1, world frame) N times and exit")
    ap.add_argument("--kernel-stats", default=None, metavar="CSV", help="append the cloud kernels' rows of a rocprofv3 stats file")
    a = ap.parse_args()

    if a.kernel_stats is not None:
        lines = [f"rocprofv3 --kernel-trace --stats, a run of its own: batch 1, {a.size}x{a.size}, stride 1, world frame"]
        lines += kernel_stats(a.kernel_stats)
        print("\n".join(lines))
        if a.out:
            with open(a.out, "a") as fh:
                fh.write("\n" + "\n".join(lines) + "\n")
        return 0

    import torch
    import m4depth_amd as M
    from m4depth_amd import main as MAIN, network as net, network_ops as nops, synthetic as S
    from m4depth_amd.export import PredictionWriter, FrameNamer
    dev = torch.device("cuda:0")

    def make_frames(b):
        samples, cam = S.make_sequence(b, 8, a.size, a.size, seed=7, motion="lateral")
        cam_d = {k: torch.from_numpy(v).to(dev) for k, v in cam.items()}
        return [{"RGB_im": torch.from_numpy(s["RGB_im"]).to(dev), "depth": torch.from_numpy(s["depth"]).to(dev),
                 "rot": torch.from_numpy(s["rot"]).to(dev), "trans": torch.from_numpy(s["trans"]).to(dev),
                 "new_traj": torch.zeros(b, dtype=torch.bool), "camera": cam_d} for s in samples]

    if a.kernel_only:
        f = make_frames(1)[0]
        pose = torch.empty((1, 7), dtype=torch.float64, device=dev)
        nops.pose_accumulate(f["rot"], f["trans"], pose, force_all=True)
        for _ in range(a.kernel_only):
            nops.pose_accumulate(f["rot"], f["trans"], pose)
            nops.depth_cloud(f["depth"], f["RGB_im"], f["camera"]["f"], f["camera"]["c"], step=1, near=1.0, far=80.0, pose=pose)
        torch.cuda.synchronize()
        return 0

    tmp = tempfile.mkdtemp(prefix="m4d_cloud_bench_")
    lines = [f"predict loop, --stream --graph, synthetic {a.size}x{a.size}, {a.levels} levels; {a.frames} steps per run after "
             f"{a.warmup} warm-up steps, {a.runs} runs per form, interleaved; frames/s (steps x batch) by the host clock, close() "
             f"included; writer: 4 slots, 8 threads, kitti16, --save_range 1 80; {os.cpu_count()} CPUs visible, "
             f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}"]
    try:
        for b in (int(v) for v in a.batches.split(",")):
            frames = make_frames(b)
            model = M.M4Depth(nbre_levels=a.levels)
            model.load_numpy_weights(S.init_weights(a.levels, seed=42), dev)
            runner = net.GraphedStream(model, MAIN._stream_frame(dict(frames[0], new_traj=torch.ones(b, dtype=torch.bool)), dev))
            kept = []

            def run(form, encode):
                out = os.path.join(tmp, f"{form}_{b}")
                stride = FORMS[form]
                writer = PredictionWriter(out, "kitti16", encode=encode, cloud=stride is not None, cloud_step=stride or 2)
                namer = FrameNamer(b)
                t0 = None
                for i in range(a.warmup + a.frames):
                    if i == a.warmup:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                    f = frames[i % 8]
                    est = runner(MAIN._stream_frame(f, dev))["depth"]
                    cloud = dict(rgb=f["RGB_im"], rot=f["rot"], trans=f["trans"], camera=f["camera"], reset=f["new_traj"]) \
                        if stride else {}
                    writer.submit(est, namer(f["new_traj"]), **cloud)
                writer.close()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if stride and encode and not kept:
                    from m4depth_amd.export import read_cloud_ply
                    first = os.path.join(out, "s00_t0000", "000000_cloud.ply")
                    kept.append((len(read_cloud_ply(first)[0]), nops.cloud_capacity(a.size, a.size, stride)))
                shutil.rmtree(out, ignore_errors=True)
                return a.frames * b / dt

            variants = [(f, True) for f in FORMS] + ([(f, False) for f in FORMS] if a.dry else [])
            fps = {v: [] for v in variants}
            for _ in range(a.runs):
                for v in variants:
                    fps[v].append(run(*v))
                    print(f"batch {b} {v[0]}{'' if v[1] else ' (dry)'}: {fps[v][-1]:.1f} frames/s", flush=True)
            lines += ["", f"batch {b}"]
            for v in variants:
                x = fps[v]
                label = {"save": "--save_dir", "cloud2": "--save_dir --save_cloud (stride 2)",
                         "cloud1": "--save_dir --save_cloud --cloud_stride 1"}[v[0]] + ("" if v[1] else ", encode=False")
                lines.append(f"  {label:58s} runs {', '.join(f'{y:7.1f}' for y in x)}   median {np.median(x):7.1f}")
            if kept:
                lines.append(f"  (the first frame's cloud at stride 2 holds {kept[0][0]} of {kept[0][1]} possible vertices)")
            del runner, model
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
