"""Streaming inference throughput: configs[1]'s geometry (384x1280, 6 levels), one frame per step, three forms compared --
eager ``predict_step`` per frame (the batch-synchronised path), eager ``M4Depth.stream_step`` and ``network.GraphedStream``
replay -- under two reset patterns: all-continue, and staggered (sample s starts a new trajectory every 8th frame, at offset
s mod 8).  Timed with device events over ``--frames`` frames after ``--warmup``; writes one JSON file per batch size and a
combined ``stream_bench.json`` into ``--out``.

    python tools/bench_stream.py --batches 1,8,32 --frames 200 --warmup 20 --out DIR
    python tools/bench_stream.py --trace kernel_trace.csv      # masked vs unmasked level closes, per level (rocprofv3 trace)

``predict_step`` only runs all-continue (it reads new_traj[0] and resets the whole batch: it cannot express the staggered
pattern).  The frames cycle through 8 distinct synthetic frames resident on the device, so no host-to-device copy is timed."""
import argparse
import collections
import csv
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CLOSE_KERNELS = ("refiner_tail6_kernel", "refiner_tail_kernel", "level_post_kernel")


def summarize_trace(path):
    """Mean / median duration of the level-closing kernels by (kernel, MASK, grid): at batch 1 of configs[1] the grid tells the
    level apart (m4d_refiner_tail6 is persistent: level 1 fills 2 workgroups per CU, the coarser levels launch one per tile)."""
    groups = collections.defaultdict(list)
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"]
        k = next((k for k in CLOSE_KERNELS if k in name), None)
        if k is None:
            continue
        m = re.search(k + r"<(true|false)>", name)
        mask = m.group(1) if m else "?"
        wg = int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"]) // max(1, int(r["Workgroup_Size_X"]))
        groups[(k, mask, wg)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = []
    for (k, mask, wg), d in sorted(groups.items()):
        out.append({"kernel": k, "mask": mask, "workgroups": wg, "calls": len(d), "mean_us": round(float(np.mean(d)), 3),
                    "median_us": round(float(np.median(d)), 3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--forms", default="predict_step,stream_step,graphed")
    ap.add_argument("--patterns", default="all_continue,staggered")
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--levels", type=int, default=6)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, help="summarise a rocprofv3 kernel trace instead of measuring")
    a = ap.parse_args()
    if a.trace:
        res = summarize_trace(a.trace)
        for r in res:
            print(json.dumps(r))
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "close_kernels.json"), "w") as fh:
                json.dump(res, fh, indent=1)
        return 0

    import torch
    import m4depth_amd as M
    from m4depth_amd import network as net, synthetic as S
    dev = torch.device("cuda:0")
    forms = a.forms.split(",")
    patterns = a.patterns.split(",")
    results = []
    for b in [int(x) for x in a.batches.split(",")]:
        model = M.M4Depth(nbre_levels=a.levels)
        model.load_numpy_weights(S.init_weights(a.levels, seed=42), dev)
        samples, cam = S.make_sequence(b, 8, a.height, a.width, seed=7, motion="lateral")
        cam_d = {k: torch.from_numpy(v).to(dev) for k, v in cam.items()}
        frames = [{"RGB_im": torch.from_numpy(s["RGB_im"]).to(dev), "rot": torch.from_numpy(s["rot"]).to(dev),
                   "trans": torch.from_numpy(s["trans"]).to(dev), "camera": cam_d} for s in samples]
        n_total = a.warmup + a.frames
        masks = {"all_continue": [torch.zeros(b, dtype=torch.bool, device=dev)] * 8,
                 "staggered": [torch.tensor([(t - s) % 8 == 0 for s in range(b)], device=dev) for t in range(8)]}
        host_false = torch.zeros(b, dtype=torch.bool)
        row = {"batch": b, "height": a.height, "width": a.width, "levels": a.levels, "frames": a.frames, "forms": {}}

        def timed(step):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for i in range(n_total):
                if i == a.warmup:
                    e0.record()
                step(i)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1) / a.frames
            return {"ms_per_frame": round(ms, 4), "frames_per_s": round(b * 1000.0 / ms, 1)}

        if "predict_step" in forms:
            model.reset_state()
            model.predict_step(dict(frames[0], new_traj=torch.ones(b, dtype=torch.bool)))
            row["forms"]["predict_step/all_continue"] = timed(
                lambda i: model.predict_step(dict(frames[i % 8], new_traj=host_false)))
        for pat in patterns:
            if "stream_step" in forms:
                model.reset_state()
                row["forms"][f"stream_step/{pat}"] = timed(
                    lambda i: model.stream_step(dict(frames[i % 8], new_traj=masks[pat][i % 8])))
            if "graphed" in forms:
                model.reset_state()
                runner = net.GraphedStream(model, dict(frames[0], new_traj=masks[pat][0]))
                ins = runner.input_buffers()
                # the producer writes each frame straight into the static inputs (what a camera loader would do); the
                # frame's device-to-device hand-over copies are part of the timed loop
                def step(i, runner=runner, ins=ins, pat=pat):
                    f = frames[i % 8]
                    for k in ("RGB_im", "rot", "trans"):
                        ins[k].copy_(f[k], non_blocking=True)
                    ins["new_traj"].copy_(masks[pat][i % 8], non_blocking=True)
                    runner()
                row["forms"][f"graphed/{pat}"] = timed(step)
                del runner
        f = row["forms"]
        if "graphed/all_continue" in f and "graphed/staggered" in f:
            row["graphed_staggered_over_all_continue"] = round(f["graphed/staggered"]["ms_per_frame"] / f["graphed/all_continue"]["ms_per_frame"], 4)
        if "graphed/all_continue" in f and "predict_step/all_continue" in f:
            row["graphed_speedup_over_predict_step"] = round(f["predict_step/all_continue"]["ms_per_frame"] / f["graphed/all_continue"]["ms_per_frame"], 3)
        print(json.dumps(row), flush=True)
        results.append(row)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, f"stream_bench_b{b}.json"), "w") as fh:
                json.dump(row, fh, indent=1)
        del model
        torch.cuda.empty_cache()
    if a.out:
        with open(os.path.join(a.out, "stream_bench.json"), "w") as fh:
            json.dump(results, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
