"""What saving predictions costs the predict loop: main.py --mode=predict --stream --graph on synthetic frames (384x1280, 6
levels, batch 1), four forms of the loop body, ``--runs`` runs of ``--frames`` frames each, interleaved --

  (a) list   : ``preds.append(predict(frame).cpu().numpy())`` -- the loop without --save_dir (one synchronisation and a
               4 B/pixel copy per frame, every frame kept)
  (b) dry    : export.PredictionWriter(encode=False) -- kernel, 2 B/pixel copy, ring, worker hand-off; no PNG encoder
  (c) kitti16: the writer, depth PNGs
  (d) panels : the writer, depth PNGs + the four panels

-- timed with the host clock from the first timed frame to the end of ``close()`` (or of the last ``.cpu()``), after
``--warmup`` frames.  The resident set size is sampled during (c).  Writes the table to ``--out``.

    python tools/bench_predict_export.py --out profiles/predict_export.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_predict_export.py --kernel-only 200     # a run of its own
    python tools/bench_predict_export.py --kernel-stats DIR/.../*_kernel_stats.csv --out profiles/predict_export.txt  # appends
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

ALL_PANELS = ("rgb", "est", "gt", "err")


def rss_mb():
    with open("/proc/self/statm") as fh:
        return int(fh.read().split()[1]) * os.sysconf("SC_PAGE_SIZE") / 2 ** 20


def kernel_stats(path, h, w):
    """The export kernel's rows of a rocprofv3 ``*_kernel_stats.csv`` against its algorithmic bytes."""
    lines = []
    for r in csv.DictReader(open(path)):
        if "depth_export_kernel" not in r["Name"]:
            continue
        avg_us = float(r["AverageNs"]) / 1e3
        lines.append(f"depth_export_kernel: {r['Calls']} calls, average {avg_us:.2f} us, min {float(r['MinNs']) / 1e3:.2f} us, "
                     f"max {float(r['MaxNs']) / 1e3:.2f} us (rocprofv3 --kernel-trace --stats, a run of its own: kitti16, no panels)")
        lines.append(f"  algorithmic bytes at {h}x{w}: 4 B read + 2 B written per pixel = {6 * h * w / 1e6:.2f} MB -> "
                     f"{6 * h * w / 1e3 / avg_us:.1f} GB/s at the average duration")
    return lines or ["depth_export_kernel: not found in " + path]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--levels", type=int, default=6)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--slots", type=int, default=4)
    ap.add_argument("--forms", default="list,dry,kitti16,panels")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", type=int, default=0, metavar="N",
                    help="launch the export kernel (kitti16, no panels) N times and exit (for a rocprofv3 run)")
    ap.add_argument("--kernel-stats", default=None, metavar="CSV", help="append the export kernel's rows of a rocprofv3 stats file")
    a = ap.parse_args()

    if a.kernel_stats is not None:
        lines = kernel_stats(a.kernel_stats, a.height, a.width)
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
    samples, cam = S.make_sequence(1, 8, a.height, a.width, seed=7, motion="lateral")
    cam_d = {k: torch.from_numpy(v).to(dev) for k, v in cam.items()}
    frames = [{"RGB_im": torch.from_numpy(s["RGB_im"]).to(dev), "depth": torch.from_numpy(s["depth"]).to(dev),
               "rot": torch.from_numpy(s["rot"]).to(dev), "trans": torch.from_numpy(s["trans"]).to(dev),
               "new_traj": torch.tensor([False]), "camera": cam_d} for s in samples]

    if a.kernel_only:
        f = frames[0]
        for i in range(a.kernel_only):
            nops.depth_export(f["depth"], "kitti16")
        torch.cuda.synchronize()
        return 0

    model = M.M4Depth(nbre_levels=a.levels)
    model.load_numpy_weights(S.init_weights(a.levels, seed=42), dev)
    first = MAIN._stream_frame(dict(frames[0], new_traj=torch.tensor([True])), dev)
    runner = net.GraphedStream(model, first)
    predict = lambda f: runner(MAIN._stream_frame(f, dev))["depth"]          # noqa: E731  (main.py's predict(), --stream --graph)
    tmp = tempfile.mkdtemp(prefix="m4d_export_bench_")
    rss = []

    def run(form):
        n_total = a.warmup + a.frames
        t0 = None
        if form == "list":
            preds = []
            for i in range(n_total):
                if i == a.warmup:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                preds.append(predict(frames[i % 8]).cpu().numpy())
            dt = time.perf_counter() - t0
            del preds
            return a.frames / dt
        panels = ALL_PANELS if form == "panels" else ()
        out = os.path.join(tmp, form)
        writer = PredictionWriter(out, "kitti16", panels, slots=a.slots, threads=a.threads, encode=form != "dry")
        namer = FrameNamer(1)
        for i in range(n_total):
            if i == a.warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            f = frames[i % 8]
            writer.submit(predict(f), namer(f["new_traj"]), gt=f["depth"] if panels else None, rgb=f["RGB_im"] if panels else None)
            if form == "kitti16" and i in (a.warmup + a.frames // 4, a.warmup + a.frames // 2, n_total - 1):
                rss.append((i - a.warmup + 1, rss_mb()))
        writer.close()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        shutil.rmtree(out, ignore_errors=True)
        return a.frames / dt

    forms = a.forms.split(",")
    fps = {f: [] for f in forms}
    try:
        for _ in range(a.runs):
            for f in forms:
                fps[f].append(run(f))
                print(f"{f}: {fps[f][-1]:.1f} frames/s", flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

    label = {"list": "(a) list    .cpu().numpy() per frame, all kept", "dry": "(b) dry     writer, encode=False",
             "kitti16": f"(c) kitti16 writer, depth PNGs, {a.threads} threads", "panels": f"(d) panels  writer, depth + 4-panel PNGs, {a.threads} threads"}
    lines = [f"predict loop, --stream --graph, synthetic {a.height}x{a.width}, {a.levels} levels, batch 1; {a.frames} frames per run "
             f"after {a.warmup} warm-up frames, {a.runs} runs per form, interleaved; frames/s by the host clock, close() included;",
             f"writer: slots {a.slots}, threads {a.threads}, compress_level 1; {os.cpu_count()} CPUs visible, "
             f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}", ""]
    for f in forms:
        v = fps[f]
        lines.append(f"{label[f]:58s} runs {', '.join(f'{x:7.1f}' for x in v)}   median {np.median(v):7.1f}   spread {max(v) - min(v):5.1f}")
    if "list" in fps and "dry" in fps:
        spread = max(fps["list"]) - min(fps["list"])
        ok = np.median(fps["dry"]) >= np.median(fps["list"]) - spread
        lines += ["", f"required: (b) not below (a) by more than (a)'s run-to-run spread ({spread:.1f} frames/s): "
                      f"{np.median(fps['dry']):.1f} vs {np.median(fps['list']):.1f} -> {'met' if ok else 'NOT MET'}"]
    if rss:
        lines += ["", "resident set size of the process during (c), MB after N timed frames (it must not grow with N): "
                  + "; ".join(f"{n}: {m:.0f}" for n, m in rss)]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
