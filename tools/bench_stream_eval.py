"""Streaming evaluation throughput on a Mid-Air-format dataset (main.py --mode=eval without --db_seq_len).

On the CPU, before any GPU work, writes a dataset in the on-disk format of the Mid-Air loader (JPEG colour frames, float16
disparity PNGs, tab-separated trajectory csv files) at the Mid-Air eval geometry, 384x384: ``--n_traj`` trajectories of
40-160 frames.  Then times, each in a child process of its own under its own time limit:

  seq        today's one-frame-at-a-time loop (``main.py --mode=eval``: eager test_step at batch 1, one prefetch thread),
             as a whole run and, timed from its second frame, in a child of this script;
  slots      ``main.py --mode=eval --eval_streams B`` for each B of ``--slots``, eager and with ``--graph``;
  decode     the slot loader alone (host decompression + device decode, no network): the input rate at B slots;
  gpu        the --eval_streams loop on frames decoded on the device beforehand: the GPU-only rate at B slots.

Every child prints its wall time and rate; the table goes to stdout and to ``--out`` (a text file).  Random seeded weights
(no checkpoint): the timing does not depend on them.

    python tools/bench_stream_eval.py --slots 8,32 --out profiles/r08_stream_eval.txt
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def write_dataset(root, n_traj, lo, hi, size, seed=0, workers=8):
    """Mid-Air-format trajectories of lo..hi frames; smooth images (compress and decode like real frames, unlike noise)."""
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    rng = np.random.default_rng(seed)
    h, w = size
    lengths = rng.integers(lo, hi + 1, size=n_traj).tolist()
    db, rec = os.path.join(root, "db"), os.path.join(root, "records")
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)

    def frame(t, i):
        r = np.random.default_rng([seed, t, i])
        ph = r.uniform(0, 6.3, 3)
        img = np.stack([127 + 100 * np.sin(xx / (17 + 5 * c) + yy / 23 + ph[c] + 0.05 * i) for c in range(3)], -1)
        img = np.clip(img + r.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(db, f"traj_{t}", "color", f"{i:06d}.JPEG"), format="JPEG", quality=95)
        depth = (20 + 15 * np.sin(xx / 40 + ph[0]) * np.cos(yy / 50 + 0.02 * i) + r.uniform(0, 1, (h, w))).astype(np.float32)
        bits = (np.float32(512.0) / depth).astype(np.float16).view(np.uint16)
        Image.fromarray(bits).save(os.path.join(db, f"traj_{t}", "gt", f"{i:06d}.PNG"), format="PNG")

    jobs = []
    for t, n in enumerate(lengths):
        for sub in ("color", "gt"):
            os.makedirs(os.path.join(db, f"traj_{t}", sub), exist_ok=True)
        os.makedirs(os.path.join(rec, f"set_{t}"), exist_ok=True)
        lines = ["\t".join(["id", "camera_l", "disp", "qw", "qx", "qy", "qz", "tx", "ty", "tz"])]
        for i in range(n):
            aa = rng.normal(0.0, 0.01, 3)
            ang = np.linalg.norm(aa)
            q = np.concatenate([[np.cos(ang / 2)], aa / max(ang, 1e-12) * np.sin(ang / 2)])
            tr = rng.normal([0.0, 0.0, 0.3], 0.05, 3)
            lines.append("\t".join([str(i), f"traj_{t}/color/{i:06d}.JPEG", f"traj_{t}/gt/{i:06d}.PNG"]
                                   + [repr(float(v)) for v in np.concatenate([q, tr])]))
            jobs.append((t, i))
        with open(os.path.join(rec, f"set_{t}", f"traj_{t:04d}.csv"), "w") as fh:
            fh.write("\n".join(lines) + "\n")
    with ThreadPoolExecutor(max_workers=workers) as pool:
        list(pool.map(lambda j: frame(*j), jobs))
    cfg = os.path.join(root, "datasets_location.json")
    with open(cfg, "w") as fh:
        json.dump({"midair": db}, fh)
    return cfg, rec, lengths


# ---- children --------------------------------------------------------------------------------------------------------------
def _loader(cfg, rec, slots, dev):
    from m4depth_amd import dataloaders as dl
    roots = json.load(open(cfg))
    settings = dl.DataloaderParameters(roots, rec, None, 4, False)
    return dl.get_loader("midair").get_dataset("eval_streams", settings, batch_size=slots, device=dev)


def child_seq(cfg, rec, arch_depth):
    """Today's loop (main.py --mode=eval without --db_seq_len) timed from its second frame: eager test_step at batch 1 on the
    batch-1 streaming plan (one prefetch thread decoding one frame at a time)."""
    import torch
    import m4depth_amd as M
    from m4depth_amd import dataloaders as dl
    from m4depth_amd import synthetic as S
    from m4depth_amd.metrics import default_metrics
    dev = torch.device("cuda:0")
    settings = dl.DataloaderParameters(json.load(open(cfg)), rec, None, 4, False)
    ds = dl.get_loader("midair").get_dataset("eval", settings, batch_size=1, device=dev)
    model = M.M4Depth(nbre_levels=arch_depth)
    model.load_numpy_weights(S.init_weights(arch_depth, seed=42), dev)
    model.compile(metrics=default_metrics())
    t0, n = None, 0
    for i, data in enumerate(ds):
        if i == 1:
            torch.cuda.synchronize()
            t0, n = time.perf_counter(), 0
        model.test_step(data)
        n += 1
    torch.cuda.synchronize()
    print(f"RESULT seq: {n / (time.perf_counter() - t0):.1f} frames/s")


def child_decode(cfg, rec, slots):
    import torch
    dev = torch.device("cuda:0")
    ds = _loader(cfg, rec, slots, dev)
    act = (ds.schedule.cells[..., 0] >= 0).sum(axis=1)
    t0 = None
    for step, _ in enumerate(ds):
        if step == 1:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"RESULT decode {slots} slots: {int(act[1:].sum()) / dt:.1f} sample-frames/s")


def child_gpu(cfg, rec, slots, graph, arch_depth):
    """The --eval_streams loop (main.eval_streams) on steps decoded on the device beforehand."""
    import torch
    import m4depth_amd as M
    from m4depth_amd import network_ops as nops
    from m4depth_amd import synthetic as S
    dev = torch.device("cuda:0")
    ds = _loader(cfg, rec, slots, dev)
    steps = list(ds)
    torch.cuda.synchronize()
    model = M.M4Depth(nbre_levels=arch_depth)
    model.load_numpy_weights(S.init_weights(arch_depth, seed=42), dev)
    n_steps, B = ds.schedule.cells.shape[:2]
    act = (ds.schedule.cells[..., 0] >= 0).sum(axis=1)
    rows = torch.empty((n_steps, B, 7), dtype=torch.float32, device=dev)
    counted = torch.empty((n_steps, B), dtype=torch.uint8, device=dev)
    runner, t0 = None, None
    for step, batch in enumerate(steps):
        if step == 1:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        frame = {"RGB_im": batch["RGB_im"], "rot": batch["rot"], "trans": batch["trans"], "new_traj": batch["reset"],
                 "camera": batch["camera"]}
        if graph:
            if runner is None:
                from m4depth_amd.network import GraphedStream
                runner = GraphedStream(model, frame)
            est = runner(frame)["depth"]
        else:
            est = model.stream_step(frame)["depth"]
        nops.depth_metrics_per_sample(batch["depth"], est, batch["new_traj"], batch["active"], 80., rows=rows[step],
                                      counted=counted[step])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"RESULT gpu {slots} slots {'graph' if graph else 'eager'}: {int(act[1:].sum()) / dt:.1f} sample-frames/s")


# ---- parent ------------------------------------------------------------------------------------------------------------
def run(cmd, limit, env):
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    dt = time.perf_counter() - t0
    out = p.stdout + p.stderr
    if p.returncode != 0:
        print(out[-3000:])
        raise SystemExit(f"child failed with exit status {p.returncode}: {' '.join(cmd)}")
    return out, dt


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n_traj", type=int, default=24)
    ap.add_argument("--min_len", type=int, default=40)
    ap.add_argument("--max_len", type=int, default=160)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--arch_depth", type=int, default=6)
    ap.add_argument("--slots", default="8,32")
    ap.add_argument("--data", default=None, help="dataset directory (default: a fresh one under /tmp)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=300, help="time limit of one child, seconds")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--graph", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    data = a.data or os.path.join("/tmp", f"m4d_stream_eval_{os.getpid()}")
    cfg, rec = os.path.join(data, "datasets_location.json"), os.path.join(data, "records")
    if a.child == "seq":
        return child_seq(cfg, rec, a.arch_depth)
    if a.child == "decode":
        return child_decode(cfg, rec, int(a.slots))
    if a.child == "gpu":
        return child_gpu(cfg, rec, int(a.slots), a.graph, a.arch_depth)

    t0 = time.perf_counter()
    cfg, rec, lengths = write_dataset(data, a.n_traj, a.min_len, a.max_len, (a.size, a.size))
    n_frames = sum(lengths)
    lines = [f"dataset: {a.n_traj} Mid-Air-format trajectories, {n_frames} frames of {a.size}x{a.size} (lengths {lengths}), "
             f"written in {time.perf_counter() - t0:.1f} s; {a.arch_depth} levels, seeded random weights"]
    env = dict(os.environ)
    main_argv = [sys.executable, "-m", "m4depth_amd.main", "--mode=eval", "--dataset=midair", "--db_path_config", cfg,
                 "--records_path", rec, "--arch_depth", str(a.arch_depth), "--height", str(a.size), "--width", str(a.size)]
    me = [sys.executable, os.path.abspath(__file__), "--data", data, "--arch_depth", str(a.arch_depth)]
    rows = []

    def record(name, out, dt, pattern=None):
        m = re.search(pattern, out) if pattern else None
        rate = float(m.group(1)) if m else float("nan")
        rows.append((name, rate, n_frames / dt, dt))
        print(f"{name:<34} loop {rate:10.1f}   frames / wall {n_frames / dt:8.1f}   wall {dt:7.1f} s", flush=True)

    out, dt = run(main_argv + ["--ckpt_dir", os.path.join(data, "ck_seq")], a.limit, env)
    record("main.py, batch 1 (today)", out, dt)
    out, dt = run(me + ["--child", "seq"], a.limit, env)
    record("batch-1 loop alone (today)", out, dt, r"RESULT seq: ([0-9.]+)")
    from m4depth_amd.stream_eval import schedule
    for B in [int(s) for s in a.slots.split(",")]:
        sch = schedule(lengths, B, "lpt")
        n_steps, Be = sch.cells.shape[:2]
        lines.append(f"{B} slots (lpt): effective B {Be}, {n_steps} steps, {n_frames / (n_steps * Be):.3f} of the "
                     f"{n_steps * Be} sample-cells active")
        for graph in (False, True):
            tag = "graph" if graph else "eager"
            out, dt = run(main_argv + ["--eval_streams", str(B), "--ckpt_dir", os.path.join(data, f"ck_{B}_{tag}")]
                          + (["--graph"] if graph else []), a.limit, env)
            record(f"--eval_streams {B} {tag}", out, dt, r"([0-9.]+) sample-frames/s")
        out, dt = run(me + ["--child", "decode", "--slots", str(B)], a.limit, env)
        record(f"decode only, {B} slots", out, dt, r"RESULT decode .*: ([0-9.]+)")
        for graph in (False, True):
            out, dt = run(me + ["--child", "gpu", "--slots", str(B)] + (["--graph"] if graph else []), a.limit, env)
            record(f"gpu only, {B} slots {'graph' if graph else 'eager'}", out, dt, r"RESULT gpu .*: ([0-9.]+)")
    lines.append("loop = active sample-frames per second of the timed loop, the first step excluded (main.py's batch-1 loop "
                 "prints none: 'batch-1 loop alone' times it); "
                 "frames / wall = all frames over the child's wall time, start-up (imports, weights, graph capture, and for "
                 "'gpu only' the decode of the whole set beforehand) included")
    lines += [f"{n:<34} loop {r:10.1f} frames/s   frames / wall {fw:8.1f}   child wall {d:7.1f} s" for n, r, fw, d in rows]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    if a.data is None:
        import shutil
        shutil.rmtree(data, ignore_errors=True)


if __name__ == "__main__":
    main()
