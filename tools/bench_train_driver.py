"""Training-driver throughput on the MI355X: ``m4depth_amd.main --mode=train`` eager vs ``--graph`` at the reference's
training geometry (384x384, batch 3, seq_len 4: scripts/1a-train-midair.sh) on synthetic data.  The batches are generated
once and kept on the device (the synthetic generator runs on the host and would otherwise be timed), so the rates are the
driver's own: the steps, the step log and its reads.  The driver times the steps after its first one (the eager warm-up /
capture).  Prints one JSON line.

    python tools/bench_train_driver.py --steps 40 [--modes graph] [--summary_interval 20]
"""
import argparse
import json
import os
import re
import sys
import tempfile
from contextlib import redirect_stdout
from io import StringIO

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=384)
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--seq_len", type=int, default=4)
    ap.add_argument("--levels", type=int, default=6)
    ap.add_argument("--steps", type=int, default=40, help="driver steps per mode (the first one is not timed)")
    ap.add_argument("--distinct", type=int, default=4, help="distinct device-resident batches, cycled")
    ap.add_argument("--summary_interval", type=int, default=20)
    ap.add_argument("--modes", default="eager,graph")
    args = ap.parse_args()
    from m4depth_amd import main as MAIN, synthetic as S
    dev = torch.device("cuda:0")
    batches = []
    for i in range(args.distinct):
        samples, cam = S.make_sequence(args.batch, args.seq_len, args.height, args.width, seed=1 + i)
        d = {k: torch.from_numpy(np.stack([s[k] for s in samples], axis=1)).to(dev) for k in ("depth", "RGB_im", "rot", "trans")}
        d["new_traj"] = torch.from_numpy(np.stack([s["new_traj"] for s in samples], axis=1))
        d["camera"] = {k: torch.from_numpy(v).to(dev) for k, v in cam.items()}
        batches.append(d)
    MAIN.default_epochs = lambda a, rank, world, dev_: (1, lambda e: (batches[i % len(batches)] for i in range(args.steps)))
    result = {"metric": "train driver steps/s",
              "config": f"{args.height}x{args.width} L={args.levels} batch {args.batch} seq_len {args.seq_len}, synthetic, "
                        f"{args.steps} steps, summary_interval {args.summary_interval}"}
    for mode in args.modes.split(","):
        with tempfile.TemporaryDirectory() as ck:
            argv = ["--mode", "train", "--arch_depth", str(args.levels), "--height", str(args.height), "--width", str(args.width),
                    "--batch_size", str(args.batch), "--seq_len", str(args.seq_len), "--ckpt_dir", ck,
                    "--summary_interval", str(args.summary_interval)] + (["--graph"] if mode == "graph" else [])
            buf = StringIO()
            with redirect_stdout(buf):
                rc = MAIN.main(argv)
            out = buf.getvalue()
        rate = re.search(r"^train \((\w+)\): ([\d.]+) steps/s over (\d+) steps", out, re.M)
        losses = [float(x) for x in re.findall(r"^step \d+: loss (\S+)", out, re.M)]
        if rc != 0 or rate is None:
            raise SystemExit(f"{mode}: driver returned {rc}\n{out[-2000:]}")
        sps = float(rate.group(2))
        result[mode] = {"steps_per_s": sps, "ms_per_step": round(1e3 / sps, 2), "timed_steps": int(rate.group(3)),
                        "loss_first": losses[0], "loss_last": losses[-1], "steps_logged": len(losses)}
        torch.cuda.synchronize()
    result["peak_mem_GB"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
