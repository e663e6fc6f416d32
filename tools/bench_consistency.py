"""What the reprojection-consistency score costs: the fused launch pair (m4d_consistency_per_sample) against the existing
composition m4d_photo_warp_fwd + m4d_photo_loss_fwd on the same frames, and main.py --eval_streams 8 --graph with and without
--consistency.

    python tools/bench_consistency.py [--out profiles/consistency_eval.txt] [--rounds 9] [--calls 200] [--window 0.3] [--no_driver]

Method (that of tools/bench_recording_decode.py): ``calls`` steps of ONE variant are captured into a hipGraph (the entry points
are plain launches), so the host's enqueue time is out of the picture; a timed window is as many replays of that graph as fill
``window`` seconds, between two device events, after a warm-up replay.  The two variants alternate inside a round so a drift of
the machine hits both; reported are the median over the rounds and the spread (min .. max) of the time per step.  That time
includes the gaps the graph executor leaves between dependent kernel nodes: two per step for the fused pair, three for the
composition (warp, loss, finish).

The composition is the yardstick from before the score existed, and it computes LESS: no geometric term, no identity error
unless auto-masking is on (it is timed with auto-masking on, which is what makes it evaluate pe(prev, cur) as the score does),
and one sum over the batch instead of a row per sample.  It writes and re-reads warped + dwarp [B,H,W,3] and valid / mask bytes.

The driver figure is main.py's own "sample-frames/s" line on a synthetic Mid-Air-format set (tools/bench_stream_eval.py's
writer), runs alternating, decode and the network included.  Needs a GPU: there is no fallback.
"""
import argparse
import contextlib
import ctypes
import io
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = [(1, 384, 384), (8, 384, 384), (8, 384, 512)]              # (batch, H, W)


def main(argv=None):
    import torch
    from m4depth_amd._lib import lib, check, dptr, stream_ptr, build_info
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consistency_eval.txt"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200, help="steps per captured graph")
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--no_driver", action="store_true", help="skip the main.py --eval_streams runs")
    ap.add_argument("--driver_rounds", type=int, default=3)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_consistency needs a GPU")
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream(device=dev)
    windows = []

    def graph_of(fn):
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
        return g, max(3, int(args.window / max(time.perf_counter() - t0, 1e-5)))

    def timed(item):
        g, replays = item
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(replays):
            g.replay()
        end.record()
        end.synchronize()
        windows.append(start.elapsed_time(end) * 1e-3)
        return start.elapsed_time(end) * 1e3 / (replays * args.calls)      # microseconds per step

    def stats(v):
        return f"median {np.median(v):8.2f} us  (min {np.min(v):8.2f} .. max {np.max(v):8.2f})"

    lines = [f"# tools/bench_consistency.py -- {build_info()}", f"# device: {torch.cuda.get_device_name(0)}",
             f"# {args.rounds} rounds per variant; a window = replays of a hipGraph of {args.calls} steps between device events; "
             "the variants alternate within a round", ""]
    for b, h, w in CASES:
        rng = np.random.default_rng(b * 1000 + w)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
        est, est_prev = t(rng.uniform(4, 12, (b, h, w, 1))), t(rng.uniform(4, 12, (b, h, w, 1)))
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        img = np.stack([0.5 + 0.4 * np.sin(xx / (17 + 5 * c) + yy / 23) for c in range(3)], -1)[None].repeat(b, 0)
        cur, prev = t(img + rng.normal(0, 0.02, img.shape)), t(np.roll(img, 2, axis=2) + rng.normal(0, 0.02, img.shape))
        aa = rng.normal(0.0, 0.01, (b, 3))
        ang = np.linalg.norm(aa, axis=1, keepdims=True)
        rot = t(np.concatenate([np.cos(ang / 2), aa / np.maximum(ang, 1e-12) * np.sin(ang / 2)], axis=1))
        trans = t(rng.normal([0.3, 0.05, 0.1], 0.03, (b, 3)))
        cam_f, cam_c = t(np.tile([[0.5 * w, 0.5 * h]], (b, 1))), t(np.tile([[0.5 * w, 0.5 * h]], (b, 1)))
        zeros, ones = torch.zeros(b, dtype=torch.uint8, device=dev), torch.ones(b, dtype=torch.uint8, device=dev)
        rows, counted = torch.empty((b, 6), device=dev), torch.empty(b, dtype=torch.uint8, device=dev)
        ws = torch.empty(lib.m4d_consistency_workspace_bytes(b, h, w) // 8 + 1, dtype=torch.float64, device=dev)
        warped, dwarp = torch.empty((b, h, w, 3), device=dev), torch.empty((b, h, w, 3), device=dev)
        valid, mask = (torch.empty((b, h, w, 1), dtype=torch.uint8, device=dev) for _ in range(2))
        out4 = torch.empty(4, device=dev)
        ws_p = torch.empty(lib.m4d_photo_workspace_bytes(b, h, w) // 8 + 1, dtype=torch.float64, device=dev)
        p = lambda x: ctypes.c_void_p(x.data_ptr())

        def fused():
            check(lib.m4d_consistency_per_sample(p(est), h * w, p(est_prev), h * w, p(cur), 3 * h * w, p(prev), 3 * h * w, p(rot), 4,
                                                 p(trans), p(cam_f), p(cam_c), p(zeros), p(ones), b, h, w, p(ws), p(rows), p(counted),
                                                 stream_ptr()), "m4d_consistency_per_sample")

        def composition():
            check(lib.m4d_photo_warp_fwd(dptr(est), dptr(rot), 4, dptr(trans), dptr(cam_f), dptr(cam_c), dptr(prev), b, h, w,
                                         dptr(warped), dptr(dwarp), p(valid), stream_ptr()), "m4d_photo_warp_fwd")
            check(lib.m4d_photo_loss_fwd(dptr(est), dptr(warped), p(valid), dptr(cur), dptr(prev), b, h, w, 1e-3, 1, p(ws_p),
                                         dptr(out4), p(mask), stream_ptr()), "m4d_photo_loss_fwd")

        g_f, g_c = graph_of(fused), graph_of(composition)
        torch.cuda.synchronize()
        r = rows.cpu().numpy()
        t_f, t_c = [], []
        for k in range(args.rounds):
            for name in (("f", "c") if k % 2 == 0 else ("c", "f")):
                (t_f if name == "f" else t_c).append(timed(g_f if name == "f" else g_c))
        ratio = np.median(t_f) / np.median(t_c)
        lines.append(f"batch {b}, {h}x{w}  (cover {r[:, 4].mean():.3f}, geo_cover {r[:, 5].mean():.3f}, counted {int(counted.sum())}/{b})")
        lines.append(f"  m4d_consistency_per_sample (2 launches)              {stats(t_f)}")
        lines.append(f"  m4d_photo_warp_fwd + m4d_photo_loss_fwd (3 launches) {stats(t_c)}  fused / composition = {ratio:.2f}")
        lines.append("")
    lines.insert(3, f"# timed windows: {min(windows):.2f} .. {max(windows):.2f} s")

    if not args.no_driver:
        from bench_stream_eval import write_dataset
        from m4depth_amd import main as MAIN
        with tempfile.TemporaryDirectory() as root:
            cfg, rec, lengths = write_dataset(root, 16, 24, 40, (384, 384), seed=1)
            common = ["--mode", "eval", "--dataset", "midair", "--db_path_config", cfg, "--records_path", rec, "--arch_depth", "6",
                      "--height", "384", "--width", "384", "--eval_streams", "8", "--graph"]
            rates = {"without": [], "with": []}
            for k in range(args.driver_rounds):
                for name in (("without", "with") if k % 2 == 0 else ("with", "without")):
                    buf = io.StringIO()
                    with contextlib.redirect_stdout(buf):
                        rc = MAIN.main(common + ["--ckpt_dir", os.path.join(root, f"ck_{name}_{k}")]
                                       + (["--consistency"] if name == "with" else []))
                    assert rc == 0
                    rates[name].append(float(re.search(r"([0-9.]+) sample-frames/s", buf.getvalue()).group(1)))
        lines.append(f"main.py --mode=eval --eval_streams 8 --graph, 384x384, 6 levels, {len(lengths)} trajectories / {sum(lengths)} "
                     f"frames, {args.driver_rounds} runs each, alternating (decode and network included):")
        for name in ("without", "with"):
            v = rates[name]
            lines.append(f"  {name:8s} --consistency   median {np.median(v):8.1f} sample-frames/s  (min {min(v):8.1f} .. max {max(v):8.1f})")
        lines.append(f"  with / without = {np.median(rates['with']) / np.median(rates['without']):.3f}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
