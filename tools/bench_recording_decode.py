"""What undistortion costs next to the plain resize: m4d_decode_rgb8_remap against m4d_decode_rgb8_resize on the same frames,
the one-off m4d_undistort_map, and the equidistant table's distance from its float64 restatement.

    python tools/bench_recording_decode.py [--out profiles/recording_decode.txt] [--rounds 9] [--calls 500] [--window 0.3]

Method: ``calls`` launches of ONE kernel are captured into a hipGraph (the entry points are plain launches), so the host's
enqueue time per launch (about 7 us through ctypes, more than these kernels take at batch 1) is out of the picture; a timed
window is as many replays of that graph as fill ``window`` seconds, between two device events, after a warm-up replay.  The
two kernels alternate inside a round so a drift of the machine hits both; reported are the median over the rounds and the
spread (min .. max) of the time per launch.  That time includes the gap the graph executor leaves between two dependent
kernel nodes, which is the same for both kernels; it is a per-launch cost, not a kernel-trace duration.
Needs a GPU: there is no fallback.
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(480, 752, 384, 512, "radtan"), (1080, 1920, 384, 640, "radtan")]         # EuRoC-sized and full-HD sources
BATCHES = (1, 8)
EUROC = {"fx": 458.654, "fy": 457.296, "cx": 367.715, "cy": 248.875, "distortion": [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0]}


def camera_for(ih, iw):
    """EuRoC cam0's lens scaled to the source size (same field of view, same coefficients)."""
    s = iw / 752.0
    return {"width": iw, "height": ih, "fx": EUROC["fx"] * s, "fy": EUROC["fy"] * s, "cx": EUROC["cx"] * s, "cy": ih / 2.0 + 8.875 * s,
            "model": "radtan", "distortion": EUROC["distortion"], "zoom": 1.0}


def equidistant_table(dist, src_cam, out_cam, oh, ow, T):
    """m4d_undistort_map's equidistant formula (include/m4depth_hip.h) in numpy at precision ``T``, camera numbers rounded to
    float32 first as the entry point takes them; no validity test (the caller's geometry has a source everywhere).  The tool
    stands alone, so this repeats tests/recording_ref.py's undistort_map; tests/test_recording_host.py holds the two equal."""
    f = np.float32
    fx, fy, cx, cy = (T(f(v)) for v in src_cam)
    fxo, fyo, cxo, cyo = (T(f(v)) for v in out_cam)
    k = [T(f(v)) for v in dist]
    col, row = np.meshgrid(np.arange(ow).astype(T), np.arange(oh).astype(T))
    x, y = ((col + T(0.5)) - cxo) / fxo, ((row + T(0.5)) - cyo) / fyo
    r = np.sqrt(x * x + y * y)
    th = np.arctan(r)
    th2 = th * th
    thd = th * (T(1) + th2 * (k[0] + th2 * (k[1] + th2 * (k[2] + th2 * k[3]))))
    s = np.where(r > T(f(1e-8)), thd / np.where(r > 0, r, T(1)), T(1))
    return np.stack([(x * s * fx + cx) - T(0.5), (y * s * fy + cy) - T(0.5)], axis=-1)


def main(argv=None):
    import torch
    from m4depth_amd._lib import lib, check, dptr, stream_ptr, build_info
    from m4depth_amd.dataloaders.recording import output_camera, MODELS
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recording_decode.txt"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=500, help="launches per captured graph")
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_recording_decode needs a GPU")
    dev = torch.device("cuda:0")
    f4 = ctypes.c_float * 4

    side = torch.cuda.Stream(device=dev)

    def graph_of(fn):
        """``calls`` launches of ``fn`` as one graph, and the number of replays that fill a window."""
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
        return start.elapsed_time(end) * 1e3 / (replays * args.calls)      # microseconds per launch

    windows = []                                                   # seconds of every timed window

    def stats(v):
        return f"median {np.median(v):8.2f} us  (min {np.min(v):8.2f} .. max {np.max(v):8.2f})"

    lines = [f"# tools/bench_recording_decode.py -- {build_info()}", f"# device: {torch.cuda.get_device_name(0)}",
             f"# {args.rounds} rounds per kernel; a window = replays of a hipGraph of {args.calls} launches between device events; "
             "kernels alternate within a round",
             ""]
    for ih, iw, oh, ow, model in CASES:
        cam = camera_for(ih, iw)
        out_cam = output_camera(cam, oh, ow)
        dist = (ctypes.c_float * 5)(*cam["distortion"])
        table = torch.empty((oh, ow, 2), dtype=torch.float32, device=dev)

        def build_table():
            check(lib.m4d_undistort_map(MODELS[model], dist, f4(cam["fx"], cam["fy"], cam["cx"], cam["cy"]), f4(*out_cam), ih, iw,
                                        oh, ow, dptr(table), stream_ptr()), "m4d_undistort_map")
        build_table()
        torch.cuda.synchronize()
        none = float((table[..., 0] < -0.5).float().mean())
        g_map = graph_of(build_table)
        t_map = [timed(g_map) for _ in range(args.rounds)]
        lines.append(f"{ih}x{iw} -> {oh}x{ow} ({model}, {100 * none:.1f} % of the table without a source)")
        lines.append(f"  m4d_undistort_map (once per recording)      {stats(t_map)}")
        for n in BATCHES:
            frames = torch.from_numpy(np.random.default_rng(n).integers(0, 256, (n, ih, iw, 3), dtype=np.uint8)).to(dev)
            out_a = torch.empty((n, oh, ow, 3), dtype=torch.float32, device=dev)
            out_b = torch.empty_like(out_a)

            def remap():
                check(lib.m4d_decode_rgb8_remap(dptr(frames, "rgb", torch.uint8), dptr(table), n, ih, iw, oh, ow, dptr(out_a),
                                                stream_ptr()), "m4d_decode_rgb8_remap")

            def resize():
                check(lib.m4d_decode_rgb8_resize(dptr(frames, "rgb", torch.uint8), n, ih, iw, oh, ow, dptr(out_b), stream_ptr()),
                      "m4d_decode_rgb8_resize")
            g_remap, g_resize = graph_of(remap), graph_of(resize)  # each warmed up by its calibration replays
            t_remap, t_resize = [], []
            for r in range(args.rounds):
                order = ("remap", "resize") if r % 2 == 0 else ("resize", "remap")
                for name in order:
                    (t_remap if name == "remap" else t_resize).append(timed(g_remap if name == "remap" else g_resize))
            ratio = np.median(t_remap) / np.median(t_resize)
            lines.append(f"  batch {n}: m4d_decode_rgb8_remap              {stats(t_remap)}")
            lines.append(f"  batch {n}: m4d_decode_rgb8_resize             {stats(t_resize)}  remap / resize = {ratio:.2f}")
        lines.append("")

    # the equidistant table of the test fixture (camera B, 64x64 -> 40x56) against the float64 restatement
    B = {"width": 64, "height": 64, "fx": 23.87225, "fy": 23.871625, "cx": 31.92875, "cy": 32.175,
         "distortion": [0.0034823894, 0.0007150348, -0.0020532361, 0.00020293673]}                # TUM-VI's lens scaled by 1/8
    src = (B["fx"], B["fy"], B["cx"], B["cy"])
    out_cam = output_camera(dict(B, zoom=1.0), 40, 56)
    table = torch.empty((40, 56, 2), dtype=torch.float32, device=dev)
    check(lib.m4d_undistort_map(2, (ctypes.c_float * 4)(*B["distortion"]), f4(*src), f4(*out_cam), 64, 64, 40, 56, dptr(table),
                                stream_ptr()), "m4d_undistort_map")
    got = table.cpu().numpy().astype(np.float64)
    m32, m64 = equidistant_table(B["distortion"], src, out_cam, 40, 56, np.float32), \
        equidistant_table(B["distortion"], src, out_cam, 40, 56, np.float64)
    assert (got[..., 0] >= -0.5).all()                             # every entry has a source at this geometry
    lines.append("equidistant table, the tests' camera B, 64x64 -> 40x56, distance from the float64 evaluation of the header's formula:")
    lines.append(f"  device                      {np.hypot(*np.moveaxis(got - m64, -1, 0)).max():.3e} px")
    lines.append(f"  float32 numpy evaluation    {np.hypot(*np.moveaxis(m32 - m64, -1, 0)).max():.3e} px")
    lines.insert(3, f"# timed windows: {min(windows):.2f} .. {max(windows):.2f} s")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
