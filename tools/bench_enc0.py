"""Encoder level 0 (RGB -> conv 3->16 -> DomainNormalization -> leaky_relu -> conv 16->16 stride 2, no full-resolution
intermediate) as the step launches it: the statistics of all `--stats-frames` frames (enc0_stats_kernel<2> +
enc0_moments_finalize_kernel), then the fused pass (enc0_fused_kernel) on one encoder batch of `--frames` frames with those
statistics.  Each part is graph-replayed on its own: us per call by HIP events.  Run under
`rocprofv3 --kernel-trace --stats` for the durations of the three launches one by one (the event time of the statistics
part is the sum of its two)."""
import argparse, os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import m4depth_amd as M
from m4depth_amd import synthetic as S, network_ops as nops
ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=2); ap.add_argument("--stats-frames", type=int, default=4)
ap.add_argument("--iters", type=int, default=50)
a = ap.parse_args()
dev = torch.device("cuda:0")
model = M.M4Depth(nbre_levels=6); model.load_numpy_weights(S.init_weights(6, seed=42), dev)
n = max(a.frames, a.stats_frames)
img = torch.rand(n, 384, 1280, 3, device=dev)
enc = model.encoder
c1, c2, dn = enc.conv_layers_s1[0], enc.conv_layers_s2[0], enc.dn_layers[0]
w1, w2 = c1.packed("hwio"), c2.packed("hwio")
mean, var = nops.encoder_level0_stats(img[:a.stats_frames], w1, c1.bias)
st = (mean[:a.frames].contiguous(), var[:a.frames].contiguous())
parts = [(f"statistics, {a.stats_frames} frames (2 launches)", lambda: nops.encoder_level0_stats(img[:a.stats_frames], w1, c1.bias)),
         (f"fused pass, {a.frames} frames (1 launch)", lambda: nops.encoder_level0(img[:a.frames], w1, c1.bias, dn.scale, dn.bias, w2, c2.bias, 0.1, stats=st)),
         (f"m4d_enc_level0_fwd, {a.frames} frames (3 launches)", lambda: nops.encoder_level0(img[:a.frames], w1, c1.bias, dn.scale, dn.bias, w2, c2.bias, 0.1))]
for what, fn in parts:
    for _ in range(3): fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(a.iters): fn()
    g.replay(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
    print(f"encoder level 0 at 384x1280, {what}: {e0.elapsed_time(e1) * 1e3 / a.iters:.1f} us per call")
