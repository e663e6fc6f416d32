"""Records what a chain of fp16 two-term Winograd layers (m4d_conv3x3_winof16_bias_act_ks, csrc/m4d_wino_f16.hip: every layer
scans its own halo for the per-pixel maxima) computes on seeded inputs, as tests/golden/wino_f16_chain_parent.npz: ``out``
[2,20,36,32], the last layer's output of the chain 64 -> 128 -> 96 -> 64 -> 32 on a [2,20,36] map.  tests/test_gpu_wino_handover.py
holds the scanning path of every later library to these bits, and the path on which a layer takes the maxima from its producer
to the scanning path.

Run on the GPU with the library whose results are the reference:   python tools/gen_wino_handover_golden.py [--out PATH]
The inputs are regenerated from the seeds below by the test; only the result is stored."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F = np.float32
CHAIN = (64, 128, 96, 64, 32)                  # the refiner's widths from conv1's output on: conv2 .. conv5
MAPS = ((2, 20, 36), (1, 5, 7), (1, 33, 17))   # every one ragged against the 16x16 tile
GOLDEN_MAP = MAPS[0]
SLOPE = 0.1


def chain_weights(widths=CHAIN, seed=77):
    """[(kernel [3,3,cin,cout], bias [cout])] of the chain's layers, He-normal, float32 numpy."""
    rng = np.random.default_rng(seed)
    layers = []
    for cin, cout in zip(widths[:-1], widths[1:]):
        k = (rng.standard_normal([3, 3, cin, cout]) * np.sqrt(2.0 / (9 * cin))).astype(F)
        layers.append((k, (0.1 * rng.standard_normal([cout])).astype(F)))
    return layers


def chain_input(shape, cin=CHAIN[0]):
    """The first layer's input [b,h,w,cin] of a map, float32 numpy."""
    b, h, w = shape
    return np.random.default_rng(1000 * h + w).standard_normal([b, h, w, cin]).astype(F)


def pack_chain(layers, dev):
    """[(packed weights, bias, cout, cout_pad)] on the device."""
    import torch
    from m4depth_amd import network_ops as nops
    packed = []
    for k, bias in layers:
        wu, cpad = nops.pack_conv_weights_winof16(k)
        packed.append((torch.from_numpy(wu.view(np.int16)).to(dev), torch.from_numpy(bias).to(dev), k.shape[3], cpad))
    return packed


def run_chain(xd, packed, handover=False):
    """Every layer's output [b,h,w,cout] (device tensors).  ``handover``: every layer but the last writes its pixel maxima and
    the next one reads them instead of scanning its halo; otherwise every layer scans (the only form an older library has)."""
    from m4depth_amd import network_ops as nops
    outs, x = [], xd
    for i, (wd, bd, cout, cpad) in enumerate(packed):
        if handover:
            x = nops.conv3x3_winof16_bias_act(x, wd, bd, cout, cpad, SLOPE, want_maxima=i + 1 < len(packed))
            outs.append(x.tensor if isinstance(x, nops.ActMaxima) else x)
        else:
            x = nops.conv3x3_winof16_bias_act(x, wd, bd, cout, cpad, SLOPE)
            outs.append(x)
    return outs


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "wino_f16_chain_parent.npz"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    packed = pack_chain(chain_weights(), dev)
    xd = torch.from_numpy(chain_input(GOLDEN_MAP)).to(dev)
    out = run_chain(xd, packed)[-1]
    again = run_chain(xd, packed)[-1]
    assert torch.equal(out.view(torch.int32), again.view(torch.int32)), "not run-to-run identical"
    print(f"chain {' -> '.join(map(str, CHAIN))} on {GOLDEN_MAP}: out {tuple(out.shape)}, |out| max {float(out.abs().max()):.4f}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, out=out.cpu().numpy())
    print(f"wrote {a.out} ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
