"""Records what the level-0 head of the encoder (m4d_enc_level0_stats: enc0_stats_kernel<2> + enc0_moments_finalize_kernel;
m4d_enc_level0_fwd: the two + enc0_fused_kernel) computes on seeded inputs, as tests/golden/enc0_head_parent.npz: per case
``<name>.mean``, ``<name>.var`` [b,16] and ``<name>.out`` [b,ceil(h/2),ceil(w/2),16].  tests/test_gpu_enc0_head.py holds every
later library to these bits (the kernels may move data and schedule instructions differently; their arithmetic is fixed).

Run on the GPU with the library whose results are the reference:   python tools/gen_enc0_head_golden.py [--out PATH]
The inputs are regenerated from the seeds below by the test; only the results are stored."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F = np.float32
# name: (b, h, w, weights); "init12" = the level-0 layers of synthetic.init_weights(seed=12), "he" = He-normal with biases
CASES = {
    "b1_5x7": (1, 5, 7, "he"),             # smaller than a tile in both directions
    "b2_9x129": (2, 9, 129, "he"),         # one tile + one row and one column; rows start off 16-byte alignment; also a FrameStack
    "b1_37x53": (1, 37, 53, "init12"),     # odd sizes: TF 'SAME' pads top / left too
    "b3_16x130": (3, 16, 130, "he"),
}
FRAMESTACK_CASE = "b2_9x129"


def case_inputs(name):
    """(img [b,h,w,3], k1 [3,3,3,16], b1, dn_scale, dn_bias, k2 [3,3,16,16], b2) of a case, float32 numpy."""
    b, h, w, kind = CASES[name]
    rng = np.random.default_rng(1000 * h + w)
    img = rng.random([b, h, w, 3]).astype(F)
    if kind == "init12":
        from m4depth_amd import synthetic as S
        W = S.init_weights(1, seed=12)
        return (img, W["enc.s1.0.kernel"], W["enc.s1.0.bias"], W["enc.dn.0.scale"], W["enc.dn.0.bias"],
                W["enc.s2.0.kernel"], W["enc.s2.0.bias"])
    k1 = (rng.standard_normal([3, 3, 3, 16]) * np.sqrt(2.0 / 27)).astype(F)
    b1 = (0.1 * rng.standard_normal([16])).astype(F)
    k2 = (rng.standard_normal([3, 3, 16, 16]) * np.sqrt(2.0 / 144)).astype(F)
    b2 = (0.1 * rng.standard_normal([16])).astype(F)
    sc = (1.0 + 0.1 * rng.standard_normal([16])).astype(F)
    bs = (0.1 * rng.standard_normal([16])).astype(F)
    return img, k1, b1, sc, bs, k2, b2


def run_case(name, dev):
    """(mean, var, out) device tensors of a case through network_ops (dense batch)."""
    import torch
    from m4depth_amd import network_ops as nops
    img, *wts = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in case_inputs(name)]
    mean, var = nops.encoder_level0_stats(img, wts[0], wts[1])
    out = nops.encoder_level0(img, *wts, 0.1)
    return mean, var, out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "enc0_head_parent.npz"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rec = {}
    for name in CASES:
        mean, var, out = run_case(name, dev)
        m2, v2, o2 = run_case(name, dev)
        assert torch.equal(mean, m2) and torch.equal(var, v2) and torch.equal(out, o2), f"{name}: not run-to-run identical"
        rec[name + ".mean"], rec[name + ".var"], rec[name + ".out"] = (t.cpu().numpy() for t in (mean, var, out))
        print(f"{name}: mean {tuple(mean.shape)}, out {tuple(out.shape)}, |out| max {float(out.abs().max()):.4f}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **rec)
    print(f"wrote {a.out} ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
