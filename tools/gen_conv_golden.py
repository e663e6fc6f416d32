"""Bit-level golden values of the direct and the fp32 Winograd convolutions: one sha256 of the output bytes per case, stored in
tests/golden/conv_golden.json and compared by tests/test_gpu_conv_golden.py.  The tolerance tests of these kernels cannot see a
change of summation order or a dropped term; this one sees any change of any output bit.

    python tools/gen_conv_golden.py            prints kernel instantiation and digest of every case
    python tools/gen_conv_golden.py --write    ... and rewrites the JSON (only after a change that is MEANT to move bits;
                                               --write PATH writes elsewhere)

Inputs are seeded normals, batch 2.  Every case names the kernel instantiation the library's dispatch puts it on (the rules of
csrc/m4d_conv.hip and csrc/m4d_wino.hip, restated in kernel_of): the small maps run the narrow direct kernel whatever Cout is,
so the wide ones (2, 3, 4 N-tiles per workgroup) have cases on a 128x256 output map, and the three-workgroups-per-CU form of
the widest one a case of 3072 workgroups."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_golden.json")
B, SLOPE = 2, 0.1


def _direct(cin, cout, stride, h, w, ws=False):
    return dict(entry="m4d_conv3x3s_bias_act_ws", cin=cin, cout=cout, stride=stride, h=h, w=w, ws=ws)


CASES = (
    # Cin 32 = two K chunks (the re-staging branch runs); 9x17 = one ragged tile, 24x40 = 3x3 ragged tiles (stride 2: of the output)
    [_direct(32, cout, stride, h, w) for cout in (32, 64, 128) for stride in (1, 2) for (h, w) in ((9, 17), (24, 40))]
    + [_direct(256, 64, 1, 6, 10, ws=True)]                                           # split-K through the workspace
    # the wide kernels: 256 output tiles x 2 images = 512 workgroups of 2 / 3 / 4 N-tiles
    + [_direct(32, cout, stride, 128 * stride, 256 * stride) for cout in (64, 96, 128) for stride in (1, 2)]
    + [_direct(32, 128, 1, 256, 768)]                                                 # 3072 workgroups: 3 per CU
    + [dict(entry="m4d_conv3x3s_small_bias_act", cin=32, cout=64, stride=1, h=9, w=17),
       dict(entry="m4d_conv3x3s2_dinl_bias_act", cin=16, cout=16, stride=2, h=18, w=34)]
    # 24x40 = 9 tiles in plain order, 32x64 = 16 tiles in the XCD order; Cout 96 = 1 N-tile per workgroup, 64 = 2
    + [dict(entry="m4d_conv3x3_wino_bias_act", cin=32, cout=cout, stride=1, h=h, w=w) for cout in (96, 64) for (h, w) in ((24, 40), (32, 64))]
    + [dict(entry="m4d_conv3x3_wino2_bias_act", cin=32, cout=64, stride=1, h=32, w=48)]
)


def case_id(c):
    return f"{c['entry'][4:]}-cin{c['cin']}-cout{c['cout']}-s{c['stride']}-{c['h']}x{c['w']}" + ("-ws" if c.get("ws") else "")


def kernel_of(c):
    """The kernel instantiation the library's dispatch runs the case on."""
    e, s = c["entry"], c["stride"]
    if e == "m4d_conv3x3s_small_bias_act":
        return f"conv3x3_small_kernel<{s}>"
    if e == "m4d_conv3x3s2_dinl_bias_act":
        return "conv3x3_mfma_kernel<1, 9, 2, false, 2, true>"
    cpad = -(-c["cout"] // 32) * 32
    n32 = cpad // 32
    if e == "m4d_conv3x3_wino_bias_act":
        tiles = -(-c["w"] // 16) * -(-c["h"] // 8)
        return f"conv3x3_wino_kernel<{2 if n32 % 2 == 0 else 1}> ({'XCD' if tiles % 8 == 0 else 'plain'} order)"
    if e == "m4d_conv3x3_wino2_bias_act":
        from m4depth_amd import _lib
        sw = _lib.switches()
        wgs = -(-c["w"] // 16) * -(-c["h"] // 16) * (cpad // 64) * B
        four = sw["wino_variant"] == 4 and cpad % 64 == 0 and c["cin"] >= 32 and c["cin"] % 8 == 0 and wgs >= sw["wino4_min_wg"]
        return "conv3x3_wino4_kernel<false>" if four else "conv3x3_wino2_kernel"
    oh, ow = -(-c["h"] // s), -(-c["w"] // s)
    tiles = -(-ow // 16) * -(-oh // 8)
    nt = 4 if n32 >= 4 and n32 % 4 == 0 else 3 if n32 % 3 == 0 else 2 if n32 % 2 == 0 else 1
    while nt > 1 and tiles * B * (n32 // nt) < 512:
        nt = nt // 2 if nt in (4, 2) else 1
    blocks = tiles * B * (n32 // nt)
    n_chunks = -(-c["cin"] // 16)
    ksplit = 1
    if c.get("ws") and blocks < 128 and n_chunks >= 4:
        ksplit = min(-(-256 // blocks), n_chunks // 2, 16)
        ksplit = -(-n_chunks // -(-n_chunks // ksplit))
    if nt == 4:
        minb = (3 if blocks * ksplit >= 3072 else 2) if s == 1 else 1
    else:
        minb = {3: (3, 2), 2: (3, 2), 1: (4, 2)}[nt][s - 1]
    ts = 3 if nt >= 3 or (nt == 2 and s == 2) else 9
    return f"conv3x3_mfma_kernel<{nt}, {ts}, {s}, false, {minb}, false>" + (f" split-K x{ksplit} + conv_splitk_reduce_kernel" if ksplit > 1 else "")


def run_case(c, dev):
    """The output of the case as a host array.  Calls only the C entry points and the host-side weight packers."""
    from m4depth_amd import network_ops as nops
    from m4depth_amd._lib import lib, dptr, stream_ptr, check
    rng = np.random.default_rng(1000 + [case_id(k) for k in CASES].index(case_id(c)))
    cin, cout, s, h, w, e = c["cin"], c["cout"], c["stride"], c["h"], c["w"], c["entry"]
    x = torch.from_numpy(rng.standard_normal((B, h, w, cin), dtype=np.float32)).to(dev)
    k = (rng.standard_normal((3, 3, cin, cout)) * (2.0 / (9 * cin)) ** 0.5).astype(np.float32)
    bias = torch.from_numpy((0.1 * rng.standard_normal(cout)).astype(np.float32)).to(dev)
    oh, ow = -(-h // s), -(-w // s)
    out = torch.full((B, oh, ow, cout), float("nan"), dtype=torch.float32, device=dev)
    if e in ("m4d_conv3x3_wino_bias_act", "m4d_conv3x3_wino2_bias_act"):
        wu, cpad = nops.pack_conv_weights_winograd(k, chunk=16 if e == "m4d_conv3x3_wino_bias_act" else 8)
        wd = torch.from_numpy(wu).to(dev)
        rc = getattr(lib, e)(dptr(x), dptr(wd), dptr(bias), B, h, w, cin, cout, cpad, SLOPE, dptr(out), stream_ptr())
    else:
        wp, cpad = nops.pack_conv_weights(k)
        wd = torch.from_numpy(wp).to(dev)
        if e == "m4d_conv3x3s_small_bias_act":
            rc = lib.m4d_conv3x3s_small_bias_act(dptr(x), dptr(wd), dptr(bias), B, h, w, cin, cout, cpad, s, SLOPE, dptr(out), stream_ptr())
        elif e == "m4d_conv3x3s2_dinl_bias_act":
            mean = torch.from_numpy((0.2 * rng.standard_normal(B * cin)).astype(np.float32)).to(dev)
            var = torch.from_numpy((0.5 + rng.random(B * cin)).astype(np.float32)).to(dev)
            scale = torch.from_numpy((1.0 + 0.1 * rng.standard_normal(cin)).astype(np.float32)).to(dev)
            shift = torch.from_numpy((0.1 * rng.standard_normal(cin)).astype(np.float32)).to(dev)
            rc = lib.m4d_conv3x3s2_dinl_bias_act(dptr(x), dptr(mean), dptr(var), dptr(scale), dptr(shift), SLOPE, dptr(wd), dptr(bias),
                                                 B, h, w, cout, cpad, SLOPE, dptr(out), stream_ptr())
        else:
            ws, ws_floats = None, 0
            if c.get("ws"):
                ws_floats = int(lib.m4d_conv3x3_workspace_floats(B, oh, ow, cpad))
                ws = torch.empty(ws_floats, dtype=torch.float32, device=dev)
            rc = lib.m4d_conv3x3s_bias_act_ws(dptr(x), dptr(wd), dptr(bias), B, h, w, cin, cout, cpad, s, SLOPE, dptr(out), dptr(ws),
                                              ws_floats, stream_ptr())
    check(rc, e)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", nargs="?", const=GOLDEN, default=None, metavar="PATH")
    args = ap.parse_args()
    from m4depth_amd import _lib
    dev = torch.device("cuda:0")
    print("library:", _lib.build_info(), flush=True)
    table = {}
    for c in CASES:
        out = run_case(c, dev)
        assert np.isfinite(out).all(), case_id(c)
        table[case_id(c)] = digest(out)
        print(f"{case_id(c):60s} {kernel_of(c):70s} {table[case_id(c)][:16]}", flush=True)
    if args.write:
        with open(args.write, "w") as f:
            json.dump(table, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
