"""The convolution kernels on the trained encoder's weights and activations (tests/trained_cases.py): dead output and input
channels, per-channel exponents up to 32 in the fp16 two-term packers, ``lo`` terms in fp16's subnormal range, and layer inputs
whose channels lie 2^15 and more apart under one tile / window scale -- against the float32 oracle and its float64 evaluation,
at the bars the suite already holds these kernels to on He-initialised weights and Gaussian inputs."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import m4depth_oracle as O
from m4depth_amd import synthetic as S
from helpers import F, to_dev, npy
import trained_cases as T

pytestmark = pytest.mark.gpu

SNAPSHOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_dispatch_snapshot.json")
CROP = (37, 53)
SLOPE = 0.1
# ("enc", level, conv): the layer as the encoder runs it; ("s1", level, 2): the stride-2 kernel as a stride-1 layer
CASES = [("enc", l, c) for l, c in T.LAYERS] + [("s1", l, 2) for l in range(2, 7)]
SPLIT_STRIDE1 = (("conv3x3_wino6_bias_act", "wino6"), ("conv3x3_wino6_bias_act", "winof16"), ("conv3x3_lat", "lat"),
                 ("conv3x3_lat_f16", "lat_f16"), ("conv3x3_small6_bias_act", "small6"))
FP32_DIRECT = ("conv3x3_bias_act", "direct")
FP32_WINO = ("conv3x3_wino2_bias_act", "wino8")
_cases = {}


def snapshot_wrappers():
    """{layer tag: {(wrapper, layout)}}: every launch wrapper tests/golden/conv_dispatch_snapshot.json names for an encoder
    layer, in any workload under any arithmetic."""
    with open(SNAPSHOT) as fh:
        snap = json.load(fh)
    col = {n: i for i, n in enumerate(snap["columns"])}
    out = {}
    for per_workload in snap["rows"].values():
        for rows in per_workload.values():
            for r in rows:
                if r[col["layer"]].startswith("enc."):
                    out.setdefault(r[col["layer"]], set()).add((r[col["wrapper"]], r[col["layout"]]))
    return out


def _act(r):
    return np.where(r > 0, r, r * r.dtype.type(SLOPE))


def _crops(a):
    """Batch 2 from one [1,h,w,c] map: the top-left and the bottom-right crop of at most 37x53; a map no larger than that
    (levels 5 and 6) whole, and turned by 180 degrees as the second image."""
    _, h, w, _ = a.shape
    ch, cw = min(h, CROP[0]), min(w, CROP[1])
    second = a[0, ::-1, ::-1] if (ch, cw) == (h, w) else a[0, h - ch:, w - cw:]
    return np.ascontiguousarray(np.stack([a[0, :ch, :cw], second])).astype(F)


def layer_case(kind, l, c):
    """Inputs and references of one case, computed once: x [2,h,w,cin] (the layer's real input, teacher-forced), kernel, bias,
    stride, the float32 oracle, its float64 evaluation, and sum |x||w| + |bias| in float64."""
    if (kind, l, c) not in _cases:
        tw = T.trained_encoder_weights()
        k, bias = tw[l, c, "kernel"], tw[l, c, "bias"]
        x = _crops(T.trained_activations()[l, c])
        stride = c if kind == "enc" else 1
        ref32 = _act(O.conv2d_same(x, k, bias, stride)).astype(F)
        with O.float64_reference():
            k64, b64 = k.astype(np.float64), bias.astype(np.float64)
            ref64 = _act(O.conv2d_same(x.astype(np.float64), k64, b64, stride))
            mag = O.conv2d_same(np.abs(x).astype(np.float64), np.abs(k64), np.abs(b64), stride)
        dead = np.abs(k).max(axis=(0, 1, 2)) < T.DEAD
        _cases[kind, l, c] = dict(x=x, k=k, bias=bias, stride=stride, ref32=ref32, ref64=ref64, mag=mag, dead=dead)
    return _cases[kind, l, c]


def wrappers_for(kind, l, c):
    """[(wrapper, layout)] to run: what the snapshot names for the encoder layer; for a stride-2 kernel run as a stride-1 layer,
    every stride-1 split kernel whose layout the shape admits (_Conv3x3SameTF.can_use)."""
    from m4depth_amd import network as N
    if kind == "enc":
        return sorted(snapshot_wrappers()[f"enc.s{c}.{l - 1}"])
    cin, cout = T.layer_shape(l, c)[2:]
    conv = N._Conv3x3SameTF(cout, 1)
    conv.small_maps_ok = True                                  # a refiner layer
    return [(w, lay) for w, lay in SPLIT_STRIDE1 if conv.can_use(lay, cin)]


def launch(wrapper, layout, case, xd, bd, dev, final=True):
    """One launch of ``wrapper`` on weights packed by the layout's own packer (network._LAYOUTS), as _Conv3x3SameTF.forward does."""
    from m4depth_amd import network as N
    from m4depth_amd import network_ops as nops
    k, stride = case["k"], case["stride"]
    cout = k.shape[3]
    key = ("packed", layout, dev)
    if key not in case:
        pack, int16, has_pad = N._LAYOUTS[layout]
        res = pack(k)
        wp, cpad = res if has_pad else (res, None)
        case[key] = (torch.from_numpy(wp.view(np.int16) if int16 else wp).to(dev), cpad)
    wd, cpad = case[key]
    b, h, w, cin = xd.shape
    if wrapper == "conv3x3_bias_act":
        return nops.conv3x3_bias_act(xd, wd, bd, cout, cpad, SLOPE, stride)
    if wrapper == "conv3x3_small_bias_act":
        return nops.conv3x3_small_bias_act(xd, wd, bd, cout, cpad, SLOPE, stride=stride)
    assert stride == 1, wrapper
    if wrapper == "conv3x3_wino2_bias_act":
        return nops.conv3x3_wino2_bias_act(xd, wd, bd, cout, cpad, SLOPE)
    if wrapper == "conv3x3_wino6_bias_act":
        return nops.conv3x3_wino6_bias_act(xd, wd, bd, cout, cpad, SLOPE, arith="f16x2" if layout == "winof16" else "bf16x3")
    if wrapper == "conv3x3_small6_bias_act":
        return nops.conv3x3_small6_bias_act(xd, wd, bd, cout, cpad, SLOPE)
    if wrapper in ("conv3x3_lat", "conv3x3_lat_f16"):
        out = getattr(nops, wrapper)(xd, wd, bd, cout, SLOPE, config=nops.lat_config(b, h, w, cin, cout, final))
        return out.dense() if isinstance(out, nops.PartialAct) else out
    raise KeyError(f"the dispatch snapshot names a wrapper this test cannot launch: {wrapper}")


def _per_channel(got64, case):
    """max over pixels of |got - float64| / (sum |x||w| + |bias|) per output channel -> (dead channels' max, live channels' max)."""
    r = (np.abs(got64 - case["ref64"]) / np.maximum(case["mag"], 1e-300)).max(axis=(0, 1, 2))
    dead = case["dead"]
    return (float(r[dead].max()) if dead.any() else 0.0), float(r[~dead].max())


def _check_dead_channels(got, case, what):
    """A dead output channel is act(bias + s) with |s| <= sum |x||w|: 1e-5 to 5e-3 on these inputs, beside biases of 4e-4 to
    3e-2, so neither a dropped bias nor a dropped s hides.  Within float32 rounding of its float64 value -- 2^-20 (sum |x||w| +
    |bias|), the floor of the per-channel bars --, not zero, and not the sum without the activation (10x as far below zero)."""
    dead = case["dead"]
    if not dead.any():
        return
    g, want, tol = got[..., dead], case["ref64"][..., dead], 2.0 ** -20 * case["mag"][..., dead]
    assert np.all(np.abs(g - want) <= tol), (what, float((np.abs(g - want) / tol).max()))
    assert np.all(np.abs(want) > 2 * tol) and np.all(g != 0), what
    neg = want < 0
    assert neg.mean() > 0.5 and np.all(np.abs(g[neg] - want[neg] / SLOPE) > 4 * tol[neg]), what


@pytest.mark.parametrize("kind,l,c", CASES, ids=[f"{k}-L{l}-conv2d_{c}" for k, l, c in CASES])
def test_trained_layer_teacher_forced(dev, kind, l, c):
    """Every wrapper the dispatch snapshot names for the encoder layer ("enc"), or every stride-1 split kernel the shape admits
    for the stride-2 kernels run as stride-1 layers ("s1": the refiner's code paths, handing partial slabs on), on the layer's
    real input; the fp32 direct kernel runs beside them as the yardstick of the per-channel bar.  Bars, all the suite's own: within
    1e-5 x max(1, |ref32|max) of the float32 oracle; Winograd split kernels: mean / max error to float64 <= 2x / 3x the oracle's;
    f16x2 latency kernel <= 1.25x the bf16x3 one's mean and max; a repeated launch bit-identical; per output channel max |got -
    float64| / (sum |x||w| + |bias|), dead and live channels apart: f16x2 <= max(4 x bf16x3, 2^-20), bf16x3 <= max(4 x the fp32
    kernel, 2^-20); dead output channels = act(bias + s) (_check_dead_channels).

    Measured on the MI355X, per kernel: mean / max |error| to float64 (per-channel figure: dead, live channels).  direct / small =
    the fp32 kernels, wino2 = fp32 Winograd, wino6 / lat / small6 = bf16x3, winof16 / lat_f16 = f16x2.  Closest to a bar: wino6 on
    L6 conv2d_1, 1.83x / 2.64x the oracle's mean / max (bars 2x / 3x; the oracle is nearly exact on 178 dead channels of 192).
    enc L1 conv2d_1 3->16 stride 1, 37x53, 0 dead:
        float32 oracle 2.92e-08 / 3.39e-07  (0.0e+00, 1.0e-07) | direct 3.79e-08 / 5.92e-07 (0.0e+00, 1.7e-07)
    enc L1 conv2d_2 16->16 stride 2, 37x53, 0 dead:
        float32 oracle 1.67e-08 / 1.96e-07  (0.0e+00, 1.1e-07) | direct 3.95e-08 / 9.19e-07 (0.0e+00, 4.5e-07)
    enc L2 conv2d_1 16->32 stride 1, 37x53, 0 dead:
        float32 oracle 3.37e-08 / 5.78e-07  (0.0e+00, 1.6e-07) | direct 7.76e-08 / 1.86e-06 (0.0e+00, 4.6e-07) |
        wino2 4.97e-08 / 1.10e-06 (0.0e+00, 2.4e-07)
    enc L2 conv2d_2 32->32 stride 2, 37x53, 0 dead:
        float32 oracle 6.04e-08 / 1.09e-06  (0.0e+00, 9.8e-08) | direct 1.58e-07 / 3.41e-06 (0.0e+00, 3.9e-07) |
        small 1.17e-07 / 2.64e-06 (0.0e+00, 2.0e-07)
    enc L3 conv2d_1 32->64 stride 1, 37x53, 0 dead:
        float32 oracle 9.56e-08 / 2.34e-06  (0.0e+00, 1.5e-07) | lat 1.50e-07 / 3.94e-06 (0.0e+00, 2.5e-07) |
        lat_f16 1.25e-07 / 2.35e-06 (0.0e+00, 1.7e-07) | small 1.78e-07 / 3.88e-06 (0.0e+00, 2.8e-07) |
        wino2 1.46e-07 / 4.05e-06 (0.0e+00, 2.4e-07) | wino6 1.19e-07 / 2.23e-06 (0.0e+00, 2.3e-07) |
        winof16 1.35e-07 / 1.77e-06 (0.0e+00, 1.9e-07) | direct 2.75e-07 / 6.47e-06 (0.0e+00, 5.7e-07)
    enc L3 conv2d_2 64->64 stride 2, 37x53, 0 dead:
        float32 oracle 1.34e-07 / 3.14e-06  (0.0e+00, 1.4e-07) | direct 2.56e-07 / 7.31e-06 (0.0e+00, 2.6e-07) |
        small 1.86e-07 / 4.02e-06 (0.0e+00, 1.5e-07)
    enc L4 conv2d_1 64->96 stride 1, 37x53, 0 dead:
        float32 oracle 1.33e-07 / 2.91e-06  (0.0e+00, 2.0e-07) | wino2 2.24e-07 / 6.77e-06 (0.0e+00, 6.3e-07) |
        wino6 1.85e-07 / 4.43e-06 (0.0e+00, 3.2e-07) | winof16 1.74e-07 / 4.07e-06 (0.0e+00, 3.6e-07) |
        direct 2.81e-07 / 7.15e-06 (0.0e+00, 5.0e-07)
    enc L4 conv2d_2 96->96 stride 2, 37x53, 11 dead:
        float32 oracle 1.46e-07 / 4.13e-06  (1.2e-08, 2.1e-07) | direct 1.70e-07 / 4.82e-06 (1.3e-08, 2.5e-07) |
        small 1.68e-07 / 4.62e-06 (1.4e-08, 2.8e-07)
    enc L5 conv2d_1 96->128 stride 1, 24x40, 43 dead:
        float32 oracle 4.58e-08 / 1.63e-06  (9.6e-09, 2.8e-07) | lat 6.78e-08 / 2.21e-06 (9.5e-09, 3.6e-07) |
        lat_f16 5.62e-08 / 1.71e-06 (9.5e-09, 3.6e-07) | small 7.68e-08 / 3.97e-06 (9.6e-09, 4.2e-07) |
        wino2 7.67e-08 / 2.75e-06 (9.5e-09, 5.8e-07) | wino6 6.80e-08 / 2.08e-06 (9.5e-09, 8.7e-07) |
        winof16 6.14e-08 / 2.27e-06 (9.6e-09, 6.5e-07) | direct 8.78e-08 / 3.68e-06 (9.5e-09, 5.2e-07)
    enc L5 conv2d_2 128->128 stride 2, 24x40, 65 dead:
        float32 oracle 4.45e-08 / 2.01e-06  (8.9e-09, 2.6e-07) | direct 5.45e-08 / 1.96e-06 (9.1e-09, 3.9e-07) |
        small 6.11e-08 / 2.08e-06 (9.7e-09, 4.2e-07)
    enc L6 conv2d_1 128->192 stride 1, 12x20, 178 dead:
        float32 oracle 1.51e-09 / 3.20e-07  (3.7e-08, 1.9e-07) | lat 2.52e-09 / 7.96e-07 (4.1e-08, 2.4e-07) |
        lat_f16 2.16e-09 / 4.96e-07 (3.4e-08, 2.1e-07) | small 2.33e-09 / 6.18e-07 (3.7e-08, 2.5e-07) |
        wino2 2.46e-09 / 5.74e-07 (3.8e-08, 9.4e-07) | wino6 2.77e-09 / 8.44e-07 (3.4e-08, 1.6e-06) |
        winof16 2.44e-09 / 7.32e-07 (3.5e-08, 1.4e-06) | direct 2.37e-09 / 5.54e-07 (3.8e-08, 2.6e-07)
    enc L6 conv2d_2 192->192 stride 2, 12x20, 174 dead:
        float32 oracle 9.46e-09 / 9.87e-07  (4.8e-08, 8.3e-07) | direct 9.25e-09 / 9.08e-07 (4.8e-08, 8.4e-07) |
        small 1.44e-08 / 1.31e-06 (4.8e-08, 1.2e-06)
    s1 L2 conv2d_2 32->32 stride 1, 37x53, 0 dead:
        float32 oracle 6.27e-08 / 1.29e-06  (0.0e+00, 1.2e-07) | wino6 6.42e-08 / 9.63e-07 (0.0e+00, 1.3e-07) |
        winof16 7.39e-08 / 1.28e-06 (0.0e+00, 1.5e-07) | lat 1.01e-07 / 2.71e-06 (0.0e+00, 2.5e-07) |
        lat_f16 8.30e-08 / 1.91e-06 (0.0e+00, 1.7e-07) | small6 1.01e-07 / 2.71e-06 (0.0e+00, 2.5e-07) |
        direct 1.63e-07 / 4.32e-06 (0.0e+00, 3.9e-07)
    s1 L3 conv2d_2 64->64 stride 1, 37x53, 0 dead:
        float32 oracle 1.36e-07 / 4.08e-06  (0.0e+00, 1.4e-07) | wino6 1.26e-07 / 3.65e-06 (0.0e+00, 1.6e-07) |
        winof16 1.30e-07 / 3.40e-06 (0.0e+00, 1.5e-07) | lat 1.64e-07 / 5.90e-06 (0.0e+00, 2.0e-07) |
        lat_f16 1.35e-07 / 4.44e-06 (0.0e+00, 1.4e-07) | small6 1.64e-07 / 5.90e-06 (0.0e+00, 2.0e-07) |
        direct 2.64e-07 / 8.10e-06 (0.0e+00, 3.0e-07)
    s1 L4 conv2d_2 96->96 stride 1, 37x53, 11 dead:
        float32 oracle 1.47e-07 / 4.13e-06  (1.2e-08, 2.1e-07) | wino6 1.18e-07 / 4.58e-06 (1.2e-08, 4.8e-07) |
        winof16 1.06e-07 / 3.46e-06 (1.3e-08, 3.3e-07) | lat 1.47e-07 / 4.18e-06 (1.2e-08, 2.4e-07) |
        lat_f16 1.18e-07 / 3.48e-06 (1.2e-08, 1.8e-07) | small6 1.42e-07 / 5.25e-06 (1.3e-08, 2.2e-07) |
        direct 1.72e-07 / 5.54e-06 (1.3e-08, 3.5e-07)
    s1 L5 conv2d_2 128->128 stride 1, 24x40, 65 dead:
        float32 oracle 4.50e-08 / 2.01e-06  (9.2e-09, 3.4e-07) | wino6 3.38e-08 / 2.09e-06 (1.0e-08, 5.2e-07) |
        winof16 3.05e-08 / 1.48e-06 (9.4e-09, 7.7e-07) | lat 3.81e-08 / 2.71e-06 (9.8e-09, 3.2e-07) |
        lat_f16 3.18e-08 / 1.64e-06 (9.3e-09, 3.1e-07) | small6 4.16e-08 / 2.00e-06 (9.2e-09, 3.0e-07) |
        direct 5.50e-08 / 4.22e-06 (1.0e-08, 5.2e-07)
    s1 L6 conv2d_2 192->192 stride 1, 12x20, 174 dead:
        float32 oracle 9.20e-09 / 9.87e-07  (5.0e-08, 8.3e-07) | wino6 2.54e-09 / 4.71e-07 (5.1e-08, 2.3e-06) |
        winof16 2.54e-09 / 3.60e-07 (5.0e-08, 8.9e-07) | lat 2.66e-09 / 5.02e-07 (5.0e-08, 4.1e-07) |
        lat_f16 2.34e-09 / 3.96e-07 (5.0e-08, 2.9e-07) | small6 3.70e-09 / 8.02e-07 (5.0e-08, 4.4e-07) |
        direct 9.08e-09 / 9.08e-07 (5.0e-08, 8.4e-07)
    With the stored exponents capped at 18 while the weights keep their true scale (a kernel that ignores exponents above 18; scratch
    packers, not committed) the five cases that run an f16x2 kernel on a kernel with dead channels fail -- enc L5 / L6 conv2d_1, s1
    L4 / L5 / L6 -- and so do both f16x2 chains and the f16x2 whole model; test_gpu_wino_f16.py and test_gpu_lat_f16.py pass."""
    case = layer_case(kind, l, c)
    cin, cout = case["k"].shape[2:]
    xd, bd = to_dev(case["x"], dev), to_dev(case["bias"], dev)
    ref32, ref64 = case["ref32"], case["ref64"]
    todo = wrappers_for(kind, l, c)
    assert todo, (kind, l, c)
    yard = [y for y in (FP32_DIRECT,) if y not in todo and case["stride"] == 1]       # the fp32 kernel the split kernels are held to
    e_or = np.abs(ref32.astype(np.float64) - ref64)
    pc_or = _per_channel(ref32.astype(np.float64), case)
    print(f"\n{kind} L{l} conv2d_{c} {cin}->{cout} stride {case['stride']} on {case['x'].shape[1]}x{case['x'].shape[2]}, {int(case['dead'].sum())} dead "
          f"output channels; float32 oracle to float64: mean {e_or.mean():.2e} max {e_or.max():.2e}, per channel dead {pc_or[0]:.1e} live {pc_or[1]:.1e}")
    err, pc = {}, {}
    for wrapper, layout in todo + yard:
        what = (kind, l, c, wrapper, layout)
        out = launch(wrapper, layout, case, xd, bd, dev, final=kind == "enc")
        assert torch.equal(out, launch(wrapper, layout, case, xd, bd, dev, final=kind == "enc")), what    # bit-identical
        got = npy(out)
        assert got.shape == ref32.shape and np.isfinite(got).all(), what
        d32 = float(np.max(np.abs(got - ref32)))
        got = got.astype(np.float64)
        err[wrapper, layout] = np.abs(got - ref64)
        pc[wrapper, layout] = _per_channel(got, case)
        e = err[wrapper, layout]
        print(f"  {wrapper:26s} {layout:8s} to float32 oracle {d32:.2e} | to float64 mean {e.mean():.2e} max {e.max():.2e} "
              f"| per channel dead {pc[wrapper, layout][0]:.1e} live {pc[wrapper, layout][1]:.1e}")
        assert d32 < 1e-5 * max(1.0, float(np.abs(ref32).max())), what
        _check_dead_channels(got, case, what)
        if wrapper == "conv3x3_wino6_bias_act":
            assert e.mean() <= 2.0 * e_or.mean() and e.max() <= 3.0 * e_or.max(), what
    floor = 2.0 ** -20
    for f16, bf, f32 in ((SPLIT_STRIDE1[1], SPLIT_STRIDE1[0], FP32_WINO if FP32_WINO in pc else FP32_DIRECT),
                         (SPLIT_STRIDE1[3], SPLIT_STRIDE1[2], FP32_DIRECT), (None, SPLIT_STRIDE1[4], FP32_DIRECT)):
        if bf in pc and f32 in pc:
            for cls in (0, 1):
                assert pc[bf][cls] <= max(4.0 * pc[f32][cls], floor), (kind, l, c, bf, "dead" if cls == 0 else "live")
        if f16 in pc:
            assert bf in pc, (kind, l, c, f16)
            for cls in (0, 1):
                assert pc[f16][cls] <= max(4.0 * pc[bf][cls], floor), (kind, l, c, f16, "dead" if cls == 0 else "live")
    lat16, lat = SPLIT_STRIDE1[3], SPLIT_STRIDE1[2]
    if lat16 in err:
        assert err[lat16].mean() <= 1.25 * err[lat].mean() and err[lat16].max() <= 1.25 * err[lat].max(), (kind, l, c)


# ------------------------------------------------------------------------------------------------ encoder chain
CHAIN = (2, 128, 192, 77)            # batch, height, width, seed of synthetic.make_sequence


def _chain_refs():
    if "chain" not in _cases:
        b, h, w, seed = CHAIN
        img = S.make_sequence(b, 1, h, w, seed=seed)[0][0]["RGB_im"]
        W = T.model_weights(6)
        ref32 = O.feature_pyramid(img, W, 6)
        with O.float64_reference():
            ref64 = O.feature_pyramid(img.astype(np.float64), {k: v.astype(np.float64) for k, v in W.items()}, 6)
        _cases["chain"] = (img, W, ref32, ref64)
    return _cases["chain"]


@pytest.mark.parametrize("seq_batch", [1, 8])
@pytest.mark.parametrize("arith", ["f16x2", "bf16x3", "f32"])
def test_trained_encoder_chain(dev, arith, seq_batch):
    """M4Depth(6 levels) with the trained encoder: its FeaturePyramid on a 2x128x192 batch, dispatched for a sequence batch of 1
    (latency-first kernels on the coarse levels) and 8 (Winograd / direct), every level's mean / max error to the float64
    evaluation of oracle.feature_pyramid <= 2x / 3x the float32 oracle's.

    Measured on the MI355X, mean / max |error| to float64, levels 1 to 6.  The float32 oracle: 2.54e-06 / 3.94e-05, 6.45e-06 /
    1.16e-04, 9.96e-06 / 1.68e-04, 8.86e-06 / 2.35e-04, 3.34e-06 / 1.17e-04, 2.18e-07 / 3.15e-05 -- it takes the DINL statistics of
    level 1 in float32 and carries that error down the chain; the GPU sums them in double, so every GPU figure is 0.02x to 0.10x
    the oracle's and these bars are slack (the teacher-forced test above is the sharp one; this one sees a wrong scale).
      f16x2, batch 1 (direct, direct, lat_f16 x 4):  1.36e-07 / 1.66e-06, 2.77e-07 / 3.39e-06, 3.68e-07 / 7.96e-06, 2.83e-07 /
                                                     6.23e-06, 8.27e-08 / 1.84e-06, 1.43e-08 / 1.26e-06
      f16x2, batch 8 (direct, wino2, wino6 x 2, lat_f16 x 2): 1.36e-07 / 1.66e-06, 2.93e-07 / 5.10e-06, 4.92e-07 / 1.52e-05,
                                                     3.28e-07 / 6.83e-06, 9.32e-08 / 2.28e-06, 1.42e-08 / 1.44e-06
      bf16x3, batch 1 (direct, direct, lat x 4):     1.36e-07 / 1.66e-06, 2.77e-07 / 3.39e-06, 3.73e-07 / 7.72e-06, 2.84e-07 /
                                                     5.40e-06, 8.16e-08 / 2.47e-06, 1.42e-08 / 1.20e-06
      bf16x3, batch 8 (direct, wino2, wino6 x 2, lat x 2): 1.36e-07 / 1.66e-06, 2.93e-07 / 5.10e-06, 4.89e-07 / 1.62e-05,
                                                     3.26e-07 / 6.02e-06, 8.71e-08 / 2.25e-06, 1.46e-08 / 1.32e-06
      f32, batch 1 (direct, direct, small x 4):      1.36e-07 / 1.66e-06, 2.77e-07 / 3.39e-06, 3.79e-07 / 8.44e-06, 2.92e-07 /
                                                     6.23e-06, 8.74e-08 / 2.00e-06, 1.54e-08 / 1.38e-06
      f32, batch 8 (direct, wino2 x 2, direct, small x 2): 1.36e-07 / 1.66e-06, 2.93e-07 / 5.10e-06, 4.91e-07 / 1.43e-05,
                                                     3.90e-07 / 7.12e-06, 9.95e-08 / 2.72e-06, 1.44e-08 / 1.26e-06"""
    import m4depth_amd as M
    from m4depth_amd import network as N
    img, W, ref32, ref64 = _chain_refs()
    with N.conv_arithmetic(arith):
        model = M.M4Depth(nbre_levels=6)
        model.load_numpy_weights(W, dev)
        model.encoder.set_sequence_batch(seq_batch)
        plans = [conv.plan(img.shape[0], -(-img.shape[1] // 2 ** i), -(-img.shape[2] // 2 ** i), conv.weight.shape[1]).kernel
                 for i, conv in enumerate(model.encoder.conv_layers_s1)]
        outs = [npy(t) for t in model.encoder(to_dev(img, dev))]
    print(f"\nencoder chain {arith}, sequence batch {seq_batch}: stride-1 layers on {plans}")
    if arith != "f32":
        assert ("lat_f16" if arith == "f16x2" else "lat") in plans if seq_batch == 1 else "wino6" in plans, plans
    bad = []
    for l, (got, r32, r64) in enumerate(zip(outs, ref32, ref64)):
        assert got.shape == r32.shape and np.isfinite(got).all()
        e_g, e_o = np.abs(got.astype(np.float64) - r64), np.abs(r32.astype(np.float64) - r64)
        print(f"  level {l + 1} {got.shape[1]}x{got.shape[2]}x{got.shape[3]}: to float64 mean / max: gpu {e_g.mean():.2e} / {e_g.max():.2e}, "
              f"float32 oracle {e_o.mean():.2e} / {e_o.max():.2e}  ({e_g.mean() / e_o.mean():.2f}x / {e_g.max() / e_o.max():.2f}x)")
        if not (e_g.mean() <= 2.0 * e_o.mean() and e_g.max() <= 3.0 * e_o.max()):
            bad.append(l + 1)
    assert not bad, (arith, seq_batch, bad)


# ------------------------------------------------------------------------------------------------ whole model
@pytest.mark.parametrize("arith", ["f16x2", "bf16x3"])
def test_trained_encoder_whole_model(dev, arith):
    """6 levels, 128x192, batch 2, 3 frames: trained encoder, synthetic.init_weights refiner (seed 42), every level of the last
    frame through test_gpu_configs.check_against_float64_truth at its factor 2.5.  The float32 oracle's own quantiles are
    not vacuous on this case (parallax error to float64, median 1.4e-06 at the two finest levels, 5e-08 to 5e-07 below), so the
    factor is asserted as it stands.

    Measured on the MI355X, relative parallax error to float64, median / p99 / max, levels 0 to 5 (64x96 down to 2x3):
      float32 oracle: 1.36e-06 / 6.99e-05 / 4.29e-04, 1.44e-06 / 3.52e-04 / 1.16e-03, 4.40e-07 / 4.02e-06 / 7.07e-06,
                      5.16e-07 / 2.29e-06 / 2.89e-06, 3.33e-07 / 1.10e-06 / 1.19e-06, 4.86e-08 / 1.09e-07 / 1.11e-07
      f16x2:          4.86e-07 / 2.45e-05 / 1.18e-04, 4.93e-07 / 9.72e-05 / 3.06e-04, 1.32e-07 / 3.29e-06 / 5.63e-06,
                      3.76e-08 / 4.03e-07 / 4.78e-07, 5.64e-08 / 4.77e-07 / 5.36e-07, 1.53e-08 / 3.66e-08 / 3.71e-08
      bf16x3:         5.29e-07 / 3.81e-05 / 2.06e-04, 5.18e-07 / 1.32e-04 / 5.45e-04, 1.31e-07 / 2.54e-06 / 4.74e-06,
                      4.48e-08 / 3.82e-07 / 4.78e-07, 1.70e-07 / 4.60e-07 / 5.36e-07, 1.53e-08 / 3.28e-08 / 3.31e-08
    depth within 1e-4 of float64 at levels 0 / 1: f16x2 99.87 % / 98.67 %, bf16x3 99.55 % / 97.04 %, oracle 98.76 % / 94.79 %."""
    from m4depth_amd import network as N
    from test_gpu_configs import _model, check_against_float64_truth
    L, H, Wd, T_, b = 6, 128, 192, 3, 2
    if "model" not in _cases:
        W = T.model_weights(L)
        samples, cam = S.make_sequence(b, T_, H, Wd, seed=91)
        _, seq32 = O.M4Depth(W, L)(samples, cam)
        with O.float64_reference():
            _, seq64 = O.M4Depth(W, L)(samples, cam)
        _cases["model"] = (W, samples, cam, seq32, seq64)
    W, samples, cam, seq32, seq64 = _cases["model"]
    with N.conv_arithmetic(arith):
        model = _model(dev, L, W)
        model([to_dev(samples, dev), to_dev(cam, dev)])
    for l in range(L):
        est = model.last_estimates[-1][l]
        check_against_float64_truth({"parallax": npy(est["parallax"]), "depth": npy(est["depth"])}, seq32[-1][l], seq64[-1][l],
                                    f"[trained encoder {arith}] level {l}", factor=2.5)
