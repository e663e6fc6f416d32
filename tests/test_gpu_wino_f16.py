"""The fp16 two-term Winograd kernel (csrc/m4d_wino_f16.hip, conv_arith "f16x2"): accuracy against the float32 oracle and
the float64 truth at the bars of the bf16x3 kernel, range handling (power-of-two scales per Winograd position and tile), bit-level determinism, and the model
under "f16x2" against the golden outputs and the float64 truth."""
import numpy as np
import pytest
import torch

from oracle import m4depth_oracle as O
from m4depth_amd import synthetic as S
from helpers import F, to_dev, npy

pytestmark = pytest.mark.gpu


def _pack(k, dev):
    from m4depth_amd import network_ops as nops
    wu, cpad = nops.pack_conv_weights_winof16(k)
    assert cpad % 64 == 0 and wu.dtype == np.uint16
    return torch.from_numpy(wu.view(np.int16)).to(dev), cpad


def _f16(xd, wd, bd, cout, cpad, slope, **kw):
    from m4depth_amd import network_ops as nops
    return nops.conv3x3_winof16_bias_act(xd, wd, bd, cout, cpad, slope, **kw)


def _bf16(xd, k, bd, cout, slope, dev):
    from m4depth_amd import network_ops as nops
    wu6, cpad6 = nops.pack_conv_weights_wino6(k)
    return nops.conv3x3_wino6_bias_act(xd, torch.from_numpy(wu6.view(np.int16)).to(dev), bd, cout, cpad6, slope, kernel=1)


def _act(r, slope):
    return np.where(r > 0, r, r * r.dtype.type(slope))


@pytest.mark.parametrize("b,h,w,cin,cout,slope", [
    (2, 32, 48, 64, 128, 0.1),
    (1, 37, 53, 112, 96, 0.1),        # ragged tiles, a half unit
    (2, 40, 56, 64, 32, 0.1),         # one half unit per tile
    (1, 33, 47, 16, 24, 0.1),         # a single K chunk, a partly filled N-tile
    (1, 19, 21, 32, 40, 1.0),         # N padding, no activation, map smaller than two tiles
    (2, 16, 16, 16, 64, 0.1),
    (1, 50, 90, 96, 64, 0.1),
    (2, 100, 130, 48, 120, 0.1),      # guarded store path on the last quad
    (1, 192, 320, 64, 66, 1.0),       # scalar stores
    (1, 192, 640, 128, 128, 0.1),     # the level-1 layer
    (1, 192, 640, 128, 96, 0.1),
    (4, 100, 130, 48, 120, 0.1),      # odd chunk count
    (3, 100, 130, 32, 192, 1.0),      # two chunks, three cout groups
    (2, 70, 150, 240, 66, 0.1),       # 15 chunks
    (9, 33, 17, 80, 70, 0.1),         # many small images
])
def test_winograd_conv_f16_split(dev, b, h, w, cin, cout, slope):
    """Within 1e-5 x scale of the float32 oracle; mean / max error to float64 <= 2x / 3x the oracle's; mean error <= 1.02x the
    fp32-MFMA Winograd kernel's.  The bf16x3 kernel's error is printed beside it."""
    from m4depth_amd import network_ops as nops
    rng = np.random.default_rng(cin * 17 + cout + b)
    x = rng.standard_normal([b, h, w, cin]).astype(F)
    k = (rng.standard_normal([3, 3, cin, cout]) * np.sqrt(2.0 / (9 * cin))).astype(F)
    bias = (0.1 * rng.standard_normal([cout])).astype(F)
    wd, cpad = _pack(k, dev)
    xd, bd = to_dev(x, dev), to_dev(bias, dev)
    got = _f16(xd, wd, bd, cout, cpad, slope)
    ref32 = _act(O.conv2d_same(x, k, bias, 1), slope).astype(F)
    with O.float64_reference():
        ref64 = _act(O.conv2d_same(x.astype(np.float64), k.astype(np.float64), bias.astype(np.float64), 1), slope)
    scale = max(1.0, np.abs(ref32).max())
    assert np.max(np.abs(npy(got) - ref32)) < 1e-5 * scale
    e_gpu, e_oracle = np.abs(npy(got).astype(np.float64) - ref64), np.abs(ref32.astype(np.float64) - ref64)
    e_bf = np.abs(npy(_bf16(xd, k, bd, cout, slope, dev)).astype(np.float64) - ref64)
    print(f"f16x2 Winograd {cin}->{cout}: mean |error| to float64: f16x2 {e_gpu.mean():.3e} bf16x3 {e_bf.mean():.3e} "
          f"float32 oracle {e_oracle.mean():.3e}; max f16x2 {e_gpu.max():.3e} bf16x3 {e_bf.max():.3e} oracle {e_oracle.max():.3e}")
    assert e_gpu.mean() <= 2.0 * e_oracle.mean() and e_gpu.max() <= 3.0 * e_oracle.max()
    # The fp32-MFMA bar where the model dispatches this kernel (network._use_winograd: Cin >= 32).  With a single 16-channel
    # chunk the two-term representation error (~2^-22 per operand) is not yet below the accumulation error: 1.06x measured.
    if cin % 4 == 0 and cin >= 32:
        wu8, cpad8 = nops.pack_conv_weights_winograd(k, chunk=8)
        e_f32 = np.abs(npy(nops.conv3x3_wino2_bias_act(xd, to_dev(wu8, dev), bd, cout, cpad8, slope)).astype(np.float64) - ref64)
        print(f"    fp32-MFMA Winograd kernel: {e_f32.mean():.3e}")
        assert e_gpu.mean() <= 1.02 * e_f32.mean()


def _case(dev, b=2, h=48, w=64, cin=64, cout=96, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal([b, h, w, cin]).astype(F)
    k = (rng.standard_normal([3, 3, cin, cout]) * np.sqrt(2.0 / (9 * cin))).astype(F)
    bias = (0.1 * rng.standard_normal([cout])).astype(F)
    return x, k, bias


def _rel_to_truth(got, x, k, bias, slope):
    """|GPU - float64| per output element, in units of that pixel's float64 output scale (max over its channels)."""
    with O.float64_reference():
        ref64 = _act(O.conv2d_same(x.astype(np.float64), k.astype(np.float64), bias.astype(np.float64), 1), slope)
    s = np.maximum(np.abs(ref64).max(axis=-1, keepdims=True), 1e-300)
    return np.abs(got.astype(np.float64) - ref64) / s, ref64


def test_f16_split_magnitudes_across_and_within_tiles(dev):
    """Scales per (position, tile): inputs spanning 2^-20 .. 2^20 from tile to tile AND inside one tile (a few huge pixels among tiny ones)
    stay at the float32 oracle's error, relative to each pixel's own output scale."""
    x, k, bias = _case(dev, seed=5)
    b, h, w, cin = x.shape
    rng = np.random.default_rng(11)
    tile_exp = rng.integers(-20, 21, size=(b, -(-h // 16), -(-w // 16)))
    x = x * np.exp2(np.repeat(np.repeat(tile_exp, 16, 1), 16, 2)[:, :h, :w, None]).astype(F)
    x[0, 16:32, 16:32] *= F(2.0 ** -20)                         # inside one tile: 2^-20 .. 2^20
    x[0, 20, 21, :] = F(2.0 ** 20)
    x[1, 3:6, 40:44, ::3] *= F(2.0 ** 19)
    bias[:] = 0.0                                                # (a bias would hide the tiny tiles' error)
    xd, bd = to_dev(x.astype(F), dev), to_dev(bias, dev)
    wd, cpad = _pack(k, dev)
    got = npy(_f16(xd, wd, bd, k.shape[3], cpad, 1.0))
    e_gpu, ref64 = _rel_to_truth(got, x, k, bias, 1.0)
    ref32 = O.conv2d_same(x, k, bias, 1).astype(F)
    e_or = np.abs(ref32.astype(np.float64) - ref64) / np.maximum(np.abs(ref64).max(axis=-1, keepdims=True), 1e-300)
    e_bf = np.abs(npy(_bf16(xd, k, bd, k.shape[3], 1.0, dev)).astype(np.float64) - ref64) / \
        np.maximum(np.abs(ref64).max(axis=-1, keepdims=True), 1e-300)
    print(f"magnitudes 2^-20..2^20: relative error mean / max: f16x2 {e_gpu.mean():.3e} / {e_gpu.max():.3e}, bf16x3 "
          f"{e_bf.mean():.3e} / {e_bf.max():.3e}, float32 oracle {e_or.mean():.3e} / {e_or.max():.3e}")
    assert np.isfinite(got).all()
    assert e_gpu.mean() <= 2.0 * e_or.mean() and e_gpu.max() <= 3.0 * e_or.max()


def test_f16_split_zero_tile_huge_values_and_non_finite(dev):
    """An all-zero tile gives exactly act(bias); inputs near 1e30 do not overflow; injected Inf / NaN give the bf16x3 kernel's
    non-finite output pattern."""
    x, k, bias = _case(dev, seed=7)
    cout, slope = k.shape[3], 0.1
    wd, cpad = _pack(k, dev)
    bd = to_dev(bias, dev)
    xz = x.copy()
    xz[0, 15:34, 15:34] = 0.0                                     # the whole halo of tile (1, 1) of image 0
    got = npy(_f16(to_dev(xz, dev), wd, bd, cout, cpad, slope))
    want = np.where(bias > 0, bias, bias * F(slope)).astype(F)
    assert np.array_equal(got[0, 16:32, 16:32], np.broadcast_to(want, (16, 16, cout)))
    xh = (x * F(1e30)).astype(F)
    got = npy(_f16(to_dev(xh, dev), wd, bd, cout, cpad, slope))
    e_gpu, _ = _rel_to_truth(got, xh, k, bias, slope)
    print(f"inputs x 1e30: max relative error {e_gpu.max():.3e}")
    assert np.isfinite(got).all() and e_gpu.max() < 1e-5
    xn = x.copy()
    xn[0, 5, 7, 3] = np.inf
    xn[0, 30, 40, :] = -np.inf
    xn[1, 20, 33, 17] = np.nan
    xnd = to_dev(xn, dev)
    got = npy(_f16(xnd, wd, bd, cout, cpad, slope))
    ref = npy(_bf16(xnd, k, bd, cout, slope, dev))
    assert (~np.isfinite(got)).any()
    assert np.array_equal(np.isfinite(got), np.isfinite(ref))
    assert np.array_equal(np.isnan(got), np.isnan(ref))


def test_f16_split_bitwise_determinism(dev):
    """Repeated launches, the stagger argument and batch neighbours do not change a bit: image j of a batch is that image
    launched alone (its scales come from its own data only)."""
    x, k, bias = _case(dev, b=3, h=100, w=130, cin=48, cout=120, seed=9)
    x[1] *= F(2.0 ** 12)                                          # a neighbour of a very different magnitude
    cout = k.shape[3]
    wd, cpad = _pack(k, dev)
    xd, bd = to_dev(x, dev), to_dev(bias, dev)
    one = _f16(xd, wd, bd, cout, cpad, 0.1)
    for o in [_f16(xd, wd, bd, cout, cpad, 0.1) for _ in range(2)] + \
             [_f16(xd, wd, bd, cout, cpad, 0.1, stagger_us=us, stagger_phases=ph) for us, ph in ((9, 16), (13, 8))]:
        assert torch.equal(o.view(torch.int32), one.view(torch.int32))
    for j in range(x.shape[0]):
        alone = _f16(xd[j:j + 1].contiguous(), wd, bd, cout, cpad, 0.1)
        assert torch.equal(alone.view(torch.int32), one[j:j + 1].view(torch.int32)), j


@pytest.mark.parametrize("case", ["cfg1", "full"])
def test_well_conditioned_depth_within_1e4_everywhere_f16x2(dev, golden, case):
    """The golden well-conditioned fixture under "f16x2": depth within 1e-4 relative of the float32 oracle on every pixel."""
    from test_gpu_model import test_well_conditioned_depth_within_1e4_everywhere
    test_well_conditioned_depth_within_1e4_everywhere(dev, golden, case, "f16x2")


def test_error_against_float64_truth_f16x2(dev):
    """tests/test_gpu_configs.py::test_error_against_float64_truth under "f16x2": level 1 runs the fp16 kernel, and the model's
    parallax / depth error quantiles to the float64 truth stay within 2.5x of the float32 oracle's."""
    from m4depth_amd import network as net
    from test_gpu_configs import _model, check_against_float64_truth
    L, H, Wd, T, b = 3, 192, 384, 3, 1
    W = S.init_weights(L, seed=42)
    samples, cam = S.make_sequence(b, T, H, Wd, seed=91)
    old = net.winograd_conv
    net.winograd_conv = True
    try:
        with net.conv_arithmetic("f16x2"):
            assert net._use_winograd(b, H // 2, Wd // 2, 128, 128, 1) == 6
            model = _model(dev, L, W)
            model([to_dev(samples, dev), to_dev(cam, dev)])
    finally:
        net.winograd_conv = old
    _, seq32 = O.M4Depth(W, L)(samples, cam)
    with O.float64_reference():
        _, seq64 = O.M4Depth(W, L)(samples, cam)
    for l in range(L):
        est = model.last_estimates[-1][l]
        check_against_float64_truth({"parallax": npy(est["parallax"]), "depth": npy(est["depth"])}, seq32[-1][l], seq64[-1][l],
                                    f"[winograd f16x2] level {l}", factor=2.5)
