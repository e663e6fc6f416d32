"""The fp16 two-term latency-first convolution (csrc/m4d_convlat_f16.hip, conv_arith "f16x2"): error to float64 against the
bf16x3 latency-first kernel on every default-dispatched geometry, range handling (power-of-two scales per output pixel's
3x3 window), Inf / NaN, and bit-level determinism, including partial-sum slabs handed between the two arithmetics."""
import numpy as np
import pytest
import torch

from oracle import m4depth_oracle as O
from helpers import F, to_dev, npy

pytestmark = pytest.mark.gpu


def _nops():
    from m4depth_amd import network_ops as nops
    return nops


def _weights(k, dev):
    nops = _nops()
    w16 = torch.from_numpy(nops.pack_conv_weights_lat_f16(k).view(np.int16)).to(dev)
    w6 = torch.from_numpy(nops.pack_conv_weights_lat(k).view(np.int16)).to(dev)
    return w16, w6


def _dense(out):
    return out.dense() if isinstance(out, _nops().PartialAct) else out


def _act(r, slope):
    return np.where(r > 0, r, r * r.dtype.type(slope))


def _case(rng, b, h, w, cin, cout):
    x = rng.standard_normal([b, h, w, cin]).astype(F)
    k = (rng.standard_normal([3, 3, cin, cout]) * np.sqrt(2.0 / (9 * cin))).astype(F)
    bias = (0.1 * rng.standard_normal([cout])).astype(F)
    return x, k, bias


# (b, h, w, cin, cout, final, cfg_b): the refiner layers of levels 6 / 5 / 4 at batch 1 and 2 wherever the model dispatches them
# to the latency-first kernel (first layer on the zero-padded input, 96 -> 64 and 64 -> 32 handing partial slabs on), and the
# coarse stride-1 encoder layers on an encoder batch of two frames, configured from the per-image grid x the sequence batch
# (cfg_b: 1, as in bench.py, and 2)
_REFINER = [(6, 20, 472), (12, 40, 240), (24, 80, 240)]
GEOMS = [(b, h, w, ci, co, i < 3, b) for b in (1, 2) for (h, w, c0) in _REFINER if b * h * w <= 2048
         for i, (ci, co) in enumerate(zip([c0, 128, 128, 96, 64], [128, 128, 96, 64, 32]))] + \
        [(2, h, w, ci, co, False, cb) for (h, w, ci, co) in [(24, 80, 96, 128), (12, 40, 128, 192)] for cb in (1, 2)
         if cb * h * w <= 2048]


@pytest.mark.parametrize("b,h,w,cin,cout,final,cfg_b", GEOMS)
def test_lat_f16_accuracy(dev, b, h, w, cin, cout, final, cfg_b):
    """Default configuration (network_ops.lat_config): mean and max |error| to float64 at most 1.25x the bf16x3 latency-first
    kernel's on the same inputs; both within the float32 tolerance of the oracle.  All three errors are printed."""
    nops = _nops()
    rng = np.random.default_rng(cin * 13 + cout + 7 * b + h)
    x, k, bias = _case(rng, b, h, w, cin, cout)
    xd, bd = to_dev(x, dev), to_dev(bias, dev)
    w16, w6 = _weights(k, dev)
    cfg = nops.lat_config(cfg_b, h, w, cin, cout, final)
    got = npy(_dense(nops.conv3x3_lat_f16(xd, w16, bd, cout, 0.1, config=cfg))).astype(np.float64)
    bf = npy(_dense(nops.conv3x3_lat(xd, w6, bd, cout, 0.1, config=cfg))).astype(np.float64)
    ref32 = _act(O.conv2d_same(x, k, bias, 1), 0.1).astype(F)
    with O.float64_reference():
        ref64 = _act(O.conv2d_same(x.astype(np.float64), k.astype(np.float64), bias.astype(np.float64), 1), 0.1)
    assert np.max(np.abs(got - ref32)) < 1e-5 * max(1.0, np.abs(ref32).max())
    e16, ebf, e32 = np.abs(got - ref64), np.abs(bf - ref64), np.abs(ref32.astype(np.float64) - ref64)
    print(f"lat {b}x{h}x{w} {cin}->{cout} {cfg} (configured for batch {cfg_b}): |error| to float64 mean / max: f16x2 {e16.mean():.3e} / {e16.max():.3e}, "
          f"bf16x3 {ebf.mean():.3e} / {ebf.max():.3e}, float32 oracle {e32.mean():.3e} / {e32.max():.3e}")
    assert e16.mean() <= 1.25 * ebf.mean()
    assert e16.max() <= 1.25 * ebf.max()


def _mixed_magnitudes(rng, b, h, w, cin):
    """Signed inputs whose magnitude is 2^u, u uniform in [-20, 20], drawn per pixel (and jittered per channel): neighbours
    inside one tile differ by up to 2^40."""
    u = rng.uniform(-20, 20, [b, h, w, 1]) + rng.uniform(-1, 1, [b, h, w, cin])
    return (np.exp2(u) * np.sign(rng.standard_normal([b, h, w, cin]))).astype(F)


@pytest.mark.parametrize("b,h,w,cin,cout,final", [(1, 12, 40, 128, 128, True), (1, 24, 80, 96, 64, False),
                                                  (1, 6, 20, 472, 128, True), (2, 12, 40, 64, 32, False)])
def test_lat_f16_range(dev, b, h, w, cin, cout, final):
    """Mixed magnitudes 2^-20..2^20: each output's error relative to its own sum of |x| |w| stays in the bf16x3 kernel's class
    (the per-window scale; a tile-wide one would lose the small pixels); inputs x 1e30 stay finite and accurate."""
    nops = _nops()
    rng = np.random.default_rng(cin + cout + h)
    x = _mixed_magnitudes(rng, b, h, w, cin)
    k = (rng.standard_normal([3, 3, cin, cout]) * np.sqrt(2.0 / (9 * cin))).astype(F)
    bias = np.zeros([cout], F)
    w16, w6 = _weights(k, dev)
    cfg = nops.lat_config(b, h, w, cin, cout, final)
    with O.float64_reference():
        ref64 = O.conv2d_same(x.astype(np.float64), k.astype(np.float64), bias.astype(np.float64), 1)
        mag = O.conv2d_same(np.abs(x).astype(np.float64), np.abs(k).astype(np.float64), bias.astype(np.float64), 1)
    for scale in (1.0, 1e30):
        xd, bd = to_dev(x * F(scale), dev), to_dev(bias, dev)
        got = npy(_dense(nops.conv3x3_lat_f16(xd, w16, bd, cout, None, config=cfg))).astype(np.float64)
        bf = npy(_dense(nops.conv3x3_lat(xd, w6, bd, cout, None, config=cfg))).astype(np.float64)
        assert np.isfinite(got).all()
        r16 = np.abs(got - ref64 * scale) / (mag * scale)
        rbf = np.abs(bf - ref64 * scale) / (mag * scale)
        print(f"lat range {cin}->{cout} x{scale:g}: error / sum |x||w|: f16x2 max {r16.max():.3e} mean {r16.mean():.3e}, "
              f"bf16x3 max {rbf.max():.3e} mean {rbf.mean():.3e}")
        assert r16.max() <= max(4.0 * rbf.max(), 2.0 ** -20)
        assert r16.mean() <= max(4.0 * rbf.mean(), 2.0 ** -24)


def test_lat_f16_inf_nan(dev):
    """An Inf and a NaN input make exactly the outputs whose 3x3 window holds them non-finite, as in the bf16x3 kernel; every
    other output matches the clean input's bit for bit (the scales of other windows do not see them)."""
    nops = _nops()
    b, h, w, cin, cout = 1, 12, 40, 128, 128
    rng = np.random.default_rng(5)
    x, k, bias = _case(rng, b, h, w, cin, cout)
    w16, w6 = _weights(k, dev)
    bd = to_dev(bias, dev)
    cfg = nops.lat_config(b, h, w, cin, cout, True)
    clean = npy(nops.conv3x3_lat_f16(to_dev(x, dev), w16, bd, cout, 0.1, config=cfg))
    xb = x.copy()
    xb[0, 3, 7, 5] = np.inf
    xb[0, 9, 30, 100] = np.nan
    got = npy(nops.conv3x3_lat_f16(to_dev(xb, dev), w16, bd, cout, 0.1, config=cfg))
    bf = npy(nops.conv3x3_lat(to_dev(xb, dev), w6, bd, cout, 0.1, config=cfg))
    bad = np.zeros([b, h, w, cout], bool)
    bad[0, 2:5, 6:9, :] = True
    bad[0, 8:11, 29:32, :] = True
    assert np.array_equal(~np.isfinite(got), bad)
    assert np.array_equal(~np.isfinite(bf), bad)
    assert np.array_equal(got[~bad], clean[~bad])


@pytest.mark.parametrize("b,h,w,cin,cout", [(1, 24, 80, 240, 128), (2, 12, 40, 100, 40), (1, 13, 17, 64, 32)])
def test_lat_f16_determinism(dev, b, h, w, cin, cout):
    """Repeated calls are bit-identical; every M-tile count gives the same bits for equal (kw, s_out); a PartialAct handed on
    gives the bits of its .dense() form, to an f16x2 and to a bf16x3 consumer alike."""
    nops = _nops()
    rng = np.random.default_rng(cin * 3 + cout)
    x, k, bias = _case(rng, b, h, w, cin, cout)
    xd, bd = to_dev(x, dev), to_dev(bias, dev)
    w16, _ = _weights(k, dev)
    n_chunks = -(-cin // 16)
    same_order, tried = {}, 0
    for kw in (1, 2, 4):
        for s_out in (1, 2, 3, 4):
            if s_out > n_chunks or (s_out - 1) * (-(-n_chunks // s_out)) >= n_chunks:
                continue
            for mt in (1, 2, 4):
                if 2 * kw * nops._lat_halo_pixels(mt, 1) * 96 > 160 * 1024:
                    continue
                out = nops.conv3x3_lat_f16(xd, w16, bd, cout, 0.1, config=(mt, kw, s_out))
                t = out.slabs if isinstance(out, nops.PartialAct) else out
                again = nops.conv3x3_lat_f16(xd, w16, bd, cout, 0.1, config=(mt, kw, s_out))
                assert torch.equal(t, again.slabs if isinstance(again, nops.PartialAct) else again)
                tried += 1
                if (kw, s_out) in same_order:
                    assert torch.equal(t, same_order[(kw, s_out)]), f"mt {mt} differs bitwise at {(kw, s_out)}"
                else:
                    same_order[(kw, s_out)] = t
    assert tried >= 6
    # a chain: this layer -> (slabs) -> a 32-channel consumer, on either arithmetic
    c2 = 32
    k2 = (rng.standard_normal([3, 3, cout, c2]) * np.sqrt(2.0 / (9 * cout))).astype(F)
    b2 = to_dev((0.1 * rng.standard_normal([c2])).astype(F), dev)
    w16b, w6b = _weights(k2, dev)
    cfg = nops.lat_config(b, h, w, cin, cout, False)
    if cfg[2] == 1:
        cfg = (cfg[0], cfg[1], 2)
    part = nops.conv3x3_lat_f16(xd, w16, bd, cout, 0.1, config=cfg)
    assert isinstance(part, nops.PartialAct)
    if cout % 4 == 0:
        dense = part.dense()
        assert torch.equal(nops.conv3x3_lat_f16(part, w16b, b2, c2, 0.1, final=True),
                           nops.conv3x3_lat_f16(dense, w16b, b2, c2, 0.1, final=True))
        assert torch.equal(nops.conv3x3_lat(part, w6b, b2, c2, 0.1, final=True),
                           nops.conv3x3_lat(dense, w6b, b2, c2, 0.1, final=True))
