"""The fp16 two-term Winograd kernel in a chain (csrc/m4d_wino_f16.hip, m4d_conv3x3_winof16_bias_act_pm): a layer writes the
per-pixel maxima of its output, the next one reads them instead of scanning its halo.  The maxima are what the scan would find,
and every output is the scanning entry's, bit for bit -- on ragged maps, on adversarial inputs, against the bits recorded on the
commit before the hand-over existed (tools/gen_wino_handover_golden.py), and in the model, eager and graph-replayed."""
import functools
import os

import numpy as np
import pytest
import torch

from m4depth_amd import synthetic as S
from helpers import F, to_dev, npy
from tools import gen_wino_handover_golden as G

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wino_f16_chain_parent.npz")
FINITE_MAX = 0x7f7fffff


@functools.lru_cache(maxsize=None)
def _packed(dev, zero_bias=False):
    layers = G.chain_weights()
    if zero_bias:
        layers = [(k, np.zeros_like(b)) for k, b in layers]
    return G.pack_chain(layers, dev)


def _bits(t):
    return npy(t.contiguous().view(torch.int32))


def _assert_chain_bitwise(xd, packed, what, nonfinite=False):
    """Every layer's output with the hand-over = the same chain through the scanning entry, as int32 views.  ``nonfinite``: the
    positions of NaN and of Inf are identical and every finite value is bitwise equal."""
    want = G.run_chain(xd, packed)
    got = G.run_chain(xd, packed, handover=True)
    assert len(got) == len(want) == len(G.CHAIN) - 1
    for i, (g, w) in enumerate(zip(got, want)):
        gb, wb = _bits(g), _bits(w)
        if nonfinite:
            gn, wn = npy(g), npy(w)
            assert np.array_equal(np.isnan(gn), np.isnan(wn)), (what, i, "NaN positions")
            assert np.array_equal(np.isinf(gn), np.isinf(wn)) and np.array_equal(gn == np.inf, wn == np.inf), (what, i, "Inf positions")
            fin = np.isfinite(wn)
            assert np.array_equal(gb[fin], wb[fin]), (what, i, int((gb[fin] != wb[fin]).sum()))
        else:
            assert np.array_equal(gb, wb), (what, f"layer {i}", int((gb != wb).sum()), "elements differ")
    return want, got


def _reference_maxima(y, groups):
    """uint32 [b,h,w,groups]: per pixel and group of 64 channels the largest min(bits(|y|), 0x7f7fffff), NaN counting as 0."""
    u = y.view(np.uint32) & np.uint32(0x7fffffff)
    u = np.where(u > np.uint32(0x7f800000), np.uint32(0), np.minimum(u, np.uint32(FINITE_MAX)))
    full = np.zeros(y.shape[:3] + (groups * 64,), np.uint32)
    full[..., :y.shape[3]] = u
    return full.reshape(y.shape[:3] + (groups, 64)).max(axis=-1)


@pytest.mark.parametrize("cout", [32, 40, 64, 66, 96, 128])
def test_maxima_are_the_scans(dev, cout):
    """pm_out against a numpy reference computed from the stored output: the exponent field everywhere, the full bits wherever
    the maximum is a normal number; every element is written (the buffer starts as a sentinel); the output is the scanning
    entry's.  Cout 40 = a full unit with padded channels, 66 = a half unit with 2 real channels."""
    from m4depth_amd import network_ops as nops
    from m4depth_amd._lib import lib, dptr, check, stream_ptr
    for cin in (32, 64, 128):
        rng = np.random.default_rng(1000 * cin + cout)
        k = (rng.standard_normal([3, 3, cin, cout]) * np.sqrt(2.0 / (9 * cin))).astype(F)
        bias = (0.1 * rng.standard_normal([cout])).astype(F)
        wu, cpad = nops.pack_conv_weights_winof16(k)
        wd, bd = torch.from_numpy(wu.view(np.int16)).to(dev), to_dev(bias, dev)
        for b, h, w in G.MAPS:
            x = rng.standard_normal([b, h, w, cin]).astype(F)
            x *= np.exp2(rng.integers(-12, 13, size=(b, h, w, 1))).astype(F)        # pixel maxima over many exponents
            x[0, h // 2, w // 2] = 0.0
            xd = to_dev(x, dev)
            want = nops.conv3x3_winof16_bias_act(xd, wd, bd, cout, cpad, 0.1)
            out = torch.empty_like(want)
            pm = torch.full((b, h, w, cpad // 64), -559038737, dtype=torch.int32, device=dev)
            check(lib.m4d_conv3x3_winof16_bias_act_pm(dptr(xd), dptr(wd, "w", torch.int16), dptr(bd), b, h, w, cin, cout, cpad, 0.1,
                                                      dptr(out), None, dptr(pm, "pm", torch.int32), 0, 16, stream_ptr()), "pm")
            assert np.array_equal(_bits(out), _bits(want)), (cin, cout, (b, h, w))
            got = npy(pm).view(np.uint32)
            ref = _reference_maxima(npy(out), cpad // 64)
            assert np.array_equal(got >> 23, ref >> 23), (cin, cout, (b, h, w), int(((got >> 23) != (ref >> 23)).sum()))
            normal = ref >= np.uint32(0x00800000)
            assert normal.any() and np.array_equal(got[normal], ref[normal]), (cin, cout, (b, h, w))


@pytest.mark.parametrize("shape", G.MAPS)
def test_chain_is_bitwise_the_scanning_chain(dev, shape):
    """64 -> 128 -> 96 -> 64 -> 32: the first layer scans and writes maxima, three layers read and write, the last one reads."""
    xd = to_dev(G.chain_input(shape), dev)
    _assert_chain_bitwise(xd, _packed(dev), shape)


def _adversarial(case):
    """(first-layer input [2,20,36,64], zero biases?, non-finite?)"""
    x = G.chain_input(G.GOLDEN_MAP).copy()
    b, h, w, c = x.shape
    rng = np.random.default_rng(5)
    if case == "zero_tile":
        x[0, :18, 15:34] = 0.0                                      # the whole halo of tile (0, 1) of image 0, and a zero image
        x[1] = 0.0
    elif case == "magnitudes":
        tile_exp = rng.integers(-20, 21, size=(b, -(-h // 16), -(-w // 16)))
        x = x * np.exp2(np.repeat(np.repeat(tile_exp, 16, 1), 16, 2)[:, :h, :w, None]).astype(F)
        x[0, 2:14, 2:14] *= F(2.0 ** -20)                           # inside one tile: 2^-20 .. 2^20
        x[0, 6, 7, :] = F(2.0 ** 20)
        x[1, 3:6, 20:24, ::3] *= F(2.0 ** 19)
    elif case == "huge":
        x = x * F(1e30)
    elif case == "denormals":
        x[0] *= F(1e-40)                                            # a denormal image: with zero biases the handed-over tensors
        x[1, :, 18:] *= F(1e-39)                                    # are denormal or zero too; denormal next to normal pixels
    elif case == "nonfinite":
        x[0, 2, 2, 3] = np.inf
        x[1, 10, 30, :] = -np.inf
        x[1, 17, 3, 17] = np.nan
        x[0, 19, 35, 5] = np.nan
    return x.astype(F), case in ("denormals", "magnitudes"), case == "nonfinite"


@pytest.mark.parametrize("case", ["zero_tile", "magnitudes", "huge", "denormals", "nonfinite"])
def test_chain_on_adversarial_inputs(dev, case):
    x, zero_bias, nonfinite = _adversarial(case)
    want, got = _assert_chain_bitwise(to_dev(x, dev), _packed(dev, zero_bias), case, nonfinite)
    if nonfinite:                                                   # Inf and NaN did reach the handed-over tensors
        assert all((~np.isfinite(npy(t))).any() and np.isfinite(npy(t)).any() for t in want[:-1])
        assert np.isnan(npy(want[0])).any()
    if case == "denormals":
        assert ((np.abs(x) > 0) & (np.abs(x) < np.finfo(F).tiny)).any()


def test_chain_matches_the_parent_golden(dev):
    """The chain's last output on [2,20,36], scanning and handed over, is what the scanning kernel computed before the
    hand-over existed: this pins the scanning path itself."""
    want = np.load(GOLDEN)["out"]
    xd = to_dev(G.chain_input(G.GOLDEN_MAP), dev)
    for handover in (False, True):
        out = G.run_chain(xd, _packed(dev), handover=handover)[-1]
        assert np.array_equal(_bits(out), want.view(np.int32)), f"handover={handover}"


def test_model_depth_is_bitwise_with_and_without_handover(dev, monkeypatch):
    """A 3-level model on 64x96 frames with the Winograd layers dispatched: the depth with the switch on and off is bitwise
    equal, eager and graph-replayed; with the switch on layers did read maxima."""
    from m4depth_amd import network as net
    from m4depth_amd import network_ops as nops
    import m4depth_amd as M
    monkeypatch.setattr(net, "wino6_min_workgroups", 1)
    monkeypatch.setattr(net, "lat_conv_max_pixels", 0)
    monkeypatch.setattr(net, "_WINO_HANDOVER_MIN_TILES", 1)
    L, H, Wd, T, b = 3, 64, 96, 2, 1
    W = S.init_weights(L, seed=8)
    samples, cam = S.make_sequence(b, T, H, Wd, seed=31)
    d = {k: torch.stack([to_dev(s[k], dev) for s in samples], dim=1) for k in ("depth", "RGB_im", "rot", "trans")}
    d["new_traj"] = torch.stack([torch.from_numpy(s["new_traj"]) for s in samples], dim=1)
    d["camera"] = to_dev(cam, dev)
    ds, dc = to_dev(samples, dev), to_dev(cam, dev)
    reads = []
    real = nops.conv3x3_winof16_bias_act

    def counting(x, *args, **kw):
        reads.append(isinstance(x, nops.ActMaxima))
        return real(x, *args, **kw)
    monkeypatch.setattr(nops, "conv3x3_winof16_bias_act", counting)
    depth = {}
    for on in (True, False):
        monkeypatch.setattr(net, "wino_handover", on)
        del reads[:]
        model = M.M4Depth(nbre_levels=L)
        model.load_numpy_weights(W, dev)
        depth[on, "eager"] = model([ds, dc])["depth"].clone()
        assert reads and any(reads) == on, (on, reads)
        model.reset_state()
        runner = net.GraphedSequence(model, d, autotune=False)
        depth[on, "graph"] = runner(d).clone()
        assert torch.equal(runner(d), depth[on, "graph"])
    ref = _bits(depth[False, "eager"])
    assert np.isfinite(npy(depth[False, "eager"])).all()
    for key, t in depth.items():
        assert np.array_equal(_bits(t), ref), key
