"""The trained-encoder fixture (tests/trained_cases.py) stays the stress case it is, and the host packers hold on it.  No GPU.

What the fixture is, per kernel (two-term split restated in trained_cases.two_term_split, not taken from the packers; He-init
kernels of the same shapes: exponents 16..18, at most 3 weights in 10^5 above 2^-22):

| layer                | t_n    | weights with two-term error > 2^-22 |w| (worst relative) | dead output channels | dead input channels |
| L1-L3, six kernels   | 15..17 | up to 0.06 % (2.7e-5)                                  | 0                    | 0                   |
| L4 conv2d_1, 64->96  | 17..18 | 0.08 % (2.5e-5)                                        | 0                    | 0                   |
| L4 conv2d_2, 96->96  | 17..32 | 0.06 % (7.1e-6)                                        | 11                   | 0                   |
| L5 conv2d_1, 96->128 | 17..32 | 1.1 % (8.0e-4)                                         | 43                   | 11                  |
| L5 conv2d_2, 128->128| 17..32 | 1.9 % (3.4e-3)                                         | 65                   | 43                  |
| L6 conv2d_1, 128->192| 17..32 | 0.6 % (2.1e-4)                                         | 178                  | 65                  |
| L6 conv2d_2, 192->192| 16..32 | 1.3 % (4.4e-3)                                         | 174                  | 178                 |

(dead: the channel's largest |weight| is below 1e-4; nonzero weights go down to 1.1e-12 beside channel maxima of 0.3.)"""
import numpy as np
import pytest

import trained_cases as T

F = np.float32
# (level, conv): (t_min, t_max, dead output channels, dead input channels)
TABLE = {(4, 2): (17, 32, 11, 0), (5, 1): (17, 32, 43, 11), (5, 2): (17, 32, 65, 43), (6, 1): (17, 32, 178, 65),
         (6, 2): (16, 32, 174, 178)}


@pytest.fixture(scope="module")
def tw():
    return T.trained_encoder_weights()


def test_every_tensor_passes_its_tensorflow_checksum_and_has_the_encoder_shape(tw):
    """read_bundle verifies the masked crc32c of every tensor (CheckpointReader, verify on); the byte ranges are contiguous,
    end where TensorFlow's file ends, and every committed file stays below 1 MiB; shapes are FeaturePyramid's."""
    import os
    import torch
    from m4depth_amd import network as N
    parts = T.data_parts()
    assert parts[0] == (0, T.HEAD) and os.path.getsize(T.HEAD) == 66624 and len(parts) >= 2
    assert all(os.path.getsize(p) <= 1 << 20 for _, p in parts)
    assert len(tw) == 24 and all(v.dtype == F and np.isfinite(v).all() for v in tw.values())
    torch.manual_seed(0)
    enc = N.M4Depth(nbre_levels=6).encoder
    for l, c in T.LAYERS:
        conv = (enc.conv_layers_s1 if c == 1 else enc.conv_layers_s2)[l - 1]
        o, i = conv.weight.shape[:2]
        assert tw[l, c, "kernel"].shape == (3, 3, i, o) == T.layer_shape(l, c) and tw[l, c, "bias"].shape == (o,)
        assert conv.stride == c


def test_a_changed_byte_in_the_new_ranges_is_rejected(tmp_path):
    from m4depth_amd import tf_checkpoint as TC
    parts = T.data_parts()
    off, path = parts[-1]
    raw = bytearray(open(path, "rb").read())
    raw[1000] ^= 0x01
    bad = str(tmp_path / "last")
    open(bad, "wb").write(bytes(raw))
    with pytest.raises(TC.ChecksumError):
        T.read_bundle(parts[:-1] + [(off, bad)])
    with pytest.raises(ValueError):
        T.read_bundle(parts[:-1])                                         # a missing range: loudly


def test_table_facts_of_the_fixture(tw):
    """The table of this file's docstring, as assertions: a regenerated or truncated fixture that turned benign fails here."""
    for l, c in T.LAYERS:
        k = tw[l, c, "kernel"]
        f, he = T.kernel_facts(k), T.kernel_facts(T.he_init_like(k, seed=100 * l + c))
        print(f"L{l} conv2d_{c} {k.shape[2]}->{k.shape[3]}: t {f['t_min']}..{f['t_max']}, over 2^-22: {100 * f['share']:.3f} % "
              f"(worst {f['worst']:.1e}), dead out {f['dead_out']} in {f['dead_in']}, smallest |w| {f['smallest']:.1e} | He-init: "
              f"t {he['t_min']}..{he['t_max']}, over 2^-22: {he['share']:.1e}")
        if l <= 3:
            assert 15 <= f["t_min"] and f["t_max"] <= 17 and f["share"] <= 1e-3 and f["dead_out"] == 0 and f["dead_in"] == 0
        if (l, c) in TABLE:
            assert (f["t_min"], f["t_max"], f["dead_out"], f["dead_in"]) == TABLE[l, c], (l, c, f)
        if l >= 5:
            assert f["share"] >= 0.005, (l, c, f)
            assert f["smallest"] < 1e-10 and f["worst"] > 1e-4
        # He-init, the same shape: 0.0000 -- not one weight in ten thousand (a Gaussian weight below 2^-13 of its channel's
        # maximum has its lo term in fp16's subnormal range too: 0 to 4 weights per kernel here, at most 2.7e-5), exponents 14..18
        assert he["share"] <= 5e-5 and he["dead_out"] == 0 and he["dead_in"] == 0 and 14 <= he["t_min"] and he["t_max"] <= 18
        if l >= 5:
            assert f["share"] >= 100 * he["share"]
    # a dead output channel is the next layer's dead input channel
    for a, b in zip(T.LAYERS[7:], T.LAYERS[8:]):
        dead_out = np.abs(tw[a + ("kernel",)]).max(axis=(0, 1, 2)) < T.DEAD
        dead_in = np.abs(tw[b + ("kernel",)]).max(axis=(0, 1, 3)) < T.DEAD
        assert np.array_equal(dead_out, dead_in), (a, b)
    # live output channels hold small but nonzero weights on the dead input channels
    k = tw[6, 1, "kernel"]
    live_o, dead_i = np.abs(k).max(axis=(0, 1, 2)) >= T.DEAD, np.abs(k).max(axis=(0, 1, 3)) < T.DEAD
    on_dead = np.abs(k[:, :, dead_i][..., live_o])
    assert 0 < np.median(on_dead) < 1e-4 and on_dead.max() < T.DEAD


def _stride1(k):
    """The kernel as a stride-1 layer that may take the small-map kernels (what FeaturePyramid sets on its layers)."""
    from m4depth_amd import network as N
    conv = N._Conv3x3SameTF(k.shape[3], 1)
    conv.small_maps_ok = True
    return conv


def _unpack_lat_f16(wp, cin, cout):
    nch, ng = -(-cin // 16), -(-cout // 32)
    n = ng * nch * 9 * 2 * 64 * 8
    assert wp.dtype == np.uint16 and wp.size == n + ng * 32
    parts = wp[:n].view(np.float16).reshape(ng, nch, 9, 2, 2, 32, 8)      # group, chunk, tap, part, k_half, n, e
    full = parts.transpose(3, 2, 1, 4, 6, 0, 5).reshape(2, 9, nch * 16, ng * 32).astype(np.float64)
    return full[0], full[1], wp[n:].view(np.int16).astype(np.int64)


def _unpack_winof16(wp, cpad, cin, cout):
    nch, ng = -(-cin // 16), -(-cout // 64)
    n = nch * ng * 16 * 2 * 2 * 64 * 8
    assert wp.dtype == np.uint16 and cpad == ng * 64 and wp.size == n + cpad
    parts = wp[:n].view(np.float16).reshape(nch, ng, 16, 2, 2, 2, 32, 8)  # chunk, group, pos, n-tile, part, k_half, j, e
    full = parts.transpose(4, 2, 0, 5, 7, 1, 3, 6).reshape(2, 16, nch * 16, cpad).astype(np.float64)
    return full[0], full[1], wp[n:].view(np.int16).astype(np.int64)


def _wino_u(k):
    """U = G g G^T in float64, rounded once to float32: what both Winograd split packers start from."""
    from m4depth_amd import network_ops as nops
    G = np.array(nops._WINO_G, np.float64)
    return np.einsum('ij,jkco,lk->ilco', G, k.astype(np.float64), G).reshape(16, k.shape[2], k.shape[3]).astype(F)


def _check_two_term(hi, lo, texp, w, cin, cout, what):
    """|(hi + lo) 2^-t - w| <= max(2^-22 |w|, 2^-25 2^-t): hi = fp16(2^t w) is within 2^-11 relative, lo = fp16 of the exact
    residual within 2^-11 of THAT while it is a normal fp16 number, and within half the subnormal spacing 2^-24 below."""
    full = np.zeros(hi.shape, np.float64)
    full[:, :cin, :cout] = w
    amax = np.abs(full).max(axis=(0, 1))
    live = amax > 0
    want_t = np.where(live, 15 - np.frexp(amax)[1], 0)
    assert np.array_equal(texp, want_t), what                            # stored exponents; padding channels t = 0
    assert live[:cout].all() and not live[cout:].any() and np.all(texp[cout:] == 0)
    assert np.all(hi[:, cin:, :] == 0) and np.all(lo[:, cin:, :] == 0) and np.all(hi[:, :, cout:] == 0) and np.all(lo[:, :, cout:] == 0)
    inv = np.ldexp(1.0, -texp)[None, None, :]
    err = np.abs((hi + lo) * inv - full)
    bound = np.maximum(2.0 ** -22 * np.abs(full), 2.0 ** -25 * inv)
    assert np.all(err <= bound), (what, float((err / bound).max()))
    assert np.isfinite(hi).all() and np.abs(hi).max() <= 2.0 ** 15         # (|2^t w| < 2^15 may round up to it: finite in fp16)
    return int(texp[:cout].max()), float((lo != 0).mean()), int(((lo != 0) & (np.abs(lo) < 2.0 ** -14)).sum())


def test_f16_packers_reconstruct_every_trained_kernel(tw):
    """pack_conv_weights_lat_f16 and pack_conv_weights_winof16, fragment order inverted, on every trained kernel whose shape the
    layout admits (_Conv3x3SameTF.can_use as a stride-1 layer): bound derived in _check_two_term, exponents, zero padding."""
    from m4depth_amd import network_ops as nops
    n_lat = n_wino = 0
    for l, c in T.LAYERS:
        k = tw[l, c, "kernel"]
        cin, cout = k.shape[2:]
        conv = _stride1(k)
        if conv.can_use("lat_f16", cin):
            hi, lo, texp = _unpack_lat_f16(nops.pack_conv_weights_lat_f16(k), cin, cout)
            tmax, _, sub = _check_two_term(hi, lo, texp, k.reshape(9, cin, cout).astype(np.float64), cin, cout, (l, c, "lat_f16"))
            print(f"L{l} conv2d_{c} lat_f16: largest exponent {tmax}, {sub} subnormal lo terms")
            assert sub > 0 and (tmax == 32 or (l, c) not in TABLE)
            n_lat += 1
        if conv.can_use("winof16", cin):
            wp, cpad = nops.pack_conv_weights_winof16(k)
            hi, lo, texp = _unpack_winof16(wp, cpad, cin, cout)
            _check_two_term(hi, lo, texp, _wino_u(k).astype(np.float64), cin, cout, (l, c, "winof16"))
            n_wino += 1
    assert n_lat == 11 and n_wino == 9                                     # all but 3 -> 16; from 32 -> 32 on


def test_bf16x3_packers_are_exact_on_every_trained_kernel(tw):
    """pack_conv_weights_wino6 / _lat / _small6: the three bf16 terms sum to the float32 value exactly, down to weights of 1e-12."""
    from m4depth_amd import network_ops as nops

    def widen(u16):
        return (u16.astype(np.uint32) << 16).view(F).astype(np.float64)
    seen = set()
    for l, c in T.LAYERS:
        k = tw[l, c, "kernel"]
        cin, cout = k.shape[2:]
        conv = _stride1(k)
        nch = -(-cin // 16)
        if conv.can_use("wino6", cin):
            w, cpad = nops.pack_conv_weights_wino6(k)
            p = w.reshape(nch, cpad // 64, 16, 2, 3, 2, 32, 8).transpose(4, 2, 0, 5, 7, 1, 3, 6).reshape(3, 16, nch * 16, cpad)
            full = np.zeros((16, nch * 16, cpad), F)
            full[:, :cin, :cout] = _wino_u(k)
            assert np.array_equal(widen(p).sum(axis=0), full.astype(np.float64)), (l, c, "wino6")
            seen.add("wino6")
        if conv.can_use("lat", cin):
            ng = -(-cout // 32)
            p = nops.pack_conv_weights_lat(k).reshape(ng, nch, 9, 3, 2, 32, 8).transpose(3, 2, 1, 4, 6, 0, 5).reshape(3, 9, nch * 16, ng * 32)
            full = np.zeros((9, nch * 16, ng * 32), F)
            full[:, :cin, :cout] = k.reshape(9, cin, cout)
            assert np.array_equal(widen(p).sum(axis=0), full.astype(np.float64)), (l, c, "lat")
            seen.add("lat")
        if conv.can_use("small6", cin):
            w, cpad = nops.pack_conv_weights_small6(k)
            p = w.transpose(3, 1, 0, 4, 2).reshape(3, 9, nch * 16, cpad)
            full = np.zeros((9, nch * 16, cpad), F)
            full[:, :cin, :cout] = k.reshape(9, cin, cout)
            assert np.array_equal(widen(p).sum(axis=0), full.astype(np.float64)), (l, c, "small6")
            seen.add("small6")
    assert seen == {"wino6", "lat", "small6"}
    assert min(float(np.abs(v[v != 0]).min()) for (l, c, p), v in tw.items() if p == "kernel") < 2e-12


def test_trained_activations_are_the_stress_case():
    """The 12 layer inputs: the loop that keeps them gives oracle.feature_pyramid's outputs bit for bit; at levels 5 and 6 the
    per-channel maxima of the stride-1 layer's input span at least 2^15 (measured 2^18.1 and 2^15.1) under a scale all channels
    share; at least 40 % of the channels of both level-6 inputs are near-constant (65 / 128 and 178 / 192, at leaky_relu(bias) of a
    dead channel); live channels are post-leaky-ReLU, not zero-mean."""
    from oracle import m4depth_oracle as O
    from m4depth_amd import synthetic
    acts = T.trained_activations()
    h, w, seed = T.ACTIVATION_CASE
    assert sorted(acts) == T.LAYERS
    for (l, c), a in acts.items():
        assert a.dtype == F and a.shape == (1, -(-h // 2 ** (l - 1)), -(-w // 2 ** (l - 1)), T.layer_shape(l, c)[2]) and np.isfinite(a).all()
    W = T.encoder_weight_dict()
    ref = O.feature_pyramid(synthetic.make_sequence(1, 1, h, w, seed=seed)[0][0]["RGB_im"], W, 6)
    for got, want in zip(T._cache["pyramid"], ref):
        assert np.array_equal(got, want)
    tw = T.trained_encoder_weights()
    for (l, c), a in acts.items():
        m = np.abs(a).max(axis=(0, 1, 2)).astype(np.float64)
        span = a.max(axis=(0, 1, 2)).astype(np.float64) - a.min(axis=(0, 1, 2))
        flat = span <= 1e-3 * m.max()
        print(f"L{l} conv2d_{c} input {a.shape[1]}x{a.shape[2]}x{a.shape[3]}: channel maxima {m.min():.2e} .. {m.max():.2e} "
              f"(2^{np.log2(m.max() / m.min()):.1f}), {int(flat.sum())} near-constant channels, mean {a.mean():+.3f}, {100 * (a < 0).mean():.0f} % negative")
        if l >= 5 and c == 1:
            assert m.max() / m.min() >= 2.0 ** 15, (l, c)
        if l == 6:
            assert flat.mean() >= 0.4, (l, c)
        if l >= 5:
            # the near-constant channels are the previous layer's dead output channels, at leaky_relu(bias) to 1e-3 of the map's scale
            pl, pc = T.LAYERS[T.LAYERS.index((l, c)) - 1]
            dead = np.abs(tw[pl, pc, "kernel"]).max(axis=(0, 1, 2)) < T.DEAD
            assert np.array_equal(flat, dead), (l, c)
            b = tw[pl, pc, "bias"][dead].astype(np.float64)
            assert np.max(np.abs(a[..., dead].astype(np.float64) - np.where(b > 0, b, 0.1 * b))) <= 1e-3 * m.max()
            live = a[..., ~dead]
            assert abs(live.mean()) > 0.05 * np.abs(live).mean()               # not zero-mean
