"""Host packer of the fp16 two-term latency-first convolution (network_ops.pack_conv_weights_lat_f16): the two fp16 parts
and the per-output-channel exponent reassemble every float32 weight to within the dropped lo x lo term's bound, in the
fragment order of pack_conv_weights_lat.  No GPU."""
import numpy as np
import pytest


def _unpack(wp, cin, cout):
    nch, ng = -(-cin // 16), -(-cout // 32)
    n_frag = ng * nch * 9 * 2 * 64 * 8
    assert wp.dtype == np.uint16 and wp.size == n_frag + ng * 32
    parts = wp[:n_frag].view(np.float16).reshape(ng, nch, 9, 2, 2, 32, 8)   # group, chunk, tap, part, k_half, n, e
    texp = wp[n_frag:].view(np.int16).astype(np.int64)
    # -> part, tap, chunk, k_half, e, group, n  -> [part][tap][Cin padded][Cout padded]
    full = parts.transpose(3, 2, 1, 4, 6, 0, 5).reshape(2, 9, nch * 16, ng * 32).astype(np.float64)
    return full[0], full[1], texp


@pytest.mark.parametrize("cin,cout,seed", [(472, 128, 0), (128, 96, 1), (100, 40, 2), (16, 5, 3), (64, 32, 4)])
def test_pack_conv_weights_lat_f16_reassembles(cin, cout, seed):
    from m4depth_amd import network_ops as nops
    rng = np.random.default_rng(seed)
    k = (rng.standard_normal([3, 3, cin, cout]) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    k[..., 0] *= np.float32(2.0 ** -30)                 # a tiny output channel and a large one: per-channel exponents
    if cout > 1:
        k[..., 1] *= np.float32(2.0 ** 20)
    hi, lo, texp = _unpack(nops.pack_conv_weights_lat_f16(k), cin, cout)
    w = np.zeros((9, hi.shape[1], hi.shape[2]), np.float64)
    w[:, :cin, :cout] = k.reshape(9, cin, cout)
    amax = np.abs(w).max(axis=(0, 1))
    live = amax > 0
    # 2^t amax in [2^14, 2^15): the scaled weights use fp16's range, the hi part stays finite
    assert np.all(np.ldexp(amax[live], texp[live]) < 2.0 ** 15) and np.all(np.ldexp(amax[live], texp[live]) >= 2.0 ** 14)
    assert np.all(texp[~live] == 0) and np.all(hi[..., ~live] == 0) and np.all(lo[..., ~live] == 0)
    scaled = w * np.ldexp(1.0, texp)[None, None, :]
    assert np.array_equal(hi, scaled.astype(np.float16).astype(np.float64))          # hi = fp16(2^t w), round to nearest
    rec = hi + lo
    # |2^t w - hi - lo| <= 2^-11 |2^t w - hi| + fp16's smallest subnormal step / 2 <= 2^-22 |2^t w| + 2^-25
    assert np.all(np.abs(scaled - rec) <= 2.0 ** -22 * np.abs(scaled) + 2.0 ** -25)
    # the padding is zero
    assert np.all(hi[:, cin:, :] == 0) and np.all(hi[:, :, cout:] == 0)


def test_pack_conv_weights_lat_f16_layout_matches_bf16x3():
    """Fragment order: the same (group, chunk, tap, lane, element) slots as pack_conv_weights_lat, two parts instead of three."""
    from m4depth_amd import network_ops as nops
    cin, cout = 48, 64
    k = np.zeros([3, 3, cin, cout], np.float32)
    k[1, 2, 21, 37] = 1.0                               # tap 5, chunk 1, channel 5 (k_half 0, e 5), group 1, n 5
    wp = nops.pack_conv_weights_lat_f16(k)
    n_frag = 2 * 3 * 9 * 2 * 64 * 8
    frag = wp[:n_frag].view(np.float16).reshape(2, 3, 9, 2, 64, 8)
    nz = np.argwhere(frag != 0)
    assert nz.tolist() == [[1, 1, 5, 0, 5, 5]]
    assert float(frag[1, 1, 5, 0, 5, 5]) == 2.0 ** 14    # 2^t x 1 with t = 14
    b6 = nops.pack_conv_weights_lat(k)                  # [group][chunk][tap][3 parts][64][8] bf16
    assert np.argwhere(b6 != 0).tolist() == [[1, 1, 5, 0, 5, 5]]


def test_pack_conv_weights_lat_f16_rejects_non_finite():
    from m4depth_amd import network_ops as nops
    k = np.ones([3, 3, 16, 8], np.float32)
    k[0, 0, 0, 0] = np.inf
    with pytest.raises(ValueError):
        nops.pack_conv_weights_lat_f16(k)
