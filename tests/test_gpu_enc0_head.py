"""The three launches at the head of every step -- enc0_stats_kernel<2>, enc0_moments_finalize_kernel, enc0_fused_kernel
(m4d_enc_level0_stats / _apply / _fwd) -- after their staging was rewritten to keep every load in flight: the data movement
changed, the arithmetic did not, so

  * the results are the bits recorded from the library before that change (tests/golden/enc0_head_parent.npz, written by
    tools/gen_enc0_head_golden.py, which also holds the seeded inputs' definition);
  * the shapes at which staging can go wrong (smaller than a tile, one tile plus a row and a column with row starts off
    16-byte alignment, odd sizes, two and three statistics tiles per workgroup with a ragged last round) agree with the
    oracle within the bars of test_gpu_ops.test_encoder_level0_without_intermediate (fused output: max error
    < 2e-5 x max(1, |ref|max)) and test_gpu_ops.test_encoder_level0_statistics_single_pass (mean: |m - mean| / (|mean| + sd)
    < 2e-6, variance: relative error < 2e-5, against float64 moments of the oracle's convolution);
  * batch, FrameStack and statistics-up-front invariances hold bit for bit;
  * nothing is written outside mean, var, the partial workspace and the output."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import m4depth_oracle as O
from helpers import F, to_dev, npy
from tools import gen_enc0_head_golden as G

pytestmark = pytest.mark.gpu

SMALL = [(1, 5, 7), (2, 9, 129), (1, 37, 53), (3, 16, 130)]
MULTI_TILE = [(1, 264, 1024), (1, 520, 1024)]      # 264 / 520 statistics tiles: 2 per workgroup / 3 with a ragged last round


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _inputs(b, h, w):
    """(img, k1, b1, sc, bs, k2, b2): He-normal layers with biases, seeded by the shape."""
    rng = np.random.default_rng(100003 * b + 1009 * h + w)
    img = rng.random([b, h, w, 3]).astype(F)
    k1 = (rng.standard_normal([3, 3, 3, 16]) * np.sqrt(2.0 / 27)).astype(F)
    b1 = (0.1 * rng.standard_normal([16])).astype(F)
    k2 = (rng.standard_normal([3, 3, 16, 16]) * np.sqrt(2.0 / 144)).astype(F)
    b2 = (0.1 * rng.standard_normal([16])).astype(F)
    sc = (1.0 + 0.1 * rng.standard_normal([16])).astype(F)
    bs = (0.1 * rng.standard_normal([16])).astype(F)
    return img, k1, b1, sc, bs, k2, b2


@functools.lru_cache(maxsize=None)
def _conv1(b, h, w):
    img, k1, b1 = _inputs(b, h, w)[:3]
    return O.conv2d_same(img, k1, b1, 1)


def _check_moments(mean, var, y, what):
    y = y.astype(np.float64)
    mean_ref, var_ref = y.mean(axis=(1, 2)), y.var(axis=(1, 2))
    m, v = npy(mean).astype(np.float64), npy(var).astype(np.float64)
    e_m = np.max(np.abs(m - mean_ref) / (np.abs(mean_ref) + np.sqrt(var_ref)))
    e_v = np.max(np.abs(v - var_ref) / var_ref)
    print(f"{what}: mean error {e_m:.2e} (bar 2e-6), variance relative error {e_v:.2e} (bar 2e-5)")
    assert e_m < 2e-6, (what, e_m)
    assert e_v < 2e-5, (what, e_v)


# ------------------------------------------------------------------------------------------- the bits before the change
@pytest.fixture(scope="module")
def parent(golden):
    return golden("enc0_head_parent")


@pytest.mark.parametrize("name", list(G.CASES))
def test_head_bits_are_those_before_the_staging_change(dev, parent, name):
    """mean, var and the fused output of the seeded cases of tools/gen_enc0_head_golden.py, bit for bit; one case also read in
    place as a [bsz = 1, T = b] FrameStack."""
    from m4depth_amd import network_ops as nops
    want = {k: torch.from_numpy(parent[f"{name}.{k}"]).to(dev) for k in ("mean", "var", "out")}
    mean, var, out = G.run_case(name, dev)
    assert _same_bits(mean, want["mean"]), f"{name}: mean"
    assert _same_bits(var, want["var"]), f"{name}: var"
    assert _same_bits(out, want["out"]), f"{name}: fused output"
    if name == G.FRAMESTACK_CASE:
        img, *wts = to_dev(list(G.case_inputs(name)), dev)
        stack = nops.FrameStack(img[None])
        m_s, v_s = nops.encoder_level0_stats(stack, wts[0], wts[1])
        assert _same_bits(m_s, want["mean"]) and _same_bits(v_s, want["var"]), f"{name}: statistics through a FrameStack"
        assert _same_bits(nops.encoder_level0(stack, *wts, 0.1), want["out"]), f"{name}: fused output through a FrameStack"


# ------------------------------------------------------------------------------------------- shapes against the oracle
@pytest.mark.parametrize("b,h,w", SMALL)
def test_fused_output_at_staging_edge_shapes(dev, b, h, w):
    from m4depth_amd import network_ops as nops
    img, k1, b1, sc, bs, k2, b2 = _inputs(b, h, w)
    t = O.leaky_relu(O.domain_normalization(_conv1(b, h, w), sc, bs), 0.1)
    ref = O.leaky_relu(O.conv2d_same(t, k2, b2, 2), 0.1)
    got = nops.encoder_level0(*to_dev([img, k1, b1, sc, bs, k2, b2], dev), 0.1)
    assert got.shape == ref.shape
    err = np.max(np.abs(npy(got) - ref))
    print(f"fused {b}x{h}x{w}: max error {err:.2e} (bar {2e-5 * max(1.0, np.abs(ref).max()):.2e})")
    assert err < 2e-5 * max(1.0, np.abs(ref).max()), err


@pytest.mark.parametrize("b,h,w", SMALL + MULTI_TILE)
def test_statistics_at_staging_edge_shapes(dev, b, h, w):
    from m4depth_amd import network_ops as nops
    img, k1, b1 = _inputs(b, h, w)[:3]
    args = to_dev([img, k1, b1], dev)
    mean, var = nops.encoder_level0_stats(*args)
    _check_moments(mean, var, _conv1(b, h, w), f"statistics {b}x{h}x{w}")
    m2, v2 = nops.encoder_level0_stats(*args)
    assert _same_bits(mean, m2) and _same_bits(var, v2)                     # run-to-run identical


# ------------------------------------------------------------------------------------------- invariances, bit for bit
def test_image_in_a_batch_equals_image_alone(dev):
    from m4depth_amd import network_ops as nops
    img, *wts = to_dev(list(_inputs(3, 16, 130)), dev)
    mean, var = nops.encoder_level0_stats(img, wts[0], wts[1])
    out = nops.encoder_level0(img, *wts, 0.1)
    for j in range(img.shape[0]):
        one = img[j:j + 1].contiguous()
        mj, vj = nops.encoder_level0_stats(one, wts[0], wts[1])
        assert _same_bits(mean[j:j + 1], mj) and _same_bits(var[j:j + 1], vj), j
        assert _same_bits(out[j:j + 1], nops.encoder_level0(one, *wts, 0.1)), j


def test_dense_batch_equals_framestack_view(dev):
    """Frames 1..2 of a [2, 4] sequence batch read in place (sequence stride != frame stride) = the dense batch of the same four
    images in frame-major order."""
    from m4depth_amd import network_ops as nops
    img, *wts = to_dev(list(_inputs(8, 9, 129)), dev)
    seq = img.reshape(2, 4, 9, 129, 3)
    stack = nops.FrameStack(seq[:, 1:3])
    dense = seq[:, 1:3].transpose(0, 1).reshape(4, 9, 129, 3).contiguous()      # image t * bsz + i = seq[i, 1 + t]
    m_d, v_d = nops.encoder_level0_stats(dense, wts[0], wts[1])
    m_s, v_s = nops.encoder_level0_stats(stack, wts[0], wts[1])
    assert _same_bits(m_d, m_s) and _same_bits(v_d, v_s)
    assert _same_bits(nops.encoder_level0(dense, *wts, 0.1), nops.encoder_level0(stack, *wts, 0.1))


def test_statistics_of_four_frames_applied_to_two(dev):
    """m4d_enc_level0_stats over all four frames of a sequence, m4d_enc_level0_apply on the last two with their rows = what
    m4d_enc_level0_fwd computes on those two."""
    from m4depth_amd import network_ops as nops
    img, *wts = to_dev(list(_inputs(4, 37, 53)), dev)
    seq = img[None]                                                            # [1, 4, h, w, 3]
    mean, var = nops.encoder_level0_stats(nops.FrameStack(seq), wts[0], wts[1])
    got = nops.encoder_level0(nops.FrameStack(seq[:, 2:4]), *wts, 0.1, stats=(mean[2:4].contiguous(), var[2:4].contiguous()))
    assert _same_bits(got, nops.encoder_level0(img[2:4].contiguous(), *wts, 0.1))


# ------------------------------------------------------------------------------------------- guard regions
GUARD = 256                                          # floats on either side of every buffer the kernels write
SENTINEL = -7.25e9


def _guarded(n, dev):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n):
    want = torch.full((GUARD,), SENTINEL, dtype=torch.float32, device=buf.device)
    return _same_bits(buf[:GUARD], want) and _same_bits(buf[GUARD + n:], want)


@pytest.mark.parametrize("b,h,w", [(1, 5, 7), (2, 9, 129), (1, 37, 53), (3, 16, 130)])
def test_nothing_is_written_outside_the_outputs(dev, b, h, w):
    """mean, var, the partial workspace and the output each sit between two guard regions; the library is called on the raw
    pointers.  The results are those of the wrappers; the guards keep their bits."""
    from m4depth_amd import network_ops as nops
    from m4depth_amd._lib import lib, stream_ptr
    img, k1, b1, sc, bs, k2, b2 = to_dev(list(_inputs(b, h, w)), dev)
    oh, ow = (h + 1) // 2, (w + 1) // 2
    n_ws = int(lib.m4d_dinl_workspace_floats(b, 16))
    ws_buf, ws = _guarded(n_ws, dev)
    mean_buf, mean = _guarded(b * 16, dev)
    var_buf, var = _guarded(b * 16, dev)
    out_buf, out = _guarded(b * oh * ow * 16, dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.m4d_enc_level0_stats(p(img), b, h * w * 3, 0, p(k1), p(b1), b, h, w, p(ws), p(mean), p(var), stream_ptr()) == 0
    assert lib.m4d_enc_level0_apply(p(img), b, h * w * 3, 0, p(k1), p(b1), p(mean), p(var), p(sc), p(bs), 0.1, p(k2), p(b2), 0.1,
                                    b, h, w, p(out), stream_ptr()) == 0
    torch.cuda.synchronize()
    m_w, v_w = nops.encoder_level0_stats(img, k1, b1)
    assert _same_bits(mean.reshape(b, 16), m_w) and _same_bits(var.reshape(b, 16), v_w)
    assert _same_bits(out.reshape(b, oh, ow, 16), nops.encoder_level0(img, k1, b1, sc, bs, k2, b2, 0.1))
    for what, buf, n in (("workspace", ws_buf, n_ws), ("mean", mean_buf, b * 16), ("var", var_buf, b * 16),
                         ("output", out_buf, b * oh * ow * 16)):
        assert _guards_intact(buf, n), f"{what}: a guard region was written"
    # m4d_enc_level0_fwd keeps mean / var at the end of its workspace: the same guards around the whole of it
    ws_buf.fill_(SENTINEL)
    out_buf.fill_(SENTINEL)
    assert lib.m4d_enc_level0_fwd(p(img), b, h * w * 3, 0, p(k1), p(b1), p(sc), p(bs), 0.1, p(k2), p(b2), 0.1, b, h, w, p(ws), p(out),
                                  stream_ptr()) == 0
    torch.cuda.synchronize()
    assert _guards_intact(ws_buf, n_ws) and _guards_intact(out_buf, b * oh * ow * 16), "m4d_enc_level0_fwd: a guard region was written"
    assert _same_bits(ws[n_ws - 2 * b * 16:n_ws - b * 16].reshape(b, 16), m_w) and _same_bits(ws[n_ws - b * 16:].reshape(b, 16), v_w)
