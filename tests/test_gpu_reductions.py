"""The reductions at the head and the tail of a step against float64: the level-0 DomainNormalization statistics
(m4d_enc_level0_stats), encoder level 0 end to end (fused and unfused heads), the two-pass DINL (m4d_dinl_fwd_padded) and
the depth metrics (m4d_depth_metrics[_strided]) -- on the inputs where a reduction loses digits: flat and dark frames with
an outlier at the centre pixel, constant and all-zero frames, degenerate sizes, means that dwarf the spread, exposures far
apart inside one batch, ratios exactly on the Delta thresholds, batches without a valid pixel.

Bars (the GPU error is printed beside each):
  * statistics: mean |m - mean| / (|mean| + sd) < 2e-6, variance relative error < 2e-5 (the bars of
    test_gpu_ops.test_encoder_level0_statistics_single_pass); all-zero frame: mean == bias, var == 0 exactly;
  * normalised outputs: max / mean |gpu - f64| <= 3x / 2x the error of a float32 evaluation, + 1e-6 / 1e-7 x the output
    scale (the maximum over a map of a few pixels is one rounding of conv1 or conv2: a few ulps of the scale).
    That evaluation is the oracle's with its mean / variance replaced by the float64 moments rounded to float32: in a flat
    region x - mean is ~1e-5 of |mean|, so the float32 mean alone costs ~1e-3 relative there in any kernel, and an absolute
    bar would measure the frame, not the kernel.  The plain float32 oracle is no yardstick on these frames: numpy sums its
    float32 mean over (h, w) one element after the other, and its error (printed) reaches 0.8 of the output scale;
  * metrics: AbsRel, SqRel, RMSE, RMSE_log relative error < 2e-5; Delta1..3 within 1 ulp (exact counts on both sides)."""
import numpy as np
import pytest
import torch

from oracle import m4depth_oracle as O
from helpers import F, to_dev, npy

pytestmark = pytest.mark.gpu

FRAMES = ["black_lit", "flat_lit", "flat_1e3", "dark_sat9", "grey_black3", "constant", "zero", "random"]
SIZES = [(384, 1280), (37, 53), (3, 5), (2, 2), (1, 7), (7, 1)]


def _frame(kind, h, w, rng):
    """[h,w,3] float32; the outliers sit on the pixel the statistics kernel takes its shift from, (h // 2, w // 2)."""
    cy, cx = h // 2, w // 2
    img = np.zeros([h, w, 3], F)
    if kind == "black_lit":
        img[cy, cx] = 1.0
    elif kind == "flat_lit":
        img[:] = 0.3
        img[cy, cx] = 1.0
    elif kind == "flat_1e3":
        img[:] = 0.3
        img[cy, cx] = 1e3
    elif kind == "dark_sat9":
        img[:] = 0.02
        img[max(cy - 4, 0):cy + 5, max(cx - 4, 0):cx + 5] = 1.0
    elif kind == "grey_black3":
        img[:] = 0.5
        img[max(cy - 1, 0):cy + 2, max(cx - 1, 0):cx + 2] = 0.0
    elif kind == "constant":
        img[:] = 0.7
    elif kind == "random":
        img[:] = rng.random([h, w, 3])
    else:
        assert kind == "zero"
    return img


def _weights(seed=5):
    """He-normal 3 -> 16 and 16 -> 16 convolutions and the DomainNormalization scale / bias."""
    rng = np.random.default_rng(seed)
    k1 = (rng.standard_normal([3, 3, 3, 16]) * np.sqrt(2.0 / 27)).astype(F)
    b1 = (0.1 * rng.standard_normal([16])).astype(F)
    k2 = (rng.standard_normal([3, 3, 16, 16]) * np.sqrt(2.0 / 144)).astype(F)
    b2 = (0.1 * rng.standard_normal([16])).astype(F)
    sc = (1.0 + 0.1 * rng.standard_normal([16])).astype(F)
    bs = (0.1 * rng.standard_normal([16])).astype(F)
    return k1, b1, k2, b2, sc, bs


def _moments_f64(img, k1, b1):
    """float64 mean / biased variance over (h, w) of the oracle's float32 conv1 output (the float32 conv is the definition;
    numpy's float32 .var of it is not a reference on these frames)."""
    y = O.conv2d_same(img, k1, b1, 1).astype(np.float64)
    mean = y.mean(axis=(1, 2))
    var = ((y - mean[:, None, None, :]) ** 2).mean(axis=(1, 2))
    return mean, var


def _check_stats(mean, var, mean_ref, var_ref, bias, what):
    m, v = npy(mean).astype(np.float64), npy(var).astype(np.float64)
    zero = var_ref == 0.0                              # only the all-zero frame: conv1 = bias on every pixel
    if zero.any():
        assert np.array_equal(m[zero], np.broadcast_to(bias.astype(np.float64), m.shape)[zero]), (what, m[zero])
        assert (v[zero] == 0.0).all(), (what, v[zero])
    nz = ~zero
    if not nz.any():
        print(f"{what}: mean == bias, var == 0 exactly")
        return
    e_m = np.max(np.abs(m - mean_ref)[nz] / (np.abs(mean_ref) + np.sqrt(var_ref))[nz])
    e_v = np.max(np.abs(v - var_ref)[nz] / var_ref[nz])
    print(f"{what}: mean error {e_m:.2e} (bar 2e-6), variance relative error {e_v:.2e} (bar 2e-5)")
    assert e_m < 2e-6, (what, e_m)
    assert e_v < 2e-5, (what, e_v)


# ---------------------------------------------------------------------------------------------------- level-0 statistics
@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("kind", FRAMES)
def test_level0_statistics_adversarial_frames(dev, kind, h, w):
    """m4d_enc_level0_stats on frames whose centre pixel (the shift of the single-pass moments) is unlike the rest of the
    frame, on constant and all-zero frames, and on sizes where the centre and the border exclusions coincide."""
    from m4depth_amd import network_ops as nops
    k1, b1 = _weights()[:2]
    img = _frame(kind, h, w, np.random.default_rng(h * 31 + w))[None]
    mean_ref, var_ref = _moments_f64(img, k1, b1)
    mean, var = nops.encoder_level0_stats(to_dev(img, dev), to_dev(k1, dev), to_dev(b1, dev))
    _check_stats(mean, var, mean_ref, var_ref, b1, f"{kind} {h}x{w}")
    m2, v2 = nops.encoder_level0_stats(to_dev(img, dev), to_dev(k1, dev), to_dev(b1, dev))
    assert torch.equal(mean, m2) and torch.equal(var, v2)                  # run-to-run identical


@pytest.mark.parametrize("h,w", [(96, 272), (37, 53)])
def test_level0_statistics_batch_independence(dev, h, w):
    """Frames with exposures up to 2^12 apart, outlier frames among normal ones: image j's statistics are those of image j
    launched alone, bit for bit; a [bsz, T] sequence read in place (FrameStack) gives the bits of the dense batch."""
    from m4depth_amd import network_ops as nops
    k1, b1 = _weights()[:2]
    rng = np.random.default_rng(h + w)
    kinds = ["random", "black_lit", "random", "flat_1e3", "dark_sat9", "random", "grey_black3", "zero"]
    exps = [2.0 ** e for e in (0, 6, -6, 0, 3, 6, -3, 0)]
    imgs = np.stack([(_frame(k, h, w, rng) * F(s)).astype(F) for k, s in zip(kinds, exps)])
    kd, bd = to_dev(k1, dev), to_dev(b1, dev)
    mean, var = nops.encoder_level0_stats(to_dev(imgs, dev), kd, bd)
    _check_stats(mean, var, *_moments_f64(imgs, k1, b1), b1, f"batch of {len(kinds)} at {h}x{w}")
    for j in range(len(kinds)):
        mj, vj = nops.encoder_level0_stats(to_dev(imgs[j:j + 1], dev), kd, bd)
        assert torch.equal(mean[j:j + 1], mj) and torch.equal(var[j:j + 1], vj), (j, kinds[j])
    bsz, T = 2, len(kinds) // 2                         # image t * bsz + i of the sequence batch = seq[i, t]
    seq = np.ascontiguousarray(imgs.reshape(T, bsz, h, w, 3).transpose(1, 0, 2, 3, 4))
    ms, vs = nops.encoder_level0_stats(nops.FrameStack(to_dev(seq, dev)), kd, bd)
    assert torch.equal(mean, ms) and torch.equal(var, vs)
    m2, v2 = nops.encoder_level0_stats(to_dev(imgs, dev), kd, bd)
    assert torch.equal(mean, m2) and torch.equal(var, v2)


# ------------------------------------------------------------------------------------------- encoder level 0 end to end
def _bar(got, e32, r64, what, o32=None):
    """max / mean |gpu - f64| <= 3x / 2x those of ``e32`` (float32 with correctly rounded statistics), + a floor of 1e-6 / 1e-7
    x the output scale; ``o32`` (the plain float32 oracle) only printed."""
    g = np.asarray(got, np.float64)
    e_gpu, e_32 = np.abs(g - r64), np.abs(np.asarray(e32, np.float64) - r64)
    scale = max(float(np.abs(r64).max()), 1e-30)
    oracle = "" if o32 is None else f"; float32 oracle max {np.abs(np.asarray(o32, np.float64) - r64).max():.3e}"
    print(f"{what}: |gpu - f64| max {e_gpu.max():.3e} mean {e_gpu.mean():.3e}; float32 with rounded statistics max "
          f"{e_32.max():.3e} mean {e_32.mean():.3e}; scale {scale:.2e}{oracle}")
    assert np.isfinite(g).all(), what
    assert e_gpu.max() <= 3.0 * e_32.max() + 1e-6 * scale, (what, e_gpu.max(), e_32.max())
    assert e_gpu.mean() <= 2.0 * e_32.mean() + 1e-7 * scale, (what, e_gpu.mean(), e_32.mean())


def _dn_rounded_stats(x, scale, bias):
    """O.domain_normalization in float32 with the mean / variance of ``x`` taken in float64 and rounded to float32: what a
    kernel whose statistics are exact and whose apply pass is float32 computes, up to rounding."""
    x = np.asarray(x, F)
    x64 = x.astype(np.float64)
    m64 = x64.mean(axis=(1, 2), keepdims=True)
    mean = m64.astype(F)
    var = ((x64 - m64) ** 2).mean(axis=(1, 2), keepdims=True).astype(F)
    n = (x - mean) / (var + F(1e-12))
    ss = (n * n).sum(axis=-1, keepdims=True, dtype=F)
    n = n * (F(1.0) / np.sqrt(np.maximum(ss, F(1e-12))))
    return (scale.reshape(1, 1, 1, -1) * n + bias.reshape(1, 1, 1, -1)).astype(F)


def _level0_references(img, k1, b1, k2, b2, sc, bs):
    """(float32 with rounded statistics, plain float32 oracle, float64) of conv -> DN -> leaky_relu -> stride-2 conv ->
    leaky_relu."""
    def run(dn):
        t = O.leaky_relu(dn(O.conv2d_same(img, k1, b1, 1), sc, bs), 0.1)
        return O.leaky_relu(O.conv2d_same(t, k2, b2, 2), 0.1)
    e32, o32 = run(_dn_rounded_stats), run(O.domain_normalization)
    with O.float64_reference():
        r64 = run(O.domain_normalization)
    return e32, o32, r64


@pytest.mark.parametrize("h,w", [(384, 1280), (37, 53), (3, 5), (2, 2), (1, 7), (7, 1)])
@pytest.mark.parametrize("kind", FRAMES)
def test_encoder_level0_adversarial_frames(dev, kind, h, w):
    """m4d_enc_level0_fwd (stats=None), m4d_enc_level0_apply with statistics taken over a larger FrameStack, and the unfused
    head (m4d_enc_head_fwd + the normalising stride-2 convolution) on the frames of the statistics test, vs conv ->
    domain_normalization -> leaky_relu -> stride-2 conv -> leaky_relu in float64."""
    from m4depth_amd import network_ops as nops
    k1, b1, k2, b2, sc, bs = _weights()
    rng = np.random.default_rng(h * 13 + w)
    img = _frame(kind, h, w, rng)[None]
    e32, o32, r64 = _level0_references(img, k1, b1, k2, b2, sc, bs)
    args = (to_dev(k1, dev), to_dev(b1, dev), to_dev(sc, dev), to_dev(bs, dev), to_dev(k2, dev), to_dev(b2, dev), 0.1)
    got = nops.encoder_level0(to_dev(img, dev), *args)
    assert got.shape == r64.shape
    _bar(npy(got), e32, r64, f"fused {kind} {h}x{w}", o32)
    # statistics of a [1, 3] sequence whose middle frame is this one, applied to the frame alone: the same bits
    seq = np.stack([rng.random([h, w, 3]).astype(F), img[0], 0.5 * rng.random([h, w, 3]).astype(F)])[None]
    mean, var = nops.encoder_level0_stats(nops.FrameStack(to_dev(seq, dev)), args[0], args[1])
    got_s = nops.encoder_level0(to_dev(img, dev), *args, stats=(mean[1:2].contiguous(), var[1:2].contiguous()))
    assert torch.equal(got, got_s), f"{kind} {h}x{w}: statistics from the sequence differ from the frame's own"
    wp2, cpad2 = nops.pack_conv_weights(k2)
    head = nops.encoder_head(to_dev(img, dev), to_dev(k1.reshape(27, 16).copy(), dev), args[1], args[2], args[3],
                             to_dev(wp2, dev), args[5], 16, cpad2, 0.1)
    _bar(npy(head), e32, r64, f"unfused {kind} {h}x{w}", o32)


# ---------------------------------------------------------------------------------------------------- two-pass DINL
@pytest.mark.parametrize("C", [16, 32])
@pytest.mark.parametrize("slope", [1.0, 0.1])
def test_dinl_two_pass_ill_conditioned(dev, C, slope):
    """m4d_dinl_fwd_padded: a mean that dwarfs the spread (1e3 + 1e-2 x noise), one constant channel (var = 0: the 1e-12
    path; a dyadic constant, so that every evaluation takes its mean exactly), images of one batch 2^-10 .. 2^10 apart,
    written into a larger zero-bordered buffer at an offset whose border must stay untouched."""
    from m4depth_amd import network_ops as nops
    rng = np.random.default_rng(C + int(10 * slope))
    b, h, w = 3, 40, 56
    x = (1e3 + 1e-2 * rng.standard_normal([b, h, w, C])).astype(F)
    x[1] = (2.0 * rng.standard_normal([h, w, C]) + 0.5).astype(F)
    x[..., 3] = 0.375
    x *= np.array([2.0 ** -10, 1.0, 2.0 ** 10], F)[:, None, None, None]
    scale = (1 + 0.1 * rng.standard_normal(C)).astype(F)
    bias = (0.1 * rng.standard_normal(C)).astype(F)
    e32 = O.leaky_relu(_dn_rounded_stats(x, scale, bias), slope)
    o32 = O.leaky_relu(O.domain_normalization(x, scale, bias), slope)
    with O.float64_reference():
        r64 = O.leaky_relu(O.domain_normalization(x, scale, bias), slope)
    xd, sd, bd = to_dev(x, dev), to_dev(scale, dev), to_dev(bias, dev)
    got = nops.dinl_act(xd, sd, bd, slope)
    _bar(npy(got), e32, r64, f"DINL C={C} slope={slope}", o32)
    oy, ox = 2, 3
    out = torch.zeros((b, h + 5, w + 4, C), dtype=torch.float32, device=dev)
    nops.dinl_act(xd, sd, bd, slope, out=out, offset=(oy, ox))
    o = npy(out)
    assert np.array_equal(o[:, oy:oy + h, ox:ox + w], npy(got)), "padded target: other bits than the dense one"
    border = np.ones(o.shape[:3], bool)
    border[:, oy:oy + h, ox:ox + w] = False
    assert (o[border] == 0.0).all() and not np.signbit(o[border]).any(), "the border was written"


# ---------------------------------------------------------------------------------------------------- depth metrics
def _metrics_f64(gt, est, max_d=80.0):
    """metrics.py restated in float64 on the float32 clipped inputs; the masks and the Delta ratios in float32, as defined
    (a ratio exactly on a threshold is decided by its float32 value), so the Delta counts are exact integers."""
    gt = np.clip(gt.astype(F), F(0.0), F(max_d)).ravel()
    est = np.clip(est.astype(F), F(0.001), F(max_d)).ravel()
    m = gt > F(1e-6)
    cnt = max(float(m.sum()), 1.0)
    g, e = gt[m].astype(np.float64), est[m].astype(np.float64)
    d = g - e
    g6 = (gt[m] + F(1e-6)).astype(np.float64)
    absrel = np.sum(np.abs(d) / g6) / cnt
    sqrel = np.sum(d * d / g6) / cnt
    rmse = np.sqrt(np.sum(d * d) / cnt)
    lg32 = np.log(gt + F(1e-6))
    m2 = lg32 > F(1e-6)
    lg = np.log((gt[m2] + F(1e-6)).astype(np.float64))
    le = np.log((est[m2] + F(1e-6)).astype(np.float64))
    rmsel = np.sqrt(np.sum((lg - le) ** 2) / max(float(m2.sum()), 1.0))
    th = np.maximum(gt[m] / est[m], est[m] / gt[m])                       # float32
    deltas = [np.count_nonzero(th < F(t)) / cnt for t in (1.25, 1.5625, 1.953125)]
    return np.array([absrel, sqrel, rmse, rmsel] + deltas, np.float64)


def _check_metrics(vals, ref, what):
    vals = np.asarray(vals, np.float64)
    rel = np.abs(vals[:4] - ref[:4]) / np.maximum(np.abs(ref[:4]), 1e-30)
    ulps = np.abs(vals[4:].astype(F).view(np.int32).astype(np.int64) - ref[4:].astype(F).view(np.int32).astype(np.int64))
    print(f"{what}: AbsRel..RMSE_log relative error {rel.max():.2e} (bar 2e-5), Delta1..3 ulps {ulps.tolist()} (bar 1)")
    assert np.isfinite(vals).all()
    assert (rel < 2e-5).all(), (what, vals, ref)
    assert (ulps <= 1).all(), (what, vals, ref)


def _adversarial_depths(rng, shape, max_d=80.0):
    gt = (0.5 + 79.0 * rng.random(shape)).astype(F)
    est = (gt * (1 + 0.3 * rng.standard_normal(shape))).astype(F)
    flat_g, flat_e = gt.reshape(-1), est.reshape(-1)
    n = flat_g.size
    idx = rng.permutation(n)[: 12 * (n // 64)].reshape(12, -1)
    for r, t in enumerate((1.25, 1.5625, 1.953125)):                      # est exactly on a ratio, both sides, float32
        flat_e[idx[2 * r]] = flat_g[idx[2 * r]] * F(t)
        flat_e[idx[2 * r + 1]] = flat_g[idx[2 * r + 1]] / F(t)
    flat_g[idx[6]] = 0.0
    flat_g[idx[7]] = F(1e-6)
    flat_g[idx[8]] = F(max_d)
    flat_g[idx[9]] = F(max_d) * F(1.5)                                    # above max_d: clipped to it
    flat_e[idx[10]] = 0.0
    flat_e[idx[11]] = -rng.random(idx[11].size).astype(F)                 # est <= 0: clipped to 0.001
    return gt, est


def test_depth_metrics_full_size_adversarial(dev):
    """The bench's configs[2] size (32 x 384 x 1280: ~120 values per thread), est exactly on the Delta ratios, gt at 0,
    1e-6, max_d and above it, est <= 0; the sequence form reading data["depth"][:, -1] in place gives the dense bits."""
    from m4depth_amd import network_ops as nops
    rng = np.random.default_rng(2)
    b, h, w = 32, 384, 1280
    gt, est = _adversarial_depths(rng, (b, h, w, 1))
    ref = _metrics_f64(gt, est)
    gt_d, est_d = to_dev(gt, dev), to_dev(est, dev)
    vals = nops.depth_metrics(gt_d, est_d, 80.0)
    _check_metrics(npy(vals), ref, f"metrics {b}x{h}x{w}")
    seq = torch.empty((b, 2, h, w, 1), dtype=torch.float32, device=dev)
    seq[:, 0] = 1.0
    seq[:, 1] = gt_d
    del gt_d
    strided = nops.depth_metrics(seq[:, -1], est_d, 80.0)
    assert not seq[:, -1].is_contiguous()
    assert torch.equal(vals, strided)
    assert torch.equal(vals, nops.depth_metrics(seq[:, -1], est_d, 80.0))     # run-to-run identical


def test_depth_metrics_edges_and_accumulation(dev):
    """No valid pixel: all seven outputs 0 and finite (masked_reduce_mean divides by max(count, 1)).  Five updates through
    total / count / mean: total is the float32 running sum of the per-batch values (Keras Mean), mean matches
    O.MetricAccumulator."""
    from m4depth_amd import network_ops as nops
    rng = np.random.default_rng(3)
    gt = np.zeros([2, 40, 56, 1], F)
    gt[0, :3] = F(1e-6)
    est = (80 * rng.random(gt.shape)).astype(F)
    vals = npy(nops.depth_metrics(to_dev(gt, dev), to_dev(est, dev), 80.0))
    print(f"no valid pixel: {vals.tolist()}")
    assert np.isfinite(vals).all() and (vals == 0.0).all(), vals
    assert (O.metrics_batch(gt, est) == 0.0).all()
    total = torch.zeros(7, dtype=torch.float32, device=dev)
    mean = torch.zeros(7, dtype=torch.float32, device=dev)
    acc = O.MetricAccumulator()
    t32 = np.zeros(7, F)
    for k in range(1, 6):
        g, e = _adversarial_depths(rng, (2, 64, 96, 1))
        out = npy(nops.depth_metrics(to_dev(g, dev), to_dev(e, dev), 80.0, total=total, count=k, mean=mean))
        _check_metrics(out, _metrics_f64(g, e), f"update {k}")
        acc.update(g, e)
        t32 = (t32 + out).astype(F)
        assert np.array_equal(npy(total), t32), k
        assert np.array_equal(npy(mean), (t32 / F(k)).astype(F)), k
    rel = np.abs(npy(mean).astype(np.float64) - acc.result()) / np.maximum(np.abs(acc.result()), 1e-30)
    print(f"five updates: mean vs MetricAccumulator relative error {rel.max():.2e} (bar 2e-5)")
    assert (rel < 2e-5).all(), (npy(mean), acc.result())
