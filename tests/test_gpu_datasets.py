"""The forward at the sizes the network evaluates the datasets at -- KITTI 256 x 768, Mid-Air 384 x 384, TartanAir 384 x 512, six
levels: pyramids that end in 4 x 12, 6 x 6 and 6 x 8 maps -- against the NumPy oracle.  The cases and what the model runs on
each are tabulated in tests/dataset_cases.py; tests/test_dataset_cases.py keeps that table honest on the CPU.

  (a) both cost volumes on the coarse maps, bit for bit (every DSCV variant and the merged entry on the 4 x 12 and 6 x 6 maps);
  (b) the one-launch level fronts against the separate launches, bit for bit;
  (c) one teacher-forced level step at batch 1, 3 and (level 4) 8: level 4 through the latency kernels, the direct kernel and
      the Winograd + fused-front path;
  (d) ``DispRefiner.forward`` -- the product's dispatch, partial-sum slabs between layers included -- against the same seven
      layers in the oracle, float32 and float64;
  (e) the whole model at the three sizes with each loader's own intrinsics.

Tolerances: the ones the suite already applies to the same quantities -- bit-exact cost volumes and refiner inputs, 2e-6 on the
log channels, ``check_depth_and_parallax``'s defaults, 1e-5 x scale to the float32 oracle and 2x / 3x its mean / max error to
float64 for convolutions, ``check_against_float64_truth`` with 2.0 ("bf16x3") and 2.5 ("f16x2").

What the model runs ("f16x2"; D = direct split-K, L = latency-first fp16, W = fp16 Winograd; F / s = fused / small front), levels 1-6:
  batch 1, every dataset      W W D L L L       FFFsss
  batch 3, KITTI / TartanAir  W W W D L L       FFFsss      Mid-Air  W W W+D L L L   FFFsss
  batch 8, KITTI              W W W W+D L L     FFFFss      TartanAir  W W W W L L  FFFFss      Mid-Air  W W W W L L  FFFsss

Measured on an MI355X (seeds: KITTI 2561, Mid-Air 3841, TartanAir 3842, the first tried; the float32 oracle against the float64
one is within 2.5e-5 on every depth pixel of every level for all three):
  (d) over the 40 cases x 2 outputs: max |gpu - ref32| / scale 1.5e-6; error to float64 against the float32 oracle's: mean at most
      1.83x, max at most 2.03x (level 3, 32 x 96, batch 1, the estimate: 9.3e-7 / 6.6e-6 against 5.1e-7 / 3.2e-6), both arithmetics;
  (e) depth against the float32 oracle, worst level: KITTI 2.1e-5, Mid-Air 2.0e-5, TartanAir 1.9e-5 (100 % within 1e-4);
      well-conditioned weights: 6.5e-6 / 4.4e-6 / 4.6e-6; KITTI parallax error to float64, median per level: GPU 1.7e-7 .. 6.3e-7,
      float32 oracle 1.3e-6 .. 3.2e-6.  The KITTI float64 oracle takes 10 s of CPU time, the float32 ones 3.5 to 5.5 s each."""
import functools

import numpy as np
import pytest
import torch

import dataset_cases as DC
from oracle import m4depth_oracle as O
from m4depth_amd import synthetic as S
from helpers import F, to_dev, npy, assert_bits_equal, rel_err
from test_gpu_model import check_depth_and_parallax, level_step_teacher_forced, _build
from test_gpu_ops import (dscv_sncv_vs_oracle, merged_cost_volume_vs_separate, _front_small_vs_separate,
                          _fused_front_vs_separate)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    import m4depth_amd
    return m4depth_amd


# ------------------------------------------------------------------------------- (a) cost volumes
@pytest.mark.parametrize("b", DC.CV_BATCHES)
@pytest.mark.parametrize("h,w,C,k", DC.CV_CASES)
def test_cost_volumes_on_dataset_maps(M, dev, b, h, w, C, k):
    """DSCV r = 4 (9 hypotheses) and SNCV r = 3 (7 x 7) on the coarse maps: on the 4-row one both windows leave the map on both
    sides at every pixel."""
    dscv_sncv_vs_oracle(M, dev, b, h, w, C, k, 1000 * b + 10 * h + w)


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("h,w", DC.CV_VARIANT_MAPS)
def test_dscv_variants_on_the_coarsest_maps(M, dev, h, w, variant):
    from m4depth_amd._lib import lib
    try:
        lib.m4d_dscv_set_variant(variant)
        for b in DC.CV_BATCHES:
            dscv_sncv_vs_oracle(M, dev, b, h, w, 192, 8, 2000 * b + 10 * h + w + variant)
    finally:
        lib.m4d_dscv_set_variant(1)


@pytest.mark.parametrize("b", DC.CV_BATCHES)
@pytest.mark.parametrize("h,w", DC.CV_VARIANT_MAPS)
def test_merged_cost_volume_entry_on_the_coarsest_maps(dev, b, h, w):
    merged_cost_volume_vs_separate(dev, b, h, w, 192, 8, 3000 * b + 10 * h + w)


# ------------------------------------------------------------------------------- (b) level fronts
@pytest.mark.parametrize("depth,b,h,w,quat,cv_accum", DC.FRONT_SMALL_CASES)
def test_level_front_small_on_dataset_maps(M, dev, depth, b, h, w, quat, cv_accum, monkeypatch):
    _front_small_vs_separate(M, dev, depth, b, h, w, quat, cv_accum, monkeypatch)


@pytest.mark.parametrize("depth,b,h,w,quat,cv_accum", DC.FRONT_FUSED_CASES)
def test_fused_level_front_on_dataset_maps(M, dev, depth, b, h, w, quat, cv_accum):
    _fused_front_vs_separate(M, dev, depth, b, h, w, quat, cv_accum, 4, 3)


# ------------------------------------------------------------------------------- (c) one whole level
def _level_id(case):
    depth, b, h, w, form = case
    return f"L{depth}-b{b}-{h}x{w}-{form or 'default'}"


@pytest.mark.parametrize("case", DC.level_step_cases(), ids=_level_id)
def test_level_step_teacher_forced_on_dataset_maps(dev, case, monkeypatch):
    """tests/test_gpu_model.py::test_level_step_teacher_forced at the datasets' maps and batches: state and refiner input bit
    for bit, the log channels within 2e-6, depth and parallax through ``check_depth_and_parallax``."""
    depth, b, h, w, form = case
    lat = all(DC.conv_row(c)[2] is not None for c in DC.refiner_calls(depth, b, h, w) if "level" in c.callers)
    level_step_teacher_forced(dev, depth, b, h, w, form, monkeypatch, seed=7000 + 100 * depth + 10 * b + h + w,
                              one_launch_convs=lat)


# ------------------------------------------------------------------------------- (d) the refiner chain
def _leaky(x):
    return np.where(x > 0, x, x * x.dtype.type(0.1))


@functools.lru_cache(maxsize=None)
def _refiner_reference(depth, b, h, w):
    """(input, float32 and float64 oracle of the last prep layer's output and of the 5-channel estimate)."""
    W = S.init_weights(6, seed=3)
    rng = np.random.default_rng(8000 + 100 * depth + 10 * b + h + w)
    f_in = W[f"lvl.{depth}.conv.0.kernel"].shape[2]
    x = rng.standard_normal([b, h, w, f_in]).astype(F)

    def chain(dtype):
        y, prep = x.astype(dtype), None
        for i in range(7):
            y = O.conv2d_same(y, W[f"lvl.{depth}.conv.{i}.kernel"].astype(dtype), W[f"lvl.{depth}.conv.{i}.bias"].astype(dtype), 1)
            if i < 6:
                y = _leaky(y)
            if i == 2:
                prep = y
        return prep, y
    ref32 = chain(F)
    with O.float64_reference():
        ref64 = chain(np.float64)
    return W, x, ref32, ref64


@pytest.mark.parametrize("arith", DC.REFINER_ARITHS)
@pytest.mark.parametrize("depth,b,h,w", DC.refiner_cases())
def test_refiner_chain_on_dataset_maps(M, dev, depth, b, h, w, arith):
    """``DispRefiner.forward`` on a random refiner input of the level's padded width (the padding channels zero, as in the
    product): within 1e-5 x max(1, |ref32|max) of the float32 oracle, mean / max error to float64 at most 2x / 3x the float32
    oracle's -- on the last prep layer's output and on the 5-channel estimate."""
    from m4depth_amd import network as net
    W, x, ref32, ref64 = _refiner_reference(depth, b, h, w)
    settings = {"nbre_lvls": 6, "is_training": False, "ablation": M.M4depthAblationParameters()}
    gl = M.DepthEstimatorLevel(settings, depth)
    refiner = gl.disp_refiner
    for i, cv in enumerate(list(refiner.prep_conv_layers) + list(refiner.est_d_conv_layers)):
        cv.load_hwio(W[f"lvl.{depth}.conv.{i}.kernel"], W[f"lvl.{depth}.conv.{i}.bias"], dev)
    xp = np.zeros([b, h, w, net._padded_refiner_width(x.shape[-1])], F)
    xp[..., :x.shape[-1]] = x
    with net.conv_arithmetic(arith):
        out5, prep = refiner(to_dev(xp, dev))
        torch.cuda.synchronize()
    for what, got, r32, r64 in (("prep", npy(prep), ref32[0], ref64[0]), ("estimate", npy(out5), ref32[1], ref64[1])):
        assert got.shape == r32.shape, (what, got.shape, r32.shape)
        e_gpu, e_or = np.abs(got.astype(np.float64) - r64), np.abs(r32.astype(np.float64) - r64)
        d32 = np.max(np.abs(got - r32))
        scale = max(1.0, np.abs(r32).max())
        print(f"refiner L{depth} b{b} {h}x{w} [{arith}] {what}: max |gpu - ref32| {d32:.3e} (scale {scale:.2f}); |error| to float64 "
              f"mean / max: gpu {e_gpu.mean():.3e} / {e_gpu.max():.3e}, float32 oracle {e_or.mean():.3e} / {e_or.max():.3e}")
        assert d32 < 1e-5 * scale, what
        assert e_gpu.mean() <= 2.0 * e_or.mean() and e_gpu.max() <= 3.0 * e_or.max(), what


# ------------------------------------------------------------------------------- (e) the whole model
def _cam_l(cam, l):
    return {"f": cam["f"] / F(2.0 ** (l + 1)), "c": cam["c"] / F(2.0 ** (l + 1))}


@functools.lru_cache(maxsize=None)
def _model_case(name, kind):
    """(weights, samples, camera, the float32 oracle's (output, per-frame per-level estimates)).  ``kind``: "random" = He-normal
    weights (seed 42) / "wc" = ``S.well_conditioned_case``; lateral motion, the loader's own intrinsics."""
    H, Wd = DC.network_size(name)
    cam = DC.camera_np(name, DC.MODEL_BATCH)
    if kind == "wc":
        W, samples, _ = S.well_conditioned_case(DC.LEVELS, DC.MODEL_BATCH, DC.MODEL_FRAMES, H, Wd, DC.MODEL_SEEDS[name])
    else:
        W = S.init_weights(DC.LEVELS, seed=42)
        samples, _ = S.make_sequence(DC.MODEL_BATCH, DC.MODEL_FRAMES, H, Wd, seed=DC.MODEL_SEEDS[name], motion="lateral")
    return W, samples, cam, O.M4Depth(W, DC.LEVELS)(samples, cam)


@functools.lru_cache(maxsize=None)
def _kitti_float64():
    W, samples, cam, _ = _model_case("kitti", "random")
    with O.float64_reference():
        return O.M4Depth(W, DC.LEVELS)(samples, cam)[1]


def _stream_frame(sample, cam, dev):
    return {"RGB_im": torch.from_numpy(sample["RGB_im"]).to(dev), "rot": torch.from_numpy(sample["rot"]).to(dev),
            "trans": torch.from_numpy(sample["trans"]).to(dev), "new_traj": torch.from_numpy(sample["new_traj"]).to(dev),
            "camera": {k: torch.from_numpy(v).to(dev) for k, v in cam.items()}}


@pytest.mark.parametrize("name", DC.DATASETS)
def test_model_at_dataset_size_vs_oracle(dev, name):
    """Six levels, batch 1, a reset and two full frames: depth and parallax of the last frame at every level through
    ``check_depth_and_parallax``, and the same frames through ``stream_step`` one at a time, bit for bit the sequence call."""
    W, samples, cam, (oout, oseq) = _model_case(name, "random")
    H, Wd = DC.network_size(name)
    model = _build(dev, DC.LEVELS, 4, 3, W)
    out = model([to_dev(samples, dev), to_dev(cam, dev)])
    assert out["depth"].shape == (DC.MODEL_BATCH, H, Wd, 1) and torch.isfinite(out["depth"]).all()
    seq = [{k: npy(v) for k, v in est.items()} for est in model.last_estimates[-1]]
    for l in range(DC.LEVELS):
        check_depth_and_parallax(seq[l]["depth"], seq[l]["parallax"], oseq[-1][l]["depth"], oseq[-1][l]["parallax"],
                                 samples[-1]["rot"], samples[-1]["trans"], _cam_l(cam, l), f"{name} {H}x{Wd} level {l}")
    stream = _build(dev, DC.LEVELS, 4, 3, W)
    for s in samples:
        last = stream.stream_step(_stream_frame(s, cam, dev))
    assert_bits_equal(npy(last["depth"]), npy(out["depth"]), f"{name}: stream_step depth vs the sequence call")
    for l, est in enumerate(stream.last_estimates[-1]):
        for key in ("depth", "parallax", "other"):
            assert_bits_equal(npy(est[key]), seq[l][key], f"{name}: stream_step level {l} {key} vs the sequence call")


@pytest.mark.parametrize("name", DC.DATASETS)
def test_model_at_dataset_size_well_conditioned_within_1e4_everywhere(dev, name):
    """``test_well_conditioned_depth_within_1e4_everywhere``'s check with the oracle evaluated here: depth within 1e-4 relative
    of the float32 oracle on every pixel of every level and of the output."""
    W, samples, cam, (oout, oseq) = _model_case(name, "wc")
    H, Wd = DC.network_size(name)
    model = _build(dev, DC.LEVELS, 4, 3, W)
    out = model([to_dev(samples, dev), to_dev(cam, dev)])
    torch.cuda.synchronize()
    worst = 0.0
    for l in range(DC.LEVELS):
        est = model.last_estimates[-1][l]
        rel = rel_err(npy(est["depth"]), oseq[-1][l]["depth"], 1e-30)
        rp = rel_err(npy(est["parallax"]), oseq[-1][l]["parallax"], 1e-30)
        print(f"well-conditioned {name} {H}x{Wd} level {l}: depth rel max {rel.max():.2e} median {np.median(rel):.2e} | "
              f"parallax rel max {rp.max():.2e}")
        worst = max(worst, float(rel.max()))
    worst = max(worst, float(rel_err(npy(out["depth"]), O.resize_nearest(oseq[-1][0]["depth"], H, Wd), 1e-30).max()))
    print(f"well-conditioned {name}: max relative depth error over all levels and the output {worst:.2e}")
    assert worst < 1e-4


@pytest.mark.parametrize("h,w,cin,cout,stride", [(32, 96, 64, 96, 1), (64, 192, 64, 64, 2), (48, 64, 64, 96, 1), (32, 96, 96, 96, 2)])
def test_encoder_direct_conv_bits_do_not_depend_on_frames_stacked(dev, h, w, cin, cout, stride):
    """What the stream-against-sequence comparison above exposed at 256 x 768 and 384 x 512: the direct kernel's launcher chose
    its split-K factor (the summation order) from the batch of the launch, so encoder levels 2-3 gave other last bits on one
    streamed frame than on two stacked frames.  With ``split_batch`` one, two and three stacked images give the same bits per
    image, within the float32 tolerance of the oracle."""
    from m4depth_amd import network_ops as nops
    rng = np.random.default_rng(cin + cout + h + stride)
    x = rng.standard_normal([3, h, w, cin]).astype(F)
    k = (rng.standard_normal([3, 3, cin, cout]) * np.sqrt(2.0 / (9 * cin))).astype(F)
    bias = (0.1 * rng.standard_normal([cout])).astype(F)
    wp, cpad = nops.pack_conv_weights(k)
    xd, wd, bd = to_dev(x, dev), to_dev(wp, dev), to_dev(bias, dev)
    outs = [nops.conv3x3_bias_act(xd[:n].contiguous(), wd, bd, cout, cpad, 0.1, stride=stride, split_batch=2) for n in (1, 2, 3)]
    for n, o in zip((1, 2), outs):
        assert torch.equal(o, outs[2][:n]), f"{n} stacked image(s) against 3"
    ref = _leaky(O.conv2d_same(x, k, bias, stride)).astype(F)
    assert np.max(np.abs(npy(outs[2]) - ref)) < 1e-5 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("arith,factor", [("f16x2", 2.5), ("bf16x3", 2.0)])
def test_kitti_size_against_float64_truth(dev, arith, factor):
    """The KITTI pyramid (the one with no neighbour in the suite): the GPU as close to the float64 evaluation as the float32
    oracle is, at every level.  The inputs' own conditioning first: the float32 oracle against the float64 one meets
    ``check_depth_and_parallax`` alone."""
    from m4depth_amd import network as net
    from test_gpu_configs import check_against_float64_truth
    W, samples, cam, (_, seq32) = _model_case("kitti", "random")
    seq64 = _kitti_float64()
    with net.conv_arithmetic(arith):
        model = _build(dev, DC.LEVELS, 4, 3, W)
        model([to_dev(samples, dev), to_dev(cam, dev)])
        torch.cuda.synchronize()
    for l in range(DC.LEVELS):
        check_depth_and_parallax(seq32[-1][l]["depth"], seq32[-1][l]["parallax"], seq64[-1][l]["depth"], seq64[-1][l]["parallax"],
                                 samples[-1]["rot"], samples[-1]["trans"], _cam_l(cam, l), f"float32 oracle vs float64, level {l}")
        est = model.last_estimates[-1][l]
        check_against_float64_truth({"parallax": npy(est["parallax"]), "depth": npy(est["depth"])}, seq32[-1][l], seq64[-1][l],
                                    f"kitti 256x768 [{arith}] level {l}", factor=factor)
