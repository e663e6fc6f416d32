"""DepthEstimatorLevel / M4Depth on the MI355X vs the CPU oracle.

Tolerances:
  * teacher-forced level step (identical inputs, convolutions excluded): the
    refiner input ``f_input`` matches the oracle bit-exactly on the cost-volume /
    memory channels and to 2e-6 relative on the two log channels;
  * full model (hand-written fp32-MFMA / Winograd convolutions vs the oracle's BLAS convolutions --
    different summation orders): depth within 1e-4 relative of the oracle
    (north_star tolerance) on >= 99.5 % of pixels, median below 1e-5, AbsRel metric
    within 1e-4 relative.  The few outliers come from float16 rounding flips of
    DSCV products fed by features that differ in the last bits; see DESIGN.md.
"""
import os

import numpy as np
import pytest
import torch

from oracle import m4depth_oracle as O
from m4depth_amd import synthetic as S
from helpers import F, camera_np, motion_np, to_dev, npy, assert_bits_equal, rel_err

pytestmark = pytest.mark.gpu


def check_depth_and_parallax(depth, para, o_depth, o_para, rot, trans, cam, what, frac_ok=0.99, max_tol=1e-4):
    """The north-star tolerance is 1e-4 relative on depth.  depth = (s/para - tz)/alpha
    cancels when s/para ~ tz (only reachable with random weights: a trained net keeps
    depth in [0.1, 1000]), so relative depth error is unbounded there however accurate
    the parallax is.  Asserted: parallax within 1e-4 relative everywhere; depth within
    1e-4 of the magnitude of the operands it is the difference of, everywhere; and within
    1e-4 relative of itself on >= frac_ok of the pixels."""
    b, h, w = o_depth.shape[:3]
    m = O.motion_factors(b, h, w, rot, trans, cam)
    rp = rel_err(para, o_para, 1e-12)
    scale = ((m["sqrt"] / o_para[..., 0] + np.abs(m["stz"])) / np.abs(m["alpha"]))[..., None]
    ed = np.abs(depth.astype(np.float64) - o_depth)
    rd = rel_err(depth, o_depth, 1e-9)
    print(f"{what}: parallax rel max {rp.max():.2e} | depth rel median {np.median(rd):.2e} p99 {np.percentile(rd, 99):.2e} "
          f"max {rd.max():.2e} within1e-4 {100 * np.mean(rd < 1e-4):.3f}% | cond-scaled max {np.max(ed / scale):.2e}")
    assert rp.max() < max_tol, what
    assert np.max(ed / scale) < max_tol, what
    assert np.mean(rd < 1e-4) >= frac_ok and np.median(rd) < 1e-5, what


def _build(dev, L, rd, rs, weights):
    import m4depth_amd as M
    model = M.M4Depth(nbre_levels=L, dscv_range=rd, sncv_range=rs)
    model.load_numpy_weights(weights, dev)
    return model


@pytest.mark.parametrize("depth,h,w,coarse_front", [(1, 32, 48, False), (2, 16, 24, False), (3, 16, 24, False), (4, 8, 12, False),
                                                     (6, 6, 10, False), (4, 8, 12, True), (5, 8, 12, True), (6, 6, 10, True),
                                                     (4, 8, 12, "small"), (5, 8, 12, "small"), (6, 6, 10, "small")])
def test_level_step_teacher_forced(dev, depth, h, w, coarse_front, monkeypatch):
    """One full DepthEstimatorLevel step per level geometry with identical inputs on
    both sides; compares the assembled refiner input and the state handling.  Levels 1-3 go through the fused level front;
    levels 4-6 through the small-map kernels (their default at this size) and, with ``coarse_front``, through the fused
    front instantiations of their geometries (the default from batch >= 4 at 384x1280); ``"small"`` = the one-launch opening of a
    coarse level on features normalised ahead of it (m4d_normalize_levels + m4d_level_front_small: what the batch-1 bench path
    runs on levels 4-6 since round 6), against the oracle directly."""
    level_step_teacher_forced(dev, depth, 2, h, w, coarse_front, monkeypatch)


def level_step_teacher_forced(dev, depth, b, h, w, coarse_front, monkeypatch, seed=None, one_launch_convs=True):
    """The body of ``test_level_step_teacher_forced`` at batch ``b`` (tests/test_gpu_datasets.py runs it on the datasets' maps).
    ``one_launch_convs``: the level's five convolutions are one launch each (the latency-first kernels), so that the "small"
    form can be held to its launch count."""
    import m4depth_amd as M
    from m4depth_amd import network as net, network_ops as nops
    if coarse_front is True:
        monkeypatch.setattr(net, "fused_front_coarse_min_pixels", 0)
    rng = np.random.default_rng(200 + depth if seed is None else seed)
    C = S.ENCODER_CHANNELS[depth - 1]
    W = S.init_weights(6, seed=3)
    ol = O.DepthEstimatorLevel(W, depth)
    settings = {"nbre_lvls": 6, "is_training": False, "ablation": M.M4depthAblationParameters()}
    gl = M.DepthEstimatorLevel(settings, depth)
    convs = list(gl.disp_refiner.prep_conv_layers) + list(gl.disp_refiner.est_d_conv_layers)
    for i, cv in enumerate(convs):
        cv.load_hwio(W[f"lvl.{depth}.conv.{i}.kernel"], W[f"lvl.{depth}.conv.{i}.bias"], dev)
    cam = camera_np(b, h, w)
    prev = None
    if depth < 6:
        prev = {"depth": (1 + 50 * rng.random([b, h // 2, w // 2, 1])).astype(F),
                "parallax": (0.2 + 2 * rng.random([b, h // 2, w // 2, 1])).astype(F),
                "other": rng.standard_normal([b, h // 2, w // 2, 4]).astype(F)}
    for step in range(3):
        rot, trans = motion_np(rng, b, t_scale=(3.0, 3.0, 1.0))
        f = rng.standard_normal([b, h, w, C]).astype(F)
        nt = np.full([b], step == 0)
        eo = ol(f, prev, rot, trans, cam, nt)
        nf = None
        if coarse_front == "small":
            assert gl.wants_prenormalized(b, h, w, C)
            nf = nops.normalize_levels([(to_dev(f, dev), gl.nbre_cuts)])[0]
        n0 = int(net.lib.m4d_launch_count())
        eg = gl(to_dev(f, dev), to_dev(prev, dev), to_dev(rot, dev), to_dev(trans, dev), to_dev(cam, dev), nt, curr_f_normalized=nf)
        if coarse_front == "small" and step > 0 and one_launch_convs:
            assert int(net.lib.m4d_launch_count()) - n0 == 7, "a coarse level = front + 5 convolutions + tail"
        assert_bits_equal(npy(gl.prev_f_maps), ol.prev_f_maps, "state: normalised features")
        if step == 0:
            for key in ("depth", "parallax", "other"):
                assert_bits_equal(npy(eg[key]), eo[key], f"reset branch {key}")
            assert torch.all(gl.depth_prev_t == 1000.0)
            continue
        fo, fg = ol.last_f_input, npy(gl.last_f_input)
        k = 2 ** (depth // 2)
        log_a, log_b = 9 * k, fo.shape[-1] - 1
        exact = [c for c in range(fo.shape[-1]) if c not in (log_a, log_b)]
        assert_bits_equal(fg[..., exact], fo[..., exact], "f_input (cv | other | sncv)")
        assert np.max(rel_err(fg[..., [log_a, log_b]], fo[..., [log_a, log_b]], 1e-3)) < 2e-6
        # convolutions differ in summation order: compare outputs with the north-star tolerance
        check_depth_and_parallax(npy(eg["depth"]), npy(eg["parallax"]), eo["depth"], eo["parallax"], rot, trans, cam,
                                 f"level {depth} batch {b} {h}x{w} step {step}")
        # hand the oracle's state to the GPU level so that the next step is teacher-forced again
        gl.depth_prev_t.copy_(to_dev(ol.depth_prev_t, dev))


@pytest.mark.parametrize("arith", ["bf16x3", "f32"])
@pytest.mark.parametrize("case", ["cfg1", "full"])
def test_well_conditioned_depth_within_1e4_everywhere(dev, golden, case, arith):
    """THE north-star tolerance, asserted on 100 % of the pixels: depth within 1e-4 relative of the oracle's, at every
    level, on the well-conditioned fixture (m4depth_amd.synthetic.well_conditioned_case; golden outputs of the float32
    oracle: tests/golden/model_wc_{cfg1,full}.npz) -- BASELINE config-1 size (3 levels, two full frames) and one
    384x1280 / 6-level frame pair (configs[1]'s geometry, every kernel of the bench path: fused fronts, the bf16-split /
    fp32 Winograd kernels, small-map kernels on levels 4-6, fused tails), in both convolution arithmetics.  The only
    depth assertion is max(rel) < 1e-4.  (m4depth_network.py:247-251)"""
    from m4depth_amd import network as net
    g = golden(f"model_wc_{case}")
    L, rd, rs, H, Wd, T, b, seed = [int(v) for v in g["meta"]]
    W, samples, cam = S.well_conditioned_case(L, b, T, H, Wd, seed, rd, rs)
    with net.conv_arithmetic(arith):
        model = _build(dev, L, rd, rs, W)
        out = model([to_dev(samples, dev), to_dev(cam, dev)])
        torch.cuda.synchronize()
    worst = 0.0
    for l in range(L):
        est = model.last_estimates[-1][l]
        rel = rel_err(npy(est["depth"]), g[f"l{l}_depth"], 1e-30)
        rp = rel_err(npy(est["parallax"]), g[f"l{l}_parallax"], 1e-30)
        print(f"well-conditioned {case} [{arith}] level {l}: depth rel max {rel.max():.2e} median {np.median(rel):.2e} | "
              f"parallax rel max {rp.max():.2e}")
        worst = max(worst, float(rel.max()))
    full = rel_err(npy(out["depth"]), O.resize_nearest(g["l0_depth"], H, Wd), 1e-30)
    worst = max(worst, float(full.max()))
    print(f"well-conditioned {case} [{arith}]: max relative depth error over all levels and the output {worst:.2e} "
          f"(float32 oracle vs its float64 evaluation: {float(g['f32_vs_f64_max_rel_depth']):.2e})")
    assert worst < 1e-4


def test_model_config1_vs_oracle_and_golden(dev, golden):
    """BASELINE config 1: 128x256, 3 levels, ranges 2/2, b=1, one reset + two full frames."""
    g = golden("model_cfg1")
    L, rd, rs, H, Wd, T, b, seed = [int(v) for v in g["meta"]]
    W = S.init_weights(L, seed=42, dscv_range=rd, sncv_range=rs)
    samples, cam = S.make_sequence(b, T, H, Wd, seed=seed)
    model = _build(dev, L, rd, rs, W)
    ds = to_dev(samples, dev)
    out = model([ds, to_dev(cam, dev)])
    depth = npy(out["depth"])
    assert depth.shape == (b, H, Wd, 1)
    re = rel_err(depth, g["depth"], 1e-9)
    frac = float(np.mean(re < 1e-4))
    print(f"config1 depth: median rel {np.median(re):.2e}, p99 {np.percentile(re, 99):.2e}, max {re.max():.2e}, "
          f"within 1e-4: {100 * frac:.3f}%")
    assert np.median(re) < 1e-5
    assert frac > 0.99
    # per-level estimates of the last frame against the golden ones
    est = model.last_estimates[-1]
    cam_l = lambda l: {"f": cam["f"] / F(2.0 ** (l + 1)), "c": cam["c"] / F(2.0 ** (l + 1))}
    for l in range(L):
        check_depth_and_parallax(npy(est[l]["depth"]), npy(est[l]["parallax"]), g[f"t{T - 1}_l{l}_depth"],
                                 g[f"t{T - 1}_l{l}_parallax"], samples[-1]["rot"], samples[-1]["trans"], cam_l(l),
                                 f"config1 level {l}", frac_ok=0.98)
    # AbsRel & co through the product's metric classes vs the oracle's numbers
    import m4depth_amd as M
    mets = M.default_metrics()
    gt = torch.clamp(ds[-1]["depth"], 0.0, 80.0)
    est = torch.clamp(out["depth"], 0.001, 80.0)
    for m in mets:
        m.update_state(gt, est)
    got = np.array([float(m.result()) for m in mets])
    assert np.max(rel_err(got, g["metrics"], 1e-6)) < 1e-4, (got, g["metrics"])
    # first (reset) frame only: everything is exactly the initial estimate
    model.reset_state()
    out0 = model([ds[:1], to_dev(cam, dev)])
    assert torch.all(out0["depth"] == 1000.0)


def test_model_streaming_equals_sequence(dev):
    """Feeding frames one at a time (main.py eval on a stream, test_step 4-D branch)
    must give the same depth as feeding the whole sequence: state is carried by the
    levels, not by the call.  Bitwise: every kernel of the forward is deterministic, and the
    sequence call's batched encoder has the same per-sample arithmetic."""
    L, H, Wd, T, b = 4, 64, 128, 2, 2
    W = S.init_weights(L, seed=5)
    samples, cam = S.make_sequence(b, T, H, Wd, seed=99)
    model = _build(dev, L, 4, 3, W)
    ds, dc = to_dev(samples, dev), to_dev(cam, dev)
    full = model([ds, dc])
    full_para = npy(model.last_estimates[-1][0]["parallax"])
    model.reset_state()
    for s in ds:
        last = model([[s], dc])
    last_para = npy(model.last_estimates[-1][0]["parallax"])
    assert torch.isfinite(full["depth"]).all()
    assert_bits_equal(last_para, full_para, "stream vs sequence parallax")
    assert torch.equal(last["depth"], full["depth"])


def test_test_step_semantics(dev):
    """m4depth_network.py:433-474: 5-D input -> metrics on the last frame only; 4-D
    input with new_traj -> no metric update."""
    import m4depth_amd as M
    L, H, Wd, T, b = 3, 64, 96, 3, 2
    W = S.init_weights(L, seed=6)
    samples, cam = S.make_sequence(b, T, H, Wd, seed=17)
    model = _build(dev, L, 4, 3, W)
    model.compile(metrics=M.default_metrics())
    seq = {k: torch.stack([to_dev(s[k], dev) if k != "new_traj" else torch.from_numpy(s[k]) for s in samples], dim=1)
           for k in ("depth", "RGB_im", "new_traj", "rot", "trans")}
    seq["camera"] = to_dev(cam, dev)
    res = model.test_step(seq)
    assert set(res) == {"AbsRel", "SqRel", "RMSE", "RMSE_log", "Delta1", "Delta2", "Delta3"}
    assert all(m.count == 1 for m in model.compiled_metrics)
    ref = float(res["AbsRel"])
    # stream form: frame 0 (new_traj) must not update the metrics
    model.reset_state()
    for m in model.compiled_metrics:
        m.reset_state()
    for t, s in enumerate(samples):
        d = to_dev(s, dev)
        d["camera"] = to_dev(cam, dev)
        model.test_step(d)
        assert model.compiled_metrics[0].count == t
    assert np.isfinite(ref) and ref > 0


@pytest.mark.parametrize("keep", ["", "staggered", "lock_step"])
def test_graphed_sequence_matches_eager(dev, keep, monkeypatch):
    """hipGraph replay of the sequence forward (the bench's launch path) against the
    eager forward of the same batch, bit for bit, and replay on a second batch copied into the
    static buffers; a batch with another shape or new_traj pattern is refused.  GraphedSequence captures the sequence twice (the
    Winograd first round staggered / in lock step) and keeps the faster graph: whichever it keeps (``keep`` forces one), the
    replay, ``model.last_estimates`` and the returned depth are that graph's."""
    import m4depth_amd as M
    from m4depth_amd import network as net
    monkeypatch.setattr(net, "wino6_stagger_force", keep)
    L, H, Wd, T, b = 3, 64, 96, 2, 2
    W = S.init_weights(L, seed=8)
    model = _build(dev, L, 4, 3, W)
    model.compile(metrics=M.default_metrics())

    def batch(seed):
        samples, cam = S.make_sequence(b, T, H, Wd, seed=seed)
        d = {k: torch.stack([to_dev(s[k], dev) for s in samples], dim=1) for k in ("depth", "RGB_im", "rot", "trans")}
        d["new_traj"] = torch.stack([torch.from_numpy(s["new_traj"]) for s in samples], dim=1)
        d["camera"] = to_dev(cam, dev)
        return d

    d1, d2 = batch(31), batch(32)
    model.test_step(d1)
    eager1 = npy(model.last_estimates[-1][0]["parallax"])
    fin1 = npy(model.d_estimator.levels[0].last_f_input)
    model.test_step(d2)
    eager2 = npy(model.last_estimates[-1][0]["parallax"])
    runner = net.GraphedSequence(model, d1)
    for m in model.compiled_metrics:
        m.reset_state()
    for d, ref in ((d1, eager1), (d2, eager2), (d1, eager1)):
        res = model.graphed_test_step(d, runner)
        torch.cuda.synchronize()
        assert_bits_equal(npy(model.last_estimates[-1][0]["parallax"]), ref, "graph replay vs eager")
    # the per-level inspection tensors are the KEPT capture's too (after the loser's pool is freed nothing may point into it)
    assert_bits_equal(npy(model.d_estimator.levels[0].last_f_input), fin1, "level-1 refiner input of the kept graph")
    assert model.compiled_metrics[0].count == 3 and np.isfinite(float(res["AbsRel"]))
    assert runner.capture_passes == 2 and runner.stagger_us == {"staggered": net.wino6_stagger_us, "lock_step": 0}.get(keep, runner.stagger_us)
    # the choice is THIS model's setting (a launch argument from here on), not library state
    assert model.wino6_stagger_us == runner.stagger_us
    assert all(c.wino6_stagger_us == runner.stagger_us for c in model.modules() if isinstance(c, net._Conv3x3SameTF))
    # a caller can switch the double capture off: one capture, with the model's own setting
    single = net.GraphedSequence(model, d1, autotune=False)
    assert single.capture_passes == 1 and single.stagger_us == runner.stagger_us and single.stagger_autotune_ms is None
    assert torch.equal(single(d2), runner(d2))
    assert torch.equal(runner(d2), model([[{k: d2[k][:, t] for k in ("RGB_im", "rot", "trans", "new_traj")} for t in range(T)],
                                          d2["camera"]])["depth"])
    bad = dict(d1)
    bad["new_traj"] = torch.zeros_like(d1["new_traj"])
    with pytest.raises(ValueError):
        runner(bad)
    bad = dict(d1)
    bad["RGB_im"] = d1["RGB_im"][:1]
    with pytest.raises(ValueError):
        runner(bad)


@pytest.mark.parametrize("split", [2, 4])
def test_graph_replay_writes_only_memory_it_owns(dev, split, monkeypatch):
    """Round 6 regression (a GPU memory fault under M4D_PIPELINE_ENCODER_SPLIT=4, a silent hazard otherwise): a captured step has the
    addresses of the levels' state buffers baked in.  With a coarse level opening on features normalised ahead of it, the
    normalised tensor becomes ``prev_f_maps`` -- and the level's own buffer it replaced was DROPPED, returned to the caching
    allocator and handed to the next eager allocation of that size, which every replay (frame 0's reset writes that address) then
    overwrote.  The level now owns its two buffers for life and only borrows the caller's tensor.  Here: capture (both Winograd
    forms, the loser freed), then allocate many eager tensors of exactly the levels' state sizes, fill them with a sentinel,
    replay, and require every sentinel intact and the replay equal to the eager forward."""
    import m4depth_amd as M
    from m4depth_amd import network as net
    monkeypatch.setattr(net, "pipeline_encoder_split", split)
    L, H, Wd, T, b = 6, 192, 320, 4, 1                     # levels 3-6 open with m4d_level_front_small at this size
    W = S.init_weights(L, seed=11)
    model = _build(dev, L, 4, 3, W)
    samples, cam = S.make_sequence(b, T, H, Wd, seed=12)
    d = {k: torch.stack([to_dev(s[k], dev) for s in samples], dim=1) for k in ("depth", "RGB_im", "rot", "trans")}
    d["new_traj"] = torch.stack([torch.from_numpy(s["new_traj"]) for s in samples], dim=1)
    d["camera"] = to_dev(cam, dev)
    frames = [{k: d[k][:, t] for k in ("RGB_im", "rot", "trans", "new_traj")} for t in range(T)]
    ref = model([frames, d["camera"]])["depth"].clone()
    assert any(lv.wants_prenormalized(b, H >> (i + 1), Wd >> (i + 1), S.ENCODER_CHANNELS[i]) for i, lv in enumerate(model.d_estimator.levels))
    runner = net.GraphedSequence(model, d)
    shapes = [tuple(lv._own[0].shape) for lv in model.d_estimator.levels] + [(b, H >> (i + 1), Wd >> (i + 1), 1) for i in range(L)]
    guards = [torch.full(sh, 12345.0, device=dev) for _ in range(6) for sh in shapes]
    torch.cuda.synchronize()
    for _ in range(3):
        out = runner(d)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    for g in guards:
        assert bool((g == 12345.0).all()), f"a replay wrote into an eager tensor of shape {tuple(g.shape)}"
    for lv in model.d_estimator.levels:                    # the level still owns two distinct buffers, neither of them the borrowed one
        assert lv._own is not None and lv._spare_f is not lv.prev_f_maps and any(lv._spare_f is o for o in lv._own)


def test_two_models_two_threads_keep_their_own_stagger(dev, monkeypatch):
    """two models with different staggered-first-round settings, each driven from its own host thread at the
    same time, each hand THEIR OWN value to every Winograd launch (the argument of m4d_conv3x3_wino6_bias_act_ks; round 5 kept it
    in a process-wide variable of the library that the last writer won) -- and compute the same bits."""
    import threading
    import m4depth_amd as M
    from m4depth_amd import network as net, network_ops as nops
    L, H, Wd, T, b = 2, 192, 640, 2, 1                   # level 1 = 96x320: 120 tiles x 2 cout groups = 240 workgroups >= 200
    W = S.init_weights(L, seed=3)
    models = {"a": _build(dev, L, 4, 3, W).set_wino6_stagger(0), "b": _build(dev, L, 4, 3, W).set_wino6_stagger(23)}
    samples, cam = S.make_sequence(b, T, H, Wd, seed=5)
    seen = {"a": set(), "b": set()}
    real = nops.conv3x3_wino6_bias_act
    names = {}

    def spy(*args, **kw):
        seen[names[threading.get_ident()]].add(int(kw.get("stagger_us", 0)))
        return real(*args, **kw)
    monkeypatch.setattr(nops, "conv3x3_wino6_bias_act", spy)
    outs, start = {}, threading.Barrier(2)

    def worker(name):
        names[threading.get_ident()] = name
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            start.wait()
            for _ in range(3):
                models[name].reset_state()
                outs[name] = models[name]([to_dev(samples, dev), to_dev(cam, dev)])["depth"]
            st.synchronize()
    th = [threading.Thread(target=worker, args=(n,)) for n in ("a", "b")]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert seen["a"] == {0}, seen
    assert 23 in seen["b"] and seen["b"] <= {0, 23}, seen       # (its small grids launch in lock step: the policy of launch_stagger_us)
    assert torch.equal(outs["a"], outs["b"])


def test_graphed_batch2_has_only_library_kernels(dev, tmp_path):
    """from batch 2 on the [:, t] slices of batch-major rot / trans are non-contiguous and every level
    wrapper used to copy them with a framework kernel INSIDE the captured graph (batch 32: ~43 at::native copy nodes per step).
    GraphedSequence keeps them frame-major now and ``as_f32`` refuses to copy under a capture; here a batch-2 sequence is
    captured, the graph dumped (hipGraphDebugDotPrint) and every kernel node must be one of libm4depth_hip.so's; the strided
    ground truth of the metric kernel (data["depth"][:, -1] read in place) gives the bits of the dense copy."""
    import re
    import m4depth_amd as M
    from m4depth_amd import network as net, network_ops as nops
    L, H, Wd, T, b = 3, 64, 96, 3, 2
    W = S.init_weights(L, seed=8)
    model = _build(dev, L, 4, 3, W)
    model.compile(metrics=M.default_metrics())
    samples, cam = S.make_sequence(b, T, H, Wd, seed=33)
    d = {k: torch.stack([to_dev(s[k], dev) for s in samples], dim=1) for k in ("depth", "RGB_im", "rot", "trans")}
    d["new_traj"] = torch.stack([torch.from_numpy(s["new_traj"]) for s in samples], dim=1)
    d["camera"] = to_dev(cam, dev)
    assert not d["rot"][:, 1].is_contiguous()                       # the slices that used to be copied inside the graph
    model.test_step(d)
    eager = npy(model.last_estimates[-1][0]["parallax"])
    runner = net.GraphedSequence(model, d)
    model.graphed_test_step(d, runner)
    torch.cuda.synchronize()
    assert_bits_equal(npy(model.last_estimates[-1][0]["parallax"]), eager, "batch-2 graph replay vs eager")
    # the node list of the same capture, from the HIP runtime's own dump of the instantiated graph (a fresh process: the
    # runtime reads DEBUG_HIP_GRAPH_DOT_PRINT when it starts): tools/dump_graph_nodes.py exits non-zero on a foreign node
    import subprocess
    import sys as _sys
    dot = tmp_path / "graph.dot"
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "dump_graph_nodes.py")
    res = subprocess.run([_sys.executable, tool, "--batch", str(b), "--height", str(H), "--width", str(Wd), "--levels", str(L),
                          "--frames", str(T), "--out", str(dot)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    names = re.findall(r"_Z\w+", dot.read_text())
    assert len(names) >= 40, f"no kernel nodes recognised in the graph dump ({len(names)})"
    assert not [n for n in names if "at6native" in n or "at4cuda" in n or "rocclr" in n]
    # a non-contiguous input inside a capture is refused loudly instead of being copied by a framework kernel
    g = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with pytest.raises(RuntimeError, match="hipGraph capture"):
        with torch.cuda.graph(g, stream=st):
            net.as_f32(d["rot"][:, 1], "rot")
    # metric kernel: strided ground truth == dense copy, bit for bit
    est = runner.depth
    gt_view = d["depth"][:, -1]
    assert not gt_view.is_contiguous()
    a = nops.depth_metrics(gt_view, est, 80.0)
    c = nops.depth_metrics(gt_view.contiguous(), est, 80.0)
    assert torch.equal(a, c)


def test_forward_is_deterministic_bitwise(dev):
    """No MIOpen / framework kernel is in the model and every hand-written kernel is deterministic: the same
    sequence twice, and frame-by-frame streaming vs one sequence call, are bit-identical."""
    L, H, Wd, T, b = 4, 64, 128, 3, 2
    W = S.init_weights(L, seed=5)
    samples, cam = S.make_sequence(b, T, H, Wd, seed=99)
    model = _build(dev, L, 4, 3, W)
    ds, dc = to_dev(samples, dev), to_dev(cam, dev)
    first = model([ds, dc])["depth"].clone()
    model.reset_state()
    again = model([ds, dc])["depth"].clone()
    assert torch.equal(first, again)
    model.reset_state()
    for s in ds:
        last = model([[s], dc])["depth"]
    # the sequence call batches the encoder over the frames; per-sample arithmetic is identical
    assert torch.equal(first, last)


def test_model_large_search_windows(dev):
    """BASELINE config 5 geometry at reduced size: DSCV range 6 (13 hypotheses) and SNCV range 6
    (13x13 = 169 displacements per cut) -- the runtime-window kernels -- against the oracle."""
    L, H, Wd, T, b, rd, rs = 3, 64, 96, 2, 1, 6, 6
    W = S.init_weights(L, seed=9, dscv_range=rd, sncv_range=rs)
    samples, cam = S.make_sequence(b, T, H, Wd, seed=55)
    model = _build(dev, L, rd, rs, W)
    model([to_dev(samples, dev), to_dev(cam, dev)])
    omodel = O.M4Depth(W, L, dscv_range=rd, sncv_range=rs)
    _, seq = omodel(samples, cam)
    for l in range(L):
        k = 2 ** ((l + 1) // 2)
        fo, fg = omodel.levels[l].last_f_input, npy(model.d_estimator.levels[l].last_f_input)
        assert fo.shape[-1] == 13 * k + 169 * k + 6 == fg.shape[-1]
        cam_l = {"f": cam["f"] / F(2.0 ** (l + 1)), "c": cam["c"] / F(2.0 ** (l + 1))}
        est = model.last_estimates[-1][l]
        check_depth_and_parallax(npy(est["depth"]), npy(est["parallax"]), seq[-1][l]["depth"], seq[-1][l]["parallax"],
                                 samples[-1]["rot"], samples[-1]["trans"], cam_l, f"r=6 level {l}", frac_ok=0.98)
    # coarsest level: its cost-volume channels only depend on the encoder features, which differ
    # from the oracle's in the last bits (convolution order) -> at most one float16 ulp of a DSCV
    # entry (3e-5 at 1/16) or a float32 ulp-level SNCV difference
    lc = L - 1
    fo, fg = omodel.levels[lc].last_f_input, npy(model.d_estimator.levels[lc].last_f_input)
    err = np.abs(fg - fo).max()
    assert err < 1e-4, err


def test_frame_pipeline_is_bitwise_neutral(dev):
    """The (frame, level) wavefront on one stream per frame -- eager, round-robin over 8 streams for a
    10-frame sequence, and captured in the hipGraph for 4 frames -- gives bit-identical depth to the
    single-stream loop."""
    from m4depth_amd import network as net
    old = net.level_pipeline_streams
    try:
        L, H, Wd, b = 3, 64, 96, 2
        W = S.init_weights(L, seed=6)
        for T in (4, 10):
            samples, cam = S.make_sequence(b, T, H, Wd, seed=100 + T)
            ds, dc = to_dev(samples, dev), to_dev(cam, dev)
            net.level_pipeline_streams = 0
            model = _build(dev, L, 4, 3, W)
            ref = model([ds, dc])["depth"].clone()
            net.level_pipeline_streams = 8
            model = _build(dev, L, 4, 3, W)
            assert model.d_estimator.pipeline_streams_for(ds, dev) == min(T, 8)
            got = model([ds, dc])["depth"].clone()
            assert torch.equal(ref, got), f"eager pipeline differs at T={T}"
            if T == 4:
                data = {k: torch.stack([s[k] for s in ds], dim=1) for k in ("depth", "RGB_im", "rot", "trans")}
                data["new_traj"] = torch.stack([torch.from_numpy(s["new_traj"]) for s in samples], dim=1)
                data["camera"] = dc
                model = _build(dev, L, 4, 3, W)
                runner = net.GraphedSequence(model, data)
                for _ in range(2):
                    out = runner(data).clone()
                    torch.cuda.synchronize()
                    assert torch.equal(ref, out), "captured pipeline differs"
    finally:
        net.level_pipeline_streams = old


def test_encoder_statistics_up_front_are_bitwise_neutral(dev):
    """Level 0's DINL statistics of all frames taken in the first encoder batch's launches (m4d_enc_level0_stats over the whole
    sequence, m4d_enc_level0_apply per batch) against each batch computing its own (m4d_enc_level0_fwd): same feature maps and
    depth, bit for bit; and four launches fewer are not claimed -- the same kernels run, on more images at once."""
    from m4depth_amd import network as net, network_ops as nops
    old = net.encoder_stats_up_front
    try:
        L, H, Wd, b, T = 3, 64, 96, 2, 4
        W = S.init_weights(L, seed=12)
        samples, cam = S.make_sequence(b, T, H, Wd, seed=77)
        ds, dc = to_dev(samples, dev), to_dev(cam, dev)
        # frames as views of one [b,T,H,W,3] tensor (test_step's unstacking): the FrameStack path
        seq = torch.stack([s["RGB_im"] for s in ds], dim=1).contiguous()
        for t in range(T):
            ds[t]["RGB_im"] = seq[:, t]
        outs = {}
        for flag in (False, True):
            net.encoder_stats_up_front = flag
            model = _build(dev, L, 4, 3, W)
            outs[flag] = model([ds, dc])["depth"].clone()
        assert torch.equal(outs[False], outs[True])
        enc = model.encoder
        stack = net._stack_frames(ds)
        assert isinstance(stack, nops.FrameStack)
        mean, var = enc.head_stats(stack)
        whole = enc(stack)
        for a, z in ((0, 2), (2, 4), (1, 2)):
            part = enc(net._stack_frames(ds[a:z]), head_stats=(mean[a * b:z * b], var[a * b:z * b]))
            for lw, lp in zip(whole, part):
                assert torch.equal(lw[a * b:z * b], lp)
    finally:
        net.encoder_stats_up_front = old


def test_one_launch_pyramid_reset_is_bitwise_the_per_level_reset(dev):
    """m4d_pyramid_reset (the new-trajectory frame of every level in one launch) against the per-level reset branch
    (m4d_level_pre_normalize level by level, m4depth_network.py:207-214): every estimate of the reset frame, every level's
    seeded state, and the frames that follow are the same bits -- single stream, frame pipeline and hipGraph; a sequence with a
    second reset frame in the middle takes the fused launch on the single-stream path and the per-level one in the pipeline."""
    from m4depth_amd import network as net, _lib
    old = (net.fused_pyramid_reset, net.level_pipeline_streams)
    try:
        L, H, Wd, b, T = 4, 96, 160, 2, 5
        W = S.init_weights(L, seed=9)
        samples, cam = S.make_sequence(b, T, H, Wd, seed=321)
        samples[3]["new_traj"] = np.ones_like(samples[3]["new_traj"])              # a reset frame in mid-sequence
        ds, dc = to_dev(samples, dev), to_dev(cam, dev)
        results = {}
        for fused in (False, True):
            for streams in (0, 8):
                net.fused_pyramid_reset, net.level_pipeline_streams = fused, streams
                model = _build(dev, L, 4, 3, W)
                n0 = _lib.lib.m4d_launch_count()
                out = model([ds, dc])
                launches = _lib.lib.m4d_launch_count() - n0
                ests = [[{k: v.clone() for k, v in e.items()} for e in fr] for fr in model.last_estimates]
                state = [(lv.prev_f_maps.clone(), lv.depth_prev_t.clone()) for lv in model.d_estimator.levels]
                results[(fused, streams)] = (out["depth"].clone(), ests, state, launches)
        ref = results[(False, 0)]
        for key, got in results.items():
            assert torch.equal(ref[0], got[0]), key
            for fr_r, fr_g in zip(ref[1], got[1]):
                for e_r, e_g in zip(fr_r, fr_g):
                    for k in e_r:
                        assert torch.equal(e_r[k], e_g[k]), (key, k)
            for (f_r, d_r), (f_g, d_g) in zip(ref[2], got[2]):
                assert torch.equal(f_r, f_g) and torch.equal(d_r, d_g), key
        # the reset frame's estimates are the constants of :198-204
        fr0 = ref[1][0]
        for i, e in enumerate(fr0):                                                 # fine -> coarse
            assert torch.all(e["depth"] == 1000.0) and torch.all(e["other"] == 0.0)
            assert torch.all(e["parallax"] == 2.0 ** (L - 1 - i))
        # launches: two reset frames x (L - 1) launches fewer on one stream, one reset frame's worth in the pipeline
        assert results[(False, 0)][3] - results[(True, 0)][3] == 2 * (L - 1)
        assert results[(False, 8)][3] - results[(True, 8)][3] == L - 1
    finally:
        net.fused_pyramid_reset, net.level_pipeline_streams = old


@pytest.mark.parametrize("H,Wd,rd,rs,name", [(384, 1280, 4, 3, "configs[1]"), (768, 2560, 6, 6, "configs[4]")])
def test_fullsize_configs_properties(dev, H, Wd, rd, rs, name):
    """BASELINE.json's full-size geometries, 6 levels, batch 1 (no oracle run at these sizes: size-independent
    properties).  768x2560 with 13 DSCV hypotheses and 13x13 SNCV displacements is the large-window configuration: the
    runtime-window kernels, LDS tile shrinking and the 470-channel / 1462-channel refiner inputs at full scale."""
    L, T, b = 6, 3, 1
    W = S.init_weights(L, seed=21, dscv_range=rd, sncv_range=rs)
    samples, cam = S.make_sequence(b, T, H, Wd, seed=77)
    model = _build(dev, L, rd, rs, W)
    ds, dc = to_dev(samples, dev), to_dev(cam, dev)
    # frame 0 alone = new_traj: the reset branch (Appendix B invariant 9)
    first = model([ds[:1], dc])["depth"]
    assert first.shape == (b, H, Wd, 1) and torch.all(first == 1000.0)
    for l, lvl in enumerate(model.d_estimator.levels):
        assert torch.all(lvl.depth_prev_t == 1000.0)
        fs = lvl.prev_f_maps
        k = 2 ** ((l + 1) // 2)
        n2 = (fs.reshape(*fs.shape[:3], k, -1) ** 2).sum(-1)
        assert torch.allclose(n2, torch.ones_like(n2), atol=1e-5)           # the state holds the NORMALISED features
    model.reset_state()
    out = model([ds, dc])["depth"].clone()
    assert out.shape == (b, H, Wd, 1) and torch.isfinite(out).all()
    for l in range(L):
        k = 2 ** ((l + 1) // 2)
        fin = model.d_estimator.levels[l].last_f_input
        assert fin.shape == (b, H >> (l + 1), Wd >> (l + 1), (2 * rd + 1) * k + (2 * rs + 1) ** 2 * k + 6)
        assert torch.isfinite(fin).all()
        est = model.last_estimates[-1][l]
        cam_l = {"f": dc["f"] / float(2 ** (l + 1)), "c": dc["c"] / float(2 ** (l + 1))}
        import m4depth_amd as M
        # depth and parallax of a level are tied by parallax2depth with the level's intrinsics, bit for bit
        assert torch.equal(est["depth"], M.parallax2depth(est["parallax"], ds[-1]["rot"], ds[-1]["trans"], cam_l))
        lo, hi = np.exp(-7.0) / 2.0 ** (l + 1 - 3), np.exp(7.0) / 2.0 ** (l + 1 - 3)
        assert est["parallax"].min() >= lo * (1 - 1e-5) and est["parallax"].max() <= hi * (1 + 1e-5)     # exp(clip(., -7, 7)) / 2^(l-3)
    # the output is the nearest x2 upsample of the finest level
    fine = model.last_estimates[-1][0]["depth"]
    assert torch.equal(out[:, ::2, ::2], fine) and torch.equal(out[:, 1::2, 1::2], fine)
    # deterministic: a second run from the same state gives the same bits
    model.reset_state()
    assert torch.equal(model([ds, dc])["depth"], out)


def test_main_eval_with_host_resident_input(dev, tmp_path, capsys):
    """python -m m4depth_amd.main --mode=eval --host_input: the batch is handed over from pinned host memory every step
    (PCIe inside the loop); same metrics file as the HBM-resident run, bit for bit, plus the PCIe-inclusive rate."""
    from m4depth_amd import main as MAIN
    common = ["--mode", "eval", "--arch_depth", "3", "--seq_len", "3", "--batch_size", "2", "--n_batches", "3",
              "--height", "64", "--width", "96"]
    assert MAIN.main(common + ["--ckpt_dir", str(tmp_path / "a")]) == 0
    assert MAIN.main(common + ["--ckpt_dir", str(tmp_path / "b"), "--host_input", "--graph"]) == 0
    out = capsys.readouterr().out
    assert "host-resident input" in out and "frames/s" in out
    a = np.loadtxt(tmp_path / "a" / "perfs-synthetic.txt")
    b = np.loadtxt(tmp_path / "b" / "perfs-synthetic.txt")
    assert a.shape == (7,) and np.array_equal(a, b)


def test_taped_sequence_is_bitwise_the_graphed_sequence(dev):
    """network.TapedSequence (launch tapes of libm4depth_hip.so replayed as plain stream launches, one stream per frame)
    against network.GraphedSequence (one hipGraph) and the eager forward: the same depth bits, stable over replays, new input
    batches picked up through the static buffers; the recorded tapes hold every launch of the step."""
    import m4depth_amd as M
    from m4depth_amd import network as net, _lib
    if not _lib.has_experiments:
        with pytest.raises(RuntimeError, match="experiments build"):
            net.TapedSequence(None, None)
        pytest.skip("the launch tape is an experiment: make EXPERIMENTS=1 (include/m4depth_hip_experiments.h)")
    L, H, Wd, T, b = 4, 96, 160, 4, 2
    W = S.init_weights(L, seed=12)
    samples, cam = S.make_sequence(b, T, H, Wd, seed=55)
    samples2, _ = S.make_sequence(b, T, H, Wd, seed=56)

    def batch(smp):
        d = {k: torch.stack([to_dev(s[k], dev) for s in smp], dim=1) for k in ("depth", "RGB_im", "rot", "trans")}
        d["new_traj"] = torch.stack([torch.from_numpy(s["new_traj"]) for s in smp], dim=1)
        d["camera"] = to_dev(cam, dev)
        return d
    d1, d2 = batch(samples), batch(samples2)
    models = [_build(dev, L, 4, 3, W) for _ in range(3)]
    eager1 = models[0]([to_dev(samples, dev), to_dev(cam, dev)])["depth"].clone()
    models[0].reset_state()
    eager2 = models[0]([to_dev(samples2, dev), to_dev(cam, dev)])["depth"].clone()
    graphed = net.GraphedSequence(models[1], d1)
    taped = net.TapedSequence(models[2], d1)
    assert taped.launches_per_step() > 50 and all(n > 0 for _, n, _ in taped.tapes.values())
    for d, want in ((d1, eager1), (d2, eager2), (d1, eager1)):
        g = graphed(d).clone()
        t = taped(d).clone()
        torch.cuda.synchronize()
        assert torch.equal(g, want) and torch.equal(t, want)
    est_t, est_g = models[2].last_estimates, models[1].last_estimates
    assert len(est_t) == T and all(torch.equal(est_t[-1][l]["parallax"], est_g[-1][l]["parallax"]) for l in range(L))
    with pytest.raises(ValueError):
        bad = dict(d1)
        bad["RGB_im"] = d1["RGB_im"][:, :, :-2]
        taped(bad)
