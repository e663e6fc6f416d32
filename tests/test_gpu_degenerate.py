"""Degenerate inputs on the MI355X (DESIGN.md "Degenerate inputs", rules R1-R4): a stationary camera (trans = 0: every DSCV
query is 0/0), an epipole pixel, all-zero feature cuts (NaN normalised features), queries 1e6 pixels away and at +-Inf, a zero
denominator in prev_d2para -- the cases of tests/degenerate_cases.py, kept on their edge by tests/test_degenerate_oracle.py.

Every input is finite; the non-finite values arise inside the kernels.  (Two ops take the query itself as their input:
``dense_image_warp`` and ``_interpolate_bilinear`` get the case's own sweep queries, evaluated on the host -- NaN / Inf where
the case makes them -- since nothing else reaches R1 in those two kernels.)

Tolerances: everything built from + - * / sqrt, the float16 casts and the clamps is compared BIT FOR BIT (NaN equal to NaN:
``helpers.assert_bits_equal``), the int32 index grids exactly; the two log channels of the refiner input and exp() in the level
tails keep the suite's 2e-6 relative bar (libm differs) on finite entries, with equal NaN / +Inf / -Inf masks.

Nothing here is built to fault: every index a kernel derives from a query goes through ``m4d_bilinear_axis`` (the table of
routes is in DESIGN.md), and part d places inputs and outputs inside sentinel-filled allocations to show it.

Part f runs the BACKWARD on the same cases (rules R5, R6 and R4 for gradients) against autodiff of the rule-bearing training
restatement (oracle/m4depth_oracle_train.py; tests/test_degenerate_oracle.py shows that its non-finite masks do not depend on
its precision): NaN / +Inf / -Inf masks equal on 100 % of the entries, the suite's bars on the finite ones PER SAMPLE.
Measured on the MI355X, largest max |diff| / max |finite ref of the sample| over all cases and samples (bar):
  m4d_dscv_bwd              g_c1 1.5e-4, g_c2 1.3e-6, g_disp_prev_t 5.0e-6, g_disp 2.7e-6 (4e-3); with the LDS window off alike
  m4d_sncv_bwd              g_c1 4.7e-7, g_c2 3.5e-7; both inputs one map 2.8e-7 (1e-5)
  m4d_normalize_cuts_bwd    3.3e-7 (1e-5)
  m4d_level_post_bwd        1.1e-8 (1e-5)
  m4d_loss_level_fwd / bwd  loss 5.5e-8 / 6.4e-9 relative (2e-6), g_pred 5.6e-8 / 1.0e-7 (1e-5)              [map / velodyne]
  conv layer 32 -> 32       weight gradient 1.1e-7, bias 7.0e-8, data gradient 3.3e-7 (2e-5)
  photometric, stationary   term / photo / smooth 4.1e-8 / 3.0e-8 / 4.0e-8 (bar 1.6e-7), g_depth 1.2e-6 of max |g| (bar 5.2e-6)
  train step, stationary    loss 9.017019 eager (the restatement's bits) and 9.017015 replayed; the 21 refiner kernels of the three
                            levels carry NaN gradients, the 35 other tensors none: restatement, eager and graph alike
No kernel diverged from the rules."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import m4depth_oracle as O
from oracle import m4depth_oracle_train as OT
from helpers import F, camera_np, motion_np, to_dev, npy, assert_bits_equal, rel_err
import degenerate_cases as D

pytestmark = pytest.mark.gpu

CASES = pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
S_ENC = [16, 32, 64, 96, 128, 192]


@pytest.fixture(scope="module")
def M():
    import m4depth_amd
    return m4depth_amd


def _assert_masks_and_close(got, want, what, bar=2e-6, floor=1e-3):
    """exp / log outputs: the same NaN, +Inf and -Inf entries, and ``bar`` relative on the finite ones."""
    got, want = np.asarray(got, F), np.asarray(want, F)
    for name, fn in (("NaN", np.isnan), ("+Inf", np.isposinf), ("-Inf", np.isneginf)):
        assert np.array_equal(fn(got), fn(want)), f"{what}: {name} mask differs ({int(fn(got).sum())} vs {int(fn(want).sum())})"
    fin = np.isfinite(want)
    if fin.any():
        err = rel_err(got[fin], want[fin], floor).max()
        assert err < bar, f"{what}: {err:.2e} relative on the finite entries"


def _features(case, dev):
    """The case's feature maps normalised ON THE DEVICE (a zero cut becomes NaN there), checked against the oracle's."""
    from m4depth_amd import network_ops as nops
    r = D.reference(case)
    d = r["inputs"]
    c1 = nops.normalize_cuts(to_dev(d["f1"], dev), d["k"])
    c2 = nops.normalize_cuts(to_dev(d["f2"], dev), d["k"])
    assert_bits_equal(npy(c1), r["c1"], f"{case}: normalize_cuts(f1)")
    assert_bits_equal(npy(c2), r["c2"], f"{case}: normalize_cuts(f2)")
    return r, d, c1, c2


# ================================================================================== a. op level, against the oracle
@CASES
def test_converters_reproject_and_gathers(M, dev, case):
    r, d, c1, c2 = _features(case, dev)
    rot, trans, cam = to_dev(d["rot"], dev), to_dev(d["trans"], dev), to_dev(d["cam"], dev)
    disp, dprev = to_dev(d["disp"], dev), to_dev(d["depth_prev_t"], dev)
    assert_bits_equal(npy(M.parallax2depth(disp, rot, trans, cam)), r["p2d"], "parallax2depth")
    assert_bits_equal(npy(M.depth2parallax(dprev, rot, trans, cam)), r["d2p"], "depth2parallax")
    assert_bits_equal(npy(M.prev_d2para(dprev, rot, trans, cam)), r["pd2p"], "prev_d2para")
    assert_bits_equal(npy(M.recompute_depth(dprev, rot, trans, cam)), r["recompute"], "recompute_depth")
    out, (pmr, rotc) = M.reproject(c2[..., :4].contiguous(), to_dev(D.reproject_depth(d), dev), rot, trans, cam)
    assert_bits_equal(npy(out), r["reproject"], "reproject")
    assert_bits_equal(npy(pmr), r["reproject_pmr"], "reproject aux 0")
    assert_bits_equal(npy(rotc), r["reproject_rotc"], "reproject aux 1")
    out, idx = M.dense_image_warp(c2, to_dev(np.array(r["flow"]), dev), return_index=True)
    assert np.array_equal(npy(idx), r["warp_idx"]), "dense_image_warp index grid"
    assert_bits_equal(npy(out), r["warp"], "dense_image_warp")
    out, idx = M._interpolate_bilinear(c2, to_dev(np.array(r["points"]), dev), return_index=True)
    assert np.array_equal(npy(idx), r["interp_idx"]), "_interpolate_bilinear index grid"
    assert_bits_equal(npy(out), r["interp"], "_interpolate_bilinear")


@CASES
def test_cost_volumes_every_dscv_variant(M, dev, case):
    """get_parallax_sweeping_cv under every kernel variant and both float16 accumulations, cost_volume and the merged launch
    m4d_dscv_sncv_fwd: cv, the warped parallax, the NaN mask and the int32 index grid as the oracle has them."""
    from m4depth_amd._lib import lib, check, dptr, stream_ptr
    r, d, c1, c2 = _features(case, dev)
    b, h, w, C, k = D.B, d["h"], d["w"], d["C"], d["k"]
    rot, trans, cam = to_dev(d["rot"], dev), to_dev(d["trans"], dev), to_dev(d["cam"], dev)
    disp = to_dev(d["disp"], dev)
    dpt = M.prev_d2para(to_dev(d["depth_prev_t"], dev), rot, trans, cam)
    assert_bits_equal(npy(dpt), r["pd2p"], "prev_d2para")
    try:
        for variant in range(5):
            lib.m4d_dscv_set_variant(variant)
            for acc in ("fp32_round", "fp16_seq"):
                cv, pd, idx = M.get_parallax_sweeping_cv(c1, c2, dpt, disp, rot, trans, cam, D.DSCV_RANGE, k, cv_accum=acc,
                                                         return_index=True)
                what = f"{D.case_id(case)} variant {variant} {acc}"
                assert np.array_equal(npy(idx), r["idx"]), f"{what}: index grid"
                assert_bits_equal(npy(cv), r[f"cv_{acc}"], f"{what}: cv")
                assert_bits_equal(npy(pd), r["prev_disp"], f"{what}: prev_disp")
    finally:
        lib.m4d_dscv_set_variant(1)
    assert_bits_equal(npy(M.cost_volume(c1, c1, D.SNCV_RANGE, nbre_cuts=k)), r["sncv_auto"], "cost_volume(c1, c1)")
    assert_bits_equal(npy(M.cost_volume(c1, c2, D.SNCV_RANGE, nbre_cuts=k)), r["sncv"], "cost_volume(c1, c2)")
    ncp, mo2 = 2 * D.DSCV_RANGE + 1, (2 * D.SNCV_RANGE + 1) ** 2
    stride = ncp * k + mo2 * k + 3
    for acc_i, acc in enumerate(("fp32_round", "fp16_seq")):
        buf = torch.zeros(b, h, w, stride, device=dev)
        pd = torch.empty(b, h, w, ncp, device=dev)
        base = buf.data_ptr()
        check(lib.m4d_dscv_sncv_fwd(dptr(c1), dptr(c2), dptr(dpt), dptr(disp), dptr(rot), 4, dptr(trans), dptr(cam["f"]),
                                    dptr(cam["c"]), b, h, w, C, D.DSCV_RANGE, k, acc_i, ctypes.c_void_p(base), stride, dptr(pd),
                                    None, 1, 1.0, D.SNCV_RANGE, ctypes.c_void_p(base + 4 * (ncp * k + 1)), stride, stream_ptr()),
              "m4d_dscv_sncv_fwd")
        assert_bits_equal(npy(buf[..., :ncp * k]), r[f"cv_{acc}"], f"merged launch {acc}: cv")
        assert_bits_equal(npy(pd), r["prev_disp"], f"merged launch {acc}: prev_disp")
        assert_bits_equal(npy(buf[..., ncp * k + 1:ncp * k + 1 + mo2 * k]), r["sncv_auto"], f"merged launch {acc}: sncv")


# ================================================================================== b. the fused level fronts
def _degenerate_frame(rng, b, h, w, C, k, depth_state):
    """Frame 1 of the front tests.  Sample 0: stationary.  Sample 1: forward motion under an identity rotation (an epipole pixel
    when h and w are odd), zero feature cuts, a coarser parallax that puts hypotheses on both clamps (and a negative one: the
    log feature is NaN), and a depth memory equal to tz on four pixels (prev_d2para = Inf).  Returns the finite inputs and the
    planted depth state."""
    rot, trans = motion_np(rng, b, quat=True, t_scale=(3.0, 3.0, 1.0))
    trans[0] = 0.0
    rot[1] = np.array([1.0, 0.0, 0.0, 0.0], F)
    trans[1] = np.array([0.0, 0.0, 0.3], F)
    f = rng.standard_normal([b, h, w, C]).astype(F)
    nc = C // k
    f[1, h // 3, w // 2, (k - 1) * nc:] = 0.0
    f[1, h // 2:h // 2 + 2, w // 4:w // 4 + 3, :nc] = 0.0
    f[0, 0, 0, :] = 0.0
    ph, pw = (h + 1) // 2, (w + 1) // 2
    prev = {"depth": (1 + 50 * rng.random([b, ph, pw, 1])).astype(F),
            "parallax": (0.2 + 2 * rng.random([b, ph, pw, 1])).astype(F),
            "other": rng.standard_normal([b, ph, pw, 4]).astype(F)}
    prev["parallax"][:, 0, 0, 0] = 1e6
    prev["parallax"][:, ph - 1, pw - 1, 0] = 5e5 - 1.0
    prev["parallax"][:, ph // 2, pw // 2, 0] = -5.0
    prev["parallax"][:, 0, pw - 1, 0] = 0.0
    state = depth_state.copy()
    for (j, i) in D.d2para_plant(h, w):
        state[1, j, i, 0] = trans[1, 2]
    return rot, trans, f, prev, state


def _front_routes_on_degenerate_frames(M, dev, depth, h, w, cv_accum, rd, rs, route, monkeypatch):
    """Three frames -- reset, a degenerate frame, a healthy frame on the state the degenerate one left -- through a fused front
    (``route`` "front": m4d_level_front / _r; "small": m4d_level_front_small) and through the separate launches: refiner input,
    feature state, depth state and outputs bit for bit between the two, and the refiner input against the oracle's f_input
    (the oracle level is handed the GPU's state before each frame: the convolutions behind the front are not compared)."""
    from m4depth_amd import network as net, network_ops as nops, synthetic as S
    b = D.B
    rng = np.random.default_rng(8100 + depth * 10 + h)
    C, k = S_ENC[depth - 1], 2 ** (depth // 2)
    W = S.init_weights(6, seed=4, dscv_range=rd, sncv_range=rs)
    settings = {"nbre_lvls": 6, "is_training": False, "ablation": M.M4depthAblationParameters(), "cv_accum": cv_accum,
                "dscv_range": rd, "sncv_range": rs}
    levels = []
    for _ in range(2):
        gl = M.DepthEstimatorLevel(settings, depth)
        convs = list(gl.disp_refiner.prep_conv_layers) + list(gl.disp_refiner.est_d_conv_layers)
        for i, cv in enumerate(convs):
            cv.load_hwio(W[f"lvl.{depth}.conv.{i}.kernel"], W[f"lvl.{depth}.conv.{i}.bias"], dev)
        levels.append(gl)
    ol = O.DepthEstimatorLevel(W, depth, dscv_range=rd, sncv_range=rs, cv_accum=cv_accum)
    cam_np = camera_np(b, h, w)
    cam = to_dev(cam_np, dev)
    ncp = 2 * rd + 1
    f_in = (ncp + (2 * rs + 1) ** 2) * k + 6
    logs = [ncp * k, f_in - 1]
    if route == "small":
        monkeypatch.setattr(net, "fused_front_min_pixels", 10 ** 9)
        assert levels[0].wants_prenormalized(b, h, w, C)
    else:
        monkeypatch.setattr(net, "fused_front_coarse_min_pixels", 0)
        assert bool(net.lib.m4d_level_front_supported(C, k, rd, rs, (f_in + 7) // 8 * 8))
    for step in range(3):
        if step == 1:
            rot, trans, f, prev, state = _degenerate_frame(rng, b, h, w, C, k, npy(levels[1].depth_prev_t))
            for gl in levels:
                gl.depth_prev_t.copy_(to_dev(state, dev))
        else:
            rot, trans = motion_np(rng, b, quat=True, t_scale=(3.0, 3.0, 1.0))
            f = rng.standard_normal([b, h, w, C]).astype(F)
            prev = {"depth": (1 + 50 * rng.random([b, (h + 1) // 2, (w + 1) // 2, 1])).astype(F),
                    "parallax": (0.2 + 2 * rng.random([b, (h + 1) // 2, (w + 1) // 2, 1])).astype(F),
                    "other": rng.standard_normal([b, (h + 1) // 2, (w + 1) // 2, 4]).astype(F)}
        for name, x in (("rot", rot), ("trans", trans), ("f", f), *prev.items()):
            assert np.isfinite(x).all(), f"step {step}: input {name} must be finite"
        nt = np.full([b], step == 0)
        fd, prevd = to_dev(f, dev), to_dev(prev, dev)
        if step > 0:
            ol.prev_f_maps, ol.depth_prev_t = npy(levels[1].prev_f_maps).copy(), npy(levels[1].depth_prev_t).copy()
        outs, fins = [], []
        for fused, gl in zip((True, False), levels):
            kw = {}
            if route == "small":
                if fused:
                    kw["curr_f_normalized"] = nops.normalize_levels([(fd, gl.nbre_cuts)])[0]
            else:
                monkeypatch.setattr(net, "fused_front", fused)
                monkeypatch.setattr(net, "fused_front_min_pixels", 0)
            n0 = int(net.lib.m4d_launch_count())
            outs.append(gl(fd, prevd, to_dev(rot, dev), to_dev(trans, dev), cam, nt, **kw))
            launches = int(net.lib.m4d_launch_count()) - n0
            fins.append(npy(gl.last_f_input).copy() if step > 0 else None)
            if step > 0:
                outs[-1]["launches"] = launches
        what = f"level {depth} {h}x{w} {route} step {step}"
        assert_bits_equal(npy(levels[0].prev_f_maps), npy(levels[1].prev_f_maps), f"{what}: feature state")
        assert_bits_equal(npy(levels[0].depth_prev_t), npy(levels[1].depth_prev_t), f"{what}: depth state")
        for key in ("depth", "parallax", "other"):
            assert_bits_equal(npy(outs[0][key]), npy(outs[1][key]), f"{what}: {key}")
        if step == 0:
            continue
        assert outs[0]["launches"] < outs[1]["launches"], f"{what}: the fused route was not taken"
        assert_bits_equal(fins[0], fins[1], f"{what}: refiner input, fused vs separate")
        with np.errstate(all="ignore"):
            ol(f, prev, rot, trans, cam_np, nt)
        want = ol.last_f_input
        rest = [c for c in range(f_in) if c not in logs]
        assert_bits_equal(fins[0][..., rest], want[..., rest], f"{what}: refiner input vs the oracle")
        for c in logs:
            _assert_masks_and_close(fins[0][..., c], want[..., c], f"{what}: log channel {c}")
        assert float(np.isfinite(want).mean()) >= 0.9, f"{what}: the oracle's refiner input is mostly non-finite"
        if step == 1:
            assert not np.isfinite(want).all(), f"{what}: the degenerate frame left the refiner input finite"
            for key in ("depth", "parallax"):                                           # R2: the tail's clamp drops the NaN
                assert torch.isfinite(outs[0][key]).all(), f"{what}: {key} not finite"
            assert torch.isfinite(levels[0].depth_prev_t).all()


@pytest.mark.parametrize("depth,h,w,cv_accum", [(1, 37, 45, "fp32_round"), (2, 21, 27, "fp16_seq"), (3, 19, 33, "fp32_round"),
                                                (4, 21, 19, "fp32_round"), (5, 13, 17, "fp16_seq"), (6, 13, 11, "fp32_round")])
def test_fused_level_front_on_degenerate_frames(M, dev, depth, h, w, cv_accum, monkeypatch):
    _front_routes_on_degenerate_frames(M, dev, depth, h, w, cv_accum, 4, 3, "front", monkeypatch)


def test_fused_level_front_large_windows_on_degenerate_frames(M, dev, monkeypatch):
    _front_routes_on_degenerate_frames(M, dev, 2, 19, 21, "fp32_round", 6, 6, "front", monkeypatch)


@pytest.mark.parametrize("depth,h,w,cv_accum", [(4, 21, 19, "fp16_seq"), (5, 13, 17, "fp32_round"), (6, 13, 11, "fp32_round"),
                                                (6, 6, 20, "fp32_round")])
def test_level_front_small_on_degenerate_frames(M, dev, depth, h, w, cv_accum, monkeypatch):
    _front_routes_on_degenerate_frames(M, dev, depth, h, w, cv_accum, 4, 3, "small", monkeypatch)


# ================================================================================== c. the level tails
TAIL_PLANTS = [((0, 0), np.nan), ((3, 7), np.inf), ((5, 2), -np.inf), ((10, 13), np.nan), ((10, 14), np.inf)]


def test_level_post_drops_nan_to_the_lower_bound(M, dev):
    """level_post and its masked form on a refiner output with NaN, +Inf and -Inf in channel 0 and in the "other" channels:
    parallax exp(-7) / scale, exp(7) / scale, exp(-7) / scale (R2), depth from the kernel's own parallax bit for bit, "other"
    passed through bit for bit."""
    from m4depth_amd import network_ops as nops
    rng = np.random.default_rng(31)
    b, h, w, scale = 2, 11, 15, F(4.0)
    rot, trans = motion_np(rng, b)
    cam = camera_np(b, h, w)
    ro = (rng.standard_normal([b, h, w, 5]) * 4).astype(F)
    for n, ((j, i), v) in enumerate(TAIL_PLANTS):
        ro[:, j, i, 0] = v
        ro[:, (j + 1) % h, i, 1 + n % 4] = v
    want_p = (np.exp(np.fmin(np.fmax(ro[..., :1], F(-7)), F(7))) / scale).astype(F)
    lo, hi = np.exp(F(-7)) / scale, np.exp(F(7)) / scale
    for (j, i), v in TAIL_PLANTS:
        assert want_p[0, j, i, 0] == (hi if v == np.inf else lo)
    args = (to_dev(ro, dev), to_dev(rot, dev), to_dev(trans, dev), to_dev(cam, dev), float(scale))
    state = torch.empty((b, h, w, 1), device=dev)
    p, d, o = nops.level_post(*args, depth_state=state)
    assert torch.isfinite(p).all() and torch.isfinite(d).all()
    assert rel_err(npy(p), want_p).max() < 2e-6
    assert_bits_equal(npy(d), O.parallax2depth(npy(p), rot, trans, cam), "depth from the kernel's own parallax")
    assert_bits_equal(npy(state), npy(d), "depth state")
    assert_bits_equal(npy(o), ro[..., 1:], "other")
    state_m = torch.full((b, h, w, 1), -1.0, device=dev)
    pm, dm, om = nops.level_post(*args, depth_state=state_m, reset=torch.tensor([False, True], device=dev), reset_parallax=2.0)
    for got, ref, name in ((pm, p, "parallax"), (dm, d, "depth"), (om, o, "other"), (state_m, state, "depth state")):
        assert_bits_equal(npy(got)[:1], npy(ref)[:1], f"masked close, continuing sample: {name}")
    assert torch.all(pm[1] == 2.0) and torch.all(dm[1] == 1000.0) and torch.all(om[1] == 0.0) and torch.all(state_m[1] == 1000.0)


@pytest.mark.parametrize("kernel", ["f32", "bf16x3"])
def test_fused_refiner_tails_drop_nan_to_the_lower_bound(M, dev, kernel):
    """refiner_tail / refiner_tail6 and their masked forms.  Their refiner output never leaves the kernel, so the non-finite
    values are planted (i) through the last layer's bias -- NaN, +Inf, -Inf on channel 0 of every pixel, NaN on one "other"
    channel -- where the parallax must be exactly the clamp's bound and the untouched channels those of the healthy run bit for
    bit, and (ii) through one finite pixel of 3e38 in the 32-channel activation, whose sums overflow inside the kernel: the
    parallax stays finite and inside the clamp, depth is parallax2depth of it bit for bit, and pixels more than two away (the
    reach of the two 3x3 layers) keep the healthy run's bits.  All tails agree with level_post on the healthy part under the
    suite's bars (refiner output 1e-5, parallax 3e-5)."""
    from m4depth_amd import network_ops as nops
    rng = np.random.default_rng(32)
    b, h, w, scale = 2, 19, 21, F(0.5)
    x = np.maximum(rng.standard_normal([b, h, w, 32]), -0.3).astype(F)
    k6 = (rng.standard_normal([3, 3, 32, 16]) * np.sqrt(2.0 / (9 * 32))).astype(F)
    k7 = (rng.standard_normal([3, 3, 16, 5]) * np.sqrt(1.0 / (9 * 16))).astype(F)
    k6[1, 1, :, 0] = 8.0                               # 32 x (3e38 * 8) overflows whatever the order of the sum (part ii)
    b6 = (0.1 * rng.standard_normal([16])).astype(F)
    b7 = (0.1 * rng.standard_normal([5])).astype(F)
    rot, trans = motion_np(rng, b)
    cam = camera_np(b, h, w)
    if kernel == "f32":
        w6, w7 = [to_dev(v, dev) for v in nops.pack_refiner_tail_weights(k6, k7)]
        fn = nops.refiner_tail
    else:
        w6, w7 = [torch.from_numpy(v.view(np.int16)).to(dev) for v in nops.pack_refiner_tail_weights6(k6, k7)]
        fn = nops.refiner_tail6
    motion = (to_dev(rot, dev), to_dev(trans, dev), to_dev(cam, dev), float(scale))

    def run(xx, bias7, **kw):
        state = torch.full((b, h, w, 1), -1.0, device=dev)
        p, d, o = fn(to_dev(xx, dev), w6, to_dev(b6, dev), w7, to_dev(bias7, dev), *motion, depth_state=state, **kw)
        assert_bits_equal(npy(state), npy(d), "depth state")
        keep = 1 if kw else 0                          # (the masked runs reset sample 0: its depth is the constant 1000)
        assert_bits_equal(npy(d)[keep:], O.parallax2depth(npy(p), rot, trans, cam)[keep:], "depth from the kernel's own parallax")
        return npy(p), npy(d), npy(o)

    p0, d0, o0 = run(x, b7)
    assert np.isfinite(p0).all() and np.isfinite(o0).all()
    # the healthy run against level_post on the oracle's refiner output: the tails agree under their existing bars
    mid = O.conv2d_same(x, k6, b6, 1)
    out5 = O.conv2d_same(np.where(mid > 0, mid, mid * F(0.1)).astype(F), k7, b7, 1)
    lp, _, lo_ = nops.level_post(to_dev(out5, dev), *motion)
    assert np.max(np.abs(o0 - npy(lo_))) < 1e-5 * max(1.0, np.abs(out5).max()) and rel_err(p0, npy(lp)).max() < 3e-5
    lo, hi = np.exp(F(-7)) / scale, np.exp(F(7)) / scale
    for v, bound in ((np.nan, lo), (np.inf, hi), (-np.inf, lo)):
        bias = b7.copy()
        bias[0], bias[2] = v, np.nan
        p, d, o = run(x, bias)
        assert rel_err(p, np.full_like(p, bound)).max() < 2e-6, f"bias {v}: parallax"
        assert np.isfinite(d).all()
        assert np.isnan(o[..., 1]).all(), "the NaN bias of an 'other' channel reaches every pixel"
        assert_bits_equal(o[..., [0, 2, 3]], o0[..., [0, 2, 3]], f"bias {v}: untouched channels")
        pm, dm, om = run(x, bias, reset=torch.tensor([True, False], device=dev), reset_parallax=4.0)
        assert_bits_equal(pm[1:], p[1:], "masked close: parallax")
        assert_bits_equal(dm[1:], d[1:], "masked close: depth")
        assert_bits_equal(om[1:], o[1:], "masked close: other")
        assert np.all(pm[0] == 4.0) and np.all(dm[0] == 1000.0) and np.all(om[0] == 0.0)
    xo = x.copy()
    pj, pi = 9, 10
    xo[0, pj, pi, :] = 3e38
    assert np.isfinite(xo).all()
    p, d, o = run(xo, b7)
    assert np.isfinite(p).all() and p.min() >= lo * (1 - 2e-6) and p.max() <= hi * (1 + 2e-6)
    assert not np.isfinite(o[0, pj, pi]).all(), "3e38 on 32 channels was meant to overflow the sums"
    far = np.ones([b, h, w], bool)
    far[0, pj - 2:pj + 3, pi - 2:pi + 3] = False
    assert_bits_equal(p[far], p0[far], "parallax away from the overflowing pixel")
    assert_bits_equal(o[far], o0[far], "other away from the overflowing pixel")


# ================================================================================== d. memory guards, raw C-ABI calls
SENTINEL = -0x3F213F22          # int32 bit pattern of the guard words (a finite negative float)
GUARD = 4096                    # guard words before and after every region


class _Arena:
    """One allocation filled with a sentinel; inputs and outputs are carved out of it with guard words on both sides, so a
    write past an output shows as a changed guard and a read past an input stays inside the test's own memory."""

    def __init__(self, dev, words):
        self.buf = torch.full((words,), SENTINEL, dtype=torch.int32, device=dev)
        self.at = GUARD
        self.outputs = []

    def _take(self, n):
        lo = self.at
        self.at = (lo + n + GUARD + 63) // 64 * 64
        assert self.at <= self.buf.numel(), "arena too small"
        return lo

    def put(self, array):
        t = torch.from_numpy(np.array(array))               # a copy: the shared reference is read-only
        lo = self._take(t.numel())
        view = self.buf[lo:lo + t.numel()].view(t.dtype).reshape(t.shape)
        view.copy_(t.to(self.buf.device))
        return view

    def out(self, shape, dtype=torch.float32):
        n = int(np.prod(shape))
        lo = self._take(n)
        self.outputs.append((lo, n))
        return self.buf[lo:lo + n].view(dtype).reshape(shape)

    def snapshot(self):
        self._before = self.buf.clone()

    def assert_only_outputs_changed(self, what):
        changed = self.buf != self._before
        for lo, n in self.outputs:
            assert bool((self.buf[lo:lo + n] != SENTINEL).any()), f"{what}: an output was not written"
            changed[lo:lo + n] = False
        bad = changed.nonzero().flatten()
        assert bad.numel() == 0, f"{what}: {bad.numel()} words outside the outputs changed, first at {int(bad[0])}"


GUARD_CASES = [c for c in D.CASES if c.kind in ("stationary", "far_query")]


@pytest.mark.parametrize("case", GUARD_CASES, ids=D.case_id)
def test_no_write_outside_the_outputs(M, dev, case):
    """m4d_dscv_fwd under every variant, m4d_dscv_sncv_fwd, m4d_dense_image_warp and m4d_interpolate_bilinear through the C ABI
    with every input and output inside a sentinel-filled allocation: the guard words before and after every region, and the
    inputs, are intact after the call, and the outputs carry the oracle's bits."""
    from m4depth_amd._lib import lib, check, stream_ptr
    r = D.reference(case)
    d = r["inputs"]
    b, h, w, C, k = D.B, d["h"], d["w"], d["C"], d["k"]
    assert np.isfinite(r["c1"]).all() and np.isfinite(r["c2"]).all() and np.isfinite(r["pd2p"]).all()
    ncp, mo2 = 2 * D.DSCV_RANGE + 1, (2 * D.SNCV_RANGE + 1) ** 2
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def arena():
        a = _Arena(dev, 2 * b * h * w * C + b * h * w * (2 * ncp * k + 4 * ncp + mo2 * k + 2 * C + 16) + 16 * GUARD + 4096)
        ins = {n: a.put(v) for n, v in (("c1", r["c1"]), ("c2", r["c2"]), ("dpt", r["pd2p"]), ("disp", d["disp"]), ("rot", d["rot"]),
                                        ("trans", d["trans"]), ("f", d["cam"]["f"]), ("c", d["cam"]["c"]))}
        assert ins["c1"].data_ptr() % 16 == 0 and ins["c2"].data_ptr() % 16 == 0
        return a, ins

    try:
        for variant in range(5):
            lib.m4d_dscv_set_variant(variant)
            a, t = arena()
            cv, pd, idx = a.out((b, h, w, ncp * k)), a.out((b, h, w, ncp)), a.out((b, h, w, ncp, 2), torch.int32)
            a.snapshot()
            check(lib.m4d_dscv_fwd(P(t["c1"]), P(t["c2"]), P(t["dpt"]), P(t["disp"]), P(t["rot"]), 4, P(t["trans"]), P(t["f"]),
                                   P(t["c"]), b, h, w, C, D.DSCV_RANGE, k, 0, P(cv), ncp * k, P(pd), None, 1, 1.0, P(idx),
                                   stream_ptr()), "m4d_dscv_fwd")
            what = f"{D.case_id(case)} m4d_dscv_fwd variant {variant}"
            a.assert_only_outputs_changed(what)
            assert np.array_equal(npy(idx), r["idx"]), f"{what}: index grid"
            assert_bits_equal(npy(cv), r["cv_fp32_round"], f"{what}: cv")
            assert_bits_equal(npy(pd), r["prev_disp"], f"{what}: prev_disp")
    finally:
        lib.m4d_dscv_set_variant(1)
    a, t = arena()
    cv, pd, sn = a.out((b, h, w, ncp * k)), a.out((b, h, w, ncp)), a.out((b, h, w, mo2 * k))
    a.snapshot()
    check(lib.m4d_dscv_sncv_fwd(P(t["c1"]), P(t["c2"]), P(t["dpt"]), P(t["disp"]), P(t["rot"]), 4, P(t["trans"]), P(t["f"]),
                                P(t["c"]), b, h, w, C, D.DSCV_RANGE, k, 0, P(cv), ncp * k, P(pd), None, 1, 1.0, D.SNCV_RANGE,
                                P(sn), mo2 * k, stream_ptr()), "m4d_dscv_sncv_fwd")
    a.assert_only_outputs_changed(f"{D.case_id(case)} m4d_dscv_sncv_fwd")
    assert_bits_equal(npy(cv), r["cv_fp32_round"], "merged launch: cv")
    assert_bits_equal(npy(sn), r["sncv_auto"], "merged launch: sncv")
    a, t = arena()
    flow, pts = a.put(r["flow"]), a.put(r["points"])
    wo, wi = a.out((b, h, w, C)), a.out((b, h, w, 2), torch.int32)
    io, ii = a.out((b, h * w, C)), a.out((b, h * w, 2), torch.int32)
    a.snapshot()
    check(lib.m4d_dense_image_warp(P(t["c2"]), P(flow), b, h, w, C, P(wo), P(wi), stream_ptr()), "m4d_dense_image_warp")
    check(lib.m4d_interpolate_bilinear(P(t["c2"]), P(pts), b, h, w, C, h * w, P(io), P(ii), stream_ptr()), "m4d_interpolate_bilinear")
    a.assert_only_outputs_changed(f"{D.case_id(case)} warps")
    assert np.array_equal(npy(wi), r["warp_idx"]) and np.array_equal(npy(ii), r["interp_idx"])
    assert_bits_equal(npy(wo), r["warp"], "m4d_dense_image_warp")
    assert_bits_equal(npy(io), r["interp"], "m4d_interpolate_bilinear")


# ================================================================================== e. sample independence (R4)
@pytest.mark.parametrize("case", [D.Case(k, "13x21") for k in D.KINDS], ids=D.case_id)
def test_a_degenerate_sample_leaves_its_neighbour_alone_op_level(M, dev, case):
    """Both cost volumes and the merged launch at batch 2: with either sample's data replaced by healthy data, the OTHER
    sample's outputs keep their bits."""
    from m4depth_amd import network_ops as nops
    d = D.make(case)
    rng = np.random.default_rng(77)
    k = d["k"]

    def run(x):
        dv = {n: to_dev(x[n], dev) for n in ("f1", "f2", "disp", "depth_prev_t", "rot", "trans")}
        cam = to_dev(x["cam"], dev)
        c1, c2 = nops.normalize_cuts(dv["f1"], k), nops.normalize_cuts(dv["f2"], k)
        dpt = M.prev_d2para(dv["depth_prev_t"], dv["rot"], dv["trans"], cam)
        cv, pd, idx = M.get_parallax_sweeping_cv(c1, c2, dpt, dv["disp"], dv["rot"], dv["trans"], cam, 4, k, return_index=True)
        return {"cv": npy(cv), "prev_disp": npy(pd), "idx": npy(idx).astype(F), "sncv": npy(M.cost_volume(c1, c2, 3, nbre_cuts=k)),
                "sncv_auto": npy(M.cost_volume(c1, c1, 3, nbre_cuts=k)), "p2d": npy(M.parallax2depth(dv["disp"], dv["rot"], dv["trans"], cam))}

    base = run(d)
    rot_h, trans_h = motion_np(rng, D.B, t_scale=(3.0, 3.0, 1.0))
    for s in range(D.B):
        healed = {n: (v.copy() if isinstance(v, np.ndarray) else v) for n, v in d.items()}
        healed["rot"][s], healed["trans"][s] = rot_h[s], trans_h[s]
        for n in ("f1", "f2"):
            healed[n][s] = rng.standard_normal(healed[n][s].shape).astype(F)
        healed["disp"][s] = (0.2 + 6.0 * rng.random(healed["disp"][s].shape)).astype(F)
        healed["depth_prev_t"][s] = (1.0 + 50.0 * rng.random(healed["depth_prev_t"][s].shape)).astype(F)
        got = run(healed)
        o = 1 - s
        for name in base:
            assert_bits_equal(got[name][o], base[name][o], f"{D.case_id(case)}: {name} of sample {o} with sample {s} healed")
        assert np.isfinite(got["cv"][s]).all() and np.isfinite(got["sncv"][s]).all(), "the healed sample is healthy"


def _model(dev, weights):
    import m4depth_amd as M
    model = M.M4Depth(nbre_levels=D.MODEL_LEVELS)
    model.load_numpy_weights(weights, dev)
    return model


def _frame(sample, cam, dev):
    g = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return {"RGB_im": g(sample["RGB_im"]), "rot": g(sample["rot"]), "trans": g(sample["trans"]), "new_traj": g(sample["new_traj"]),
            "camera": {k: g(v) for k, v in cam.items()}}


def _snapshot(model):
    out = []
    for lvl, est in zip(model.d_estimator.levels, model.last_estimates[-1]):
        out.append({"depth": npy(est["depth"]), "parallax": npy(est["parallax"]), "other": npy(est["other"]),
                    "prev_f": npy(lvl.prev_f_maps), "depth_prev_t": npy(lvl.depth_prev_t)})
    return out


def test_a_degenerate_stream_leaves_the_other_streams_alone(dev):
    """Four streams through M4Depth.stream_step (3 levels, 64 x 96, four frames), three times: every stream moving; stream 1
    stationary at frame 2; stream 2 with all-zero feature cuts at frame 2 (a 2 x 3 block of level 1's map and one cut of a
    level-2 pixel, zeroed in the encoder's output: no image gives an exactly zero cut behind the DINL layer).  Every OTHER
    stream's estimates, feature state and depth state are bitwise the all-moving run's at every level and frame, and the
    degenerate stream itself differs."""
    b, T, bad_frame = 4, 4, D.STATIONARY_FRAME
    W, samples, cam = D.model_sequence(b, T, seed=10)
    stationary = D.make_stationary(samples, bad_frame, [1])

    def run(seq, zero_cuts_of=None):
        model = _model(dev, W)
        state = {"t": 0}

        def hook(_mod, _inp, out):
            if zero_cuts_of is not None and state["t"] == bad_frame:
                out[0][zero_cuts_of, 5:7, 8:11, :] = 0.0
                out[1][zero_cuts_of, 3, 4, :16] = 0.0
            return out
        handle = model.encoder.register_forward_hook(hook)
        snaps = []
        try:
            for t in range(T):
                state["t"] = t
                depth = npy(model.stream_step(_frame(seq[t], cam, dev))["depth"])
                snaps.append((depth, _snapshot(model)))
        finally:
            handle.remove()
        return snaps

    base = run(samples)
    for name, got, bad in (("stationary", run(stationary), 1), ("zero cuts", run(samples, zero_cuts_of=2), 2)):
        others = [s for s in range(b) if s != bad]
        differs = False
        for t in range(T):
            assert_bits_equal(got[t][0][others], base[t][0][others], f"{name}: frame {t} depth of the other streams")
            for l, (x, y) in enumerate(zip(got[t][1], base[t][1])):
                for key in x:
                    assert_bits_equal(x[key][others], y[key][others], f"{name}: frame {t} level {l + 1} {key} of the other streams")
                    differs = differs or not np.array_equal(x[key][bad], y[key][bad], equal_nan=True)
            if t < bad_frame:
                assert_bits_equal(got[t][0], base[t][0], f"{name}: frame {t} precedes the degenerate one")
        assert differs, f"{name}: the degenerate stream equals the healthy one -- the case did not bite"
        if name == "zero cuts":
            assert np.isnan(got[bad_frame][1][0]["prev_f"][bad]).any() and not np.isnan(got[bad_frame][1][0]["prev_f"][others]).any()


def test_metric_rows_of_healthy_samples_ignore_a_degenerate_neighbour(dev):
    """depth_metrics_per_sample: the rows of the healthy samples keep their bits when a neighbour's estimate is NaN / +-Inf / 0."""
    from m4depth_amd import network_ops as nops
    rng = np.random.default_rng(41)
    b, h, w = 4, 64, 96
    gt = torch.from_numpy((1.0 + 79.0 * rng.random([b, h, w, 1])).astype(F)).to(dev)
    est = torch.from_numpy((1.0 + 79.0 * rng.random([b, h, w, 1])).astype(F)).to(dev)
    nt = torch.zeros(b, dtype=torch.uint8, device=dev)
    act = torch.ones(b, dtype=torch.uint8, device=dev)
    rows0, counted0 = nops.depth_metrics_per_sample(gt, est, nt, act)
    rows0, counted0 = npy(rows0).copy(), npy(counted0).copy()
    assert np.isfinite(rows0).all()
    for fill in (np.nan, np.inf, -np.inf, 0.0, "mixed"):
        bad = est.clone()
        if fill == "mixed":
            bad[2, ::3] = float("nan")
            bad[2, 1::3] = float("inf")
            bad[2, 2::3, ::2] = float("-inf")
        else:
            bad[2] = fill
        rows, counted = nops.depth_metrics_per_sample(gt, bad, nt, act)
        assert_bits_equal(npy(rows)[[0, 1, 3]], rows0[[0, 1, 3]], f"estimate of sample 2 = {fill}: rows of the others")
        assert np.array_equal(npy(counted), counted0)


# ================================================================================== f. recovery
@pytest.mark.parametrize("arith", ["f16x2", "bf16x3", "f32"])
def test_a_stream_recovers_after_a_stationary_frame(dev, arith):
    """One stream: reset, healthy, STATIONARY, healthy, healthy, healthy.  On the stationary frame depth_prev_t and every level's
    parallax and depth are finite (R2: the refiner sees log(0) = -inf, its output is NaN, the tail's clamp makes it parallax
    exp(-7) / scale; only "other" is NaN).  From K frames after motion resumes everything, "other" included, is finite again:
    K = 1, measured on the rule-bearing CPU oracle (``degenerate_cases.ORACLE_K``, asserted by
    tests/test_degenerate_oracle.py::test_oracle_model_recovers_one_frame_after_motion_resumes); the GPU recovers no later.
    Eager stream_step, GraphedStream and the sequence call agree bit for bit within the arithmetic."""
    from m4depth_amd import network as net
    T = 6
    W, samples, cam = D.model_sequence(1, T)
    samples = D.make_stationary(samples, D.STATIONARY_FRAME, [0])
    with net.conv_arithmetic(arith):
        eager, graphed, seq = _model(dev, W), _model(dev, W), _model(dev, W)
        runner = net.GraphedStream(graphed, _frame(samples[0], cam, dev))
        finite = []
        for t in range(T):
            fr = _frame(samples[t], cam, dev)
            d_e = npy(eager.stream_step(fr)["depth"])
            d_g = npy(runner(fr)["depth"])
            assert_bits_equal(d_g, d_e, f"[{arith}] frame {t}: GraphedStream vs stream_step")
            snap_e, snap_g = _snapshot(eager), _snapshot(graphed)
            for l, (x, y) in enumerate(zip(snap_g, snap_e)):
                for key in x:
                    assert_bits_equal(x[key], y[key], f"[{arith}] frame {t} level {l + 1}: {key}, GraphedStream vs stream_step")
            assert np.isfinite(d_e).all(), f"[{arith}] frame {t}: depth"
            for l, x in enumerate(snap_e):
                for key in ("depth", "parallax", "depth_prev_t", "prev_f"):
                    assert np.isfinite(x[key]).all(), f"[{arith}] frame {t} level {l + 1}: {key} not finite"
            finite.append(all(np.isfinite(x["other"]).all() for x in snap_e))
        assert all(finite[:D.STATIONARY_FRAME]), f"[{arith}] the healthy frames before the stationary one: {finite}"
        assert not finite[D.STATIONARY_FRAME], f"[{arith}] the stationary frame was meant to put NaN into the refiner"
        k = D.first_recovered(finite)
        print(f"[{arith}] wholly finite per frame: {finite}; recovered {k} frame(s) after motion resumed (oracle: {D.ORACLE_K})")
        assert k is not None and k <= D.ORACLE_K, f"[{arith}] recovered after {k} frames, the oracle after {D.ORACLE_K}"
        assert all(finite[D.STATIONARY_FRAME + k:]), f"[{arith}] not finite from frame {D.STATIONARY_FRAME + k} on: {finite}"
        last_e = _snapshot(eager)
        full = seq([to_dev(samples, dev), to_dev(cam, dev)])
        assert_bits_equal(npy(full["depth"]), d_e, f"[{arith}] sequence call vs stream_step: depth of the last frame")
        for l, (x, y) in enumerate(zip(_snapshot(seq), last_e)):
            for key in x:
                assert_bits_equal(x[key], y[key], f"[{arith}] level {l + 1}: {key}, sequence call vs stream_step")


# ================================================================================== f. the backward (R5, R6; R4 for gradients)
BWD_CASES = pytest.mark.parametrize("case", D.BACKWARD_CASES, ids=D.case_id)
_MASKS = (("NaN", np.isnan), ("+Inf", np.isposinf), ("-Inf", np.isneginf))


def _masks_and_per_sample_bar(got, want, bar, what):
    """The same NaN, +Inf and -Inf entries on 100 % of the tensor, and on the finite ones max |diff| < ``bar`` x the largest
    finite |reference| OF THAT SAMPLE (a degenerate sample piles thousands of terms onto the cells at the origin; a scale
    taken over the batch would hide its neighbour behind it).  A sample whose finite reference is all zero must be all zero."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for name, fn in _MASKS:
        assert np.array_equal(fn(got), fn(want)), \
            f"{what}: {name} mask differs ({int(fn(got).sum())} entries vs {int(fn(want).sum())} in the restatement)"
    errs = []
    for s in range(want.shape[0]):
        fin = np.isfinite(want[s])
        if not fin.any():
            errs.append(float("nan"))
            continue
        errs.append(float(np.abs(got[s][fin] - want[s][fin]).max()) / (float(np.abs(want[s][fin]).max()) + 1e-30))
    print(f"{what}: max |diff| / max |ref| per sample " + " ".join(f"{e:.2e}" for e in errs) + f" (bar {bar})")
    for s, e in enumerate(errs):
        assert not e >= bar, f"{what}: sample {s}: {e:.3e} of its largest finite gradient (bar {bar})"
    return errs


def _dscv_bwd_in_arena(dev, case, rows):
    """m4d_dscv_bwd through the C ABI on the samples ``rows`` of a case, every input, output and scatter target inside a
    sentinel-filled allocation; the guards and the inputs are intact afterwards.  Returns the four gradients."""
    from m4depth_amd._lib import lib, check, stream_ptr
    r, u = D.reference(case), D.backward_upstream(case)
    d = r["inputs"]
    n, h, w, C, k = len(rows), d["h"], d["w"], d["C"], d["k"]
    ncp = 2 * D.DSCV_RANGE + 1
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    a = _Arena(dev, n * h * w * (4 * C + ncp * k + ncp + 4) + 24 * GUARD + 4096)
    t = {name: a.put(np.asarray(v)[rows]) for name, v in (("c1", r["c1"]), ("c2", r["c2"]), ("dpt", r["pd2p"]), ("disp", d["disp"]),
                                                          ("rot", d["rot"]), ("trans", d["trans"]), ("f", d["cam"]["f"]),
                                                          ("c", d["cam"]["c"]), ("g_cv", u["g_cv"]), ("g_pd", u["g_prev_disp"]))}
    g_c1, g_c2 = a.out((n, h, w, C)), a.out((n, h, w, C))
    g_disp, g_dpt = a.out((n, h, w, 1)), a.out((n, h, w, 1))
    a.snapshot()
    check(lib.m4d_dscv_bwd(P(t["c1"]), P(t["c2"]), P(t["dpt"]), P(t["disp"]), P(t["rot"]), 4, P(t["trans"]), P(t["f"]), P(t["c"]),
                           n, h, w, C, D.DSCV_RANGE, k, P(t["g_cv"]), ncp * k, P(t["g_pd"]), P(g_c1), P(g_c2), P(g_disp), P(g_dpt),
                           stream_ptr()), "m4d_dscv_bwd")
    torch.cuda.synchronize()
    a.assert_only_outputs_changed(f"{D.case_id(case)} m4d_dscv_bwd on samples {rows}")
    return {"dscv_g_c1": npy(g_c1), "dscv_g_c2": npy(g_c2), "dscv_g_disp": npy(g_disp), "dscv_g_disp_prev_t": npy(g_dpt)}


DSCV_BWD_BAR = 4e-3      # tests/test_gpu_grad.py: float16 multiplies (relative step 1e-3) and an atomic scatter


def dscv_backward_on_a_degenerate_case(M, dev, case):
    """The comparison of ``test_dscv_backward_on_degenerate_frames``; also run by the child process with the LDS window off."""
    r, u, ref = D.reference(case), D.backward_upstream(case), D.backward_reference(case)
    d = r["inputs"]
    k = d["k"]
    what = f"dscv backward {D.case_id(case)}"
    rot, trans, cam = to_dev(d["rot"], dev), to_dev(d["trans"], dev), to_dev(d["cam"], dev)
    leaves = [to_dev(np.array(v), dev).requires_grad_(True) for v in (r["c1"], r["c2"], r["pd2p"], d["disp"])]
    cv, pd = M.get_parallax_sweeping_cv(*leaves, rot, trans, cam, D.DSCV_RANGE, nbre_cuts=k)
    ((cv * to_dev(u["g_cv"], dev)).sum() + (pd * to_dev(u["g_prev_disp"], dev)).sum()).backward()
    names = ("dscv_g_c1", "dscv_g_c2", "dscv_g_disp_prev_t", "dscv_g_disp")
    op = {n: npy(t.grad) for n, t in zip(names, leaves)}
    errs = {n: _masks_and_per_sample_bar(op[n], ref[n], DSCV_BWD_BAR, f"{what} {n}") for n in names}
    # the C ABI inside guarded memory: batch of two, then every sample alone (R4)
    both = _dscv_bwd_in_arena(dev, case, [0, 1])
    for n in ("dscv_g_c1", "dscv_g_disp"):                 # owned by the pixel: deterministic
        assert_bits_equal(both[n], op[n], f"{what} {n}: C ABI vs the differentiable op")
    for n in ("dscv_g_c2", "dscv_g_disp_prev_t"):          # atomic scatters
        _masks_and_per_sample_bar(both[n], ref[n], DSCV_BWD_BAR, f"{what} {n} (C ABI)")
    for s in range(D.B):
        alone = _dscv_bwd_in_arena(dev, case, [s])
        for n in ("dscv_g_c1", "dscv_g_disp"):
            assert_bits_equal(alone[n][0], both[n][s], f"{what} {n}: sample {s} alone vs beside its neighbour (R4)")
        for n in ("dscv_g_c2", "dscv_g_disp_prev_t"):
            _masks_and_per_sample_bar(alone[n], ref[n][s:s + 1], DSCV_BWD_BAR, f"{what} {n}: sample {s} alone")
    return errs


@BWD_CASES
def test_dscv_backward_on_degenerate_frames(M, dev, case):
    """m4d_dscv_bwd through ``M.get_parallax_sweeping_cv`` on every case of the table, against autodiff of the rule-bearing
    restatement (``D.backward_reference``): equal NaN / +Inf / -Inf masks on 100 % of g_c1, g_c2, g_disp_prev_t and g_disp,
    4e-3 of the sample's largest finite gradient on the rest; the same call through the C ABI inside sentinel-guarded memory
    (inputs, outputs and both scatter targets); every sample alone as a batch of one gives the bits of its rows in the batch
    for g_c1 and g_disp (R4; the atomic targets keep the per-sample bar).

    Blocks of dscv_bwd_kernel per case, both samples: [with an LDS window, scattering straight to memory], and of those the
    blocks holding a pixel with a NaN or infinite query:

      stationary-13x21   [24, 0] / [12, 0]    stationary-37x45  [60, 0] / [30, 0]    stationary-6x20   [57, 3] / [30, 0]
      epipole-13x21      [24, 0] / [2, 0]     epipole-37x45     [58, 2] / [0, 2]     far_query-6x20    [60, 0] / [30, 0]
      zero_cut-13x21     [24, 0] / [0, 0]     far_query-37x45   [60, 0] / [30, 0]    zero_cut-6x20     [57, 3] / [0, 0]
      far_query-13x21    [24, 0] / [12, 0]    stationary-21x19  [110, 0] / [55, 0]   stationary-20x44  [36, 0] / [18, 0]
      prev_d2para-13x21  [24, 0] / [0, 0]     epipole-21x19     [107, 3] / [0, 2]    far_query-20x44   [36, 0] / [18, 0]
      (12x20: [18, 0], 9 of them with NaN / Inf queries under stationary and far_query)   zero_cut-21x19    [109, 1] / [0, 0]

    A stationary sample's NaN queries all read cell 0 (R1), so its blocks keep a 2 x 2 window at the origin.  The epipole block
    of 37x45 (8 x 8 pixels, C = 16) spans from cell (0, 0) -- its NaN query -- past the middle of the map, where its healthy
    queries point: over 12288 floats, so it scatters straight to memory; likewise the 2 x 4 block of 21x19 at C = 96.  (The
    far-query samples do NOT overflow the window: sideways motion clamps one axis only, and sample 1's +-Inf queries all land
    in one corner.  Their direct path runs in the child process of the test below.)

    clamped_corner (backward only, tests/degenerate_cases.py) is the case that tells R5's select from a product with a
    0/1 mask: with ``pass_x ? dax : 0.f`` written as ``dax * (pass_x ? 1.f : 0.f)`` in dscv_bwd_kernel its two geometries fail
    here on the NaN mask of g_disp (83 entries against 65, 84 against 71) and every other case passes -- no case of the forward
    table has a query clamped on BOTH axes at a non-finite cell, and with one axis inside the other axis's alpha gradient is
    non-finite too.  Both of its geometries keep every block's window in LDS ([24, 0] and [60, 0]).

    Measured errors: the module docstring."""
    import test_gpu_grad as GG
    r = D.reference(case)
    d = r["inputs"]
    with torch.no_grad():
        idx = npy(M.get_parallax_sweeping_cv(to_dev(np.array(r["c1"]), dev), to_dev(np.array(r["c2"]), dev),
                                             to_dev(np.array(r["pd2p"]), dev), to_dev(d["disp"], dev), to_dev(d["rot"], dev),
                                             to_dev(d["trans"], dev), to_dev(d["cam"], dev), D.DSCV_RANGE, nbre_cuts=d["k"],
                                             return_index=True)[2])
    assert np.array_equal(idx, r["idx"]), "the forward's index grid"
    private, direct = GG.dscv_window_mix(idx, d["C"])
    priv, bh, bw = D.dscv_bwd_blocks(idx, d["C"])
    assert (int(priv.sum()), int((~priv).sum())) == (private, direct)
    odd = D.blocks_with(~np.isfinite(r["queries"]).all(axis=(3, 4)), bh, bw)
    print(f"dscv backward {D.case_id(case)}: {private} blocks with an LDS window, {direct} scattering straight to memory; "
          f"with a NaN / Inf query: {int((priv & odd).sum())} / {int((~priv & odd).sum())}")
    dscv_backward_on_a_degenerate_case(M, dev, case)


def test_dscv_backward_paths_over_the_case_list():
    """Both scatter paths of dscv_bwd_kernel meet a NaN or infinite query somewhere in the table: the LDS window (a
    stationary sample: every block, at the origin) and the direct scatter (the epipole block of 37x45 and of 21x19).  From the
    oracle's index grid, which the test above holds the device's to."""
    seen = {"window": [], "direct": []}
    for case in D.CASES:
        r = D.reference(case)
        priv, bh, bw = D.dscv_bwd_blocks(r["idx"], r["inputs"]["C"])
        odd = D.blocks_with(~np.isfinite(r["queries"]).all(axis=(3, 4)), bh, bw)
        if (priv & odd).any():
            seen["window"].append(D.case_id(case))
        if (~priv & odd).any():
            seen["direct"].append(D.case_id(case))
        if case.kind == "stationary":
            y0x0 = r["idx"][0]
            assert (y0x0 == 0).all() and priv[0].all(), f"{case}: private windows at the origin"
    print(seen)
    assert "stationary-13x21" in seen["window"] and "far_query-37x45" in seen["window"]
    assert "epipole-37x45" in seen["direct"] and "epipole-21x19" in seen["direct"]


def test_dscv_backward_direct_scatter_on_degenerate_frames():
    """stationary-13x21 and far_query-37x45 once more with the LDS window switched off (M4D_DSCV_BWD_WINDOW_KB=0: every block
    scatters straight to memory, the stationary sample's thousands of adds onto the four cells at the origin included).  The
    switch is read once per process, hence a fresh child; it gets its own time limit and is started once."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import torch, m4depth_amd as M, degenerate_cases as D, test_gpu_degenerate as T\n"
            "for c in (D.Case('stationary', '13x21'), D.Case('far_query', '37x45')):\n"
            "    T.dscv_backward_on_a_degenerate_case(M, torch.device('cuda:0'), c)\n"
            "print('both cases done')\n")
    env = dict(os.environ, M4D_DSCV_BWD_WINDOW_KB="0")
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(root, "tests"), root] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    res = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, timeout=300, capture_output=True, text=True)
    print(res.stdout)
    assert res.returncode == 0, f"child exited with status {res.returncode}:\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
    assert "both cases done" in res.stdout, res.stdout


ZERO_CUT_CASES = [c for c in D.CASES if c.kind == "zero_cut"]


@pytest.mark.parametrize("case", ZERO_CUT_CASES, ids=D.case_id)
def test_sncv_and_normalize_backward_on_zero_cuts(M, dev, case):
    """m4d_sncv_bwd (both inputs one map, and two maps) on NaN features, and m4d_normalize_cuts_bwd on the RAW features with
    their planted all-zero cuts (the 0 / 0 arises in the kernel: dot / (ss * n) with ss = 0): masks equal on 100 %, 1e-5 of
    the sample's largest finite gradient on the rest (the bars of tests/test_gpu_grad.py), the C ABI inside guarded memory,
    and every sample alone bit for bit (all three gradients are gathers: deterministic)."""
    from m4depth_amd import training as TR
    from m4depth_amd._lib import lib, check, stream_ptr
    r, u, ref = D.reference(case), D.backward_upstream(case), D.backward_reference(case)
    d = r["inputs"]
    h, w, C, k = d["h"], d["w"], d["C"], d["k"]
    mo2 = (2 * D.SNCV_RANGE + 1) ** 2
    what = f"{D.case_id(case)}"

    def run(rows):
        out = {}
        g = to_dev(u["g_sncv"][rows], dev)
        a = to_dev(np.array(r["c1"])[rows], dev).requires_grad_(True)
        (M.cost_volume(a, a, D.SNCV_RANGE, nbre_cuts=k) * g).sum().backward()
        out["sncv_auto_g_c1"] = npy(a.grad)
        a, b_ = to_dev(np.array(r["c1"])[rows], dev).requires_grad_(True), to_dev(np.array(r["c2"])[rows], dev).requires_grad_(True)
        (M.cost_volume(a, b_, D.SNCV_RANGE, nbre_cuts=k) * g).sum().backward()
        out["sncv_g_c1"], out["sncv_g_c2"] = npy(a.grad), npy(b_.grad)
        f1 = to_dev(d["f1"][rows], dev).requires_grad_(True)
        (TR._normalize_cuts(f1, k) * to_dev(u["g_feat"][rows], dev)).sum().backward()
        out["norm_g_f1"] = npy(f1.grad)
        return out

    both = run([0, 1])
    for n in both:
        _masks_and_per_sample_bar(both[n], ref[n], 1e-5, f"{what} {n}")
    for s in range(D.B):
        alone = run([s])
        for n in both:
            assert_bits_equal(alone[n][0], both[n][s], f"{what} {n}: sample {s} alone vs beside its neighbour (R4)")
    # the C ABI inside guarded memory
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    n_px = D.B * h * w
    a = _Arena(dev, n_px * (7 * C + 2 * mo2 * k) + 24 * GUARD + 4096)
    t = {name: a.put(v) for name, v in (("c1", r["c1"]), ("c2", r["c2"]), ("out", r["sncv"]), ("g", u["g_sncv"]), ("f1", d["f1"]),
                                        ("g_feat", u["g_feat"]))}
    g1, g2, gx = a.out((D.B, h, w, C)), a.out((D.B, h, w, C)), a.out((D.B, h, w, C))
    a.snapshot()
    check(lib.m4d_sncv_bwd(P(t["c1"]), P(t["c2"]), P(t["out"]), mo2 * k, P(t["g"]), mo2 * k, D.B, h, w, C, D.SNCV_RANGE, 1, k, 0.1,
                           P(g1), P(g2), stream_ptr()), "m4d_sncv_bwd")
    check(lib.m4d_normalize_cuts_bwd(P(t["f1"]), P(t["g_feat"]), D.B, h, w, C, k, P(gx), stream_ptr()), "m4d_normalize_cuts_bwd")
    torch.cuda.synchronize()
    a.assert_only_outputs_changed(f"{what} m4d_sncv_bwd / m4d_normalize_cuts_bwd")
    assert_bits_equal(npy(g1), both["sncv_g_c1"], "m4d_sncv_bwd g_c1: C ABI vs the differentiable op")
    assert_bits_equal(npy(g2), both["sncv_g_c2"], "m4d_sncv_bwd g_c2")
    assert_bits_equal(npy(gx), both["norm_g_f1"], "m4d_normalize_cuts_bwd")


LEVEL_POST_PLANTS = [((0, 0), np.nan), ((3, 7), np.inf), ((5, 2), -np.inf), ((10, 13), 9.0), ((10, 14), -7.5), ((12, 20), np.nan)]


def test_level_post_backward_with_planted_refiner_outputs(M, dev):
    """m4d_level_post_bwd at 2 x 13 x 21 with per-sample cameras, sample 0 stationary (s = 0 on every pixel) beside a moving
    one, and NaN, +Inf, -Inf, 9 and -7.5 planted into the refiner's parallax channel of both samples beside healthy values:
    g_ro[..., 0] is EXACTLY 0 at the planted pixels (R5: the clamp's gradient is a select, whatever arrives), everything is
    finite, the rest within 1e-5 of the sample's largest gradient of autodiff of the restatement; guards intact; each sample
    alone gives the same bits (R4)."""
    from m4depth_amd._lib import lib, check, stream_ptr
    from helpers import cameras_np
    rng = np.random.default_rng(501)
    b, h, w, scale = 2, 13, 21, 0.5
    ro = rng.normal(0, 3.0, size=[b, h, w, 5]).astype(F)
    for (j, i), v in LEVEL_POST_PLANTS:
        ro[:, j, i, 0] = v
    rot, trans = motion_np(rng, b, t_scale=(3.0, 3.0, 1.0))
    trans[0] = 0.0
    cam = cameras_np(b, h, w)
    gs = [rng.normal(size=[b, h, w, n]).astype(F) for n in (1, 1, 4)]
    tro = torch.from_numpy(ro).requires_grad_(True)
    para = torch.exp(OT._clip(tro[..., :1], -7., 7.)) / scale
    depth = OT.parallax2depth(para, rot, trans, cam)
    ((para * torch.from_numpy(gs[0])).sum() + (depth * torch.from_numpy(gs[1])).sum() + (tro[..., 1:] * torch.from_numpy(gs[2])).sum()).backward()
    want = tro.grad.numpy()
    assert np.isfinite(want).all() and np.isfinite(depth.detach().numpy()).all()
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def run(rows):
        n = len(rows)
        a = _Arena(dev, n * h * w * 16 + 16 * GUARD + 4096)
        t = {name: a.put(v[rows]) for name, v in (("ro", ro), ("g0", gs[0]), ("g1", gs[1]), ("g2", gs[2]), ("rot", rot), ("trans", trans),
                                                  ("f", cam["f"]), ("c", cam["c"]))}
        g_ro = a.out((n, h, w, 5))
        a.snapshot()
        check(lib.m4d_level_post_bwd(P(t["ro"]), P(t["g0"]), P(t["g1"]), P(t["g2"]), P(t["rot"]), 4, P(t["trans"]), P(t["f"]), P(t["c"]),
                                     n, h, w, scale, P(g_ro), stream_ptr()), "m4d_level_post_bwd")
        torch.cuda.synchronize()
        a.assert_only_outputs_changed(f"m4d_level_post_bwd on samples {rows}")
        return npy(g_ro)

    got = run([0, 1])
    _masks_and_per_sample_bar(got, want, 1e-5, "level tail backward, planted refiner outputs")
    for (j, i), v in LEVEL_POST_PLANTS:
        assert_bits_equal(got[:, j, i, 0], np.zeros(b, F), f"g_ro[..., 0] at the planted {v}")
        assert (want[:, j, i, 0] == 0).all()
    assert np.array_equal(got[..., 0] == 0, ~(np.abs(ro[..., 0]) <= 7)), "zero exactly where the refiner output is outside [-7, 7] or NaN"
    for s in range(b):
        assert_bits_equal(run([s])[0], got[s], f"level tail backward: sample {s} alone vs beside its neighbour (R4)")


LOSS_PLANTS = [((0, 0), np.nan), ((1, 3), np.inf), ((2, 5), -np.inf), ((3, 1), 0.0), ((4, 4), 0.005), ((5, 8), 250.0), ((5, 0), -3.0)]


def test_loss_level_kernels_with_planted_predictions(M, dev):
    """m4d_loss_level_fwd / _bwd (both ground-truth kinds) at 2 x 6 x 9 against a 24 x 36 ground truth, with a prediction
    planted at each of NaN, +Inf, -Inf, 0, 0.005 (below 0.01), 250 (above 200) and -3 in sample 0 beside healthy pixels:
    log(clip(d, 0.01, 200)) drops the NaN to 0.01 (R2), so the loss is finite and within 2e-6 of the float64 restatement;
    g_pred is 0 at the planted pixels (R5) and within 1e-5 of the sample's largest gradient elsewhere; guards intact; with
    sample 0's plants replaced by healthy values sample 1's gradient keeps its bits (R4)."""
    from m4depth_amd._lib import lib, check, stream_ptr
    rng = np.random.default_rng(502)
    b, h, w, up = 2, 6, 9, 4
    gt = rng.uniform(1, 80, size=[b, up * h, up * w, 1]).astype(F)
    healthy = rng.uniform(0.5, 150, size=[b, h, w, 1]).astype(F)
    pred = healthy.copy()
    for (j, i), v in LOSS_PLANTS:
        pred[0, j, i, 0] = v
    n_ws = int(lib.m4d_loss_workspace_floats())
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def run(p, gtk, velodyne):
        a = _Arena(dev, gtk.size + 2 * p.size + n_ws + 16 * GUARD + 4096)
        tp, tg, one = a.put(p), a.put(gtk), a.put(np.ones(1, F))
        ws, out2, g_pred = a.out((n_ws,)), a.out((2,)), a.out(p.shape)
        a.snapshot()
        check(lib.m4d_loss_level_fwd(P(tp), P(tg), b, h, w, up * h, up * w, velodyne, P(ws), P(out2), stream_ptr()), "m4d_loss_level_fwd")
        check(lib.m4d_loss_level_bwd(P(tp), P(tg), P(out2), P(one), b, h, w, up * h, up * w, velodyne, P(g_pred), stream_ptr()),
              "m4d_loss_level_bwd")
        torch.cuda.synchronize()
        a.assert_only_outputs_changed(f"m4d_loss_level_fwd / _bwd (velodyne={velodyne})")
        return float(out2[0]), npy(g_pred)

    for velodyne, kind in ((0, "map"), (1, "velodyne")):
        gtk = (gt * (rng.random(gt.shape) > 0.8)).astype(F) if velodyne else gt
        tp = torch.from_numpy(pred).double().requires_grad_(True)
        ref = OT.m4depth_loss([None, {"depth": torch.from_numpy(gtk).double()}], [None, [{"depth": tp}]], kind)
        ref.backward()
        # the product's weighting of one level (0.64 / 2^(i - 1), i = 0) is applied by its caller: the kernel gives the plain term
        ref_v, want = ref.item() / 1.28, tp.grad.numpy() / 1.28
        got_v, got = run(pred, gtk, velodyne)
        print(f"loss with planted predictions ({kind}): {got_v!r} vs {ref_v!r}, relative {abs(got_v - ref_v) / abs(ref_v):.3e}")
        assert np.isfinite(got_v) and abs(got_v - ref_v) <= 2e-6 * abs(ref_v), (kind, got_v, ref_v)
        _masks_and_per_sample_bar(got, want, 1e-5, f"loss backward with planted predictions ({kind})")
        for (j, i), v in LOSS_PLANTS:
            assert got[0, j, i, 0] == 0.0 and want[0, j, i, 0] == 0.0, f"g_pred at the planted {v}"
        _, healed = run(healthy, gtk, velodyne)
        assert_bits_equal(healed[1], got[1], f"loss backward ({kind}): sample 1 with sample 0's plants healed (R4)")
        assert (healed[0] != 0).sum() > (got[0] != 0).sum()


def test_backproject_backward_with_planted_coordinates(M, dev):
    """m4d_backproject_bwd at 2 x 13 x 21 (3 hypotheses, 4 channels) with NaN, +Inf, -Inf, negative and beyond-the-border
    coordinates planted beside healthy ones (and one exactly on the last column / row, which is inside): the planted items add
    nothing to ``input_grad`` (equal to the run with their upstream gradient zeroed and their coordinates healed, up to the
    atomics' order; 1e-5 of the sample's largest entry against the oracle), ``coords_grad`` is exactly 0 there and the
    oracle's bits elsewhere; guards intact."""
    from m4depth_amd._lib import lib, check, stream_ptr
    rng = np.random.default_rng(503)
    b, h, w, s, f, c = 2, 13, 21, 3, 1, 4
    inp = rng.standard_normal([b, h, w, f, c]).astype(F)
    co = (rng.random([b, h, w, s, f, 2]) * np.array([w - 1.0, h - 1.0])).astype(F)
    grad = rng.standard_normal([b, h, w, s, f, c]).astype(F)
    nan, inf = np.nan, np.inf
    plants = [(nan, 3.0), (4.0, nan), (nan, nan), (inf, 2.0), (1.0, -inf), (-0.25, 5.0), (6.0, -1e-7), (w - 0.5, 3.0), (2.0, float(h)),
              (3e38, 1.0), (-3e38, -3e38)]
    where = [(n % b, (5 * n + 1) % h, (7 * n + 2) % w, n % s, 0) for n in range(len(plants))]
    healed = co.copy()
    zeroed = grad.copy()
    for at, xy in zip(where, plants):
        co[at] = xy
        zeroed[at] = 0.0
    co[1, 0, 0, 0, 0] = (w - 1.0, h - 1.0)                 # the far corner itself is inside
    healed[1, 0, 0, 0, 0] = co[1, 0, 0, 0, 0]
    dims = (ctypes.c_int * 6)(b, h, w, s, f, c)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def run(coords, g):
        a = _Arena(dev, inp.size * 2 + coords.size * 2 + g.size + 16 * GUARD + 4096)
        ti, tc, tg = a.put(inp), a.put(coords), a.put(g)
        gi, gc = a.out(inp.shape), a.out(coords.shape)
        a.snapshot()
        check(lib.m4d_backproject_bwd(P(tg), P(ti), P(tc), dims, P(gi), P(gc), stream_ptr()), "m4d_backproject_bwd")
        torch.cuda.synchronize()
        a.assert_only_outputs_changed("m4d_backproject_bwd")
        return npy(gi), npy(gc)

    gi, gc = run(co, grad)
    with np.errstate(invalid="ignore"):
        want_i, want_c = O.back_project_grad(inp, co, grad)
    assert np.isfinite(gi).all() and np.isfinite(gc).all()
    assert_bits_equal(gc, want_c, "coords_grad")
    for at in where:
        assert_bits_equal(gc[at], np.zeros(2, F), f"coords_grad at the planted {co[at]}")
    _masks_and_per_sample_bar(gi, want_i, 1e-5, "backproject input_grad, planted coordinates")
    gi_h, _ = run(healed, zeroed)
    _masks_and_per_sample_bar(gi, gi_h, 1e-5, "backproject input_grad vs the run without the planted items")


def test_conv_backward_with_non_finite_activations(M, dev):
    """One layer of the training graph (training._ConvBiasAct, 2 x 12 x 20, 32 -> 32: m4d_bias_act_bwd, m4d_conv3x3_wgrad and
    the data-gradient convolution on the rotated weights) with a NaN and a +Inf planted in the activations and an exact 0 in
    the incoming gradient at those two pixels -- what a stationary sample hands the refiner's layers.  R6: 0 * NaN = NaN, so
    the weight gradient's NaN / +Inf / -Inf masks are those of float64 autodiff (the whole input channel of the NaN; the +Inf
    channel is +-Inf by the sign of the neighbouring gradient and NaN on the centre tap), 2e-5 of the largest finite entry on
    the rest; the bias and the data gradient are finite and within 2e-5 (the bars of tests/test_gpu_grad.py).  The slope of
    the activation is taken from the device's output, as there.  m4d_conv3x3_wgrad once more through the C ABI inside guarded
    memory, the same bits."""
    import torch.nn.functional as TF
    from m4depth_amd import training as TR
    from m4depth_amd._lib import lib, check, stream_ptr
    rng = np.random.default_rng(504)
    b, h, w, cin, cout = 2, 12, 20, 32, 32
    x = rng.standard_normal([b, h, w, cin]).astype(F)
    k = (rng.standard_normal([cout, cin, 3, 3]) * np.sqrt(2.0 / (9 * cin))).astype(F)
    bias = (0.1 * rng.standard_normal([cout])).astype(F)
    gout = rng.standard_normal([b, h, w, cout]).astype(F)
    x[0, 3, 5, 7], x[1, 8, 11, 20] = np.nan, np.inf
    gout[0, 3, 5, :], gout[1, 8, 11, :] = 0.0, 0.0
    xd = to_dev(x, dev).requires_grad_(True)
    wd = torch.nn.Parameter(to_dev(k, dev).contiguous(memory_format=torch.channels_last))
    bd = torch.nn.Parameter(to_dev(bias, dev))
    yd = TR._ConvBiasAct.apply(xd, wd, bd, 1, 0.1, {})
    (yd * to_dev(gout, dev)).sum().backward()
    positive = (yd.detach() > 0).cpu()
    xr = torch.from_numpy(x).double().requires_grad_(True)
    kr = torch.from_numpy(k).double().requires_grad_(True)
    br = torch.from_numpy(bias).double().requires_grad_(True)
    y_lin = TF.conv2d(TF.pad(xr.permute(0, 3, 1, 2), (1, 1, 1, 1)), kr, br, 1, 0).permute(0, 2, 3, 1)
    fin = torch.isfinite(y_lin.detach())
    print(f"outputs: {int((~fin).sum())} non-finite in float64, {int((~torch.isfinite(yd.detach())).sum())} on the device")
    flipped = (positive != (y_lin.detach() > 0)) & fin
    assert bool((y_lin.detach().abs()[flipped] <= 2e-5 * float(y_lin.detach()[fin].abs().max())).all())
    slope = torch.where(positive, torch.tensor(1.0, dtype=torch.float64), torch.tensor(0.1, dtype=torch.float64))
    g_eff = slope * torch.from_numpy(gout).double()
    # d/dk, d/dx, d/dbias of sum(y_lin * g_eff) with g_eff held constant
    gk, gx, gb = torch.autograd.grad(y_lin, (kr, xr, br), grad_outputs=g_eff)
    want_w = gk.numpy()
    assert np.isnan(want_w[:, 7]).all() and np.isnan(want_w[:, 20, 1, 1]).all() and np.isinf(want_w[:, 20]).any()
    assert np.isfinite(np.delete(want_w, [7, 20], axis=1)).all()
    _masks_and_per_sample_bar(npy(wd.grad)[None], want_w[None], 2e-5, "weight gradient with NaN / Inf activations")
    assert np.isfinite(npy(bd.grad)).all() and np.isfinite(npy(xd.grad)).all()
    _masks_and_per_sample_bar(npy(bd.grad)[None], gb.numpy()[None], 2e-5, "bias gradient")
    _masks_and_per_sample_bar(npy(xd.grad), gx.numpy(), 2e-5, "data gradient")
    # the weight-gradient kernel inside guarded memory
    gp = (gout * np.where(positive.numpy(), F(1.0), F(0.1))).astype(F)
    n_ws = int(lib.m4d_conv3x3_wgrad_workspace_floats(b, h, w, cin, cout, 1))
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    a = _Arena(dev, x.size + gp.size + n_ws + 9 * cin * cout + 16 * GUARD + 4096)
    tx, tg = a.put(x), a.put(gp)
    ws, dw = a.out((max(n_ws, 1),)), a.out((cout, 3, 3, cin))
    a.snapshot()
    check(lib.m4d_conv3x3_wgrad(P(tx), P(tg), b, h, w, cin, cout, 1, P(ws), n_ws, P(dw), stream_ptr()), "m4d_conv3x3_wgrad")
    torch.cuda.synchronize()
    changed = a.buf != a._before                           # the workspace may stay untouched on a small layer
    for lo, n in a.outputs:
        changed[lo:lo + n] = False
    assert int(changed.sum()) == 0, "m4d_conv3x3_wgrad wrote outside its workspace and output"
    assert_bits_equal(npy(dw).transpose(0, 3, 1, 2), npy(wd.grad), "m4d_conv3x3_wgrad: C ABI vs the autograd node")


def _photo_stationary(dev, automask):
    import photometric_ref as R
    from m4depth_amd import network_ops as nops
    y = R.stationary_yardstick()
    d = {k: to_dev(np.asarray(v), dev) for k, v in y["case"].items() if k != "name"}
    warped, dwarp, valid = nops.photo_warp_fwd(d["depth"], d["rot"], d["trans"], d["f"], d["c"], d["prev"])
    out4, mask = nops.photo_loss_fwd(d["depth"], warped, valid, d["cur"], d["prev"], 1e-3, automask)
    return y, d, warped, dwarp, valid, out4, mask


def test_photometric_loss_on_a_stationary_sample(dev):
    """photo_warp_fwd / photo_loss_fwd / m4d_photo_loss_bwd on photometric_ref.stationary_case (13 x 21, sample 0 stationary
    under an identity rotation beside a moving sample), auto-mask off, against the float64 restatement exactly as
    tests/test_gpu_photometric.py does on the healthy cases: the same mask and N, term / photo / smooth within 4 x the float32
    restatement's own error, g_depth (C ABI, fed the reference's mask and totals) within 4 x its error of max |g| on the
    well-conditioned pixels -- all of sample 0, whose cell border carries no gradient (stationary_well).  warped and valid
    carry the float32 restatement's bits: sample 0's warp is ``prev``."""
    import photometric_ref as R
    from m4depth_amd._lib import lib, dptr, stream_ptr
    y, d, warped, dwarp, valid, out4, mask = _photo_stationary(dev, False)
    r64, g64, well = y["ref"]
    r32 = y["r32"]
    assert np.array_equal(npy(valid)[..., 0].astype(bool), r32["valid"].numpy()) and npy(valid)[0].all()
    assert_bits_equal(npy(warped), r32["warped"].detach().numpy(), "warped vs the float32 restatement")
    assert_bits_equal(npy(warped)[0, :-1, :-1], npy(d["prev"])[0, :-1, :-1], "the stationary sample's warp is the previous image")
    assert np.isfinite(npy(dwarp)).all()
    assert np.array_equal(npy(mask)[..., 0].astype(bool), r64["mask"].numpy()), "mask differs from the float64 restatement's"
    o = npy(out4).astype(np.float64)
    errs = {k: abs(o[i] - r64[k].item()) / abs(r64[k].item()) for i, k in enumerate(("term", "photo", "smooth"))}
    print("stationary, automask off: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items())
          + f" (float32 restatement {y['loss']:.2e}, bar {4 * y['loss']:.2e}); N {o[3]:.0f}")
    assert o[3] == r64["n"].item() and 0 < o[3] < mask.numel()
    for k, e in errs.items():
        assert e <= 4 * y["loss"], (k, e)
    rmask = to_dev(r64["mask"].numpy().astype(np.uint8)[..., None], dev)
    rout4 = to_dev(np.array([r64[k].item() for k in ("term", "photo", "smooth", "n")], np.float32), dev)
    b, h, w, _ = d["depth"].shape
    g = torch.full_like(d["depth"], float("nan"))
    rc = lib.m4d_photo_loss_bwd(dptr(d["depth"]), dptr(warped), dptr(dwarp), dptr(d["cur"]), dptr(rmask, "mask", torch.uint8),
                                dptr(rout4), dptr(to_dev(np.array([1.0], np.float32), dev)), b, h, w, 1e-3, dptr(g), stream_ptr())
    assert rc == 0
    g, g64 = npy(g)[..., 0].astype(np.float64), g64.numpy()[..., 0]
    assert np.isfinite(g).all()
    err = np.abs(g - g64)[well.numpy()].max() / np.abs(g64).max()
    per = [np.abs(g - g64)[s][well.numpy()[s]].max() / np.abs(g64[s]).max() for s in range(b)]
    print(f"stationary, automask off: g_depth error {err:.3e} of max |g| (float32 restatement {y['grad']:.3e}, bar {4 * y['grad']:.3e}); "
          f"per sample, of its own max |g|: {per[0]:.3e} {per[1]:.3e}")
    assert well.double().mean().item() >= 0.99 and err <= 4 * y["grad"]


def test_photometric_automask_on_a_stationary_sample_stays_finite(dev):
    """The same case with the auto-mask on.  Sample 0's mask asks whether pe(warped, cur) < pe(prev, cur) where warped IS prev
    (to an ulp in the last row / column): the answer is last-bit noise of two evaluations of one number -- the float32 and
    float64 restatements themselves disagree (N = 61 against 58) -- so no mask can be demanded.  What holds whatever the noise
    does: every output and the gradient are finite, and the auto-mask only removes pixels (N <= N without it, mask a subset)."""
    from m4depth_amd import network_ops as nops
    _, d, warped, dwarp, valid, out4, mask = _photo_stationary(dev, True)
    _, _, _, _, _, out4_off, mask_off = _photo_stationary(dev, False)
    g = nops.photo_loss_bwd(d["depth"], warped, dwarp, d["cur"], mask, out4, torch.ones(1, device=dev), 1e-3)
    print(f"stationary, automask on: N {float(out4[3]):.0f} (off: {float(out4_off[3]):.0f}), "
          f"{int(mask[0].sum())} pixels of the stationary sample kept")
    assert np.isfinite(npy(out4)).all() and np.isfinite(npy(g)).all()
    assert float(out4[3]) <= float(out4_off[3]) and float(out4[3]) == float(mask.sum())
    assert bool((mask <= mask_off).all())


def _model_batch(dev):
    weights, samples, cam = D.model_sequence(2, D.STATIONARY_FRAME + 1)
    samples = D.make_stationary(samples, D.STATIONARY_FRAME, [0])
    data = {k: np.stack([s[k] for s in samples], axis=1) for k in ("RGB_im", "depth", "rot", "trans", "new_traj")}
    data["camera"] = cam
    return weights, data


def _trainable_model(dev, weights):
    import m4depth_amd as M
    from m4depth_amd import training as TR
    model = M.M4Depth(nbre_levels=D.MODEL_LEVELS, is_training=True)
    model.load_numpy_weights(weights, dev)
    return TR.set_trainable(model), TR


def _gradient_flags(model):
    """{parameter name of the oracle: whether its gradient holds a non-finite value}."""
    import test_gpu_train as GT
    return {name: not bool(torch.isfinite(g).all()) for name, g in GT._named_grads(model, D.MODEL_LEVELS).items()}


def test_train_step_on_a_stationary_frame_eager_and_graph(dev):
    """One training step (3 levels, 64 x 96, batch 2, three frames) whose last frame is stationary for sample 0
    (``D.model_sequence`` / ``D.make_stationary``), eagerly through ``train_step`` and once through ``GraphedTrainStep``.
    The loss is finite (R2) and within 1e-4 of ``OT.train_loss`` on the same batch (the bar of
    test_gpu_train.py::test_loss_and_gradients_match_oracle).  The backward then meets NaN refiner activations with a zero
    incoming gradient (R5 selects it) and R6 makes 0 * NaN = NaN of it: the parameter tensors holding a non-finite gradient
    are those of the restatement, one flag per tensor -- every refiner kernel of every level, no bias, nothing of the encoder
    (a Winograd kernel spreads a NaN over its tile, a direct one over its 3 x 3 window: finer masks are not comparable).
    Eager and graph agree on the flags; the graph's warm-up step runs on the healthy batch at a learning rate of 1e-9."""
    weights, data = _model_batch(dev)
    tw = {k: torch.from_numpy(v).requires_grad_(True) for k, v in weights.items()}
    tdata = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) and v.dtype != np.bool_ else v) for k, v in data.items()}
    ref_loss, _ = OT.train_loss(tw, tdata, D.MODEL_LEVELS)
    ref_loss.backward()
    want = {k: not bool(torch.isfinite(v.grad).all()) for k, v in tw.items()}
    assert np.isfinite(ref_loss.item()) and any(want.values()) and not all(want.values())
    ddata = to_dev(data, dev)
    model, TR = _trainable_model(dev, weights)
    model.compile(optimizer=torch.optim.Adam(model.parameters(), lr=1e-9, eps=1e-7))
    out = model.train_step(ddata)
    loss = float(out["loss"])
    print(f"loss {loss!r} vs {ref_loss.item()!r}: relative {abs(loss - ref_loss.item()) / abs(ref_loss.item()):.3e}")
    assert np.isfinite(loss) and abs(loss - ref_loss.item()) <= 1e-4 * abs(ref_loss.item())
    eager = _gradient_flags(model)
    print("non-finite gradients:", sorted(k for k, v in eager.items() if v))
    assert eager == {k: want[k] for k in eager}, sorted(k for k in eager if eager[k] != want[k])
    assert set(eager) == set(want)
    # the replayed step: capture on the healthy batch (its warm-up step is a real one), one replay on the stationary batch
    healthy = dict(ddata, trans=to_dev(np.stack([s["trans"] for s in D.model_sequence(2, D.STATIONARY_FRAME + 1)[1]], axis=1), dev))
    model_g, _ = _trainable_model(dev, weights)
    opt = torch.optim.Adam(model_g.parameters(), lr=1e-9, eps=1e-7, capturable=True)
    model_g.compile(optimizer=opt)
    runner = TR.GraphedTrainStep(model_g, healthy, opt, warmup=1)
    assert all(bool(torch.isfinite(p).all()) for p in model_g.parameters())
    loss_g = float(runner(ddata)[0])
    torch.cuda.synchronize()
    print(f"graph: loss {loss_g!r}")
    assert np.isfinite(loss_g) and abs(loss_g - ref_loss.item()) <= 1e-4 * abs(ref_loss.item())
    graph = _gradient_flags(model_g)
    assert graph == eager, sorted(k for k in eager if eager[k] != graph[k])
