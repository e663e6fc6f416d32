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
routes is in DESIGN.md), and part d places inputs and outputs inside sentinel-filled allocations to show it."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import m4depth_oracle as O
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
