"""Streaming inference on the MI355X: B independent camera streams in one batch, per-sample trajectory resets from a device mask
(M4Depth.stream_step, network.GraphedStream; the masked level close m4d_refiner_tail6_m / m4d_refiner_tail_m / m4d_level_post_m
and m4d_stream_prepare).

Contract: sample s of a streamed batch gets exactly -- bit for bit -- what a batch-synchronised run of its own stream gives
(today's predict_step path): the reset estimate and state where its new_traj is set (m4depth_network.py:206-214), the normal
level step on its own state otherwise (:216-260).  Reduced sizes (4 levels, 64x128) unless a test says otherwise."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import m4depth_oracle as O
from m4depth_amd import synthetic as S
from helpers import npy, assert_bits_equal, rel_err, cameras_np, motion_np

pytestmark = pytest.mark.gpu

L, H, WD = 4, 64, 128


def _model(dev, weights, levels=L):
    import m4depth_amd as M
    model = M.M4Depth(nbre_levels=levels)
    model.load_numpy_weights(weights, dev)
    return model


def _frame(sample, cam, dev, new_traj=None, rows=None):
    """Device frame for stream_step from a make_sequence sample (``rows``: the batch rows to take, in order)."""
    sel = (lambda x: x) if rows is None else (lambda x: x[rows])
    nt = sample["new_traj"] if new_traj is None else np.asarray(new_traj, bool)
    return {"RGB_im": torch.from_numpy(np.ascontiguousarray(sel(sample["RGB_im"]))).to(dev),
            "rot": torch.from_numpy(np.ascontiguousarray(sel(sample["rot"]))).to(dev),
            "trans": torch.from_numpy(np.ascontiguousarray(sel(sample["trans"]))).to(dev),
            "new_traj": torch.from_numpy(np.ascontiguousarray(sel(nt) if new_traj is None else nt)).to(dev),
            "camera": {k: torch.from_numpy(np.ascontiguousarray(sel(v))).to(dev) for k, v in cam.items()}}


def _host_nt(frame):
    """The same frame for predict_step (today's path: new_traj on the host steers the control flow)."""
    return dict(frame, new_traj=frame["new_traj"].cpu())


def _levels_snapshot(model):
    """Per level (fine -> coarse): estimates and state, on the host."""
    out = []
    for lvl, est in zip(model.d_estimator.levels, model.last_estimates[-1]):
        out.append({"depth": npy(est["depth"]), "parallax": npy(est["parallax"]), "other": npy(est["other"]),
                    "prev_f": npy(lvl.prev_f_maps), "depth_prev_t": npy(lvl.depth_prev_t)})
    return out


def _arith(name):
    from m4depth_amd import network as net
    return net.conv_arithmetic("f32" if name == "f32" else "bf16x3")


@pytest.mark.parametrize("b", [2, 4])
@pytest.mark.parametrize("close", ["bf16x3", "f32", "level_post"])
def test_all_continue_equals_predict_step(dev, b, close, monkeypatch):
    """A synchronised batch (one reset frame, then continuing frames) through stream_step with the mask taken from new_traj:
    every frame's depth and every level's estimates and state are bit-identical to predict_step's -- under both convolution
    arithmetics (m4d_refiner_tail6_m / m4d_refiner_tail_m) and with the unfused close (m4d_level_post_m)."""
    from m4depth_amd import network as net
    if close == "level_post":
        monkeypatch.setattr(net, "fused_refiner_tail", False)
    W = S.init_weights(L, seed=11)
    samples, cam = S.make_sequence(b, 6, H, WD, seed=5, motion="lateral")
    with _arith(close):
        ref, got = _model(dev, W), _model(dev, W)
        for t, smp in enumerate(samples):
            fr = _frame(smp, cam, dev)
            d_ref = npy(ref.predict_step(_host_nt(fr))["depth"])
            d_got = npy(got.stream_step(fr)["depth"])
            assert_bits_equal(d_got, d_ref, f"[{close}] b={b} frame {t}: depth")
            for l, (x, y) in enumerate(zip(_levels_snapshot(got), _levels_snapshot(ref))):
                for k in x:
                    assert_bits_equal(x[k], y[k], f"[{close}] b={b} frame {t} level {l + 1}: {k}")


def _staggered(b, T):
    """new_traj[t][s]: every stream starts at frame 0 and starts a new trajectory once more at frame 2 + s % (T - 2)."""
    return [[t == 0 or t == 2 + s % (T - 2) for s in range(b)] for t in range(T)]


@pytest.mark.parametrize("b", [4, 8])
def test_staggered_resets_sample_independence(dev, b):
    """b streams with different reset frames in one batch.  For each sample j, a batch of b replicas of stream j is
    synchronised and runs today's path (predict_step); sample j of the mixed run equals sample j of the replica run bit for bit
    at every frame, output and every level.  b = 8 covers the persistent Winograd / batch dispatch."""
    T = 7
    W = S.init_weights(L, seed=12)
    samples, cam = S.make_sequence(b, T, H, WD, seed=6, motion="lateral")
    nt = _staggered(b, T)
    mixed = _model(dev, W)
    got = []
    for t in range(T):
        d = npy(mixed.stream_step(_frame(samples[t], cam, dev, new_traj=nt[t]))["depth"])
        got.append((d, _levels_snapshot(mixed)))
    for j in range(b):
        rep = _model(dev, W)
        for t in range(T):
            fr = _frame(samples[t], cam, dev, new_traj=[nt[t][j]] * b, rows=[j] * b)
            d = npy(rep.predict_step(_host_nt(fr))["depth"])
            assert_bits_equal(got[t][0][j], d[j], f"b={b} sample {j} frame {t}: depth")
            for l, (x, y) in enumerate(zip(got[t][1], _levels_snapshot(rep))):
                for k in x:
                    assert_bits_equal(x[k][j], y[k][j], f"b={b} sample {j} frame {t} level {l + 1}: {k}")


def test_reset_constants_and_state(dev):
    """Masked samples -- carrying trans = 0 and a stale state from another trajectory -- output exactly 1000 / pv / 0 at every
    level, store the features m4d_pyramid_reset stores for the same features and depth_prev_t = 1000; their unmasked neighbours
    are bit-identical to a run in which no sample was masked."""
    from m4depth_amd import network_ops as nops
    b, T = 4, 4
    W = S.init_weights(L, seed=13)
    samples, cam = S.make_sequence(b, T, H, WD, seed=7, motion="lateral")
    other, _ = S.make_sequence(b, 1, H, WD, seed=70, motion="lateral")
    a, ref = _model(dev, W), _model(dev, W)
    for t in range(T - 1):
        fr = _frame(samples[t], cam, dev)
        a.stream_step(fr)
        ref.stream_step(fr)
    mask = [True, False, True, False]
    last = dict(samples[T - 1])
    for k in ("RGB_im", "rot"):
        last[k] = np.where(np.reshape(mask, [b] + [1] * (last[k].ndim - 1)), other[0][k], last[k])
    last["trans"] = np.where(np.reshape(mask, [b, 1]), np.float32(0.0), last["trans"]).astype(np.float32)
    fa = _frame(last, cam, dev, new_traj=mask)
    out_a = npy(a.stream_step(fa)["depth"])
    out_r = npy(ref.stream_step(_frame(samples[T - 1], cam, dev, new_traj=[False] * b))["depth"])
    snap_a, snap_r = _levels_snapshot(a), _levels_snapshot(ref)
    f_pyr = a.encoder(fa["RGB_im"])
    for l, (x, y) in enumerate(zip(snap_a, snap_r)):
        lvl = a.d_estimator.levels[l]
        pv = np.float32(2.0 ** (L - 1 - l))
        # what m4d_pyramid_reset stores for these features (scratch state buffers)
        feats = f_pyr[l]
        st_f = torch.empty_like(feats)
        st_d = torch.empty(feats.shape[:3] + (1,), dtype=torch.float32, device=dev)
        nops.pyramid_reset([{"features": feats, "cuts": lvl.nbre_cuts, "state_features": st_f, "depth_state": st_d}], b)
        st_f = npy(st_f)
        for s in range(b):
            if mask[s]:
                assert np.all(x["depth"][s] == np.float32(1000.0)), (l, s)
                assert np.all(x["parallax"][s] == pv), (l, s)
                assert np.all(x["other"][s] == np.float32(0.0)) and not np.signbit(x["other"][s]).any(), (l, s)
                assert np.all(x["depth_prev_t"][s] == np.float32(1000.0)), (l, s)
                assert_bits_equal(x["prev_f"][s], st_f[s], f"level {l + 1} sample {s}: stored features")
            else:
                for k in x:
                    assert_bits_equal(x[k][s], y[k][s], f"level {l + 1} unmasked sample {s}: {k}")
    for s in range(b):
        if mask[s]:
            assert np.all(out_a[s] == np.float32(1000.0))
        else:
            assert_bits_equal(out_a[s], out_r[s], f"output, unmasked sample {s}")


@pytest.mark.parametrize("kernel", ["tail6", "tail", "post"])
def test_masked_close_kernels_guard_bands(dev, kernel):
    """The three masked closes on odd map sizes (partial tiles), outputs inside guard bands: masked samples get the reset
    constants, unmasked samples the bits of the unmasked entry point, and not one word outside the outputs changes."""
    b = 3
    rot = np.tile(np.array([[1.0, 0.01, -0.02, 0.005]], np.float32), (b, 1))
    trans = np.tile(np.array([[0.3, 0.1, 0.02]], np.float32), (b, 1))
    cam = {"f": np.full((b, 2), 20.0, np.float32), "c": np.full((b, 2), 10.0, np.float32)}
    _masked_close_case(dev, kernel, [1, 0, 1], rot, trans, cam)


@pytest.mark.parametrize("mask", [[1, 0, 1], [0, 1, 0]])
@pytest.mark.parametrize("kernel", ["tail6", "tail", "post"])
def test_masked_close_kernels_per_sample_cameras(dev, kernel, mask):
    """The same with another pose and another, off-centre camera per sample (helpers.cameras_np), every sample once the live
    one; the depth of every live sample is also held to the oracle: parallax2depth of the kernel's own parallax, bit for bit."""
    b, h, w = 3, 13, 29
    rot, trans = motion_np(np.random.default_rng(15), b)
    _masked_close_case(dev, kernel, mask, rot, trans, cameras_np(b, h, w), oracle=True)


def _masked_close_case(dev, kernel, mask, rot, trans, cam, oracle=False):
    from m4depth_amd import network as net, network_ops as nops
    from m4depth_amd._lib import lib
    b, h, w = 3, 13, 29
    rot_np, trans_np, cam_np = rot, trans, cam
    W = S.init_weights(2, seed=14)
    model = _model(dev, W, levels=2)
    lvl = model.d_estimator.levels[0]
    convs = list(lvl.disp_refiner.prep_conv_layers) + list(lvl.disp_refiner.est_d_conv_layers)
    g = torch.Generator(device="cpu").manual_seed(3)
    x32 = torch.randn((b, h, w, 32), generator=g).to(dev)
    ro = torch.randn((b, h, w, 5), generator=g).to(dev)
    rot = torch.from_numpy(rot_np).to(dev)
    trans = torch.from_numpy(trans_np).to(dev)
    cf = torch.from_numpy(cam_np["f"]).to(dev)
    cc = torch.from_numpy(cam_np["c"]).to(dev)
    mask = torch.tensor(mask, dtype=torch.uint8, device=dev)
    G = 256
    sentinel = -12345.5

    def guarded(n):
        buf = torch.full((n + 2 * G,), sentinel, dtype=torch.float32, device=dev)
        return buf, buf[G:G + n]

    n = b * h * w
    bufs = {k: guarded(n * c) for k, c in (("para", 1), ("depth", 1), ("other", 4), ("dstate", 1))}
    p = {k: ctypes.c_void_p(v[1].data_ptr()) for k, v in bufs.items()}
    scale, pv = 0.25, 8.0
    if kernel == "post":
        rc = lib.m4d_level_post_m(ctypes.c_void_p(ro.data_ptr()), ctypes.c_void_p(rot.data_ptr()), 4, ctypes.c_void_p(trans.data_ptr()),
                                  ctypes.c_void_p(cf.data_ptr()), ctypes.c_void_p(cc.data_ptr()), b, h, w, scale, p["para"], p["depth"],
                                  p["other"], p["dstate"], ctypes.c_void_p(mask.data_ptr()), pv, nops.stream_ptr())
        ref = nops.level_post(ro, rot, trans, {"f": cf, "c": cc}, scale)
    else:
        split = kernel == "tail6"
        with net.conv_arithmetic("bf16x3" if split else "f32"):
            w6, w7 = lvl._tail_weights(convs, split)
        fn = lib.m4d_refiner_tail6_m if split else lib.m4d_refiner_tail_m
        rc = fn(ctypes.c_void_p(x32.data_ptr()), ctypes.c_void_p(w6.data_ptr()), ctypes.c_void_p(convs[5].bias.data_ptr()),
                ctypes.c_void_p(w7.data_ptr()), ctypes.c_void_p(convs[6].bias.data_ptr()), ctypes.c_void_p(rot.data_ptr()), 4,
                ctypes.c_void_p(trans.data_ptr()), ctypes.c_void_p(cf.data_ptr()), ctypes.c_void_p(cc.data_ptr()), b, h, w, scale,
                p["para"], p["depth"], p["other"], p["dstate"], ctypes.c_void_p(mask.data_ptr()), pv, nops.stream_ptr())
        ref = (nops.refiner_tail6 if split else nops.refiner_tail)(x32, w6, convs[5].bias, w7, convs[6].bias, rot, trans,
                                                                    {"f": cf, "c": cc}, scale)
    assert rc == 0
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        band = npy(torch.cat([buf[:G], buf[-G:]]))
        assert np.all(band == np.float32(sentinel)), f"{kernel}: guard band of {k} overwritten"
    para, depth, oth, dst = (npy(bufs[k][1]) for k in ("para", "depth", "other", "dstate"))
    para, depth, dst = (v.reshape(b, h, w) for v in (para, depth, dst))
    oth = oth.reshape(b, h, w, 4)
    rp, rd, ro_ = (npy(t) for t in ref)
    for s in range(b):
        if int(mask[s]):
            assert np.all(para[s] == np.float32(pv)) and np.all(depth[s] == 1000.0) and np.all(dst[s] == 1000.0)
            assert np.all(oth[s] == 0.0)
        else:
            assert_bits_equal(para[s], rp[s, ..., 0], f"{kernel} parallax")
            assert_bits_equal(depth[s], rd[s, ..., 0], f"{kernel} depth")
            assert_bits_equal(dst[s], rd[s, ..., 0], f"{kernel} depth state")
            assert_bits_equal(oth[s], ro_[s], f"{kernel} other")
            if oracle:
                want = O.parallax2depth(para[s:s + 1, ..., None], rot_np[s:s + 1], trans_np[s:s + 1],
                                        {k: v[s:s + 1] for k, v in cam_np.items()})
                assert_bits_equal(depth[s], want[0, ..., 0], f"{kernel} sample {s}: depth = parallax2depth(parallax)")
    if oracle:                                                                    # ... and the unmasked entry, every sample
        assert_bits_equal(rd, O.parallax2depth(rp, rot_np, trans_np, cam_np), f"unmasked {kernel}: depth = parallax2depth(parallax)")


def test_staggered_resets_against_the_oracle(dev):
    """Well-conditioned fixture (synthetic.well_conditioned_case), staggered resets: every sample of the batch agrees with a
    batch-1 oracle.M4Depth stream of that sample, frame by frame, within 1e-4 relative on every pixel."""
    b, T, rd, rs = 4, 5, 4, 3
    W, samples, cam = S.well_conditioned_case(L, b, T, H, WD, 4321, rd, rs)
    nt = _staggered(b, T)
    model = _model(dev, W)
    got = [npy(model.stream_step(_frame(samples[t], cam, dev, new_traj=nt[t]))["depth"]) for t in range(T)]
    worst = 0.0
    for j in range(b):
        seq = [{"RGB_im": s["RGB_im"][j:j + 1], "rot": s["rot"][j:j + 1], "trans": s["trans"][j:j + 1],
                "new_traj": np.array([nt[t][j]])} for t, s in enumerate(samples)]
        _, d_seq = O.M4Depth(W, L, dscv_range=rd, sncv_range=rs)(seq, {k: v[j:j + 1] for k, v in cam.items()})
        for t in range(T):
            want = O.resize_nearest(d_seq[t][0]["depth"], H, WD)
            rel = rel_err(got[t][j:j + 1], want, 1e-30)
            worst = max(worst, float(rel.max()))
            assert rel.max() < 1e-4, f"sample {j} frame {t}: max relative depth error {rel.max():.2e}"
    print(f"streamed staggered resets vs the batch-1 oracle: max relative depth error {worst:.2e}")


def _graph_vs_eager(dev, b, levels, h, w, masks, reset_at=None, seed=21):
    from m4depth_amd import network as net
    W = S.init_weights(levels, seed=seed)
    samples, cam = S.make_sequence(b, len(masks), h, w, seed=seed, motion="lateral")
    eager, graphed = _model(dev, W, levels), _model(dev, W, levels)
    runner = net.GraphedStream(graphed, _frame(samples[0], cam, dev, new_traj=masks[0]))
    for t, m in enumerate(masks):
        fr = _frame(samples[t], cam, dev, new_traj=m)
        force = reset_at is not None and t == reset_at
        if force:
            runner.reset_state()
        d_e = npy(eager.stream_step(fr, force_reset=force)["depth"])
        d_g = npy(runner(fr)["depth"])
        assert_bits_equal(d_g, d_e, f"b={b} {h}x{w} frame {t}: GraphedStream vs stream_step")
        if t == 0 or force:
            assert np.all(d_g == np.float32(1000.0)), f"frame {t}: not a full reset"
        for l, (x, y) in enumerate(zip(_levels_snapshot(graphed), _levels_snapshot(eager))):
            for k in ("prev_f", "depth_prev_t"):
                assert_bits_equal(x[k], y[k], f"b={b} frame {t} level {l + 1}: {k}")
    return runner


@pytest.mark.parametrize("b", [1, 4])
def test_graphed_stream_equals_stream_step(dev, b):
    """GraphedStream replays (two graphs, alternating parity) == eager stream_step, bit for bit, over 9 frames (both parities,
    an odd count) with the mask changing every frame: a fresh runner's first frame is a full reset although new_traj is all
    false; all-set, all-clear and mixed masks; reset_state() forces the next frame to reset every sample."""
    F, Tr = [False] * b, [True] * b
    mixed = [s % 2 == 0 for s in range(b)]
    mixed2 = [s % 3 == 1 for s in range(b)]
    masks = [F, F, Tr, F, mixed, F, mixed2, F, F]
    runner = _graph_vs_eager(dev, b, L, H, WD, masks, reset_at=6)
    assert len(runner.graphs) == 2


def test_graphed_stream_equals_stream_step_fullsize(dev):
    """The same at configs[1]'s geometry (384x1280, 6 levels), batch 1, 7 frames."""
    masks = [[False], [False], [False], [True], [False], [False], [False]]
    _graph_vs_eager(dev, 1, 6, 384, 1280, masks, seed=22)


def test_graphed_stream_has_only_library_kernels(tmp_path):
    """Every kernel node of the captured per-frame graphs is one of libm4depth_hip.so's (the HIP runtime's own graph dump, in a
    fresh process: tools/dump_graph_nodes.py --stream exits non-zero on a foreign node)."""
    import re
    dot = tmp_path / "stream.dot"
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "dump_graph_nodes.py")
    res = subprocess.run([sys.executable, tool, "--stream", "--batch", "2", "--height", str(H), "--width", str(WD),
                          "--levels", str(L), "--frames", "1", "--out", str(dot)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    names = re.findall(r"_Z\w+", dot.read_text())
    assert len(names) >= 20, f"no kernel nodes recognised in the graph dump ({len(names)})"
    assert any("stream_prepare_kernel" in n for n in names)
    assert not [n for n in names if "at6native" in n or "at4cuda" in n or "rocclr" in n]


def test_stream_input_validation(dev):
    """Wrong shapes, a CPU tensor among device ones, and a training-mode model each raise a clear error."""
    import m4depth_amd as M
    from m4depth_amd import network as net
    W = S.init_weights(L, seed=15)
    samples, cam = S.make_sequence(2, 1, H, WD, seed=8)
    model = _model(dev, W)
    fr = _frame(samples[0], cam, dev)
    with pytest.raises(ValueError, match="rot"):
        model.stream_step(dict(fr, rot=torch.zeros(2, 5, device=dev)))
    with pytest.raises(ValueError, match="new_traj"):
        model.stream_step(dict(fr, new_traj=torch.zeros(3, dtype=torch.bool, device=dev)))
    with pytest.raises(ValueError, match="camera"):
        model.stream_step(dict(fr, camera={"f": fr["camera"]["f"][:1], "c": fr["camera"]["c"]}))
    with pytest.raises(RuntimeError, match="new_traj is on cpu"):
        model.stream_step(dict(fr, new_traj=fr["new_traj"].cpu()))
    with pytest.raises(TypeError, match="new_traj"):
        model.stream_step(dict(fr, new_traj=torch.zeros(2, dtype=torch.float32, device=dev)))
    trainee = M.M4Depth(nbre_levels=L, is_training=True)
    trainee.load_numpy_weights(W, dev)
    with pytest.raises(RuntimeError, match="is_training=False"):
        trainee.stream_step(fr)
    with pytest.raises(RuntimeError, match="not training mode"):
        lvl = trainee.d_estimator.levels[0]
        lvl(torch.zeros(2, 32, 64, 16, device=dev), None, fr["rot"], fr["trans"], fr["camera"], None,
            reset_mask=torch.zeros(2, dtype=torch.uint8, device=dev), reset_parallax=1.0)
    runner = net.GraphedStream(model, fr)
    with pytest.raises(ValueError, match="captured for"):
        runner(dict(fr, trans=torch.zeros(2, 4, device=dev)))
    with pytest.raises(RuntimeError, match="device tensor"):
        runner(dict(fr, RGB_im=fr["RGB_im"].cpu()))
    model.reset_state()
    with pytest.raises(RuntimeError, match="reset_state"):
        runner(fr)
