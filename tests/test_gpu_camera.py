"""Every camera-consuming kernel with per-sample, off-centre intrinsics (helpers.cameras_np: f != c, another camera per
sample, no dyadic value) at batch 3 -- the other GPU tests tile f = c = (0.5 w, 0.5 h) over the batch, so a kernel that read
cam_c for cam_f, sample 0's camera for every sample, or a camera captured into a graph would pass them
(tests/test_camera_cases.py shows on the CPU that each of these errors changes what is compared here).

Every kernel case asserts (a) the oracle's result and (b) batch independence on the device: sample s of the batch-3 launch
is, bit for bit, the batch-1 launch on sample s's inputs and camera.  Tolerances: those of test_gpu_ops.py (converters, DSCV,
prev_d2para, normalisation: bit-exact) and of the model tests (depth within 1e-4 relative of the oracle on every pixel of the
well-conditioned fixture).  The masked closes with these cameras are in test_gpu_stream.py, the fused fronts in
test_gpu_ops.py, the backward kernels in test_gpu_grad.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import m4depth_oracle as O
from m4depth_amd import synthetic as S
from helpers import (F, camera_np, cameras_np, stream_camera_np, camera_model_case, CAMERA_MODEL_CASE, take, motion_np, to_dev,
                     npy, assert_bits_equal, rel_err)

pytestmark = pytest.mark.gpu

B = 3


@pytest.fixture(scope="module")
def M():
    import m4depth_amd
    return m4depth_amd


def _each_sample(batch_out, names, launch_one):
    """(b): ``launch_one(s)`` -- the same kernel at batch 1 on sample s -- gives sample s of the batch launch, bit for bit."""
    for s in range(B):
        one = launch_one(s)
        for name, whole, part in zip(names, batch_out, one):
            assert part.shape[0] == 1
            assert torch.equal(whole[s:s + 1], part), f"sample {s} of the batch launch is not its batch-1 launch: {name}"


# ------------------------------------------------------------------------------- converters and reproject
@pytest.mark.parametrize("h,w", [(10, 14), (37, 53)])                  # one workgroup; eight workgroups, the last one ragged
@pytest.mark.parametrize("quat", [True, False])
def test_converters_and_reproject(M, dev, quat, h, w):
    rng = np.random.default_rng(1000 + h)
    rot, trans = motion_np(rng, B, quat=quat)
    cam = cameras_np(B, h, w)
    depth = (1 + 50 * rng.random([B, h, w, 1])).astype(F)
    para = (0.2 + 6.0 * rng.random([B, h, w, 1])).astype(F)
    img = rng.standard_normal([B, h, w, 3]).astype(F)
    d = {k: to_dev(v, dev) for k, v in dict(rot=rot, trans=trans, depth=depth, para=para, img=img, cam=cam).items()}

    def launch(x):
        warped, (pmr, rotc) = M.reproject(x["img"], x["depth"], x["rot"], x["trans"], x["cam"])
        return [M.parallax2depth(x["para"], x["rot"], x["trans"], x["cam"]),
                M.depth2parallax(x["depth"], x["rot"], x["trans"], x["cam"]),
                M.prev_d2para(x["depth"], x["rot"], x["trans"], x["cam"]),
                M.recompute_depth(x["depth"], x["rot"], x["trans"], x["cam"]), warped, pmr, rotc]

    names = ["parallax2depth", "depth2parallax", "prev_d2para", "recompute_depth", "reproject", "reproject aux 0", "reproject aux 1"]
    o_warped, (o_pmr, o_rotc) = O.reproject(img, depth, rot, trans, cam)
    want = [O.parallax2depth(para, rot, trans, cam), O.depth2parallax(depth, rot, trans, cam),
            O.prev_d2para(depth, rot, trans, cam), O.recompute_depth(depth, rot, trans, cam), o_warped, o_pmr, o_rotc]
    got = launch(d)
    for name, g, o in zip(names, got, want):
        assert_bits_equal(npy(g), o, f"{name} {h}x{w} quat={quat}")
    _each_sample(got, names, lambda s: launch(take(d, s)))


# ------------------------------------------------------------------------------- DSCV forward
def _cv_inputs(h, w, C, k, seed):
    """As test_dscv_sncv_level_geometries builds them, at batch 3 with cameras_np."""
    rng = np.random.default_rng(seed)
    cam = cameras_np(B, h, w)
    rot, trans = motion_np(rng, B, t_scale=(3.0, 3.0, 1.0))
    c1 = O.normalize_cuts(rng.standard_normal([B, h, w, C]).astype(F), k)
    c2 = O.normalize_cuts(rng.standard_normal([B, h, w, C]).astype(F), k)
    disp = (0.2 + 6.0 * rng.random([B, h, w, 1])).astype(F)
    dpt = (0.2 + 6.0 * rng.random([B, h, w, 1])).astype(F)
    return dict(c1=c1, c2=c2, dpt=dpt, disp=disp, rot=rot, trans=trans, cam=cam)


@functools.lru_cache(maxsize=None)
def _dscv_case(h, w, C, k):
    """Inputs and the oracle's results for both accumulation modes, computed once for the five kernel variants."""
    x = _cv_inputs(h, w, C, k, 100 + C + k)
    want = {}
    for acc in ("fp32_round", "fp16_seq"):
        cv, pd, oy, ox = O.get_parallax_sweeping_cv(x["c1"], x["c2"], x["dpt"], x["disp"], x["rot"], x["trans"], x["cam"], 4, k,
                                                    cv_accum=acc, return_index=True)
        want[acc] = (cv, pd, np.stack([oy, ox], -1))
    return x, want


@pytest.mark.parametrize("h,w,C,k", [(12, 20, 16, 1), (12, 20, 32, 2), (6, 10, 96, 4), (6, 20, 192, 8)])
@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4])
def test_dscv_forward_variants(M, dev, variant, h, w, C, k):
    """Every kernel variant of m4d_dscv_fwd, both float16-mean accumulations: index grid, cost volume and warped parallax."""
    from m4depth_amd._lib import lib
    x, want = _dscv_case(h, w, C, k)
    d = to_dev(x, dev)

    def launch(v, acc):
        return list(M.get_parallax_sweeping_cv(v["c1"], v["c2"], v["dpt"], v["disp"], v["rot"], v["trans"], v["cam"], 4, k,
                                               cv_accum=acc, return_index=True))

    try:
        lib.m4d_dscv_set_variant(variant)
        for acc in ("fp32_round", "fp16_seq"):
            cv, pd, idx = got = launch(d, acc)
            assert np.array_equal(npy(idx), want[acc][2]), f"variant {variant} {acc}: DSCV index grid"
            assert_bits_equal(npy(cv), want[acc][0], f"dscv cv, variant {variant} {acc} C={C}")
            assert_bits_equal(npy(pd), want[acc][1], f"dscv prev_disp, variant {variant} {acc}")
            _each_sample(got, ["cv", "prev_disp", "index grid"], lambda s: launch(take(d, s), acc))
    finally:
        lib.m4d_dscv_set_variant(1)


def test_merged_cost_volume_launch(M, dev):
    """m4d_dscv_sncv_fwd (both volumes of a small map in one launch), called as test_gpu_ops.test_merged_cost_volume_launch
    calls it."""
    from m4depth_amd._lib import lib, check, dptr, stream_ptr
    h, w, C, k = 12, 20, 128, 4
    x = _cv_inputs(h, w, C, k, 7)
    stride = 9 * k + 49 * k + 3

    def launch(v):
        b = v["c1"].shape[0]
        t = to_dev(v, dev)
        cf, cc = t["cam"]["f"], t["cam"]["c"]
        buf = torch.zeros(b, h, w, stride, device=dev)
        base = buf.data_ptr()
        check(lib.m4d_dscv_sncv_fwd(dptr(t["c1"]), dptr(t["c2"]), dptr(t["dpt"]), dptr(t["disp"]), dptr(t["rot"]), t["rot"].shape[1],
                                    dptr(t["trans"]), dptr(cf), dptr(cc), b, h, w, C, 4, k, 0, ctypes.c_void_p(base), stride, None, None,
                                    1, 1.0, 3, ctypes.c_void_p(base + 4 * (9 * k + 1)), stride, stream_ptr()), "m4d_dscv_sncv_fwd")
        return [buf]

    got = launch(x)
    ocv, _ = O.get_parallax_sweeping_cv(x["c1"], x["c2"], x["dpt"], x["disp"], x["rot"], x["trans"], x["cam"], 4, k)
    assert_bits_equal(npy(got[0][..., :9 * k]), ocv, "dscv through the merged entry")
    assert_bits_equal(npy(got[0][..., 9 * k + 1:9 * k + 1 + 49 * k]), O.cost_volume(x["c1"], x["c1"], 3, nbre_cuts=k),
                      "sncv through the merged entry")
    _each_sample(got, ["merged rows"], lambda s: launch(take(x, s)))


# ------------------------------------------------------------------------------- level_pre / level_pre_normalize
@pytest.mark.parametrize("normalize", [False, True])
def test_level_pre_kernels(M, dev, normalize):
    """para_prev_t of m4d_level_pre / m4d_level_pre_normalize is the oracle's prev_d2para, as in test_level_pre_post_kernels."""
    from m4depth_amd import network_ops as nops
    rng = np.random.default_rng(10)
    h, w, C, k = 13, 21, 32, 2
    rot, trans = motion_np(rng, B)
    cam = cameras_np(B, h, w)
    x = {"depth": (1 + 50 * rng.random([B, 7, 11, 1])).astype(F), "parallax": (0.1 + 3 * rng.random([B, 7, 11, 1])).astype(F),
         "other": rng.standard_normal([B, 7, 11, 4]).astype(F), "dprev": (1 + 50 * rng.random([B, h, w, 1])).astype(F),
         "raw": rng.standard_normal([B, h, w, C]).astype(F), "trans": trans, "cam": cam}

    def launch(v):
        v = to_dev(v, dev)
        b = v["dprev"].shape[0]
        prev = {n: v[n] for n in ("depth", "parallax", "other")}
        nout = torch.empty_like(v["raw"])
        para, depth, other, para_t = nops.level_pre(prev, v["dprev"], v["trans"], v["cam"], b, h, w, dev,
                                                    normalize=(v["raw"], k, nout) if normalize else None)
        return [para, depth, other, para_t] + ([nout] if normalize else [])

    got = launch(x)
    names = ["para_prev_l", "depth_prev_l", "other_prev_l", "para_prev_t", "normalised features"]
    want = [O.resize_bilinear_v1(x["parallax"], h, w) * F(2.), O.resize_bilinear_v1(x["depth"], h, w),
            O.resize_bilinear_v1(x["other"], h, w), O.prev_d2para(x["dprev"], rot, trans, cam), O.normalize_cuts(x["raw"], k)]
    for name, g, o in zip(names, got, want):
        assert_bits_equal(npy(g), o, name)
    _each_sample(got, names, lambda s: launch(take(x, s)))


# ------------------------------------------------------------------------------- unmasked closes
@pytest.mark.parametrize("kernel", ["post", "tail", "tail6"])
def test_level_closes(M, dev, kernel):
    """m4d_level_post, m4d_refiner_tail and m4d_refiner_tail6 on a 13 x 29 map: the depth is the oracle's parallax2depth of the
    kernel's own parallax, and the depth state is that depth (their masked forms: test_gpu_stream.py)."""
    from m4depth_amd import network_ops as nops
    rng = np.random.default_rng(29)
    h, w = 13, 29
    rot, trans = motion_np(rng, B)
    cam = cameras_np(B, h, w)
    scale = 0.25
    k6 = (rng.standard_normal([3, 3, 32, 16]) * np.sqrt(2.0 / (9 * 32))).astype(F)
    k7 = (rng.standard_normal([3, 3, 16, 5]) * np.sqrt(1.0 / (9 * 16))).astype(F)
    b6, b7 = (0.1 * rng.standard_normal([16])).astype(F), (0.1 * rng.standard_normal([5])).astype(F)
    x = {"x32": np.maximum(rng.standard_normal([B, h, w, 32]), -0.3).astype(F), "ro": (rng.standard_normal([B, h, w, 5]) * 2).astype(F),
         "rot": rot, "trans": trans, "cam": cam}
    if kernel == "tail":
        w6, w7 = (to_dev(a, dev) for a in nops.pack_refiner_tail_weights(k6, k7))
    elif kernel == "tail6":
        w6, w7 = (torch.from_numpy(a.view(np.int16)).to(dev) for a in nops.pack_refiner_tail_weights6(k6, k7))

    def launch(v):
        v = to_dev(v, dev)
        state = torch.zeros(v["ro"].shape[:3] + (1,), device=dev)
        if kernel == "post":
            out = nops.level_post(v["ro"], v["rot"], v["trans"], v["cam"], scale, depth_state=state)
        else:
            fn = nops.refiner_tail if kernel == "tail" else nops.refiner_tail6
            out = fn(v["x32"], w6, to_dev(b6, dev), w7, to_dev(b7, dev), v["rot"], v["trans"], v["cam"], scale, depth_state=state)
        return list(out) + [state]

    para, depth, other, state = got = launch(x)
    assert_bits_equal(npy(depth), O.parallax2depth(npy(para), rot, trans, cam), f"{kernel}: depth = parallax2depth(parallax)")
    assert torch.equal(state, depth)
    if kernel == "post":
        want = (np.exp(np.clip(x["ro"][..., :1], F(-7), F(7))) / F(scale)).astype(F)
        assert rel_err(npy(para), want).max() < 2e-6
        assert_bits_equal(npy(other), x["ro"][..., 1:], "other")
    _each_sample(got, ["parallax", "depth", "other", "depth state"], lambda s: launch(take(x, s)))


# ------------------------------------------------------------------------------- camera pyramid
def test_camera_pyramid(dev):
    """m4d_camera_pyramid: camera / 2^(l+1) for every level (an exact halving).  Non-contiguous [b, 2] views must be copied or
    refused, never read with the wrong stride."""
    from m4depth_amd import network_ops as nops
    cam = cameras_np(B, 64, 96)
    levels = 6

    def check_levels(out):
        assert len(out) == levels
        for l, lc in enumerate(out):
            for k in ("f", "c"):
                assert tuple(lc[k].shape) == (B, 2)
                assert_bits_equal(npy(lc[k]), cam[k] / F(2.0 ** (l + 1)), f"level {l} camera[{k}]")

    check_levels(nops.camera_pyramid(to_dev(cam, dev), levels))
    one = nops.camera_pyramid(to_dev(take(cam, 1), dev), levels)
    for l in range(levels):
        for k in ("f", "c"):
            assert_bits_equal(npy(one[l][k]), cam[k][1:2] / F(2.0 ** (l + 1)), f"batch 1, level {l} camera[{k}]")
    rng = np.random.default_rng(5)
    views = {}
    wide = {k: to_dev(rng.standard_normal([B, 4]).astype(F), dev) for k in cam}          # every other column of a [b, 4] tensor
    for k in cam:
        wide[k][:, ::2] = to_dev(cam[k], dev)
    views["strided columns"] = {k: v[:, ::2] for k, v in wide.items()}
    views["transposed"] = {k: to_dev(np.ascontiguousarray(cam[k].T), dev).t() for k in cam}
    packed = to_dev(np.stack([cam["f"], cam["c"]], axis=1), dev)                         # [b, 2, 2]: f and c interleaved per sample
    views["rows of a packed tensor"] = {"f": packed[:, 0], "c": packed[:, 1]}
    for name, v in views.items():
        assert not v["f"].is_contiguous() and not v["c"].is_contiguous(), name
        try:
            out = nops.camera_pyramid(v, levels)
        except (ValueError, RuntimeError) as e:
            print(f"camera_pyramid refuses {name}: {e}")
            continue
        check_levels(out)


# ------------------------------------------------------------------------------- the model
def _model(dev, W, levels):
    import m4depth_amd
    model = m4depth_amd.M4Depth(nbre_levels=levels)
    model.load_numpy_weights(W, dev)
    return model


def _stream_frame(sample, cam, dev):
    return {"RGB_im": to_dev(sample["RGB_im"], dev), "rot": to_dev(sample["rot"], dev), "trans": to_dev(sample["trans"], dev),
            "new_traj": torch.from_numpy(np.ascontiguousarray(sample["new_traj"])).to(dev), "camera": to_dev(cam, dev)}


@functools.lru_cache(maxsize=None)
def _oracle_per_sample():
    """[sample][frame] -> the finest depth of the BATCH-1 oracle.M4Depth run of that sample with that sample's camera."""
    W, samples, cam = camera_model_case()
    L = CAMERA_MODEL_CASE[0]
    out = []
    for s in range(B):
        _, seq = O.M4Depth(W, L)(take(samples, s), take(cam, s))
        out.append([fr[0]["depth"] for fr in seq])
    return out


def _run_model_both_ways(dev, W, samples, cam):
    """The sequence call and a stream_step loop: per frame the finest-level depth [b,h/2,w/2,1] and the returned full-size depth
    ((sequence, stream), each a list over frames of (finest, output or None))."""
    L = CAMERA_MODEL_CASE[0]
    model = _model(dev, W, L)
    out = model([to_dev(samples, dev), to_dev(cam, dev)])["depth"]
    n = len(samples)
    seq = [(npy(fr[0]["depth"]), npy(out) if t == n - 1 else None) for t, fr in enumerate(model.last_estimates)]
    model = _model(dev, W, L)
    stream = []
    for smp in samples:
        d = model.stream_step(_stream_frame(smp, cam, dev))["depth"]
        stream.append((npy(model.last_estimates[-1][0]["depth"]), npy(d)))
    return seq, stream


@pytest.mark.parametrize("streams,fused_reset", [(0, True), (8, True), (0, False), (8, False)])
def test_model_against_the_batch_1_oracle(dev, streams, fused_reset):
    """The model case (well_conditioned_case(3, 3, 3, 64, 96, 4321) with cameras_np): every sample of the batch, on every frame,
    within 1e-4 relative on every pixel of the batch-1 oracle run of that sample with that sample's camera -- the sequence call
    and a stream_step loop, under each forward plan test_gpu_model.py switches between."""
    from m4depth_amd import network as net
    W, samples, cam = camera_model_case()
    H, Wd = CAMERA_MODEL_CASE[3:5]
    want = _oracle_per_sample()
    old = (net.fused_pyramid_reset, net.level_pipeline_streams)
    try:
        net.fused_pyramid_reset, net.level_pipeline_streams = fused_reset, streams
        runs = _run_model_both_ways(dev, W, samples, cam)
    finally:
        net.fused_pyramid_reset, net.level_pipeline_streams = old
    worst = 0.0
    for how, frames in zip(("sequence", "stream_step"), runs):
        assert len(frames) == len(samples)
        for t, (finest, output) in enumerate(frames):
            for s in range(B):
                rel = float(rel_err(finest[s:s + 1], want[s][t]).max())
                worst = max(worst, rel)
                assert rel < 1e-4, f"{how} sample {s} frame {t}: max relative depth error {rel:.2e}"
                if output is not None:
                    rel = float(rel_err(output[s:s + 1], O.resize_nearest(want[s][t], H, Wd)).max())
                    assert rel < 1e-4, f"{how} sample {s} frame {t}: output, max relative depth error {rel:.2e}"
    print(f"per-sample cameras, streams={streams} fused_reset={fused_reset}: max relative depth error to the batch-1 oracle {worst:.2e}")


def test_model_batch_permutation(dev):
    """The batch permuted by [2, 0, 1], camera rows included: the permuted output, bit for bit (same batch size, same dispatch)."""
    W, samples, cam = camera_model_case()
    perm = [2, 0, 1]
    ref = _run_model_both_ways(dev, W, samples, cam)
    got = _run_model_both_ways(dev, W, take(samples, perm), take(cam, perm))
    for how, fr_ref, fr_got in zip(("sequence", "stream_step"), ref, got):
        for t, (a, b) in enumerate(zip(fr_ref, fr_got)):
            for what, x, y in zip(("finest depth", "output"), a, b):
                if x is not None:
                    assert_bits_equal(y, x[perm], f"{how} frame {t}: {what} of the permuted batch")


# ------------------------------------------------------------------------------- graphs
def _state(model):
    return [(npy(l.prev_f_maps), npy(l.depth_prev_t)) for l in model.d_estimator.levels]


def test_graphed_stream_follows_a_changing_camera(dev):
    """GraphedStream, b = 2, 4 levels, 64 x 128, 6 frames, another camera on every frame (stream_camera_np): each replay is the
    eager stream_step of a second model on the same frames -- output and every level's state, bit for bit.  On frame 4 the caller
    writes the camera in place into the runner's static buffers and hands those back (no hand-over copy)."""
    from m4depth_amd import network as net
    b, L, H, Wd, T = 2, 4, 64, 128, 6
    W = S.init_weights(L, seed=21)
    samples, _ = S.make_sequence(b, T, H, Wd, seed=21, motion="lateral")
    eager, graphed = _model(dev, W, L), _model(dev, W, L)
    runner = net.GraphedStream(graphed, _stream_frame(samples[0], stream_camera_np(0, b, H, Wd), dev))
    previous = None
    for t, smp in enumerate(samples):
        cam = stream_camera_np(t, b, H, Wd)
        fr = _stream_frame(smp, cam, dev)
        d_e = npy(eager.stream_step(fr)["depth"])
        if t == 4:
            static = runner.input_buffers()["camera"]
            for k in static:
                static[k].copy_(fr["camera"][k])
            fr = dict(fr, camera=static)
        d_g = npy(runner(fr)["depth"])
        assert_bits_equal(d_g, d_e, f"frame {t}: GraphedStream vs stream_step")
        for l, (x, y) in enumerate(zip(_state(graphed), _state(eager))):
            assert_bits_equal(x[0], y[0], f"frame {t} level {l + 1}: prev_f")
            assert_bits_equal(x[1], y[1], f"frame {t} level {l + 1}: depth_prev_t")
        if t == 0:
            assert np.all(d_g == F(1000.0))
        else:
            assert np.isfinite(d_g).all() and not np.array_equal(d_g, previous)
        previous = d_g


def test_graphed_sequence_follows_the_camera_of_the_call(dev):
    """GraphedSequence captured with camera_np: a replay with cameras_np is the eager model on that data, bit for bit, and a
    replay with the first camera again gives the first result."""
    from m4depth_amd import network as net
    L, b, T, H, Wd = CAMERA_MODEL_CASE[:5]
    W, samples, cam_b = camera_model_case()
    cam_a = camera_np(b, H, Wd)
    ds = to_dev(samples, dev)
    data = {k: torch.stack([s[k] for s in ds], dim=1) for k in ("RGB_im", "rot", "trans")}
    data["new_traj"] = torch.stack([torch.from_numpy(s["new_traj"]) for s in samples], dim=1)
    eager = {}
    for name, cam in (("a", cam_a), ("b", cam_b)):
        eager[name] = _model(dev, W, L)([ds, to_dev(cam, dev)])["depth"].clone()
    assert not torch.equal(eager["a"], eager["b"])
    runner = net.GraphedSequence(_model(dev, W, L), dict(data, camera=to_dev(cam_a, dev)), autotune=False)
    first = runner(dict(data, camera=to_dev(cam_a, dev))).clone()
    assert torch.equal(first, eager["a"]), "replay with the captured camera"
    second = runner(dict(data, camera=to_dev(cam_b, dev))).clone()
    assert torch.equal(second, eager["b"]), "replay with another camera than the captured one"
    third = runner(dict(data, camera=to_dev(cam_a, dev))).clone()
    assert torch.equal(third, first), "replay with the first camera again"
