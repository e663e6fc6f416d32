"""Backward kernels of the cost volumes (m4d_dscv_bwd / m4d_sncv_bwd through the
reference-named differentiable ops) vs autodiff of the torch-CPU restatement of the same
TF graph (oracle/m4depth_oracle_train.py).

Tolerances: the SNCV gradient is float32 sums of <= 49 products: 1e-5 relative to the
largest gradient.  The DSCV gradient passes through float16 multiplies (relative step 1e-3)
and an atomic scatter: 4e-3 of the largest gradient per tensor.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import m4depth_oracle as O
from oracle import m4depth_oracle_train as OT
from helpers import F, camera_np, cameras_np, motion_np, to_dev, npy, hbm_pressure
from grad_cases import CONV_BACKWARD_RECIPE_CASES, CV_RECIPE_LEVELS, conv_case_id

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    import m4depth_amd
    return m4depth_amd


def _close(got, want, tol, what):
    scale = float(np.max(np.abs(want))) + 1e-30
    err = float(np.max(np.abs(got - want))) / scale
    print(f"{what}: max |diff| / max |ref| = {err:.3e} (tol {tol})")
    assert err < tol, f"{what}: max |diff| / max |grad| = {err:.3e} (tol {tol})"


@pytest.mark.parametrize("C,k,r,h,w", [(16, 1, 4, 24, 40), (32, 2, 4, 12, 20), (96, 4, 2, 6, 10), (192, 8, 4, 6, 10)])
def test_dscv_backward(M, dev, C, k, r, h, w):
    _dscv_backward_case(M, dev, 2, C, k, r, h, w, seed=C + k)


@pytest.mark.parametrize("C,k,r,h,w", [(32, 2, 4, 12, 20), (192, 8, 4, 6, 10)])
def test_dscv_backward_per_sample_cameras(M, dev, C, k, r, h, w):
    """m4d_dscv_bwd at batch 3 with another, off-centre camera per sample (helpers.cameras_np; test_camera_cases.py checks that
    the restatement reads the camera per sample); the 4e-3 bar of the other cases."""
    _dscv_backward_case(M, dev, 3, C, k, r, h, w, seed=300 + C + k, cam_fn=cameras_np)


def _dscv_backward_case(M, dev, b, C, k, r, h, w, seed, t_scale=(1.0, 1.0, 1.0), disp_hi=6.0, cam_fn=camera_np):
    """Gradients of the DSCV on the device vs autodiff of the restatement; returns the forward's (y0, x0) grid."""
    rng = np.random.default_rng(seed)
    c1 = O.normalize_cuts(rng.normal(size=[b, h, w, C]).astype(F), k)
    c2 = O.normalize_cuts(rng.normal(size=[b, h, w, C]).astype(F), k)
    disp = rng.uniform(0.5, disp_hi, [b, h, w, 1]).astype(F)
    dpt = rng.uniform(0.5, 6.0, [b, h, w, 1]).astype(F)
    rot, trans = motion_np(rng, b, t_scale=t_scale)
    cam = cam_fn(b, h, w)
    ncp = 2 * r + 1
    g_cv = rng.normal(size=[b, h, w, k * ncp]).astype(F)
    g_pd = rng.normal(size=[b, h, w, ncp]).astype(F)

    tc = [torch.from_numpy(a).requires_grad_(True) for a in (c1, c2, dpt, disp)]
    cv, pd = OT.get_parallax_sweeping_cv(*tc, rot, trans, cam, r, nbre_cuts=k)
    (cv * torch.from_numpy(g_cv)).sum().add((pd * torch.from_numpy(g_pd)).sum()).backward()

    dc = [to_dev(a, dev).requires_grad_(True) for a in (c1, c2, dpt, disp)]
    cv_d, pd_d = M.get_parallax_sweeping_cv(*dc, to_dev(rot, dev), to_dev(trans, dev), to_dev(cam, dev), r, nbre_cuts=k)
    ((cv_d * to_dev(g_cv, dev)).sum() + (pd_d * to_dev(g_pd, dev)).sum()).backward()
    for name, t_cpu, t_dev in zip(("g_c1", "g_c2", "g_disp_prev_t", "g_disp"), tc, dc):
        assert t_dev.grad is not None, name
        _close(npy(t_dev.grad), t_cpu.grad.numpy(), 4e-3, f"dscv {name} {b}x{h}x{w} C={C} k={k}")
    with torch.no_grad():
        idx = M.get_parallax_sweeping_cv(*[t.detach() for t in dc], to_dev(rot, dev), to_dev(trans, dev), to_dev(cam, dev), r,
                                         nbre_cuts=k, return_index=True)[2]
    return npy(idx)


@pytest.mark.parametrize("C,k,r,same", [(16, 1, 3, True), (32, 2, 3, True), (32, 2, 2, False), (96, 4, 3, True)])
def test_sncv_backward(M, dev, C, k, r, same):
    _sncv_backward_case(M, dev, 2, 10, 14, C, k, r, same, seed=C + r)


def _sncv_backward_case(M, dev, b, h, w, C, k, r, same, seed):
    rng = np.random.default_rng(seed)
    c1 = O.normalize_cuts(rng.normal(size=[b, h, w, C]).astype(F), k)
    c2 = c1 if same else O.normalize_cuts(rng.normal(size=[b, h, w, C]).astype(F), k)
    g = rng.normal(size=[b, h, w, (2 * r + 1) ** 2 * k]).astype(F)

    t1 = torch.from_numpy(c1).requires_grad_(True)
    t2 = t1 if same else torch.from_numpy(c2).requires_grad_(True)
    (OT.cost_volume(t1, t2, r, nbre_cuts=k) * torch.from_numpy(g)).sum().backward()
    d1 = to_dev(c1, dev).requires_grad_(True)
    d2 = d1 if same else to_dev(c2, dev).requires_grad_(True)
    (M.cost_volume(d1, d2, r, nbre_cuts=k) * to_dev(g, dev)).sum().backward()
    _close(npy(d1.grad), t1.grad.numpy(), 1e-5, f"sncv g_c1 {b}x{h}x{w} C={C} k={k} same={same}")
    if not same:
        _close(npy(d2.grad), t2.grad.numpy(), 1e-5, f"sncv g_c2 {b}x{h}x{w} C={C} k={k}")


# ---- the cost volumes at the recipe's geometries: batch 3, the six levels of a 384 x 384 crop, level 1 of a KITTI frame ----
DSCV_WINDOW_FLOATS = 48 * 256          # the default LDS budget of m4d_dscv_bwd (csrc/m4d_grad.hip:333-334)


def dscv_window_mix(idx, C):
    """(private, direct): how many pixel blocks of dscv_bwd_kernel keep their g_c2 window in LDS and how many scatter
    straight to memory, from the forward's (y0, x0) grid [b, h, w, 2r+1, 2] and the block shape of the launcher
    (csrc/m4d_grad.hip:324-332), with the window test of the kernel (:128-130)."""
    b, h, w = idx.shape[:3]
    ppw = 64 // (C // 4)
    p2 = 0
    while (2 << p2) <= 4 * ppw:
        p2 += 1
    bh = 1 << (p2 // 2)
    bw = 1 << (p2 - p2 // 2)
    ph, pw = -(-h // bh) * bh, -(-w // bw) * bw
    pad = np.pad(idx, ((0, 0), (0, ph - h), (0, pw - w), (0, 0), (0, 0)), mode="edge")      # edge copies change no extreme
    blk = pad.reshape(b, ph // bh, bh, pw // bw, bw, -1, 2)
    lo, hi = blk.min(axis=(2, 4, 5)), blk.max(axis=(2, 4, 5))
    cells = (hi[..., 0] - lo[..., 0] + 2).astype(np.int64) * (hi[..., 1] - lo[..., 1] + 2)
    private = cells * C <= DSCV_WINDOW_FLOATS
    return int(private.sum()), int((~private).sum())


# The map with the wide motion (t_scale (3, 3, 1), as test_dscv_sncv_level_geometries) and parallaxes up to 24 pixels: the
# hypotheses of a block then sweep up to ~30 pixels along its epipolar line.  Where that line is diagonal the block's window
# (~38 x 38 cells x 16 floats) spills past the 48 KB budget and the block scatters straight to memory; where it runs along an
# axis (~38 x 10 cells) the window stays in LDS.  The test asserts that both kinds occur.
_DSCV_WIDE = dict(t_scale=(3.0, 3.0, 1.0), disp_hi=24.0)


@pytest.mark.parametrize("h,w,C,k", CV_RECIPE_LEVELS)
def test_dscv_backward_recipe_levels(M, dev, h, w, C, k):
    """m4d_dscv_bwd at batch 3, range 4, on every level geometry of the training recipe -- (64, 2) and (128, 4), 16 and 32
    lanes per pixel, run backward nowhere else -- against autodiff of the restatement.  The bar of the small cases holds
    unchanged: an entry of g_c2 is a scatter target of a handful of bilinear corners whatever the map size."""
    wide = (h, w) == (192, 192)
    idx = _dscv_backward_case(M, dev, 3, C, k, 4, h, w, seed=1000 + C + k + h, **(_DSCV_WIDE if wide else {}))
    private, direct = dscv_window_mix(idx, C)
    print(f"dscv {h}x{w} C={C}: {private} blocks with an LDS window, {direct} scattering straight to memory")
    if wide:
        # 24 x 24 = 576 blocks of 8 x 8 pixels per image: a multiple of 8, so the one-image-band-per-XCD swizzle is on
        assert private > 0 and direct > 0, (private, direct)


def test_dscv_backward_direct_scatter_at_level_1():
    """The same comparison at level 1's size with the LDS window switched off (M4D_DSCV_BWD_WINDOW_KB=0: every block
    scatters straight to memory).  The switch is read once per process, hence a fresh child; it gets its own time limit and
    is started once."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import torch, m4depth_amd as M, test_gpu_grad as T\n"
            "T._dscv_backward_case(M, torch.device('cuda:0'), 3, 16, 1, 4, 192, 192, seed=1209, **T._DSCV_WIDE)\n")
    env = dict(os.environ, M4D_DSCV_BWD_WINDOW_KB="0")
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(root, "tests"), root] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    res = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, timeout=600, capture_output=True, text=True)
    print(res.stdout)
    assert res.returncode == 0, f"child exited with status {res.returncode}:\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
    assert res.stdout.count("dscv g_") == 4, res.stdout


@pytest.mark.parametrize("h,w,C,k,same", [g + (True,) for g in CV_RECIPE_LEVELS] + [(48, 48, 64, 2, False)])
def test_sncv_backward_recipe_levels(M, dev, h, w, C, k, same):
    """m4d_sncv_bwd at batch 3, range 3 (the model's call: both inputs the same map) on the recipe's level geometries.  The
    bar does not depend on the map size: an entry is a float32 sum of <= 49 products (98 when both inputs are one map)."""
    _sncv_backward_case(M, dev, 3, h, w, C, k, 3, same, seed=2000 + C + h)


def test_dscv_backward_no_grad_paths(M, dev):
    """disp_prev_t comes out of prev_d2para's stop_gradient in the model (depth_operations.py:215):
    the op must work when only some inputs record gradients, and stay on the plain path otherwise."""
    rng = np.random.default_rng(2)
    b, h, w, C, k, r = 1, 8, 12, 16, 1, 4
    c1 = to_dev(O.normalize_cuts(rng.normal(size=[b, h, w, C]).astype(F), k), dev)
    c2 = to_dev(O.normalize_cuts(rng.normal(size=[b, h, w, C]).astype(F), k), dev)
    disp = to_dev(rng.uniform(0.5, 6.0, [b, h, w, 1]).astype(F), dev).requires_grad_(True)
    dpt = to_dev(rng.uniform(0.5, 6.0, [b, h, w, 1]).astype(F), dev)
    rot, trans = motion_np(rng, b)
    cam = to_dev(camera_np(b, h, w), dev)
    cv, pd = M.get_parallax_sweeping_cv(c1, c2, dpt, disp, to_dev(rot, dev), to_dev(trans, dev), cam, r)
    cv.sum().backward()
    assert disp.grad is not None and torch.isfinite(disp.grad).all()
    with torch.no_grad():
        cv2, _ = M.get_parallax_sweeping_cv(c1, c2, dpt, disp, to_dev(rot, dev), to_dev(trans, dev), cam, r)
    assert not cv2.requires_grad and torch.equal(cv2, cv.detach())


# ------------------------------------------------------------------ training glue kernels
def test_pack_conv_weights_kernel_matches_host_packer(M, dev):
    from m4depth_amd import network_ops as nops, training as TR
    rng = np.random.default_rng(0)
    for O, I in ((45, 37), (128, 122), (5, 16)):
        w = torch.from_numpy(rng.normal(size=[O, I, 3, 3]).astype(F)).to(dev).contiguous(memory_format=torch.channels_last)
        hwio = npy(w).transpose(2, 3, 1, 0)
        want, cpad = nops.pack_conv_weights(hwio)
        got, npad = TR._packed({}, w, False)
        assert npad == cpad and np.array_equal(npy(got), want)
        want_t, cpad_t = nops.pack_conv_weights(np.ascontiguousarray(hwio[::-1, ::-1].transpose(0, 1, 3, 2)))
        got_t, npad_t = TR._packed({}, w, True)
        assert npad_t == cpad_t and np.array_equal(npy(got_t), want_t)


def test_pack_conv_weights_lat_kernel_matches_host_packer(M, dev):
    """m4d_pack_conv_weights_lat (the per-step device packer of the training path: fragment-major layout of m4d_conv3x3_lat,
    every weight split exactly into three bf16 terms) against network_ops.pack_conv_weights_lat, forward and data-gradient
    (rotated / transposed) forms, bit for bit."""
    from m4depth_amd import network_ops as nops, training as TR
    rng = np.random.default_rng(1)
    for O, I in ((45, 37), (128, 122), (5, 16), (96, 128)):
        w = torch.from_numpy(rng.normal(size=[O, I, 3, 3]).astype(F)).to(dev).contiguous(memory_format=torch.channels_last)
        hwio = npy(w).transpose(2, 3, 1, 0)
        want = nops.pack_conv_weights_lat(hwio).view(np.int16)
        got = TR._packed_lat({}, w, False)
        assert got.shape == want.shape and np.array_equal(npy(got), want)
        want_t = nops.pack_conv_weights_lat(np.ascontiguousarray(hwio[::-1, ::-1].transpose(0, 1, 3, 2))).view(np.int16)
        got_t = TR._packed_lat({}, w, True)
        assert got_t.shape == want_t.shape and np.array_equal(npy(got_t), want_t)


def _upsample_case(dev, rng, b, h, w, c):
    from m4depth_amd import training as TR
    x = rng.normal(size=[b, h, w, c]).astype(F)
    g = rng.normal(size=[b, 2 * h, 2 * w, c]).astype(F)
    tx = torch.from_numpy(x).requires_grad_(True)
    (OT.resize_bilinear(tx, 2 * h, 2 * w, False) * 2.0 * torch.from_numpy(g)).sum().backward()
    dx = to_dev(x, dev).requires_grad_(True)
    (TR._upsample2_v1(dx, 2 * h, 2 * w, 2.0) * to_dev(g, dev)).sum().backward()
    _close(npy(dx.grad), tx.grad.numpy(), 1e-6, f"upsample adjoint {b}x{h}x{w}x{c}")


def _normalize_cuts_case(dev, rng, b, h, w, C, k):
    from m4depth_amd import training as TR
    x = rng.normal(size=[b, h, w, C]).astype(F)
    g = rng.normal(size=[b, h, w, C]).astype(F)
    tx = torch.from_numpy(x).requires_grad_(True)
    (OT.normalize_cuts(tx, k) * torch.from_numpy(g)).sum().backward()
    dx = to_dev(x, dev).requires_grad_(True)
    (TR._normalize_cuts(dx, k) * to_dev(g, dev)).sum().backward()
    _close(npy(dx.grad), tx.grad.numpy(), 1e-5, f"normalize_cuts backward {b}x{h}x{w}x{C} k={k}")


def _level_post_case(dev, rng, b, h, w, cam_fn=camera_np):
    from m4depth_amd import training as TR
    ro = rng.normal(0, 3.0, size=[b, h, w, 5]).astype(F)
    ro[0, 0, 0, 0] = 9.0                                   # outside the clip: no gradient
    rot, trans = motion_np(rng, b)
    cam = cam_fn(b, h, w)
    gs = [rng.normal(size=[b, h, w, n]).astype(F) for n in (1, 1, 4)]
    tro = torch.from_numpy(ro).requires_grad_(True)
    para = torch.exp(torch.clamp(tro[..., :1], -7., 7.)) / 0.5
    depth = OT.parallax2depth(para, rot, trans, cam)
    ((para * torch.from_numpy(gs[0])).sum() + (depth * torch.from_numpy(gs[1])).sum()
     + (tro[..., 1:] * torch.from_numpy(gs[2])).sum()).backward()
    dro = to_dev(ro, dev).requires_grad_(True)
    dcam = to_dev(cam, dev)
    p_d, d_d, o_d = TR._LevelPost.apply(dro, to_dev(rot, dev), to_dev(trans, dev), dcam["f"], dcam["c"], 0.5)
    ((p_d * to_dev(gs[0], dev)).sum() + (d_d * to_dev(gs[1], dev)).sum() + (o_d * to_dev(gs[2], dev)).sum()).backward()
    _close(npy(dro.grad), tro.grad.numpy(), 1e-5, f"level tail backward {b}x{h}x{w}")
    assert npy(dro.grad)[0, 0, 0, 0] == 0.0


def _loss_level_case(dev, rng, b, h, w, up, double=False):
    """The loss term of one level, both ground-truth kinds; ``double``: the restatement evaluated in float64."""
    from m4depth_amd import training as TR
    gt = rng.uniform(1, 80, size=[b, up * h, up * w, 1]).astype(F)
    pred = rng.uniform(0.005, 250, size=[b, h, w, 1]).astype(F)
    for kind in ("map", "velodyne"):
        gtk = gt * (rng.random(gt.shape) > 0.8) if kind == "velodyne" else gt
        gtk = gtk.astype(F)
        tp = torch.from_numpy(pred)
        tg = torch.from_numpy(gtk)
        if double:
            tp, tg = tp.double(), tg.double()
        tp.requires_grad_(True)
        ref = OT.m4depth_loss([None, {"depth": tg}], [None, [{"depth": tp}]], kind)
        ref.backward()
        dp = to_dev(pred, dev).requires_grad_(True)
        got = TR.m4depth_loss([None, {"depth": to_dev(gtk, dev)}], [None, [{"depth": dp}]], kind)
        got.backward()
        print(f"loss {b}x{h}x{w} ({kind}): {got.item()!r} vs {ref.item()!r}, relative {abs(got.item() - ref.item()) / abs(ref.item()):.3e}")
        assert abs(got.item() - ref.item()) <= 2e-6 * abs(ref.item()), (kind, got.item(), ref.item())
        _close(npy(dp.grad), tp.grad.numpy(), 1e-5, f"loss backward ({kind}) {b}x{h}x{w}")


def test_glue_backward_kernels_match_autodiff_of_the_restatement(M, dev):
    rng = np.random.default_rng(4)
    b, h, w = 2, 6, 9
    _upsample_case(dev, rng, b, h, w, 4)                   # x2 legacy upsample
    _normalize_cuts_case(dev, rng, b, h, w, 32, 2)         # per-cut normalisation
    _level_post_case(dev, rng, b, h, w)                    # level tail
    _loss_level_case(dev, rng, b, h, w, 4)                 # loss term of one level, both ground-truth kinds


def test_level_post_backward_per_sample_cameras(M, dev):
    """m4d_level_post_bwd at 3 x 6 x 9 with another, off-centre camera per sample (helpers.cameras_np); the 1e-5 bar."""
    _level_post_case(dev, np.random.default_rng(41), 3, 6, 9, cam_fn=cameras_np)


def test_glue_backward_kernels_at_recipe_geometries(M, dev):
    """The same kernels, references and bars on the maps of a batch-3 384 x 384 training step (the grids of
    m4d_resize_bilinear_v1_bwd, m4d_normalize_cuts_bwd and m4d_level_post_bwd are capped, so their grid-stride loops only
    run at such sizes).  None of the bars depends on the map size: every entry is a sum of at most 9 (upsample adjoint) or
    2 x C / cuts (normalisation) float32 terms."""
    rng = np.random.default_rng(40)
    _upsample_case(dev, rng, 3, 96, 96, 4)                 # 'other' of level 2 -> level 1
    _upsample_case(dev, rng, 3, 96, 96, 1)                 # parallax / depth
    _normalize_cuts_case(dev, rng, 3, 192, 192, 16, 1)
    _normalize_cuts_case(dev, rng, 3, 48, 48, 64, 2)
    _level_post_case(dev, rng, 3, 192, 192)


@pytest.mark.parametrize("h,w", [(192, 192), (128, 384)])
def test_loss_level_kernels_past_the_grid_cap(M, dev, h, w):
    """_LevelL1 (m4d_loss_level_fwd / _bwd) on level 1 of the recipe, against the restatement in float64.  m4d_loss_level_fwd
    launches at most 512 blocks of 256 lanes: 3 x 192 x 192 = 110592 predicted pixels (against a 384 x 384 ground truth)
    stay just below that cap, 3 x 128 x 384 = 147456 (KITTI finetuning, 256 x 768) are above it and every lane loops.  Bars
    as on the small maps: loss 2e-6 relative, gradient 1e-5 of its largest entry."""
    _loss_level_case(dev, np.random.default_rng(h + w), 3, h, w, 2, double=True)


def _bias_act_backward_case(dev, rng, rows, C, recipe):
    from m4depth_amd._lib import lib, dptr, stream_ptr, check
    g = rng.normal(size=[rows, C]).astype(F)
    out = rng.normal(size=[rows, C]).astype(F)
    dg, dout = to_dev(g, dev), to_dev(out, dev)
    gp = torch.empty_like(dg)
    gb = torch.empty(C, dtype=torch.float32, device=dev)
    n_ws = int(lib.m4d_bias_act_bwd_workspace_floats(rows, C))
    ws = torch.empty(n_ws, dtype=torch.float32, device=dev)
    check(lib.m4d_bias_act_bwd(dptr(dg), dptr(dout), rows, C, 0.1, dptr(gp), dptr(gb), dptr(ws), stream_ptr()), "bwd")
    want = g * np.where(out > 0, F(1.0), F(0.1))
    assert np.array_equal(npy(gp), want)
    ref = want.sum(axis=0, dtype=np.float64)
    err = float(np.max(np.abs(npy(gb) - ref)))
    if not recipe:
        print(f"bias gradient {rows}x{C}: max |diff| = {err:.3e}")
        np.testing.assert_allclose(npy(gb), ref, rtol=1e-5, atol=1e-4)
        return
    # The bound for the long columns, derived (not scaled from the 1000-row figure).  A term g * (1 or 0.1) has variance
    # (1 + 0.01) / 2, so a column sum -- and every partial sum on the way to it -- stays within 4 sigma = 4 * sqrt(0.505 * rows).
    # One float32 add rounds by at most 2^-24 of its result.  A term passes through: the lane's chain over its rows of the
    # block (rows_per_block / RP adds), the RP lane sums of the block, the finalize lane's chain over blocks / 64 partials, the
    # 6 butterfly steps.  The worst case -- every one of these adds rounding the same way at the final magnitude -- is the
    # bound; the expected error (a random walk, most adds at a far smaller magnitude) is some 30 times below it.
    # For 442368 x 16: 27 + 16 + 16 + 6 = 65 adds, sigma 473: 65 * 2^-24 * 1890 = 7.3e-3, i.e. 1.5e-5 sigma.  One row dropped
    # or counted twice moves an entry by ~0.5; one block's partial by ~15.
    blocks = n_ws // C
    rpb = -(-rows // blocks)
    rp = 256 // C
    adds = -(-rpb // rp) + rp + -(-blocks // 64) + 6
    bound = adds * 2.0 ** -24 * 4.0 * np.sqrt(0.505 * rows)
    print(f"bias gradient {rows}x{C}: {blocks} blocks, max |diff| = {err:.3e} (bound {bound:.3e}, column sigma {np.sqrt(0.505 * rows):.1f})")
    assert blocks > 64, (rows, C, blocks)                   # the finalize lanes chain several partials (<= 25 blocks on the small maps)
    assert err <= bound, f"bias gradient {rows}x{C}: max |diff| {err:.3e} > {bound:.3e}"


def test_bias_act_backward_kernel(M, dev):
    rng = np.random.default_rng(8)
    for rows, C in ((1000, 5), (777, 96), (300, 128), (64, 470)):
        _bias_act_backward_case(dev, rng, rows, C, recipe=False)


@pytest.mark.parametrize("rows,C", [(110592, 128), (442368, 16), (110592, 5), (27648, 192)])
def test_bias_act_backward_kernel_on_the_grid_cap(M, dev, rows, C):
    """The outputs of a batch-3 384 x 384 step: 3 x 192 x 192 rows of 128 and of 5 channels, 3 x 384 x 384 rows of 16, and the
    model's widest layer output (192 channels).  All but the 5-channel one (136 blocks) launch the 1024 blocks that
    bias_bwd_plan caps the grid at, and bias_grad_finalize_kernel adds 1024 partials per channel."""
    _bias_act_backward_case(dev, np.random.default_rng(rows + C), rows, C, recipe=True)


@pytest.mark.parametrize("b,h,w,cin,cout,stride", [
    (2, 16, 24, 32, 64, 1),       # whole 32-blocks (a small map: forward and data gradient on the latency-first kernel)
    (3, 24, 24, 128, 96, 1),      # level 4 of a 384x384 training crop at batch 3: the same kernels, partly filled last cout group
    (1, 40, 60, 32, 64, 1),       # above the small-map threshold: the fp32-MFMA pair
    (1, 9, 21, 122, 96, 1),       # ragged tiles, Cin not a multiple of 4 (the training graph's exact-width refiner input)
    (3, 12, 16, 16, 16, 2),       # stride 2, even size: TF pads bottom / right only
    (1, 11, 13, 64, 64, 2),       # stride 2, odd sizes: one before, one after
    (2, 20, 28, 3, 16, 1),        # the 3-channel image layer
    (1, 6, 10, 470, 128, 1),      # the widest refiner input
])
def test_conv_backward_kernels_match_float64_autodiff(M, dev, b, h, w, cin, cout, stride):
    _conv_backward_case(dev, b, h, w, cin, cout, stride)


def _conv_backward_case(dev, b, h, w, cin, cout, stride):
    """training._ConvBiasAct (forward MFMA convolution; backward = bias/activation kernel, data gradient through the MFMA
    convolution on rotated weights (+ m4d_dilate2 for stride 2), weight gradient through m4d_conv3x3_wgrad) against
    float64 autodiff of the same TF-'SAME' convolution on the CPU.  Tolerance: 2e-5 of the largest gradient entry (float32
    sums over up to b*h*w pixels / 9*Cout products).

    Why the same bar holds on the recipe's maps: a weight-gradient entry of layer (3, 192, 192, 128, 128) is a sum of 110592
    products of unit-variance values: magnitude ~330, the largest of the 147456 entries ~1500.  A workgroup accumulates
    18 tiles x 128 pixels = 2304 of them in float32 (random-walk rounding error ~1e-4), the 48 slices are then added in order
    (~7e-4 in total): the expected worst error is a few 1e-6 of the largest entry.  Dropping, duplicating or misplacing ONE
    tile changes entries by ~sqrt(128 / 110592) = 3 % of their size -- four orders of magnitude above the bar.

    The kink of the activation.  leaky_relu has no derivative at 0, and among the 10 million outputs of a level-1 layer a
    few lie within float32 rounding of it: there the device's output and the float64 one fall on different sides, each with
    a correct derivative of its own (1 or 0.1).  One such output moves its 9 * Cin weight-gradient entries by 0.9 * g * x ~ 1,
    i.e. ~1e-3 of the largest entry (measured on (3, 192, 192, 128, 96): 8.5e-4) -- the reference's arbitrary choice, not an
    error of either side.  So the float64 reference differentiates the function the device evaluated: the slope of every
    output is taken from the sign of the DEVICE's output, after asserting that the two sides disagree on that sign only
    where the float64 pre-activation is below the forward bar (2e-5 of the largest output).  Everything else -- the
    convolution, its three gradients, the bars -- is float64 autodiff as before."""
    import torch.nn.functional as TF
    from m4depth_amd import training as TR
    rng = np.random.default_rng(cin * 3 + cout + stride)
    x = rng.standard_normal([b, h, w, cin]).astype(F)
    k = (rng.standard_normal([cout, cin, 3, 3]) * np.sqrt(2.0 / (9 * cin))).astype(F)
    bias = (0.1 * rng.standard_normal([cout])).astype(F)
    oh, ow = -(-h // stride), -(-w // stride)
    gout = rng.standard_normal([b, oh, ow, cout]).astype(F)
    # float64 reference
    xr = torch.from_numpy(x).double().requires_grad_(True)
    kr = torch.from_numpy(k).double().requires_grad_(True)
    br = torch.from_numpy(bias).double().requires_grad_(True)
    ph = max((oh - 1) * stride + 3 - h, 0)
    pw = max((ow - 1) * stride + 3 - w, 0)
    xp = TF.pad(xr.permute(0, 3, 1, 2), (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2))
    y_lin = TF.conv2d(xp, kr, br, stride, 0).permute(0, 2, 3, 1)
    yr = TF.leaky_relu(y_lin, 0.1)
    # the product's autograd node
    xd = to_dev(x, dev).requires_grad_(True)
    wd = torch.nn.Parameter(to_dev(k, dev).contiguous(memory_format=torch.channels_last))
    bd = torch.nn.Parameter(to_dev(bias, dev))
    yd = TR._ConvBiasAct.apply(xd, wd, bd, stride, 0.1, {})
    print(f"conv {b}x{h}x{w} {cin}->{cout} s{stride} forward: max |diff| / max |ref| = "
          f"{float(np.max(np.abs(npy(yd) - yr.detach().numpy()))) / float(yr.detach().abs().max()):.3e} (tol 2e-05)")
    np.testing.assert_allclose(npy(yd), yr.detach().numpy(), atol=2e-5 * float(yr.detach().abs().max()))
    positive = (yd.detach() > 0).cpu()                     # the slope m4d_bias_act_bwd applies: out > 0 ? 1 : 0.1
    flipped = positive != (y_lin.detach() > 0)
    print(f"outputs on the other side of the activation's kink than in float64: {int(flipped.sum())} of {flipped.numel()}")
    assert bool((y_lin.detach().abs()[flipped] <= 2e-5 * float(yr.detach().abs().max())).all())
    slope = torch.where(positive, torch.tensor(1.0, dtype=torch.float64), torch.tensor(0.1, dtype=torch.float64))
    (y_lin * slope * torch.from_numpy(gout).double()).sum().backward()
    (yd * to_dev(gout, dev)).sum().backward()
    assert wd.grad.shape == wd.shape
    _close(npy(wd.grad), kr.grad.numpy(), 2e-5, "weight gradient")
    _close(npy(bd.grad), br.grad.numpy(), 2e-5, "bias gradient")
    _close(npy(xd.grad), xr.grad.numpy(), 2e-5, "data gradient")
    # deterministic: a second backward gives the same bits
    wd.grad = None
    xd.grad = None
    yd2 = TR._ConvBiasAct.apply(xd, wd, bd, stride, 0.1, {})
    (yd2 * to_dev(gout, dev)).sum().backward()
    assert torch.equal(yd2, yd)
    g1 = wd.grad.clone()
    wd.grad = None
    yd3 = TR._ConvBiasAct.apply(xd, wd, bd, stride, 0.1, {})
    (yd3 * to_dev(gout, dev)).sum().backward()
    assert torch.equal(wd.grad, g1)


@pytest.mark.parametrize("case", CONV_BACKWARD_RECIPE_CASES, ids=conv_case_id)
def test_conv_backward_kernels_at_recipe_geometries(M, dev, case):
    """The same comparison, bars and determinism check on the layers of a batch-3 384 x 384 training step (and of the
    256 x 768 KITTI finetuning step) that make a weight-gradient workgroup walk several tiles, or a wave of the thin kernel
    several items: tests/grad_cases.py, kept on those loops by tests/test_grad_cases.py."""
    _conv_backward_case(dev, case.b, case.h, case.w, case.cin, case.cout, case.stride)


@pytest.mark.parametrize("b,h,w,cin,cout", [(3, 192, 192, 128, 128), (3, 384, 384, 3, 16)])
def test_conv_wgrad_same_bits_beside_hbm_traffic(M, dev, b, h, w, cin, cout):
    """m4d_conv3x3_wgrad beside streaming HBM traffic gives the bits of the quiet chip: 18 tiles per workgroup on the
    prefetch / commit path, and 27 items per wave of the thin kernel's ping-pong.  A barrier missing around the commit, or a
    load of the second operand set consumed early, shows when memory is slow, not in a quiet run.  One comparison per case."""
    import ctypes
    from m4depth_amd._lib import lib, dptr, stream_ptr, check
    gen = torch.Generator(device="cpu").manual_seed(cin + cout)
    x = torch.randn(b, h, w, cin, generator=gen).to(dev)
    g = torch.randn(b, h, w, cout, generator=gen).to(dev)
    n_ws = int(lib.m4d_conv3x3_wgrad_workspace_floats(b, h, w, cin, cout, 1))
    ws = torch.empty(n_ws, dtype=torch.float32, device=dev)

    def wgrad():
        dw = torch.empty(cout, 9 * cin, dtype=torch.float32, device=dev)
        check(lib.m4d_conv3x3_wgrad(dptr(x), dptr(g), b, h, w, cin, cout, 1, dptr(ws), n_ws, ctypes.c_void_p(dw.data_ptr()),
                                    stream_ptr()), "m4d_conv3x3_wgrad")
        return dw

    quiet = wgrad()
    torch.cuda.synchronize()
    load = hbm_pressure(dev)
    load.queue(40)                                        # ~40 x 1 GB of copy traffic: far longer than the kernel
    busy = wgrad()
    torch.cuda.synchronize()
    assert torch.equal(busy.view(torch.int32), quiet.view(torch.int32)), \
        f"{int((busy.view(torch.int32) != quiet.view(torch.int32)).sum())} of {busy.numel()} entries differ beside HBM traffic"
