"""The photometric reprojection loss on the MI355X (csrc/m4d_photo.hip, training._LevelPhoto / photometric_loss) against the
torch-CPU restatement tests/photometric_ref.py.

Every case runs at b = 2 with per-sample, off-centre cameras (helpers.cameras_np), quaternion and small-angle rotations, at
6x8 (the coarsest TartanAir map, interior 4x6), 13x21 (odd: partial tiles, a halo that crosses tile borders in both axes)
and 24x40 (more than one 16x16 tile per axis).

Bars.  Nothing is fixed by hand: each bar is 4 x the error of the FLOAT32 restatement to the float64 one on the same case
(photometric_ref.yardstick; tests/test_photometric_ref.py records the figures) -- 4 x because a kernel may sum windows and
partials in another, equally valid order at two stages.  A wrong derivative term shows at 1e-2 and above (the planted-error
test).  The seeds are well conditioned (asserted by the CPU test): no auto-mask margin below 1e-5, so the masks must be equal
bit for bit, and at most 1 % of pixels within 1e-5 of a local kink, which the gradient comparisons leave out.

Measured on an MI355X, error (float32 restatement's own error; the bar is 4 x that):
  dwarp, of max |dwarp|:    6x8 1.2e-6 / 9.9e-7 (1.1e-6 / 1.4e-6), 13x21 1.7e-6 / 1.4e-6 (1.8e-6 / 1.0e-6),
                            24x40 2.9e-6 / 4.1e-6 (3.1e-6 / 4.1e-6)                          [quaternion / small angle]
  term, photo, smooth:      at most 6.5e-8 relative over all 12 forward cases (5.6e-8 .. 1.4e-7); masks and N identical
  g_depth, of max |g|:      6x8 5.1e-7 (1.3e-6) / 4.5e-7 (4.6e-7), 13x21 1.2e-6 (1.4e-6) / 1.1e-6 (1.8e-6),
                            24x40 2.3e-6 (2.4e-6) / 2.1e-6 (2.5e-6); 100 % of pixels compared
  nothing in view:          g_depth 8.0e-8 (1.2e-7)
  driver, depth-less rec.:  losses 0.134 0.176 0.149 | 0.117 0.137 0.133 over two epochs of three batches (eager; --graph alike)
  it learns:                median relative depth error 25 % -> 0.138 % (p90 0.365 %); float64 restatement 0.146 % (0.363 %)
"""
import os

import numpy as np
import pytest
import torch

import photometric_ref as R
from helpers import to_dev, npy, assert_bits_equal

pytestmark = pytest.mark.gpu

CASE_NAMES = list(R.CASES)


def _dev_case(case, dev):
    return {k: to_dev(np.asarray(v), dev) for k, v in case.items() if k != "name"}


def _forward(d, smooth=1e-3, automask=True):
    from m4depth_amd import network_ops as nops
    warped, dwarp, valid = nops.photo_warp_fwd(d["depth"], d["rot"], d["trans"], d["f"], d["c"], d["prev"])
    out4, mask = nops.photo_loss_fwd(d["depth"], warped, valid, d["cur"], d["prev"], smooth, automask)
    return warped, dwarp, valid, out4, mask


@pytest.mark.parametrize("H,W,levels", [(64, 96, 3), (48, 80, 4)])
def test_image_pyramid_bitwise(dev, H, W, levels):
    from m4depth_amd import network_ops as nops
    img = np.random.default_rng(H).uniform(0.0, 1.0, [3, H, W, 3]).astype(np.float32)
    got = nops.image_pyramid_box(to_dev(img, dev), levels)
    want = R.image_pyramid(torch.from_numpy(img), levels)
    assert len(got) == levels
    for i, (g, w_) in enumerate(zip(got, want)):
        assert tuple(g.shape) == (3, H >> (i + 1), W >> (i + 1), 3)
        assert_bits_equal(npy(g), w_.numpy(), f"pyramid level {i}")
    with pytest.raises(ValueError):
        nops.image_pyramid_box(to_dev(img, dev), 6)                  # 48 and 96 are no multiples of 64


def _warp_bits(dev, case):
    import m4depth_amd as M
    from m4depth_amd import network_ops as nops
    d = _dev_case(case, dev)
    warped, dwarp, valid = nops.photo_warp_fwd(d["depth"], d["rot"], d["trans"], d["f"], d["c"], d["prev"])
    dc = torch.clamp(d["depth"], 0.01, 200.0)
    want = M.depth_operations.reproject(d["prev"], dc, d["rot"], d["trans"], {"f": d["f"], "c": d["c"]})[0]
    assert_bits_equal(npy(warped), npy(want), case["name"] + ": warped vs depth_operations.reproject")
    t = {k: torch.from_numpy(np.asarray(v)) for k, v in case.items() if k != "name"}
    ref = R.warp(t["depth"], t["rot"], t["trans"], t["f"], t["c"], t["prev"])
    assert np.array_equal(npy(valid)[..., 0].astype(bool), ref["valid"].numpy()), case["name"] + ": valid"
    assert_bits_equal(npy(warped), ref["warped"].numpy(), case["name"] + ": warped vs the float32 restatement")
    assert np.isfinite(npy(dwarp)).all()
    return npy(valid)[..., 0].astype(bool)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_warp_bitwise(dev, name):
    valid = _warp_bits(dev, R.make_case(name))
    assert 0.5 < valid.mean() < 1.0                                   # both branches


def test_warp_bitwise_hostile_depths_and_motions(dev):
    """Depths outside [0.01, 200], negative and infinite ones; part of sample 0 out of view, part of sample 1 at Pz <= 0."""
    case = R.hostile_depth_case()
    valid = _warp_bits(dev, case)
    assert not valid[0, 2, 6] and not valid[0, 2, 8] and not valid[1, 5, 4]          # the infinite depths
    assert valid[0].any() and not valid[0].all() and valid[1].any() and not valid[1].all()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_dwarp_against_float64(dev, name):
    from m4depth_amd import network_ops as nops
    case = R.make_case(name)
    d = _dev_case(case, dev)
    _, dwarp, valid = nops.photo_warp_fwd(d["depth"], d["rot"], d["trans"], d["f"], d["c"], d["prev"])
    refs = {}
    for dt in (torch.float64, torch.float32):
        t = {k: torch.from_numpy(np.asarray(v)).to(dt) for k, v in case.items() if k != "name"}
        depth = t["depth"].clone().requires_grad_(True)
        wp = R.warp(depth, t["rot"], t["trans"], t["f"], t["c"], t["prev"])
        refs[dt] = torch.stack([torch.autograd.grad(wp["warped"][..., c].sum(), depth, retain_graph=True)[0][..., 0]
                                for c in range(3)], dim=-1).double().numpy()
        if dt == torch.float64:
            keep = (wp["valid"] & (R.well_conditioned(R.term_and_grad(case, torch.float64)[0]["margins"]))).numpy()
    scale = np.abs(refs[torch.float64][keep]).max()
    yard = np.abs(refs[torch.float32] - refs[torch.float64])[keep].max() / scale
    err = np.abs(npy(dwarp).astype(np.float64) - refs[torch.float64])[keep].max() / scale
    print(f"{name}: dwarp error {err:.3e} of max |dwarp| (float32 restatement {yard:.3e}, bar {4 * yard:.3e}), "
          f"{keep.mean():.3f} of pixels compared")
    assert keep.mean() > 0.5
    assert err <= 4 * yard


@pytest.mark.parametrize("automask", [True, False])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_forward_against_float64(dev, name, automask):
    y = R.yardstick(name)
    r64, _, _ = y["ref"][automask]
    _, _, _, out4, mask = _forward(_dev_case(y["case"], dev), 1e-3, automask)
    assert np.array_equal(npy(mask)[..., 0].astype(bool), r64["mask"].numpy()), "mask differs from the float64 restatement's"
    out4 = npy(out4).astype(np.float64)
    errs = {k: abs(out4[i] - r64[k].item()) / abs(r64[k].item()) for i, k in enumerate(("term", "photo", "smooth"))}
    print(f"{name} automask={automask}: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items())
          + f" (float32 restatement {y['loss']:.2e}, bar {4 * y['loss']:.2e}); N {out4[3]:.0f}")
    assert out4[3] == r64["n"].item() and 0 < out4[3] < mask.numel()
    for k, e in errs.items():
        assert e <= 4 * y["loss"], (k, e)


@pytest.mark.parametrize("automask", [True, False])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_backward_raw_abi_with_reference_mask(dev, name, automask):
    """m4d_photo_loss_bwd through the C ABI, fed the REFERENCE's mask and (term, photo, smooth, N)."""
    from m4depth_amd._lib import lib, dptr, stream_ptr
    y = R.yardstick(name)
    r64, g64, well = y["ref"][automask]
    d = _dev_case(y["case"], dev)
    warped, dwarp, _, _, _ = _forward(d, 1e-3, automask)
    mask = to_dev(r64["mask"].numpy().astype(np.uint8)[..., None], dev)
    out4 = to_dev(np.array([r64[k].item() for k in ("term", "photo", "smooth", "n")], np.float32), dev)
    g_out = to_dev(np.array([1.0], np.float32), dev)
    b, h, w, _ = d["depth"].shape
    g = torch.full_like(d["depth"], float("nan"))
    rc = lib.m4d_photo_loss_bwd(dptr(d["depth"]), dptr(warped), dptr(dwarp), dptr(d["cur"]), dptr(mask, "mask", torch.uint8),
                                dptr(out4), dptr(g_out), b, h, w, 1e-3, dptr(g), stream_ptr())
    assert rc == 0
    g, g64 = npy(g)[..., 0].astype(np.float64), g64.numpy()[..., 0]
    assert np.isfinite(g).all()
    err = np.abs(g - g64)[well.numpy()].max() / np.abs(g64).max()
    print(f"{name} automask={automask}: g_depth error {err:.3e} of max |g| (float32 restatement {y['grad']:.3e}, "
          f"bar {4 * y['grad']:.3e}), {well.double().mean().item():.4f} of pixels compared")
    assert well.double().mean().item() >= 0.99
    assert err <= 4 * y["grad"]


def _preds(depths, dev):
    return [[{"depth": to_dev(d, dev).requires_grad_(True)} for d in lv] for lv in depths]


def test_level_photo_and_photometric_loss_end_to_end(dev):
    """_LevelPhoto + photometric_loss, T = 3, 2 levels: loss and every level's depth gradient against float64 autodiff."""
    from m4depth_amd import training as TR
    samples, depths, cam = R.loss_case()
    l64, g64, res = R.loss_and_grads(samples, depths, cam, torch.float64)
    l32, g32, res32 = R.loss_and_grads(samples, depths, cam, torch.float32)
    preds = _preds(depths, dev)
    loss = TR.photometric_loss(to_dev(samples, dev), preds, to_dev(cam, dev), smooth=1e-3, automask=True)
    loss.backward()
    # the yardstick of the sum is that of its parts: the float32 restatement's total can land within 1e-9 of the float64 one by
    # cancellation among the four level terms, closer than a float32 can state it (6e-8), while each term is 1e-7 off
    yard = max([abs(l32.item() - l64.item()) / l64.item()]
               + [abs(res32[k][p].item() - res[k][p].item()) / res[k][p].item() for k in res for p in ("term", "photo", "smooth")])
    err = abs(loss.item() - l64.item()) / l64.item()
    print(f"loss {loss.item()!r} vs {l64.item()!r}: {err:.2e} (float32 restatement {yard:.2e}, bar {4 * yard:.2e})")
    assert err <= 4 * yard
    assert all(p["depth"].grad is None for p in preds[0])              # frame 0 has no term
    for key in sorted(g64):
        t, i = key
        well = R.well_conditioned(res[key]["margins"]).numpy()
        want = g64[key].numpy()[..., 0]
        yard = np.abs(g32[key].double().numpy()[..., 0] - want)[well].max() / np.abs(want).max()
        err = np.abs(npy(preds[t][i]["depth"].grad)[..., 0] - want)[well].max() / np.abs(want).max()
        print(f"frame {t} level {i}: g_depth error {err:.3e} (float32 restatement {yard:.3e}, bar {4 * yard:.3e})")
        assert well.mean() >= 0.99
        assert err <= 4 * yard


def test_nothing_in_view(dev):
    """N = 0: loss = lambda * smooth, mask empty, the gradient finite and the smoothness term's alone."""
    from m4depth_amd import training as TR
    y = R.yardstick("out-of-view")
    r64, g64, well = y["ref"][True]
    d = _dev_case(y["case"], dev)
    depth = d["depth"].clone().requires_grad_(True)
    _, _, valid, out4, mask = _forward(d)
    assert not npy(valid).any() and not npy(mask).any() and r64["n"].item() == 0
    out4 = npy(out4).astype(np.float64)
    assert out4[3] == 0 and out4[1] == 0
    assert abs(out4[2] - r64["smooth"].item()) <= 4 * y["loss"] * r64["smooth"].item()
    assert abs(out4[0] - 1e-3 * r64["smooth"].item()) <= 4 * y["loss"] * 1e-3 * r64["smooth"].item()
    term = TR._LevelPhoto.apply(depth, d["rot"], d["trans"], d["f"], d["c"], d["cur"], d["prev"], 1e-3, True)
    term.backward()
    g = npy(depth.grad)[..., 0].astype(np.float64)
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    err = np.abs(g - g64.numpy()[..., 0])[well.numpy()].max() / g64.abs().max().item()
    print(f"nothing in view: g_depth error {err:.3e} (float32 restatement {y['grad']:.3e})")
    assert err <= 4 * y["grad"]


def test_same_bits_every_run(dev):
    from m4depth_amd import network_ops as nops
    d = _dev_case(R.make_case("24x40-quat"), dev)
    g_out = to_dev(np.array([0.37], np.float32), dev)
    runs = []
    for _ in range(2):
        warped, dwarp, valid, out4, mask = _forward(d)
        g = nops.photo_loss_bwd(d["depth"], warped, dwarp, d["cur"], mask, out4, g_out, 1e-3)
        runs.append([npy(t).copy() for t in (warped, dwarp, out4, g)] + [npy(valid).copy(), npy(mask).copy()])
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()


def test_graphed_photometric_step_follows_eager(dev):
    """GraphedTrainStep(loss="photometric") on a 2-level 64x64 model: the replayed losses follow the eager ones over 4 steps,
    at the bar of test_gpu_train.test_graphed_train_step_equals_eager (rtol 2e-3); default settings (auto-masking on).

    What differs between the two runs is the atomic scatter order of the DSCV backward, 1e-7 of a gradient.  On this model
    (random weights, random textures) the photometric loss is so steep in the weights that a training trajectory amplifies
    such a difference about tenfold per step at Adam's lr 1e-4 .. 1e-3 or SGD's 1e-2: two EAGER runs agree to 1e-6 on the
    first compared step and differ by 1e-3 .. 4e-3 three steps later, with either motion and with auto-masking on or off
    (measured; the supervised loss stays at 1e-6).  That says nothing about the capture.  The comparison therefore runs where
    the trajectory is stable -- plain SGD at lr 1e-3, |1 - lr H| near 1 -- so that what it shows is whether the replay
    computes the eager step: measured 6e-7, 4e-5, 4e-4, 6e-4 on the four steps at worst (two sessions).  The ground truth is all zeros: nothing of
    the step reads it."""
    import m4depth_amd as M
    from m4depth_amd import synthetic, training as TR
    wts = synthetic.init_weights(nbre_levels=2, seed=5, dscv_range=2, sncv_range=2)
    samples, cam = synthetic.make_sequence(2, 3, 64, 64, seed=35)
    data = {k: np.stack([s[k] for s in samples], axis=1) for k in ("RGB_im", "depth", "rot", "trans", "new_traj")}
    data["depth"] = np.zeros_like(data["depth"])
    data["camera"] = cam
    ddata = to_dev(data, dev)
    traj = []
    for graphed in (False, True):
        model = TR.set_trainable(M.M4Depth(depth_type="map", nbre_levels=2, is_training=True, dscv_range=2, sncv_range=2)
                                 .load_numpy_weights(wts, dev))
        model.train_loss = "photometric"
        opt = torch.optim.SGD(model.parameters(), lr=1e-3)
        model.compile(optimizer=opt)
        losses = []
        if graphed:
            runner = TR.GraphedTrainStep(model, ddata, opt, warmup=2, loss="photometric")
            for _ in range(4):
                losses.append(float(runner(ddata)[0]))
        else:
            for i in range(6):
                out = model.train_step(ddata)
                if i >= 2:
                    losses.append(float(out["loss"]))
        traj.append(losses)
    print("eager", traj[0], "graph", traj[1])
    assert all(np.isfinite(traj[0])) and all(np.isfinite(traj[1]))
    assert len(set(traj[0])) == 4 and len(set(traj[1])) == 4           # the weights do move
    np.testing.assert_allclose(traj[1], traj[0], rtol=2e-3)
    with pytest.raises(ValueError):
        TR.train_step(model, ddata, opt, loss="photometric ")


def test_it_learns(dev):
    """A depth map optimised directly (no network) through _LevelPhoto: b = 2, 24x40, a smooth texture warped with a sloped
    plane, start at 1.25 x the true depth (25 % error), Adam lr 0.02 on log depth, 100 steps.  The float64 restatement, run in
    the same test, reaches a median relative error of 0.15 % (p90 0.36 %); the bar is 2 x its median (its plateau wanders
    between 0.13 % and 0.19 %, plus the float32 gradients)."""
    from m4depth_amd import training as TR
    case = R.learn_case()
    t = {k: torch.from_numpy(np.asarray(v)).double() for k, v in case.items() if k != "name"}
    ref = R.optimise(case, lambda dep: R.level_term(dep, t["rot"], t["trans"], t["f"], t["c"], t["cur"], t["prev"])["term"])
    d = _dev_case(case, dev)
    got = R.optimise(case, lambda dep: TR._LevelPhoto.apply(dep, d["rot"], d["trans"], d["f"], d["c"], d["cur"], d["prev"], 1e-3, True),
                     dtype=torch.float32, dev=dev)
    m_ref, p_ref = R.median_error(ref, case["true"])
    m_got, p_got = R.median_error(got, case["true"])
    print(f"median relative depth error: device {m_got:.4%} (p90 {p_got:.4%}), float64 restatement {m_ref:.4%} (p90 {p_ref:.4%}), "
          f"start {R.median_error(case['depth'], case['true'])[0]:.2%}")
    assert m_ref <= 0.01
    assert m_got <= 2 * m_ref


@pytest.mark.parametrize("graph", [False, True])
def test_driver_trains_on_a_recording_without_depth(dev, tmp_path, capsys, graph):
    """--mode=train --dataset=recording --loss=photometric [--graph] on a recording without depth.txt: six steps with finite
    losses, no RMSE_log printed (there is nothing to score against), the summaries without the two ground-truth images; the
    supervised loss refuses the same recording."""
    import re
    from recording_ref import CAMERA_B, write_recording
    from m4depth_amd import main as MAIN
    rec = str(tmp_path / "rec")
    write_recording(rec, CAMERA_B, 12, with_depth=False)
    argv = ["--mode", "train", "--dataset", "recording", "--records_path", rec, "--arch_depth", "2", "--height", "64", "--width", "64",
            "--seq_len", "4", "--db_seq_len", "4", "--epochs", "2", "--ckpt_dir", str(tmp_path / "ck"), "--no_augmentation",
            "--log_dir", str(tmp_path / "log"), "--summary_interval", "2"]
    with pytest.raises(SystemExit):
        MAIN.main(argv)
    assert "needs --loss=photometric" in capsys.readouterr().err
    assert MAIN.main(argv + ["--loss", "photometric"] + (["--graph"] if graph else [])) == 0
    out = capsys.readouterr().out
    losses = [float(v) for v in re.findall(r"step \d+: loss ([0-9.eE+-]+|nan|inf)", out)]
    print("losses", losses)
    assert len(losses) == 6 and all(np.isfinite(losses)) and "RMSE_log" not in out
    blob = b"".join(open(os.path.join(tmp_path / "log", f), "rb").read() for f in os.listdir(tmp_path / "log"))
    assert b"depth_lvl_0" in blob and b"RGB_im" in blob and b"depth_gt" not in blob and b"camera_prev_t_reproj" not in blob
