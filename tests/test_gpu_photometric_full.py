"""The photometric loss's options on the MI355X -- full-resolution terms (U_s, its adjoint), the per-pixel minimum over the
previous and the next frame (csrc/m4d_photo.hip, training._MultiPhoto / photometric_loss(scale=, sources=)) -- against the
torch-CPU restatement tests/photometric_full_ref.py.

Bars.  Nothing is fixed by hand: each bar is 4 x the error of the FLOAT32 restatement to the float64 one on the same case and
over the same well-conditioned pixels (photometric_full_ref.yardstick; tests/test_photometric_full_ref.py asserts the
conditions and records the figures).  The seeds have no auto-mask and no select margin below 1e-5, so the selections must
be equal at every pixel.

Measured on an MI355X, error (float32 restatement's own error; the bar is 4 x that):
  U_s forward:              bit-equal to the float32 restatement at 6x8 s2, 3x5 s16, 1x3 s8, 6x6 s64; to float64 interpolate
                            7.1e-8 / 9.1e-8 / 3.6e-8 / 1.0e-7 of max |x| (the float32 restatement's error exactly)
  U_s^T:                    4.8e-8 (7.0e-8) / 2.6e-8 (9.6e-8) / 4.1e-8 (1.3e-7) / 2.7e-8 (2.2e-7) of max |g|; two runs, same bytes
  pe_id:                    at most 4.7e-8 of max (7.6e-7 .. 1.1e-6), one and two sources
  one source, R.CASES:      sel != 0 == the level loss's mask, N equal; term, photo, smooth at most 6.5e-8 (5.6e-8 .. 1.4e-7)
  two sources, five cases:  sel equal to float64's at every pixel, next frame selected by 47 .. 55 %; term, photo, smooth at
                            most 5.8e-8 (2.7e-8 .. 1.1e-7)
  g_D (raw ABI), of max |g|: 12x16-s2 1.1e-6 (9.5e-7), 24x40-s2 5.6e-6 (5.7e-6), 32x48-s8 3.1e-6 (3.8e-6),
                            48x80-s16 7.0e-6 (7.1e-6), 24x40-level 1.6e-6 (2.2e-6); 99.7 .. 100 % of pixels compared
  next frame out of view:   term and gradient identical to the one-source call (0 difference); to float64 2.0e-6
  end to end, loss:         full/both 1.2e-7 (1.5e-7), full/prev 4.0e-8 (2.1e-7), level/both 4.1e-8 (9.0e-7), level/prev 4.3e-8
  end to end, g_d:          full/both 3.6e-6 .. 6.9e-6 (3.7e-6 .. 7.1e-6), 91.7 % (s = 8) .. 99.4 % (s = 2) of coarse pixels
                            compared; full/prev at most 9.9e-6 (9.4e-6); level/both 3.7e-6 (3.8e-6); level/prev 3.4e-6 (3.4e-6)
  graph vs eager:           the four losses identical (0.442562 0.440972 0.441115 0.441046)
  it learns:                s = 2: 25 % -> 0.755 % median (p90 2.52 %), float64 restatement 0.753 % (2.52 %);
                            s = 4: 0.796 % (1.80 %), float64 restatement 0.812 % (1.81 %)
  driver, full/both:        losses 0.124 0.138 0.113 | 0.096 0.112 0.111 over two epochs of three batches (eager; --graph alike)
"""
import os

import numpy as np
import pytest
import torch

import photometric_full_ref as F
import photometric_ref as R
from helpers import to_dev, npy, assert_bits_equal

pytestmark = pytest.mark.gpu

CASE_NAMES = list(F.CASES)


def _dev_case(case, dev):
    return {k: to_dev(np.asarray(v), dev) for k, v in case.items() if k not in ("name", "s", "true")}


def _forward(case, dev, two=True, automask=True, smooth=1e-3):
    """The launches of training._MultiPhoto's forward, by hand: dict of everything the tests compare."""
    from m4depth_amd import network_ops as nops, training as TR
    d = _dev_case(case, dev)
    D = nops.upsample_hp(d["depth"], case["s"]) if case["s"] > 1 else d["depth"]
    w0, dw0, v0 = nops.photo_warp_fwd(D, d["rot0"], d["trans0"], d["f"], d["c"], d["prev"])
    w1 = dw1 = v1 = None
    if two:
        r1, t1 = TR.motion_inverse(d["rot1"], d["trans1"])
        w1, dw1, v1 = nops.photo_warp_fwd(D, r1, t1, d["f"], d["c"], d["next"])
    pe_id = nops.photo_identity(d["cur"], d["prev"], d["next"] if two else None) if automask else None
    out4, sel = nops.photo_min_fwd(D, w0, v0, w1, v1, d["cur"], pe_id, smooth)
    return {"d": d, "D": D, "w": (w0, w1), "dw": (dw0, dw1), "v": (v0, v1), "pe_id": pe_id, "out4": out4, "sel": sel}


def _term(case, dev, depth, two=True, automask=True, smooth=1e-3, identity_of_both=False):
    """training._MultiPhoto on a case; ``depth`` is the leaf.  ``identity_of_both``: a one-source call whose auto-mask still
    compares against the identity error of both frames (the two-source call's input)."""
    from m4depth_amd import network_ops as nops, training as TR
    d = _dev_case(case, dev)
    r1 = t1 = nxt = None
    if two:
        (r1, t1), nxt = TR.motion_inverse(d["rot1"], d["trans1"]), d["next"]
    pe_id = nops.photo_identity(d["cur"], d["prev"], d["next"] if identity_of_both else nxt) if automask else None
    return TR._MultiPhoto.apply(depth, d["rot0"], d["trans0"], r1, t1, d["f"], d["c"], d["cur"], d["prev"], nxt, pe_id, case["s"], smooth)


def _up_inputs(h, w, s):
    rng = np.random.default_rng(h * 100 + w + s)
    x = rng.uniform(4.0, 12.0, [2, h, w, 1]).astype(np.float32)
    g = rng.normal(0.0, 1.0, [2, h * s, w * s, 1]).astype(np.float32)
    return x, g


@pytest.mark.parametrize("h,w,s", F.UPSAMPLE_SHAPES)
def test_upsample_forward(dev, h, w, s):
    from m4depth_amd import network_ops as nops
    x, _ = _up_inputs(h, w, s)
    got = npy(nops.upsample_hp(to_dev(x, dev), s))
    want32 = F.upsample_hp(torch.from_numpy(x), s).numpy()
    assert got.shape == (2, h * s, w * s, 1)
    assert_bits_equal(got, want32, f"U_{s} of {h}x{w} vs the float32 restatement")
    x64 = torch.from_numpy(x).double().permute(0, 3, 1, 2)
    want64 = torch.nn.functional.interpolate(x64, scale_factor=s, mode="bilinear", align_corners=False).permute(0, 2, 3, 1).numpy()
    scale = np.abs(want64).max()
    yard = np.abs(want32 - want64).max() / scale
    err = np.abs(got - want64).max() / scale
    print(f"U_{s} {h}x{w}: error {err:.2e} of max |x| to float64 interpolate (float32 restatement {yard:.2e}, bar {4 * yard:.2e})")
    assert err <= 4 * yard


@pytest.mark.parametrize("h,w,s", F.UPSAMPLE_SHAPES)
def test_upsample_backward(dev, h, w, s):
    from m4depth_amd import network_ops as nops
    x, g = _up_inputs(h, w, s)
    grads = {}
    for dt in (torch.float64, torch.float32):
        xr = torch.from_numpy(x).to(dt).requires_grad_(True)
        grads[dt] = torch.autograd.grad((F.upsample_hp(xr, s) * torch.from_numpy(g).to(dt)).sum(), xr)[0].double().numpy()
    runs = [npy(nops.upsample_hp_bwd(to_dev(g, dev), s)).copy() for _ in range(2)]
    assert runs[0].tobytes() == runs[1].tobytes()
    scale = np.abs(grads[torch.float64]).max()
    yard = np.abs(grads[torch.float32] - grads[torch.float64]).max() / scale
    err = np.abs(runs[0] - grads[torch.float64]).max() / scale
    print(f"U_{s}^T {h}x{w}: error {err:.2e} of max |g| to float64 autodiff (float32 restatement {yard:.2e}, bar {4 * yard:.2e})")
    assert err <= 4 * yard


def test_upsample_refused_arguments(dev):
    from m4depth_amd._lib import lib, dptr, stream_ptr
    from m4depth_amd import network_ops as nops
    x, out = to_dev(np.zeros([2, 6, 8, 1], np.float32), dev), to_dev(np.zeros([2, 768, 1024, 1], np.float32), dev)
    for fn in (lib.m4d_upsample_hp_fwd, lib.m4d_upsample_hp_bwd):
        for b, h, w, s in ((2, 6, 8, 3), (2, 6, 8, 128), (2, 0, 8, 2), (2, 6, 0, 2), (0, 6, 8, 2), (1 << 10, 64, 64, 4), (2, 6, 8, 1)):
            assert fn(dptr(x), b, h, w, s, dptr(out), stream_ptr()) == 1, (b, h, w, s)
    with pytest.raises(ValueError):
        nops.upsample_hp(x, 3)
    with pytest.raises(ValueError):
        nops.upsample_hp_bwd(out, 128)


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("name", ["12x16-s2", "24x40-s2", "48x80-s16"])
def test_photo_identity(dev, name, two):
    from m4depth_amd import network_ops as nops
    case = F.make_case(name)
    d = _dev_case(case, dev)
    got = npy(nops.photo_identity(d["cur"], d["prev"], d["next"] if two else None)).astype(np.float64)
    refs = {}
    for dt in (torch.float64, torch.float32):
        t = F.case_tensors(case, dt)
        e = R.photo_error(t["prev"], t["cur"])
        refs[dt] = (torch.minimum(e, R.photo_error(t["next"], t["cur"])) if two else e).double().numpy()
    scale = np.abs(refs[torch.float64]).max()
    yard = np.abs(refs[torch.float32] - refs[torch.float64]).max() / scale
    err = np.abs(got[:, 1:-1, 1:-1] - refs[torch.float64]).max() / scale
    print(f"{name} sources={1 + two}: pe_id error {err:.2e} of max (float32 restatement {yard:.2e}, bar {4 * yard:.2e})")
    assert err <= 4 * yard
    border = got.copy()
    border[:, 1:-1, 1:-1] = 0
    assert not border.any()


@pytest.mark.parametrize("automask", [True, False])
@pytest.mark.parametrize("name", list(R.CASES))
def test_min_forward_one_source_is_the_level_loss(dev, name, automask):
    """One source on photometric_ref's cases: the selection is m4d_photo_loss_fwd's mask and N its N, bit for bit."""
    from m4depth_amd import network_ops as nops
    y = R.yardstick(name)
    r64, _, _ = y["ref"][automask]
    d = {k: to_dev(np.asarray(v), dev) for k, v in y["case"].items() if k != "name"}
    warped, _, valid = nops.photo_warp_fwd(d["depth"], d["rot"], d["trans"], d["f"], d["c"], d["prev"])
    old4, mask = nops.photo_loss_fwd(d["depth"], warped, valid, d["cur"], d["prev"], 1e-3, automask)
    pe_id = nops.photo_identity(d["cur"], d["prev"]) if automask else None
    out4, sel = nops.photo_min_fwd(d["depth"], warped, valid, None, None, d["cur"], pe_id, 1e-3)
    assert npy(sel).max() <= 1
    assert np.array_equal(npy(sel) != 0, npy(mask) != 0)
    out4, old4 = npy(out4).astype(np.float64), npy(old4).astype(np.float64)
    assert out4[3] == old4[3] == r64["n"].item()
    errs = {k: abs(out4[i] - r64[k].item()) / abs(r64[k].item()) for i, k in enumerate(("term", "photo", "smooth"))}
    print(f"{name} automask={automask}: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items())
          + f" (float32 restatement {y['loss']:.2e}, bar {4 * y['loss']:.2e}); N {out4[3]:.0f}")
    for k, e in errs.items():
        assert e <= 4 * y["loss"], (k, e)


@pytest.mark.parametrize("automask", [True, False])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_min_forward_two_sources(dev, name, automask):
    y = F.yardstick(name)
    r64 = y["ref"][automask][0]
    fw = _forward(y["case"], dev, True, automask)
    sel = npy(fw["sel"])[..., 0]
    assert np.array_equal(sel, r64["sel"].numpy()), "sel differs from the float64 restatement's"
    for k in (0, 1):
        assert np.array_equal(npy(fw["v"][k])[..., 0].astype(bool), r64["valid"][k].numpy())
    out4 = npy(fw["out4"]).astype(np.float64)
    errs = {k: abs(out4[i] - r64[k].item()) / abs(r64[k].item()) for i, k in enumerate(("term", "photo", "smooth"))}
    print(f"{name} automask={automask}: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items())
          + f" (float32 restatement {y['loss']:.2e}, bar {4 * y['loss']:.2e}); N {out4[3]:.0f}, next {np.mean(sel[sel > 0] == 2):.0%}")
    assert out4[3] == r64["n"].item() and (sel == 1).any() and (sel == 2).any()
    for k, e in errs.items():
        assert e <= 4 * y["loss"], (k, e)


@pytest.mark.parametrize("automask", [True, False])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_min_backward_raw_abi_with_reference_sel(dev, name, automask):
    """m4d_photo_min_bwd through the C ABI, fed the REFERENCE's sel and (term, photo, smooth, N): g_D at the resolution of D."""
    from m4depth_amd._lib import lib, dptr, stream_ptr
    y = F.yardstick(name)
    r64, _, gD64, _, well = y["ref"][automask]
    fw = _forward(y["case"], dev, True, automask)
    sel = to_dev(r64["sel"].numpy()[..., None], dev)
    out4 = to_dev(np.array([r64[k].item() for k in ("term", "photo", "smooth", "n")], np.float32), dev)
    g_out = to_dev(np.array([1.0], np.float32), dev)
    b, h, w, _ = fw["D"].shape
    g = torch.full_like(fw["D"], float("nan"))
    rc = lib.m4d_photo_min_bwd(dptr(fw["D"]), dptr(fw["w"][0]), dptr(fw["dw"][0]), dptr(fw["w"][1]), dptr(fw["dw"][1]), dptr(fw["d"]["cur"]),
                               dptr(sel, "sel", torch.uint8), dptr(out4), dptr(g_out), b, h, w, 1e-3, dptr(g), stream_ptr())
    assert rc == 0
    g, gD64 = npy(g)[..., 0].astype(np.float64), gD64.numpy()[..., 0]
    assert np.isfinite(g).all()
    err = np.abs(g - gD64)[well.numpy()].max() / np.abs(gD64).max()
    print(f"{name} automask={automask}: g_D error {err:.3e} of max |g| (float32 restatement {y['grad_D']:.3e}, "
          f"bar {4 * y['grad_D']:.3e}), {well.double().mean().item():.4f} of pixels compared")
    assert well.double().mean().item() >= 0.99
    assert err <= 4 * y["grad_D"]


def test_one_source_out_of_view(dev):
    """The next frame out of view everywhere: no pixel selects it, term and gradient are those of the one-source call on the
    same inputs (with auto-masking the identity error is an input: the minimum over both frames, which does not depend on
    the depth); both out of view: N = 0, the loss is lambda * smooth, the gradient finite."""
    case = F.out_of_view(F.make_case("24x40-s2"), "next")
    y = F.yardstick_of(case)
    for automask in (False, True):
        fw = _forward(case, dev, True, automask)
        assert not (npy(fw["sel"]) == 2).any() and not npy(fw["v"][1]).any() and (npy(fw["sel"]) == 1).any()
        out = {}
        for two in (True, False):
            depth = to_dev(case["depth"], dev).requires_grad_(True)
            term = _term(case, dev, depth, two=two, automask=automask, identity_of_both=True)
            term.backward()
            out[two] = (term.item(), npy(depth.grad).astype(np.float64))
        d_term = abs(out[True][0] - out[False][0]) / abs(out[False][0])
        d_grad = np.abs(out[True][1] - out[False][1]).max() / np.abs(out[False][1]).max()
        r64, g64, _, cw, _ = y["ref"][automask]
        assert not (r64["sel"] == 2).any()
        err = np.abs(out[True][1] - g64.numpy())[..., 0][cw.numpy()].max() / g64.abs().max().item()
        print(f"next out of view, automask={automask}: term differs by {d_term:.2e} (bar {4 * y['loss']:.2e}), gradient by {d_grad:.2e} "
              f"(bar {4 * y['grad']:.2e}) from the one-source call; to float64 {err:.2e}")
        assert d_term <= 4 * y["loss"] and d_grad <= 4 * y["grad"] and err <= 4 * y["grad"]
    case = F.out_of_view(F.make_case("24x40-s2"), "both")
    r64 = F.term_and_grad(case, torch.float64)[0]
    depth = to_dev(case["depth"], dev).requires_grad_(True)
    fw = _forward(case, dev, True, True)
    out4 = npy(fw["out4"]).astype(np.float64)
    assert not npy(fw["sel"]).any() and out4[3] == 0 and out4[1] == 0 and r64["n"].item() == 0
    assert abs(out4[0] - 1e-3 * r64["smooth"].item()) <= 1e-6 * 1e-3 * r64["smooth"].item()
    _term(case, dev, depth).backward()
    g = npy(depth.grad)
    assert np.isfinite(g).all() and np.abs(g).max() > 0


def test_hostile_coarse_depths_at_scale_full(dev):
    """Coarse depths outside [0.01, 200], negative, zero and infinite, upsampled by 8 (the infinities spread NaN over their
    stencils): validity, selection and N are the float32 restatement's; loss and g_d finite."""
    case = F.hostile_case()
    r32 = F.term_and_grad_free(case, torch.float32)
    fw = _forward(case, dev, True, True)
    D = npy(fw["D"])
    assert np.array_equal(np.isnan(D), np.isnan(r32["D"].numpy())) and not np.isfinite(D).all()
    for k in (0, 1):
        valid = npy(fw["v"][k])[..., 0].astype(bool)
        assert np.array_equal(valid, r32["valid"][k].numpy()), k
        assert valid.any() and not valid.all()
    assert np.array_equal(npy(fw["sel"])[..., 0], r32["sel"].numpy())
    out4 = npy(fw["out4"])
    assert out4[3] == r32["n"].item() > 0 and np.isfinite(out4).all()
    depth = to_dev(case["depth"], dev).requires_grad_(True)
    term = _term(case, dev, depth)
    term.backward()
    assert np.isfinite(term.item()) and np.isfinite(npy(depth.grad)).all() and np.abs(npy(depth.grad)).max() > 0


def _preds(depths, dev):
    return [[{"depth": to_dev(d, dev).requires_grad_(True)} for d in lv] for lv in depths]


@pytest.mark.parametrize("scale,sources", list(F.LOSS_CASES))
def test_photometric_loss_end_to_end(dev, scale, sources):
    """photometric_loss(scale=, sources=), T = 3, 48x80, b = 2 (full/both: 3 levels, maps 24x40, 12x20, 6x10; the others 2):
    the loss and every level's depth gradient against float64 autodiff.  Frame 1 has both neighbours, frame 2 the previous one."""
    from m4depth_amd import training as TR
    samples, depths, cam = F.loss_case(scale, sources)
    l64, g64, res = F.loss_and_grads(samples, depths, cam, torch.float64, scale=scale, sources=sources)
    l32, g32, res32 = F.loss_and_grads(samples, depths, cam, torch.float32, scale=scale, sources=sources)
    preds = _preds(depths, dev)
    loss = TR.photometric_loss(to_dev(samples, dev), preds, to_dev(cam, dev), smooth=1e-3, automask=True, scale=scale, sources=sources)
    loss.backward()
    # the yardstick of the sum is that of its parts (test_gpu_photometric.py gives the reason)
    yard = max([abs(l32.item() - l64.item()) / l64.item()]
               + [abs(res32[k][p].item() - res[k][p].item()) / res[k][p].item() for k in res for p in ("term", "photo", "smooth")])
    err = abs(loss.item() - l64.item()) / l64.item()
    print(f"{scale}/{sources}: loss {loss.item()!r} vs {l64.item()!r}: {err:.2e} (float32 restatement {yard:.2e}, bar {4 * yard:.2e})")
    assert err <= 4 * yard
    assert all(p["depth"].grad is None for p in preds[0])              # frame 0 has no term
    for key in sorted(g64):
        t, i = key
        assert (res[key]["sel"] == 2).any().item() == (sources == "both" and t == 1)
        s = 2 ** (i + 1) if scale == "full" else 1
        well = F.coarse_well(F.well_conditioned(res[key]["margins"]), s).numpy()
        want = g64[key].numpy()[..., 0]
        yard = np.abs(g32[key].double().numpy()[..., 0] - want)[well].max() / np.abs(want).max()
        err = np.abs(npy(preds[t][i]["depth"].grad)[..., 0] - want)[well].max() / np.abs(want).max()
        print(f"{scale}/{sources} frame {t} level {i}: g_depth error {err:.3e} (float32 restatement {yard:.3e}, bar {4 * yard:.3e}), "
              f"{well.mean():.3f} of pixels compared")
        assert well.mean() >= 0.9
        assert err <= 4 * yard


def test_both_sources_refuse_small_angle_rotations(dev):
    from m4depth_amd import training as TR
    samples, depths, cam = R.loss_case()                               # 3-component rotations
    with pytest.raises(ValueError, match="quaternion"):
        TR.photometric_loss(to_dev(samples, dev), _preds(depths, dev), to_dev(cam, dev), sources="both")
    with pytest.raises(ValueError, match="scale: expected one of"):
        TR.photometric_loss(to_dev(samples, dev), _preds(depths, dev), to_dev(cam, dev), scale="half")


def test_graphed_full_both_step_follows_eager(dev):
    """test_gpu_photometric.test_graphed_photometric_step_follows_eager with scale full and both sources: 2-level 64x64 model,
    T = 3, SGD lr 1e-3 (that test gives the reason for the optimiser; it holds here too), 4 steps, rtol 2e-3."""
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
        model.photo_scale, model.photo_sources = "full", "both"
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


@pytest.mark.parametrize("s", [2, 4])
def test_it_learns(dev, s):
    """A coarse depth map optimised directly through _MultiPhoto at scale full with both sources: a textured 3-D plane rendered
    analytically into the previous, current and next camera (b = 2, 48x80), start 25 % off, Adam lr 0.02 on log depth, 100
    steps.  The float64 restatement, run in the same test, must reach 2 % median relative error; the device run 2 x its median."""
    case = F.learn_scene(s)
    t = F.case_tensors(case, torch.float64)
    ref = R.optimise(case, lambda dep: F.multi_term(dep, s, t["rot0"], t["trans0"], t["f"], t["c"], t["cur"], t["prev"], src1=t["next"],
                                                    rot1=t["rot1"], trans1=t["trans1"])["term"])
    got = R.optimise(case, lambda dep: _term(case, dev, dep), dtype=torch.float32, dev=dev)
    m_ref, p_ref = R.median_error(ref, case["true"])
    m_got, p_got = R.median_error(got, case["true"])
    print(f"s={s}: median relative depth error: device {m_got:.4%} (p90 {p_got:.4%}), float64 restatement {m_ref:.4%} (p90 {p_ref:.4%}), "
          f"start {R.median_error(case['depth'], case['true'])[0]:.2%}")
    assert m_ref <= 0.02
    assert m_got <= 2 * m_ref


@pytest.mark.parametrize("graph", [False, True])
def test_driver_trains_full_both_on_a_recording_without_depth(dev, tmp_path, capsys, graph):
    """--mode=train --dataset=recording --loss=photometric --photo_scale full --photo_sources both [--graph] on a recording
    without depth.txt: six steps with finite losses, exit status 0."""
    import re
    from recording_ref import CAMERA_B, write_recording
    from m4depth_amd import main as MAIN
    rec = str(tmp_path / "rec")
    write_recording(rec, CAMERA_B, 12, with_depth=False)
    argv = ["--mode", "train", "--dataset", "recording", "--records_path", rec, "--arch_depth", "2", "--height", "64", "--width", "64",
            "--seq_len", "4", "--db_seq_len", "4", "--epochs", "2", "--ckpt_dir", str(tmp_path / "ck"), "--no_augmentation",
            "--loss", "photometric", "--photo_scale", "full", "--photo_sources", "both"]
    assert MAIN.main(argv + (["--graph"] if graph else [])) == 0
    out = capsys.readouterr().out
    losses = [float(v) for v in re.findall(r"step \d+: loss ([0-9.eE+-]+|nan|inf)", out)]
    print("losses", losses)
    assert len(losses) == 6 and all(np.isfinite(losses))
