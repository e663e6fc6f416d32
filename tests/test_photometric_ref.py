"""The restatement of the photometric reprojection loss (tests/photometric_ref.py) checked on its own, on the CPU: its
float64 autodiff against central differences, planted errors, the conditioning of every case the GPU tests run, and the
float32 restatement's error to float64 -- the yardstick the GPU bars are 4 x of.

Figures of the committed restatement (b = 2, per-sample off-centre cameras, random images, depth in [4, 12]):
  case            auto-mask margin   M / valid     float32 loss error   float32 g_depth error (of max |g|)
  6x8-quat        8.3e-5             12 % / 73 %   1.0e-7               1.3e-6
  6x8-angle       6.0e-3              9 % / 73 %   6.0e-8               4.6e-7
  13x21-quat      2.5e-4             32 % / 86 %   1.4e-7               1.4e-6
  13x21-angle     6.1e-4             36 % / 84 %   7.1e-8               1.8e-6
  24x40-quat      3.1e-5             37 % / 91 %   8.1e-8               2.4e-6
  24x40-angle     3.4e-5             39 % / 91 %   5.6e-8               2.5e-6
  out-of-view     (N = 0)             0 % /  0 %   1.1e-7               1.2e-7
No case has a pixel within 1e-5 of a local kink; the masks of the float32 and the float64 restatement are identical.  The
errors are the largest over both auto-mask settings and, for the loss, over (term, photo, smooth).  Autodiff against central
differences: 9.7e-8 of max |g|.  Planted errors move the gradient by 5.1 (Px C term), 1.9 (mu term), 0.15 (`valid` ignored)
and 1.2 (sample 0's camera) of max |g|.  The optimisation reaches 0.146 % median relative depth error (p90 0.363 %) from 25 %.
"""
import numpy as np
import pytest
import torch

import photometric_ref as R

CASE_NAMES = list(R.CASES)


def test_autodiff_matches_central_differences():
    """float64, 13x21: d term / d depth(q) by central differences (step 1e-6) at well-conditioned pixels spread over both
    samples, masked and unmasked, against autodiff; the mask is held (it carries no gradient)."""
    case = R.make_case("13x21-quat")
    res, g = R.term_and_grad(case, torch.float64)
    well = R.well_conditioned(res["margins"]) & (res["margins"]["automask"] >= 1e-4)
    idx = np.argwhere(well.numpy())
    idx = idx[np.random.default_rng(0).choice(len(idx), 40, replace=False)]
    t = {k: torch.from_numpy(np.asarray(v)).double() for k, v in case.items() if k != "name"}
    f = lambda dep: R.level_term(dep, t["rot"], t["trans"], t["f"], t["c"], t["cur"], t["prev"], mask=res["mask"])["term"].item()
    scale = g.abs().max().item()
    worst = 0.0
    for bi, y, x in idx:
        hi, lo = t["depth"].clone(), t["depth"].clone()
        hi[bi, y, x, 0] += 1e-6
        lo[bi, y, x, 0] -= 1e-6
        fd = (f(hi) - f(lo)) / 2e-6
        worst = max(worst, abs(fd - g[bi, y, x, 0].item()) / scale)
    print(f"autodiff vs central differences: worst {worst:.2e} of max |g|")
    assert worst < 1e-6


@pytest.mark.parametrize("planted", ["drop_px_c", "drop_mu", "ignore_valid", "camera_of_sample0"])
def test_planted_errors_show(planted):
    """Each planted error moves the gradient by far more than any GPU bar (which are below 2e-5 of max |g|): dropping the
    Px C term of dq/ddc, dropping the mu term of the SSIM derivative, ignoring `valid` in the window test, reading sample 0's
    camera.  The motion has a forward component (the Px C term vanishes for a purely sideways one)."""
    case = R.make_case("24x40-quat")
    case["trans"] = case["trans"] + np.array([[0.0, 0.0, 0.6]], np.float32)
    _, g = R.term_and_grad(case, torch.float64)
    _, bad = R.term_and_grad(case, torch.float64, **{planted: True})
    moved = ((bad - g).abs().max() / g.abs().max()).item()
    print(f"{planted}: gradient moved by {moved:.2e} of max |g|")
    assert moved >= 1e-2


def _assert_conditioned(margins, what):
    am = margins["automask"].min().item()
    bad = 1.0 - R.well_conditioned(margins).double().mean().item()
    print(f"{what}: smallest auto-mask margin {am:.2e}, {bad:.4%} of pixels within {R.MARGIN} of a local kink")
    assert am >= R.MARGIN, what
    assert bad <= 0.01, what


@pytest.mark.parametrize("name", CASE_NAMES)
def test_gpu_cases_are_well_conditioned(name):
    """Conditions on the INPUTS of every GPU case: no auto-mask margin below 1e-5 (so the float64 mask is THE mask), at most
    1 % of pixels with another margin below 1e-5 (what a GPU comparison may leave out); both masks have both branches."""
    y = R.yardstick(name)
    for am in (True, False):
        r64, _, _ = y["ref"][am]
        _assert_conditioned(r64["margins"], f"{name} automask={am}")
        assert 0 < r64["n"].item() < r64["mask"].numel()
        assert 0.5 < r64["valid"].double().mean().item() < 1.0
        r32, _ = R.term_and_grad(y["case"], torch.float32, automask=am)
        assert torch.equal(r32["mask"], r64["mask"]) and torch.equal(r32["valid"], r64["valid"])


def test_end_to_end_case_is_well_conditioned():
    samples, depths, cam = R.loss_case()
    _, _, res = R.loss_and_grads(samples, depths, cam, torch.float64)
    assert sorted(res) == [(1, 0), (1, 1), (2, 0), (2, 1)]
    for key, r in res.items():
        _assert_conditioned(r["margins"], f"frame {key[0]} level {key[1]}")


@pytest.mark.parametrize("name", CASE_NAMES + ["out-of-view"])
def test_float32_restatement_error(name):
    """Records the yardstick: the float32 restatement's error to float64 per case (loss relative, g_depth relative to
    max |g_depth|).  float32 carries 6e-8; anything above 1e-5 would mean the case is badly conditioned after all."""
    y = R.yardstick(name)
    print(f"{name}: float32 restatement loss error {y['loss']:.2e}, g_depth error {y['grad']:.2e} of max |g|")
    assert 0 < y["loss"] < 1e-5 and 0 < y["grad"] < 1e-5


def test_nothing_in_view_reference():
    y = R.yardstick("out-of-view")
    r64, g64, _ = y["ref"][True]
    assert r64["n"].item() == 0 and not r64["valid"].any()
    assert r64["term"].item() == pytest.approx(1e-3 * r64["smooth"].item(), rel=1e-12)
    assert torch.isfinite(g64).all() and g64.abs().max() > 0


def test_pyramid_and_weights():
    img = torch.arange(2 * 8 * 8 * 3, dtype=torch.float32).reshape(2, 8, 8, 3)
    pyr = R.image_pyramid(img, 3)
    assert [tuple(p.shape) for p in pyr] == [(2, 4, 4, 3), (2, 2, 2, 3), (2, 1, 1, 3)]
    assert torch.equal(pyr[0][0, 0, 0], (img[0, 0, 0] + img[0, 0, 1] + img[0, 1, 0] + img[0, 1, 1]) * 0.25)


def test_restatement_learns():
    """The optimisation of the GPU test on the float64 restatement: from 25 % to at most 1 % median relative depth error
    (measured: 0.15 %, p90 0.36 %)."""
    case = R.learn_case()
    t = {k: torch.from_numpy(np.asarray(v)).double() for k, v in case.items() if k != "name"}
    out = R.optimise(case, lambda dep: R.level_term(dep, t["rot"], t["trans"], t["f"], t["c"], t["cur"], t["prev"])["term"])
    start, (med, p90) = R.median_error(case["depth"], case["true"])[0], R.median_error(out, case["true"])
    print(f"median relative depth error {start:.2%} -> {med:.4%} (p90 {p90:.4%})")
    assert start == pytest.approx(0.25, abs=1e-6)
    assert med <= 0.01


def test_stationary_case_is_exact_in_both_precisions():
    """R.stationary_case (a stationary sample beside a moving one): sample 0's queries are the pixel centres exactly, in float32
    and float64 alike, so both agree on ``valid`` (all of sample 0), on the mask without the auto-mask and on N; ``warped`` is
    ``prev`` off the last row / column and within an ulp there; the depth gradient of sample 0 is the smoothness term's alone.
    With the auto-mask, sample 0's mask compares pe(warped, cur) with pe(prev, cur) of the same image: last-bit noise decides,
    and the two precisions need not agree (they do not: N = 58 against 61)."""
    y = R.stationary_yardstick()
    r64, g64, well = y["ref"]
    r32, case = y["r32"], y["case"]
    prev = torch.from_numpy(case["prev"])
    for r in (r32, r64):
        assert bool(r["valid"][0].all()) and not bool(r["valid"][1].all())
        assert torch.equal(r["warped"][0, :-1, :-1].detach().float(), prev[0, :-1, :-1])
        assert float((r["warped"][0].detach().float() - prev[0]).abs().max()) <= 2.0 ** -23
    assert torch.equal(r32["mask"], r64["mask"]) and r32["n"].item() == r64["n"].item() > 11 * 19
    assert bool(r64["mask"][0, 1:-1, 1:-1].all())
    assert float(well.double().mean()) >= 0.99 and bool(well[0].all())
    assert (r64["margins"]["cell"][0] == 0).all()
    assert 0 < float(g64[0].abs().max()) < 0.05 * float(g64[1].abs().max())
    print(f"stationary: float32 restatement's error: loss {y['loss']:.2e}, g_depth {y['grad']:.2e} of max |g|")
    a64, _ = R.term_and_grad(case, torch.float64, automask=True)
    assert a64["n"].item() <= r64["n"].item() and not bool(a64["mask"][0].any())
