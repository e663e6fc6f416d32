"""The restatement of the photometric loss's options (tests/photometric_full_ref.py) checked on its own, on the CPU: U_s against
torch's interpolate, its adjoint, the inverse motion, the defaults against photometric_ref.level_term, planted errors, the
conditioning of every case the GPU tests run, and the float32 restatement's error to float64 -- the yardstick the GPU bars are
4 x of.

Figures of the committed restatement (b = 2, per-sample off-centre cameras, random images, coarse depth in [4, 12]; margins
and shares with auto-masking on, errors the largest over both settings):
  case          auto-mask / select margin   N of interior   previous / next   float32 error: loss, g_depth, g_D (of max |g|)
  12x16-s2      3.2e-5 / 1.1e-4             49 %            50 % / 50 %       9.2e-8, 1.3e-6, 9.5e-7
  24x40-s2      1.8e-5 / 1.3e-5             47 %            51 % / 49 %       6.0e-8, 2.9e-6, 5.7e-6
  32x48-s8      2.4e-5 / 3.2e-5             46 %            45 % / 55 %       2.7e-8, 4.6e-6, 3.8e-6
  48x80-s16     2.7e-5 / 2.9e-5             47 %            48 % / 52 %       9.6e-8, 5.3e-6, 7.1e-6
  24x40-level   4.5e-5 / 2.6e-5             45 %            46 % / 54 %       1.1e-7, 2.2e-6, 2.2e-6
At most 0.3 % of pixels lie within 1e-5 of another kink; the selections of the float32 and the float64 restatement are identical.
End-to-end cases (T = 3, 48x80): smallest auto-mask / select margin 1.1e-5 / 1.1e-5 (full/both, 3 levels, seed 19 of 0..19),
2.0e-5 (full/prev, seed 17), 3.3e-5 / 2.0e-5 (level/both), 3.3e-5 (level/prev).  Planted errors on 32x48-s8 move (term, gradient
of max |g|): only_prev 1.1e-1, 0.62; identity_prev_only 4.1e-2, 0.25; next_not_inverted 9.7e-3, 0.56; align_corners 4.7e-3,
0.69; legacy_v1 2.9e-5, 0.94; adjoint_no_clamp 0, 0.97.  The optimisation of the rendered plane reaches 0.75 % (s = 2, p90
2.5 %) and 0.81 % (s = 4, p90 1.8 %) median relative depth error from 25 %.
U_s against interpolate(align_corners=False), float64: at most 3.6e-15 on values up to 12; <U x, g> and <x, U^T g> agree to
1e-16 relative; motion_inverse composed with the motion is the identity to 1.3e-15.
"""
import numpy as np
import pytest
import torch

import photometric_full_ref as F
import photometric_ref as R

CASE_NAMES = list(F.CASES)
# the GPU bars these planted errors are held against (tests/test_gpu_photometric_full.py): a few 1e-7 on the term, 1e-5 of
# max |g| on the gradient
GPU_BAR_TERM, GPU_BAR_GRAD = 5e-7, 1e-5


@pytest.mark.parametrize("h,w,s", F.UPSAMPLE_SHAPES)
def test_upsample_matches_interpolate_and_adjoint(h, w, s):
    rng = np.random.default_rng(h * 100 + w + s)
    x = torch.from_numpy(rng.uniform(4.0, 12.0, [2, h, w, 1]))
    up = F.upsample_hp(x, s)
    want = torch.nn.functional.interpolate(x.permute(0, 3, 1, 2), scale_factor=s, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    err = (up - want).abs().max().item()
    g = torch.from_numpy(rng.normal(0.0, 1.0, list(up.shape)))
    xr = x.clone().requires_grad_(True)
    ut_g, = torch.autograd.grad((F.upsample_hp(xr, s) * g).sum(), xr)
    lhs, rhs = (up * g).sum().item(), (x * ut_g).sum().item()
    print(f"{h}x{w} s={s}: |U - interpolate| {err:.1e}, <Ux,g> {lhs!r} vs <x,U^T g> {rhs!r}")
    assert err <= 1e-12
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
    # the adjoint's weights sum to s^2 per sample: U reproduces constants
    assert torch.allclose(F.upsample_hp(torch.ones_like(x), s), torch.ones_like(up), atol=1e-15)
    # float32: src and a are exact, so the float32 restatement is the float64 one rounded at the three lerps only
    up32 = F.upsample_hp(x.float(), s)
    assert (up32.double() - F.upsample_hp(x.float().double(), s)).abs().max().item() <= 4 * 12.0 * 2.0 ** -24


def test_motion_inverse_composes_to_identity():
    rng = np.random.default_rng(3)
    rot = torch.from_numpy(F._quat(rng.normal(0.0, 0.3, [5, 3])))
    trans = torch.from_numpy(rng.normal(0.0, 1.0, [5, 3]))
    x = torch.from_numpy(rng.normal(0.0, 3.0, [5, 3]))
    ri, ti = F.motion_inverse(rot, trans)
    back = F.apply_motion(ri, ti, F.apply_motion(rot, trans, x))
    forth = F.apply_motion(rot, trans, F.apply_motion(ri, ti, x))
    print(f"inverse o motion - id: {(back - x).abs().max().item():.1e}, motion o inverse - id: {(forth - x).abs().max().item():.1e}")
    assert (back - x).abs().max().item() <= 1e-12 and (forth - x).abs().max().item() <= 1e-12


@pytest.mark.parametrize("name", list(R.CASES))
@pytest.mark.parametrize("automask", [True, False])
def test_defaults_reproduce_level_term(name, automask):
    """scale = level, sources = prev: multi_term IS photometric_ref.level_term -- term, parts, mask and gradient, exactly."""
    case = R.make_case(name)
    for dt in (torch.float64, torch.float32):
        t = {k: torch.from_numpy(np.asarray(v)).to(dt) for k, v in case.items() if k != "name"}
        d1, d2 = t["depth"].clone().requires_grad_(True), t["depth"].clone().requires_grad_(True)
        a = R.level_term(d1, t["rot"], t["trans"], t["f"], t["c"], t["cur"], t["prev"], 1e-3, automask)
        b = F.multi_term(d2, 1, t["rot"], t["trans"], t["f"], t["c"], t["cur"], t["prev"], smooth=1e-3, automask=automask)
        for k in ("term", "photo", "smooth", "n"):
            assert a[k].item() == b[k].item(), k
        assert torch.equal(a["mask"], b["sel"] != 0)
        assert torch.equal(torch.autograd.grad(a["term"], d1)[0], torch.autograd.grad(b["term"], d2)[0])


def _assert_conditioned(res, what, two):
    mg = res["margins"]
    am, se = mg["automask"].min().item(), mg["select"].min().item()
    bad = 1.0 - R.well_conditioned(mg).double().mean().item()
    sel, n = res["sel"], res["n"].item()
    b, H, W = sel.shape
    share = [(sel == k).sum().item() / max(n, 1.0) for k in (1, 2)]
    print(f"{what}: auto-mask margin {am:.1e}, select margin {se:.1e}, {bad:.3%} within {F.MARGIN} of another kink, "
          f"N {n / (b * (H - 2) * (W - 2)):.0%} of the interior, previous / next {share[0]:.0%} / {share[1]:.0%}")
    assert am >= F.MARGIN and se >= F.MARGIN, what
    assert bad <= 0.01, what
    assert n >= 0.25 * b * (H - 2) * (W - 2), what
    if two:
        assert min(share) >= 0.30, what


@pytest.mark.parametrize("name", CASE_NAMES)
def test_gpu_cases_are_well_conditioned(name):
    y = F.yardstick(name)
    for am in (True, False):
        r64 = y["ref"][am][0]
        _assert_conditioned(r64, f"{name} automask={am}", True)
        r32, _, _ = F.term_and_grad(y["case"], torch.float32, automask=am)
        assert torch.equal(r32["sel"], r64["sel"]) and all(torch.equal(a, b) for a, b in zip(r32["valid"], r64["valid"]))
        assert y["ref"][am][4].double().mean().item() >= 0.99
    print(f"{name}: float32 restatement loss error {y['loss']:.2e}, g_depth error {y['grad']:.2e}, g_D error {y['grad_D']:.2e} of max |g|")
    assert 0 < y["loss"] < 1e-5 and 0 < y["grad"] < 1e-5 and 0 < y["grad_D"] < 1e-5


@pytest.mark.parametrize("scale,sources", list(F.LOSS_CASES))
def test_end_to_end_cases_are_well_conditioned(scale, sources):
    samples, depths, cam = F.loss_case(scale, sources)
    _, _, res = F.loss_and_grads(samples, depths, cam, torch.float64, scale=scale, sources=sources)
    L = F.LOSS_CASES[(scale, sources)][0]
    assert sorted(res) == [(t, i) for t in (1, 2) for i in range(L)]
    for (t, i), r in res.items():
        two = sources == "both" and t == 1                        # the last frame has the previous one only
        assert (r["sel"] == 2).any().item() == two
        _assert_conditioned(r, f"{scale}/{sources} frame {t} level {i}", two)


PLANTED = ["only_prev", "identity_prev_only", "next_not_inverted", "align_corners", "legacy_v1", "adjoint_no_clamp"]


@pytest.mark.parametrize("planted", PLANTED)
def test_planted_errors_show(planted):
    """Every planted error moves the term or the gradient by at least 10 x the GPU bar for that quantity, on 32x48-s8."""
    case = F.make_case("32x48-s8")
    r, g, _ = F.term_and_grad(case, torch.float64)
    rb, gb, _ = F.term_and_grad(case, torch.float64, **{planted: True})
    d_term = abs(rb["term"].item() - r["term"].item()) / r["term"].item()
    d_grad = ((gb - g).abs().max() / g.abs().max()).item()
    print(f"{planted}: term moved by {d_term:.2e}, gradient by {d_grad:.2e} of max |g|")
    assert d_term >= 10 * GPU_BAR_TERM or d_grad >= 10 * GPU_BAR_GRAD
    if planted == "adjoint_no_clamp":
        assert d_term == 0.0 and d_grad >= 10 * GPU_BAR_GRAD      # the forward is untouched: only the gradient can show it


def test_one_source_out_of_view_reference():
    """The next frame thrown out of view: no pixel selects it and the term is the one-source term on the same inputs; both out
    of view: N = 0, the loss is lambda * smooth, the gradient finite."""
    case = F.out_of_view(F.make_case("24x40-s2"), "next")
    r2, g2, _ = F.term_and_grad(case, torch.float64, automask=False)
    r1, g1, _ = F.term_and_grad(case, torch.float64, automask=False, two=False)
    assert not (r2["sel"] == 2).any() and not r2["valid"][1].any() and r2["n"].item() > 0
    assert r2["term"].item() == pytest.approx(r1["term"].item(), rel=1e-13) and torch.allclose(g1, g2, rtol=1e-12, atol=0)
    r0, g0, _ = F.term_and_grad(F.out_of_view(F.make_case("24x40-s2"), "both"), torch.float64)
    assert r0["n"].item() == 0 and r0["term"].item() == pytest.approx(1e-3 * r0["smooth"].item(), rel=1e-12)
    assert torch.isfinite(g0).all() and g0.abs().max() > 0


def test_hostile_case_is_decided_alike_in_both_precisions():
    """photometric_full_ref.hostile_case: the infinite coarse depths spread NaN over their stencils; validity, selection and N
    agree between the float32 and the float64 restatement and no decision is within 1e-5 of flipping."""
    case = F.hostile_case()
    r32, r64 = F.term_and_grad_free(case, torch.float32), F.term_and_grad_free(case, torch.float64)
    assert torch.isnan(r64["D"]).any() and torch.equal(torch.isnan(r32["D"]), torch.isnan(r64["D"]))
    assert torch.equal(r32["sel"], r64["sel"]) and all(torch.equal(a, b) for a, b in zip(r32["valid"], r64["valid"]))
    assert r32["n"].item() == r64["n"].item() > 0 and (r64["sel"] == 1).any() and (r64["sel"] == 2).any()
    assert r64["margins"]["automask"].min().item() >= F.MARGIN and r64["margins"]["select"].min().item() >= F.MARGIN
    assert all(v[i].any() and not v[i].all() for v in r64["valid"] for i in (0, 1))


@pytest.mark.parametrize("s", [2, 4])
def test_restatement_learns(s):
    """The optimisation of the GPU test on the float64 restatement: from 25 % to at most 2 % median relative depth error."""
    case = F.learn_scene(s)
    t = F.case_tensors(case, torch.float64)
    fn = lambda dep: F.multi_term(dep, s, t["rot0"], t["trans0"], t["f"], t["c"], t["cur"], t["prev"], src1=t["next"], rot1=t["rot1"],
                                  trans1=t["trans1"])["term"]
    out = R.optimise(case, fn)
    start, (med, p90) = R.median_error(case["depth"], case["true"])[0], R.median_error(out, case["true"])
    print(f"s={s}: median relative depth error {start:.2%} -> {med:.4%} (p90 {p90:.4%})")
    assert start == pytest.approx(0.25, abs=1e-6)
    assert med <= 0.02
