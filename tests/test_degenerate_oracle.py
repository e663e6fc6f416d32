"""CPU side of DESIGN.md "Degenerate inputs": the rules R1 / R2 as the oracle states them, and the guard that keeps every case
of tests/degenerate_cases.py on its edge -- recomputed from ``O.motion_factors`` and the inputs, so a change of the table, of
``helpers.camera_np`` or of the sweep that moves a case off the degenerate point names the case instead of letting the GPU
tests (tests/test_gpu_degenerate.py) pass on healthy data."""
import numpy as np
import pytest

from oracle import m4depth_oracle as O
from helpers import F, assert_bits_equal
import degenerate_cases as D

CASES = pytest.mark.parametrize("case", D.CASES, ids=D.case_id)


def _s_zero(d):
    m = O.motion_factors(D.B, d["h"], d["w"], d["rot"], d["trans"], d["cam"])
    return (m["sqrt"] == 0).reshape(D.B, -1).sum(axis=1)


# ------------------------------------------------------------------------------------------------ the rules
def test_r1_nan_query_gives_index_0_weight_0_and_inf_clamps():
    rng = np.random.default_rng(1)
    grid = rng.standard_normal([1, 5, 7, 3]).astype(F)
    nan, inf = F(np.nan), F(np.inf)
    q = np.array([[[nan, nan], [nan, 2.25], [1.5, nan], [inf, -inf], [-inf, inf], [3e38, -3e38], [1.5, 2.25]]], F)
    with np.errstate(invalid="ignore"):
        out, y0, x0 = O.interpolate_bilinear(grid, q, return_index=True)
    assert y0.dtype == np.int32 and x0.dtype == np.int32
    assert y0[0].tolist() == [0, 0, 1, 3, 0, 3, 1] and x0[0].tolist() == [0, 2, 0, 0, 5, 0, 2]
    assert np.isfinite(out).all()
    assert_bits_equal(out[0, 0], grid[0, 0, 0], "NaN query: weight 0 on both axes")                       # 0 * (r - l) + l == l
    top = F(0.25) * (grid[0, 0, 3] - grid[0, 0, 2]) + grid[0, 0, 2]
    assert_bits_equal(out[0, 1], top, "NaN row: row 0, weight 0; the column axis is untouched")
    one = F(1.0)
    bot = F(0.0) * (grid[0, 4, 1] - grid[0, 4, 0]) + grid[0, 4, 0]
    top = F(0.0) * (grid[0, 3, 1] - grid[0, 3, 0]) + grid[0, 3, 0]
    assert_bits_equal(out[0, 3], one * (bot - top) + top, "+Inf row / -Inf column: index size-2 / 0, weight 1 / 0")
    assert_bits_equal(out[0, 5], out[0, 3], "a finite query beyond the map clamps like the infinite one")


def test_r2_parallax_clamp_drops_nan_to_its_lower_bound():
    """clip(disp + n, 1e-6, 1e6) of a NaN parallax is 1e-6: the sweep of that pixel is the sweep of any parallax below the
    range.  (R2's second clamp, the level tail, is checked through ``O.M4Depth`` below.)"""
    case = D.Case("zero_cut", "13x21")
    d = D.make(case)
    c1, c2 = O.normalize_cuts(d["f1"], d["k"]), O.normalize_cuts(d["f2"], d["k"])
    dpt = O.prev_d2para(d["depth_prev_t"], d["rot"], d["trans"], d["cam"])
    a, b_ = d["disp"].copy(), d["disp"].copy()
    a[0, 4, 5, 0], b_[0, 4, 5, 0] = np.nan, -100.0
    with np.errstate(invalid="ignore"):
        ra = O.get_parallax_sweeping_cv(c1, c2, dpt, a, d["rot"], d["trans"], d["cam"], 4, d["k"], return_index=True)
        rb = O.get_parallax_sweeping_cv(c1, c2, dpt, b_, d["rot"], d["trans"], d["cam"], 4, d["k"], return_index=True)
    assert_bits_equal(ra[0], rb[0], "cv")
    assert_bits_equal(ra[1], rb[1], "prev_disp")
    assert np.array_equal(ra[2], rb[2]) and np.array_equal(ra[3], rb[3])


def test_the_nan_propagating_clamp_leaves_the_floor_undefined():
    """Why the rules exist: with maximum / minimum (the NaN-propagating pair the oracle used before) the floor of a 0/0 query is
    NaN, and its int32 cast -- the gather index -- is whatever the platform makes of it."""
    for case in (D.Case("stationary", "13x21"), D.Case("epipole", "13x21")):
        q = D.reference(case)["queries"]
        assert np.isnan(q).any(), case
        with np.errstate(invalid="ignore"):
            fl = np.minimum(np.maximum(F(0.0), np.floor(q[..., 0])), F(D.GEOMS[case.geom].h - 2))
        assert np.isnan(fl).any(), case
        idx = D.reference(case)["idx"]
        assert (idx[np.isnan(q)] == 0).all(), f"{case}: R1 -- NaN query, floor index 0"


# ------------------------------------------------------------------------------------------------ the guards
@CASES
def test_case_sits_on_its_edge(case):
    r = D.reference(case)
    d = r["inputs"]
    h, w, k, C = d["h"], d["w"], d["k"], d["C"]
    for name in ("f1", "f2", "disp", "depth_prev_t", "rot", "trans"):
        assert np.isfinite(d[name]).all(), f"{case}: input {name} must be finite"
    s0 = _s_zero(d)
    q = r["queries"]
    if case.kind == "stationary":
        assert s0.tolist() == [h * w, 0], f"{case}: s == 0 on {s0} pixels"
        assert np.isnan(q[0]).all() and np.isfinite(q[1]).all()
    elif case.kind == "epipole":
        assert s0.tolist() == [1, 1], f"{case}: s == 0 on {s0} pixels per image"
        assert np.isnan(q[:, h // 2, w // 2]).all() and int(np.isnan(q).sum()) == 2 * 2 * (2 * D.DSCV_RANGE + 1)
    else:
        want = [0, h * w] if case.kind == "far_query" else [0, 0]
        assert s0.tolist() == want, f"{case}: s == 0 on {s0} pixels"
    nan1, nan2 = np.isnan(r["c1"]), np.isnan(r["c2"])
    if case.kind == "zero_cut":
        nc = C // k
        ((j1, i1), k1), ((j2, i2), k2) = D.zero_plant(h, w, k)
        want1, want2 = np.zeros_like(nan1), np.zeros_like(nan2)
        want1[0, j1, i1, k1 * nc:(k1 + 1) * nc] = True
        want2[0, j2:j2 + 2, i2:i2 + 3, k2 * nc:(k2 + 1) * nc] = True
        want2[1, 0, 0, :] = True
        assert np.array_equal(nan1, want1) and np.array_equal(nan2, want2), f"{case}: NaN features off the planted cuts"
        assert np.isnan(r["cv_fp32_round"]).any() and np.isnan(r["sncv_auto"]).any() and np.isnan(r["sncv"]).any()
    else:
        assert not nan1.any() and not nan2.any()
    if case.kind == "far_query":
        fin = np.isfinite(q)
        assert np.abs(q[fin]).max() > 1e6 and np.isposinf(q).any() and np.isneginf(q).any(), f"{case}: no far / infinite query"
        hyp = d["disp"] + np.arange(-D.DSCV_RANGE, D.DSCV_RANGE + 1, dtype=F)
        for px_hyp in (hyp[0][(hyp[0] <= 1e-6).any(-1)], hyp[0][(hyp[0] >= 1e6).any(-1)]):
            assert len(px_hyp) >= 2, f"{case}: a clamp of the hypothesis parallax is not reached"
        assert ((hyp <= 1e-6).any(-1) & ~(hyp <= 1e-6).all(-1)).any() and ((hyp >= 1e6).any(-1) & ~(hyp >= 1e6).all(-1)).any(), \
            f"{case}: no pixel whose sweep crosses a clamp"
        assert set(np.unique(r["idx"][1, ..., 0])) <= {0, h - 2} and set(np.unique(r["idx"][1, ..., 1])) <= {0, w - 2}
    if case.kind == "prev_d2para":
        planted = np.zeros([D.B, h, w], bool)
        for (j, i) in D.d2para_plant(h, w):
            planted[:, j, i] = True
            assert (d["depth_prev_t"][:, j, i, 0] == d["trans"][:, 2]).all()
        assert np.array_equal(np.isinf(r["pd2p"][..., 0]), planted), f"{case}: prev_d2para is infinite off the planted pixels"
    else:
        assert np.isfinite(r["pd2p"]).all()


@CASES
def test_the_oracle_stays_finite_enough_to_compare(case):
    """At least 90 % of every output compared bit for bit is finite in the oracle: a comparison of NaN masks alone would say
    little."""
    r = D.reference(case)
    for name in D.PARITY_OUTPUTS:
        frac = float(np.isfinite(r[name]).mean())
        assert frac >= 0.9, f"{case}: {name} is {100 * frac:.1f} % finite"
    if case.kind in ("stationary", "far_query"):
        for name in ("cv_fp32_round", "cv_fp16_seq", "prev_disp"):
            assert np.isfinite(r[name]).all(), f"{case}: {name}"


def test_the_table_covers_every_kind_and_geometry():
    assert {c.kind for c in D.CASES} == set(D.KINDS) and {c.geom for c in D.CASES} == set(D.GEOMS)
    for kind in ("stationary", "far_query"):                     # the two kinds that move every gather of a sample
        assert {c.geom for c in D.CASES if c.kind == kind} >= {"13x21", "12x20", "37x45", "6x20", "20x44"}
    assert [D.GEOMS[g][:4] for g in ("37x45", "21x19", "6x20")] == [(37, 45, 16, 1), (21, 19, 96, 4), (6, 20, 192, 8)]
    assert D.GEOMS["20x44"].t_scale == 40.0


def test_even_map_has_no_epipole_pixel():
    """12 x 20 under helpers.camera_np: the principal point lies between four pixels, forward motion leaves s > 0 everywhere."""
    d = D.make(D.Case("stationary", "12x20"))
    d["rot"] = np.tile(np.array([[1.0, 0.0, 0.0, 0.0]], F), [D.B, 1])
    d["trans"] = np.array([[0.0, 0.0, 0.3], [0.0, 0.0, -0.45]], F)
    assert _s_zero(d).tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ recovery (R2, level tail)
def test_oracle_model_recovers_one_frame_after_motion_resumes():
    """``O.M4Depth`` over reset, healthy, stationary, healthy ...: on the stationary frame the refiner input holds log(0) = -inf,
    the refiner output is NaN and the level tail's clamp (R2) turns it into parallax exp(-7) / scale, so depth and depth state
    stay finite (only "other" is NaN); K = 1: the first frame after motion resumes is wholly finite again."""
    weights, samples, cam = D.model_sequence(1, 6)
    samples = D.make_stationary(samples, D.STATIONARY_FRAME, [0])
    model = O.M4Depth(weights, D.MODEL_LEVELS)
    finite = []
    with np.errstate(all="ignore"):
        for t, smp in enumerate(samples):
            _, est = model([smp], cam)
            for lvl, e in zip(model.levels, est[-1]):
                assert np.isfinite(e["depth"]).all() and np.isfinite(e["parallax"]).all(), f"frame {t}"
                assert np.isfinite(lvl.depth_prev_t).all() and np.isfinite(lvl.prev_f_maps).all(), f"frame {t}: state"
            finite.append(all(np.isfinite(e["other"]).all() for e in est[-1]))
    assert not finite[D.STATIONARY_FRAME], "the stationary frame was meant to put NaN into the refiner"
    assert D.first_recovered(finite) == D.ORACLE_K == 1


# ------------------------------------------------------------------------------------------------ the backward (R5, R6)
BACKWARD_CASES = pytest.mark.parametrize("case", D.BACKWARD_CASES, ids=D.case_id)

def _masks(a):
    return np.isnan(a), np.isposinf(a), np.isneginf(a)


@BACKWARD_CASES
def test_restatement_forward_masks_equal_the_numpy_oracle(case):
    """The rule-bearing training restatement (oracle/m4depth_oracle_train.py, fmax / fmin clamps) can be evaluated on every
    case, and its forward NaN / +Inf / -Inf masks are the numpy oracle's."""
    r, t = D.reference(case), D.backward_reference(case)
    for name, ref in (("cv", "cv_fp32_round"), ("prev_disp", "prev_disp"), ("sncv_auto", "sncv_auto"), ("sncv", "sncv"), ("c1n", "c1")):
        for kind, a, b in zip(("NaN", "+Inf", "-Inf"), _masks(t[name]), _masks(r[ref])):
            assert np.array_equal(a, b), f"{case}: {kind} mask of {name}: {int(a.sum())} entries vs {int(b.sum())}"


@BACKWARD_CASES
def test_case_sits_on_its_edge_in_the_backward(case):
    """Autodiff of the restatement under R5 / R6 with the case's fixed upstream gradients (``D.backward_upstream``): the pattern
    each kind is in the table for.  Share of FINITE entries, sample 0 / sample 1, in per cent (13x21; the other geometries
    give the same pattern, the zero-cut shares depend on the map size):

      kind          g_c1         g_c2         g_disp_prev_t  g_disp        SNCV g_c1 (c1, c1)  SNCV g_c1 / g_c2 (c1, c2)  normalize g_f1
      stationary    100 / 100    100 / 100    100 / 100      0 / 100       100 / 100           100 / 100, 100 / 100       100 / 100
      epipole       100 / 100    100 / 100    100 / 100      99.6 / 99.6   100 / 100           100 / 100, 100 / 100       100 / 100
      zero_cut      75.3 / 99.3  97.1 / 100   100 / 100      51.3 / 99.6   91.0 / 100          86.8 / 94.1, 91.0 / 100    99.8 / 100
      far_query     100 / 100    100 / 100    100 / 100      100 / 1.5     100 / 100           100 / 100, 100 / 100       100 / 100
      prev_d2para   100 / 100    100 / 100    100 / 100      84.6 / 86.8   100 / 100           100 / 100, 100 / 100       100 / 100

    stationary: 0 * NaN on the way from the (selected-to-zero, R5) query gradient to g_disp (R6) -- every g_disp of sample 0
    is NaN, nothing else is, and the neighbour is wholly finite.  epipole: the same on the one pixel with s = 0.  zero_cut:
    NaN features reach g_c1 (through the warped c2), g_c2 (through c1) and g_disp.  far_query: sample 1's queries are +-Inf,
    delta / (0 / p) = +-Inf meets a zero query gradient; the finite rest is exactly 0 (every hypothesis on a clamp of the
    parallax: R5).  prev_d2para: the warped parallax interpolates Inf, its alpha gradient is Inf - Inf.  clamped_corner
    (backward only): see tests/degenerate_cases.py; g_disp of pixel (0, 0) is exactly 0 beside NaN / Inf alpha gradients."""
    t = D.backward_reference(case)
    d = D.reference(case)["inputs"]
    h, w = d["h"], d["w"]
    fin = {n: np.isfinite(t[n]) for n in D.BACKWARD_TENSORS}
    print(D.case_id(case), {n: [round(100 * float(f[s].mean()), 1) for s in range(D.B)] for n, f in fin.items()})
    g_disp = t["dscv_g_disp"][..., 0]
    if case.kind == "stationary":
        assert np.isnan(g_disp[0]).all(), f"{case}: g_disp of the stationary sample"
        for n in D.BACKWARD_TENSORS:
            assert fin[n][1].all(), f"{case}: {n} of the neighbour sample is not finite"
            assert n == "dscv_g_disp" or fin[n][0].all(), f"{case}: {n} of the stationary sample"
    elif case.kind == "epipole":
        want = np.zeros([D.B, h, w], bool)
        want[:, h // 2, w // 2] = True
        assert np.array_equal(np.isnan(g_disp), want), f"{case}: NaN g_disp off the epipole pixel"
        assert all(fin[n].all() for n in D.BACKWARD_TENSORS if n != "dscv_g_disp")
    elif case.kind == "zero_cut":
        for n in ("dscv_g_disp", "dscv_g_c1", "dscv_g_c2", "sncv_auto_g_c1", "sncv_g_c1", "sncv_g_c2", "norm_g_f1"):
            assert np.isnan(t[n][0]).any(), f"{case}: no NaN in {n} of sample 0"
        assert fin["dscv_g_disp_prev_t"].all()
    elif case.kind == "far_query":
        nan1 = np.isnan(g_disp[1])
        assert nan1.mean() > 0.9, f"{case}: {100 * nan1.mean():.1f} % of sample 1's g_disp is NaN"
        assert (~nan1).any() and (g_disp[1][~nan1] == 0).all(), f"{case}: the finite rest is where every hypothesis is clamped"
        assert fin["dscv_g_disp"][0].all() and (g_disp[0] == 0).any() and (g_disp[0] != 0).any()
        assert all(fin[n].all() for n in D.BACKWARD_TENSORS if n != "dscv_g_disp")
    elif case.kind == "clamped_corner":
        r = D.reference(case)
        q00 = r["queries"][:, 0, 0]                                     # [b, 2r+1, 2]
        assert (q00 < 0).all(), f"{case}: a hypothesis of pixel (0, 0) stays inside the map"
        assert (r["idx"][:, 0, 0] == 0).all() and np.isnan(r["c2"][0, 0, 0]).any() and np.isposinf(r["pd2p"][1, 0, 0, 0])
        assert_bits_equal(np.abs(g_disp[:, 0, 0]), np.zeros(D.B, F), f"{case}: g_disp of pixel (0, 0) is selected to 0 (R5)")
        assert np.isnan(t["dscv_g_c1"][0, 0, 0]).any() and not np.isfinite(t["prev_disp"][1, 0, 0]).all()
        # the same graph with the clamp gradient written as a product with a 0/1 mask is NaN there: the case tells the two apart
        import torch
        from oracle import m4depth_oracle_train as OT

        class ProductClip(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x, lo, hi):
                ctx.save_for_backward(((x >= lo) & (x <= hi)).to(x.dtype))
                return torch.fmin(torch.fmax(x, torch.tensor(lo, dtype=x.dtype)), torch.tensor(hi, dtype=x.dtype))

            @staticmethod
            def backward(ctx, g):
                return g * ctx.saved_tensors[0], None, None

        old_clip = OT._clip
        OT._clip = lambda x, lo, hi: ProductClip.apply(x, float(lo), float(hi))
        try:
            u = D.backward_upstream(case)
            leaves = [torch.from_numpy(np.array(a)).requires_grad_(True) for a in (r["c1"], r["c2"], r["pd2p"], d["disp"])]
            cv, pd = OT.get_parallax_sweeping_cv(*leaves, d["rot"], d["trans"], d["cam"], D.DSCV_RANGE, nbre_cuts=d["k"])
            ((cv * torch.from_numpy(u["g_cv"])).sum() + (pd * torch.from_numpy(u["g_prev_disp"])).sum()).backward()
        finally:
            OT._clip = old_clip
        assert np.isnan(leaves[3].grad.numpy()[:, 0, 0, 0]).all(), f"{case}: a mask-multiplying clamp gradient gives the same answer"
    elif case.kind == "prev_d2para":
        assert np.isinf(t["prev_disp"]).any() and not fin["dscv_g_disp"].all(), f"{case}: the infinite parallax reaches no gradient"
        assert all(fin[n].all() for n in D.BACKWARD_TENSORS if n != "dscv_g_disp")


@BACKWARD_CASES
def test_float32_and_float64_restatements_agree_on_the_non_finite_masks(case):
    """What lets the GPU tests ask for equal masks on 100 % of the entries: the reference's own masks do not depend on its
    precision.  Demanded of every tensor whose graph has no float16 step (``D.NO_HALF_TENSORS``); it also holds for the three
    DSCV gradients behind the float16 product, with one exception that is a property of the forward input, not of the
    gradient: sample 1 of far_query moves by 1e-30, delta^2 underflows to s = 0 in float32 only, so its queries are +-Inf in
    float32 and finite (1e30 pixels away) in float64, and g_disp is NaN against 0."""
    a, b = D.backward_reference(case), D.backward_reference(case, double=True)
    for n in D.BACKWARD_TENSORS:
        if case.kind == "far_query" and n == "dscv_g_disp":
            assert all(np.array_equal(x[0], y[0]) for x, y in zip(_masks(a[n]), _masks(b[n]))), f"{case}: {n}, sample 0"
            continue
        for kind, x, y in zip(("NaN", "+Inf", "-Inf"), _masks(a[n]), _masks(b[n])):
            assert np.array_equal(x, y), f"{case}: {kind} mask of {n}: {int(x.sum())} entries in float32, {int(y.sum())} in float64"


def test_r5_clamp_gradient_is_a_select():
    """R5: outside the bounds, and on a NaN input, the gradient is exactly 0 even when NaN or Inf arrives; inside it is the
    incoming gradient.  Forward: a NaN drops to the lower bound (R1, R2)."""
    import torch
    from oracle import m4depth_oracle_train as OT
    nan, inf = float("nan"), float("inf")
    x = torch.tensor([nan, -inf, -8.0, -7.0, 0.5, 7.0, 8.0, inf], requires_grad=True)
    y = OT._clip(x, -7.0, 7.0)
    assert y.tolist() == [-7.0, -7.0, -7.0, -7.0, 0.5, 7.0, 7.0, 7.0]
    y.backward(torch.tensor([nan, nan, inf, 2.0, nan, 3.0, -inf, nan]))
    g = x.grad.numpy()
    assert_bits_equal(g[[0, 1, 2, 6, 7]], np.zeros(5, F), "outside or NaN: +0")
    assert g[3] == 2.0 and np.isnan(g[4]) and g[5] == 3.0
    q = torch.tensor([nan, inf, -inf, 2.75])
    assert OT._floor_index(q, 7).tolist() == [0.0, 5.0, 0.0, 2.0]
