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
