"""The reprojection-consistency score's restatement (tests/consistency_ref.py) checked on its own, without a GPU: an exact
scene with closed-form values, the conditioning of the random cases the GPU tests share, planted wiring errors, hostile
inputs."""
import numpy as np
import pytest

import consistency_ref as C

BAR = C.GPU_ULPS * C.ULP32            # the GPU bar as a relative error: 2 float32 ulps are at most 2 * 2^-23 of the value


@pytest.mark.parametrize("k", [1, 2, 3])
def test_exact_scene(k):
    h, w = 12, 20
    case = C.exact_scene(h, w, k)
    r = C.score(case)
    v = r["valid"][0].numpy()
    assert v.sum() == h * (w - k) and v[:, :w - k].all()                     # the query of column i is column i + k
    got, want = r["warped"][0].numpy()[v], case["cur"][0][v]
    assert got.tobytes() == want.tobytes()                                   # bit for bit
    photo, photo_id, better, geo, cover, geo_cover = r["rows"][0]
    assert photo == 0.0 and geo == 0.0 and better == 1.0 and photo_id > 0.0
    assert r["n"][0] == (h - 2) * (w - 2 - k) and r["ng"][0] == h * (w - k)
    assert cover == (w - 2 - k) / (w - 2) and geo_cover == (w - k) / w
    assert C.counted(r).all()


@pytest.mark.parametrize("scale", [0.5, 0.8, 1.25, 2.0])
def test_exact_scene_wrong_depth_costs(scale):
    r = C.score(C.exact_scene(scale=scale))
    assert r["rows"][0, 0] > 0.0 and r["n"][0] > 0


@pytest.mark.parametrize("scale", [0.5, 1.0, 2.0])
def test_forward_motion_closed_form(scale):
    """Forward translation tz, both estimates k z0 (k = ``scale``): Pz = k z0 + tz, Dq = k z0, geo = tz / (2 k z0 + tz)."""
    tz, z0 = 0.5, 8.0
    r = C.score(C.exact_scene(scale=scale, forward=tz))
    assert r["ng"][0] > 0
    assert abs(r["rows"][0, 3] - tz / (2 * scale * z0 + tz)) <= 1e-12


@pytest.mark.parametrize("name", C.RANDOM_CASES + ("exact", "hostile", "out-of-view"))
def test_shared_cases_are_well_conditioned(name):
    """No pixel of M has |pe_w - pe_id| < 1e-9: `better` and every count are then exact on the GPU.  Holds for the seeds of
    every case the GPU tests share."""
    case, r = C.case_and_ref(name)
    for s in range(case["depth"].shape[0]):
        m = r["M"][s]
        if name == "out-of-view" and s == 0:
            continue
        assert r["n"][s] > 0 and r["ng"][s] > 0
        assert float((r["pe_w"][s] - r["pe_id"][s]).abs()[m].min()) >= 1e-9
    assert np.isfinite(r["rows"]).all()


@pytest.mark.parametrize("planted", ["camera_of_sample0", "no_motion", "dp_at_pixel", "halo"])
def test_planted_wiring_errors_show(planted):
    """Each planted error moves at least one row value by more than 100 x the GPU bar, on every case it can show on: the
    halo needs more than one tile, and with sample 0's camera for everyone sample 0's own row stays right."""
    names = [n for n in C.RANDOM_CASES if not (planted == "halo" and n.startswith("6x8"))]
    for name in names:
        case, r = C.case_and_ref(name)
        bad = C.score(case, planted=planted)
        rel = np.abs(bad["rows"] - r["rows"]) / np.abs(r["rows"])
        rows = slice(1, None) if planted == "camera_of_sample0" else slice(None)
        assert (rel[rows].max(axis=1) > 100 * BAR).all(), (name, planted, rel)


def test_hostile_inputs():
    case, r = C.case_and_ref("hostile")
    assert np.isfinite(r["rows"]).all() and C.counted(r).all()
    valid, G, M = r["valid"].numpy(), r["G"].numpy(), r["M"].numpy()
    D, Dp = case["depth"][..., 0], case["depth_prev"][..., 0]
    assert not valid[~np.isfinite(D)].any()                                  # NaN / +-Inf in D: not valid, so out of G ...
    assert not G[~np.isfinite(D)].any()
    for s, y, x in zip(*np.nonzero(~np.isfinite(D))):                        # ... and every window that holds it out of M
        win = M[s, max(y - 2, 0):y + 1, max(x - 2, 0):x + 1]                 # M is indexed by interior pixel (y - 1, x - 1)
        assert not win.any()
    # a previous-estimate pixel that is NaN, Inf, 0 or negative removes exactly the pixels whose four taps hold it
    clean = dict(case, depth_prev=np.where(np.isfinite(Dp) & (Dp > 0), Dp, 8.0).astype(np.float32)[..., None])
    rc = C.score(clean)
    assert (rc["M"].numpy() == M).all() and (rc["valid"].numpy() == valid).all()
    lost = rc["G"].numpy() & ~G
    assert lost.any() and not (G & ~rc["G"].numpy()).any()
    assert np.array_equal(r["rows"][:, :3], rc["rows"][:, :3])               # the photometric part does not read Dp


def test_out_of_view_sample_is_not_counted():
    _, r = C.case_and_ref("out-of-view")
    assert r["n"][0] == 0 and r["ng"][0] == 0 and not r["rows"][0].any()
    assert list(C.counted(r)) == [False, True]
    assert list(C.counted(r, reset=[0, 1])) == [False, False] and list(C.counted(r, active=[1, 0])) == [False, False]
