"""The numpy restatement of the pose refinement (tests/pose_align_ref.py) checked against itself: the analytic Jacobian against
finite differences, the recovery of a perturbed pose on a rendered plane, and that no comparison input of
tests/test_gpu_pose_align.py sits on a discontinuity of the definition."""
import numpy as np
import pytest

import pose_align_ref as P
from pose_align_ref import ONE_ITERATION, one_iteration_case


def test_jacobian_against_central_differences():
    """J = [g, Y x g] for Y <- exp(w^) Y + v is the derivative of the restatement's own residual (float64), at every valid
    pixel whose query is not within 0.02 px of a cell boundary (the bilinear sample has a kink there)."""
    sc = P.recovery_scene()
    A, a = P.begin(sc["rot"], sc["trans"])
    args = (sc["cur"], sc["prev"], sc["Dp"], sc["f"], sc["c"])
    for s in (1, 2):
        p = P.pixel_terms(*args, A, a, s, np.float64)
        fx, fy = p["qx"] - np.floor(p["qx"]), p["qy"] - np.floor(p["qy"])
        use = p["ok"] & (fx > 0.02) & (fx < 0.98) & (fy > 0.02) & (fy < 0.98)
        assert use.sum() > 0.5 * use.size
        eps, worst = 1e-6, 0.0
        for k in range(6):
            d = np.zeros(6)
            d[k] = eps
            rp = P.pixel_terms(*args, *P.update(A, a, d), s, np.float64)["r"]
            rm = P.pixel_terms(*args, *P.update(A, a, -d), s, np.float64)["r"]
            fd = (rp - rm) / (2 * eps)
            err = np.abs(fd - p["J"][..., k])[use].max()
            worst = max(worst, err / np.abs(p["J"][..., k][use]).max())
        print(f"[pose-align] stride {s}: Jacobian against central differences, worst relative error {worst:.2e}")
        assert worst < 1e-6


def _recover(dtype):
    sc = P.recovery_scene()
    S = P.RECOVERY
    out = P.run(sc["cur"], sc["prev"], sc["Dp"], sc["f"], sc["c"], sc["rot"], sc["trans"], S["strides"], S["iters"], S["huber"],
                S["damping"], S["prior"], dtype)
    A0, a0 = P.begin(sc["rot"], sc["trans"])
    return sc, out, P.pose_errors(A0, a0, sc["A_true"], sc["a_true"]), P.pose_errors(out["A"], out["a"], sc["A_true"], sc["a_true"])


def test_recovery_of_a_perturbed_pose():
    """Strides 4, 2, 1 with 5 iterations each on the noise-free plane: both errors shrink at least 10x in float64.  The start
    pose is the true one perturbed as the definition perturbs a pose (Y <- exp(w^) Y + v): 0.405 deg and |w x a + v| =
    0.0531 m off (adding v to a alone would give |v| = 0.0539 m)."""
    sc, out, before, after = _recover(np.float64)
    print(f"[pose-align] recovery: {before[0]:.4f} m / {np.degrees(before[1]):.3f} deg -> {after[0]:.5f} m / "
          f"{np.degrees(after[1]):.4f} deg, row {out['row'].tolist()}")
    S = P.RECOVERY
    want = np.linalg.norm(P.rodrigues(S["d_rot"]) @ sc["a_true"] + np.array(S["d_trans"]) - sc["a_true"])
    assert abs(before[0] - want) < 1e-6 and abs(want - 0.0531) < 1e-4 and abs(np.degrees(before[1]) - 0.405) < 1e-3
    assert after[0] * 10 <= before[0] and after[1] * 10 <= before[1]
    assert out["applied"] and out["row"][1] < out["row"][0] and out["row"][5] == 15


def test_recovery_schedule_sits_on_no_discontinuity():
    """No pixel of any of the 15 iterations on the 48 x 64 scene within 1e-4 of the Huber switch or within 1e-3 px of the
    validity border (nor within 2e-5 px of a cell boundary), in float64 and in float32."""
    for dtype in (np.float64, np.float32):
        _, out, _, _ = _recover(dtype)
        print(f"[pose-align] recovery schedule, {dtype.__name__}: near {out['near']}, near_cell {out['near_cell']}")
        assert out["near_cell"] == 0
        assert out["near"] == 0, (dtype, out["near"])


def test_recovery_schedule_selects_the_same_pixels():
    _, o64, _, _ = _recover(np.float64)
    _, o32, _, _ = _recover(np.float32)
    assert o64["counts"] == o32["counts"] and len(o64["counts"]) == 15 and o64["near_cell"] == o32["near_cell"] == 0


def test_single_iteration_inputs_sit_on_no_discontinuity():
    """The Huber switch, the validity border and the cell boundaries: no pixel of the single-iteration case of
    tests/test_gpu_pose_align.py is near one, so float32 and float64 select the same pixels and branches."""
    case, c = one_iteration_case(), ONE_ITERATION
    for smp in range(c["b"]):
        A, a = P.begin(case["rot"][smp], case["trans"][smp])
        for s in c["strides"]:
            n = {}
            for dtype in (np.float64, np.float32):
                sm = P.sums(case["cur"][smp], case["prev"][smp], case["Dp"][smp, ..., 0], case["f"][smp], case["c"][smp], A, a, s,
                            c["huber"], dtype)
                assert sm["near"] == 0 and sm["near_cell"] == 0, (smp, s, dtype, sm["near"], sm["near_cell"])
                n[dtype] = sm["N"]
            assert n[np.float64] == n[np.float32] and 0 < n[np.float64] < sm["hw"]


def test_float32_restatement_is_close_to_float64():
    _, o64, _, _ = _recover(np.float64)
    _, o32, _, _ = _recover(np.float32)
    assert o32["applied"] and np.abs(o32["a"] - o64["a"]).max() < 1e-3 and P.rotation_angle(o32["A"], o64["A"]) < 1e-3


def test_rejections_of_the_restatement():
    sc = P.recovery_scene()
    S = P.RECOVERY
    flat = np.full_like(sc["cur"], 0.5)
    out = P.run(flat, flat, sc["Dp"], sc["f"], sc["c"], sc["rot"], sc["trans"], S["strides"], 2, S["huber"], 0.0, (0.0, 0.0), np.float64)
    assert not out["applied"] and out["rot"].tobytes() == sc["rot"].tobytes() and out["trans"].tobytes() == sc["trans"].tobytes()
    out = P.run(sc["cur"], sc["prev"], sc["Dp"], sc["f"], sc["c"], sc["rot"], sc["trans"], S["strides"], 2, S["huber"], S["damping"],
                (0.0, 0.0), np.float64, caps=(0.0, 0.0))
    assert not out["applied"] and out["rot"].tobytes() == sc["rot"].tobytes()
