"""Batched streaming evaluation, host side (no GPU): the slot schedule of m4depth_amd.stream_eval, the order-exact fold of the
per-sample metric log, main.py's --eval_streams flag, and the argument validation of m4d_depth_metrics_per_sample."""
import ctypes
import os
import re

import numpy as np
import pytest

from m4depth_amd import stream_eval as SE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [
    ([5], 1), ([5], 4), ([1], 3), ([1, 1, 1], 2), ([3, 1, 4, 1, 5, 9, 2, 6], 3), ([7, 7, 7, 7], 2), ([7, 7, 7, 7], 4),
    ([2, 40, 1, 17, 17, 3], 8), ([1, 2, 3, 4, 5, 6, 7, 8, 9, 10], 4), ([4, 0, 6, 2], 2), ([160, 40, 80, 100, 120, 60], 5),
]


def _check(lengths, n_slots, policy):
    sch = SE.schedule(lengths, n_slots, policy)
    cells, feed, reset = sch.cells, sch.feed, sch.reset
    n_live = sum(1 for n in lengths if n > 0)
    B = min(n_slots, n_live)
    assert sch.n_slots == B and cells.shape[1:] == (B, 2) and feed.shape == cells.shape and reset.shape == cells.shape[:2]
    # every (trajectory, frame) exactly once
    live = cells[..., 0] >= 0
    got = sorted(map(tuple, cells[live].tolist()))
    assert got == [(t, f) for t, n in enumerate(lengths) for f in range(n)]
    for s in range(B):
        col = cells[:, s]
        idle = np.nonzero(col[:, 0] < 0)[0]
        busy = np.nonzero(col[:, 0] >= 0)[0]
        assert busy.size > 0
        # idle cells only after the slot's last assignment (the tail), each re-feeding the slot's last frame with a reset
        if idle.size:
            assert idle[0] > busy[-1] and idle[-1] == len(col) - 1 and idle.size == len(col) - busy.size
            assert (feed[idle, s] == col[busy[-1]]).all() and reset[idle, s].all()
        assert (feed[busy, s] == col[busy]).all()
        # within a slot: frames of an assignment in order, a forced reset exactly where an assignment starts
        for k in busy:
            t, f = col[k]
            starts = f == 0
            assert reset[k, s] == starts
            if not starts:
                assert k > 0 and tuple(col[k - 1]) == (t, f - 1)
    assert SE.makespan(sch) == cells.shape[0] >= max(lengths)
    return sch


@pytest.mark.parametrize("policy", SE.POLICIES)
@pytest.mark.parametrize("lengths,n_slots", CASES)
def test_schedule_invariants(lengths, n_slots, policy):
    _check(lengths, n_slots, policy)


def test_schedule_random_invariants():
    rng = np.random.default_rng(3)
    for _ in range(200):
        lengths = rng.integers(1, 12, size=int(rng.integers(1, 10))).tolist()
        B = int(rng.integers(1, 12))
        for policy in SE.POLICIES:
            _check(lengths, B, policy)


def test_schedule_effective_slots_and_policies():
    assert SE.schedule([3, 5], 8).n_slots == 2                           # min(n_slots, n_traj)
    assert SE.schedule([4, 9, 2], 1, "arrival").cells.shape[0] == 15     # one slot: trajectories back to back
    arr = SE.schedule([2, 9, 3], 1, "arrival").cells[:, 0, 0]
    assert arr.tolist() == [0] * 2 + [1] * 9 + [2] * 3                   # csv order
    lpt = SE.schedule([2, 9, 3], 1, "lpt").cells[:, 0, 0]
    assert lpt.tolist() == [1] * 9 + [2] * 3 + [0] * 2                   # longest first
    with pytest.raises(ValueError):
        SE.schedule([3], 2, "random")
    with pytest.raises(ValueError):
        SE.schedule([3], 0)
    assert SE.schedule([], 4).cells.shape[0] == 0 and SE.schedule([0, 0], 4).n_slots == 0


@pytest.mark.parametrize("lengths,n_slots", [
    ([40, 60, 80, 100, 120, 160], 2), ([1, 2, 3, 4, 5, 6, 7, 8, 9, 10], 4), ([20] * 7 + [160], 4),
    (list(range(40, 161, 5)), 8), ([5, 5, 5, 50], 2), ([7, 7, 7, 7], 3),
])
def test_lpt_makespan_not_above_arrival(lengths, n_slots):
    """Longest first shortens the tail of csv orders that put long trajectories late (the typical case: the longest
    trajectory dealt last leaves its slot running alone)."""
    assert SE.makespan(SE.schedule(lengths, n_slots, "lpt")) <= SE.makespan(SE.schedule(lengths, n_slots, "arrival"))


def test_lpt_makespan_bound():
    """LPT list scheduling stays within Graham's 4/3 - 1/(3B) of the optimum (bounded below by max(sum / B, longest)).  It is
    not below arrival order on EVERY input -- e.g. lengths [8, 8, 5, 9, 7] on 2 slots: arrival 20, lpt 21 -- only on the
    typical ones above."""
    rng = np.random.default_rng(7)
    for _ in range(500):
        lengths = rng.integers(1, 200, size=int(rng.integers(1, 30))).tolist()
        B = int(rng.integers(1, 33))
        Be = min(B, len(lengths))
        lower = max(-(-sum(lengths) // Be), max(lengths))
        assert SE.makespan(SE.schedule(lengths, B, "lpt")) <= (4 / 3 - 1 / (3 * Be)) * lower + 1e-9
    assert SE.makespan(SE.schedule([8, 8, 5, 9, 7], 2, "lpt")) == 21
    assert SE.makespan(SE.schedule([8, 8, 5, 9, 7], 2, "arrival")) == 20


def _keras_mean_sequential(lengths, rows_of, counted_of):
    """The sequential run: frames in csv order, total = float32(total + v) per counted frame (metrics_finalize_kernel)."""
    total = [np.float32(0.0)] * 7
    count = 0
    for t, n in enumerate(lengths):
        for f in range(n):
            if counted_of[(t, f)]:
                v = rows_of[(t, f)]
                total = [np.float32(total[i] + v[i]) for i in range(7)]
                count += 1
    return np.array(total, np.float32), count


@pytest.mark.parametrize("policy", SE.POLICIES)
@pytest.mark.parametrize("n_slots", [1, 2, 3, 8, 40])
def test_fold_equals_sequential_keras_mean(policy, n_slots):
    rng = np.random.default_rng(n_slots * 7 + len(policy))
    lengths = rng.integers(1, 25, size=9).tolist()
    # per-frame rows spanning magnitudes (sums that round differently in another order), and random counted masks
    rows_of = {(t, f): (rng.random(7) * 10.0 ** rng.integers(-3, 4, size=7)).astype(np.float32)
               for t, n in enumerate(lengths) for f in range(n)}
    counted_of = {k: bool(rng.random() < 0.8) for k in rows_of}
    sch = SE.schedule(lengths, n_slots, policy)
    n_steps, B = sch.cells.shape[:2]
    rows = rng.random((n_steps, B, 7)).astype(np.float32) * 1e6          # idle cells hold garbage: never folded
    counted = rng.integers(0, 2, size=(n_steps, B)).astype(np.uint8)
    for st in range(n_steps):
        for s in range(B):
            t, f = sch.cells[st, s]
            if t >= 0:
                rows[st, s] = rows_of[(t, f)]
                counted[st, s] = counted_of[(t, f)]
            else:
                counted[st, s] = 0
    total, count = SE.fold(rows, counted, sch.cells)
    ref_total, ref_count = _keras_mean_sequential(lengths, rows_of, counted_of)
    assert count == ref_count
    assert total.dtype == np.float32 and total.tobytes() == ref_total.tobytes()
    res = SE.fold_result(total, count)
    assert res.tobytes() == (ref_total / np.float32(max(ref_count, 1))).astype(np.float32).tobytes()
    assert count == int(counted.sum())


def test_fold_rejects_mismatched_shapes():
    sch = SE.schedule([3, 2], 2)
    with pytest.raises(ValueError):
        SE.fold(np.zeros((3, 2, 6), np.float32), np.zeros((3, 2), np.uint8), sch.cells)
    with pytest.raises(ValueError):
        SE.fold(np.zeros((3, 2, 7), np.float32), np.zeros((2, 2), np.uint8), sch.cells)


# ---- main.py --eval_streams ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv", [
    ["--mode=train", "--dataset=midair", "--eval_streams=4"],
    ["--mode=finetune", "--dataset=midair", "--eval_streams=4"],
    ["--mode=predict", "--dataset=midair", "--eval_streams=4"],
    ["--mode=eval", "--eval_streams=4"],                                   # synthetic: no trajectories
    ["--mode=eval", "--dataset=synthetic", "--eval_streams=2"],
    ["--mode=eval", "--dataset=midair", "--db_seq_len=8", "--eval_streams=4"],
    ["--mode=validation", "--dataset=tartanair", "--db_seq_len=4", "--eval_streams=1"],
    ["--mode=eval", "--dataset=midair", "--eval_streams=-1"],
    ["--mode=eval", "--dataset=midair", "--eval_streams=4", "--eval_streams_policy=random"],
    ["--mode=eval", "--dataset=midair", "--eval_streams=x"],
])
def test_eval_streams_refused_combinations_exit_2(argv):
    from m4depth_amd import main as MN
    with pytest.raises(SystemExit) as e:
        MN.main(argv)
    assert e.value.code == 2


def test_eval_streams_absent_leaves_args_as_today():
    from m4depth_amd import main as MN
    p = MN.build_parser()
    base = vars(p.parse_args(["--mode=eval", "--dataset=midair"]))
    assert base["eval_streams"] == 0 and base["eval_streams_policy"] == "lpt"
    new = {"eval_streams", "eval_streams_policy"}
    argv = ["--mode=eval", "--dataset=midair", "--graph", "--batch_size=3"]
    a = vars(p.parse_args(argv))
    b = vars(p.parse_args(argv + ["--eval_streams=8"]))
    assert {k: v for k, v in a.items() if k not in new} == {k: v for k, v in b.items() if k not in new}
    ok = p.parse_args(["--mode=validation", "--dataset=kitti-raw", "--eval_streams=32", "--eval_streams_policy=arrival"])
    assert ok.eval_streams == 32 and ok.eval_streams_policy == "arrival" and ok.db_seq_len is None


# ---- the C entry point --------------------------------------------------------------------------------------------------
def _declared():
    txt = open(os.path.join(ROOT, "include", "m4depth_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(m4d_[a-z0-9_]+)\s*\(", txt))


def test_per_sample_metrics_declared_bound_exported():
    from m4depth_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("m4d_depth_metrics_per_sample", "m4d_metrics_per_sample_workspace_bytes"):
        assert s in _declared() and s in _lib.EXPORTED_SYMBOLS and hasattr(raw, s)
    assert _lib.lib.m4d_abi_version() == 6
    for b in (1, 3, 32, 100):
        assert _lib.lib.m4d_metrics_per_sample_workspace_bytes(b) == b * 512 * 9 * 8
    assert _lib.lib.m4d_metrics_per_sample_workspace_bytes(0) == 0


def test_per_sample_metrics_validate_without_device():
    from m4depth_amd._lib import lib
    f = ctypes.c_void_p(4096)              # never dereferenced: validation fails first
    fn = lib.m4d_depth_metrics_per_sample
    assert fn(None, 16, None, 16, 1, 16, 80.0, None, None, None, None, None, None) == 1
    good = (f, 16, f, 16, 2, 16, 80.0, f, f, f, f, f, None)
    for i in (0, 2, 7, 8, 9, 10, 11):                                      # every pointer, nulled in turn
        args = list(good)
        args[i] = None
        assert fn(*args) == 1, f"null pointer argument {i} accepted"
    for i, bad in ((4, 0), (4, -3), (5, 0), (5, -1), (1, 15), (3, 8), (1, -16)):   # b, per_image, strides below per_image
        args = list(good)
        args[i] = bad
        assert fn(*args) == 1, f"argument {i} = {bad} accepted"
