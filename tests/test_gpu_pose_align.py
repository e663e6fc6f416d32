"""Pose refinement on the MI355X (m4d_pose_align_*, pose_refine.PoseRefiner, main.py --refine_pose).

Contracts: one iteration's sums and updated pose are as close to the float64 restatement (tests/pose_align_ref.py) as a
float32 evaluation of the definition is, within a factor 4 (a different operation order inside a pixel with contraction off)
and N exactly; masked-off samples are not read and pass through bit for bit; run after run and batched or alone the same
bits; the rejection rules hold on the device; the whole schedule recovers a perturbed pose; the driver writes the per-frame
file and, with both caps at 0, leaves every consistency file byte-identical."""
import os

import numpy as np
import pytest
import torch

import pose_align_ref as P
from pose_align_ref import ONE_ITERATION, one_iteration_case

pytestmark = pytest.mark.gpu

RATIO = 4.0
ST = 64                       # doubles of state per sample (network_ops.POSE_ALIGN_STATE)
S_SUMS = 32


def _dev_case(case, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in case.items()}


def _levels(t, strides):
    """{stride: (cur level, prev level)} from the product's pyramid."""
    from m4depth_amd import network_ops as nops
    n = max(int(s).bit_length() - 1 for s in strides)
    cur = [t["cur"]] + (nops.image_pyramid_box(t["cur"], n) if n else [])
    prev = [t["prev"]] + (nops.image_pyramid_box(t["prev"], n) if n else [])
    return {1 << i: (cur[i], prev[i]) for i in range(n + 1)}


def _masks(t, reset, active):
    b, dev = t["rot"].shape[0], t["rot"].device
    reset = torch.zeros(b, dtype=torch.uint8, device=dev) if reset is None else reset
    active = torch.ones(b, dtype=torch.uint8, device=dev) if active is None else active
    return reset, active


def _schedule(t, strides, iters, huber=0.1, damping=1e-9, prior=(0.0, 0.0), min_cover=0.0, caps=(1e9, 1e9), reset=None,
              active=None, **outs):
    """begin, the schedule, end through the wrappers: (rot_out, trans_out, rows, state [b,64]) as numpy."""
    from m4depth_amd import network_ops as nops
    b, h, w, _ = t["Dp"].shape
    reset, active = _masks(t, reset, active)
    lv = _levels(t, strides)
    ws = nops.pose_align_begin(t["rot"], t["trans"], h, w)
    for s in strides:
        for _ in range(iters):
            nops.pose_align_iterate(ws, lv[s][0], lv[s][1], t["Dp"], t["f"], t["c"], reset, active, s, huber, damping, prior)
    rot, trans, rows = nops.pose_align_end(ws, t["rot"], t["trans"], reset, active, h, w, min_cover, caps, **outs)
    return rot.cpu().numpy(), trans.cpu().numpy(), rows.cpu().numpy(), ws[:b * ST].reshape(b, ST).cpu().numpy()


def _unpack(sums29):
    H = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            H[i, j] = H[j, i] = sums29[k]
            k += 1
    return H, sums29[21:27], sums29[27], sums29[28]


# ---- 1. one iteration against float64 ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_case():
    return one_iteration_case()


@pytest.mark.parametrize("s", ONE_ITERATION["strides"])
def test_one_iteration_against_float64(dev, one_case, s):
    """b = 3, per-sample off-centre cameras, 24 x 40 at strides 1, 2, 4 (partial 16-pixel tiles, level maps down to 6 x 10): H
    (normalised by sqrt(H_ii H_jj)), b, cost and the updated pose entrywise within 4x the float32 restatement's own distance
    to float64; N exact."""
    from m4depth_amd import network_ops as nops
    c, case = ONE_ITERATION, one_case
    t = _dev_case(case, dev)
    reset, active = _masks(t, None, None)
    lv = _levels(t, (s,))
    ws = nops.pose_align_begin(t["rot"], t["trans"], c["h"], c["w"])
    nops.pose_align_iterate(ws, lv[s][0], lv[s][1], t["Dp"], t["f"], t["c"], reset, active, s, c["huber"], c["damping"], c["prior"])
    state = ws[:c["b"] * ST].reshape(c["b"], ST).cpu().numpy()
    worst = 0.0
    for smp in range(c["b"]):
        A0, a0 = P.begin(case["rot"][smp], case["trans"][smp])
        ref = {}
        for dtype in (np.float64, np.float32):
            A, a, _, sm = P.iterate(case["cur"][smp], case["prev"][smp], case["Dp"][smp, ..., 0], case["f"][smp], case["c"][smp], A0, a0,
                                    np.zeros(6), s, c["huber"], c["damping"], c["prior"], dtype)
            assert not sm["bad"]
            ref[dtype] = (sm, A, a)
        sm64, A64, a64 = ref[np.float64]
        sm32, A32, a32 = ref[np.float32]
        H, bv, cost, n = _unpack(state[smp, S_SUMS:S_SUMS + 29])
        assert n == sm64["N"] == sm32["N"], (smp, n, sm64["N"])
        scale = np.sqrt(np.outer(np.diag(sm64["H"]), np.diag(sm64["H"])))
        got = np.concatenate([((H - sm64["H"]) / scale).ravel(), bv - sm64["b"], [cost - sm64["cost"]],
                              (state[smp, 0:9].reshape(3, 3) - A64).ravel(), state[smp, 9:12] - a64])
        own = np.concatenate([((sm32["H"] - sm64["H"]) / scale).ravel(), sm32["b"] - sm64["b"], [sm32["cost"] - sm64["cost"]],
                              (A32 - A64).ravel(), a32 - a64])
        assert np.isfinite(got).all()
        # entries float32 itself gets exactly (own == 0) allow the rounding of the double sums only
        ratio = np.abs(got) / np.maximum(np.abs(own), 1e-15)
        worst = max(worst, ratio.max())
        print(f"[pose-align] stride {s} sample {smp}: N {int(n)}, GPU / float32 distance to float64: max {ratio.max():.3f}, "
              f"median {np.median(ratio):.3f}; float32's own max {np.abs(own).max():.2e}")
        assert (np.abs(got) <= RATIO * np.abs(own) + 1e-15).all(), (smp, ratio.max())
        assert state[smp, 21] == 1.0 and state[smp, 22] == 0.0 and state[smp, 23] == s
        assert state[smp, 18] == state[smp, 19] == cost / n and state[smp, 20] == n / sm64["hw"]


# ---- 2. masks and memory guards ---------------------------------------------------------------------------------------------------
SENTINEL = -0x3F213F22
GUARD = 1024


def test_masked_samples_pass_through_and_guards_stay_intact(dev, one_case):
    """Sample 1 reset, sample 2 inactive, their images and estimate NaN: the given motion bit for bit, a zero row, sample 0 as
    in the unmasked run; outputs and workspace inside a sentinel-filled allocation whose guard words all survive."""
    from m4depth_amd import network_ops as nops
    c = ONE_ITERATION
    t = _dev_case(one_case, dev)
    full = _schedule(t, (4, 2, 1), 2)
    assert full[2][:, 6].tolist() == [1.0, 1.0, 1.0]
    for k in ("cur", "prev", "Dp"):
        t[k] = t[k].clone()
        t[k][1:] = float("nan")
    reset = torch.tensor([0, 1, 0], dtype=torch.uint8, device=dev)
    active = torch.tensor([1, 1, 0], dtype=torch.uint8, device=dev)
    ws_words = int(nops.lib.m4d_pose_align_workspace_bytes(c["b"], c["h"], c["w"])) // 4
    sizes = [ws_words, c["b"] * 4, c["b"] * 3, c["b"] * 8]
    arena = torch.full((sum(sizes) + 5 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    views, at = [], GUARD
    for n in sizes:
        views.append(arena[at:at + n].view(torch.float32))
        at += n + GUARD
    before = arena.clone()
    key = ("pose_align", dev, torch.cuda.current_stream(dev).cuda_stream)
    saved = nops._ws_cache.get(key)
    nops._ws_cache[key] = views[0]
    try:
        rot, trans, rows, _ = _schedule(t, (4, 2, 1), 2, reset=reset.bool(), active=active, rot_out=views[1].view(c["b"], 4),
                                        trans_out=views[2].view(c["b"], 3), rows=views[3].view(c["b"], 8))
    finally:
        if saved is None:
            del nops._ws_cache[key]
        else:
            nops._ws_cache[key] = saved
    assert rot[1:].tobytes() == one_case["rot"][1:].tobytes() and trans[1:].tobytes() == one_case["trans"][1:].tobytes()
    assert not rows[1:].any()
    assert rot[0].tobytes() == full[0][0].tobytes() and trans[0].tobytes() == full[1][0].tobytes()
    assert rows[0].tobytes() == full[2][0].tobytes() and rows[0, 6] == 1.0
    changed = arena != before
    at = GUARD
    for n in sizes:
        changed[at:at + n] = False
        at += n + GUARD
    assert int(changed.sum()) == 0, "guard words changed"


# ---- 3. determinism ---------------------------------------------------------------------------------------------------------------
def test_two_runs_and_single_sample_launches_give_the_same_bits(dev, one_case):
    t = _dev_case(one_case, dev)
    a = _schedule(t, (4, 2, 1), 2)
    b = _schedule(t, (4, 2, 1), 2)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    for smp in range(ONE_ITERATION["b"]):
        one = {k: v[smp:smp + 1].contiguous() for k, v in t.items()}
        o = _schedule(one, (4, 2, 1), 2)
        for x, y in zip(a, o):
            assert x[smp:smp + 1].tobytes() == y.tobytes(), f"sample {smp}"


def test_strided_frame_slices_equal_dense_copies(dev, one_case):
    """The frames and the estimate as frame slices of [B,T,...] tensors at stride 1 (read in place, NaN around them)."""
    t = _dev_case(one_case, dev)
    dense = _schedule(t, (1,), 2)
    s = dict(t)
    for k in ("cur", "prev", "Dp"):
        big = torch.full((3, 3) + tuple(t[k].shape[1:]), float("nan"), dtype=torch.float32, device=dev)
        big[:, 1] = t[k]
        s[k] = big[:, 1]
        assert not s[k].is_contiguous()
    got = _schedule(s, (1,), 2)
    for x, y in zip(dense, got):
        assert x.tobytes() == y.tobytes()


# ---- 4. the rejection rules -------------------------------------------------------------------------------------------------------
def test_rejection_rules(dev, one_case):
    t = _dev_case(one_case, dev)
    given = (one_case["rot"].tobytes(), one_case["trans"].tobytes())
    ok = _schedule(t, (4, 2, 1), 2)
    assert ok[2][:, 6].all() and ok[0].tobytes() != given[0] and ok[1].tobytes() != given[1]
    assert (ok[2][:, 1] < ok[2][:, 0]).all() and (ok[2][:, 5] == 6).all() and (ok[2][:, 3] > 0).all() and (ok[2][:, 4] > 0).all()
    # a flat grey image: H is singular, the first pivot is 0
    flat = dict(t, cur=torch.full_like(t["cur"], 0.5), prev=torch.full_like(t["prev"], 0.5))
    rot, trans, rows, state = _schedule(flat, (4, 2, 1), 2, damping=0.0)
    assert (rot.tobytes(), trans.tobytes()) == given and not rows[:, 6].any() and (state[:, 22] == 1.0).all()
    assert (rows[:, 5] == 0).all()
    # a cap of 0, either one
    for caps in ((0.0, 1e9), (1e9, 0.0), (0.0, 0.0)):
        rot, trans, rows, _ = _schedule(t, (4, 2, 1), 2, caps=caps)
        assert (rot.tobytes(), trans.tobytes()) == given and not rows[:, 6].any(), caps
        assert rows[:, :6].tobytes() == ok[2][:, :6].tobytes()                   # the diagnostics are those of the accepted run
    # coverage below the bar
    rot, trans, rows, _ = _schedule(t, (4, 2, 1), 2, min_cover=0.999)
    assert (rot.tobytes(), trans.tobytes()) == given and not rows[:, 6].any()
    # a huge prior: the pose stays within float32 rounding of the given one
    rot, trans, rows, _ = _schedule(t, (4, 2, 1), 2, prior=(1e12, 1e12))
    assert (np.abs(rot - one_case["rot"]) <= 2 * np.spacing(np.float32(1.0))).all()
    assert (np.abs(trans - one_case["trans"]) <= 2 * np.spacing(np.abs(one_case["trans"]))).all()
    assert (rows[:, 3] < 1e-9).all() and (rows[:, 4] < 1e-9).all()


# ---- 5. the whole schedule --------------------------------------------------------------------------------------------------------
def test_whole_schedule_recovers_the_perturbed_pose(dev):
    """The 48 x 64 plane scene, strides 4, 2, 1 x 5 iterations: the GPU's final pose within 4x the float32 restatement's distance
    (metres, radians) of the float64 restatement's, its errors to the true pose at least 10x below the start's."""
    sc, S = P.recovery_scene(), P.RECOVERY
    args = (sc["cur"], sc["prev"], sc["Dp"], sc["f"], sc["c"], sc["rot"], sc["trans"], S["strides"], S["iters"], S["huber"], S["damping"],
            S["prior"])
    o64, o32 = P.run(*args, np.float64), P.run(*args, np.float32)
    t = _dev_case(dict(cur=sc["cur"][None], prev=sc["prev"][None], Dp=sc["Dp"][None, ..., None], rot=sc["rot"][None],
                       trans=sc["trans"][None], f=sc["f"][None], c=sc["c"][None]), dev)
    rot, trans, rows, state = _schedule(t, S["strides"], S["iters"], S["huber"], S["damping"], S["prior"])
    A, a = state[0, 0:9].reshape(3, 3), state[0, 9:12]
    gpu, own = P.pose_errors(A, a, o64["A"], o64["a"]), P.pose_errors(o32["A"], o32["a"], o64["A"], o64["a"])
    before = P.pose_errors(*P.begin(sc["rot"], sc["trans"]), sc["A_true"], sc["a_true"])
    after = P.pose_errors(A, a, sc["A_true"], sc["a_true"])
    print(f"[pose-align] whole schedule: GPU to float64 {gpu[0]:.3e} m / {gpu[1]:.3e} rad, float32 restatement {own[0]:.3e} m / "
          f"{own[1]:.3e} rad; to the truth {before[0]:.4f} m / {np.degrees(before[1]):.3f} deg -> {after[0]:.5f} m / "
          f"{np.degrees(after[1]):.4f} deg; row {rows[0].tolist()}")
    assert gpu[0] <= RATIO * own[0] and gpu[1] <= RATIO * own[1]
    assert after[0] * 10 <= before[0] and after[1] * 10 <= before[1]
    assert rows[0, 6] == 1.0 and rows[0, 5] == 15 and rows[0, 1] < rows[0, 0]
    # the float32 outputs are the final pose in the network's convention, each rounded once
    want_rot, want_trans = P.given_motion(A, a)
    assert rot[0].tobytes() == want_rot.tobytes() and trans[0].tobytes() == want_trans.tobytes()


# ---- 6. the refiner and the driver --------------------------------------------------------------------------------------------------
def test_refiner_passes_the_first_two_frames_of_a_trajectory_through(dev, one_case):
    """PoseRefiner over four steps of a two-slot stream: step 0 has no previous frame, step 1 follows a reset (its estimate was
    made without parallax), slot 1 restarts at step 2 -- all pass through with zero rows; the rest are refined."""
    from m4depth_amd.pose_refine import PoseRefiner
    t = _dev_case({k: v[:2] for k, v in one_case.items()}, dev)
    frame = {"RGB_im": t["cur"], "rot": t["rot"], "trans": t["trans"], "camera": {"f": t["f"], "c": t["c"]}}
    prev = dict(frame, RGB_im=t["prev"])
    r = PoseRefiner(copy_estimate=True, strides=(4, 2, 1), iters=2, damping=1e-9, caps=(1e9, 1e9), min_cover=0.0)
    resets = [[1, 1], [0, 0], [0, 1], [0, 0]]
    active = torch.ones(2, dtype=torch.uint8, device=dev)
    log = torch.full((4, 2, 8), float("nan"), device=dev)
    outs = []
    for step, rs in enumerate(resets):
        f = prev if step % 2 == 0 else frame                       # the two images alternate: every step has something to align
        out = r.step(f, torch.tensor(rs, dtype=torch.bool, device=dev), active, log[step])
        r.keep(out, t["Dp"])
        outs.append((out["rot"].cpu().numpy(), out["trans"].cpu().numpy()))
    log = log.cpu().numpy()
    same = lambda o: o[0].tobytes() == one_case["rot"][:2].tobytes() and o[1].tobytes() == one_case["trans"][:2].tobytes()
    assert same(outs[0]) and same(outs[1]) and not log[0].any() and not log[1].any()
    assert log[2, 0, 5] == 6 and not log[2, 1].any() and outs[2][0][1].tobytes() == one_case["rot"][1].tobytes()
    # step 3, slot 0: `cur` against `prev` -- the launches of the schedule itself; slot 1: the step after its restart
    want = _schedule(t, (4, 2, 1), 2)
    assert log[3, 0].tobytes() == want[2][0].tobytes() and log[3, 0, 6] == 1.0 and not log[3, 1].any()
    assert outs[3][0][0].tobytes() == want[0][0].tobytes() and outs[3][1][0].tobytes() == want[1][0].tobytes()
    assert outs[3][0][1].tobytes() == one_case["rot"][1].tobytes() and outs[3][1][1].tobytes() == one_case["trans"][1].tobytes()


N_FRAMES = 8
_runs = {}


def _files(tmp_path_factory, *extra):
    """{file name: bytes or None} of one main.py run on the recording (cached per flag set)."""
    from recording_ref import CAMERA_B, write_recording
    from m4depth_amd import main as MAIN
    if "rec" not in _runs:
        _runs["rec"] = str(tmp_path_factory.mktemp("pose_refine") / "rec")
        write_recording(_runs["rec"], CAMERA_B, N_FRAMES, with_depth=False)
    if extra not in _runs:
        ck = os.path.join(os.path.dirname(_runs["rec"]), "ck_%d" % len(_runs))
        argv = ["--mode", "eval", "--dataset", "recording", "--records_path", _runs["rec"], "--eval_streams", "2", "--consistency",
                "--ckpt_dir", ck, "--arch_depth", "2", "--height", "64", "--width", "64"]
        assert MAIN.main(argv + list(extra)) == 0
        names = ("perfs-consistency-recording.txt", "consistency-frames-recording.txt", "pose-refine-frames-recording.txt")
        _runs[extra] = {f: open(os.path.join(ck, f), "rb").read() if os.path.isfile(os.path.join(ck, f)) else None for f in names}
        _runs[extra]["dir"] = ck
    return _runs[extra]


@pytest.mark.parametrize("graph", [(), ("--graph",)], ids=["eager", "graph"])
def test_driver_end_to_end(dev, tmp_path_factory, graph):
    """--mode=eval --eval_streams 2 --consistency --refine_pose on a tiny recording: the per-frame file has one row per scored
    frame; with --refine_pose_max 0 0 both consistency files equal the run without the flag byte for byte; without the flag no
    file is added."""
    from m4depth_amd import consistency as CS
    from m4depth_amd import pose_refine as PR
    plain = _files(tmp_path_factory, *graph)
    got = _files(tmp_path_factory, "--refine_pose", *graph)
    capped = _files(tmp_path_factory, "--refine_pose", "--refine_pose_max", "0", "0", *graph)
    assert plain["pose-refine-frames-recording.txt"] is None
    scored = CS.read_frames(os.path.join(got["dir"], "consistency-frames-recording.txt"))
    rows = PR.read_frames(PR.frames_path(got["dir"], "recording"))
    assert [(t, f) for t, f, _ in rows] == [(t, f) for t, f, _ in scored] == [(0, f) for f in range(1, N_FRAMES)]
    assert not rows[0][2].any()                                                  # frame 1 follows the reset: passed through
    assert all(np.isfinite(r).all() for _, _, r in rows) and any(r[5] > 0 for _, _, r in rows[1:])   # iterations ran
    print("[pose-align] driver rows", [r.tolist() for _, _, r in rows])
    for f in ("perfs-consistency-recording.txt", "consistency-frames-recording.txt"):
        assert plain[f] is not None and capped[f] == plain[f], f
    crow = PR.read_frames(PR.frames_path(capped["dir"], "recording"))
    assert len(crow) == len(rows) and not any(r[6] for _, _, r in crow)


@pytest.mark.parametrize("graph", [(), ("--graph",)], ids=["eager", "graph"])
def test_driver_predict_stream(dev, tmp_path_factory, graph):
    """--mode=predict --stream --refine_pose: runs, and with both caps at 0 writes the predictions of the run without it."""
    from m4depth_amd import main as MAIN
    _files(tmp_path_factory, *graph)                                             # writes the recording
    root = os.path.dirname(_runs["rec"])

    def predictions(name, *extra):
        ck = os.path.join(root, "predict_%s_%s" % (name, "graph" if graph else "eager"))
        argv = ["--mode", "predict", "--stream", "--dataset", "recording", "--records_path", _runs["rec"], "--ckpt_dir", ck,
                "--arch_depth", "2", "--height", "64", "--width", "64"]
        assert MAIN.main(argv + list(graph) + list(extra)) == 0
        return np.load(os.path.join(ck, "predictions.npy"))
    plain = predictions("plain")
    capped = predictions("capped", "--refine_pose", "--refine_pose_max", "0", "0")
    free = predictions("free", "--refine_pose")
    assert plain.shape[0] == N_FRAMES and capped.tobytes() == plain.tobytes()
    assert free.shape == plain.shape and np.isfinite(free).all()


def test_driver_graph_and_eager_agree(dev, tmp_path_factory):
    a = _files(tmp_path_factory, "--refine_pose")
    g = _files(tmp_path_factory, "--refine_pose", "--graph")
    for f in ("perfs-consistency-recording.txt", "consistency-frames-recording.txt", "pose-refine-frames-recording.txt"):
        assert a[f] == g[f], f
