"""Batched streaming evaluation on the MI355X (main.py --eval_streams, m4d_depth_metrics_per_sample).

Contracts: the per-sample metric kernel scores each sample exactly -- bit for bit -- as m4d_depth_metrics scores that image
alone; a 1-slot run writes the perfs file of today's one-frame-at-a-time streaming loop, bit for bit; the per-sample results
do not depend on the slot or the step a trajectory runs in; the hipGraph replay gives the eager bits; more slots change the
kernel dispatch of the network (batch size), and the perfs only within a measured tolerance."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import make_fake_dataset

pytestmark = pytest.mark.gpu


# ---- 1. the kernel against the existing one --------------------------------------------------------------------------------
def _per_image_reference(gt, est):
    from m4depth_amd import network_ops as nops
    return np.stack([nops.depth_metrics(gt[s:s + 1].contiguous(), est[s:s + 1].contiguous()).cpu().numpy()
                     for s in range(est.shape[0])])


def _guarded(b, dev):
    """rows [b,7] / counted [b] inside buffers with 64-element guard bands on both sides."""
    rbuf = torch.full((b * 7 + 128,), float("nan"), dtype=torch.float32, device=dev)
    rbuf[:64] = 1234.5
    rbuf[64 + b * 7:] = -777.25
    cbuf = torch.full((b + 128,), 0xA5, dtype=torch.uint8, device=dev)
    return rbuf, cbuf, rbuf[64:64 + b * 7].view(b, 7), cbuf[64:64 + b]


def _guards_intact(rbuf, cbuf, b):
    r, c = rbuf.cpu().numpy(), cbuf.cpu().numpy()
    return (r[:64] == 1234.5).all() and (r[64 + b * 7:] == -777.25).all() and (c[:64] == 0xA5).all() and (c[64 + b:] == 0xA5).all()


def _pair(rng, b, n, kind):
    gt = rng.uniform(0.5, 90.0, (b, n)).astype(np.float32)             # above max_d too: the clip is part of the contract
    est = rng.uniform(-1.0, 95.0, (b, n)).astype(np.float32)
    if kind == "sparse":                                                # velodyne-style ground truth: mostly zeros
        gt[rng.random((b, n)) < 0.8] = 0.0
    if kind == "zero_sample":
        gt[b // 2] = 0.0
    if kind == "near_one":                                              # log(gt) near the RMSE_log mask threshold
        gt = rng.uniform(0.999, 1.001, (b, n)).astype(np.float32)
    return gt, est


@pytest.mark.parametrize("b", [1, 3, 32])
@pytest.mark.parametrize("n", [1, 255, 257, 4097, 131073, 384 * 384])
def test_per_sample_rows_equal_per_image_metrics(dev, b, n):
    from m4depth_amd import network_ops as nops
    rng = np.random.default_rng(b * 1000 + n % 997)
    for kind in ("dense", "sparse", "zero_sample", "near_one"):
        gt_h, est_h = _pair(rng, b, n, kind)
        gt, est = torch.from_numpy(gt_h).to(dev), torch.from_numpy(est_h).to(dev)
        nt = torch.from_numpy((np.arange(b) % 3 == 1).astype(np.uint8)).to(dev)
        act = torch.from_numpy((np.arange(b) % 4 != 2).astype(np.uint8)).to(dev)
        rbuf, cbuf, rows, counted = _guarded(b, dev)
        out = nops.depth_metrics_per_sample(gt, est, nt, act, 80.0, rows=rows, counted=counted)
        assert out[0].data_ptr() == rows.data_ptr() and out[1].data_ptr() == counted.data_ptr()
        got = rows.cpu().numpy()
        ref = _per_image_reference(gt, est)
        assert got.tobytes() == ref.tobytes(), f"b={b} n={n} {kind}: rows differ from m4d_depth_metrics per image"
        assert np.isfinite(got).all()
        if kind == "zero_sample":
            assert (got[b // 2] == 0.0).all()
        assert (counted.cpu().numpy() == (act.cpu().numpy() & (1 - nt.cpu().numpy()))).all()
        assert _guards_intact(rbuf, cbuf, b), f"b={b} n={n} {kind}: a guard band was written"


def test_per_sample_strided_ground_truth(dev):
    """gt = depth[:, -1] of a [b,T,H,W,1] sequence batch and est = a slice of a larger buffer, both read in place."""
    from m4depth_amd import network_ops as nops
    rng = np.random.default_rng(5)
    b, T, H, W = 5, 3, 48, 80
    depth = torch.from_numpy(rng.uniform(0.0, 85.0, (b, T, H, W, 1)).astype(np.float32)).to(dev)
    big = torch.from_numpy(rng.uniform(0.0, 85.0, (b, 2, H, W, 1)).astype(np.float32)).to(dev)
    gt, est = depth[:, -1], big[:, 0]
    assert not gt.is_contiguous() and not est.is_contiguous()
    ones, zeros = torch.ones(b, dtype=torch.uint8, device=dev), torch.zeros(b, dtype=torch.uint8, device=dev)
    rows, counted = nops.depth_metrics_per_sample(gt, est, zeros, ones)
    ref = _per_image_reference(gt, est)
    assert rows.cpu().numpy().tobytes() == ref.tobytes()
    assert (counted.cpu().numpy() == 1).all()


def test_per_sample_counted_for_every_mask_pattern(dev):
    from m4depth_amd import network_ops as nops
    b, n = 4, 300
    rng = np.random.default_rng(9)
    gt_h, est_h = _pair(rng, b, n, "dense")
    gt, est = torch.from_numpy(gt_h).to(dev), torch.from_numpy(est_h).to(dev)
    ref = _per_image_reference(gt, est)
    for code in range(1 << (2 * b)):
        bits = [(code >> i) & 1 for i in range(2 * b)]
        nt_h, act_h = np.array(bits[:b], np.uint8), np.array(bits[b:], np.uint8)
        nt, act = torch.from_numpy(nt_h).to(dev), torch.from_numpy(act_h).to(dev)
        rbuf, cbuf, rows, counted = _guarded(b, dev)
        nops.depth_metrics_per_sample(gt, est, nt.bool() if code % 2 else nt, act, rows=rows, counted=counted)
        assert (counted.cpu().numpy() == (act_h & (1 - nt_h))).all(), f"pattern {code}"
        assert rows.cpu().numpy().tobytes() == ref.tobytes()          # the masks never change the scores
        assert _guards_intact(rbuf, cbuf, b)


def test_per_sample_writes_into_a_log_without_host_sync(dev):
    """rows / counted as views of an [n_steps,B,7] / [n_steps,B] log, one launch per step, queued without a synchronisation."""
    from m4depth_amd import network_ops as nops
    n_steps, b, n = 6, 3, 1000
    rng = np.random.default_rng(2)
    log_r = torch.zeros((n_steps, b, 7), dtype=torch.float32, device=dev)
    log_c = torch.zeros((n_steps, b), dtype=torch.uint8, device=dev)
    data = [tuple(torch.from_numpy(x).to(dev) for x in _pair(rng, b, n, "dense")) for _ in range(n_steps)]
    nt = torch.tensor([1, 0, 0], dtype=torch.uint8, device=dev)
    act = torch.tensor([1, 1, 0], dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    for st, (gt, est) in enumerate(data):
        nops.depth_metrics_per_sample(gt, est, nt, act, rows=log_r[st], counted=log_c[st])
    for st, (gt, est) in enumerate(data):
        assert log_r[st].cpu().numpy().tobytes() == _per_image_reference(gt, est).tobytes()
    assert (log_c.cpu().numpy() == np.array([0, 1, 0], np.uint8)).all()


# ---- 2-5. the driver ---------------------------------------------------------------------------------------------------
LENGTHS = [7, 3, 11, 1, 6]                 # unequal, a one-frame trajectory (its only frame is a reset: never counted)
SIZE = 64
COMMON_ARCH = ["--arch_depth", "4", "--height", str(SIZE), "--width", str(SIZE)]


@pytest.fixture(scope="module")
def midair_set(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("stream_eval"))
    db, rec = make_fake_dataset(root, "midair", n_traj=len(LENGTHS), n_frames=max(LENGTHS), size=(SIZE, SIZE), seed=17)
    for t, n in enumerate(LENGTHS):                 # truncate the trajectory files to unequal lengths
        path = os.path.join(rec, f"set_{t}", f"traj_{t:04d}.csv")
        lines = open(path).read().splitlines()
        with open(path, "w") as fh:
            fh.write("\n".join(lines[:1 + n]) + "\n")
    cfg = os.path.join(root, "datasets_location.json")
    with open(cfg, "w") as fh:
        json.dump({"midair": db}, fh)
    return cfg, rec, root


_runs = {}


def _perfs(dataset_set, *extra, dataset="midair", arch=None):
    """perfs-<dataset>.txt of one main.py run (cached per dataset and flag set): (the file's bytes, the 7 values)."""
    from m4depth_amd import main as MAIN
    key = (dataset,) + tuple(extra)
    if key not in _runs:
        cfg, rec, root = dataset_set
        ck = os.path.join(root, "ckpt_" + str(len(_runs)))
        argv = ["--mode", "eval", "--dataset", dataset, "--db_path_config", cfg, "--records_path", rec, "--ckpt_dir", ck]
        assert MAIN.main(argv + (COMMON_ARCH if arch is None else arch) + list(extra)) == 0
        path = os.path.join(ck, "perfs-" + dataset + ".txt")
        _runs[key] = (open(path, "rb").read(), np.loadtxt(path).astype(np.float32))
    return _runs[key]


@pytest.mark.parametrize("graph", [False, True])
def test_one_slot_equals_sequential_streaming_eval(dev, midair_set, graph):
    """--eval_streams 1 writes today's --mode=eval streaming perfs file, bit for bit: the fold reproduces the in-kernel Keras
    accumulation and stream_step at batch 1 gives test_step's depth."""
    seq_bytes, seq = _perfs(midair_set)
    got_bytes, got = _perfs(midair_set, "--eval_streams", "1", *(["--graph"] if graph else []))
    assert np.isfinite(seq).all() and seq[0] > 0
    assert got_bytes == seq_bytes, f"1 slot {'graph' if graph else 'eager'}: {got} vs sequential {seq}"


def test_schedule_independence(dev, midair_set):
    """4 slots: longest-first and csv-order dealing put the trajectories in other slots and steps -- the same perfs bits."""
    a = _perfs(midair_set, "--eval_streams", "4", "--eval_streams_policy", "lpt")
    b = _perfs(midair_set, "--eval_streams", "4", "--eval_streams_policy", "arrival")
    assert a[0] == b[0], f"lpt {a[1]} vs arrival {b[1]}"


def test_graph_equals_eager(dev, midair_set):
    a = _perfs(midair_set, "--eval_streams", "4")
    b = _perfs(midair_set, "--eval_streams", "4", "--graph")
    assert a[0] == b[0], f"eager {a[1]} vs graph {b[1]}"


# measured on the MI355X (4 / 8 slots against 1): relative AbsRel 4.15e-5 / 3.48e-6, SqRel 3.52e-5 / 2.41e-5, RMSE 1.18e-5 /
# 1.10e-5, RMSE_log 8.19e-4 / 6.82e-4; Delta1-3 absolute 3.18e-5 / 4.25e-5.  Tolerances: within 2x of the larger of the two.
BATCHED_REL_TOL = np.array([8.2e-5, 7.0e-5, 2.3e-5, 1.6e-3], np.float32)
BATCHED_DELTA_TOL = 8.4e-5


@pytest.mark.parametrize("slots", [4, 8])
def test_batched_close_to_sequential(dev, midair_set, slots):
    """4 and 8 slots against 1 slot.  The network's batch size picks other convolution kernels (the latency-first and
    one-launch coarse-front forms at batch 1, the persistent Winograd kernel from batch 8), so a frame's depth differs from the
    batch-1 depth in the last bits, and the perfs differ with it.  The seeded random weights make the estimates ill-conditioned
    (AbsRel ~0.94, depth = (s / parallax - tz) / alpha cancels): last-bit differences grow most in RMSE_log, where clipped
    estimates near 0.001 dominate.  Measured (4 / 8 slots): relative AbsRel 4.15e-5 / 3.48e-6, SqRel 3.52e-5 / 2.41e-5,
    RMSE 1.18e-5 / 1.10e-5, RMSE_log 8.19e-4 / 6.82e-4; Delta1-3 absolute 3.18e-5 / 4.25e-5 (under one pixel of one 64x64
    frame, 2.4e-4).  Tolerances: 2x the larger measurement, per metric (BATCHED_REL_TOL, BATCHED_DELTA_TOL)."""
    _, one = _perfs(midair_set, "--eval_streams", "1")
    _, got = _perfs(midair_set, "--eval_streams", str(slots))
    rel = np.abs(got[:4] - one[:4]) / np.abs(one[:4])
    dd = np.abs(got[4:] - one[4:])
    print(f"[stream_eval] {slots} slots vs 1: relative {rel} (AbsRel..RMSE_log), Delta {dd}")
    assert (rel <= BATCHED_REL_TOL).all(), (got, one)
    assert (dd <= BATCHED_DELTA_TOL).all(), (got, one)


# ---- per-trajectory intrinsics: a slot must carry its own trajectory's camera into the network ------------------------------
KITTI_LENGTHS = [5, 2, 4, 3, 2]            # more trajectories than slots: a slot takes a second trajectory, with another camera
KITTI_SIZE = (48, 80)                      # the smallest 4-level size (multiples of 16) the Garg crop leaves rows and columns of
KITTI_ARCH = ["--arch_depth", "4", "--height", str(KITTI_SIZE[0]), "--width", str(KITTI_SIZE[1])]
# fx fy cx cy (normalised by the image size) of each trajectory: all different, f != c, off centre
KITTI_CAMERAS = [(0.58, 1.92, 0.49, 0.51), (0.71, 1.55, 0.53, 0.46), (0.83, 1.11, 0.31, 0.66), (0.64, 1.73, 0.44, 0.57),
                 (0.92, 1.31, 0.61, 0.38)]


@pytest.fixture(scope="module")
def kitti_set(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("stream_eval_kitti"))
    db, rec = make_fake_dataset(root, "kitti-raw", n_traj=len(KITTI_LENGTHS), n_frames=max(KITTI_LENGTHS), size=KITTI_SIZE, seed=23)
    for t, n in enumerate(KITTI_LENGTHS):           # unequal lengths, another camera per trajectory
        path = os.path.join(rec, f"set_{t}", f"traj_{t:04d}.csv")
        lines = open(path).read().splitlines()
        out = [lines[0]]
        for ln in lines[1:1 + n]:
            v = ln.split("\t")
            v[-4:] = [repr(x) for x in KITTI_CAMERAS[t]]
            out.append("\t".join(v))
        with open(path, "w") as fh:
            fh.write("\n".join(out) + "\n")
    cfg = os.path.join(root, "datasets_location.json")
    with open(cfg, "w") as fh:
        json.dump({"kitti-raw": db}, fh)
    return cfg, rec, root


def _kitti_perfs(kitti_set, *extra):
    return _perfs(kitti_set, *extra, dataset="kitti-raw", arch=KITTI_ARCH)


@pytest.mark.parametrize("graph", [False, True])
def test_one_slot_equals_sequential_with_per_trajectory_cameras(dev, kitti_set, graph):
    """KITTI format, another camera per trajectory: --eval_streams 1 writes the sequential run's perfs file, byte for byte, eager
    and from the hipGraph (whose static camera buffers must follow the trajectory in the slot)."""
    seq_bytes, seq = _kitti_perfs(kitti_set)
    got_bytes, got = _kitti_perfs(kitti_set, "--eval_streams", "1", *(["--graph"] if graph else []))
    assert np.isfinite(seq).all() and seq[0] > 0
    assert got_bytes == seq_bytes, f"1 slot {'graph' if graph else 'eager'}: {got} vs sequential {seq}"


def test_schedule_independence_with_per_trajectory_cameras(dev, kitti_set):
    """4 slots, longest-first against csv-order dealing: the trajectories run in other slots, so a slot that carried another
    trajectory's camera into the network would change these bytes (the Mid-Air set, one camera for all, cannot show that)."""
    a = _kitti_perfs(kitti_set, "--eval_streams", "4", "--eval_streams_policy", "lpt")
    b = _kitti_perfs(kitti_set, "--eval_streams", "4", "--eval_streams_policy", "arrival")
    assert np.isfinite(a[1]).all() and a[1][0] > 0
    assert a[0] == b[0], f"lpt {a[1]} vs arrival {b[1]}"


# ---- the slot loader against the batch-1 streaming plan -----------------------------------------------------------------
def test_slot_loader_feeds_the_sequential_frames(dev, tmp_path):
    """KITTI format (per-frame intrinsics, sparse velodyne depth, the Garg crop): every live cell of the slot plan carries the
    frame the batch-1 streaming plan gives for that (trajectory, frame), bit for bit -- image, depth, pose, camera -- with the
    masks of the schedule; an idle cell repeats its slot's last frame with reset and new_traj set and active clear."""
    from m4depth_amd import dataloaders as dl
    lengths = [5, 2, 4]
    db, rec = make_fake_dataset(str(tmp_path), "kitti-raw", n_traj=len(lengths), n_frames=max(lengths), size=(40, 72), seed=3)
    rng = np.random.default_rng(4)
    for t, n in enumerate(lengths):
        path = os.path.join(rec, f"set_{t}", f"traj_{t:04d}.csv")
        lines = open(path).read().splitlines()
        out = [lines[0]]
        for ln in lines[1:1 + n]:                        # per-frame intrinsics
            v = ln.split("\t")
            v[-4:] = [repr(float(x)) for x in rng.uniform(0.4, 1.9, 4)]
            out.append("\t".join(v))
        with open(path, "w") as fh:
            fh.write("\n".join(out) + "\n")
    settings = dl.DataloaderParameters({"kitti-raw": db}, rec, None, 4, False)
    seq = list(dl.get_loader("kitti-raw").get_dataset("eval", settings, batch_size=1, device=dev, out_size=[40, 72]))
    ref, k = {}, 0
    for t, n in enumerate(lengths):
        for f in range(n):
            ref[(t, f)] = seq[k]
            k += 1
    assert k == len(seq)
    ds = dl.get_loader("kitti-raw").get_dataset("eval_streams", settings, batch_size=2, device=dev, out_size=[40, 72],
                                                slot_policy="arrival")
    sch = ds.schedule
    assert ds.n_slots == 2 and len(ds) == sch.cells.shape[0]
    n_idle, last = 0, {}
    for step, b in enumerate(ds):
        assert (b["cells"] == sch.cells[step]).all()
        reset, nt, act = (b[k].cpu().numpy() for k in ("reset", "new_traj", "active"))
        for s in range(2):
            t, f = sch.cells[step, s]
            got = {"RGB_im": b["RGB_im"][s], "depth": b["depth"][s], "rot": b["rot"][s], "trans": b["trans"][s],
                   "f": b["camera"]["f"][s], "c": b["camera"]["c"][s]}
            if t < 0:                                    # idle: the slot's last frame again
                n_idle += 1
                assert reset[s] == 1 and nt[s] == 1 and act[s] == 0
                for key, v in got.items():
                    assert torch.equal(v, last[s][key]), f"idle step {step} slot {s}: {key}"
                continue
            r = ref[(int(t), int(f))]
            want = {"RGB_im": r["RGB_im"][0], "depth": r["depth"][0], "rot": r["rot"][0], "trans": r["trans"][0],
                    "f": r["camera"]["f"][0], "c": r["camera"]["c"][0]}
            for key in want:
                assert torch.equal(got[key], want[key]), f"step {step} slot {s} ({t}, {f}): {key}"
            assert act[s] == 1 and nt[s] == int(f == 0) and reset[s] == int(f == 0 or sch.reset[step, s])
            last[s] = {key: v.clone() for key, v in got.items()}
    assert n_idle > 0
