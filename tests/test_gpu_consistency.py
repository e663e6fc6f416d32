"""The reprojection-consistency score on the MI355X (m4d_consistency_per_sample, consistency.ConsistencyScorer, main.py
--consistency / --val_consistency).

Contracts: counts exact and every value within 2 float32 ulps of the float64 restatement (tests/consistency_ref.py: the bar is
derived there, not measured); masked-off samples are not read and give zero rows; row s of a batch is the row of a launch on
sample s alone, bit for bit, run after run, dense or strided; the driver writes the two files, leaves the seven metrics' file
byte-identical, and does not depend on the schedule or on eager / hipGraph execution."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import consistency_ref as C
from helpers import make_fake_dataset

pytestmark = pytest.mark.gpu


def _dev_case(case, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in case.items() if k != "name"}


def _run(t, reset=None, active=None, **kw):
    from m4depth_amd import network_ops as nops
    b = t["depth"].shape[0]
    dev = t["depth"].device
    reset = torch.zeros(b, dtype=torch.uint8, device=dev) if reset is None else reset
    active = torch.ones(b, dtype=torch.uint8, device=dev) if active is None else active
    rows, counted = nops.consistency_per_sample(t["depth"], t["depth_prev"], t["cur"], t["prev"], t["rot"], t["trans"], t["f"],
                                                t["c"], reset, active, **kw)
    return rows.cpu().numpy(), counted.cpu().numpy()


# ---- 1. against the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.RANDOM_CASES + ("exact", "hostile", "out-of-view"))
def test_rows_against_the_restatement(dev, name):
    """6 x 8 (smaller than a tile), 13 x 21 (ragged second tile, halo across a tile border), 24 x 40, 33 x 35 at b = 3 (three
    tiles per axis, the last one 1 and 3 pixels wide), quaternion and small-angle motion, the exact scene, hostile pixels, a
    sample out of view.  Counts exact, every value within 2 float32 ulps of the float64 restatement."""
    case, ref = C.case_and_ref(name)
    rows, counted = _run(_dev_case(case, dev))
    b, h, w, _ = case["depth"].shape
    u = C.ulps(rows, ref["rows"])
    print(f"[consistency] {name}: rows {rows.tolist()} ulps {u.max():.2f}")
    assert np.isfinite(rows).all()
    assert (counted == C.counted(ref)).all()
    # cover and geo_cover are counts over constants: N and Ng are exact iff these are the correctly rounded quotients
    want_cover = np.where(C.counted(ref), ref["n"] / float((h - 2) * (w - 2)), 0.0).astype(np.float32)
    want_geo_cover = np.where(C.counted(ref), ref["ng"] / float(h * w), 0.0).astype(np.float32)
    assert rows[:, 4].tobytes() == want_cover.tobytes() and rows[:, 5].tobytes() == want_geo_cover.tobytes()
    assert (u <= C.GPU_ULPS).all(), (name, u)
    # `better` is a count over N as well: exact (no pixel of M sits within 1e-9 of pe_w = pe_id, test_consistency_ref.py)
    assert rows[:, 2].tobytes() == ref["rows32"][:, 2].tobytes()
    if name == "exact":
        assert rows[0, 0] == 0.0 and rows[0, 3] == 0.0 and rows[0, 2] == 1.0
    if name == "out-of-view":
        assert not rows[0].any() and counted[0] == 0


@pytest.mark.parametrize("scale", [0.5, 2.0])
def test_forward_motion_closed_form(dev, scale):
    tz, z0 = 0.5, 8.0
    case = C.exact_scene(scale=scale, forward=tz)
    rows, counted = _run(_dev_case(case, dev))
    assert counted[0] == 1
    assert C.ulps(rows[0, 3], tz / (2 * scale * z0 + tz)) <= C.GPU_ULPS


# ---- 2. masks -----------------------------------------------------------------------------------------------------------------
def _four(dev):
    """b = 4: the two samples of 13x21-quat twice."""
    case, _ = C.case_and_ref("13x21-quat")
    four = {k: np.concatenate([v, v]) for k, v in case.items() if k != "name"}
    ref = C.score(four)
    return four, ref


def test_every_mask_pattern_and_poisoned_previous_buffers(dev):
    """b = 4, every (reset, active) pattern: uncounted rows are zero, counted rows keep their bits, and the previous image and
    estimate of every masked-off sample are NaN -- nothing of them reaches any row."""
    four, ref = _four(dev)
    clean = _dev_case(four, dev)
    full, _ = _run(clean)
    assert (C.ulps(full, ref["rows"]) <= C.GPU_ULPS).all()
    for code in range(1 << 8):
        bits = [(code >> i) & 1 for i in range(8)]
        reset_h, act_h = np.array(bits[:4], np.uint8), np.array(bits[4:], np.uint8)
        off = (reset_h == 1) | (act_h == 0)
        t = dict(clean)
        t["prev"], t["depth_prev"], t["depth"], t["cur"] = (clean[k].clone() for k in ("prev", "depth_prev", "depth", "cur"))
        for s in np.nonzero(off)[0]:
            for k in ("prev", "depth_prev", "depth", "cur"):
                t[k][int(s)] = float("nan")
        reset, act = torch.from_numpy(reset_h).to(dev), torch.from_numpy(act_h).to(dev)
        rows, counted = _run(t, reset.bool() if code % 2 else reset, act)
        assert (counted == (~off).astype(np.uint8)).all(), f"pattern {code}"
        want = np.where(off[:, None], np.float32(0.0), full)
        assert rows.tobytes() == want.tobytes(), f"pattern {code}"


# ---- 3. batch and layout ------------------------------------------------------------------------------------------------------
def test_batch_row_equals_single_sample_launch_and_repeats(dev):
    case, _ = C.case_and_ref("33x35")
    t = _dev_case(case, dev)
    rows, counted = _run(t)
    again, _ = _run(t)
    assert rows.tobytes() == again.tobytes()
    for s in range(3):
        one = {k: v[s:s + 1].contiguous() for k, v in t.items()}
        r1, c1 = _run(one)
        assert r1.tobytes() == rows[s:s + 1].tobytes() and c1[0] == counted[s], f"sample {s}"


def test_strided_frame_slices_equal_dense_copies(dev):
    """Images and estimates as frame slices of [B,T,...] tensors, read in place."""
    case, _ = C.case_and_ref("33x35")
    t = _dev_case(case, dev)
    dense, _ = _run(t)
    s = dict(t)
    for k in ("depth", "depth_prev", "cur", "prev"):
        big = torch.full((3, 3) + tuple(t[k].shape[1:]), float("nan"), dtype=torch.float32, device=dev)
        big[:, 1] = t[k]
        s[k] = big[:, 1]
        assert not s[k].is_contiguous()
    got, _ = _run(s)
    assert got.tobytes() == dense.tobytes()


def test_writes_into_a_log_without_host_sync(dev):
    """rows / counted as views of an [n_steps,B,6] / [n_steps,B] log, one launch pair per step, queued without a sync."""
    from m4depth_amd import network_ops as nops
    names = ["13x21-quat", "13x21-angle", "13x21-quat"]
    data = [_dev_case(C.case_and_ref(n)[0], dev) for n in names]
    want = [_run(t) for t in data]
    log_r = torch.full((3, 2, 6), float("nan"), dtype=torch.float32, device=dev)
    log_c = torch.full((3, 2), 0xA5, dtype=torch.uint8, device=dev)
    reset = torch.tensor([0, 1], dtype=torch.uint8, device=dev)
    active = torch.ones(2, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    for st, t in enumerate(data):
        out = nops.consistency_per_sample(t["depth"], t["depth_prev"], t["cur"], t["prev"], t["rot"], t["trans"], t["f"], t["c"],
                                          reset, active, rows=log_r[st], counted=log_c[st])
        assert out[0].data_ptr() == log_r[st].data_ptr() and out[1].data_ptr() == log_c[st].data_ptr()
    got_r, got_c = log_r.cpu().numpy(), log_c.cpu().numpy()
    for st in range(3):
        assert got_r[st, 0].tobytes() == want[st][0][0].tobytes() and not got_r[st, 1].any()
    assert (got_c == np.array([1, 0], np.uint8)).all()


# ---- 4. memory guards around the raw call -------------------------------------------------------------------------------------
SENTINEL = -0x3F213F22          # int32 bit pattern of the guard words (a finite negative float)
GUARD = 4096


class _Arena:
    """One sentinel-filled allocation; inputs and outputs are carved out of it with guard words on both sides."""

    def __init__(self, dev, words):
        self.buf = torch.full((words,), SENTINEL, dtype=torch.int32, device=dev)
        self.at = GUARD
        self.outputs = []

    def _take(self, n):
        lo = self.at
        self.at = (lo + n + GUARD + 63) // 64 * 64
        assert self.at <= self.buf.numel(), "arena too small"
        return lo

    def put(self, array):
        t = torch.from_numpy(np.array(array))
        n = (t.numel() * t.element_size() + 3) // 4
        lo = self._take(n)
        view = self.buf[lo:lo + n].view(t.dtype)[:t.numel()].reshape(t.shape)
        view.copy_(t.to(self.buf.device))
        return view

    def out(self, n_words):
        lo = self._take(n_words)
        self.outputs.append((lo, n_words))
        return self.buf[lo:lo + n_words]


@pytest.mark.parametrize("name", ["6x8-quat", "13x21-angle", "33x35", "hostile", "out-of-view"])
def test_raw_call_inside_guarded_memory(dev, name):
    """The C ABI with every input and output inside a sentinel-filled allocation: afterwards only the rows, the counted bytes
    and the workspace differ from the snapshot, and the rows are those of the wrapper."""
    from m4depth_amd._lib import lib, stream_ptr
    case, _ = C.case_and_ref(name)
    b, h, w, _ = case["depth"].shape
    ws_bytes = lib.m4d_consistency_workspace_bytes(b, h, w)
    assert ws_bytes == b * ((h + 15) // 16) * ((w + 15) // 16) * 6 * 8
    a = _Arena(dev, b * h * w * 8 + ws_bytes // 4 + 64 + 16 * GUARD + 4096)
    t = {k: a.put(v) for k, v in case.items() if k != "name"}
    reset, active = a.put(np.zeros(b, np.uint8)), a.put(np.ones(b, np.uint8))
    ws = a.out(ws_bytes // 4 + 2)
    rows, counted = a.out(b * 6), a.out((b + 3) // 4)
    ws_ptr = (ws.data_ptr() + 7) // 8 * 8
    before = a.buf.clone()
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    rc = lib.m4d_consistency_per_sample(p(t["depth"]), h * w, p(t["depth_prev"]), h * w, p(t["cur"]), 3 * h * w, p(t["prev"]),
                                        3 * h * w, p(t["rot"]), t["rot"].shape[1], p(t["trans"]), p(t["f"]), p(t["c"]), p(reset),
                                        p(active), b, h, w, ctypes.c_void_p(ws_ptr), p(rows), p(counted), stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    changed = a.buf != before
    for lo, n in a.outputs:
        changed[lo:lo + n] = False
    bad = changed.nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} words outside the outputs changed, first at {int(bad[0])}"
    got = rows.view(torch.float32).reshape(b, 6).cpu().numpy()
    want, want_c = _run(_dev_case(case, dev))
    assert got.tobytes() == want.tobytes()
    assert (counted.view(torch.uint8)[:b].cpu().numpy() == want_c).all()
    lo, n = a.outputs[-1]                                          # the bytes after counted[b-1] keep the sentinel
    assert torch.equal(a.buf[lo:lo + n].view(torch.uint8)[b:], before[lo:lo + n].view(torch.uint8)[b:])


# ---- 5. the driver ------------------------------------------------------------------------------------------------------------
LENGTHS = [7, 3, 11, 1, 6]                 # unequal, a one-frame trajectory (its only frame is a reset: never counted)
SIZE = 64
COMMON_ARCH = ["--arch_depth", "4", "--height", str(SIZE), "--width", str(SIZE)]
FILES = ("perfs-midair.txt", "perfs-consistency-midair.txt", "consistency-frames-midair.txt")


@pytest.fixture(scope="module")
def midair_set(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("consistency"))
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


def _files(midair_set, *extra):
    """{file name: bytes or None} of the checkpoint directory of one main.py run (cached per flag set)."""
    from m4depth_amd import main as MAIN
    if extra not in _runs:
        cfg, rec, root = midair_set
        ck = os.path.join(root, "ckpt_" + str(len(_runs)))
        argv = ["--mode", "eval", "--dataset", "midair", "--db_path_config", cfg, "--records_path", rec, "--ckpt_dir", ck]
        assert MAIN.main(argv + COMMON_ARCH + list(extra)) == 0
        _runs[extra] = {f: open(os.path.join(ck, f), "rb").read() if os.path.isfile(os.path.join(ck, f)) else None for f in FILES}
        _runs[extra]["dir"] = ck
    return _runs[extra]


def test_driver_writes_both_files_and_leaves_the_seven_alone(dev, midair_set):
    from m4depth_amd import consistency as CS
    plain = _files(midair_set, "--eval_streams", "4")
    got = _files(midair_set, "--eval_streams", "4", "--consistency")
    assert plain[FILES[1]] is None and plain[FILES[2]] is None                    # without the flag: no file is added
    assert got[FILES[0]] == plain[FILES[0]] and plain[FILES[0]] is not None       # the seven metrics: byte-identical
    means = CS.read_perfs(os.path.join(got["dir"], FILES[1]))
    frames = CS.read_frames(os.path.join(got["dir"], FILES[2]))
    print("[consistency] midair means", dict(zip(CS.COLUMNS, means.tolist())), len(frames), "frames")
    assert means.shape == (6,) and np.isfinite(means).all() and 0 < means[0] < 1 and 0 < means[4] <= 1
    # every frame but a trajectory's first is scored: in the sequential order
    want = [(t, f) for t, n in enumerate(LENGTHS) for f in range(1, n)]
    assert [(t, f) for t, f, _ in frames] == want
    total = np.zeros(6, np.float32)
    for _, _, row in frames:
        total = (total + row).astype(np.float32)
    assert (total / np.float32(len(frames))).astype(np.float32).tobytes() == means.tobytes()


def test_driver_schedule_and_graph_independence(dev, midair_set):
    a = _files(midair_set, "--eval_streams", "4", "--consistency")
    b = _files(midair_set, "--eval_streams", "4", "--consistency", "--eval_streams_policy", "arrival")
    g = _files(midair_set, "--eval_streams", "4", "--consistency", "--graph")
    for f in FILES:
        assert a[f] == b[f], f"lpt vs arrival: {f}"
        assert a[f] == g[f], f"eager vs graph: {f}"


def test_one_slot_equals_a_frame_by_frame_loop(dev, midair_set):
    """--eval_streams 1 --consistency against a Python loop over the batch-1 streaming loader: stream_step, then the op on
    (this estimate, the previous estimate, this image, the previous image), folded in float32."""
    from m4depth_amd import M4Depth
    from m4depth_amd import consistency as CS
    from m4depth_amd import dataloaders as dl
    from m4depth_amd import main as MAIN
    from m4depth_amd import network_ops as nops
    got = _files(midair_set, "--eval_streams", "1", "--consistency")
    cfg, rec, root = midair_set
    args = MAIN.build_parser().parse_args(["--mode", "eval", "--dataset", "midair", "--db_path_config", cfg, "--records_path", rec,
                                           "--ckpt_dir", os.path.join(root, "loop")] + COMMON_ARCH)
    ablation = MAIN.ablation_from_args(args)
    model = M4Depth(nbre_levels=args.arch_depth, ablation_settings=ablation)
    model.load_numpy_weights(MAIN.load_weights(args, ablation), dev)
    settings = dl.DataloaderParameters(MAIN.dataset_roots(cfg), rec, None, 4, False)
    frames = dl.get_loader("midair").get_dataset("eval", settings, batch_size=1, device=dev, out_size=[SIZE, SIZE])
    total, rows, prev = np.zeros(6, np.float32), [], None
    one = torch.ones(1, dtype=torch.uint8, device=dev)
    for data in frames:
        frame = MAIN._stream_frame(data, dev)
        est = model.stream_step(frame)["depth"]
        if prev is not None and not bool(data["new_traj"][0]):
            r, c = nops.consistency_per_sample(est, prev[0], frame["RGB_im"], prev[1], frame["rot"], frame["trans"],
                                               frame["camera"]["f"], frame["camera"]["c"], frame["new_traj"].to(torch.uint8), one)
            assert int(c[0]) == 1
            rows.append(r[0].cpu().numpy())
            total = (total + rows[-1]).astype(np.float32)
        prev = (est, frame["RGB_im"])
    means = (total / np.float32(len(rows))).astype(np.float32)
    assert CS.read_perfs(os.path.join(got["dir"], FILES[1])).tobytes() == means.tobytes()
    file_rows = CS.read_frames(os.path.join(got["dir"], FILES[2]))
    assert len(file_rows) == len(rows) and all(a[2].tobytes() == b.tobytes() for a, b in zip(file_rows, rows))


def test_recording_without_depth_evaluates_only_under_the_flag(dev, tmp_path):
    from recording_ref import CAMERA_B, write_recording
    from m4depth_amd import consistency as CS
    from m4depth_amd import main as MAIN
    rec, ck = str(tmp_path / "rec"), str(tmp_path / "ck")
    write_recording(rec, CAMERA_B, 8, with_depth=False)
    common = ["--mode", "eval", "--dataset", "recording", "--records_path", rec, "--eval_streams", "2", "--ckpt_dir", ck,
              "--arch_depth", "2", "--height", "64", "--width", "64"]
    with pytest.raises(ValueError, match=r"no depth\.txt -- the 'eval_streams' use case scores against ground truth"):
        MAIN.main(common)
    assert MAIN.main(common + ["--consistency"]) == 0
    assert not os.path.exists(os.path.join(ck, "perfs-recording.txt"))             # no ground truth: the seven are skipped
    means = CS.read_perfs(CS.perfs_path(ck, "recording"))
    frames = CS.read_frames(CS.frames_path(ck, "recording"))
    assert means.shape == (6,) and np.isfinite(means).all()
    assert [(t, f) for t, f, _ in frames] == [(0, f) for f in range(1, 8)]         # every frame kept, all but the first scored


def test_photometric_training_validates_on_a_recording_without_depth(dev, tmp_path, capsys):
    """--loss=photometric with --enable_validation --val_dataset=recording --val_consistency on a recording without depth.txt:
    a best directory judged on photo and one validation-consistency.txt line per epoch; refused without the flag."""
    from recording_ref import CAMERA_B, write_recording
    from m4depth_amd import checkpoints as CK
    from m4depth_amd import main as MAIN
    rec, ck = str(tmp_path / "rec"), str(tmp_path / "ck")
    write_recording(rec, CAMERA_B, 12, with_depth=False)
    cfg = str(tmp_path / "datasets_location.json")
    with open(cfg, "w") as fh:
        json.dump({}, fh)
    argv = ["--mode", "train", "--dataset", "recording", "--records_path", rec, "--arch_depth", "2", "--height", "64", "--width", "64",
            "--seq_len", "4", "--db_seq_len", "4", "--epochs", "2", "--ckpt_dir", ck, "--no_augmentation", "--loss", "photometric",
            "--enable_validation", "--val_dataset", "recording", "--val_records_path", rec, "--db_path_config", cfg]
    with pytest.raises(SystemExit):
        MAIN.main(argv)
    assert "has no depth.txt" in capsys.readouterr().err
    assert MAIN.main(argv + ["--val_consistency"]) == 0
    lines = open(os.path.join(ck, "validation-consistency.txt")).read().splitlines()
    assert len(lines) == 2 and all(len(l.split()) == 6 for l in lines)
    assert not os.path.exists(os.path.join(ck, "validation-perfs.txt"))
    best = os.path.join(ck, "best")
    table = open(os.path.join(best, "validation_perfs.csv")).read().splitlines()
    assert table[0] == "photo,ckpt_name" and len(table) == 2
    assert CK.best_checkpoint(ck) is not None and os.path.isfile(CK.best_checkpoint(ck))
    assert abs(float(table[1].split(",")[0]) - min(float(l.split()[0]) for l in lines)) < 1e-4    # lower photo wins
