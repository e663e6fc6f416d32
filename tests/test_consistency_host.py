"""Host side of the reprojection-consistency score (main.py --consistency / --val_consistency): the 6-column fold, the parser's
refusals, the recording loader's switch, best-N on ``photo``, the two file formats, the entry point's argument refusals.
No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from recording_ref import CAMERA_A, CAMERA_B, write_recording


# ---- the fold ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["lpt", "arrival"])
def test_fold_consistency_against_a_plain_loop(policy):
    from m4depth_amd import consistency as CS
    from m4depth_amd import stream_eval as SE
    assert CS.fold is SE.fold_consistency
    lengths = [7, 3, 11, 1, 6]
    rng = np.random.default_rng(3)
    per_frame = {(t, f): rng.uniform(0.0, 1.0, 6).astype(np.float32) for t, n in enumerate(lengths) for f in range(n)}
    uncounted = {(t, 0) for t in range(len(lengths))} | {(2, 5), (4, 3)}          # first frames, and two the device ruled out
    sched = SE.schedule(lengths, 3, policy)
    n_steps, B = sched.cells.shape[:2]
    rows = np.full((n_steps, B, 6), np.nan, np.float32)
    counted = np.zeros((n_steps, B), np.uint8)
    for st in range(n_steps):
        for sl in range(B):
            t, f = (int(v) for v in sched.cells[st, sl])
            if t >= 0:
                rows[st, sl] = per_frame[(t, f)]
                counted[st, sl] = (t, f) not in uncounted
    total, count, frames = SE.fold_consistency(rows, counted, sched.cells)
    want, n, walk = np.zeros(6, np.float32), 0, []
    for t, length in enumerate(lengths):                                           # the sequential run: csv order, frame order
        for f in range(length):
            if (t, f) not in uncounted:
                want = (want + per_frame[(t, f)]).astype(np.float32)
                n += 1
                walk.append((t, f))
    assert total.dtype == np.float32 and total.tobytes() == want.tobytes() and count == n
    assert [(t, f) for t, f, _ in frames] == walk
    assert all(r.tobytes() == per_frame[(t, f)].tobytes() for t, f, r in frames)
    with pytest.raises(ValueError, match="disagree"):
        SE.fold_consistency(np.zeros((n_steps, B, 7), np.float32), counted, sched.cells)
    with pytest.raises(ValueError, match="disagree"):                              # and `fold` still takes 7 columns only
        SE.fold(rows, counted, sched.cells)


# ---- the parser -------------------------------------------------------------------------------------------------------------------
REC = ["--dataset", "recording", "--arch_depth", "2", "--height", "64", "--width", "64"]


def _parse(argv, world=1):
    from m4depth_amd import main as M
    parser = M.build_parser()
    args = parser.parse_args(argv)
    M._check_eval_streams(parser, args)
    M.check_train_args(parser, args, world)
    M.check_recording_args(parser, args)
    return args


def test_refusals(tmp_path, capsys):
    write_recording(str(tmp_path / "nogt"), CAMERA_B, 6, with_depth=False)
    val = ["--mode", "train", "--enable_validation", "--db_path_config", "x.json", "--val_dataset", "recording",
           "--val_records_path", str(tmp_path / "nogt")]
    for bad, message in ((["--mode", "eval", "--consistency"], "--consistency needs --eval_streams"),
                         (["--mode", "eval", "--dataset", "midair", "--consistency", "--db_seq_len", "4"],
                          "--consistency needs --eval_streams"),
                         (["--mode", "predict", "--consistency"], "--consistency needs --eval_streams"),
                         (["--mode", "train", "--consistency"], "--consistency needs --eval_streams"),
                         (["--mode", "train", "--val_consistency"], "--val_consistency needs --enable_validation"),
                         (["--mode", "eval", "--val_consistency"], "--val_consistency needs --enable_validation"),
                         (val, "--enable_validation: a recording .* has no depth.txt")):      # today's wording stays
        with pytest.raises(SystemExit) as e:
            _parse(bad)
        assert e.value.code == 2 and re.search(message, capsys.readouterr().err), bad
    a = _parse(val + ["--val_consistency", "--loss", "photometric"])
    assert a.val_consistency
    for graph in ([], ["--graph"]):
        a = _parse(["--mode", "eval", "--dataset", "midair", "--eval_streams", "4", "--consistency"] + graph)
        assert a.consistency and a.eval_streams == 4
    a = _parse(["--mode", "eval"])
    assert a.consistency is False and a.val_consistency is False


def test_validation_args_under_val_consistency():
    from m4depth_amd import main as M
    base = ["--mode", "train", "--enable_validation", "--db_path_config", "x.json", "--val_dataset", "midair",
            "--val_records_path", "r", "--batch_size", "3"]
    v = M.validation_args(_parse(base))
    assert (v.eval_streams, v.consistency, v.db_seq_len, v.seq_len) == (0, False, 4, 4)              # as today
    v = M.validation_args(_parse(base + ["--val_consistency"]))
    assert (v.mode, v.eval_streams, v.consistency, v.db_seq_len, v.graph) == ("validation", 3, True, None, False)


def test_recording_loader_switch(tmp_path):
    """A recording without depth.txt: 'eval_streams' refuses it as every scoring use case does, word for word, unless the
    switch is set -- main.py sets it only under --consistency -- and then every frame is kept."""
    from m4depth_amd import dataloaders as dl
    from m4depth_amd import main as M
    root = str(tmp_path / "b")
    write_recording(root, CAMERA_B, 6, with_depth=False)
    settings = dl.DataloaderParameters(None, root, None, None, False)
    loader = dl.get_loader("recording")
    assert loader.allow_missing_depth_streams is False
    with pytest.raises(ValueError) as e:
        loader.get_dataset("eval_streams", settings, batch_size=2, out_size=[64, 64], device="cpu")
    assert str(e.value) == (f"{root}: no depth.txt -- the 'eval_streams' use case scores against ground truth; a recording "
                            "without it can only be predicted (--mode=predict)")
    loader = dl.get_loader("recording")
    loader.allow_missing_depth_streams = True
    ds = loader.get_dataset("eval_streams", settings, batch_size=2, out_size=[64, 64], device="cpu")
    assert len(ds) == 6 and ds.n_slots == 1
    with pytest.raises(ValueError, match=r"b: no depth\.txt"):                     # the switch is this use case's alone
        loader.get_dataset("eval", settings, batch_size=1, out_size=[64, 64], device="cpu")
    common = ["--mode", "eval", "--records_path", root, "--eval_streams", "2"] + REC
    assert not M.recording_loader(_parse(common)).allow_missing_depth_streams
    assert M.recording_loader(_parse(common + ["--consistency"])).allow_missing_depth_streams
    gt = str(tmp_path / "gt")
    write_recording(gt, CAMERA_A, 6, with_depth=True)             # with ground truth the loader behaves exactly as without the flag
    with_gt = ["--mode", "eval", "--records_path", gt, "--eval_streams", "2", "--consistency"] + REC
    assert not M.recording_loader(_parse(with_gt)).allow_missing_depth_streams


# ---- best-N on photo ----------------------------------------------------------------------------------------------------------------
def _ckpt(d, step):
    os.makedirs(d, exist_ok=True)
    np.savez(os.path.join(d, f"ckpt-{step}.npz"), w=np.full(2, float(step), np.float32))


def test_best_n_on_photo(tmp_path):
    from m4depth_amd import checkpoints as CK
    train, best = str(tmp_path / "train"), str(tmp_path / "best")
    assert CK.PHOTO_CRITERION.columns == ("photo",) and CK.PHOTO_CRITERION.lower == ("photo",)
    assert CK.DEFAULT_CRITERION.columns == CK.METRIC_COLUMNS
    mgr = CK.BestCheckpointManager(train, best, keep_top_n=1, criterion=CK.PHOTO_CRITERION)
    _ckpt(train, 10)
    assert mgr.update_backup({"photo": 0.30})                     # the table is short: backed up without comparison
    _ckpt(train, 20)
    assert not mgr.update_backup({"photo": 0.35})                 # worse (higher): nothing changes
    assert not mgr.update_backup({"photo": 0.30})                 # a tie is no win
    assert CK.best_checkpoint(str(tmp_path)).endswith("ckpt-10.npz")
    _ckpt(train, 30)
    assert mgr.update_backup([0.25])                              # lower is better: 1 of 1 is more than half
    assert CK.best_checkpoint(str(tmp_path)).endswith("ckpt-30.npz")
    assert sorted(os.listdir(best)) == ["checkpoint", "ckpt-30.npz", "validation_perfs.csv"]
    assert open(os.path.join(best, "validation_perfs.csv")).read().splitlines()[0] == "photo,ckpt_name"
    # a best directory made with one criterion is refused by the other, not mixed
    seven = dict(zip(CK.METRIC_COLUMNS, (0.1, 0.2, 3.0, 0.2, 0.9, 0.95, 0.99)))
    with pytest.raises(ValueError, match="another criterion"):
        CK.BestCheckpointManager(train, best, keep_top_n=1).update_backup(seven)
    best7 = str(tmp_path / "best7")
    assert CK.BestCheckpointManager(train, best7, keep_top_n=1).update_backup(seven)
    with pytest.raises(ValueError, match="another criterion"):
        CK.BestCheckpointManager(train, best7, keep_top_n=1, criterion=CK.PHOTO_CRITERION).update_backup({"photo": 0.1})
    assert sorted(os.listdir(best7)) == ["checkpoint", "ckpt-30.npz", "validation_perfs.csv"]


def test_majority_is_more_than_half():
    from m4depth_amd import checkpoints as CK
    base = dict(zip(CK.METRIC_COLUMNS, (0.1, 0.2, 3.0, 0.2, 0.9, 0.95, 0.99)))
    for n_better in range(8):                                     # the default criterion: today's "more than 3 of 7"
        cand = dict(base)
        for m in CK.METRIC_COLUMNS[:n_better]:
            cand[m] = base[m] * (0.5 if m in CK.DEFAULT_CRITERION.lower else 1.01)
        assert CK.criterion_wins(CK.DEFAULT_CRITERION, cand, base) == CK.majority_wins(cand, base) == n_better
    two = CK.Criterion(("photo", "better"), ("photo",))           # an even count: 1 of 2 is no majority
    assert CK.criterion_wins(two, {"photo": 0.1, "better": 0.4}, {"photo": 0.2, "better": 0.5}) == 1


def test_write_validation_routes(tmp_path):
    """write_validation: seven metrics present -> today's files and criterion, plus the consistency line when given; absent ->
    best-N on photo."""
    import argparse
    from m4depth_amd import checkpoints as CK
    from m4depth_amd import main as M
    six = np.array([0.31, 0.42, 0.55, 0.12, 0.9, 0.95], np.float32)
    seven = np.array([0.1, 0.2, 3.0, 0.2, 0.9, 0.95, 0.99], np.float32)
    for name, metrics, cons in (("a", seven, None), ("b", seven, six), ("c", None, six)):
        d = str(tmp_path / name)
        _ckpt(os.path.join(d, "train"), 10)
        M.write_validation(argparse.Namespace(ckpt_dir=d, keep_top_n=1), metrics, cons)
        assert os.path.isfile(os.path.join(d, "validation-perfs.txt")) == (metrics is not None)
        assert os.path.isfile(os.path.join(d, "validation-consistency.txt")) == (cons is not None)
        header = open(os.path.join(d, "best", "validation_perfs.csv")).read().splitlines()[0]
        assert header == (",".join(CK.METRIC_COLUMNS) if metrics is not None else "photo") + ",ckpt_name"
        if cons is not None:
            assert open(os.path.join(d, "validation-consistency.txt")).read() == CK.format_validation_line(six)
    assert open(str(tmp_path / "a" / "validation-perfs.txt")).read() == open(str(tmp_path / "b" / "validation-perfs.txt")).read()


# ---- the two files ----------------------------------------------------------------------------------------------------------------
def test_file_round_trip(tmp_path):
    from m4depth_amd import consistency as CS
    assert CS.COLUMNS == ("photo", "photo_id", "better", "geo", "cover", "geo_cover")
    rng = np.random.default_rng(1)
    means = rng.uniform(0, 1, 6).astype(np.float32)
    p = CS.perfs_path(str(tmp_path), "midair")
    assert os.path.basename(p) == "perfs-consistency-midair.txt"
    CS.write_perfs(p, means)
    lines = open(p).read().splitlines()
    assert len(lines) == 6 and all(re.fullmatch(r"\d\.\d{18}e[+-]\d\d", l) for l in lines)         # perfs-<dataset>.txt's format
    ref = str(tmp_path / "seven.txt")
    np.savetxt(ref, means, fmt='%.18e', delimiter='\t', newline='\n')
    assert open(p, "rb").read() == open(ref, "rb").read()
    assert CS.read_perfs(p).tobytes() == means.tobytes()
    frames = [(0, 1, rng.uniform(0, 1, 6).astype(np.float32)), (0, 2, np.float32([1e-30, 0.0, 1.0, 3.4e38, 0.5, 1 / 3])),
              (3, 7, rng.uniform(0, 1, 6).astype(np.float32))]
    f = CS.frames_path(str(tmp_path), "recording")
    assert os.path.basename(f) == "consistency-frames-recording.txt"
    CS.write_frames(f, frames)
    text = open(f).read().splitlines()
    assert text[0] == "trajectory\tframe\tphoto\tphoto_id\tbetter\tgeo\tcover\tgeo_cover" and len(text) == 4
    assert all(len(l.split("\t")) == 8 for l in text)
    back = CS.read_frames(f)
    assert [(t, k) for t, k, _ in back] == [(0, 1), (0, 2), (3, 7)]
    assert all(a[2].tobytes() == b[2].tobytes() for a, b in zip(frames, back))
    with pytest.raises(ValueError, match="not a consistency-frames file"):
        CS.read_frames(p)


# ---- the entry point ----------------------------------------------------------------------------------------------------------------
def test_entry_points_are_bound_and_refuse_without_a_launch():
    from m4depth_amd import _lib
    from m4depth_amd._lib import lib
    assert _lib.ABI_VERSION == 6 and lib.m4d_abi_version() == 6
    for s in ("m4d_consistency_per_sample", "m4d_consistency_workspace_bytes"):
        assert s in _lib.EXPORTED_SYMBOLS
    fake = ctypes.c_void_p(4096)            # never dereferenced: validation fails first

    def call(b=1, h=8, w=8, rot_c=4, null=None, stride=None, ws=fake):
        p = [None if null == i else fake for i in range(13)]
        es = h * w if stride is None else stride
        return lib.m4d_consistency_per_sample(p[0], es, p[1], h * w, p[2], 3 * h * w, p[3], 3 * h * w, p[4], rot_c, p[5], p[6],
                                              p[7], p[8], p[9], b, h, w, None if null == 10 else ws, p[11], p[12], None)

    assert call(h=2) == 1 and call(w=2) == 1 and call(h=4097, w=4096) == 1 and call(b=0) == 1
    assert call(rot_c=5) == 1 and call(rot_c=0) == 1
    assert call(stride=63) == 1 and call(ws=ctypes.c_void_p(4100)) == 1
    for i in range(13):
        assert call(null=i) == 1, f"null pointer {i}"
    assert lib.m4d_consistency_workspace_bytes(1, 2, 8) == -1 and lib.m4d_consistency_workspace_bytes(1, 4097, 4096) == -1
    assert lib.m4d_consistency_workspace_bytes(0, 8, 8) == -1
    assert lib.m4d_consistency_workspace_bytes(2, 4096, 4096) == 2 * 256 * 256 * 48
    assert lib.m4d_consistency_workspace_bytes(3, 33, 35) == 3 * 9 * 48


def test_wrapper_refuses_cpu_tensors_and_bad_shapes():
    import torch
    from m4depth_amd import network_ops as nops
    z = lambda *s: torch.zeros(*s)
    m = torch.zeros(2, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"est: expected \[b,H,W,1\]"):
        nops.consistency_per_sample(z(2, 8, 8, 3), z(2, 8, 8, 1), z(2, 8, 8, 3), z(2, 8, 8, 3), z(2, 4), z(2, 3), z(2, 2), z(2, 2), m, m)
    with pytest.raises(ValueError, match="prev: expected"):
        nops.consistency_per_sample(z(2, 8, 8, 1), z(2, 8, 8, 1), z(2, 8, 8, 3), z(2, 8, 9, 3), z(2, 4), z(2, 3), z(2, 2), z(2, 2), m, m)
    with pytest.raises(ValueError, match="reset: expected a uint8 / bool"):
        nops.consistency_per_sample(z(2, 8, 8, 1), z(2, 8, 8, 1), z(2, 8, 8, 3), z(2, 8, 8, 3), z(2, 4), z(2, 3), z(2, 2), z(2, 2),
                                    m.float(), m)
    with pytest.raises((TypeError, RuntimeError), match="device tensor|MI355X only"):
        nops.consistency_per_sample(z(2, 8, 8, 1), z(2, 8, 8, 1), z(2, 8, 8, 3), z(2, 8, 8, 3), z(2, 4), z(2, 3), z(2, 2), z(2, 2), m, m)
