"""Host side of pose refinement (main.py --refine_pose): every refusal of the options, the defaults they fill in, the log's fold
order, the per-frame file's round trip, the entry points' argument refusals.  No GPU."""
import ctypes
import math
import re

import numpy as np
import pytest

STREAMS = ["--mode", "eval", "--dataset", "midair", "--eval_streams", "4"]
PREDICT = ["--mode", "predict", "--stream"]


def _parser_and_args(argv):
    from m4depth_amd import options as O
    parser = O.build_parser()
    return parser, parser.parse_args(argv)


def _check(argv):
    from m4depth_amd import options as O
    parser, args = _parser_and_args(argv)
    O.check_args(parser, args, world=1)
    return args


@pytest.mark.parametrize("bad, message", [
    (["--mode", "eval", "--refine_pose"], "--refine_pose needs --eval_streams B"),
    (["--mode", "validation", "--refine_pose"], "--refine_pose needs --eval_streams B"),
    (["--mode", "predict", "--refine_pose"], "--refine_pose needs --eval_streams B"),
    (["--mode", "predict", "--graph", "--refine_pose"], "--refine_pose needs --eval_streams B"),
    (["--mode", "train", "--refine_pose"], "--refine_pose needs --eval_streams B"),
    (["--mode", "finetune", "--refine_pose"], "--refine_pose needs --eval_streams B"),
    (STREAMS + ["--refine_pose_strides", "8,4"], "--refine_pose_strides needs --refine_pose"),
    (STREAMS + ["--refine_pose_iters", "3"], "--refine_pose_iters needs --refine_pose"),
    (STREAMS + ["--refine_pose_prior", "1", "1"], "--refine_pose_prior needs --refine_pose"),
    (PREDICT + ["--refine_pose_max", "0.1", "1"], "--refine_pose_max needs --refine_pose"),
    (STREAMS + ["--refine_pose", "--refine_pose_strides", "8,3"], "--refine_pose_strides: a comma list of powers of two"),
    (STREAMS + ["--refine_pose", "--refine_pose_strides", "0"], "--refine_pose_strides: a comma list of powers of two"),
    (STREAMS + ["--refine_pose", "--refine_pose_strides", "x"], "--refine_pose_strides: a comma list of powers of two"),
    (STREAMS + ["--refine_pose", "--refine_pose_strides", ""], "--refine_pose_strides: a comma list of powers of two"),
    (STREAMS + ["--refine_pose", "--refine_pose_iters", "0"], "--refine_pose_iters must be >= 1"),
    (STREAMS + ["--refine_pose", "--refine_pose_prior", "-1", "0"], "--refine_pose_prior LT LR must be >= 0"),
    (STREAMS + ["--refine_pose", "--refine_pose_prior", "0", "nan"], "--refine_pose_prior LT LR must be >= 0"),
    (STREAMS + ["--refine_pose", "--refine_pose_max", "0.1", "-1"], "--refine_pose_max METRES DEGREES must be >= 0"),
    (STREAMS + ["--refine_pose", "--height", "60", "--width", "64"], "multiples of the largest stride"),
    (STREAMS + ["--refine_pose", "--height", "16", "--width", "64"], "multiples of the largest stride"),
])
def test_refusals(bad, message, capsys):
    with pytest.raises(SystemExit) as e:
        _check(bad)
    assert e.value.code == 2 and re.search(message, capsys.readouterr().err), bad


def test_accepted_forms_and_their_defaults():
    from m4depth_amd import pose_refine as PR
    for argv in (STREAMS, ["--mode", "validation", "--dataset", "midair", "--eval_streams", "2"], PREDICT):
        for graph in ([], ["--graph"]):
            a = _check(argv + graph + ["--refine_pose"])
            assert a.refine_pose and a.refine_pose_strides == PR.DEFAULTS["strides"] == (8, 4, 2)
            assert a.refine_pose_iters == PR.DEFAULTS["iters"] == 4 and a.refine_pose_prior == PR.DEFAULTS["prior"] == (0.0, 0.0)
            assert a.refine_pose_max[0] == PR.DEFAULTS["caps"][0] and math.isclose(a.refine_pose_max[1], 0.5)
    a = _check(STREAMS + ["--refine_pose", "--refine_pose_strides", "4,2,1", "--refine_pose_iters", "5", "--refine_pose_prior", "10",
                          "100", "--refine_pose_max", "0", "0", "--consistency", "--height", "64", "--width", "64"])
    assert a.refine_pose_strides == (4, 2, 1) and a.refine_pose_iters == 5 and a.refine_pose_prior == (10.0, 100.0)
    assert a.refine_pose_max == (0.0, 0.0)


def test_parser_without_the_flag_leaves_every_other_default_unchanged():
    """The options add five destinations and change no other: the parsed defaults without them are the parent's."""
    _, args = _parser_and_args([])
    new = {"refine_pose": False, "refine_pose_strides": None, "refine_pose_iters": None, "refine_pose_prior": None,
           "refine_pose_max": None}
    got = vars(args)
    for k, v in new.items():
        assert got.pop(k) == v or (v is None and got.get(k) is None)
    # the parent's parser, destination by destination
    parent = dict(mode="eval", dataset="synthetic", db_path_config=None, records_path=None, rec_stride=None, rec_min_baseline=None,
                  rec_max_gap=None, no_augmentation=False, epochs=1, arch_depth=6, seq_len=4, db_seq_len=None, batch_size=1,
                  n_batches=2, height=None, width=None, ckpt_dir="ckpt", tf_checkpoint=None, seed=1234, graph=False, stream=False,
                  eval_streams=0, eval_streams_policy="lpt", consistency=False, host_input=False, save_dir=None, save_format=None,
                  save_panels=None, save_range=None, save_err_max=None, save_cloud=False, cloud_stride=None, cloud_frame=None,
                  learning_rate=1e-4, loss="supervised", photo_smooth=None, no_photo_automask=False, photo_scale=None,
                  photo_sources=None, save_every=0, summary_interval=1200, log_dir=None, max_keep=0, enable_validation=False,
                  val_records_path=None, val_dataset="kitti-raw", val_consistency=False, keep_top_n=1, no_DINL=False, no_SNCV=False,
                  no_time_recurr=False, no_feature_normalization=False, no_feature_subdivision=False, no_level_memory=False)
    assert got == parent
    a = _check(["--mode", "eval"])                                 # check_args without the flag fills nothing in
    assert a.refine_pose is False and a.refine_pose_strides is None and a.refine_pose_max is None


def test_refiner_defaults_live_in_one_place_and_are_checked():
    from m4depth_amd import pose_refine as PR
    r = PR.PoseRefiner(copy_estimate=False)
    for k, v in PR.DEFAULTS.items():
        assert getattr(r, k) == v
    assert PR.PoseRefiner(True, strides=(4, 1), iters=2).strides == (4, 1)
    for bad in (dict(strides=(3,)), dict(strides=()), dict(iters=0), dict(strides=(0,))):
        with pytest.raises(ValueError, match="powers of two"):
            PR.PoseRefiner(False, **bad)


def test_fold_order_and_file_round_trip(tmp_path):
    from m4depth_amd import pose_refine as PR
    from m4depth_amd import stream_eval as SE
    assert PR.fold is SE.fold_pose_refine and len(PR.COLUMNS) == 8
    lengths = [5, 1, 7, 3, 4]
    rng = np.random.default_rng(3)
    for policy in SE.POLICIES:
        sched = SE.schedule(lengths, 2, policy)
        n_steps, B = sched.cells.shape[:2]
        rows = rng.normal(size=(n_steps, B, 8)).astype(np.float32)
        for st in range(n_steps):                                    # a row that names its own cell
            for sl in range(B):
                rows[st, sl, 0], rows[st, sl, 1] = sched.cells[st, sl]
        frames = SE.fold_pose_refine(rows, sched.cells)
        # trajectory in csv order, frame in order, every frame but a trajectory's first, idle cells never
        assert [(t, f) for t, f, _ in frames] == [(t, f) for t, n in enumerate(lengths) for f in range(1, n)]
        assert all(row[0] == t and row[1] == f for t, f, row in frames)
        back = SE.fold_pose_refine(rows, sched.cells, traj_order=[4, 3, 2, 1, 0])
        assert [(t, f) for t, f, _ in back] == [(t, f) for t in (4, 3, 2, 1, 0) for f in range(1, lengths[t])]
    with pytest.raises(ValueError, match="disagree"):
        SE.fold_pose_refine(rows[..., :6], sched.cells)
    path = str(tmp_path / "frames.txt")
    PR.write_frames(path, frames)
    assert PR.frames_path("ck", "recording").endswith("pose-refine-frames-recording.txt")
    lines = open(path).read().splitlines()
    assert lines[0] == "trajectory\tframe\t" + "\t".join(PR.COLUMNS) and len(lines) == 1 + len(frames)
    got = PR.read_frames(path)
    assert len(got) == len(frames)
    for (t, f, row), (t2, f2, row2) in zip(frames, got):
        assert (t, f) == (t2, f2) and row.tobytes() == row2.tobytes()                  # %.9e: float32 round-trips
    with open(path, "w") as fh:
        fh.write("something else\n")
    with pytest.raises(ValueError, match="not a pose-refine-frames file"):
        PR.read_frames(path)


def test_entry_points_are_bound_and_refuse_without_a_launch():
    from m4depth_amd import _lib
    from m4depth_amd._lib import lib
    assert _lib.ABI_VERSION == 6 and lib.m4d_abi_version() == 6
    for s in ("m4d_pose_align_workspace_bytes", "m4d_pose_align_begin", "m4d_pose_align_iterate", "m4d_pose_align_end"):
        assert s in _lib.EXPORTED_SYMBOLS
    fake = ctypes.c_void_p(4096)            # never dereferenced: validation fails first
    odd = ctypes.c_void_p(4100)
    assert lib.m4d_pose_align_workspace_bytes(3, 24, 40) == (3 * 64 + 3 * 2 * 3 * 29) * 8
    assert lib.m4d_pose_align_workspace_bytes(0, 8, 8) == -1 and lib.m4d_pose_align_workspace_bytes(1, 2, 8) == -1
    assert lib.m4d_pose_align_workspace_bytes(1, 4097, 4096) == -1

    def begin(b=1, h=8, w=8, rot_c=4, null=None, ws=fake):
        p = [None if null == i else fake for i in range(2)]
        return lib.m4d_pose_align_begin(p[0], rot_c, p[1], b, h, w, None if null == 2 else ws, None)
    assert begin(rot_c=3) == 1 and begin(b=0) == 1 and begin(h=2) == 1 and begin(ws=odd) == 1
    assert all(begin(null=i) == 1 for i in range(3))

    def iterate(b=1, h=16, w=16, s=2, null=None, ws=fake, cs=None, es=None, huber=0.1, damping=0.0, pt=0.0, pr=0.0):
        p = [None if null == i else fake for i in range(7)]
        hw = (h // max(s, 1)) * (w // max(s, 1))
        return lib.m4d_pose_align_iterate(p[0], 3 * hw if cs is None else cs, p[1], 3 * hw, p[2], h * w if es is None else es, p[3],
                                          p[4], p[5], p[6], b, h, w, s, huber, damping, pt, pr, None if null == 7 else ws, None)
    assert all(iterate(null=i) == 1 for i in range(8))
    assert iterate(s=3) == 1 and iterate(s=0) == 1 and iterate(s=-2) == 1          # no power of two
    assert iterate(h=18, s=4) == 1 and iterate(w=18, s=4) == 1                     # no multiple of the stride
    assert iterate(s=8) == 1                                                      # a 2 x 2 level
    assert iterate(ws=odd) == 1 and iterate(cs=3 * 64 - 1) == 1 and iterate(es=255) == 1 and iterate(b=0) == 1
    assert iterate(huber=0.0) == 1 and iterate(damping=-1.0) == 1 and iterate(pt=-1.0) == 1 and iterate(pr=float("nan")) == 1

    def end(b=1, h=8, w=8, rot_c=4, null=None, ws=fake, cover=0.5, ct=0.1, cr=0.1):
        p = [None if null == i else fake for i in range(7)]
        return lib.m4d_pose_align_end(p[0], rot_c, p[1], p[2], p[3], b, h, w, cover, ct, cr, None if null == 7 else ws, p[4], p[5],
                                      p[6], None)
    assert all(end(null=i) == 1 for i in range(8))
    assert end(rot_c=3) == 1 and end(b=0) == 1 and end(ws=odd) == 1 and end(ct=-1.0) == 1 and end(cr=float("nan")) == 1


def test_wrappers_refuse_bad_shapes_and_cpu_tensors():
    import torch
    from m4depth_amd import network_ops as nops
    z = lambda *s: torch.zeros(*s)
    with pytest.raises(ValueError, match="quaternion rotations"):
        nops.pose_align_begin(z(2, 3), z(2, 3), 16, 16)
    with pytest.raises((TypeError, RuntimeError), match="device tensor|MI355X only"):
        nops.pose_align_begin(z(2, 4), z(2, 3), 16, 16)
    ws = torch.zeros(1024, dtype=torch.float64)
    m = torch.zeros(2, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"est_prev: expected \[b,H,W,1\]"):
        nops.pose_align_iterate(ws, z(2, 8, 8, 3), z(2, 8, 8, 3), z(2, 16, 16, 3), z(2, 2), z(2, 2), m, m, 2, 0.1)
    with pytest.raises(ValueError, match="cur: expected"):
        nops.pose_align_iterate(ws, z(2, 16, 16, 3), z(2, 8, 8, 3), z(2, 16, 16, 1), z(2, 2), z(2, 2), m, m, 2, 0.1)
    with pytest.raises(ValueError, match="reset: expected a uint8 / bool"):
        nops.pose_align_iterate(ws, z(2, 8, 8, 3), z(2, 8, 8, 3), z(2, 16, 16, 1), z(2, 2), z(2, 2), m.float(), m, 2, 0.1)
    with pytest.raises(ValueError, match="expected rot_out"):
        nops.pose_align_end(ws, z(2, 4), z(2, 3), m, m, 16, 16, 0.5, (0.1, 0.1), rows=z(2, 6))
