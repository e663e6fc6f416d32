"""Host side of the fused depth (main.py --fused, --save_fused): the option refusals and defaults, the writer's and FusedDepth's
refusals, the per-frame fold and its file -- nothing here launches a kernel."""
import os

import numpy as np
import pytest

FUSED_OPTIONS = {"fused", "fused_trunc", "fused_min_frames", "fused_slots_log2", "fused_window", "save_fused"}


def _refused(argv, capsys, match):
    from m4depth_amd import main as MAIN
    with pytest.raises(SystemExit) as e:
        MAIN.main(argv)
    assert e.value.code == 2
    assert match in capsys.readouterr().err


def _checked(argv):
    from m4depth_amd import main as MAIN
    from m4depth_amd import options as O
    parser = MAIN.build_parser()
    args = parser.parse_args(argv)
    O.check_save_args(parser, args)
    O.check_fused_args(parser, args)
    return args


def test_driver_refusals(tmp_path, capsys):
    out = str(tmp_path / "out")
    streams = ["--mode", "eval", "--dataset", "midair", "--eval_streams", "2"]
    _refused(["--mode", "eval", "--dataset", "midair", "--fused", "0.1"], capsys, "--fused needs --eval_streams B")
    _refused(["--mode", "validation", "--dataset", "midair", "--eval_streams", "2", "--fused", "0.1"], capsys, "--fused needs --eval_streams B")
    _refused(["--mode", "predict", "--fused", "0.1"], capsys, "--fused needs --eval_streams B")
    for opt in ("--fused_trunc", "--fused_min_frames", "--fused_slots_log2"):
        _refused(streams + [opt, "20"], capsys, opt + " needs --fused")
    _refused(streams + ["--fused_window", "2"], capsys, "--fused_window needs --fused or --save_fused")
    for bad in ("0", "-1", "nan", "inf"):
        _refused(streams + ["--fused", bad], capsys, "--fused VOXEL needs a finite edge length > 0")
    for bad in ("1", "9"):
        _refused(streams + ["--fused", "0.1", "--fused_trunc", bad], capsys, "--fused_trunc must be in 2..8")
    _refused(streams + ["--fused", "0.1", "--fused_min_frames", "0"], capsys, "--fused_min_frames must be >= 1")
    for bad in ("15", "27"):
        _refused(streams + ["--fused", "0.1", "--fused_slots_log2", bad], capsys, "--fused_slots_log2 must be in 16..26")
    _refused(streams + ["--fused", "0.1", "--fused_window", "0"], capsys, "--fused_window must be >= 1")
    predict = ["--mode", "predict", "--save_dir", out]
    _refused(predict + ["--save_fused"], capsys, "--save_fused needs --save_mesh")
    _refused(predict + ["--save_cloud", "--save_map", "0.1", "--save_fused"], capsys, "--save_fused needs --save_mesh")
    _refused(["--mode", "predict", "--save_mesh", "0.1", "--save_fused"], capsys, "--save_mesh needs --save_dir")
    _refused(predict + ["--save_mesh", "0.1", "--save_fused", "--fused_window", "0"], capsys, "--fused_window must be >= 1")
    assert not os.path.exists(out)


def test_driver_defaults_are_the_meshs():
    from m4depth_amd import main as MAIN
    from m4depth_amd import options as O
    a = _checked(["--mode", "eval", "--dataset", "midair", "--eval_streams", "8", "--fused", "0.1"])
    assert (a.fused, a.fused_trunc, a.fused_min_frames, a.fused_slots_log2, a.fused_window, a.save_fused) == (0.1, 4, 2, 22, None, False)
    m = _checked(["--mode", "predict", "--save_dir", "x", "--save_mesh", "0.1"])
    assert (a.fused_trunc, a.fused_min_frames, a.fused_slots_log2) == (m.mesh_trunc, m.mesh_min_frames, m.mesh_slots_log2)
    assert m.fused is None and m.save_fused is False and m.fused_window is None
    mesh = dict((p[0], p[1]) for p in O._TRAJECTORY_PRODUCTS)["save_mesh"]
    assert [c[1:] for c in O._FUSED_COMPANIONS] == [c[1:] for c in mesh]
    assert [c[0] for c in O._FUSED_COMPANIONS] == ["fused_trunc", "fused_min_frames", "fused_slots_log2"]
    a = _checked(["--mode", "eval", "--dataset", "midair", "--eval_streams", "8", "--graph", "--fused", "0.05", "--fused_trunc", "8",
                  "--fused_min_frames", "1", "--fused_slots_log2", "16", "--fused_window", "3"])
    assert (a.fused, a.fused_trunc, a.fused_min_frames, a.fused_slots_log2, a.fused_window) == (0.05, 8, 1, 16, 3)
    a = _checked(["--mode", "predict", "--save_dir", "x", "--save_mesh", "0.1", "--save_fused", "--fused_window", "2"])
    assert a.save_fused is True and a.fused_window == 2 and a.fused is None
    plain = vars(MAIN.build_parser().parse_args(["--mode", "predict"]))                           # absent from the namespace until given
    assert not FUSED_OPTIONS & set(plain)


def test_writer_and_fuser_refusals(tmp_path):
    from m4depth_amd.export import PredictionWriter
    from m4depth_amd.fusion import FusedDepth
    out = str(tmp_path)
    with pytest.raises(ValueError, match="save_fused needs save_mesh"):
        PredictionWriter(out, "kitti16", save_fused=True)
    with pytest.raises(ValueError, match="fused_window needs save_fused"):
        PredictionWriter(out, "kitti16", save_mesh=0.1, fused_window=2)
    with pytest.raises(ValueError, match="fused_window needs save_fused"):
        PredictionWriter(out, "kitti16", save_mesh=0.1, save_fused=True, fused_window=0)
    w = PredictionWriter(out, "kitti16", save_mesh=0.1, save_fused=True, fused_window=2)
    assert (w.save_fused, w.fused_window, w.fused_pixels, w.fused_cap) == (True, 2, 0, 0)
    w.close()
    w = PredictionWriter(out, "kitti16", save_mesh=0.1)
    assert (w.save_fused, w.fused_window) == (False, None)
    w.close()
    assert not os.listdir(out)
    for bad in (dict(voxel=0.0), dict(voxel=float("nan")), dict(voxel=float("inf")), dict(trunc=1), dict(trunc=9), dict(min_frames=0),
                dict(slots_log2=5), dict(slots_log2=27), dict(near=0.0), dict(far=1.0), dict(window=0)):
        with pytest.raises(ValueError):
            FusedDepth(**dict(dict(voxel=0.1), **bad))
    fd = FusedDepth(0.1)
    assert (fd.voxel, fd.trunc, fd.min_frames, fd.slots_log2, fd.near, fd.far, fd.window) == (float(np.float32(0.1)), 4, 2, 22, 1.0, 80.0, None)
    assert fd.stats() == []


def test_fold_and_frames_file(tmp_path):
    """The per-frame rows follow the sequential walk whatever slot and step a frame ran in."""
    from m4depth_amd import fusion as FU
    from m4depth_amd import stream_eval as SE
    rng = np.random.default_rng(2)
    # two slots, four steps: trajectory 1 (3 frames) in slot 0, trajectory 0 (2 frames) then trajectory 2 (1 frame) in slot 1
    cells = np.array([[[1, 0], [0, 0]], [[1, 1], [0, 1]], [[1, 2], [2, 0]], [[-1, -1], [-1, -1]]])
    counted = np.array([[0, 0], [1, 1], [1, 0], [0, 0]], np.uint8)
    rows, rows_f = rng.random((4, 2, 7)).astype(np.float32), rng.random((4, 2, 7)).astype(np.float32)
    hits = rng.integers(0, 100, (4, 2))
    frames = SE.fold_fused(rows, rows_f, hits, counted, cells, 100)
    assert [(t, f) for t, f, _ in frames] == [(0, 1), (1, 1), (1, 2)]
    for (t, f, row), (st, sl) in zip(frames, ((1, 1), (1, 0), (2, 0))):
        assert row.dtype == np.float32 and row.tolist() == [np.float32(hits[st, sl]) / np.float32(100), rows[st, sl, 0], rows_f[st, sl, 0]]
    with pytest.raises(ValueError, match="disagree"):
        SE.fold_fused(rows, rows_f[:3], hits, counted, cells, 100)
    path = str(tmp_path / "fused-frames-x.txt")
    FU.write_frames(path, frames)
    back = FU.read_frames(path)
    assert [(t, f) for t, f, _ in back] == [(t, f) for t, f, _ in frames]
    assert all(np.array_equal(a[2], b[2]) for a, b in zip(back, frames))
    assert open(path).readline() == "trajectory\tframe\tcoverage\tabs_rel\tabs_rel_fused\n"
    FU.write_perfs(str(tmp_path / "p.txt"), rows[0, 0])
    assert np.array_equal(FU.read_perfs(str(tmp_path / "p.txt")), rows[0, 0])
    with pytest.raises(ValueError, match="not a fused-frames file"):
        FU.read_frames(str(tmp_path / "p.txt"))
    assert FU.perfs_path("c", "midair") == os.path.join("c", "perfs-fused-midair.txt")
    assert FU.frames_path("c", "midair") == os.path.join("c", "fused-frames-midair.txt")
