"""The training workflow's host logic, no GPU: the best-N checkpoint manager (callbacks.py:173-240), validation-perfs.txt,
checkpoint retention, eval / predict preferring <ckpt_dir>/best, the joint KITTI + Mid-Air batch sampler of finetune_kitti,
the driver's refusals, and the C ABI of the training step log."""
import ctypes
import os

import numpy as np
import pytest
import torch

from m4depth_amd import checkpoints as CK
from m4depth_amd import finetune_kitti as FK
from m4depth_amd import main as M

COLS = CK.METRIC_COLUMNS


def _ckpt(d, step, value=0.0):
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, f"ckpt-{step}.npz")
    np.savez(path, w=np.full(3, value, np.float32))
    with open(path[:-4] + ".opt.pt", "w") as fh:
        fh.write(str(step))
    return path


def _perfs(abs_rel, sq_rel, rmse, rmsel, a1, a2, a3):
    return dict(zip(COLS, (abs_rel, sq_rel, rmse, rmsel, a1, a2, a3)))


BASE = _perfs(0.2, 2.0, 6.0, 0.3, 0.7, 0.8, 0.9)


@pytest.fixture
def dirs(tmp_path):
    return str(tmp_path / "train"), str(tmp_path / "best")


def _names(mgr):
    return [r["ckpt_name"] for r in mgr.read_table()]


def _latest_named(best):
    with open(os.path.join(best, "checkpoint")) as fh:
        return fh.read()


def test_first_backup(dirs):
    train, best = dirs
    _ckpt(train, 10)
    mgr = CK.BestCheckpointManager(train, best, keep_top_n=1)
    assert mgr.update_backup(BASE)
    assert _names(mgr) == ["ckpt-10.npz"]
    assert sorted(os.listdir(best)) == ["checkpoint", "ckpt-10.npz", "ckpt-10.opt.pt", "validation_perfs.csv"]
    with open(os.path.join(best, "validation_perfs.csv")) as fh:
        assert fh.readline().strip() == "abs_rel,sq_rel,rmse,rmsel,a1,a2,a3,ckpt_name"
    row = mgr.read_table()[0]
    assert [float(row[c]) for c in COLS] == [BASE[c] for c in COLS]


def test_checkpoint_file_names_the_latest_backup(dirs):
    train, best = dirs
    _ckpt(train, 10)
    mgr = CK.BestCheckpointManager(train, best, keep_top_n=2)
    mgr.update_backup(BASE)
    _ckpt(train, 20)
    mgr.update_backup(BASE)                              # filling: no comparison, even when no better
    assert _latest_named(best) == 'model_checkpoint_path: "ckpt-20.npz"\nall_model_checkpoint_paths: "ckpt-20.npz"\n'
    assert CK.best_checkpoint(os.path.dirname(best)) == os.path.join(best, "ckpt-20.npz")


def test_fills_up_to_keep_top_n_without_comparison(dirs):
    train, best = dirs
    mgr = CK.BestCheckpointManager(train, best, keep_top_n=3)
    worse = _perfs(0.9, 9.0, 9.0, 0.9, 0.1, 0.1, 0.1)
    for i, p in enumerate((BASE, worse, worse)):
        _ckpt(train, 10 * (i + 1))
        assert mgr.update_backup(p)
    assert _names(mgr) == ["ckpt-10.npz", "ckpt-20.npz", "ckpt-30.npz"]
    _ckpt(train, 40)
    assert not mgr.update_backup(_perfs(0.95, 9.5, 9.5, 0.95, 0.05, 0.05, 0.05))     # full now: loses everywhere
    assert _names(mgr) == ["ckpt-10.npz", "ckpt-20.npz", "ckpt-30.npz"]
    assert not os.path.exists(os.path.join(best, "ckpt-40.npz"))


def test_majority_replaces_the_first_beaten_row_and_its_files(dirs):
    train, best = dirs
    mgr = CK.BestCheckpointManager(train, best, keep_top_n=2)
    good = _perfs(0.1, 1.0, 3.0, 0.1, 0.9, 0.95, 0.99)
    _ckpt(train, 10)
    mgr.update_backup(good)                               # row 0: hard to beat
    _ckpt(train, 20)
    mgr.update_backup(BASE)                               # row 1
    # 4 of 7 better than row 1 (rmse, rmsel, abs_rel, sq_rel), none better than row 0: row 1 goes
    cand = _perfs(0.19, 1.9, 5.9, 0.29, 0.6, 0.7, 0.8)
    assert CK.majority_wins(cand, BASE) == 4 and CK.majority_wins(cand, good) == 0
    _ckpt(train, 30)
    assert mgr.update_backup(cand)
    assert _names(mgr) == ["ckpt-10.npz", "ckpt-30.npz"]
    assert not os.path.exists(os.path.join(best, "ckpt-20.npz")) and not os.path.exists(os.path.join(best, "ckpt-20.opt.pt"))
    assert os.path.isfile(os.path.join(best, "ckpt-30.npz")) and os.path.isfile(os.path.join(best, "ckpt-30.opt.pt"))
    assert "ckpt-30.npz" in _latest_named(best)
    # a candidate beating BOTH rows replaces the FIRST one in file order (the reference's quirk), not the worst
    _ckpt(train, 40)
    assert mgr.update_backup(_perfs(0.01, 0.1, 0.5, 0.01, 0.99, 0.999, 0.9999))
    assert _names(mgr) == ["ckpt-30.npz", "ckpt-40.npz"]
    assert not os.path.exists(os.path.join(best, "ckpt-10.npz"))


def test_exactly_three_wins_change_nothing(dirs):
    train, best = dirs
    mgr = CK.BestCheckpointManager(train, best, keep_top_n=1)
    _ckpt(train, 10)
    mgr.update_backup(BASE)
    before = open(os.path.join(best, "validation_perfs.csv")).read()
    cand = _perfs(0.3, 3.0, 7.0, 0.4, 0.71, 0.81, 0.91)    # a1 / a2 / a3 better, the 4 errors worse: 3 wins
    assert CK.majority_wins(cand, BASE) == 3
    _ckpt(train, 20)
    assert not mgr.update_backup(cand)
    assert open(os.path.join(best, "validation_perfs.csv")).read() == before
    assert sorted(os.listdir(best)) == ["checkpoint", "ckpt-10.npz", "ckpt-10.opt.pt", "validation_perfs.csv"]
    assert "ckpt-10.npz" in _latest_named(best)
    tie = dict(BASE)                                      # ties are no wins
    assert CK.majority_wins(tie, BASE) == 0


def test_validation_perfs_line_format(tmp_path):
    m = [0.123456, 1.5, 4.25, 0.19999, 0.9, 0.95, 0.987654]
    assert CK.format_validation_line(m) == "0.1235\t\t1.5000\t\t4.2500\t\t0.2000\t\t0.9000\t\t0.9500\t\t0.9877\t\t\n"
    CK.append_validation_perfs(str(tmp_path), m)
    CK.append_validation_perfs(str(tmp_path), m)
    lines = open(tmp_path / "validation-perfs.txt").read().splitlines()
    assert len(lines) == 2 and lines[0].split("\t\t")[:7] == ["0.1235", "1.5000", "4.2500", "0.2000", "0.9000", "0.9500", "0.9877"]


def test_max_keep_prunes_the_oldest(tmp_path):
    d = str(tmp_path / "train")
    for step in (5, 10, 40, 20, 30):
        _ckpt(d, step)
    assert CK.prune_checkpoints(d, 0) == [] and CK.checkpoint_steps(d) == [5, 10, 20, 30, 40]
    assert CK.prune_checkpoints(d, 3) == [5, 10]
    assert CK.checkpoint_steps(d) == [20, 30, 40]
    assert sorted(os.listdir(d)) == sorted(f"ckpt-{s}{e}" for s in (20, 30, 40) for e in (".npz", ".opt.pt"))
    assert CK.latest_checkpoint(d) == (os.path.join(d, "ckpt-40.npz"), 40)


def _args(tmp_path, mode, *extra):
    return M.build_parser().parse_args([f"--mode={mode}", f"--ckpt_dir={tmp_path}", "--arch_depth=2", *extra])


@pytest.mark.parametrize("mode", ["eval", "predict", "validation"])
def test_inference_weights_prefer_best(tmp_path, capsys, mode):
    _ckpt(str(tmp_path / "train"), 50, value=5.0)
    args = _args(tmp_path, mode)
    w = M.load_weights(args, M.ablation_from_args(args))
    assert float(w["w"][0]) == 5.0 and "train/ckpt-50.npz" in capsys.readouterr().out       # no best/ yet: today's behaviour
    _ckpt(str(tmp_path / "train"), 30, value=3.0)
    mgr = CK.BestCheckpointManager(str(tmp_path / "train"), str(tmp_path / "best"), 1)
    os.remove(tmp_path / "train" / "ckpt-50.npz")
    mgr.update_backup(BASE)                                                                    # best/ckpt-30
    _ckpt(str(tmp_path / "train"), 50, value=5.0)
    w = M.load_weights(args, M.ablation_from_args(args))
    out = capsys.readouterr().out
    if mode == "validation":                   # validation judges the latest TRAINING checkpoint (main.py:113-116)
        assert float(w["w"][0]) == 5.0 and "train/ckpt-50.npz" in out
    else:
        assert float(w["w"][0]) == 3.0 and "best/ckpt-30.npz" in out


def test_training_resumes_from_train_not_best(tmp_path):
    _ckpt(str(tmp_path / "train"), 30)
    CK.BestCheckpointManager(str(tmp_path / "train"), str(tmp_path / "best"), 1).update_backup(BASE)
    _ckpt(str(tmp_path / "train"), 60)
    assert M.latest_checkpoint(_args(tmp_path, "train")) == (str(tmp_path / "train" / "ckpt-60.npz"), 60)


class _Source:
    def __init__(self, tag, n):
        self.tag, self.n = tag, n

    def __iter__(self):
        return iter([{"src": self.tag, "i": i, "rows": [self.tag] * 3} for i in range(self.n)])


def test_joint_sampler_deterministic_balanced_unmixed():
    def draw(seed, n):
        j = FK.JointBatches([_Source("kitti", 3), _Source("midair", 5)], seed)
        return list(j.epoch(n)), j
    a, ja = draw(7, 2000)
    b, _ = draw(7, 2000)
    c, _ = draw(8, 2000)
    assert [x["src"] for x in a] == [x["src"] for x in b]
    assert [x["src"] for x in a] != [x["src"] for x in c]
    frac = np.mean([x["src"] == "kitti" for x in a])
    assert 0.46 < frac < 0.54, frac                           # 2000 Bernoulli(0.5): sd 0.011
    for x in a:                                               # a batch comes whole from one source
        assert x["rows"] == [x["src"]] * 3
    assert ja.drawn == [0 if x["src"] == "kitti" else 1 for x in a]
    # each source repeats forever, in its own order
    ks = [x["i"] for x in a if x["src"] == "kitti"]
    assert ks[:7] == [0, 1, 2, 0, 1, 2, 0]
    # epochs continue the same stream
    j = FK.JointBatches([_Source("kitti", 3), _Source("midair", 5)], 7)
    two = list(j.epoch(900)) + list(j.epoch(1100))
    assert [x["src"] for x in two] == [x["src"] for x in a]


def test_joint_sampler_refuses_an_empty_source():
    j = FK.JointBatches([_Source("kitti", 0), _Source("midair", 0)], 0)
    with pytest.raises(ValueError):
        list(j.epoch(3))


def test_finetune_epoch_arithmetic():
    assert FK.finetune_schedule(100) == (200, 101)            # 20000 // 200 + 1
    assert FK.finetune_schedule(3000) == (6000, 4)
    assert FK.finetune_schedule(2, 4) == (4, 2)
    assert FK.finetune_schedule(5, 4) == (10, 1)
    with pytest.raises(ValueError):
        FK.finetune_schedule(0)
    assert FK.build_parser().parse_args([]).finetune_steps == 20000


def test_parser_defaults():
    a = M.build_parser().parse_args([])
    assert (a.summary_interval, a.max_keep, a.keep_top_n, a.val_dataset, a.enable_validation) == (1200, 0, 1, "kitti-raw", False)


@pytest.mark.parametrize("argv,world,msg", [
    (["--mode=train", "--enable_validation"], 1, "--val_records_path"),
    (["--mode=train", "--enable_validation", "--val_records_path=r", "--db_path_config=c"], 2, "several ranks"),
    (["--mode=train", "--graph"], 2, "several ranks"),
    (["--mode=finetune", "--graph"], 2, "several ranks"),
    (["--mode=train", "--keep_top_n=0"], 1, "--keep_top_n"),
    (["--mode=train", "--max_keep=-1"], 1, "--max_keep"),
    (["--mode=train", "--summary_interval=0"], 1, "--summary_interval"),
])
def test_parser_refusals(monkeypatch, capsys, argv, world, msg):
    monkeypatch.setenv("WORLD_SIZE", str(world))
    with pytest.raises(SystemExit) as e:
        M.main(argv)
    assert e.value.code == 2 and msg in capsys.readouterr().err


def test_finetune_parser_refusals(monkeypatch, capsys):
    monkeypatch.setenv("WORLD_SIZE", "1")
    with pytest.raises(SystemExit) as e:
        FK.main(["--enable_validation"])
    assert e.value.code == 2 and "--records_path" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        FK.main(["--records_path=r", "--db_path_config=c", "--enable_validation"])
    assert e.value.code == 2 and "--val_records_path" in capsys.readouterr().err
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        FK.main(["--records_path=r", "--db_path_config=c", "--graph"])
    assert e.value.code == 2 and "several ranks" in capsys.readouterr().err


def test_graph_batches_must_reset_on_frame_zero_only():
    b, T = 2, 4
    data = {"depth": torch.zeros(b, T, 8, 8, 1), "RGB_im": torch.zeros(b, T, 8, 8, 3), "rot": torch.zeros(b, T, 4),
            "trans": torch.zeros(b, T, 3), "camera": {"f": torch.zeros(b, 2), "c": torch.zeros(b, 2)},
            "new_traj": torch.tensor([[True, False, False, False]] * b)}
    M.check_graph_batch(data)
    geo = M._geometry(data)
    M.check_graph_batch(data, geo)
    bad = dict(data, new_traj=torch.tensor([[True, False, True, False]] * b))
    with pytest.raises(ValueError, match="frame 0"):
        M.check_graph_batch(bad, geo)
    with pytest.raises(ValueError, match="frame 0"):
        M.check_graph_batch(dict(data, new_traj=torch.tensor([[True, False, False, False], [False] * 4])), geo)
    other = dict(data, RGB_im=torch.zeros(b, T, 8, 16, 3))
    with pytest.raises(ValueError, match="geometry"):
        M.check_graph_batch(other, geo)


def test_train_log_abi_declared_bound_exported():
    from m4depth_amd import _lib
    import test_library as TL
    syms = TL.header_symbols()
    for s in ("m4d_train_log_step", "m4d_train_log_workspace_bytes"):
        assert s in syms and s in _lib.EXPORTED_SYMBOLS and hasattr(ctypes.CDLL(_lib.LIB_PATH), s)
    assert _lib.lib.m4d_train_log_workspace_bytes() >= 512 * 2 * 8


def test_train_log_argument_validation_without_gpu():
    from m4depth_amd._lib import lib
    f = ctypes.c_void_p(4096)                                 # never dereferenced: validation fails first
    ok = dict(loss=f, gt=f, gt_stride=64, est=f, b=1, H=8, W=8, h=4, w=4, log=f, log_rows=4, counter=f, first_bad=f,
              workspace=f)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.m4d_train_log_step(a["loss"], a["gt"], a["gt_stride"], a["est"], a["b"], a["H"], a["W"], a["h"], a["w"],
                                      a["log"], a["log_rows"], a["counter"], a["first_bad"], a["workspace"], None)
    for name in ("loss", "gt", "est", "log", "counter", "first_bad", "workspace"):
        assert call(**{name: None}) == 1, name
    for name in ("b", "H", "W", "h", "w", "log_rows"):
        assert call(**{name: 0}) == 1, name
        assert call(**{name: -1}) == 1, name
    assert call(gt_stride=63) == 1                            # an image stride below H * W
    assert call(gt_stride=-64) == 1
