"""The training workflow on the MI355X: the device-side step log of the replayed training step (m4d_train_log_step), eager
vs ``--graph`` training through the driver, TerminateOnNaN, and the reference's recipe end to end (train with validation and
best-N, finetune on the joint KITTI + Mid-Air stream, eval from best/) on miniature datasets.

The NaN runs poison one batch with a NaN depth pixel.  The loss kernels clip ground truth and estimate with fmaxf / fminf,
which drop a NaN (tf.clip_by_value propagates it), so the tests wrap m4depth_loss to carry the ground truth's NaN into the
loss scalar as the reference's loss would -- the NaN never enters a kernel's arithmetic."""
import json
import os
import re
import shutil

import numpy as np
import pytest
import torch

from helpers import make_fake_dataset, to_dev
from m4depth_amd import synthetic

pytestmark = pytest.mark.gpu

L, H, W, T, B = 2, 64, 64, 3, 2


def _data(seed):
    samples, cam = synthetic.make_sequence(B, T, H, W, seed=seed)
    data = {k: np.stack([s[k] for s in samples], axis=1) for k in ("RGB_im", "depth", "rot", "trans", "new_traj")}
    data["camera"] = cam
    return data


def _model(dev):
    import m4depth_amd as M
    from m4depth_amd import training as TR
    wts = synthetic.init_weights(nbre_levels=L, seed=5, dscv_range=2, sncv_range=2)
    model = M.M4Depth(nbre_levels=L, is_training=True, dscv_range=2, sncv_range=2).load_numpy_weights(wts, dev)
    return TR.set_trainable(model), TR


def _rmse_log_f64(gt, est):
    """train_step's RMSE_log in float64: est resized to gt's size by tf.image.resize NEAREST (m4d_resize_nearest's index
    rule, in float32 as the kernel computes it), clamps, mask on the log (metrics.py:24-28)."""
    b, Hg, Wg = gt.shape[:3]
    h, w = est.shape[1:3]
    iy = np.minimum(np.floor((np.arange(Hg, dtype=np.float32) + np.float32(0.5)) * (np.float32(h) / np.float32(Hg))), h - 1)
    ix = np.minimum(np.floor((np.arange(Wg, dtype=np.float32) + np.float32(0.5)) * (np.float32(w) / np.float32(Wg))), w - 1)
    e = est[:, iy.astype(int)][:, :, ix.astype(int)].astype(np.float64).reshape(b, Hg, Wg)
    g = gt.astype(np.float64).reshape(b, Hg, Wg)
    g = np.clip(g, 0.0, 80.0)
    e = np.clip(e, 0.001, 80.0)
    lg, le = np.log(g + 1e-6), np.log(e + 1e-6)
    m = lg > 1e-6
    return np.sqrt(np.sum(np.where(m, (lg - le) ** 2, 0.0)) / max(m.sum(), 1))


def test_log_kernel_rows_equal_the_replayed_steps(dev):
    model, TR = _model(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4, eps=1e-7, capturable=True)
    model.compile(optimizer=opt)
    batches = [to_dev(_data(40 + i), dev) for i in range(4)]
    log = TR.TrainStepLog(8, dev)
    runner = TR.GraphedTrainStep(model, batches[0], opt, warmup=1, step_log=log)
    rows0, bad = log.read()
    assert rows0.shape == (1, 2) and bad == -1                      # the warm-up step is logged
    want = []
    for data in batches[1:]:
        loss, est = runner(data)
        gt = data["depth"][:, -1].cpu().numpy()
        want.append((loss.cpu().numpy().reshape(1), _rmse_log_f64(gt, est.cpu().numpy())))
    rows, bad = log.read()
    assert bad == -1 and rows.shape == (3, 2) and int(log.counter.item()) == 4
    for (loss, rmse), row in zip(want, rows):
        assert row[:1].view(np.uint32) == loss.view(np.uint32), (row, loss)     # the graph's loss tensor, bit for bit
        assert abs(float(row[1]) - rmse) <= 1e-5 * rmse, (row[1], rmse)
        assert np.isfinite(row).all() and row[1] > 0
    # the same step log on the same tensors: deterministic
    again = TR.TrainStepLog(2, dev)
    for _ in range(2):
        again.record(runner.loss, runner.static["depth"][:, -1], runner.est)
    r2, _ = again.read()
    assert r2.view(np.uint32).tolist() == [rows[-1].view(np.uint32).tolist()] * 2


def test_log_kernel_latches_the_first_non_finite_loss(dev):
    from m4depth_amd import training as TR
    d = to_dev(_data(50), dev)
    gt = d["depth"][:, -1]
    est = torch.full((B, H // 2, W // 2, 1), 10.0, device=dev)
    log = TR.TrainStepLog(4, dev)                                   # a ring: 6 steps through 4 rows, read twice
    losses = [1.0, 2.0, float("nan"), 3.0, float("inf"), 4.0]
    for i, v in enumerate(losses):
        log.record(torch.tensor([v], device=dev), gt, est)
        if i == 1:
            rows, bad = log.read()
            assert bad == -1 and rows[:, 0].tolist() == [1.0, 2.0]
    rows, bad = log.read()
    assert bad == 2 and int(log.counter.item()) == 6
    assert np.isnan(rows[0, 0]) and rows[1:, 0].tolist() == [3.0, float("inf"), 4.0]
    # the metric of the same gt / est every step
    assert np.allclose(rows[:, 1], _rmse_log_f64(gt.cpu().numpy(), est.cpu().numpy()), rtol=1e-5)
    # a NaN ground-truth pixel is masked out, as in metrics.py
    gt_nan = d["depth"].clone()
    gt_nan[0, -1, 3, 4, 0] = float("nan")
    log2 = TR.TrainStepLog(1, dev)
    log2.record(torch.tensor([1.0], device=dev), gt_nan[:, -1], est)
    r, bad = log2.read()
    assert bad == -1 and np.isfinite(r).all()


def _losses(out):
    return [(int(m.group(1)), float(m.group(2))) for m in re.finditer(r"^step (\d+): loss (\S+)", out, re.M)]


SYN = ["--arch_depth", "2", "--height", str(H), "--width", str(W), "--seq_len", str(T), "--batch_size", str(B),
       "--learning_rate", "1e-3"]


def test_eager_and_graph_driver_walk_the_same_losses(dev, tmp_path, capsys):
    from m4depth_amd import main as MAIN
    traj = []
    for graph in (False, True):
        ck = str(tmp_path / ("graph" if graph else "eager"))
        argv = ["--mode", "train", "--n_batches", "5", "--ckpt_dir", ck, "--summary_interval", "2"] + SYN
        assert MAIN.main(argv + (["--graph"] if graph else [])) == 0
        out = capsys.readouterr().out
        traj.append(_losses(out))
        assert os.path.isfile(os.path.join(ck, "train", "ckpt-5.npz")) and os.path.isfile(os.path.join(ck, "train", "ckpt-5.opt.pt"))
        assert re.search(r"RMSE_log \d", out)
    assert [s for s, _ in traj[0]] == [s for s, _ in traj[1]] == [1, 2, 3, 4, 5]
    np.testing.assert_allclose([l for _, l in traj[1]], [l for _, l in traj[0]], rtol=2e-3)


def _poisoned_epochs(dev, epochs=2, per_epoch=2, bad=(1, 0)):
    """epoch -> device batches of synthetic data; batch bad[1] of epoch bad[0] carries a NaN depth pixel."""
    def epoch(e):
        for i in range(per_epoch):
            d = to_dev(_data(60 + e * per_epoch + i), dev)
            if (e, i) == bad:
                d["depth"][0, -1, 5, 7, 0] = float("nan")
            yield d
    return epochs, epoch


def _nan_propagating_loss(TR, monkeypatch):
    loss_fn = TR.m4depth_loss

    def loss(gts, preds, depth_type="map"):
        return loss_fn(gts, preds, depth_type) + gts[-1]["depth"].sum() * 0.0       # NaN iff the ground truth holds one
    monkeypatch.setattr(TR, "m4depth_loss", loss)


@pytest.mark.parametrize("graph", [False, True])
def test_nan_stops_training_and_saves_nothing_of_its_epoch(dev, tmp_path, capsys, monkeypatch, graph):
    from m4depth_amd import main as MAIN
    from m4depth_amd import training as TR
    monkeypatch.setattr(MAIN, "default_epochs", lambda args, rank, world, dev_: _poisoned_epochs(dev))
    _nan_propagating_loss(TR, monkeypatch)
    ck = str(tmp_path / "ck")
    argv = ["--mode", "train", "--ckpt_dir", ck, "--save_every", "2"] + SYN + (["--graph"] if graph else [])
    assert MAIN.main(argv) == 1
    out = capsys.readouterr().out
    assert "step 3: non-finite loss" in out
    assert sorted(os.listdir(os.path.join(ck, "train"))) == ["ckpt-2.npz", "ckpt-2.opt.pt"]
    assert [s for s, _ in _losses(out)] == [1, 2]                  # the bad step and those replayed after it are discarded
    with np.load(os.path.join(ck, "train", "ckpt-2.npz")) as z:
        assert all(np.isfinite(z[k]).all() for k in z.files)


def _stationary_epochs(dev, epochs=2, per_epoch=2):
    """epoch -> device batches of synthetic data; in the LAST batch of the first epoch sample 0 does not move on the last
    frame (a hovering drone, a car at a traffic light).  Every input is finite."""
    def epoch(e):
        for i in range(per_epoch):
            d = to_dev(_data(60 + e * per_epoch + i), dev)
            if (e, i) == (0, per_epoch - 1):
                d["trans"][0, -1] = 0.0
            yield d
    return epochs, epoch


@pytest.mark.parametrize("graph", [False, True])
def test_a_stationary_frame_never_reaches_a_checkpoint(dev, tmp_path, capsys, monkeypatch, graph):
    """A stationary sample leaves the loss finite (DESIGN.md "Degenerate inputs", R2) and the gradients NaN (R6), so the
    optimizer step makes the weights NaN and only the NEXT step's loss shows it.  Here the poisoning step is the last of an
    epoch and a checkpoint is due right after it (--save_every 2): the driver checks the parameters where it saves, writes
    nothing and exits with status 1; no file with a non-finite value is ever on disk."""
    from m4depth_amd import main as MAIN
    monkeypatch.setattr(MAIN, "default_epochs", lambda args, rank, world, dev_: _stationary_epochs(dev))
    ck = str(tmp_path / "ck")
    argv = ["--mode", "train", "--ckpt_dir", ck, "--save_every", "2"] + SYN + (["--graph"] if graph else [])
    assert MAIN.main(argv) == 1
    out = capsys.readouterr().out
    steps = _losses(out)
    assert [s for s, _ in steps] == [1, 2] and all(np.isfinite(l) for _, l in steps), out    # the poisoning step's loss is finite
    assert "step 2: non-finite parameters" in out and "saved" not in out
    train = os.path.join(ck, "train")
    written = sorted(os.listdir(train)) if os.path.isdir(train) else []
    for name in written:
        if name.endswith(".npz"):
            with np.load(os.path.join(train, name)) as z:
                assert all(np.isfinite(z[k]).all() for k in z.files), name
    assert written == [], written


def _tree(tmp_path):
    """Fake Mid-Air (training) and KITTI (finetuning and validation) sets with one datasets_location.json, and the records
    tree finetune_kitti reads (<records>/kitti-raw-filtered/train_data, <records>/midair/train_data)."""
    root = str(tmp_path)
    db_m, rec_m = make_fake_dataset(os.path.join(root, "midair"), "midair", n_traj=2, n_frames=9, size=(H, W), seed=1)
    db_k, rec_k = make_fake_dataset(os.path.join(root, "kitti"), "kitti-raw", n_traj=2, n_frames=8, size=(H, W), seed=2)
    cfg = os.path.join(root, "datasets_location.json")
    with open(cfg, "w") as fh:
        json.dump({"midair": db_m, "kitti-raw": db_k}, fh)
    recs = os.path.join(root, "records")
    shutil.copytree(rec_k, os.path.join(recs, "kitti-raw-filtered", "train_data"))
    shutil.copytree(rec_m, os.path.join(recs, "midair", "train_data"))
    return cfg, rec_m, rec_k, recs


def test_reference_recipe_end_to_end(dev, tmp_path, capsys):
    from m4depth_amd import main as MAIN
    from m4depth_amd import finetune_kitti as FK
    cfg, rec_m, rec_k, recs = _tree(tmp_path)
    ck = str(tmp_path / "ckpt")
    size = ["--arch_depth", "2", "--height", str(H), "--width", str(W), "--batch_size", "2", "--ckpt_dir", ck,
            "--db_path_config", cfg]
    val = ["--enable_validation", "--val_records_path", rec_k, "--keep_top_n", "2"]
    # 1a: Mid-Air with validation after every epoch, graph-replayed
    assert MAIN.main(["--mode", "train", "--dataset", "midair", "--records_path", rec_m, "--db_seq_len", "4", "--seq_len", "4",
                      "--epochs", "3", "--max_keep", "5", "--graph"] + size + val) == 0
    out = capsys.readouterr().out
    assert len(re.findall(r"^Validating ", out, re.M)) == 3
    lines = open(os.path.join(ck, "validation-perfs.txt")).read().splitlines()
    assert len(lines) == 3 and all(len(l.split("\t\t")) == 8 for l in lines)
    best = os.path.join(ck, "best")
    table = open(os.path.join(best, "validation_perfs.csv")).read().splitlines()
    assert table[0] == "abs_rel,sq_rel,rmse,rmsel,a1,a2,a3,ckpt_name" and 2 <= len(table) <= 3
    named = re.search(r'model_checkpoint_path: "(ckpt-\d+\.npz)"', open(os.path.join(best, "checkpoint")).read()).group(1)
    assert os.path.isfile(os.path.join(best, named))
    assert sorted(os.listdir(os.path.join(ck, "train"))) == [f"ckpt-{s}{e}" for s in (2, 4, 6) for e in (".npz", ".opt.pt")]
    assert all(np.isfinite(l) for _, l in _losses(out))
    # the in-process validation of the last epoch == --mode=validation run afterwards on the same checkpoint, bit for bit
    in_process = open(os.path.join(ck, "perfs-kitti-raw.txt")).read()
    assert MAIN.main(["--mode", "validation", "--dataset", "kitti-raw", "--records_path", rec_k, "--db_seq_len", "4",
                      "--seq_len", "4", "--keep_top_n", "2"] + size) == 0
    assert "train/ckpt-6.npz" in capsys.readouterr().out
    assert open(os.path.join(ck, "perfs-kitti-raw.txt")).read() == in_process
    assert len(open(os.path.join(ck, "validation-perfs.txt")).read().splitlines()) == 4
    # 1b: best -> train, then the joint KITTI + Mid-Air finetuning, graph-replayed, with validation
    os.rename(os.path.join(ck, "train"), os.path.join(ck, "train-midair"))
    os.rename(best, os.path.join(ck, "train"))
    resume = int(named[5:-4])
    assert FK.main(["--records_path", recs, "--finetune_steps", "4", "--graph"] + size + val) == 0
    out = capsys.readouterr().out
    assert "4 steps per epoch, 2 epochs" in out                    # KITTI: 2 batches of 2 x 4-frame chunks; 4 // 4 + 1
    losses = _losses(out)
    assert [s for s, _ in losses] == list(range(resume + 1, resume + 9)) and all(np.isfinite(l) for _, l in losses)
    assert os.path.isfile(os.path.join(ck, "train", f"ckpt-{resume + 8}.npz"))
    assert os.path.isfile(os.path.join(ck, "best", "checkpoint"))
    # 2: eval reads best/
    assert MAIN.main(["--mode", "eval", "--dataset", "kitti-raw", "--records_path", rec_k, "--db_seq_len", "4"] + size) == 0
    out = capsys.readouterr().out
    assert re.search(r"Restoring weights from .*best/ckpt-\d+\.npz", out)
    assert np.isfinite(np.loadtxt(os.path.join(ck, "perfs-kitti-raw.txt"))).all()
