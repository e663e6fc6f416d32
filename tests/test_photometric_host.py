"""Host side of training without ground-truth depth (``--loss=photometric``): the parser and its refusals, the recording
loader's train use case with and without depth.txt, RMSE_log suppressed without ground truth, the summaries without the two
ground-truth images, argument validation of the new entry points.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from recording_ref import CAMERA_A, CAMERA_B, write_recording


def _parse(argv, world=1):
    from m4depth_amd import main as M
    parser = M.build_parser()
    args = parser.parse_args(argv)
    M.check_train_args(parser, args, world)
    M.check_recording_args(parser, args)
    return args


REC = ["--dataset", "recording", "--arch_depth", "2", "--height", "64", "--width", "64"]


def test_loss_options_parse(tmp_path):
    a = _parse(["--mode", "train"])
    assert (a.loss, a.photo_smooth, a.no_photo_automask) == ("supervised", None, False)
    a = _parse(["--mode", "train", "--loss", "photometric"])
    assert a.loss == "photometric"
    for graph in ([], ["--graph"]):
        a = _parse(["--mode", "train", "--loss", "photometric", "--photo_smooth", "0.01", "--no_photo_automask"] + graph)
        assert (a.loss, a.photo_smooth, a.no_photo_automask, a.graph) == ("photometric", 0.01, True, bool(graph))
    write_recording(str(tmp_path / "r"), CAMERA_B, 6, with_depth=False)
    a = _parse(["--mode", "train", "--loss", "photometric", "--records_path", str(tmp_path / "r")] + REC)
    from m4depth_amd import main as M
    assert M.recording_loader(a).allow_missing_depth
    a.loss = "supervised"
    assert not M.recording_loader(a).allow_missing_depth


def test_loss_refusals(tmp_path, capsys):
    write_recording(str(tmp_path / "nogt"), CAMERA_B, 6, with_depth=False)
    write_recording(str(tmp_path / "gt"), CAMERA_A, 6, with_depth=True)
    val = ["--mode", "train", "--enable_validation", "--db_path_config", "x.json", "--val_dataset", "recording"]
    for bad, message in ((["--mode", "train", "--loss", "l2"], "invalid choice"),
                         (["--mode", "eval", "--loss", "photometric"], "--loss=photometric is a --mode=train option"),
                         (["--mode", "finetune", "--loss", "photometric"], "--loss=photometric is a --mode=train option"),
                         (["--mode", "train", "--photo_smooth", "0.01"], "--photo_smooth needs --loss=photometric"),
                         (["--mode", "train", "--no_photo_automask"], "--no_photo_automask needs --loss=photometric"),
                         (["--mode", "train", "--loss", "photometric", "--photo_smooth", "-1"], "--photo_smooth must be >= 0"),
                         (["--mode", "train", "--records_path", str(tmp_path / "nogt")] + REC, "needs --loss=photometric"),
                         (val + ["--val_records_path", str(tmp_path / "nogt")], "--enable_validation: a recording .* has no depth.txt"),
                         (val + ["--val_records_path", str(tmp_path)], "--enable_validation: a recording .* has no depth.txt")):
        with pytest.raises(SystemExit):
            _parse(bad)
        assert re.search(message, capsys.readouterr().err), bad
    _parse(val + ["--val_records_path", str(tmp_path / "gt")])
    _parse(["--mode", "train", "--records_path", str(tmp_path / "gt")] + REC)


def test_recording_train_use_case_without_depth(tmp_path):
    """Train rows of a recording without depth.txt exist only when asked for; the default refusal is word for word the one of
    every scoring use case; with depth.txt for some frames only, the photometric run keeps every frame."""
    from m4depth_amd import dataloaders as dl
    root = str(tmp_path / "b")
    write_recording(root, CAMERA_B, 6, with_depth=False)
    settings = dl.DataloaderParameters(None, root, 3, 3, False)
    loader = dl.get_loader("recording")
    assert loader.allow_missing_depth is False
    with pytest.raises(ValueError) as e:
        loader.get_dataset("train", settings, batch_size=1, out_size=[64, 64], device="cpu")
    assert str(e.value) == (f"{root}: no depth.txt -- the 'train' use case scores against ground truth; a recording without it can "
                            "only be predicted (--mode=predict)")
    loader = dl.get_loader("recording")
    loader.allow_missing_depth = True
    ds = loader.get_dataset("train", settings, batch_size=1, out_size=[64, 64], device="cpu")
    assert ds.cardinality() == 2
    rows = loader._get_trajectories()[0]
    assert len(rows) == 6 and not any(r["depth"] for r in rows)
    for usecase in ("eval", "eval_streams"):                       # the option is the train use case's alone
        with pytest.raises(ValueError, match=r"b: no depth\.txt"):
            loader.get_dataset(usecase, dl.DataloaderParameters(None, root, None, None, False), batch_size=1, out_size=[64, 64],
                               device="cpu")
    part = str(tmp_path / "part")
    write_recording(part, CAMERA_A, 8, with_depth=True)
    path = os.path.join(part, "depth.txt")
    with open(path) as fh:
        text = fh.read()
    with open(path, "w") as fh:
        fh.write("\n".join(l for l in text.splitlines() if "0003.png" not in l) + "\n")
    for allow, n in ((False, 7), (True, 8)):
        loader = dl.get_loader("recording")
        loader.allow_missing_depth = allow
        loader.get_dataset("train", dl.DataloaderParameters(None, part, 4, 4, False), batch_size=1, out_size=[64, 64], device="cpu")
        assert len(loader._get_trajectories()[0]) == n


def test_rmse_log_is_suppressed_without_ground_truth():
    from m4depth_amd import main as M
    assert M.format_step(7, 0.5, 0.25) == "step 7: loss 0.500000  RMSE_log 0.250000"
    assert M.format_step(7, 0.5) == "step 7: loss 0.500000"
    assert "RMSE" not in M.format_step(7, float("nan"), None)


def test_summaries_without_ground_truth(tmp_path):
    """Scalars: the loss alone.  Images: RGB_im and depth_lvl_i, not the two made of ground truth."""
    import torch
    from m4depth_amd.summaries import TrainSummaryWriter
    data = {"RGB_im": torch.zeros(2, 3, 16, 24, 3)}
    pyramid = [torch.zeros(2, 8, 12, 1), torch.zeros(2, 4, 6, 1)]
    tags, shapes = TrainSummaryWriter._geometry(data, pyramid, has_gt=False)
    assert tags == ["RGB_im", "depth_lvl_0", "depth_lvl_1"] and shapes == [(16, 24, 3), (8, 12, 1), (4, 6, 1)]
    tags, shapes = TrainSummaryWriter._geometry(data, pyramid)
    assert tags == ["RGB_im", "camera_prev_t_reproj", "depth_gt", "depth_lvl_0", "depth_lvl_1"]
    w = TrainSummaryWriter(str(tmp_path))
    w.scalars(1, 0.5)
    w.scalars(2, 0.25, 0.125)
    w.close()
    blob = b"".join(open(os.path.join(tmp_path, f), "rb").read() for f in os.listdir(tmp_path))
    assert blob.count(b"loss") == 2 and blob.count(b"RMSE_log") == 1


def test_train_step_refuses_an_unknown_loss():
    from m4depth_amd import training as TR
    assert TR.LOSSES == ("supervised", "photometric")
    with pytest.raises(ValueError, match="loss: expected one of"):
        TR.train_step(None, {}, None, loss="photo")
    with pytest.raises(ValueError, match="loss: expected one of"):
        TR.GraphedTrainStep(None, {}, None, loss="photo")


def test_photo_abi_declared_bound_exported():
    from m4depth_amd import _lib
    names = ["m4d_image_pyramid_floats", "m4d_image_pyramid_box", "m4d_photo_warp_fwd", "m4d_photo_workspace_bytes",
             "m4d_photo_loss_fwd", "m4d_photo_loss_bwd"]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "m4depth_hip.h")).read()
    for n in names:
        assert n in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, n) and re.search(r"\b%s\s*\(" % n, header)
    assert _lib.lib.m4d_abi_version() == 6


def test_photo_argument_validation_without_gpu():
    from m4depth_amd._lib import lib
    fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)      # never dereferenced: validation fails first
    assert lib.m4d_image_pyramid_floats(4, 64, 96, 3) == 4 * 3 * (32 * 48 + 16 * 24 + 8 * 12)
    assert lib.m4d_image_pyramid_floats(4, 64, 96, 6) == -1 and lib.m4d_image_pyramid_floats(0, 64, 96, 1) == -1
    assert lib.m4d_image_pyramid_floats(1, 64, 96, 0) == -1
    assert lib.m4d_image_pyramid_box(None, 1, 64, 96, 2, fake, None) == 1
    assert lib.m4d_image_pyramid_box(fake, 1, 64, 96, 2, None, None) == 1
    assert lib.m4d_image_pyramid_box(fake, 1, 64, 90, 2, fake, None) == 1          # 90 is no multiple of 4
    warp = lambda **kw: lib.m4d_photo_warp_fwd(*[kw.get(k, d) for k, d in (
        ("depth", fake), ("rot", fake), ("rot_c", 4), ("trans", fake), ("f", fake), ("c", fake), ("prev", fake), ("b", 2), ("h", 6),
        ("w", 8), ("warped", fake), ("dwarp", fake), ("valid", fake))], None)
    for ptr in ("depth", "rot", "trans", "f", "c", "prev", "warped", "dwarp", "valid"):
        assert warp(**{ptr: None}) == 1, ptr
    assert warp(rot_c=5) == 1 and warp(rot_c=0) == 1
    assert warp(h=2) == 1 and warp(w=2) == 1 and warp(b=0) == 1 and warp(b=1 << 12, h=1 << 7, w=1 << 7) == 1
    assert lib.m4d_photo_workspace_bytes(2, 24, 40) == 2 * 2 * 3 * 3 * 8
    assert lib.m4d_photo_workspace_bytes(2, 2, 40) == -1 and lib.m4d_photo_workspace_bytes(2, 24, 2) == -1
    fwd = lambda **kw: lib.m4d_photo_loss_fwd(*[kw.get(k, d) for k, d in (
        ("depth", fake), ("warped", fake), ("valid", fake), ("cur", fake), ("prev", fake), ("b", 2), ("h", 6), ("w", 8),
        ("smooth", 1e-3), ("automask", 1), ("ws", fake), ("out4", fake), ("mask", fake))], None)
    for ptr in ("depth", "warped", "valid", "cur", "prev", "ws", "out4", "mask"):
        assert fwd(**{ptr: None}) == 1, ptr
    assert fwd(ws=odd) == 1 and fwd(h=2) == 1 and fwd(w=1) == 1 and fwd(b=-1) == 1
    bwd = lambda **kw: lib.m4d_photo_loss_bwd(*[kw.get(k, d) for k, d in (
        ("depth", fake), ("warped", fake), ("dwarp", fake), ("cur", fake), ("mask", fake), ("out4", fake), ("g_out", fake), ("b", 2),
        ("h", 6), ("w", 8), ("smooth", 1e-3), ("g_depth", fake))], None)
    for ptr in ("depth", "warped", "dwarp", "cur", "mask", "out4", "g_out", "g_depth"):
        assert bwd(**{ptr: None}) == 1, ptr
    assert bwd(h=2) == 1 and bwd(w=2) == 1 and bwd(b=0) == 1


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    import torch
    from m4depth_amd import network_ops as nops
    with pytest.raises(ValueError, match=r"expected \[n,H,W,3\]"):
        nops.image_pyramid_box(torch.zeros(1, 8, 8, 1), 1)
    with pytest.raises(RuntimeError, match="MI355X only"):
        nops.image_pyramid_box(torch.zeros(1, 8, 8, 3), 1)
    with pytest.raises(ValueError, match=r"depth: expected \[b,h,w,1\]"):
        nops.photo_warp_fwd(torch.zeros(1, 8, 8), torch.zeros(1, 3), torch.zeros(1, 3), torch.zeros(1, 2), torch.zeros(1, 2),
                            torch.zeros(1, 8, 8, 3))
    with pytest.raises(ValueError, match="Rotation must be expressed"):
        nops.photo_warp_fwd(torch.zeros(1, 8, 8, 1), torch.zeros(1, 5), torch.zeros(1, 3), torch.zeros(1, 2), torch.zeros(1, 2),
                            torch.zeros(1, 8, 8, 3))
