"""Train / eval / predict driver -- the counterpart of the reference ``main.py --mode=train``
(main.py:73-109), ``--mode=eval`` (:111-148) and ``--mode=predict`` (:150-172) over a seeded
synthetic dataset (no dataset or checkpoint exists in the build environment).

    python -m m4depth_amd.main --mode=eval --arch_depth=6 --seq_len=4 --batch_size=2 \\
           --n_batches=4 --ckpt_dir=/tmp/m4d
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \\
           -m m4depth_amd.main --mode=eval --batch_size=256        # global batch, sharded

Flag names follow ``m4depth_options.py`` where the flag exists there.  Like the
reference it writes the 7 metrics with ``%.18e`` (one per line, as np.savetxt does for the 1-D list) to
``<ckpt_dir>/perfs-<dataset>.txt`` (main.py:144-148).  With several ranks the batch
is sharded (m4depth_amd.dist) and the metric accumulators are all-gathered over RCCL.
``--mode=predict --save_dir DIR`` writes every frame's estimate as a 16-bit depth PNG in a dataset's own encoding (and, with
``--save_panels``, a colour panel PNG) through ``m4depth_amd.export.PredictionWriter`` instead of collecting predictions.npy;
``--save_cloud`` adds a coloured point cloud per frame (binary PLY), compacted on the GPU, in the frame of the trajectory's first
camera.
``--mode=train --log_dir DIR`` writes the training summaries (loss, RMSE_log, the reference's summary images) as a TensorBoard
event file through ``m4depth_amd.summaries.TrainSummaryWriter``.
``--eval_streams B`` runs a dataset's streaming evaluation (no ``--db_seq_len``) with B whole trajectories side by side
(m4depth_amd.stream_eval) and writes the same perfs file as the one-frame-at-a-time loop.  ``--consistency`` adds a score that
needs no ground truth (m4depth_amd.consistency: every frame's estimate against the previous frame, photometric and geometric)
and its two files; ``--enable_validation --val_consistency`` validates a training run that way, best-N on ``photo`` where the
validation set has no depth.
``--dataset=recording --records_path REC --height H --width W`` runs eval / predict on a user's own recording (frames, a
TUM-style trajectory, a calibration with lens distortion: m4depth_amd.dataloaders.recording); the frames are undistorted and
resized on the GPU.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

from . import checkpoints as CK
from . import dist as D
from . import synthetic as S
from .metrics import default_metrics
from .network import M4Depth, M4depthAblationParameters, GraphedSequence


def build_parser():
    p = argparse.ArgumentParser(description="M4Depth (MI355X native) train / eval / predict driver")
    p.add_argument("--mode", default="eval", choices=["train", "finetune", "eval", "validation", "predict"])
    p.add_argument("--dataset", default="synthetic", choices=["synthetic", "midair", "tartanair", "kitti-raw", "recording"],
                   help="a dataset of the reference (m4depth_options.py:11-14), the seeded synthetic one, or your own recording "
                        "(--records_path = a recording directory or a directory of them, dataloaders/recording.py; needs "
                        "--height and --width, no --db_path_config)")
    p.add_argument("--db_path_config", default=None, help="json file with the dataset roots (m4depth_options.py:27-29)")
    p.add_argument("--records_path", default=None, help="directory of trajectory csv files (m4depth_options.py:33-35)")
    p.add_argument("--rec_stride", type=int, default=None, metavar="N",
                   help="--dataset=recording: take every N-th frame of a trajectory (default 1)")
    p.add_argument("--rec_min_baseline", type=float, default=None, metavar="METRES",
                   help="--dataset=recording: of those, keep a frame when the camera centre has moved at least this far since "
                        "the last kept frame (default 0)")
    p.add_argument("--rec_max_gap", type=float, default=None, metavar="SECONDS",
                   help="--dataset=recording: drop a frame whose bracketing poses are further apart than this; the next kept "
                        "frame starts a new trajectory (default 0.5)")
    p.add_argument("--no_augmentation", action="store_true")
    p.add_argument("--epochs", type=int, default=1, help="train on a real dataset: passes over the records")
    p.add_argument("--arch_depth", type=int, default=6, help="number of pyramid levels (m4depth_options.py:64)")
    p.add_argument("--seq_len", type=int, default=4)
    p.add_argument("--db_seq_len", type=int, default=None)
    p.add_argument("--batch_size", type=int, default=1, help="GLOBAL batch (sharded over ranks)")
    p.add_argument("--n_batches", type=int, default=2, help="synthetic dataset: batches to generate")
    p.add_argument("--height", type=int, default=None, help="frame height (default: 384 synthetic, else the dataset's)")
    p.add_argument("--width", type=int, default=None)
    p.add_argument("--ckpt_dir", default="ckpt")
    p.add_argument("--tf_checkpoint", default=None,
                   help="TensorFlow checkpoint of the reference model (prefix, or a directory holding a 'checkpoint' state "
                        "file, e.g. pretrained_weights/midair): used instead of <ckpt_dir>/train for the initial weights")
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--graph", action="store_true", help="replay the sequence forward from a hipGraph")
    p.add_argument("--stream", action="store_true",
                   help="predict: run the frames as B independent streams with per-sample trajectory resets (M4Depth.stream_step; "
                        "with --graph replayed from network.GraphedStream)")
    p.add_argument("--eval_streams", type=int, default=0, metavar="N",
                   help="eval / validation on a dataset's whole trajectories (no --db_seq_len): run N trajectories side by side "
                        "as the samples of M4Depth.stream_step (with --graph replayed from network.GraphedStream), score each "
                        "sample on the device and fold the scores in the sequential run's order -- the same perfs file as the "
                        "one-frame-at-a-time loop.  0 = that loop")
    p.add_argument("--eval_streams_policy", default="lpt", choices=["lpt", "arrival"],
                   help="--eval_streams: the order trajectories are dealt to free slots (lpt = longest first, arrival = csv order)")
    p.add_argument("--consistency", action="store_true",
                   help="--eval_streams: also score every frame without ground truth -- the previous frame reprojected with the "
                        "estimated depth against the current one (photo: SSIM + L1, the criterion) and the estimate against the "
                        "previous frame's (geo, a diagnostic); m4depth_amd.consistency.  Writes perfs-consistency-<dataset>.txt "
                        "and consistency-frames-<dataset>.txt; a set without ground truth (a recording without depth.txt) is then "
                        "accepted and the seven metrics are skipped")
    p.add_argument("--host_input", action="store_true",
                   help="synthetic eval: hand every batch over from pinned HOST memory (the PCIe copy is part of the step) and "
                        "print the frames/s of the loop -- the PCIe-inclusive rate, next to bench.py's HBM-resident one")
    p.add_argument("--save_dir", default=None, metavar="DIR",
                   help="predict: write every frame to DIR/s<slot>_t<trajectory>/<frame>_depth.png (16-bit, --save_format), "
                        "encoded on the GPU and compressed in host threads (m4depth_amd.export), instead of predictions.npy")
    p.add_argument("--save_format", default=None, choices=["kitti16", "midair16"],
                   help="--save_dir: uint16 = depth * 256 (kitti16, the default) or float16 bits of 512 / depth (midair16)")
    p.add_argument("--save_panels", default=None, metavar="LIST",
                   help="--save_dir: comma list of rgb,est,gt,err -- also write <frame>_panels.png with these panels stacked "
                        "vertically (default: none)")
    p.add_argument("--save_range", type=float, nargs=2, default=None, metavar=("NEAR", "FAR"),
                   help="--save_panels: the depths the colour scale of est / gt spans, linear in inverse depth (default 1 80)")
    p.add_argument("--save_err_max", type=float, default=None,
                   help="--save_panels: the relative error the colour scale of err saturates at (default 0.5)")
    p.add_argument("--save_cloud", action="store_true",
                   help="--save_dir: also write <frame>_cloud.ply, the estimate as coloured 3-D points (depths within "
                        "--save_range), back-projected, posed and compacted on the GPU")
    p.add_argument("--cloud_stride", type=int, default=None, metavar="N",
                   help="--save_cloud: keep every N-th pixel of every N-th row (default 2)")
    p.add_argument("--cloud_frame", default=None, choices=["world", "camera"],
                   help="--save_cloud: coordinates in the frame of the trajectory's first camera (world, the default; the "
                        "frame-to-frame motions are chained on the GPU) or of each frame's own camera")
    p.add_argument("--learning_rate", type=float, default=1e-4, help="Adam step size (main.py:88)")
    p.add_argument("--loss", default="supervised", choices=["supervised", "photometric"],
                   help="train: supervised = the reference's log-depth L1 against ground truth; photometric = the reprojection "
                        "loss between neighbouring frames (SSIM + L1, auto-masking, edge-aware smoothness), which needs poses "
                        "but no ground-truth depth -- the way to finetune on a --dataset=recording without depth.txt")
    p.add_argument("--photo_smooth", type=float, default=None,
                   help="--loss=photometric: weight of the edge-aware smoothness term (default 1e-3, Monodepth2's value; not "
                        "tuned for this network)")
    p.add_argument("--no_photo_automask", action="store_true",
                   help="--loss=photometric: keep the pixels whose unwarped previous frame already matches better (auto-masking off)")
    p.add_argument("--photo_scale", default=None, choices=["level", "full"],
                   help="--loss=photometric: level (default) = each term at its level's resolution against the image pyramid; "
                        "full = every level's depth upsampled to the input resolution and compared there (Monodepth2's form)")
    p.add_argument("--photo_sources", default=None, choices=["prev", "both"],
                   help="--loss=photometric: prev (default) = frame t-1 only; both = the per-pixel minimum over frame t-1 and frame "
                        "t+1, which drops pixels one neighbour does not see (needs quaternion rotations)")
    p.add_argument("--save_every", type=int, default=0, help="train: checkpoint every N steps (0 = at the end)")
    p.add_argument("--summary_interval", type=int, default=1200,
                   help="train --graph: read the device-side step log every N steps (m4depth_options.py:47-49); it is also "
                        "read at every epoch end and before every checkpoint")
    p.add_argument("--log_dir", default=None, metavar="DIR",
                   help="train: write a TensorBoard event file to DIR (m4depth_options.py:43; m4depth_amd.summaries): loss and "
                        "RMSE_log of every step, and every --summary_interval steps the images of the reference's train_step "
                        "(RGB_im, camera_prev_t_reproj, depth_gt, depth_lvl_i), converted on the GPU and compressed in host "
                        "threads.  Rank 0 only")
    p.add_argument("--max_keep", type=int, default=0,
                   help="train: keep only the newest N checkpoints of <ckpt_dir>/train (0 = keep all)")
    p.add_argument("--enable_validation", action="store_true",
                   help="train: checkpoint at every epoch end and validate that checkpoint in-process (--mode=validation on "
                        "--val_dataset / --val_records_path, seq_len 4 / db_seq_len 4), keeping the best-N in <ckpt_dir>/best")
    p.add_argument("--val_records_path", default=None, help="--enable_validation: trajectory csv files of the validation set")
    p.add_argument("--val_dataset", default="kitti-raw", choices=["midair", "tartanair", "kitti-raw", "recording"],
                   help="--enable_validation: the validation set's dataset")
    p.add_argument("--val_consistency", action="store_true",
                   help="--enable_validation: validate as --eval_streams <batch_size> --consistency on whole trajectories instead "
                        "of the 4-frame sequence batches, appending a line to validation-consistency.txt; required for a "
                        "validation set without ground truth, where best-N is then judged on photo alone (lower is better)")
    p.add_argument("--keep_top_n", type=int, default=1,
                   help="validation: how many best checkpoints <ckpt_dir>/best keeps (callbacks.py:173-240)")
    # ablation flags, spelled as in m4depth_options.py:67-84
    for flag in ("DINL", "SNCV", "time_recurr", "feature_normalization", "feature_subdivision", "level_memory"):
        p.add_argument(f"--no_{flag}", action="store_true")
    return p


def ablation_from_args(args):
    return M4depthAblationParameters(not args.no_DINL, not args.no_SNCV, not args.no_time_recurr,
                                     not args.no_feature_normalization, not args.no_feature_subdivision,
                                     not args.no_level_memory)                  # m4depth_options.py:96-98


def synthetic_batches(args, rank, world, dev, on_host=False):
    """``on_host``: the batch stays in pinned host memory (the consumer uploads it: PCIe inside the step)."""
    lo, hi = D.shard_range(args.batch_size, rank, world)
    h, w = args.height or 384, args.width or 1280
    put = (lambda t: t.pin_memory()) if on_host else (lambda t: t.to(dev))
    for i in range(args.n_batches):
        samples, cam = S.make_sequence(args.batch_size, args.seq_len, h, w, seed=args.seed + i)
        data = {k: put(torch.from_numpy(np.stack([s[k][lo:hi] for s in samples], axis=1)))
                for k in ("depth", "RGB_im", "rot", "trans")}
        data["new_traj"] = torch.from_numpy(np.stack([s["new_traj"][lo:hi] for s in samples], axis=1))
        data["camera"] = {k: put(torch.from_numpy(v[lo:hi])) for k, v in cam.items()}
        yield data


def _upload(data, dev):
    """Host-resident batch -> device (non-blocking copies on the current stream); new_traj stays on the host."""
    out = {k: (v.to(dev, non_blocking=True) if isinstance(v, torch.Tensor) and k != "new_traj" else v) for k, v in data.items()
           if k != "camera"}
    out["camera"] = {k: v.to(dev, non_blocking=True) for k, v in data["camera"].items()}
    return out


def dataset_roots(db_path_config):
    """{dataset: root directory} of the json file (relative roots are relative to the file), m4depth_options.py:88-94."""
    import json
    cfg_dir = os.path.dirname(os.path.abspath(db_path_config))
    with open(db_path_config) as fh:
        return {k: (v if os.path.isabs(v) else os.path.normpath(os.path.join(cfg_dir, v)))
                for k, v in json.load(fh).items() if not k.startswith("_")}


def dataset_batches(args, usecase, rank, world, dev):
    """Batches of one of the reference's datasets (main.py:67,77,120,152).  Returns (iterable, depth_type).
    With several ranks the PER-RANK batch is batch_size / world; the loader shards the chunk list itself
    (``shard=(rank, world)``): every rank gets the same number of batches and reads / decodes only its own
    sequences.  Streaming evaluation is inherently sequential and stays single-rank."""
    from . import dataloaders as dl
    if args.dataset == "recording":
        if args.records_path is None:
            raise SystemExit("--dataset recording needs --records_path")
        roots = dataset_roots(args.db_path_config) if args.db_path_config else {}
        loader = recording_loader(args)
    else:
        if args.db_path_config is None or args.records_path is None:
            raise SystemExit("--dataset %s needs --db_path_config and --records_path" % args.dataset)
        roots = dataset_roots(args.db_path_config)
        loader = dl.get_loader(args.dataset)
    settings = dl.DataloaderParameters(roots, args.records_path, args.db_seq_len, args.seq_len, not args.no_augmentation)
    if usecase == "eval_streams":
        kw = {"out_size": [args.height, args.width]} if args.height and args.width else {}
        return loader.get_dataset(usecase, settings, batch_size=args.eval_streams, device=dev, seed=args.seed,
                                  slot_policy=args.eval_streams_policy, **kw), loader.depth_type
    streaming = usecase in ("eval", "predict") and args.db_seq_len is None
    if streaming and world > 1:
        raise SystemExit("streaming evaluation (no --db_seq_len) is sequential: run it on one rank")
    per_rank = 1 if streaming else D.shard_range(args.batch_size, rank, world)[1] - D.shard_range(args.batch_size, rank, world)[0]
    kw = {"out_size": [args.height, args.width]} if args.height and args.width else {}
    ds = loader.get_dataset(usecase, settings, batch_size=per_rank, device=dev, seed=args.seed,
                            shard=(0, 1) if streaming else (rank, world), **kw)
    return ds, loader.depth_type


def recording_loader(args):
    """The loader of ``--dataset=recording`` with the ``--rec_*`` options (their defaults where not given)."""
    from . import dataloaders as dl
    loader = dl.get_loader("recording")
    loader.stride = 1 if args.rec_stride is None else args.rec_stride
    loader.min_baseline = 0.0 if args.rec_min_baseline is None else args.rec_min_baseline
    loader.max_gap = 0.5 if args.rec_max_gap is None else args.rec_max_gap
    panels = getattr(args, "save_panels", None) or ()
    panels = panels.split(",") if isinstance(panels, str) else panels
    loader.require_depth = any(p in ("gt", "err") for p in panels)      # those panels need ground truth for every frame
    loader.allow_missing_depth = getattr(args, "loss", "supervised") == "photometric"      # train: that loss reads no ground truth
    # eval_streams under --consistency: a recording without depth.txt is scored without ground truth, every frame kept
    loader.allow_missing_depth_streams = bool(getattr(args, "consistency", False)) and args.records_path is not None \
        and not loader.has_depth(args.records_path)
    return loader


def check_recording_args(parser, args):
    """Refusals around ``--dataset=recording``: its ``--rec_*`` options belong to it alone, and a recording has no default
    network size."""
    given = [f for f in ("rec_stride", "rec_min_baseline", "rec_max_gap") if getattr(args, f) is not None]
    if args.dataset != "recording":
        if given:
            parser.error("--%s is a --dataset=recording option" % given[0])
        return
    if args.height is None or args.width is None:
        parser.error("--dataset=recording needs --height and --width (the size the frames are undistorted and resized to)")
    if args.records_path is not None:
        from .dataloaders.recording import find_recordings
        try:
            find_recordings(args.records_path)
        except ValueError as e:
            parser.error("--records_path %s" % e)
    unit = 2 ** args.arch_depth
    if args.height < unit or args.width < unit or args.height % unit or args.width % unit:
        parser.error("--dataset=recording: --height and --width must be positive multiples of 2**arch_depth = %d" % unit)
    if args.rec_stride is not None and args.rec_stride < 1:
        parser.error("--rec_stride must be >= 1")
    if args.rec_min_baseline is not None and not args.rec_min_baseline >= 0:
        parser.error("--rec_min_baseline must be >= 0")
    if args.rec_max_gap is not None and not args.rec_max_gap > 0:
        parser.error("--rec_max_gap must be > 0")


def _train_dir(args):
    return os.path.join(args.ckpt_dir, "train")


def latest_checkpoint(args):
    """Newest ``ckpt-<step>.npz`` of <ckpt_dir>/train (the role of tf.train.latest_checkpoint,
    callbacks.py:84), or None."""
    return CK.latest_checkpoint(_train_dir(args))


def read_weights(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files if not k.startswith("opt.")}


def load_weights(args, ablation):
    """Weights for eval / predict: the checkpoint <ckpt_dir>/best/checkpoint names when the best-N manager made one
    (main.py:116,156), else the latest training checkpoint when there is one (callbacks.py:104-111),
    otherwise the seeded random initialisation.  Training and validation read <ckpt_dir>/train only."""
    if args.tf_checkpoint:
        from . import tf_checkpoint as TC
        prefix = TC.latest_checkpoint(args.tf_checkpoint) if os.path.isdir(args.tf_checkpoint) else args.tf_checkpoint
        if prefix is None:
            raise SystemExit("no TensorFlow checkpoint found in %s" % args.tf_checkpoint)
        print("Restoring weights from TensorFlow checkpoint %s" % prefix)
        return TC.load_m4depth_weights(prefix, args.arch_depth)
    best = CK.best_checkpoint(args.ckpt_dir) if args.mode in ("eval", "predict") else None
    if best is not None:
        print("Restoring weights from %s" % best)
        return read_weights(best)
    ck = latest_checkpoint(args)
    if ck is not None:
        print("Restoring weights from %s" % ck[0])
        return read_weights(ck[0])
    return S.init_weights(args.arch_depth, seed=42, ablation=ablation)


def _set_capturable(opt, flag, dev):
    """Adam's ``capturable`` follows the launch mode, whichever mode wrote the optimizer state that was resumed: a captured
    step needs its step counters on the device, an eager one on the host (load_state_dict restores the saved flag)."""
    for g in opt.param_groups:
        g["capturable"] = flag
    for st in opt.state.values():
        if "step" in st and torch.is_tensor(st["step"]):
            st["step"] = st["step"].to(device=dev if flag else "cpu", dtype=torch.float32)


def _geometry(data):
    return ({k: tuple(data[k].shape) for k in ("depth", "RGB_im", "rot", "trans")},
            {k: tuple(v.shape) for k, v in data["camera"].items()})


def check_graph_batch(data, geometry=None):
    """A replayed training step has fixed shapes and its trajectory resets baked in: every batch must have the captured
    batch's geometry and ``new_traj`` set on frame 0 only.  Raises ValueError otherwise."""
    nt = np.asarray(data["new_traj"].cpu() if torch.is_tensor(data["new_traj"]) else data["new_traj"], dtype=bool)
    if nt.ndim != 2 or not nt[:, 0].all() or nt[:, 1:].any():
        raise ValueError("--graph: every training sequence must start a trajectory on frame 0 and only there "
                         f"(new_traj {nt.astype(int).tolist()}); the replayed step has its resets baked in")
    if geometry is not None and _geometry(data) != geometry:
        raise ValueError(f"--graph: a training batch of geometry {_geometry(data)} differs from the captured one {geometry}; "
                         "the replayed step has fixed shapes")


def default_epochs(args, rank, world, dev):
    """(number of epochs, epoch -> iterable of batches) of ``--mode=train|finetune`` on ``--dataset``."""
    if args.dataset == "synthetic":
        return 1, lambda epoch: synthetic_batches(args, rank, world, dev)
    return args.epochs, lambda epoch: dataset_batches(args, args.mode, rank, world, dev)[0]


def format_step(step, loss, rmse=None):
    """The line a reported training step prints; ``rmse`` None = the batch has no ground truth (nothing to score against)."""
    return f"step {step}: loss {loss:.6f}" + ("" if rmse is None else f"  RMSE_log {rmse:.6f}")


class _NonFiniteParameters(Exception):
    """Raised where a checkpoint would be written from non-finite parameters; carries the step."""


def train(args, ablation, rank, world, dev, epochs=None, depth_type=None):
    """``_train`` with the summary writer of ``--log_dir`` (rank 0; None without the option), closed on every way out."""
    summary = None
    if getattr(args, "log_dir", None) is not None and rank == 0:
        from .summaries import TrainSummaryWriter
        summary = TrainSummaryWriter(args.log_dir)
    try:
        return _train(args, ablation, rank, world, dev, epochs, depth_type, summary)
    except _NonFiniteParameters as e:
        print(f"step {e.args[0]}: non-finite parameters, training stopped: no checkpoint of this state is written")
        return 1
    finally:
        if summary is not None:
            summary.close()


def _train(args, ablation, rank, world, dev, epochs=None, depth_type=None, summary=None):
    """main.py:73-109: Adam(1e-4), RMSE_log as the tracked metric, resume from the latest checkpoint.
    Several ranks = data parallel: the global batch is sharded and the gradients are averaged with
    one RCCL all-reduce per step (dist.all_reduce_gradients).

    ``--graph``: the first batch runs the eager warm-up step of ``training.GraphedTrainStep`` (a real step: the same
    trajectory as the eager loop), the step is captured once, and every later batch is copied into its static buffers and
    replayed; each step ends with the device-side step log (``training.TrainStepLog``), read every ``--summary_interval``
    steps, before a checkpoint and at every epoch end -- the host reads nothing per step.

    TerminateOnNaN (callbacks.py:69-132): a non-finite loss ends training with status 1; nothing of that epoch is saved (in
    graph mode the steps replayed after the bad one are discarded with it) and the checkpoints on disk stay as they are.
    Non-finite parameters behind a finite loss are caught where a checkpoint is due (``save``): status 1, nothing written.

    ``summary`` (a ``summaries.TrainSummaryWriter``): every reported step's loss and RMSE_log go to it as they are printed, and
    at every step where ``(step - step0) % summary_interval == 0`` the step's images -- in graph mode right after that step's
    replay (and the log read that tells whether it was finite), before the next batch is copied into the static buffers.
    Nothing is written for a step with a non-finite loss or a later one.

    ``epochs`` = (count, epoch -> batches) (default: the dataset's, ``default_epochs``); ``depth_type`` defaults to the
    dataset's."""
    import time
    from . import training as TR
    from .metrics import RootMeanSquaredLogError
    torch.manual_seed(42)                                                       # tf.random.set_seed(42), main.py:76
    if depth_type is None:
        depth_type = {"kitti-raw": "velodyne"}.get(args.dataset, "map")          # the loader's depth_type (main.py:79)
    n_epochs, epoch_batches = epochs if epochs is not None else default_epochs(args, rank, world, dev)
    model = M4Depth(depth_type=depth_type, nbre_levels=args.arch_depth, ablation_settings=ablation, is_training=True)
    model.load_numpy_weights(load_weights(args, ablation), dev)
    TR.set_trainable(model)
    opt = torch.optim.Adam(model.parameters(), lr=args.learning_rate, eps=1e-7,   # Keras Adam: epsilon 1e-7
                           capturable=args.graph)
    rmse_log = RootMeanSquaredLogError()
    model.compile(optimizer=opt, metrics=[rmse_log])
    model.train_loss = getattr(args, "loss", "supervised")
    model.photo_smooth = 1e-3 if getattr(args, "photo_smooth", None) is None else args.photo_smooth
    model.photo_automask = not getattr(args, "no_photo_automask", False)
    model.photo_scale = getattr(args, "photo_scale", None) or "level"
    model.photo_sources = getattr(args, "photo_sources", None) or "prev"
    # a batch without ground truth (a recording without depth.txt under --loss=photometric): RMSE_log is a 0/0 masked mean,
    # so it is neither printed nor logged, and the loss alone decides whether a step was bad
    has_gt = args.dataset == "synthetic" or args.records_path is None or records_have_depth(args)
    ck = latest_checkpoint(args)
    step0 = 0
    if ck is not None:
        step0 = ck[1]
        opt_path = ck[0][:-4] + ".opt.pt"
        if os.path.isfile(opt_path):
            opt.load_state_dict(torch.load(opt_path, map_location=dev))
            _set_capturable(opt, args.graph, dev)
    sync = D.all_reduce_gradients if world > 1 else None
    saved, checked = set(), set()

    def save(step):
        # A step whose gradients are non-finite while its loss is finite (a stationary sample: DESIGN.md "Degenerate inputs",
        # R6) leaves non-finite weights behind that TerminateOnNaN only sees one step later: look at the parameters where they
        # are written -- once per save, reduced on the device, one host read, on every rank (the replicas hold the same
        # weights, so all ranks stop together) -- never in the step itself.
        if step not in checked:
            checked.add(step)
            if not bool(torch.stack([torch.isfinite(p.detach()).all() for p in model.parameters()]).all()):
                raise _NonFiniteParameters(step)
        if rank != 0 or step in saved:
            return None
        saved.add(step)
        os.makedirs(_train_dir(args), exist_ok=True)
        path = os.path.join(_train_dir(args), f"ckpt-{step}.npz")
        np.savez(path, **model.numpy_weights())
        torch.save(opt.state_dict(), path[:-4] + ".opt.pt")
        print("saved", path)
        CK.prune_checkpoints(_train_dir(args), args.max_keep)
        return path

    def report(step, loss, rmse):
        if rank == 0:
            print(format_step(step, loss, rmse if has_gt else None))
        if summary is not None:
            summary.scalars(step, loss, rmse if has_gt else None)

    step_log = runner = geometry = None
    logged = [step0]                                  # graph mode: the last step whose log row the host has read

    def read_log():
        """Graph mode: hands the unread log rows to the host (prints, the compiled RMSE_log Mean); returns the step of the first
        non-finite loss or None."""
        rows, first_bad = step_log.read()
        for i, (loss, rmse) in enumerate(rows):
            if first_bad >= 0 and i + logged[0] - step0 >= first_bad:
                break                                 # the steps after the bad one are discarded
            if has_gt:
                rmse_log._update(torch.tensor(rmse))
            report(logged[0] + i + 1, float(loss), float(rmse_log.result()))
        logged[0] += len(rows)
        return step0 + first_bad + 1 if first_bad >= 0 else None

    def images_due(step):
        return summary is not None and nan_step is None and (step - step0) % max(args.summary_interval, 1) == 0

    step, t0, n_timed, nan_step = step0, None, 0, None
    for epoch in range(n_epochs):
        for data in epoch_batches(epoch):
            if args.graph:
                check_graph_batch(data, geometry)
                if runner is None:
                    geometry = _geometry(data)
                    step_log = TR.TrainStepLog(max(args.summary_interval, 1) + 1, dev)
                    runner = TR.GraphedTrainStep(model, data, opt, warmup=1, grad_sync=sync, step_log=step_log,
                                                 loss=model.train_loss)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                else:
                    runner(data)
                    n_timed += 1
                step += 1
                if (step - step0) % max(args.summary_interval, 1) == 0 or (args.save_every and step % args.save_every == 0):
                    nan_step = read_log()
                if images_due(step):
                    summary.images(step, runner.static, runner.pyramid, runner.camera, has_gt=has_gt)
            else:
                out = model.train_step(data, grad_sync=sync)
                step += 1
                loss = float(out["loss"])
                if t0 is None:
                    t0 = time.perf_counter()
                else:
                    n_timed += 1
                if not np.isfinite(loss):
                    nan_step = step
                else:
                    report(step, loss, float(out["RMSE_log"]))
                    if images_due(step):
                        summary.images(step, data, model.last_pyramid, data["camera"], has_gt=has_gt)
            if nan_step is not None:
                break
            if args.save_every and step % args.save_every == 0:
                save(step)
        if args.graph and nan_step is None and runner is not None:
            nan_step = read_log()
        if nan_step is not None:
            print(f"step {nan_step}: non-finite loss, training stopped (TerminateOnNaN): nothing of epoch {epoch + 1} is saved")
            return 1
        if args.enable_validation:
            path = save(step)
            if path is None and rank == 0:
                path = os.path.join(_train_dir(args), f"ckpt-{step}.npz")
            if rank == 0:
                validate_checkpoint(args, ablation, dev, path)
    if n_timed and rank == 0:
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"train ({'graph' if args.graph else 'eager'}): {n_timed / dt:.2f} steps/s over {n_timed} steps "
              "(the first step excluded)")
    if not args.save_every or step % args.save_every != 0:
        save(step)
    return 0


def validation_args(args):
    """The options of the in-process validation of ``--enable_validation`` (callbacks.py:149-170): --mode=validation on the
    validation set at seq_len 4 / db_seq_len 4, the training batch size and --height / --width."""
    import copy
    v = copy.copy(args)
    v.mode, v.dataset, v.records_path = "validation", args.val_dataset, args.val_records_path
    v.seq_len = v.db_seq_len = 4
    v.eval_streams, v.graph, v.stream, v.host_input, v.tf_checkpoint = 0, False, False, False, None
    v.consistency = False
    if args.val_consistency:          # whole trajectories, batch_size side by side, scored with and without ground truth
        v.eval_streams, v.eval_streams_policy, v.db_seq_len, v.consistency = args.batch_size, "lpt", None, True
    return v


def validate_checkpoint(args, ablation, dev, path):
    """``--mode=validation`` of the checkpoint file ``path`` on a separate inference model (nothing shared with the training
    model or its captured step); writes what that mode writes."""
    from . import network_ops as nops
    vargs = validation_args(args)
    print("Validating %s on %s" % (path, vargs.dataset))
    torch.cuda.synchronize()
    with nops.private_workspaces():                    # the captured training step's scratch buffers stay its own
        model = M4Depth(nbre_levels=vargs.arch_depth, ablation_settings=ablation)
        model.load_numpy_weights(read_weights(path), dev)
        model.compile(metrics=default_metrics())
        metrics = evaluate(vargs, model, 0, 1, dev)
        if metrics is not None:
            write_perfs(vargs, model, metrics)
        del model
        torch.cuda.synchronize()
    write_validation(vargs, metrics, getattr(vargs, "consistency_means", None))
    return metrics


def write_perfs(args, model, metrics):
    os.makedirs(args.ckpt_dir, exist_ok=True)
    path = os.path.join(args.ckpt_dir, "perfs-" + args.dataset + ".txt")
    np.savetxt(path, metrics, fmt='%.18e', delimiter='\t', newline='\n')      # main.py:147 (1-D: one metric per line)
    for m, v in zip(model.compiled_metrics, metrics):
        print(f"{m.name}: {v:.6f}")
    print("wrote", path)


def write_validation(args, metrics, consistency=None):
    """main.py:132-142: the best-N manager judges the latest training checkpoint, and one line goes to validation-perfs.txt.
    ``consistency`` (the six means of --consistency, or None) adds a line to validation-consistency.txt; where there are no
    seven metrics (a validation set without ground truth) best-N is judged on its ``photo`` alone, lower is better."""
    best = os.path.join(args.ckpt_dir, "best")
    if metrics is not None:
        CK.BestCheckpointManager(_train_dir(args), best, keep_top_n=args.keep_top_n) \
            .update_backup(dict(zip(CK.METRIC_COLUMNS, metrics)))
        CK.append_validation_perfs(args.ckpt_dir, metrics)
    elif consistency is not None:
        CK.BestCheckpointManager(_train_dir(args), best, keep_top_n=args.keep_top_n, criterion=CK.PHOTO_CRITERION) \
            .update_backup({"photo": float(consistency[0])})
    if consistency is not None:
        CK.append_validation_perfs(args.ckpt_dir, consistency, "validation-consistency.txt")


def _stream_frame(frame, dev):
    """One frame for ``M4Depth.stream_step``: every input on the device (new_traj included: the per-sample reset mask is built
    there)."""
    out = {k: frame[k].to(dev, non_blocking=True) for k in ("RGB_im", "rot", "trans", "new_traj")}
    out["camera"] = {k: v.to(dev, non_blocking=True) for k, v in frame["camera"].items()}
    return out


def _check_eval_streams(parser, args):
    if args.eval_streams < 0:
        parser.error("--eval_streams must be >= 0")
    if args.consistency and (not args.eval_streams or args.mode not in ("eval", "validation")):
        parser.error("--consistency needs --eval_streams B (with or without --graph) in --mode=eval / --mode=validation: it scores "
                     "whole trajectories, each frame against the one before it")
    if not args.eval_streams:
        return
    if args.mode not in ("eval", "validation"):
        parser.error("--eval_streams is a --mode=eval / --mode=validation option")
    if args.dataset == "synthetic":
        parser.error("--eval_streams runs the trajectories of a real dataset (--dataset midair | tartanair | kitti-raw | recording)")
    if args.db_seq_len is not None:
        parser.error("--eval_streams evaluates whole trajectories: it excludes --db_seq_len")


def records_have_depth(args):
    """Whether the trajectory files of ``--records_path`` name a ground-truth map (the loader's depth column): known on the
    host before anything is loaded."""
    import glob
    from . import dataloaders as dl
    if args.dataset == "recording":
        return dl.get_loader("recording").has_depth(args.records_path)
    col = dl.get_loader(args.dataset)._depth_column()
    files = sorted(glob.glob(os.path.join(args.records_path, "**/*.csv"), recursive=True))
    if not files:
        return False
    with open(files[0], newline="") as fh:
        return col in fh.readline().rstrip("\r\n").split("\t")


def check_save_args(parser, args):
    """Refusals of the ``--save_*`` options; fills in their defaults and parses ``--save_panels`` into a tuple."""
    from .export import PANELS
    others = [f for f in ("save_format", "save_panels", "save_range", "save_err_max") if getattr(args, f) is not None]
    others += [f for f in ("save_cloud",) if args.save_cloud]
    cloud_others = [f for f in ("cloud_stride", "cloud_frame") if getattr(args, f) is not None]
    if args.save_dir is not None and cloud_others and not args.save_cloud:
        parser.error("--%s needs --save_cloud" % cloud_others[0])
    others += cloud_others
    if args.cloud_stride is not None and args.cloud_stride < 1:
        parser.error("--cloud_stride must be >= 1")
    args.cloud_stride = 2 if args.cloud_stride is None else args.cloud_stride
    args.cloud_frame = args.cloud_frame or "world"
    if args.save_dir is None:
        if others:
            parser.error("--%s needs --save_dir" % others[0])
        return
    if args.mode != "predict":
        parser.error("--save_dir is a --mode=predict option")
    args.save_format = args.save_format or "kitti16"
    panels = tuple(p for p in (args.save_panels or "").split(",") if p)
    if len(panels) > 4 or any(p not in PANELS for p in panels):
        parser.error("--save_panels: a comma list of up to four of %s, got %r" % (",".join(PANELS), args.save_panels))
    args.save_panels = panels
    args.save_range = tuple(args.save_range) if args.save_range is not None else (1.0, 80.0)
    args.save_err_max = 0.5 if args.save_err_max is None else args.save_err_max
    if not (0 < args.save_range[0] < args.save_range[1]):
        parser.error("--save_range NEAR FAR needs 0 < NEAR < FAR")
    if not args.save_err_max > 0:
        parser.error("--save_err_max must be > 0")
    if any(p in ("gt", "err") for p in panels) and args.dataset != "synthetic" and args.records_path is not None \
            and not records_have_depth(args):
        parser.error("--save_panels %s: the records of --records_path name no ground-truth map" % ",".join(panels))


def eval_streams(args, model, dev):
    """Streaming evaluation with ``--eval_streams`` B slots (m4depth_amd.stream_eval): per step one ``stream_step`` (or a
    ``GraphedStream`` replay) and one per-sample metric launch into a preallocated [n_steps,B,7] / [n_steps,B] device log; no
    host read of any mask.  After the last step: one copy of the log to the host, the fold in the sequential order, and the
    folded (total, count) loaded into the compiled metrics for the writer.

    ``--consistency`` adds one launch pair per step (``consistency.ConsistencyScorer``) into an [n_steps,B,6] / [n_steps,B] log
    of its own and, after the last step, ``perfs-consistency-<dataset>.txt`` and ``consistency-frames-<dataset>.txt``; the means
    are left in ``args.consistency_means``.  With ground truth the seven metrics are computed exactly as without the flag;
    without it (a recording without depth.txt, csv files without a depth column) they are skipped.  Returns whether the seven
    were computed."""
    import time
    from . import network_ops as nops
    from . import stream_eval as SE
    has_gt = records_have_depth(args) if args.consistency else True    # without --consistency the loader refuses or the step fails
    ds, _ = dataset_batches(args, "eval_streams", 0, 1, dev)
    sched = ds.schedule
    n_steps, B = sched.cells.shape[:2]
    if has_gt:
        rows = torch.empty((n_steps, B, 7), dtype=torch.float32, device=dev)
        counted = torch.empty((n_steps, B), dtype=torch.uint8, device=dev)
    scorer = None
    if args.consistency:                                           # one more launch pair per step into a log of its own
        from . import consistency as CS
        scorer = CS.ConsistencyScorer(copy_estimate=args.graph)    # GraphedStream's output buffer is overwritten by the next replay
        c_rows = torch.empty((n_steps, B, len(CS.COLUMNS)), dtype=torch.float32, device=dev)
        c_counted = torch.empty((n_steps, B), dtype=torch.uint8, device=dev)
    active = (sched.cells[..., 0] >= 0).sum(axis=1)                # the schedule's, known on the host without a device read
    runner, t0 = None, None
    for step, batch in enumerate(ds):
        if step == 1:                                              # the first step is the warm-up (allocations, graph capture)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        frame = {"RGB_im": batch["RGB_im"], "rot": batch["rot"], "trans": batch["trans"], "new_traj": batch["reset"],
                 "camera": batch["camera"]}
        if args.graph:
            if runner is None:
                from .network import GraphedStream
                runner = GraphedStream(model, frame)
            est = runner(frame)["depth"]
        else:
            est = model.stream_step(frame)["depth"]
        if has_gt:
            nops.depth_metrics_per_sample(batch["depth"], est, batch["new_traj"], batch["active"], 80., rows=rows[step],
                                          counted=counted[step])
        if scorer is not None:
            scorer.step(frame, est, batch["reset"], batch["active"], c_rows[step], c_counted[step])
    if has_gt:
        rows_h, counted_h = rows.cpu().numpy(), counted.cpu().numpy()
    if scorer is not None:
        c_rows_h, c_counted_h = c_rows.cpu().numpy(), c_counted.cpu().numpy()
    if t0 is not None:
        dt = time.perf_counter() - t0
        n = int(active[1:].sum())
        print(f"eval_streams {B} slots ({args.eval_streams_policy}, {'graph' if args.graph else 'eager'}"
              f"{', consistency' if scorer is not None else ''}): {n / dt:.1f} "
              f"sample-frames/s over {n} active sample-frames of {n_steps - 1} steps (the first step excluded)")
    if has_gt:
        total, count = SE.fold(rows_h, counted_h, sched.cells)
        for i, m in enumerate(model.compiled_metrics):
            m.load_state(torch.tensor(total[i], dtype=torch.float32, device=dev), count)
    args.consistency_means = None
    if scorer is not None:
        c_total, c_count, frames = SE.fold_consistency(c_rows_h, c_counted_h, sched.cells)
        args.consistency_means = SE.fold_result(c_total, c_count)
        os.makedirs(args.ckpt_dir, exist_ok=True)
        CS.write_perfs(CS.perfs_path(args.ckpt_dir, args.dataset), args.consistency_means)
        CS.write_frames(CS.frames_path(args.ckpt_dir, args.dataset), frames)
        for name, v in zip(CS.COLUMNS, args.consistency_means):
            print(f"consistency {name}: {v:.6f}")
        print(f"wrote {CS.perfs_path(args.ckpt_dir, args.dataset)} and {CS.frames_path(args.ckpt_dir, args.dataset)} "
              f"({c_count} counted frames)")
    return has_gt


def evaluate(args, model, rank, world, dev):
    """The eval / validation / predict loop of ``model`` (compiled with the 7 metrics): returns the metrics all-gathered over the
    ranks (numpy [7]), or None for predict (rank 0 has then written predictions.npy)."""
    runner = None
    preds = []
    writer = namer = None
    if args.mode == "predict" and args.save_dir is not None:
        from .export import PredictionWriter
        writer = PredictionWriter(args.save_dir, args.save_format, args.save_panels, near=args.save_range[0],
                                  far=args.save_range[1], err_max=args.save_err_max, cloud=args.save_cloud,
                                  cloud_step=args.cloud_stride, cloud_frame=args.cloud_frame)
    host_input = args.host_input and args.dataset == "synthetic" and args.mode != "predict"
    if args.eval_streams:
        if not eval_streams(args, model, dev):
            return None                                # no ground truth (--consistency): there are no seven metrics
        batches = ()
    elif args.dataset == "synthetic":
        batches = synthetic_batches(args, rank, world, dev, on_host=host_input)
        if host_input:
            batches = list(batches)                # generation is not part of the measured loop
    else:
        batches, _ = dataset_batches(args, "predict" if args.mode == "predict" else "eval", rank, world, dev)
    stream_runner = []

    def predict(frame):
        if not args.stream:
            return model.predict_step(frame)["depth"]
        sf = _stream_frame(frame, dev)
        if not args.graph:
            return model.stream_step(sf)["depth"]
        if not stream_runner:
            from .network import GraphedStream
            stream_runner.append(GraphedStream(model, sf))
        return stream_runner[0](sf)["depth"]

    import time
    t_save = None

    def emit(frame):
        """One predicted frame batch: to the writer (its export launch follows the forward -- or the graph replay -- on the
        same stream; nothing is kept), or to the list predictions.npy is made of."""
        nonlocal namer, t_save
        est = predict(frame)
        if writer is None:
            preds.append(est.cpu().numpy())
            return
        if namer is None:
            from .export import FrameNamer
            namer = FrameNamer(est.shape[0])
            t_save = time.perf_counter()
        want_gt = any(p in ("gt", "err") for p in writer.panels)
        cloud = {}
        if writer.cloud:                                       # the cloud launches follow the forward / the replay on its stream
            cloud = dict(rot=frame["rot"], trans=frame["trans"], camera=frame["camera"], reset=frame["new_traj"])
        writer.submit(est, namer(frame["new_traj"]), gt=frame.get("depth") if want_gt else None,
                      rgb=frame["RGB_im"] if "rgb" in writer.panels or writer.cloud else None, **cloud)

    n_frames, t_loop = 0, None
    for batch_idx, data in enumerate(batches):
        if host_input:
            if batch_idx == 1:                                 # the first batch is the warm-up (allocations, graph capture)
                torch.cuda.synchronize()
                t_loop, n_frames = time.perf_counter(), 0
            data = _upload(data, dev)
            n_frames += data["RGB_im"].shape[0] * data["RGB_im"].shape[1]
        if data["RGB_im"].dim() == 4:            # streaming frame of a real dataset (db_seq_len None)
            if args.mode == "predict":
                emit(data)
            else:
                model.test_step(data)
            continue
        if args.mode == "predict":
            for t in range(data["RGB_im"].shape[1]):
                frame = {k: data[k][:, t] for k in ("depth", "RGB_im", "rot", "trans", "new_traj")}
                frame["camera"] = data["camera"]
                emit(frame)
            continue
        if args.graph:
            if runner is None:
                model.test_step(data)              # eager warm-up (state and scratch allocation, packed weights)
                for m in model.compiled_metrics:
                    m.reset_state()
                runner = GraphedSequence(model, data)
            model.graphed_test_step(data, runner)
        else:
            model.test_step(data)
    if writer is not None:
        writer.close()
        if namer is not None:
            dt = time.perf_counter() - t_save
            print(f"predict: wrote {writer.frames} frames ({args.save_format}"
                  + (", panels " + ",".join(writer.panels) if writer.panels else "")
                  + (f", clouds at stride {writer.cloud_step}" if writer.cloud else "")
                  + f") to {args.save_dir}: {writer.frames / dt:.1f} frames/s, the first forward excluded from the clock")
        return None
    if args.mode == "predict":
        if rank == 0:
            os.makedirs(args.ckpt_dir, exist_ok=True)
            np.save(os.path.join(args.ckpt_dir, "predictions.npy"), np.concatenate(preds, axis=0))
        return None
    if host_input and t_loop is not None:
        torch.cuda.synchronize()
        dt = time.perf_counter() - t_loop
        if rank == 0 and n_frames:
            print(f"host-resident input (pinned memory, PCIe copy inside the step): {n_frames / dt:.1f} frames/s per rank "
                  f"over {n_frames} frames")
    gathered = D.all_gather_metric_states(model.compiled_metrics, dev)
    return D.reduce_metric_states(gathered).cpu().numpy()


def check_train_args(parser, args, world=None):
    """Refusals of the training workflow's options.  ``world``: the number of ranks (default: WORLD_SIZE of the environment,
    what dist.init_from_env will see)."""
    if world is None:
        world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.summary_interval < 1:
        parser.error("--summary_interval must be >= 1")
    if args.log_dir is not None and args.mode not in ("train", "finetune"):
        parser.error("--log_dir is a --mode=train / --mode=finetune option")
    if args.max_keep < 0:
        parser.error("--max_keep must be >= 0")
    if args.keep_top_n < 1:
        parser.error("--keep_top_n must be >= 1")
    if args.enable_validation:
        if args.val_records_path is None:
            parser.error("--enable_validation needs --val_records_path (the validation set's trajectory csv files)")
        if args.db_path_config is None:
            parser.error("--enable_validation needs --db_path_config (the validation set's dataset root)")
        if world > 1:
            parser.error("--enable_validation runs in-process on one GPU: it is refused with several ranks")
    elif args.val_consistency:
        parser.error("--val_consistency needs --enable_validation (it chooses how that validation scores)")
    photo_opts = [f for f, on in (("photo_smooth", args.photo_smooth is not None), ("no_photo_automask", args.no_photo_automask),
                                      ("photo_scale", args.photo_scale is not None), ("photo_sources", args.photo_sources is not None)) if on]
    if args.loss != "supervised" and args.mode != "train":
        parser.error("--loss=%s is a --mode=train option" % args.loss)
    if photo_opts and args.loss != "photometric":
        parser.error("--%s needs --loss=photometric" % photo_opts[0])
    if args.photo_smooth is not None and not args.photo_smooth >= 0:
        parser.error("--photo_smooth must be >= 0")
    if args.mode == "train" and args.loss == "supervised" and args.dataset == "recording" and args.records_path is not None:
        try:
            if not records_have_depth(args):
                parser.error("--mode=train on a recording without depth.txt needs --loss=photometric (the supervised loss reads "
                             "ground-truth depth)")
        except ValueError:
            pass                                   # a malformed --records_path: check_recording_args reports it
    if args.enable_validation and args.val_dataset == "recording" and args.val_records_path is not None:
        from . import dataloaders as dl
        try:
            scored = dl.get_loader("recording").has_depth(args.val_records_path)
        except ValueError as e:
            parser.error("--val_records_path %s" % e)
        if not scored and not args.val_consistency:
            parser.error("--enable_validation: a recording of --val_records_path has no depth.txt -- validation scores against "
                         "ground truth, which such a recording does not have")
    if args.graph and args.mode in ("train", "finetune") and world > 1:
        parser.error("--graph training is refused with several ranks (RCCL inside a captured training step is not supported)")


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.stream and args.mode != "predict":
        parser.error("--stream is a --mode=predict option")
    _check_eval_streams(parser, args)
    check_train_args(parser, args)
    check_recording_args(parser, args)
    check_save_args(parser, args)
    rank, world, _, dev = D.init_from_env()
    if args.eval_streams and world > 1:
        raise SystemExit("streaming evaluation (--eval_streams) is sequential over the trajectories: run it on one rank")
    if args.save_dir is not None and world > 1:
        raise SystemExit("--save_dir writes one directory tree from one process: run it on one rank")
    if dev.type != "cuda":
        raise SystemExit("m4depth_amd.main needs a GPU: the hot path has no CPU fallback")
    ablation = ablation_from_args(args)
    if args.mode in ("train", "finetune"):
        return train(args, ablation, rank, world, dev)
    model = M4Depth(nbre_levels=args.arch_depth, ablation_settings=ablation)
    model.load_numpy_weights(load_weights(args, ablation), dev)
    model.compile(metrics=default_metrics())
    metrics = evaluate(args, model, rank, world, dev)
    if metrics is not None and rank == 0:
        write_perfs(args, model, metrics)
    if args.mode == "validation" and rank == 0:
        write_validation(args, metrics, getattr(args, "consistency_means", None))
    return 0

if __name__ == "__main__":
    sys.exit(main())
