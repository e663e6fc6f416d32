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
camera; ``--save_map VOXEL`` adds one fused voxel map per trajectory (``map.ply``), merged on the GPU from the clouds' vertices;
``--save_mesh VOXEL`` adds one triangle mesh per trajectory (``mesh.ply``), a TSDF fused and extracted on the GPU.
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

import os
import sys
import time

import numpy as np
import torch

from . import checkpoints as CK
from . import dist as D
from . import synthetic as S
from .metrics import default_metrics
from .network import M4Depth, GraphedSequence, GraphedStream
from .options import (build_parser, ablation_from_args, check_args, check_recording_args, check_save_args,  # noqa: F401
                      check_stream_args, check_train_args, _check_eval_streams, records_have_depth)


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
    kw = {"out_size": [args.height, args.width]} if args.height and args.width else {}
    if usecase == "eval_streams":
        return loader.get_dataset(usecase, settings, batch_size=args.eval_streams, device=dev, seed=args.seed,
                                  slot_policy=args.eval_streams_policy, **kw), loader.depth_type
    streaming = usecase in ("eval", "predict") and args.db_seq_len is None
    if streaming and world > 1:
        raise SystemExit("streaming evaluation (no --db_seq_len) is sequential: run it on one rank")
    lo, hi = (0, 1) if streaming else D.shard_range(args.batch_size, rank, world)
    ds = loader.get_dataset(usecase, settings, batch_size=hi - lo, device=dev, seed=args.seed,
                            shard=(0, 1) if streaming else (rank, world), **kw)
    return ds, loader.depth_type


def input_batches(args, usecase, rank, world, dev, on_host=False):
    """The batches ``--mode=eval|validation|predict`` runs over: the seeded synthetic ones or the dataset's."""
    if args.dataset == "synthetic":
        return synthetic_batches(args, rank, world, dev, on_host=on_host)
    return dataset_batches(args, usecase, rank, world, dev)[0]


def recording_loader(args):
    """The loader of ``--dataset=recording`` with the ``--rec_*`` options (their defaults where not given)."""
    from . import dataloaders as dl
    loader = dl.get_loader("recording")
    loader.stride = 1 if args.rec_stride is None else args.rec_stride
    loader.min_baseline = 0.0 if args.rec_min_baseline is None else args.rec_min_baseline
    loader.max_gap = 0.5 if args.rec_max_gap is None else args.rec_max_gap
    panels = args.save_panels or ()
    panels = panels.split(",") if isinstance(panels, str) else panels
    loader.require_depth = any(p in ("gt", "err") for p in panels)      # those panels need ground truth for every frame
    loader.allow_missing_depth = args.loss == "photometric"             # train: that loss reads no ground truth
    # eval_streams under --consistency: a recording without depth.txt is scored without ground truth, every frame kept
    loader.allow_missing_depth_streams = args.consistency and args.records_path is not None \
        and not loader.has_depth(args.records_path)
    return loader


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


class CheckpointWriter:
    """The checkpoints of a training run, ``<ckpt_dir>/train/ckpt-<step>.npz`` with the optimizer state next to it: a step is
    written once (rank 0) and the oldest files are pruned to ``--max_keep``."""

    def __init__(self, args, model, opt, rank):
        self.dir, self.max_keep, self.model, self.opt, self.rank = _train_dir(args), args.max_keep, model, opt, rank
        self.saved, self.checked = set(), set()        # the steps written / the steps whose parameters were looked at

    def path(self, step):
        return os.path.join(self.dir, f"ckpt-{step}.npz")

    def save(self, step):
        """Writes the checkpoint of ``step``; returns its path, or None where nothing was written (rank != 0, or the step is
        on disk already).  Raises ``_NonFiniteParameters`` instead of writing non-finite weights."""
        # A step whose gradients are non-finite while its loss is finite (a stationary sample: DESIGN.md "Degenerate inputs",
        # R6) leaves non-finite weights behind that TerminateOnNaN only sees one step later: look at the parameters where they
        # are written -- once per save, reduced on the device, one host read, on every rank (the replicas hold the same
        # weights, so all ranks stop together) -- never in the step itself.
        if step not in self.checked:
            self.checked.add(step)
            if not bool(torch.stack([torch.isfinite(p.detach()).all() for p in self.model.parameters()]).all()):
                raise _NonFiniteParameters(step)
        if self.rank != 0 or step in self.saved:
            return None
        self.saved.add(step)
        os.makedirs(self.dir, exist_ok=True)
        path = self.path(step)
        np.savez(path, **self.model.numpy_weights())
        torch.save(self.opt.state_dict(), path[:-4] + ".opt.pt")
        print("saved", path)
        CK.prune_checkpoints(self.dir, self.max_keep)
        return path


class _Stepper:
    """What ``train_loop`` asks of a training step.  ``step(data)`` takes one and returns the rows ``(step, loss, rmse)`` the
    host knows right away, ``read()`` those it has to fetch; ``bad`` is the step of the first non-finite loss once its row
    was seen (that row and the later ones are never returned); ``images(summary, step)`` draws the step just taken;
    ``n_timed`` / ``rate()`` clock the steps after the first.  ``rmse`` is None where the batches have no ground truth:
    RMSE_log is then a 0/0 masked mean, and the loss alone decides whether a step was bad."""

    def __init__(self, model, rmse_log, step0, has_gt, grad_sync):
        self.model, self.rmse_log, self.has_gt, self.grad_sync = model, rmse_log, has_gt, grad_sync
        self.step0 = self.taken = step0
        self.bad, self.t0, self.n_timed = None, None, 0

    def read(self):
        return []

    def rate(self):
        torch.cuda.synchronize()
        return self.n_timed / (time.perf_counter() - self.t0)


class EagerStepper(_Stepper):
    """``model.train_step``: every step's loss is read as it is taken."""
    mode = "eager"

    def step(self, data):
        out = self.model.train_step(data, grad_sync=self.grad_sync)
        self.taken, self.data = self.taken + 1, data
        loss = float(out["loss"])
        if self.t0 is None:
            self.t0 = time.perf_counter()
        else:
            self.n_timed += 1
        if not np.isfinite(loss):
            self.bad = self.taken
            return []
        rmse = float(out["RMSE_log"])
        return [(self.taken, loss, rmse if self.has_gt else None)]

    def images(self, summary, step):
        summary.images(step, self.data, self.model.last_pyramid, self.data["camera"], has_gt=self.has_gt)


class GraphStepper(_Stepper):
    """``training.GraphedTrainStep``: the first batch runs its eager warm-up step (a real step: the same trajectory as the
    eager loop) and the step is captured once; every later batch is copied into its static buffers and replayed.  Each step
    ends with the device-side step log (``training.TrainStepLog``, ``log_rows`` rows), so ``step`` returns nothing and the
    host reads only at ``read()``; the rows from the first non-finite loss on are discarded, the replayed steps after it
    included."""
    mode = "graph"

    def __init__(self, model, rmse_log, step0, has_gt, grad_sync, opt, log_rows, dev):
        super().__init__(model, rmse_log, step0, has_gt, grad_sync)
        self.opt, self.log_rows, self.dev = opt, log_rows, dev
        self.runner = self.step_log = self.geometry = None
        self.logged = step0                            # the last step whose log row the host has read

    def step(self, data):
        from . import training as TR
        check_graph_batch(data, self.geometry)
        if self.runner is None:
            self.geometry = _geometry(data)
            self.step_log = TR.TrainStepLog(self.log_rows, self.dev)
            self.runner = TR.GraphedTrainStep(self.model, data, self.opt, warmup=1, grad_sync=self.grad_sync,
                                              step_log=self.step_log, loss=self.model.train_loss)
            torch.cuda.synchronize()
            self.t0 = time.perf_counter()
        else:
            self.runner(data)
            self.n_timed += 1
        self.taken += 1
        return []

    def read(self):
        if self.runner is None or self.bad is not None:
            return []
        rows, first_bad = self.step_log.read()
        out = []
        for i, (loss, rmse) in enumerate(rows):
            if first_bad >= 0 and i + self.logged - self.step0 >= first_bad:
                break
            if self.has_gt:
                self.rmse_log._update(torch.tensor(rmse))                       # the compiled RMSE_log Mean
            rmse = float(self.rmse_log.result())
            out.append((self.logged + i + 1, float(loss), rmse if self.has_gt else None))
        self.logged += len(rows)
        if first_bad >= 0:
            self.bad = self.step0 + first_bad + 1
        return out

    def images(self, summary, step):
        summary.images(step, self.runner.static, self.runner.pyramid, self.runner.camera, has_gt=self.has_gt)


def train_loop(args, stepper, ckpts, summary, epochs, step0=0, rank=0, validate=None):
    """The training loop over ``epochs`` = (count, epoch -> batches); steps are numbered from ``step0``.  Returns the status.

    The rows a step returns are reported at once (printed by rank 0 and handed to ``summary``, a TrainSummaryWriter or None);
    the stepper is asked to ``read`` every ``--summary_interval`` steps counted from ``step0``, where ``--save_every`` divides
    the step (no checkpoint is written from unread rows) and at every epoch end.  The images of a ``--summary_interval``-th
    step are drawn after its rows are in (they tell whether it was finite) and before the next batch is handed over.
    TerminateOnNaN (callbacks.py:69-132): a non-finite loss ends training with status 1 before any image or save; nothing of
    that epoch is saved.  Non-finite parameters behind a finite loss are caught where a checkpoint is due (``ckpts.save``
    raises): status 1, nothing written.  ``validate`` (``--enable_validation``): every epoch ends with its checkpoint, which
    rank 0 hands to ``validate(path)``."""
    def report(rows):
        for step, loss, rmse in rows:
            if rank == 0:
                print(format_step(step, loss, rmse))
            if summary is not None:
                summary.scalars(step, loss, rmse)

    n_epochs, epoch_batches = epochs
    step = step0
    try:
        for epoch in range(n_epochs):
            for data in epoch_batches(epoch):
                rows = stepper.step(data)
                step += 1
                summary_due = (step - step0) % args.summary_interval == 0
                save_due = args.save_every and step % args.save_every == 0
                report(rows + stepper.read() if summary_due or save_due else rows)
                if stepper.bad is not None:
                    break
                if summary_due and summary is not None:
                    stepper.images(summary, step)
                if save_due:
                    ckpts.save(step)
            report(stepper.read())
            if stepper.bad is not None:
                print(f"step {stepper.bad}: non-finite loss, training stopped (TerminateOnNaN): nothing of epoch {epoch + 1} "
                      "is saved")
                return 1
            if validate is not None:
                path = ckpts.save(step) or ckpts.path(step)
                if rank == 0:
                    validate(path)
        if stepper.n_timed and rank == 0:
            print(f"train ({stepper.mode}): {stepper.rate():.2f} steps/s over {stepper.n_timed} steps (the first step excluded)")
        if not args.save_every or step % args.save_every != 0:
            ckpts.save(step)
        return 0
    except _NonFiniteParameters as e:
        print(f"step {e.args[0]}: non-finite parameters, training stopped: no checkpoint of this state is written")
        return 1


def _train_setup(args, ablation, dev, depth_type):
    """main.py:73-109: the model with the weights ``load_weights`` finds, Adam(1e-4) with Keras's epsilon, RMSE_log as the
    tracked metric, and the optimizer state of the latest checkpoint when there is one.  Returns (model, optimizer, RMSE_log
    metric, the step to resume from, whether the batches carry ground truth)."""
    from . import training as TR
    from .metrics import RootMeanSquaredLogError
    if depth_type is None:
        depth_type = {"kitti-raw": "velodyne"}.get(args.dataset, "map")          # the loader's depth_type (main.py:79)
    model = M4Depth(depth_type=depth_type, nbre_levels=args.arch_depth, ablation_settings=ablation, is_training=True)
    model.load_numpy_weights(load_weights(args, ablation), dev)
    TR.set_trainable(model)
    opt = torch.optim.Adam(model.parameters(), lr=args.learning_rate, eps=1e-7,   # Keras Adam: epsilon 1e-7
                           capturable=args.graph)
    rmse_log = RootMeanSquaredLogError()
    model.compile(optimizer=opt, metrics=[rmse_log])
    model.train_loss = args.loss
    model.photo_smooth = 1e-3 if args.photo_smooth is None else args.photo_smooth
    model.photo_automask = not args.no_photo_automask
    model.photo_scale = args.photo_scale or "level"
    model.photo_sources = args.photo_sources or "prev"
    # a recording without depth.txt under --loss=photometric has no ground truth
    has_gt = args.dataset == "synthetic" or args.records_path is None or records_have_depth(args)
    ck = latest_checkpoint(args)
    step0 = 0
    if ck is not None:
        step0 = ck[1]
        opt_path = ck[0][:-4] + ".opt.pt"
        if os.path.isfile(opt_path):
            opt.load_state_dict(torch.load(opt_path, map_location=dev))
            _set_capturable(opt, args.graph, dev)
    return model, opt, rmse_log, step0, has_gt


def train(args, ablation, rank, world, dev, epochs=None, depth_type=None):
    """``--mode=train|finetune``: ``train_loop`` over ``epochs`` = (count, epoch -> batches) (default: the dataset's,
    ``default_epochs``; ``depth_type`` defaults to the dataset's) with the eager or the ``--graph`` stepper.  Several ranks =
    data parallel: the global batch is sharded and the gradients are averaged with one RCCL all-reduce per step
    (dist.all_reduce_gradients).  ``--log_dir``: rank 0 writes the summaries; the writer is closed on every way out."""
    summary = None
    if args.log_dir is not None and rank == 0:
        from .summaries import TrainSummaryWriter
        summary = TrainSummaryWriter(args.log_dir)
    try:
        torch.manual_seed(42)                                                   # tf.random.set_seed(42), main.py:76
        if epochs is None:
            epochs = default_epochs(args, rank, world, dev)
        model, opt, rmse_log, step0, has_gt = _train_setup(args, ablation, dev, depth_type)
        sync = D.all_reduce_gradients if world > 1 else None
        if args.graph:
            stepper = GraphStepper(model, rmse_log, step0, has_gt, sync, opt, args.summary_interval + 1, dev)
        else:
            stepper = EagerStepper(model, rmse_log, step0, has_gt, sync)
        validate = (lambda path: validate_checkpoint(args, ablation, dev, path)) if args.enable_validation else None
        return train_loop(args, stepper, CheckpointWriter(args, model, opt, rank), summary, epochs, step0, rank, validate)
    finally:
        if summary is not None:
            summary.close()


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
        metrics = evaluate_and_write(vargs, model, 0, 1, dev)
        del model
        torch.cuda.synchronize()
    return metrics


def evaluate_and_write(args, model, rank, world, dev):
    """``evaluate``, then what rank 0 writes from it: the perfs file where there are metrics and, in ``--mode=validation``,
    the best-N update with its lines.  Returns the metrics."""
    metrics, consistency = evaluate(args, model, rank, world, dev)
    if metrics is not None and rank == 0:
        write_perfs(args, model, metrics)
    if args.mode == "validation" and rank == 0:
        write_validation(args, metrics, consistency)
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


def eval_streams(args, model, dev):
    """Streaming evaluation with ``--eval_streams`` B slots (m4depth_amd.stream_eval): per step one ``stream_step`` (or a
    ``GraphedStream`` replay) and one per-sample metric launch into a preallocated [n_steps,B,7] / [n_steps,B] device log; no
    host read of any mask.  After the last step: one copy of the log to the host, the fold in the sequential order, and the
    folded (total, count) loaded into the compiled metrics for the writer.

    ``--consistency`` adds one launch pair per step (``consistency.ConsistencyScorer``) into an [n_steps,B,6] / [n_steps,B] log
    of its own and, after the last step, ``perfs-consistency-<dataset>.txt`` and ``consistency-frames-<dataset>.txt``.  With
    ground truth the seven metrics are computed exactly as without the flag; without it (a recording without depth.txt, csv
    files without a depth column) they are skipped.  ``--refine_pose`` puts ``pose_refine.PoseRefiner`` in front of every step
    (eager launches, also before a graph replay, which copies the frame's motion into its static inputs): the network and the
    scorer get the refined motion, its rows go to an [n_steps,B,8] log and, after the last step, to
    ``pose-refine-frames-<dataset>.txt``.  ``--fused VOXEL`` puts ``fusion.FusedDepth`` behind every step (eager launches on the
    frame the network saw): the fused depth is scored by a second per-sample metric launch into an [n_steps,B,7] log of its own,
    the pixels rendered go to an [n_steps,B] log, and after the last step ``perfs-fused-<dataset>.txt`` and
    ``fused-frames-<dataset>.txt`` are written; ``perfs-<dataset>.txt`` is what it is without the flag.
    Returns (whether the seven were computed, the six consistency means or None)."""
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
    refiner = None
    if args.refine_pose:                                           # a fixed schedule of launches in front of every step
        from . import pose_refine as PR
        refiner = PR.from_args(args, copy_estimate=args.graph)
        p_rows = torch.empty((n_steps, B, len(PR.COLUMNS)), dtype=torch.float32, device=dev)
    fuser = None
    if getattr(args, "fused", None) is not None:                   # four launches and a second metric pair behind every step
        from . import fusion as FU
        fuser = FU.from_args(args)
        rows_f = torch.empty((n_steps, B, 7), dtype=torch.float32, device=dev)
        counted_f = torch.empty((n_steps, B), dtype=torch.uint8, device=dev)
        hits = torch.zeros((n_steps, B), dtype=torch.int64, device=dev)           # the launches add: zeroed once, here
        fused = None
    active = (sched.cells[..., 0] >= 0).sum(axis=1)                # the schedule's, known on the host without a device read
    runner, t0 = None, None
    for step, batch in enumerate(ds):
        if step == 1:                                              # the first step is the warm-up (allocations, graph capture)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        frame = {"RGB_im": batch["RGB_im"], "rot": batch["rot"], "trans": batch["trans"], "new_traj": batch["reset"],
                 "camera": batch["camera"]}
        if refiner is not None:                                    # the network and the scorer see the refined motion
            frame = refiner.step(frame, batch["reset"], batch["active"], p_rows[step])
        if args.graph:
            if runner is None:
                runner = GraphedStream(model, frame)
            est = runner(frame)["depth"]
        else:
            est = model.stream_step(frame)["depth"]
        if refiner is not None:
            refiner.keep(frame, est)
        if has_gt:
            nops.depth_metrics_per_sample(batch["depth"], est, batch["new_traj"], batch["active"], 80., rows=rows[step],
                                          counted=counted[step])
        if scorer is not None:
            scorer.step(frame, est, batch["reset"], batch["active"], c_rows[step], c_counted[step])
        if fuser is not None:                                      # the motion is the refined one under --refine_pose
            if fused is None:
                fused = torch.empty_like(est)
            fuser.step(est, frame["RGB_im"], frame["rot"], frame["trans"], frame["camera"], batch["reset"], out=fused,
                       hits=hits[step])
            nops.depth_metrics_per_sample(batch["depth"], fused, batch["new_traj"], batch["active"], 80., rows=rows_f[step],
                                          counted=counted_f[step])
    if has_gt:
        rows_h, counted_h = rows.cpu().numpy(), counted.cpu().numpy()
    if fuser is not None:
        rows_f_h, hits_h, volumes = rows_f.cpu().numpy(), hits.cpu().numpy(), fuser.stats()
    if scorer is not None:
        c_rows_h, c_counted_h = c_rows.cpu().numpy(), c_counted.cpu().numpy()
    if refiner is not None:
        p_rows_h = p_rows.cpu().numpy()
    if t0 is not None:
        dt = time.perf_counter() - t0
        n = int(active[1:].sum())
        print(f"eval_streams {B} slots ({args.eval_streams_policy}, {'graph' if args.graph else 'eager'}"
              f"{', consistency' if scorer is not None else ''}{', refine_pose' if refiner is not None else ''}"
              f"{', fused' if fuser is not None else ''}): {n / dt:.1f} "
              f"sample-frames/s over {n} active sample-frames of {n_steps - 1} steps (the first step excluded)")
    if has_gt:
        total, count = SE.fold(rows_h, counted_h, sched.cells)
        for i, m in enumerate(model.compiled_metrics):
            m.load_state(torch.tensor(total[i], dtype=torch.float32, device=dev), count)
    means = None
    if scorer is not None:
        c_total, c_count, frames = SE.fold_consistency(c_rows_h, c_counted_h, sched.cells)
        means = SE.fold_result(c_total, c_count)
        os.makedirs(args.ckpt_dir, exist_ok=True)
        CS.write_perfs(CS.perfs_path(args.ckpt_dir, args.dataset), means)
        CS.write_frames(CS.frames_path(args.ckpt_dir, args.dataset), frames)
        for name, v in zip(CS.COLUMNS, means):
            print(f"consistency {name}: {v:.6f}")
        print(f"wrote {CS.perfs_path(args.ckpt_dir, args.dataset)} and {CS.frames_path(args.ckpt_dir, args.dataset)} "
              f"({c_count} counted frames)")
    if refiner is not None:
        frames = SE.fold_pose_refine(p_rows_h, sched.cells)
        os.makedirs(args.ckpt_dir, exist_ok=True)
        PR.write_frames(PR.frames_path(args.ckpt_dir, args.dataset), frames)
        applied = sum(1 for _, _, row in frames if row[6] != 0)
        print(f"wrote {PR.frames_path(args.ckpt_dir, args.dataset)} ({applied} of {len(frames)} frames refined)")
    if fuser is not None:
        total_f, count_f = SE.fold(rows_f_h, counted_h, sched.cells)
        means_f = SE.fold_result(total_f, count_f)
        h, w = fused.shape[1:3]
        frames = SE.fold_fused(rows_h, rows_f_h, hits_h, counted_h, sched.cells, h * w)
        os.makedirs(args.ckpt_dir, exist_ok=True)
        FU.write_perfs(FU.perfs_path(args.ckpt_dir, args.dataset), means_f)
        FU.write_frames(FU.frames_path(args.ckpt_dir, args.dataset), frames)
        dropped = sum(v["dropped_full"] for v in volumes)
        cover = float(np.mean([row[0] for _, _, row in frames])) if frames else 0.0
        print(f"fused depth at {fuser.voxel:g} m (K {fuser.trunc}, min_frames {fuser.min_frames}, "
              f"{'whole range' if fuser.window is None else 'window %d' % fuser.window}"
              f"{'' if fuser.interp == 'nearest' else ', %s sampling' % fuser.interp}): mean coverage {cover:.4f} over "
              f"{len(frames)} counted frames, AbsRel raw {SE.fold_result(total, count)[0]:.6f} fused {means_f[0]:.6f}, "
              f"{dropped} samples dropped by full tables" + (" (raise --fused_slots_log2)" if dropped else ""))
        print(f"wrote {FU.perfs_path(args.ckpt_dir, args.dataset)} and {FU.frames_path(args.ckpt_dir, args.dataset)}")
    return has_gt, means


def evaluate_sequences(args, model, rank, world, dev):
    """The eval / validation loop over sequence batches (eager ``test_step``, or with ``--graph`` an eager warm-up, a metric
    reset and a ``GraphedSequence`` replayed for every batch) or over the streaming frames of a real dataset (4-D, no
    ``--db_seq_len``: always ``test_step``); the compiled metrics accumulate.  ``--host_input``: the synthetic batches are
    generated before the loop, uploaded inside it, and the rate after the first batch is printed."""
    host_input = args.host_input and args.dataset == "synthetic"
    batches = input_batches(args, "eval", rank, world, dev, on_host=host_input)
    if host_input:
        batches = list(batches)                    # generation is not part of the measured loop
    runner, n_frames, t_loop = None, 0, None
    for batch_idx, data in enumerate(batches):
        if host_input:
            if batch_idx == 1:                                 # the first batch is the warm-up (allocations, graph capture)
                torch.cuda.synchronize()
                t_loop, n_frames = time.perf_counter(), 0
            data = _upload(data, dev)
            n_frames += data["RGB_im"].shape[0] * data["RGB_im"].shape[1]
        if not args.graph or data["RGB_im"].dim() == 4:
            model.test_step(data)
            continue
        if runner is None:
            model.test_step(data)              # eager warm-up (state and scratch allocation, packed weights)
            for m in model.compiled_metrics:
                m.reset_state()
            runner = GraphedSequence(model, data)
        model.graphed_test_step(data, runner)
    if t_loop is not None:
        torch.cuda.synchronize()
        dt = time.perf_counter() - t_loop
        if rank == 0 and n_frames:
            print(f"host-resident input (pinned memory, PCIe copy inside the step): {n_frames / dt:.1f} frames/s per rank "
                  f"over {n_frames} frames")


def evaluate(args, model, rank, world, dev):
    """``--mode=eval|validation`` of ``model`` (compiled with the 7 metrics).  Returns (metrics, consistency): the metrics
    all-gathered over the ranks (numpy [7]), or None where the set has no ground truth (``--consistency``), and the six
    consistency means, or None without ``--consistency``."""
    consistency = None
    if args.eval_streams:
        has_gt, consistency = eval_streams(args, model, dev)
        if not has_gt:
            return None, consistency
    else:
        evaluate_sequences(args, model, rank, world, dev)
    gathered = D.all_gather_metric_states(model.compiled_metrics, dev)
    return D.reduce_metric_states(gathered).cpu().numpy(), consistency


def predict(args, model, batches, rank, dev):
    """``--mode=predict``: every frame of ``batches`` through ``predict_step`` (``--stream``: ``stream_step``, with ``--graph``
    replayed from a ``GraphedStream`` built on the first frame).  With ``--save_dir`` each estimate goes to the
    ``PredictionWriter`` (its export launch follows the forward -- or the graph replay -- on the same stream; nothing is
    kept); without it rank 0 writes them all to ``<ckpt_dir>/predictions.npy``."""
    from .export import FrameNamer, PredictionWriter
    writer = namer = runner = t_save = refiner = None
    if args.refine_pose:
        from . import pose_refine as PR
        refiner = PR.from_args(args, copy_estimate=args.graph)
    if args.save_dir is not None:
        writer = PredictionWriter(args.save_dir, args.save_format, args.save_panels, near=args.save_range[0],
                                  far=args.save_range[1], err_max=args.save_err_max, cloud=args.save_cloud,
                                  cloud_step=args.cloud_stride, cloud_frame=args.cloud_frame, cloud_views=args.cloud_views,
                                  cloud_min_views=args.cloud_min_views, cloud_tol=args.cloud_tol, save_conf=args.save_conf,
                                  save_map=args.save_map, map_min_frames=args.map_min_frames,
                                  map_slots_log2=args.map_slots_log2, save_mesh=args.save_mesh, mesh_trunc=args.mesh_trunc,
                                  mesh_min_frames=args.mesh_min_frames, mesh_slots_log2=args.mesh_slots_log2,
                                  save_fused=getattr(args, "save_fused", False),
                                  fused_window=getattr(args, "fused_window", None),
                                  fused_interp=getattr(args, "fused_interp", None) if getattr(args, "save_fused", False) else None,
                                  save_fused_view=getattr(args, "save_fused_view", False))
        want_gt = any(p in ("gt", "err") for p in writer.panels)
    preds = []
    for data in batches:
        frames = [data]                            # one streaming frame of a real dataset (4-D), or a batch of sequences
        if data["RGB_im"].dim() != 4:
            frames = [dict({k: data[k][:, t] for k in ("depth", "RGB_im", "rot", "trans", "new_traj")}, camera=data["camera"])
                      for t in range(data["RGB_im"].shape[1])]
        for frame in frames:
            if not args.stream:
                est = model.predict_step(frame)["depth"]
            else:
                sf = _stream_frame(frame, dev)
                if refiner is not None:                        # the network and the clouds see the refined motion
                    sf = refiner.step(sf, sf["new_traj"], torch.ones_like(sf["new_traj"], dtype=torch.uint8))
                    frame = dict(frame, rot=sf["rot"], trans=sf["trans"])
                if not args.graph:
                    est = model.stream_step(sf)["depth"]
                else:
                    if runner is None:
                        runner = GraphedStream(model, sf)
                    est = runner(sf)["depth"]
                if refiner is not None:
                    refiner.keep(sf, est)
            if writer is None:
                preds.append(est.cpu().numpy())
                continue
            if namer is None:
                namer = FrameNamer(est.shape[0])
                t_save = time.perf_counter()
            cloud = {}
            if writer.needs_geometry:                         # the chain's launches follow the forward / the replay on its stream
                cloud = dict(rot=frame["rot"], trans=frame["trans"], camera=frame["camera"], reset=frame["new_traj"])
            writer.submit(est, namer(frame["new_traj"]), gt=frame.get("depth") if want_gt else None,
                          rgb=frame["RGB_im"] if "rgb" in writer.panels or writer.needs_geometry else None, **cloud)
    if writer is None:
        if rank == 0:
            os.makedirs(args.ckpt_dir, exist_ok=True)
            np.save(os.path.join(args.ckpt_dir, "predictions.npy"), np.concatenate(preds, axis=0))
        return
    writer.close()
    if namer is not None:
        dt = time.perf_counter() - t_save
        print(f"predict: wrote {writer.frames} frames ({', '.join(writer.summary())}) to {args.save_dir}: "
              f"{writer.frames / dt:.1f} frames/s, the first forward excluded from the clock")


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    check_args(parser, args)
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
    if args.mode == "predict":
        predict(args, model, input_batches(args, "predict", rank, world, dev), rank, dev)
    else:
        evaluate_and_write(args, model, rank, world, dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
