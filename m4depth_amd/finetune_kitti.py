"""KITTI finetuning on a joint KITTI + cropped Mid-Air stream -- the counterpart of the reference's ``finetune-kitti.py``
(:41-88), step 2 of its training recipe (scripts/1b-finetune-kitti.sh):

    python -m m4depth_amd.finetune_kitti --arch_depth=6 --ckpt_dir=ckpt --records_path=data \\
           --db_path_config=datasets_location.json --enable_validation --val_records_path=data/kitti-raw-filtered/val_data

* KITTI ``<records_path>/kitti-raw-filtered/train_data`` at db_seq_len 4 / seq_len 4, and Mid-Air
  ``<records_path>/midair/train_data`` at 8 / 4 with the ``"finetune"`` augmentation and random crops to KITTI's frame size;
* both repeat forever and every BATCH is drawn from one of the two with p = 0.5 (a generator seeded by ``--seed``);
* an epoch is 2 x the KITTI length in steps, and the run lasts ``--finetune_steps // steps_per_epoch + 1`` epochs from the
  latest checkpoint of ``<ckpt_dir>/train`` on, with velodyne-type supervision;
* checkpoints, TerminateOnNaN, ``--enable_validation``, ``--log_dir`` and ``--graph`` behave as in ``m4depth_amd.main --mode=finetune``
  (one captured step serves both datasets: they share the geometry).
"""
from __future__ import annotations

import os
import sys

import numpy as np

from . import dist as D
from . import main as M


def finetune_schedule(kitti_batches, finetune_steps=20000):
    """(steps per epoch, epochs to run) of finetune-kitti.py:80-88: the joint length is twice KITTI's, and the run lasts
    ``finetune_steps // steps_per_epoch + 1`` epochs beyond the resume point."""
    if kitti_batches < 1:
        raise ValueError("the KITTI training set yields no batch at this batch size")
    steps = 2 * int(kitti_batches)
    return steps, int(finetune_steps) // steps + 1


class JointBatches:
    """tf.data.Dataset.sample_from_datasets([a.repeat(), b.repeat()], weights=[p, 1 - p]) over BATCHES: every step takes the
    next whole batch of one source, chosen by a generator seeded with ``seed``; each source restarts (re-shuffled by its own
    loader) when it runs out.  ``epoch(n)`` yields the next n batches."""

    def __init__(self, sources, seed, p=0.5):
        self.sources, self.p = list(sources), float(p)
        self.rng = np.random.default_rng(seed)
        self._its = [None] * len(self.sources)
        self.drawn = []                                  # the source index of every batch handed out

    def _next(self, k):
        for _ in range(2):
            if self._its[k] is None:
                self._its[k] = iter(self.sources[k])
            try:
                return next(self._its[k])
            except StopIteration:
                self._its[k] = None
        raise ValueError(f"joint finetuning: source {k} yields no batch")

    def choose(self):
        return 0 if self.rng.random() < self.p else 1

    def epoch(self, n_steps):
        for _ in range(n_steps):
            k = self.choose()
            self.drawn.append(k)
            yield self._next(k)


def build_parser():
    p = M.build_parser()
    p.description = "M4Depth (MI355X native) KITTI finetuning on a joint KITTI + Mid-Air stream (finetune-kitti.py)"
    p.add_argument("--finetune_steps", type=int, default=20000,
                   help="steps beyond the resume point the epoch count is derived from (finetune-kitti.py:84)")
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    args.mode, args.dataset = "finetune", "kitti-raw"
    if args.records_path is None or args.db_path_config is None:
        parser.error("finetune_kitti needs --records_path (holding kitti-raw-filtered/train_data and midair/train_data) "
                     "and --db_path_config")
    if args.finetune_steps < 0:
        parser.error("--finetune_steps must be >= 0")
    M.check_train_args(parser, args)
    rank, world, _, dev = D.init_from_env()
    if dev.type != "cuda":
        raise SystemExit("m4depth_amd.finetune_kitti needs a GPU: the hot path has no CPU fallback")
    from . import dataloaders as dl
    roots = M.dataset_roots(args.db_path_config)
    lo, hi = D.shard_range(args.batch_size, rank, world)
    augment = not args.no_augmentation
    kitti = dl.get_loader("kitti-raw")
    kw = {"out_size": [args.height, args.width]} if args.height and args.width else {}
    kitti_ds = kitti.get_dataset("finetune", dl.DataloaderParameters(
        roots, os.path.join(args.records_path, "kitti-raw-filtered", "train_data"), 4, 4, augment),
        batch_size=hi - lo, device=dev, seed=args.seed, shard=(rank, world), **kw)
    midair = dl.get_loader("midair")
    midair_ds = midair.get_dataset("finetune", dl.DataloaderParameters(
        roots, os.path.join(args.records_path, "midair", "train_data"), 8, 4, augment),
        batch_size=hi - lo, out_size=kitti.out_size, crop=True, device=dev, seed=args.seed, shard=(rank, world))
    steps_per_epoch, n_epochs = finetune_schedule(len(kitti_ds), args.finetune_steps)
    joint = JointBatches([kitti_ds, midair_ds], args.seed)
    if rank == 0:
        print(f"joint KITTI + Mid-Air finetuning: {steps_per_epoch} steps per epoch, {n_epochs} epochs")
    return M.train(args, M.ablation_from_args(args), rank, world, dev,
                   epochs=(n_epochs, lambda epoch: joint.epoch(steps_per_epoch)), depth_type="velodyne")


if __name__ == "__main__":
    sys.exit(main())
