"""Checkpoint files of the training workflow: the ``<ckpt_dir>/train`` directory (latest, retention), the validation log and the
best-N backup of ``<ckpt_dir>/best`` (the roles of the reference's CustomCheckpointCallback and BestCheckpointManager,
callbacks.py:69-132 / 173-240, and of main.py:111-144's validation branch).

A checkpoint is ``ckpt-<step>.npz`` (the network) plus ``ckpt-<step>.opt.pt`` (the optimizer state), side by side.
"""
from __future__ import annotations

import collections
import csv
import os
import shutil

# the 7 metrics of metrics.default_metrics(), in that order, under the column names of the reference's validation_perfs.csv
METRIC_COLUMNS = ("abs_rel", "sq_rel", "rmse", "rmsel", "a1", "a2", "a3")
_LOWER_IS_BETTER = ("rmse", "rmsel", "abs_rel", "sq_rel")
_HIGHER_IS_BETTER = ("a1", "a2", "a3")

# What the best-N manager judges on: the table's columns and which of them are lower-is-better (the rest: higher is better).
# A candidate beats a row when it wins strictly on a majority -- more than half -- of the columns.
Criterion = collections.namedtuple("Criterion", ("columns", "lower"))
DEFAULT_CRITERION = Criterion(METRIC_COLUMNS, _LOWER_IS_BETTER)            # today's seven: a majority is more than 3 of 7
# a validation set without ground truth (main.py --val_consistency): the photometric part of the reprojection-consistency score
PHOTO_CRITERION = Criterion(("photo",), ("photo",))


def criterion_wins(criterion, candidate, row):
    """How many of the criterion's columns ``candidate`` beats ``row`` on (strictly)."""
    wins = 0
    for m in criterion.columns:
        c, r = float(candidate[m]), float(row[m])
        wins += (r > c) if m in criterion.lower else (r < c)
    return wins


def checkpoint_steps(d):
    """Steps of the ``ckpt-<step>.npz`` files in directory ``d``, ascending."""
    if not os.path.isdir(d):
        return []
    steps = []
    for f in os.listdir(d):
        if f.startswith("ckpt-") and f.endswith(".npz") and f[5:-4].isdigit():
            steps.append(int(f[5:-4]))
    return sorted(steps)


def latest_checkpoint(d):
    """(path, step) of the newest ``ckpt-<step>.npz`` of ``d`` (tf.train.latest_checkpoint), or None."""
    steps = checkpoint_steps(d)
    return (os.path.join(d, f"ckpt-{steps[-1]}.npz"), steps[-1]) if steps else None


def checkpoint_files(npz_path):
    """The files one checkpoint is made of: the network and, when there is one, the optimizer state."""
    files = [npz_path]
    opt = npz_path[:-4] + ".opt.pt"
    if os.path.isfile(opt):
        files.append(opt)
    return files


def prune_checkpoints(d, max_keep):
    """Keeps the newest ``max_keep`` checkpoints of ``d`` (0 = all); returns the removed steps."""
    if max_keep <= 0:
        return []
    gone = checkpoint_steps(d)[:-max_keep]
    for step in gone:
        for f in checkpoint_files(os.path.join(d, f"ckpt-{step}.npz")):
            os.remove(f)
    return gone


def best_checkpoint(ckpt_dir):
    """Path of the checkpoint ``<ckpt_dir>/best/checkpoint`` names (the weights eval / predict use, main.py:116,156), or None
    when there is no such file."""
    best = os.path.join(ckpt_dir, "best")
    state = os.path.join(best, "checkpoint")
    if not os.path.isfile(state):
        return None
    with open(state) as fh:
        for line in fh:
            key, _, value = line.partition(":")
            if key.strip() == "model_checkpoint_path":
                return os.path.join(best, value.strip().strip('"'))
    raise ValueError(f"{state} names no model_checkpoint_path")


def format_validation_line(metrics):
    """One line of ``validation-perfs.txt``: the 7 metrics as '%.4f' each followed by two tabs (main.py:138-142)."""
    return "".join(format(float(v), ".4f") + "\t\t" for v in metrics) + "\n"


def append_validation_perfs(ckpt_dir, metrics, name="validation-perfs.txt"):
    """One more line of ``<ckpt_dir>/<name>`` (validation-consistency.txt: the six means of main.py --val_consistency)."""
    os.makedirs(ckpt_dir, exist_ok=True)
    with open(os.path.join(ckpt_dir, name), "a") as fh:
        fh.write(format_validation_line(metrics))


def majority_wins(candidate, row):
    """How many of the 7 metrics ``candidate`` beats ``row`` on (strictly): lower rmse / rmsel / abs_rel / sq_rel, higher
    a1 / a2 / a3."""
    wins = sum(1 for m in _LOWER_IS_BETTER if float(row[m]) > float(candidate[m]))
    return wins + sum(1 for m in _HIGHER_IS_BETTER if float(row[m]) < float(candidate[m]))


class BestCheckpointManager:
    """Backup copies of the best ``keep_top_n`` networks by validation metrics, in ``best_dir`` (callbacks.py:173-240).

    ``best_dir/validation_perfs.csv`` holds one row per backup (columns abs_rel, sq_rel, rmse, rmsel, a1, a2, a3, ckpt_name),
    ``best_dir/checkpoint`` names the most recent backup.  ``update_backup(perfs)`` judges the latest checkpoint of
    ``train_dir`` with the reference's rule, quirks included:

      * while the table has fewer than ``keep_top_n`` rows, the checkpoint is backed up without comparison;
      * otherwise the rows are scanned in file order and the FIRST row the candidate beats on a majority (> 3 of 7) counts:
        the candidate is appended, and if the table then holds more than ``keep_top_n`` rows, that row and its files go.
        No row beaten: nothing changes.

    ``criterion`` (default: the seven metrics) names the columns and their direction; a majority is more than half of them.  A
    ``best_dir`` whose table has other columns than the criterion is refused (ValueError), never mixed."""

    def __init__(self, train_dir, best_dir, keep_top_n=1, criterion=DEFAULT_CRITERION):
        self.train_dir, self.backup_dir, self.max_keep = train_dir, best_dir, int(keep_top_n)
        self.criterion = criterion
        os.makedirs(self.backup_dir, exist_ok=True)
        self.perfs_file_name = os.path.join(self.backup_dir, "validation_perfs.csv")

    def read_table(self):
        if not os.path.isfile(self.perfs_file_name):
            return []
        with open(self.perfs_file_name, newline="") as fh:
            rd = csv.DictReader(fh)
            rows = list(rd)
        want = list(self.criterion.columns) + ["ckpt_name"]
        if list(rd.fieldnames or []) != want:
            raise ValueError(f"{self.perfs_file_name} has the columns {rd.fieldnames}, this run judges on {want}: the best "
                             "directory was made with another criterion -- use another --ckpt_dir or remove it")
        return rows

    def _write_table(self, rows):
        with open(self.perfs_file_name, "w", newline="") as fh:
            names = list(self.criterion.columns) + ["ckpt_name"]
            wr = csv.DictWriter(fh, fieldnames=names)
            wr.writeheader()
            for r in rows:
                wr.writerow({k: r[k] for k in names})

    def backup_last_ckpt(self):
        """Copies the latest checkpoint of the training directory (network and optimizer state); returns its file name."""
        latest = latest_checkpoint(self.train_dir)
        if latest is None:
            raise FileNotFoundError(f"no checkpoint to back up in {self.train_dir}")
        for f in checkpoint_files(latest[0]):
            shutil.copy2(f, self.backup_dir)
        return os.path.basename(latest[0])

    def _name_latest(self, name):
        with open(os.path.join(self.backup_dir, "checkpoint"), "w") as fh:
            fh.write('model_checkpoint_path: "%s"\nall_model_checkpoint_paths: "%s"\n' % (name, name))

    def update_backup(self, perfs):
        """``perfs``: {column: value} of the criterion's columns (or their list in that order; default: the 7 metrics in
        METRIC_COLUMNS order).  Returns True when the latest checkpoint was backed up."""
        columns = self.criterion.columns
        if not isinstance(perfs, dict):
            perfs = dict(zip(columns, perfs))
        cand = {m: float(perfs[m]) for m in columns}
        rows = self.read_table()
        if len(rows) < self.max_keep:
            cand["ckpt_name"] = self.backup_last_ckpt()
            self._write_table(rows + [cand])
            self._name_latest(cand["ckpt_name"])
            return True
        for i, row in enumerate(rows):
            if 2 * criterion_wins(self.criterion, cand, row) > len(columns):
                cand["ckpt_name"] = self.backup_last_ckpt()
                rows = rows + [cand]
                if len(rows) > self.max_keep:
                    gone = rows.pop(i)["ckpt_name"]
                    if gone not in [r["ckpt_name"] for r in rows]:       # the same file may sit in two rows
                        for f in checkpoint_files(os.path.join(self.backup_dir, gone)):
                            os.remove(f)
                self._write_table(rows)
                self._name_latest(cand["ckpt_name"])
                return True
        return False
