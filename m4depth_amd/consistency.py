"""Reprojection consistency: a label-free score of the depth maps ``stream_step`` writes.

Every frame of a trajectory but its first is scored against the frame before it: the previous image warped into the current
frame with the ESTIMATED depth is compared with the current image (``photo``: SSIM + L1, the photometric error of the
training loss without auto-masking), and the estimate's projected depth with the previous frame's estimate at the query
(``geo``: Bian et al., NeurIPS 2019).  One fused launch pair per step (``network_ops.consistency_per_sample``), nothing
synchronises; the definition is in include/m4depth_hip.h.

``photo`` is the criterion; ``geo`` is a diagnostic with a blind spot (under sideways motion a common scale error of both
estimates cancels in it, under forward motion far depth makes it small).  ``photo_id`` is the error of the unwarped previous
image -- the score of "nothing moved" -- and ``better`` the fraction of pixels where the warp beats it.
"""
from __future__ import annotations

import os

import numpy as np

from . import network_ops as nops
from .stream_eval import fold_consistency as fold            # noqa: F401  (the 6-column fold lives beside the 7-column one)

COLUMNS = ("photo", "photo_id", "better", "geo", "cover", "geo_cover")
FRAMES_HEADER = "\t".join(("trajectory", "frame") + COLUMNS)


class ConsistencyScorer:
    """Keeps each slot's previous image and estimate and scores every step against them.

    ``copy_estimate``: whether the estimate's producer overwrites its output on the next step -- ``GraphedStream``'s output
    buffer does (the scorer then copies it into a buffer of its own after the launch), the eager ``stream_step`` returns a
    fresh tensor (kept by reference).  The previous step's image tensor is always kept by reference, never copied."""

    def __init__(self, copy_estimate):
        self.copy_estimate = bool(copy_estimate)
        self._image = None
        self._est = None

    def step(self, frame, est, reset, active, rows, counted):
        """Scores ``est`` [B,H,W,1], the estimate of ``frame`` (RGB_im, rot, trans, camera as for ``stream_step``), into ``rows``
        [B,6] / ``counted`` [B] (views into a device log).  ``reset`` [B]: the slot restarted its state with this frame (its
        previous buffers hold another trajectory); ``active`` [B]: the slot holds a frame.  The first step after construction
        counts nothing."""
        image = frame["RGB_im"]
        if self._image is None or self._image.shape != image.shape:
            rows.zero_()
            counted.zero_()
        else:
            nops.consistency_per_sample(est, self._est, image, self._image, frame["rot"], frame["trans"], frame["camera"]["f"],
                                        frame["camera"]["c"], reset, active, rows=rows, counted=counted)
        self._image = image
        if not self.copy_estimate:
            self._est = est
        elif self._est is None or self._est.shape != est.shape:
            self._est = est.clone()
        else:
            self._est.copy_(est)
        return rows, counted


def perfs_path(ckpt_dir, dataset):
    return os.path.join(ckpt_dir, "perfs-consistency-" + dataset + ".txt")


def frames_path(ckpt_dir, dataset):
    return os.path.join(ckpt_dir, "consistency-frames-" + dataset + ".txt")


def write_perfs(path, means):
    """The six means, one per line, in the number format of ``perfs-<dataset>.txt``."""
    np.savetxt(path, np.asarray(means, np.float32), fmt='%.18e', delimiter='\t', newline='\n')


def read_perfs(path):
    return np.loadtxt(path, dtype=np.float64, ndmin=1).astype(np.float32)


def write_frames(path, frames):
    """A header line, then one tab-separated line per counted frame in the sequential order: trajectory, frame, the six values
    (%.9e: float32 round-trips)."""
    with open(path, "w") as fh:
        fh.write(FRAMES_HEADER + "\n")
        for t, f, row in frames:
            fh.write("\t".join([str(int(t)), str(int(f))] + ["%.9e" % float(v) for v in row]) + "\n")


def read_frames(path):
    """[(trajectory, frame, float32 [6])] of ``write_frames``."""
    with open(path) as fh:
        lines = fh.read().splitlines()
    if not lines or lines[0] != FRAMES_HEADER:
        raise ValueError(f"{path}: not a consistency-frames file (header {lines[:1]})")
    out = []
    for line in lines[1:]:
        p = line.split("\t")
        out.append((int(p[0]), int(p[1]), np.array([float(v) for v in p[2:]], np.float32)))
    return out
