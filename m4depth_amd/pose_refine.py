"""Pose refinement: the frame-to-frame motion a trajectory gives is aligned to the images before the network sees it
(the definition is in include/m4depth_hip.h, "Pose refinement").

Gauss-Newton direct image alignment of the current frame against the previous frame and the previous frame's ESTIMATED depth,
started from the given motion, coarse to fine over a box pyramid, per sample on the device: a fixed schedule of launches
(``network_ops.pose_align_*``), no host read, no data-dependent control flow -- whether a sample's result is taken or its given
motion passed through bit for bit is decided on the device.  It runs eagerly in front of ``M4Depth.stream_step`` or a
``GraphedStream`` replay.

A trajectory's first two frames pass through: the first has no previous frame, and the estimate of the first frame was made
without parallax.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import network_ops as nops
from .stream_eval import fold_pose_refine as fold            # noqa: F401  (the 8-column fold lives beside the others)

# UNTUNED: chosen from the literature's usual ranges and the synthetic scene of tests/pose_align_ref.py, never scored on real
# footage (README, "Pose refinement": how to check them).  The one place these defaults live.
DEFAULTS = dict(strides=(8, 4, 2),          # coarse to fine; full resolution costs the most and was not needed on the synthetic scene
                iters=4,                    # Gauss-Newton iterations per stride
                huber=0.1,                  # grey levels (images in [0,1])
                damping=1e-6,               # Levenberg factor on diag(H/N)
                prior=(0.0, 0.0),           # (lambda_t per m^2, lambda_r per rad^2) towards the given pose; 0 = off
                caps=(0.05, math.radians(0.5)),   # a correction beyond (metres, radians) is rejected
                min_cover=0.5)              # least valid fraction of the finest level

COLUMNS = ("cost_before", "cost_after", "cover", "d_trans", "d_angle", "iterations", "applied", "reserved")
FRAMES_HEADER = "\t".join(("trajectory", "frame") + COLUMNS)


class PoseRefiner:
    """Keeps each slot's previous image (by reference, with its pyramid) and estimate and refines every step's motion
    against them.  ``copy_estimate``: whether the estimate's producer overwrites its output on the next step, as for
    ``consistency.ConsistencyScorer``."""

    def __init__(self, copy_estimate, strides=None, iters=None, huber=None, damping=None, prior=None, caps=None, min_cover=None):
        given = dict(strides=strides, iters=iters, huber=huber, damping=damping, prior=prior, caps=caps, min_cover=min_cover)
        for k, v in DEFAULTS.items():
            setattr(self, k, v if given[k] is None else given[k])
        self.strides = tuple(int(s) for s in self.strides)
        self.iters = int(self.iters)
        if not self.strides or any(s < 1 or s & (s - 1) for s in self.strides) or self.iters < 1:
            raise ValueError(f"PoseRefiner: strides must be powers of two and iters >= 1, got {self.strides} and {self.iters}")
        self.copy_estimate = bool(copy_estimate)
        self._levels = max(s.bit_length() - 1 for s in self.strides)
        self._images = None          # {stride: [B, H/stride, W/stride, 3]} of the previous step
        self._est = None
        self._was_reset = None       # the previous step's reset mask: its estimate was made without parallax

    def _pyramid(self, image):
        levels = nops.image_pyramid_box(image, self._levels) if self._levels else []
        return {1 << i: lvl for i, lvl in enumerate([image] + levels)}

    def step(self, frame, reset, active, row_out=None):
        """The frame dict with ``rot`` / ``trans`` refined (new tensors; the given ones are not written).  ``reset`` [B]: the
        slot restarts with this frame; ``active`` [B]: the slot holds a frame (uint8 / bool device masks).  ``row_out`` [B,8]
        (a view into a device log) gets ``COLUMNS``.  The first step after construction passes everything through."""
        image = frame["RGB_im"]
        if not image.is_contiguous():
            raise ValueError("PoseRefiner: RGB_im must be a dense [B,H,W,3] tensor")
        reset = reset.view(torch.uint8) if reset.dtype == torch.bool else reset
        images = self._pyramid(image)
        ready = self._images is not None and self._est is not None and self._images[1].shape == image.shape
        out = frame
        if not ready:
            if row_out is not None:
                row_out.zero_()
        else:
            _, h, w, _ = image.shape
            off = torch.bitwise_or(reset, self._was_reset)
            cam = frame["camera"]
            ws = nops.pose_align_begin(frame["rot"], frame["trans"], h, w)
            for s in self.strides:
                for _ in range(self.iters):
                    nops.pose_align_iterate(ws, images[s], self._images[s], self._est, cam["f"], cam["c"], off, active, s,
                                            self.huber, self.damping, self.prior)
            rot, trans, _ = nops.pose_align_end(ws, frame["rot"], frame["trans"], off, active, h, w, self.min_cover, self.caps,
                                                rows=row_out)
            out = dict(frame, rot=rot, trans=trans)
        self._images = images
        self._was_reset = reset
        return out

    def keep(self, frame, est):
        """After the estimate of ``frame`` exists: it is the depth the next step aligns against."""
        if not self.copy_estimate:
            self._est = est
        elif self._est is None or self._est.shape != est.shape:
            self._est = est.clone()
        else:
            self._est.copy_(est)


def from_args(args, copy_estimate):
    """The refiner of the driver's ``--refine_pose*`` options (``options.check_refine_args`` has filled them in)."""
    return PoseRefiner(copy_estimate, strides=args.refine_pose_strides, iters=args.refine_pose_iters, prior=args.refine_pose_prior,
                       caps=(args.refine_pose_max[0], math.radians(args.refine_pose_max[1])))


def frames_path(ckpt_dir, dataset):
    return os.path.join(ckpt_dir, "pose-refine-frames-" + dataset + ".txt")


def write_frames(path, frames):
    """A header line, then one tab-separated line per frame in the sequential order: trajectory, frame, the eight values
    (%.9e: float32 round-trips)."""
    with open(path, "w") as fh:
        fh.write(FRAMES_HEADER + "\n")
        for t, f, row in frames:
            fh.write("\t".join([str(int(t)), str(int(f))] + ["%.9e" % float(v) for v in row]) + "\n")


def read_frames(path):
    """[(trajectory, frame, float32 [8])] of ``write_frames``."""
    with open(path) as fh:
        lines = fh.read().splitlines()
    if not lines or lines[0] != FRAMES_HEADER:
        raise ValueError(f"{path}: not a pose-refine-frames file (header {lines[:1]})")
    out = []
    for line in lines[1:]:
        p = line.split("\t")
        out.append((int(p[0]), int(p[1]), np.array([float(v) for v in p[2:]], np.float32)))
    return out
