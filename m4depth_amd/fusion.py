"""Fused depth per frame: the estimates of a trajectory fused into a TSDF volume and the volume rendered back into every frame.

``FusedDepth`` is the per-step piece ``main.py --eval_streams B --fused VOXEL`` drives: clear the volumes of the slots that
restart, chain the frame's motion into the camera-to-world pose, fuse the estimate (``network_ops.tsdf_integrate``, two
launches) and march every pixel's ray through the volume (``network_ops.tsdf_raycast``, one launch).  The result is the rendered
depth where the volume has a surface and the raw estimate elsewhere: it has the estimate's pixel set, so the seven depth metrics
of the two compare directly.  Nothing synchronises; the definitions are in include/m4depth_hip.h.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import network_ops as nops

NEAR, FAR = 1.0, 80.0            # the march range of --fused: the exporters' default near and the metrics' max_d
FRAMES_HEADER = "\t".join(("trajectory", "frame", "coverage", "abs_rel", "abs_rel_fused"))


class FusedDepth:
    """Owns ``b`` TSDF volumes of 2^``slots_log2`` slots (32 bytes per slot: 134 MB per sample at the default 22), allocated at
    the first step, and the [b,7] float64 pose chain.  ``voxel`` in metres, ``trunc`` the truncation distance in voxels (2..8),
    a voxel is rendered once ``min_frames`` frames updated it; ``window``: None marches the whole [near, far], W >= 1 only W
    truncation distances around the raw estimate of the pixel."""

    def __init__(self, voxel, trunc=4, min_frames=2, slots_log2=22, near=NEAR, far=FAR, window=None):
        voxel = float(np.float32(voxel))
        if not (0 < voxel < float("inf")):
            raise ValueError(f"voxel must be a finite edge length > 0, got {voxel}")
        trunc, min_frames, slots_log2 = int(trunc), int(min_frames), int(slots_log2)
        if not nops.TSDF_TRUNC[0] <= trunc <= nops.TSDF_TRUNC[1] or min_frames < 1 or not 6 <= slots_log2 <= 26:
            raise ValueError(f"need trunc in {nops.TSDF_TRUNC[0]}..{nops.TSDF_TRUNC[1]}, min_frames >= 1 and slots_log2 in 6..26, "
                             f"got {trunc}, {min_frames}, {slots_log2}")
        if not (0 < float(near) < float(far)):
            raise ValueError(f"need 0 < near < far, got {near}, {far}")
        if window is not None and int(window) < 1:
            raise ValueError(f"window must be >= 1 truncation distances (None: the whole range), got {window}")
        self.voxel, self.trunc, self.min_frames, self.slots_log2 = voxel, trunc, min_frames, slots_log2
        self.near, self.far = float(near), float(far)
        self.window = None if window is None else int(window)
        self.state = None
        self.pose = None

    def step(self, est, rgb, rot, trans, camera, reset, out=None, hits=None, views_est=None):
        """One frame batch, on the current stream: returns fused [b,h,w,1] (``out`` when given).  ``est`` [b,h,w,1] the
        estimate, ``rgb`` [b,h,w,3], ``rot`` [b,4] / ``trans`` [b,3] the frame's motion as the network got it, ``camera`` {f, c}
        [b,2], ``reset``: uint8 / bool [b] DEVICE mask of the samples that start a trajectory with this frame (never read by the
        host; the first step resets everybody).  ``hits``: int64 [b], zeroed by the caller, takes the pixels rendered per sample.
        ``views_est``: what is fused instead of ``est`` (a filtered copy); the guide and the fill stay the raw estimate."""
        if est.dim() != 4 or est.shape[3] != 1:
            raise ValueError(f"est: expected [b,h,w,1], got {tuple(est.shape)}")
        b, h, w = est.shape[:3]
        if not (torch.is_tensor(reset) and reset.is_cuda):
            raise ValueError("reset: expected a uint8 / bool [b] device mask (the host never reads it)")
        first = self.state is None
        if first:
            self.state = nops.tsdf_state(b, self.slots_log2, est.device)       # cleared
            self.pose = torch.empty((b, 7), dtype=torch.float64, device=est.device)
        elif int(self.state["b"]) != b:
            raise ValueError(f"est has {b} samples, the volumes {int(self.state['b'])}")
        else:
            nops.tsdf_clear(self.state, reset)
        nops.pose_accumulate(rot, trans, self.pose, reset=reset, force_all=first)
        f, c = camera["f"], camera["c"]
        nops.tsdf_integrate(est if views_est is None else views_est, rgb, f, c, self.pose, self.voxel, self.trunc, self.state,
                            near=self.near, far=self.far)
        return nops.tsdf_raycast(self.state, f, c, self.pose, h, w, self.voxel, self.trunc, self.min_frames, near=self.near,
                                 far=self.far, guide=est if self.window else None, window=self.window, fill=est, out=out,
                                 hits=hits)

    def stats(self):
        """Per sample {occupied, dropped_range, dropped_full, updates} of the volumes as they are (one wait)."""
        if self.state is None:
            return []
        return [dict(zip(nops.TSDF_STATS, row)) for row in self.state["stats"].cpu().tolist()]


def from_args(args):
    return FusedDepth(args.fused, trunc=args.fused_trunc, min_frames=args.fused_min_frames, slots_log2=args.fused_slots_log2,
                      window=args.fused_window)


def perfs_path(ckpt_dir, dataset):
    return os.path.join(ckpt_dir, "perfs-fused-" + dataset + ".txt")


def frames_path(ckpt_dir, dataset):
    return os.path.join(ckpt_dir, "fused-frames-" + dataset + ".txt")


def write_perfs(path, means):
    """The seven means of the fused depth, one per line, in the number format of ``perfs-<dataset>.txt``."""
    np.savetxt(path, np.asarray(means, np.float32), fmt='%.18e', delimiter='\t', newline='\n')


def read_perfs(path):
    return np.loadtxt(path, dtype=np.float64, ndmin=1).astype(np.float32)


def write_frames(path, frames):
    """A header line, then one tab-separated line per counted frame in the sequential order: trajectory, frame, coverage (pixels
    rendered / pixels), AbsRel of the raw and of the fused depth (%.9e: float32 round-trips)."""
    with open(path, "w") as fh:
        fh.write(FRAMES_HEADER + "\n")
        for t, f, row in frames:
            fh.write("\t".join([str(int(t)), str(int(f))] + ["%.9e" % float(v) for v in row]) + "\n")


def read_frames(path):
    """[(trajectory, frame, float32 [3] = coverage, abs_rel, abs_rel_fused)] of ``write_frames``."""
    with open(path) as fh:
        lines = fh.read().splitlines()
    if not lines or lines[0] != FRAMES_HEADER:
        raise ValueError(f"{path}: not a fused-frames file (header {lines[:1]})")
    out = []
    for line in lines[1:]:
        p = line.split("\t")
        out.append((int(p[0]), int(p[1]), np.array([float(v) for v in p[2:]], np.float32)))
    return out
