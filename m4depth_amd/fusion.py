"""The device geometry of a batch of trajectories: ``TrajectoryChain`` owns the camera-to-world pose chain and, as asked for, the
ring of the multi-view check, one TSDF volume and one voxel map per sample, and issues every launch on them (definitions:
include/m4depth_hip.h).  ``export.PredictionWriter`` (``main.py --mode=predict --save_cloud / --save_map / --save_mesh /
--save_fused``) and ``FusedDepth`` (``main.py --eval_streams B --fused VOXEL``) are its two consumers.  The second renders the
volume back into every frame: the rendered depth where the volume has a surface and the raw estimate elsewhere, so it has the
estimate's pixel set and the seven depth metrics of the two compare directly.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import network_ops as nops

NEAR, FAR = 1.0, 80.0            # the march range of --fused: the exporters' default near and the metrics' max_d
FRAMES_HEADER = "\t".join(("trajectory", "frame", "coverage", "abs_rel", "abs_rel_fused"))

# the companions of a volume's and of a map's voxel edge: (name, default, lowest, highest or None).  Tables start at 2^6 slots
# here (tests use small ones); the command line has a floor of its own (options.CLI_SLOTS_LOG2_MIN)
VOLUME_COMPANIONS = (("trunc", 4, *nops.TSDF_TRUNC), ("min_frames", 2, 1, None), ("slots_log2", 22, 6, 26))
MAP_COMPANIONS = (("min_frames", 2, 1, None), ("slots_log2", 21, 6, 26))


class TrajectoryChain:
    """The device state of ``b`` trajectories that run side by side, allocated at the first step, and the launches on it.
    Always ``pose``, the [b,7] float64 camera-to-world poses, and the range [``near``, ``far``] every reader of an estimate
    keeps to.  ``voxel=VOXEL`` (metres): ``state``, a TSDF volume per sample on a hashed grid of 2^``slots_log2`` slots (32 bytes
    each: 134 MB at 22), ``trunc`` the truncation distance in voxels; a voxel is rendered or meshed once ``min_frames`` frames
    updated it; ``window=W`` marches only W truncation distances around a pixel's raw estimate (None: the whole range);
    ``interp``: how ``render`` samples the field, "nearest" or "trilinear" (``network_ops.tsdf_render``).
    ``views=K`` (1..8): the multi-view check, a ring of the last K + 1 estimates and poses ((K+1) b h w floats) and the filtered
    copy -- a pixel survives if at least ``min_views`` (default min(2, K)) of the up to K earlier frames of its trajectory
    confirm it within ``tol`` = (pixels, relative depth).  ``map_voxel=VOXEL``: ``map_state``, a voxel map per sample, a hash
    table of 2^``map_slots_log2`` slots (168 MB at 21) whose voxels count once ``map_min_frames`` frames saw them.  A companion
    given as None takes its default (``VOLUME_COMPANIONS``, ``MAP_COMPANIONS``) and is checked only with its voxel edge.
    ``names``: what the caller's own options for these keywords are called, for the ValueError texts.

    A step is ``advance`` and then, in this order, whichever of ``filter``, ``fuse``, ``render``, ``compact`` and ``merge`` the
    consumer wants: each is one ``network_ops`` call on the current stream.  Only ``extract_*`` and ``stats`` synchronise."""

    def __init__(self, voxel=None, trunc=None, min_frames=None, slots_log2=None, near=NEAR, far=FAR, window=None, views=0,
                 min_views=None, tol=(1.0, 0.01), map_voxel=None, map_min_frames=None, map_slots_log2=None, names=None,
                 interp="nearest"):
        def name(k):                                       # what the caller calls the keyword ``k``
            return (names or {}).get(k, k)

        if not (0 < float(near) < float(far)):
            raise ValueError(f"need 0 < near < far, got {near}, {far}")
        self.near, self.far = float(near), float(far)
        views = int(views)
        if not 0 <= views <= nops.VIEWS_MAX:
            raise ValueError(f"{name('views')} must be 0 (off) or 1..{nops.VIEWS_MAX}, got {views}")
        if min_views is not None and not views:
            raise ValueError(f"{name('min_views')} needs {name('views')} >= 1")
        min_views = min(2, views) if min_views is None else int(min_views)
        if views and not 1 <= min_views <= views:
            raise ValueError(f"{name('min_views')} must be in 1..{views}, got {min_views}")
        tol = tuple(float(v) for v in tol)
        if len(tol) != 2 or not (tol[0] > 0 and tol[1] > 0):
            raise ValueError(f"{name('tol')}: expected (pixels > 0, relative depth > 0), got {tol}")
        self.views, self.min_views, self.tol = views, min_views, tol
        self.map_voxel, self.map_min_frames, self.map_slots_log2 = self._group(
            name, "map_", map_voxel, MAP_COMPANIONS, (map_min_frames, map_slots_log2))
        self.voxel, self.trunc, self.min_frames, self.slots_log2 = self._group(
            name, "", voxel, VOLUME_COMPANIONS, (trunc, min_frames, slots_log2))
        if window is not None and int(window) < 1:
            raise ValueError(f"{name('window')} must be >= 1 truncation distances (None: the whole range), got {window}")
        self.window = None if window is None else int(window)
        if interp not in nops.TSDF_INTERP:
            raise ValueError(f"{name('interp')} must be one of {', '.join(nops.TSDF_INTERP)}, got {interp!r}")
        self.interp = interp
        self.pose = self.state = self.map_state = None
        self.stamp = 0                                     # advances so far: the stamp of a step's vertices in the map
        self._views = self._filtered = self._counts = None  # depth_views' ring and ages, the filtered copy, the [b,h,w] counts
        self._reset, self._first = None, True              # of the step under way: set by advance, read by filter

    @staticmethod
    def _group(name, prefix, voxel, companions, values):
        """A voxel edge (None: off) as a float32 length and its companions as integers (None: the default)."""
        ints = [(name(prefix + c), default if v is None else int(v), lo, hi) for (c, default, lo, hi), v in zip(companions, values)]
        if voxel is not None:
            voxel = float(np.float32(voxel))
            if not (0 < voxel < float("inf")):
                raise ValueError(f"{name(prefix + 'voxel')}: the voxel edge must be a finite length > 0, got {voxel}")
            if any(v < lo or (hi is not None and v > hi) for _, v, lo, hi in ints):
                need = [f"{n} >= {lo}" if hi is None else f"{n} in {lo}..{hi}" for n, _, lo, hi in ints]
                raise ValueError(f"need {', '.join(need[:-1])} and {need[-1]}, got {', '.join(str(v) for _, v, _, _ in ints)}")
        return (voxel, *(v for _, v, _, _ in ints))

    def advance(self, rot, trans, reset=None, clear=False):
        """The frame's motion ``rot`` [b,4] / ``trans`` [b,3] into the poses; the samples of ``reset`` (uint8 / bool [b] device
        mask, None: nobody) start a trajectory with this frame.  ``clear``: first empty their volumes and maps -- at every step
        for a consumer that never reads its mask, only after extracting what a set flag ended for one that has the flags on the
        host.  The first step allocates, resets everybody and clears nothing: fresh state is clear."""
        first = self.pose is None
        if first:
            b, dev = rot.shape[0], rot.device
            self.pose = torch.empty((b, 7), dtype=torch.float64, device=dev)
            if self.map_voxel is not None:
                self.map_state = nops.voxel_map_state(b, self.map_slots_log2, dev)
            if self.voxel is not None:
                self.state = nops.tsdf_state(b, self.slots_log2, dev)
        elif clear:
            if self.map_voxel is not None:
                nops.voxel_map_clear(self.map_state, reset)
            if self.voxel is not None:
                nops.tsdf_clear(self.state, reset)
        self._reset, self._first = reset, first
        self.stamp += 1
        nops.pose_accumulate(rot, trans, self.pose, reset=reset, force_all=first)

    def filter(self, est, camera, counts=None):
        """``est`` [b,h,w,1] against the earlier frames of its trajectories: returns the filtered copy (a buffer of the chain's).
        ``counts``: uint8 [b,h,w] for the confirming views per pixel, given at every step or never (then a buffer of the chain's).
        ``est`` may be a buffer the next graph replay overwrites: the ring copy happens in this launch, on this stream."""
        if self._views is None:
            b, h, w = est.shape[:3]
            self._views = nops.depth_views_state(b, h, w, self.views, est.device)
            self._filtered = torch.empty((b, h, w, 1), dtype=torch.float32, device=est.device)
            self._counts = torch.empty((b, h, w), dtype=torch.uint8, device=est.device) if counts is None else None
        return nops.depth_views(est, camera["f"], camera["c"], self.pose, self._views, reset=self._reset, force_all=self._first,
                                tol_px=self.tol[0], tol_rel=self.tol[1], min_views=self.min_views, depth_f=self._filtered,
                                n_views=self._counts if counts is None else counts)[1]

    def fuse(self, est, rgb, camera):
        """``est`` (the filtered copy where the views check is on) into the volumes, at every pixel: two launches."""
        nops.tsdf_integrate(est, rgb, camera["f"], camera["c"], self.pose, self.voxel, self.trunc, self.state, near=self.near,
                            far=self.far)

    def render(self, raw, camera, fill=False, out=None, hits=None, normal=None, colour=None, view=None):
        """The volumes as they are, seen from the frame: [b,h,w,1] (``out`` when given).  ``raw``: the RAW estimate, the guide
        of a windowed march and, with ``fill``, what a pixel without a surface keeps; ``hits``: as ``tsdf_raycast``'s;
        ``normal`` / ``colour`` / ``view``: ``tsdf_render``'s optional destinations.  The nearest rule with none of them is
        ``tsdf_raycast``'s launch."""
        args = (self.state, camera["f"], camera["c"], self.pose, raw.shape[1], raw.shape[2], self.voxel, self.trunc, self.min_frames)
        kw = dict(near=self.near, far=self.far, guide=raw if self.window else None, window=self.window,
                  fill=raw if fill else None, out=out, hits=hits)
        if self.interp == "nearest" and normal is None and colour is None and view is None:
            return nops.tsdf_raycast(*args, **kw)
        return nops.tsdf_render(*args, interp=self.interp, normal=normal, colour=colour, view=view, **kw)

    def compact(self, est, rgb, camera, step, world, vertices, counts):
        """``est`` as ``depth_cloud``'s ``vertices`` / ``counts``, in the trajectory's frame (``world``) or the camera's."""
        nops.depth_cloud(est, rgb, camera["f"], camera["c"], step=step, near=self.near, far=self.far,
                         pose=self.pose if world else None, vertices=vertices, counts=counts)

    def merge(self, vertices, counts):
        """The step's compacted world-frame vertices into the maps, stamped with the step's number."""
        nops.voxel_map_integrate(vertices, counts, self.map_voxel, self.stamp, self.map_state)

    def extract_volume(self, s):
        """The surface of sample ``s``: ``network_ops.tsdf_extract``'s (keys, vertices, triangles, stats).  Waits."""
        return nops.tsdf_extract(self.state, s, self.min_frames, self.voxel)

    def extract_map(self, s):
        """The map of sample ``s``: ``network_ops.voxel_map_extract``'s (keys, vertices, stats).  Waits."""
        return nops.voxel_map_extract(self.map_state, s, self.map_min_frames, self.map_voxel)

    def stats(self):
        """Per sample {occupied, dropped_range, dropped_full, updates} of the volumes as they are (one wait)."""
        if self.state is None:
            return []
        return [dict(zip(nops.TSDF_STATS, row)) for row in self.state["stats"].cpu().tolist()]


class FusedDepth(TrajectoryChain):
    """A chain with a volume (``voxel`` and its companions, ``near`` / ``far``, ``window``, ``interp``: the chain's keywords), no
    views check and no map, stepped by a consumer that has the reset flags on the device only."""

    def step(self, est, rgb, rot, trans, camera, reset, out=None, hits=None, views_est=None, normal=None, colour=None, view=None):
        """One frame batch, on the current stream: returns fused [b,h,w,1] (``out`` when given).  ``est`` [b,h,w,1] the
        estimate, ``rgb`` [b,h,w,3], ``rot`` [b,4] / ``trans`` [b,3] the frame's motion as the network got it, ``camera`` {f, c}
        [b,2], ``reset``: the DEVICE mask of ``advance`` (never read by the host; the first step resets everybody).  ``hits``:
        int64 [b], zeroed by the caller, takes the pixels rendered per sample.  ``views_est``: what is fused instead of ``est``
        (a filtered copy); the guide and the fill stay the raw estimate.  ``normal`` / ``colour`` / ``view``: ``render``'s."""
        if est.dim() != 4 or est.shape[3] != 1:
            raise ValueError(f"est: expected [b,h,w,1], got {tuple(est.shape)}")
        if not (torch.is_tensor(reset) and reset.is_cuda):
            raise ValueError("reset: expected a uint8 / bool [b] device mask (the host never reads it)")
        if self.state is not None and int(self.state["b"]) != est.shape[0]:
            raise ValueError(f"est has {est.shape[0]} samples, the volumes {int(self.state['b'])}")
        self.advance(rot, trans, reset, clear=True)
        self.fuse(est if views_est is None else views_est, rgb, camera)
        return self.render(est, camera, fill=True, out=out, hits=hits, normal=normal, colour=colour, view=view)


def from_args(args):
    return FusedDepth(args.fused, trunc=args.fused_trunc, min_frames=args.fused_min_frames, slots_log2=args.fused_slots_log2,
                      window=args.fused_window, interp=args.fused_interp)


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
