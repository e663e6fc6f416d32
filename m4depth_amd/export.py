"""Prediction export -- the back end of ``main.py --mode=predict --save_dir``, the mirror of the dataloaders' front end.

The reference's predict loop hands ``d_est``, ``d_gt`` and ``i_rgb`` of every frame to the user (main.py:150-172); what users
do with them is save a depth map and a colourised estimate beside the ground truth and the image.  Here one kernel per frame
batch (``network_ops.depth_export``) writes the estimate in a dataset's own 16-bit encoding and as ready-to-save RGB8 panels,
``PredictionWriter`` moves them through a ring of pinned buffers, and host threads do the PNG compression: the predict loop
never waits for the host unless every slot of the ring is in flight, and host memory is ``slots`` frames however long the run.

With ``cloud=True`` the writer also keeps one camera-to-world pose per sample on the device (``network_ops.pose_accumulate``),
turns every estimate into a dense list of coloured vertices (``network_ops.depth_cloud``) and writes it as a binary PLY file
beside the PNGs; the host never redoes the camera model or the pose chain, and never reads a vertex count before the slot's
event has passed.

With ``cloud_views=K`` a cloud keeps only the pixels that up to K earlier frames of the sample's trajectory confirm
(``network_ops.depth_views``: a forward-backward reprojection check against a ring of the last K estimates and poses on the
device); the depth PNG and the panels keep showing the raw estimate.

With ``save_map=VOXEL`` the vertices of every step are also merged, on the device, into one voxel map per sample
(``network_ops.voxel_map_integrate``: a hash table of integer sums); when a sample's trajectory ends the map is extracted,
written as ``map.ply`` into the trajectory's directory by a worker thread (``write_map_ply``) and the table cleared.

With ``save_mesh=VOXEL`` the estimate of every step is also fused, on the device, into one truncated signed distance field per
sample (``network_ops.tsdf_integrate``: a hashed voxel grid, two launches); when a sample's trajectory ends the surface is
extracted by naive surface nets (``network_ops.tsdf_extract``), written as ``mesh.ply`` into the trajectory's directory by a
worker thread (``write_mesh_ply``) and the volume cleared.  ``save_fused=True`` also renders that volume into every frame's
camera (``network_ops.tsdf_raycast``, one launch) and writes the fused depth map as ``<frame>_fused.png``.
"""
from __future__ import annotations

import os
import queue
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import network_ops as nops

FORMATS = ("kitti16", "midair16")
PANELS = ("rgb", "est", "gt", "err")

# anchor colours of the table (position in 0..1, r, g, b): dark blue (far / no error) over green and yellow to dark red
# (near / err_max), interpolated linearly per channel
_ANCHORS = ((0.0, 24, 15, 92), (0.2, 35, 95, 180), (0.4, 30, 170, 160), (0.6, 120, 210, 70), (0.8, 250, 190, 40),
            (1.0, 180, 20, 30))
_INVALID = (0, 0, 0)


def default_lut():
    """[257,3] uint8 colour table: rows 0..255 interpolate the anchor colours, row 256 is the colour of invalid pixels."""
    pos = np.array([a[0] for a in _ANCHORS], np.float64)
    x = np.arange(256, dtype=np.float64) / 255.0
    lut = np.empty((257, 3), np.uint8)
    for c in range(3):
        lut[:256, c] = np.rint(np.interp(x, pos, np.array([a[1 + c] for a in _ANCHORS], np.float64))).astype(np.uint8)
    lut[256] = _INVALID
    return lut


class FrameNamer:
    """Relative output paths ``s{slot:02d}_t{trajectory:04d}/{frame:06d}`` of the ``b`` samples of a step, from the step's
    host-side ``new_traj``: a sample's trajectory counter advances where ``new_traj`` is set (and on its first frame), its
    frame counter restarts there."""

    def __init__(self, b):
        self.traj = [-1] * int(b)
        self.frame = [0] * int(b)

    def __call__(self, new_traj):
        flags = np.asarray(new_traj.cpu() if torch.is_tensor(new_traj) else new_traj, dtype=bool).reshape(-1)
        if len(flags) != len(self.traj):
            raise ValueError(f"new_traj has {len(flags)} samples, the namer {len(self.traj)}")
        names = []
        for s, new in enumerate(flags):
            if new or self.traj[s] < 0:
                self.traj[s] += 1
                self.frame[s] = 0
            else:
                self.frame[s] += 1
            names.append(f"s{s:02d}_t{self.traj[s]:04d}/{self.frame[s]:06d}")
        return names


def read_depth_png(path, fmt):
    """A ``<name>_depth.png`` of ``PredictionWriter`` as float32 depth, with the arithmetic of the dataloaders: value / 256
    (kitti16), 512 / float16(bits) (midair16; the invalid code 0x7C00 = +Inf reads as depth 0)."""
    from PIL import Image
    if fmt not in FORMATS:
        raise ValueError(f"fmt: expected one of {FORMATS}, got {fmt!r}")
    with Image.open(path) as im:
        bits = np.asarray(im, dtype=np.uint16)
    if fmt == "kitti16":
        return bits.astype(np.float32) / np.float32(256.0)
    with np.errstate(divide="ignore"):
        return np.float32(512.0) / bits.view(np.float16).astype(np.float32)


PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])
_PLY_PROPERTIES = ["property float x", "property float y", "property float z", "property uchar red", "property uchar green",
                   "property uchar blue", "property uchar alpha"]
CLOUD_FRAMES = ("world", "camera")


def write_cloud_ply(path, vertices, pose):
    """``vertices``: [n,16] uint8 (or n ``PLY_VERTEX`` records) as ``network_ops.depth_cloud`` writes them, stored verbatim as
    the body of a binary little-endian PLY file; ``pose``: the 7 float64 of the frame's camera-to-world pose, kept in a
    comment line at full precision."""
    body = np.ascontiguousarray(vertices).view(np.uint8).reshape(-1, 16)
    header = ["ply", "format binary_little_endian 1.0",
              "comment pose " + " ".join("%.17g" % v for v in np.asarray(pose, np.float64).reshape(7)),
              "element vertex %d" % len(body)] + _PLY_PROPERTIES + ["end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(body.data)


def read_cloud_ply(path):
    """A ``<name>_cloud.ply`` of ``PredictionWriter``: (xyz float32 [n,3], rgba uint8 [n,4], pose float64 [7])."""
    with open(path, "rb") as fh:
        lines = []
        while not lines or lines[-1] != "end_header":
            line = fh.readline()
            if not line or len(lines) > 64:
                raise ValueError(f"{path}: no PLY header")
            lines.append(line.decode("ascii").rstrip("\r\n"))
        body = fh.read()
    poses = [l for l in lines if l.startswith("comment pose ")]
    counts = [l for l in lines if l.startswith("element vertex ")]
    if lines[:2] != ["ply", "format binary_little_endian 1.0"] or len(poses) != 1 or len(counts) != 1 \
            or [l for l in lines if l.startswith("property ")] != _PLY_PROPERTIES:
        raise ValueError(f"{path}: not a point cloud of PredictionWriter")
    n = int(counts[0].split()[2])
    if len(body) != 16 * n:
        raise ValueError(f"{path}: {n} vertices in the header, {len(body)} bytes in the body")
    raw = np.frombuffer(body, np.uint8).reshape(n, 16)
    pose = np.array([float(v) for v in poses[0].split()[2:]], np.float64)
    if pose.shape != (7,):
        raise ValueError(f"{path}: the pose comment holds {pose.size} numbers")
    return raw[:, :12].copy().view(np.float32), raw[:, 12:].copy(), pose


_MAP_FIELDS = ("voxel", "min_frames", "observations", "dropped_range", "dropped_full", "occupied")


def write_map_ply(path, vertices, voxel, min_frames, stats):
    """The voxel map of a trajectory as a binary PLY file with the per-frame clouds' property list (``read_cloud_ply`` reads
    it): ``vertices`` [n,16] uint8 as ``network_ops.voxel_map_extract`` returns them, one per voxel in ascending key order --
    float x, y, z (the mean position of the voxel's points), uchar red, green, blue (their mean colour) and alpha = the number
    of frames that saw the voxel, capped at 255.  The map lives in the world frame: the pose comment is the identity.
    ``comment voxel_map`` holds the edge length, ``min_frames`` and the map's statistics ``stats`` (observations,
    dropped_range, dropped_full, occupied), as name value pairs."""
    body = np.ascontiguousarray(vertices).view(np.uint8).reshape(-1, 16)
    info = dict(stats, voxel="%.9g" % np.float32(voxel), min_frames=int(min_frames))
    header = ["ply", "format binary_little_endian 1.0", "comment pose 1 0 0 0 0 0 0",
              "comment voxel_map " + " ".join("%s %s" % (k, info[k]) for k in _MAP_FIELDS),
              "element vertex %d" % len(body)] + _PLY_PROPERTIES + ["end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(body.data)


def read_map_ply(path):
    """A ``map.ply`` of ``PredictionWriter(save_map=...)``: (xyz float32 [n,3], rgba uint8 [n,4], info) with ``info`` the
    ``comment voxel_map`` line as a dict -- voxel (float) and min_frames, observations, dropped_range, dropped_full, occupied
    (int)."""
    xyz, rgba, pose = read_cloud_ply(path)
    with open(path, "rb") as fh:
        head = fh.read(4096).split(b"end_header")[0].decode("ascii").splitlines()
    lines = [l.split()[2:] for l in head if l.startswith("comment voxel_map ")]
    if len(lines) != 1 or tuple(lines[0][0::2]) != _MAP_FIELDS or not np.array_equal(pose, [1, 0, 0, 0, 0, 0, 0]):
        raise ValueError(f"{path}: not a voxel map of PredictionWriter")
    info = {k: (float(v) if k == "voxel" else int(v)) for k, v in zip(lines[0][0::2], lines[0][1::2])}
    return xyz, rgba, info


_MESH_FIELDS = ("voxel", "trunc", "min_frames", "occupied", "dropped_range", "dropped_full", "updates", "quads_dropped")
PLY_FACE = np.dtype([("n", "u1"), ("vertex_indices", "<i4", (3,))])        # 13 bytes: a triangle of `property list uchar int`
_PLY_FACE_PROPERTY = "property list uchar int vertex_indices"


def write_mesh_ply(path, vertices, triangles, voxel, trunc, min_frames, stats):
    """The TSDF surface of a trajectory as a binary little-endian PLY mesh (MeshLab, CloudCompare and Open3D open it):
    ``vertices`` [n,16] uint8 and ``triangles`` [m,3] int32 as ``network_ops.tsdf_extract`` returns them -- the clouds' vertex
    properties (float x, y, z, uchar red, green, blue and alpha = the fewest frames that updated one of the cell's eight voxels,
    capped at 255), then ``element face`` with ``property list uchar int vertex_indices``, every face a triangle wound so that
    its normal points from the inside of the surface to the outside (towards the cameras that saw it).  World frame: the pose
    comment is the identity.  ``comment tsdf_mesh`` holds the edge length, the truncation in voxels, ``min_frames`` and
    ``stats`` (occupied, dropped_range, dropped_full, updates, quads_dropped) as name value pairs."""
    body = np.ascontiguousarray(vertices).view(np.uint8).reshape(-1, 16)
    tri = np.ascontiguousarray(triangles, dtype="<i4").reshape(-1, 3)
    if len(tri) and (tri.min() < 0 or tri.max() >= len(body)):
        raise ValueError(f"{path}: a triangle names a vertex outside 0..{len(body) - 1}")
    faces = np.zeros(len(tri), PLY_FACE)
    faces["n"] = 3
    faces["vertex_indices"] = tri
    info = dict(stats, voxel="%.9g" % np.float32(voxel), trunc=int(trunc), min_frames=int(min_frames))
    header = ["ply", "format binary_little_endian 1.0", "comment pose 1 0 0 0 0 0 0",
              "comment tsdf_mesh " + " ".join("%s %s" % (k, info[k]) for k in _MESH_FIELDS),
              "element vertex %d" % len(body)] + _PLY_PROPERTIES + ["element face %d" % len(faces), _PLY_FACE_PROPERTY,
                                                                    "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(body.data)
        fh.write(faces.tobytes())


def read_mesh_ply(path):
    """A ``mesh.ply`` of ``PredictionWriter(save_mesh=...)``: (xyz float32 [n,3], rgba uint8 [n,4], triangles int32 [m,3], info)
    with ``info`` the ``comment tsdf_mesh`` line as a dict -- voxel (float) and trunc, min_frames, occupied, dropped_range,
    dropped_full, updates, quads_dropped (int)."""
    with open(path, "rb") as fh:
        lines = []
        while not lines or lines[-1] != "end_header":
            line = fh.readline()
            if not line or len(lines) > 64:
                raise ValueError(f"{path}: no PLY header")
            lines.append(line.decode("ascii").rstrip("\r\n"))
        body = fh.read()
    info = [l.split()[2:] for l in lines if l.startswith("comment tsdf_mesh ")]
    elements = [l.split()[1:] for l in lines if l.startswith("element ")]
    if lines[:2] != ["ply", "format binary_little_endian 1.0"] or lines.count("comment pose 1 0 0 0 0 0 0") != 1 \
            or len(info) != 1 or tuple(info[0][0::2]) != _MESH_FIELDS or [e[0] for e in elements] != ["vertex", "face"] \
            or [l for l in lines if l.startswith("property ")] != _PLY_PROPERTIES + [_PLY_FACE_PROPERTY]:
        raise ValueError(f"{path}: not a TSDF mesh of PredictionWriter")
    n, m = int(elements[0][1]), int(elements[1][1])
    if len(body) != 16 * n + PLY_FACE.itemsize * m:
        raise ValueError(f"{path}: {n} vertices and {m} faces in the header, {len(body)} bytes in the body")
    raw = np.frombuffer(body[:16 * n], np.uint8).reshape(n, 16)
    faces = np.frombuffer(body[16 * n:], PLY_FACE)
    if m and ((faces["n"] != 3).any() or faces["vertex_indices"].min() < 0 or faces["vertex_indices"].max() >= n):
        raise ValueError(f"{path}: a face that is no triangle of the file's vertices")
    info = {k: (float(v) if k == "voxel" else int(v)) for k, v in zip(info[0][0::2], info[0][1::2])}
    return raw[:, :12].copy().view(np.float32), raw[:, 12:].copy(), faces["vertex_indices"].astype(np.int32), info


def read_conf_png(path, views):
    """A ``<name>_conf.png`` of ``PredictionWriter(save_conf=True)`` as the counts it was made of: uint8 [h,w], the number of
    earlier frames (0..``views``) that confirmed the pixel; the file holds ``count * 255 // views``."""
    from PIL import Image
    views = int(views)
    if not 1 <= views <= nops.VIEWS_MAX:
        raise ValueError(f"views: expected 1..{nops.VIEWS_MAX}, got {views}")
    with Image.open(path) as im:
        if im.mode != "L":
            raise ValueError(f"{path}: not an 8-bit grey image")
        grey = np.asarray(im, dtype=np.uint8).astype(np.int64)
    counts = (grey * views + 254) // 255
    if not np.array_equal(counts * 255 // views, grey):
        raise ValueError(f"{path}: not the confirmation counts of {views} views")
    return counts.astype(np.uint8)


class _Slot:
    def __init__(self, b, h, w, n_panels, dev, cloud_cap=0, conf=False, cloud_host=True, geometry=False, fused=False):
        self.depth_d = torch.empty((b, h, w), dtype=torch.int16, device=dev)
        self.depth_h = torch.empty((b, h, w), dtype=torch.int16).pin_memory()
        self.panels_d = self.panels_h = None
        if n_panels:
            self.panels_d = torch.empty((b, n_panels * h, w, 3), dtype=torch.uint8, device=dev)
            self.panels_h = torch.empty((b, n_panels * h, w, 3), dtype=torch.uint8).pin_memory()
        self.cloud_d = None
        if cloud_cap:
            self.cloud_d = torch.empty((b, cloud_cap, 16), dtype=torch.uint8, device=dev)
            self.counts_d = torch.empty(b, dtype=torch.int32, device=dev)
            if cloud_host:                                 # a writer of maps alone keeps the vertices on the device
                self.cloud_h = torch.empty((b, cloud_cap, 16), dtype=torch.uint8).pin_memory()
                self.counts_h = torch.empty(b, dtype=torch.int32).pin_memory()
                self.pose_h = torch.empty((b, 7), dtype=torch.float64).pin_memory()
        if cloud_cap or geometry:                          # (a writer of meshes alone has no vertex buffer)
            self.reset_d = torch.empty(b, dtype=torch.uint8, device=dev)
            self.reset_h = torch.empty(b, dtype=torch.uint8).pin_memory()
        self.conf_d = self.conf_h = None
        if conf:
            self.conf_d = torch.empty((b, h, w), dtype=torch.uint8, device=dev)
            self.conf_h = torch.empty((b, h, w), dtype=torch.uint8).pin_memory()
        self.fused_h = None
        if fused:                                          # the rendered volume: float32, its 16-bit form and the pixels rendered
            self.fused_f = torch.empty((b, h, w, 1), dtype=torch.float32, device=dev)
            self.fused_d = torch.empty((b, h, w), dtype=torch.int16, device=dev)
            self.fused_h = torch.empty((b, h, w), dtype=torch.int16).pin_memory()
            self.hits_d = torch.empty(b, dtype=torch.int64, device=dev)
            self.hits_h = torch.empty(b, dtype=torch.int64).pin_memory()
        self.event = torch.cuda.Event()
        self.pending = 0


class _TrajectoryProduct:
    """One per-trajectory product of the writer (the voxel map, the TSDF mesh): its device state, the directory of every
    sample's open trajectory, and the callables that are all the two differ in -- ``new_state(b, device)``;
    ``extract(state, s)`` -> (device arrays, stats, {counter of the writer: what this trajectory adds}); ``clear(state, mask)``;
    ``write(path, *host arrays, stats)``."""

    def __init__(self, file_name, new_state, extract, clear, write):
        self.file_name, self.new_state, self.extract, self.clear, self.write = file_name, new_state, extract, clear, write
        self.state = None                                  # allocated with the slots
        self.dirs = None                                   # set by the first step that went into the state


def _trajectory_options(flag, voxel, cloud_frame, reason, ints):
    """The option group of a trajectory product: ``voxel`` (None: off) as a float32 length and its companions ``ints`` = (name,
    value, default, lowest, highest or None) as integers (None: the default); the companions are checked only with the flag."""
    voxel = None if voxel is None else float(np.float32(voxel))
    ints = [(name, default if v is None else v, lo, hi) for name, v, default, lo, hi in ints]
    if voxel is not None:
        if not (0 < voxel < float("inf")):
            raise ValueError(f"{flag}: the voxel edge must be a finite length > 0, got {voxel}")
        if cloud_frame != "world":
            raise ValueError(f"{flag} needs cloud_frame='world': {reason}")
        if any(int(v) < lo or (hi is not None and int(v) > hi) for _, v, lo, hi in ints):
            need = [f"{name} >= {lo}" if hi is None else f"{name} in {lo}..{hi}" for name, _, lo, hi in ints]
            raise ValueError(f"need {', '.join(need[:-1])} and {need[-1]}, got {', '.join(str(v) for _, v, _, _ in ints)}")
    return (voxel, *(int(v) for _, v, _, _ in ints))


class PredictionWriter:
    """Writes ``<out_dir>/<name>_depth.png`` (16-bit greyscale, ``fmt``) and, with ``panels``, ``<name>_panels.png`` (RGB) for
    every sample handed to ``submit``.  A ring of ``slots`` device + pinned host buffer pairs; ``submit`` launches the export
    kernel and the device-to-host copies on the current stream, records an event and queues the files to ``threads`` worker
    threads, which wait for the event, compress and free the slot.  ``submit`` blocks only while every slot is in flight.
    ``close()`` (or leaving the ``with`` block) drains the ring and re-raises the first exception a worker hit.
    ``encode=False`` does everything but the file encoding (for measuring the loop without the PNG encoder).  All submits
    must come from one stream and have one geometry.

    ``cloud=True`` also writes ``<name>_cloud.ply``: every ``cloud_step``-th pixel of every ``cloud_step``-th row whose
    estimate is finite and within [near, far], as float x, y, z + uchar red, green, blue, alpha, in the frame of the
    trajectory's first camera (``cloud_frame="world"``) or of the frame's own camera (``"camera"``); the frame's
    camera-to-world pose is in the header either way (``read_cloud_ply``).  Each slot then also owns a [b,cap,16] byte vertex
    buffer with its pinned twin, the counts and a pinned copy of the poses; the whole ``cap`` region crosses PCIe every step
    (the count is only known on the device), the worker writes the first ``counts[s]`` vertices.

    ``cloud_views=K`` (1..8; needs ``cloud``) filters the clouds: a pixel gives a vertex only if at least ``cloud_min_views``
    (default min(2, K)) of the up to K earlier frames of its trajectory confirm it within ``cloud_tol`` = (pixels, relative
    depth) -- ``network_ops.depth_views``, one more launch per submit, at full resolution whatever ``cloud_step`` is.  The
    writer then owns the ring of the last K + 1 estimates and poses, (K+1) b h w floats.  The rule is strict: the first
    ``cloud_min_views`` frames of every trajectory give clouds without vertices.  ``save_conf=True`` also writes
    ``<name>_conf.png``: 8-bit grey, ``confirming views * 255 // K`` (``read_conf_png``).  ``cloud_kept`` / ``cloud_cap`` sum the
    vertices written and the vertices a cloud could hold at most, over the frames the workers have finished.

    ``save_map=VOXEL`` (metres; with or without ``cloud``) also writes ``<directory of the trajectory's frames>/map.ply``: the
    vertices of the trajectory's clouds merged into one vertex per occupied voxel (include/m4depth_hip.h, ``write_map_ply``).
    After ``depth_cloud`` of every submit ``network_ops.voxel_map_integrate`` adds the step's compacted vertices -- made with
    ``cloud_step``, [near, far] and the ``cloud_views`` filter, as they lie in the slot's device buffer -- to the sample's hash
    table of 2^``map_slots_log2`` slots (168 MB per sample at the default 21), stamped with the writer's step counter.  A
    sample whose host-side ``reset`` flag is set has its map extracted (voxels at least ``map_min_frames`` frames saw), handed
    to a worker thread and cleared before the new frame goes in, and ``close()`` does that for every open trajectory: the loop
    waits for the device once per finished trajectory, never per frame.  The map needs the world frame, host-side reset flags
    (a device mask raises ValueError) and names with one directory per trajectory (``FrameNamer``'s).  Without ``cloud`` the
    cloud launches still run, their buffers stay on the device and no ``_cloud.ply`` is written.  ``maps``, ``map_voxels``,
    ``map_dropped_range`` and ``map_dropped_full`` sum over the maps handed to the workers: a ``map_dropped_full`` > 0 says
    that ``map_slots_log2`` is too small for the scene.

    ``save_mesh=VOXEL`` (metres; independent of ``cloud`` and ``save_map``) also writes ``<directory of the trajectory's
    frames>/mesh.ply``: the trajectory's estimates fused into a truncated signed distance field on a hashed voxel grid and
    extracted as a triangle mesh by naive surface nets (include/m4depth_hip.h, ``write_mesh_ply``).  Every submit runs
    ``network_ops.tsdf_integrate`` -- two launches -- on what the clouds see: the ``cloud_views``-filtered copy of the estimate
    when that option is on, limited to [near, far], at EVERY pixel (``cloud_step`` does not apply: a stride wider than a voxel
    would leave holes).  ``mesh_trunc`` is the truncation distance in voxels (2..8), a voxel takes part in the extraction only if
    at least ``mesh_min_frames`` frames updated it, and each sample owns a table of 2^``mesh_slots_log2`` slots of 32 bytes (134 MB
    at the default 22).  Trajectories end, and their tables are cleared, exactly where the maps' do, under the same needs (world
    frame, host-side reset flags, one directory per trajectory).  With ``save_mesh`` alone the pose chain, the views check and
    the two mesh launches run; ``depth_cloud`` does not.  ``meshes``, ``mesh_vertices``, ``mesh_triangles``,
    ``mesh_dropped_range``, ``mesh_dropped_full`` and ``mesh_quads_dropped`` sum over the meshes handed to the workers.

    ``save_fused=True`` (needs ``save_mesh``) also writes ``<name>_fused.png``: the mesh's volume, right after the frame went
    into it, rendered into the frame's camera by ``network_ops.tsdf_raycast`` over [near, far] (``fused_window=W``: only W
    truncation distances around the raw estimate) and encoded like the estimate (``fmt``); a pixel without a surface is what the
    format makes of a non-finite estimate (0 in kitti16, 0x7C00 in midair16).  One more launch pair and one more 16-bit image
    across PCIe per submit.  Under ``cloud_views`` the volume holds the filtered estimates, so the rendered map fills pixels the
    filter dropped wherever earlier frames put a surface.  ``fused_pixels`` / ``fused_cap`` sum the pixels rendered and the
    pixels there are, over the frames the workers have finished."""

    def __init__(self, out_dir, fmt, panels=(), near=1.0, far=80.0, err_max=0.5, slots=4, threads=8, compress_level=1,
                 encode=True, cloud=False, cloud_step=2, cloud_frame="world", cloud_views=0, cloud_min_views=None,
                 cloud_tol=(1.0, 0.01), save_conf=False, save_map=None, map_min_frames=2, map_slots_log2=21, save_mesh=None,
                 mesh_trunc=4, mesh_min_frames=2, mesh_slots_log2=22, save_fused=False, fused_window=None):
        if fmt not in FORMATS:
            raise ValueError(f"fmt: expected one of {FORMATS}, got {fmt!r}")
        panels = tuple(panels)
        if len(panels) > 4 or any(p not in PANELS for p in panels):
            raise ValueError(f"panels: up to four of {PANELS}, got {panels}")
        if not (near > 0 and far > near and err_max > 0):
            raise ValueError(f"need 0 < near < far and err_max > 0, got near {near}, far {far}, err_max {err_max}")
        if slots < 1 or threads < 1:
            raise ValueError("slots and threads must be >= 1")
        if int(cloud_step) < 1 or cloud_frame not in CLOUD_FRAMES:
            raise ValueError(f"cloud_step must be >= 1 and cloud_frame one of {CLOUD_FRAMES}, got {cloud_step}, {cloud_frame!r}")
        cloud_views = int(cloud_views)
        if not 0 <= cloud_views <= nops.VIEWS_MAX:
            raise ValueError(f"cloud_views must be 0 (off) or 1..{nops.VIEWS_MAX}, got {cloud_views}")
        save_map, map_min_frames, map_slots_log2 = _trajectory_options(
            "save_map", save_map, cloud_frame, "a map merges the frames of a trajectory in one frame",
            (("map_min_frames", map_min_frames, 2, 1, None), ("map_slots_log2", map_slots_log2, 21, 6, 26)))
        save_mesh, mesh_trunc, mesh_min_frames, mesh_slots_log2 = _trajectory_options(
            "save_mesh", save_mesh, cloud_frame, "a mesh fuses the frames of a trajectory in one frame",
            (("mesh_trunc", mesh_trunc, 4, *nops.TSDF_TRUNC), ("mesh_min_frames", mesh_min_frames, 2, 1, None),
             ("mesh_slots_log2", mesh_slots_log2, 22, 6, 26)))
        if save_fused and save_mesh is None:
            raise ValueError("save_fused needs save_mesh: it renders the mesh's volume")
        if fused_window is not None and (not save_fused or int(fused_window) < 1):
            raise ValueError(f"fused_window needs save_fused and a width >= 1 truncation distances, got {fused_window}")
        self.save_fused, self.fused_window = bool(save_fused), None if fused_window is None else int(fused_window)
        self.fused_pixels = self.fused_cap = 0             # pixels rendered / pixels there are, finished frames
        if cloud_views and not (cloud or save_map is not None or save_mesh is not None):
            raise ValueError("cloud_views needs cloud=True: the check runs on the clouds' pose chain (save_map or save_mesh "
                             "run on it as well)")
        if save_conf and not cloud_views:
            raise ValueError("save_conf needs cloud_views >= 1")
        if cloud_min_views is not None and not cloud_views:
            raise ValueError("cloud_min_views needs cloud_views >= 1")
        cloud_min_views = min(2, cloud_views) if cloud_min_views is None else int(cloud_min_views)
        if cloud_views and not 1 <= cloud_min_views <= cloud_views:
            raise ValueError(f"cloud_min_views must be in 1..{cloud_views}, got {cloud_min_views}")
        cloud_tol = tuple(float(v) for v in cloud_tol)
        if len(cloud_tol) != 2 or not (cloud_tol[0] > 0 and cloud_tol[1] > 0):
            raise ValueError(f"cloud_tol: expected (pixels > 0, relative depth > 0), got {cloud_tol}")
        self.cloud, self.cloud_step, self.cloud_frame = bool(cloud), int(cloud_step), cloud_frame
        self.cloud_views, self.cloud_min_views, self.cloud_tol, self.save_conf = cloud_views, cloud_min_views, cloud_tol, bool(save_conf)
        self._views = None                                 # depth_views' ring and ages, next to the pose chain
        self._views_n = self._views_depth = None           # [b,h,w] counts (without save_conf) and the filtered copy
        self.cloud_kept = self.cloud_cap = 0               # vertices written / vertices the clouds could hold, finished frames
        self._pose = None                                  # [b,7] float64 device state of the cloud: camera-to-world poses
        self.save_map, self.map_min_frames, self.map_slots_log2 = save_map, map_min_frames, map_slots_log2
        self.save_mesh, self.mesh_trunc = save_mesh, mesh_trunc
        self.mesh_min_frames, self.mesh_slots_log2 = mesh_min_frames, mesh_slots_log2
        self._vertices3d = self.cloud or save_map is not None      # the cloud launches run
        self._geometry3d = self._vertices3d or save_mesh is not None   # the pose chain (and the views check) runs
        self._map = self._mesh = None                      # the trajectory products that are on
        if save_map is not None:
            self._map = _TrajectoryProduct("map.ply", lambda b, dev: nops.voxel_map_state(b, map_slots_log2, dev),
                                           self._extract_map, nops.voxel_map_clear, self._write_map)
        if save_mesh is not None:
            self._mesh = _TrajectoryProduct("mesh.ply", lambda b, dev: nops.tsdf_state(b, mesh_slots_log2, dev),
                                            self._extract_mesh, nops.tsdf_clear, self._write_mesh)
        self._products = [p for p in (self._map, self._mesh) if p is not None]     # in the order they finish and clear
        self.maps = self.map_voxels = self.map_dropped_range = self.map_dropped_full = 0
        self.meshes = self.mesh_vertices = self.mesh_triangles = 0
        self.mesh_dropped_range = self.mesh_dropped_full = self.mesh_quads_dropped = 0
        self._step = 0                                     # submits so far: the stamp of a step's vertices
        self.out_dir, self.fmt, self.panels = str(out_dir), fmt, panels
        self.near, self.far, self.err_max = float(near), float(far), float(err_max)
        self.n_slots, self.compress_level, self.encode = int(slots), int(compress_level), bool(encode)
        self.frames = 0                                    # samples submitted so far
        self._pool = ThreadPoolExecutor(max_workers=int(threads), thread_name_prefix="m4d-export")
        self._free = queue.Queue()
        self._slots = None                                 # allocated at the first submit (the geometry is the frame's)
        self._geometry = None
        self._lut = None
        self._lock = threading.Lock()
        self._error = None
        self._closed = False

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:                                              # the body's exception wins; still leave nothing in flight
            try:
                self.close()
            except Exception:
                pass
        return False

    def _allocate(self, est):
        b, h, w = est.shape[:3]
        self._geometry = (b, h, w)
        cap = nops.cloud_capacity(h, w, self.cloud_step) if self._vertices3d else 0
        self._slots = [_Slot(b, h, w, len(self.panels), est.device, cap, self.save_conf, self.cloud, self._geometry3d,
                             self.save_fused)
                       for _ in range(self.n_slots)]
        for product in self._products[::-1]:
            product.state = product.new_state(b, est.device)
        if any(p != "rgb" for p in self.panels):
            self._lut = torch.from_numpy(default_lut()).to(est.device)
        for i in range(self.n_slots):
            self._free.put(i)

    def _extract_map(self, state, s):
        keys, vertices, stats = nops.voxel_map_extract(state, s, self.map_min_frames, self.save_map)   # the one wait
        return (vertices,), stats, {"maps": 1, "map_voxels": len(keys), "map_dropped_range": stats["dropped_range"],
                                    "map_dropped_full": stats["dropped_full"]}

    def _write_map(self, path, vertices, stats):
        write_map_ply(path, vertices, self.save_map, self.map_min_frames, stats)

    def _extract_mesh(self, state, s):
        keys, vertices, triangles, stats = nops.tsdf_extract(state, s, self.mesh_min_frames, self.save_mesh)
        return (vertices, triangles), stats, {"meshes": 1, "mesh_vertices": len(keys), "mesh_triangles": len(triangles),
                                              "mesh_dropped_range": stats["dropped_range"],
                                              "mesh_dropped_full": stats["dropped_full"],
                                              "mesh_quads_dropped": stats["quads_dropped"]}

    def _write_mesh(self, path, vertices, triangles, stats):
        write_mesh_ply(path, vertices, triangles, self.save_mesh, self.mesh_trunc, self.mesh_min_frames, stats)

    def _finish(self, product, s):
        """``product`` of sample ``s``'s open trajectory to a worker thread; the caller clears the state on the same stream."""
        arrays, stats, counters = product.extract(product.state, s)
        hosts = [torch.empty(a.shape, dtype=a.dtype) for a in arrays]
        for i, a in enumerate(arrays):
            if len(a):                                     # (an empty map or mesh is written too: nothing survived)
                hosts[i] = hosts[i].pin_memory()
                hosts[i].copy_(a, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        for name, n in counters.items():
            setattr(self, name, getattr(self, name) + n)
        self._pool.submit(self._work_product, product, os.path.join(product.dirs[s], product.file_name), hosts, event, stats)

    def _keep_error(self, e):
        with self._lock:
            if self._error is None:
                self._error = e

    def _work_product(self, product, rel_path, hosts, event, stats):
        try:
            event.synchronize()
            if self.encode:
                path = os.path.join(self.out_dir, rel_path)
                os.makedirs(os.path.dirname(path), exist_ok=True)
                product.write(path, *(h.numpy() for h in hosts), stats)
        except BaseException as e:
            self._keep_error(e)

    def _submit_cloud(self, slot, est, rgb, rot, trans, camera, reset, names):
        """The cloud of one step into ``slot``, on the current stream: pose update, compaction, copies; with ``save_map`` the
        maps of the trajectories that ended, then the step's vertices into the maps."""
        if rgb is None or rot is None or trans is None or camera is None:
            raise ValueError("a writer with cloud=True or save_map needs rgb, rot, trans and camera at every submit")
        if self.save_map is not None or self.save_mesh is not None:
            what = "save_map" if self.save_map is not None else "save_mesh"
            if torch.is_tensor(reset) and reset.is_cuda:
                raise ValueError(f"{what} needs host-side reset flags: which trajectory ended is decided on the host")
            dirs = [os.path.dirname(n) for n in names]
            if len(set(dirs)) != len(dirs):
                raise ValueError(f"{what} needs names with one directory per sample and trajectory, got {list(names)}")
        first = self._pose is None
        if first:
            self._pose = torch.empty((est.shape[0], 7), dtype=torch.float64, device=est.device)
        # the first submit resets everybody (force_all), so its flags change nothing: host flags are checked and then not even
        # uploaded, a device mask costs nothing to pass on and so still gets pose_accumulate's dtype and shape check
        mask = None
        if reset is not None:                              # checked at every submit, used from the second on
            on_device = torch.is_tensor(reset) and reset.is_cuda
            if not on_device:                              # host flags (the frame's new_traj)
                reset = np.asarray(reset.numpy() if torch.is_tensor(reset) else reset, dtype=bool).reshape(-1)
            n = reset.numel() if on_device else len(reset)
            if n != slot.reset_h.shape[0]:
                raise ValueError(f"reset has {n} samples, the writer {slot.reset_h.shape[0]}")
            if on_device:
                mask = reset                               # dtype and shape: pose_accumulate's check
            elif not first:                                # through the slot's pinned bytes
                slot.reset_h.numpy()[:] = reset
                slot.reset_d.copy_(slot.reset_h, non_blocking=True)
                mask = slot.reset_d
                for product in self._products if reset.any() else ():
                    for s in np.nonzero(reset)[0]:         # the trajectories that ended with the previous frame
                        self._finish(product, int(s))
                    product.clear(product.state, mask)
        nops.pose_accumulate(rot, trans, self._pose, reset=mask, force_all=first)
        raw = est
        if self.cloud_views:                               # the clouds see the filtered copy; PNG and panels the estimate
            b, h, w = est.shape[:3]
            if self._views is None:
                self._views = nops.depth_views_state(b, h, w, self.cloud_views, est.device)
                self._views_depth = torch.empty((b, h, w, 1), dtype=torch.float32, device=est.device)
                if not self.save_conf:
                    self._views_n = torch.empty((b, h, w), dtype=torch.uint8, device=est.device)
            # est may be a buffer the next graph replay overwrites: the ring copy happens in this launch, on this stream
            _, est = nops.depth_views(est, camera["f"], camera["c"], self._pose, self._views, reset=mask, force_all=first,
                                      tol_px=self.cloud_tol[0], tol_rel=self.cloud_tol[1], min_views=self.cloud_min_views,
                                      n_views=slot.conf_d if self.save_conf else self._views_n, depth_f=self._views_depth)
            if self.save_conf:
                slot.conf_h.copy_(slot.conf_d, non_blocking=True)
        if self.save_mesh is not None:                     # the mesh sees what the clouds see, at every pixel
            nops.tsdf_integrate(est, rgb, camera["f"], camera["c"], self._pose, self.save_mesh, self.mesh_trunc,
                                self._mesh.state, near=self.near, far=self.far)
            self._mesh.dirs = dirs
        if self.save_fused:                                # the volume as it is now, seen from this frame
            slot.hits_d.zero_()
            nops.tsdf_raycast(self._mesh.state, camera["f"], camera["c"], self._pose, est.shape[1], est.shape[2], self.save_mesh,
                              self.mesh_trunc, self.mesh_min_frames, near=self.near, far=self.far,
                              guide=raw if self.fused_window else None, window=self.fused_window, out=slot.fused_f,
                              hits=slot.hits_d)
            nops.depth_export(slot.fused_f, self.fmt, depth16=slot.fused_d)
            slot.fused_h.copy_(slot.fused_d, non_blocking=True)
            slot.hits_h.copy_(slot.hits_d, non_blocking=True)
        if not self._vertices3d:
            return
        nops.depth_cloud(est, rgb, camera["f"], camera["c"], step=self.cloud_step, near=self.near, far=self.far,
                         pose=self._pose if self.cloud_frame == "world" else None, vertices=slot.cloud_d, counts=slot.counts_d)
        if self.save_map is not None:
            nops.voxel_map_integrate(slot.cloud_d, slot.counts_d, self.save_map, self._step, self._map.state)
            self._map.dirs = dirs
        if self.cloud:
            slot.cloud_h.copy_(slot.cloud_d, non_blocking=True)
            slot.counts_h.copy_(slot.counts_d, non_blocking=True)
            slot.pose_h.copy_(self._pose, non_blocking=True)

    def submit(self, est, names, gt=None, rgb=None, rot=None, trans=None, camera=None, reset=None):
        """``est`` [b,h,w,1] (+ ``gt`` / ``rgb`` as the panels need) of one step; ``names``: b relative paths without suffix.
        With ``cloud``: ``rgb``, the frame's motion ``rot`` [b,4] / ``trans`` [b,3], ``camera`` {f, c} [b,2] and ``reset`` --
        which samples start a trajectory with this frame (host flags or a uint8 [b] device mask, None = nobody); the first
        submit resets every sample."""
        if self._closed:
            raise RuntimeError("PredictionWriter.submit after close()")
        if self._slots is None:
            self._allocate(est)
        if tuple(est.shape[:3]) != self._geometry or len(names) != self._geometry[0]:
            raise ValueError(f"submit: est {tuple(est.shape)} with {len(names)} names, the writer was sized for {self._geometry}")
        index = self._free.get()                           # back-pressure: waits while every slot is in flight
        slot = self._slots[index]
        try:
            nops.depth_export(est, self.fmt, self.panels, gt=gt, rgb=rgb, lut=self._lut, near=self.near, far=self.far,
                              err_max=self.err_max, depth16=slot.depth_d, panels_out=slot.panels_d)
            slot.depth_h.copy_(slot.depth_d, non_blocking=True)
            if slot.panels_d is not None:
                slot.panels_h.copy_(slot.panels_d, non_blocking=True)
            self._step += 1
            if self._geometry3d:
                self._submit_cloud(slot, est, rgb, rot, trans, camera, reset, names)
            slot.event.record()
        except BaseException:
            self._free.put(index)
            raise
        jobs = []
        for s, name in enumerate(names):
            jobs.append((name + "_depth.png", slot.depth_h, s))
            if slot.panels_h is not None:
                jobs.append((name + "_panels.png", slot.panels_h, s))
            if self.cloud:
                jobs.append((name + "_cloud.ply", None, s))
            if self.save_conf:
                jobs.append((name + "_conf.png", slot.conf_h, s))
            if self.save_fused:
                jobs.append((name + "_fused.png", slot.fused_h, s))
        slot.pending = len(jobs)
        self.frames += len(names)
        for job in jobs:
            self._pool.submit(self._work, index, *job)

    def _work(self, index, rel_path, host, s):
        slot = self._slots[index]
        try:
            slot.event.synchronize()
            if host is None and self.cloud_views:          # counts the host already has: the share the filter kept
                with self._lock:
                    self.cloud_kept += int(slot.counts_h[s])
                    self.cloud_cap += slot.cloud_h.shape[1]
            if host is not None and host is slot.fused_h:  # counts the host already has: the share rendered
                with self._lock:
                    self.fused_pixels += int(slot.hits_h[s])
                    self.fused_cap += host.shape[1] * host.shape[2]
            if self.encode:
                path = os.path.join(self.out_dir, rel_path)
                os.makedirs(os.path.dirname(path), exist_ok=True)
                if host is None:                           # the cloud: the count is read here, after the event
                    write_cloud_ply(path, slot.cloud_h[s, :int(slot.counts_h[s])].numpy(), slot.pose_h[s].numpy())
                else:
                    from PIL import Image
                    arr = host[s].numpy()
                    if arr.dtype == np.int16:
                        arr = arr.view(np.uint16)          # PIL mode I;16
                    elif host is slot.conf_h:              # counts -> grey
                        arr = (arr.astype(np.uint16) * 255 // self.cloud_views).astype(np.uint8)
                    Image.fromarray(arr).save(path, format="PNG", compress_level=self.compress_level)
        except BaseException as e:                         # kept for close(); the slot is freed all the same
            self._keep_error(e)
        finally:
            with self._lock:
                slot.pending -= 1
                done = slot.pending == 0
            if done:
                self._free.put(index)

    def close(self):
        """Waits for every slot, stops the workers and re-raises the first worker exception."""
        if self._closed:
            return
        self._closed = True
        try:
            for product in self._products:                 # the open trajectories end here
                if product.dirs is not None:
                    for s in range(len(product.dirs)):
                        self._finish(product, s)
                    product.dirs = None
        except BaseException as e:
            self._keep_error(e)
        if self._slots is not None:
            for _ in range(self.n_slots):
                self._free.get()
        self._pool.shutdown(wait=True)
        if self._error is not None:
            raise self._error
