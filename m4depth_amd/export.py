"""Prediction export -- the back end of ``main.py --mode=predict --save_dir``, the mirror of the dataloaders' front end.

The reference's predict loop hands ``d_est``, ``d_gt`` and ``i_rgb`` of every frame to the user (main.py:150-172); what users
do with them is save a depth map and a colourised estimate beside the ground truth and the image.  Here one kernel per frame
batch (``network_ops.depth_export``) writes the estimate in a dataset's own 16-bit encoding and as ready-to-save RGB8 panels,
``PredictionWriter`` moves them through a ring of pinned buffers, and host threads do the PNG compression: the predict loop
never waits for the host unless every slot of the ring is in flight, and host memory is ``slots`` frames however long the run.

The 3-D outputs -- a point cloud per frame, one voxel map and one TSDF mesh per trajectory, the mesh's volume rendered into every
frame -- come from one ``fusion.TrajectoryChain``, which owns their device state and issues every launch on it; the writer
copies what it made through the same ring and hands what a finished trajectory leaves to the same threads.  The host never
redoes the camera model or the pose chain, and never reads a vertex count before the slot's event has passed.
"""
from __future__ import annotations

import os
import queue
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import network_ops as nops
from .fusion import TrajectoryChain

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
    """What one submit of ``writer`` copies to the host: the device buffers its launches fill and their pinned twins."""

    def __init__(self, writer, b, h, w, dev):
        def pair(shape, dtype):
            return torch.empty(shape, dtype=dtype, device=dev), torch.empty(shape, dtype=dtype).pin_memory()

        self.depth_d, self.depth_h = pair((b, h, w), torch.int16)
        self.panels_d = self.panels_h = self.cloud_d = self.conf_d = self.conf_h = self.fused_h = None
        self.view_d = self.view_h = None
        if writer.panels:
            self.panels_d, self.panels_h = pair((b, len(writer.panels) * h, w, 3), torch.uint8)
        if writer.cloud:
            self.cloud_d, self.cloud_h = pair((b, nops.cloud_capacity(h, w, writer.cloud_step), 16), torch.uint8)
            self.counts_d, self.counts_h = pair(b, torch.int32)
            self.pose_h = torch.empty((b, 7), dtype=torch.float64).pin_memory()
        elif writer.save_map is not None:                  # a writer of maps alone keeps the vertices on the device
            self.cloud_d = torch.empty((b, nops.cloud_capacity(h, w, writer.cloud_step), 16), dtype=torch.uint8, device=dev)
            self.counts_d = torch.empty(b, dtype=torch.int32, device=dev)
        if writer.needs_geometry:
            self.reset_d, self.reset_h = pair(b, torch.uint8)
        if writer.save_conf:
            self.conf_d, self.conf_h = pair((b, h, w), torch.uint8)
        if writer.save_fused:                              # the rendered volume: float32, its 16-bit form and the pixels rendered
            self.fused_f = torch.empty((b, h, w, 1), dtype=torch.float32, device=dev)
            self.fused_d, self.fused_h = pair((b, h, w), torch.int16)
            self.hits_d, self.hits_h = pair(b, torch.int64)
        if writer.save_fused_view:                         # the same launch's RGB8 picture
            self.view_d, self.view_h = pair((b, h, w, 3), torch.uint8)
        self.event = torch.cuda.Event()
        self.pending = 0


# what the chain's options are called here, for its ValueError texts
_CHAIN_NAMES = {"views": "cloud_views", "min_views": "cloud_min_views", "tol": "cloud_tol", "map_voxel": "save_map", "voxel": "save_mesh",
                "trunc": "mesh_trunc", "min_frames": "mesh_min_frames", "slots_log2": "mesh_slots_log2", "window": "fused_window",
                "interp": "fused_interp"}


class PredictionWriter:
    """Writes ``<out_dir>/<name>_depth.png`` (16-bit greyscale, ``fmt``) and, with ``panels``, ``<name>_panels.png`` (RGB) for
    every sample handed to ``submit``.  A ring of ``slots`` device + pinned host buffer pairs; ``submit`` launches the export
    kernel and the device-to-host copies on the current stream, records an event and queues the files to ``threads`` worker
    threads, which wait for the event, compress and free the slot.  ``submit`` blocks only while every slot is in flight.
    ``close()`` (or leaving the ``with`` block) drains the ring and re-raises the first exception a worker hit.
    ``encode=False`` does everything but the file encoding (for measuring the loop without the PNG encoder).  All submits
    must come from one stream and have one geometry.

    Everything else comes from ``chain``, a ``fusion.TrajectoryChain`` over [near, far] whose docstring has the options
    (``cloud_views`` / ``cloud_min_views`` / ``cloud_tol``: its views check; ``save_mesh`` / ``mesh_*`` / ``fused_window``: its
    volume; ``save_map`` / ``map_*``: its map); ``submit`` then needs the frame's motion (``needs_geometry``).  PNG and panels
    show the raw estimate; clouds, maps and meshes see the filtered one where the views check is on.

    ``cloud=True``: ``<name>_cloud.ply`` (``read_cloud_ply``), every ``cloud_step``-th pixel of every ``cloud_step``-th row in the
    frame of the trajectory's first camera (``cloud_frame="world"``) or of the frame's own (``"camera"``).  A cloud's whole
    capacity crosses PCIe every step (the count is only known on the device); the worker writes the first ``counts[s]``
    vertices.  ``save_conf=True`` (needs ``cloud_views=K``): ``<name>_conf.png``, 8-bit grey, ``confirming views * 255 // K``.
    ``save_fused=True`` (needs ``save_mesh``): ``<name>_fused.png``, the volume right after the frame went in, rendered into the
    frame's camera and encoded like the estimate; ``fused_interp``: "nearest" or "trilinear", how that rendering samples the
    field; ``save_fused_view=True`` (needs ``save_fused``): ``<name>_fused_view.png``, RGB8, the rendered surface's colour under a
    headlight (``network_ops.tsdf_render``'s ``view``).  ``cloud_kept`` / ``cloud_cap`` and ``fused_pixels`` / ``fused_cap``: vertices
    written / a cloud's capacity and pixels rendered / pixels there are, over the frames the workers have finished.

    ``save_map=VOXEL`` / ``save_mesh=VOXEL``: ``map.ply`` / ``mesh.ply`` in the directory of a trajectory's frames, from the step's
    cloud vertices (kept on the device without ``cloud``) and from the estimate at EVERY pixel.  A sample whose host-side
    ``reset`` flag is set has them extracted, handed to a worker thread and cleared before the new frame goes in; ``close()``
    does that for every open trajectory: the loop waits for the device once per finished trajectory, never per frame.  Both
    need the world frame, host-side reset flags and names with one directory per trajectory (``FrameNamer``'s).  ``maps`` /
    ``map_*`` and ``meshes`` / ``mesh_*`` sum over what went to the workers: a ``*_dropped_full`` > 0 asks for more slots."""

    def __init__(self, out_dir, fmt, panels=(), near=1.0, far=80.0, err_max=0.5, slots=4, threads=8, compress_level=1,
                 encode=True, cloud=False, cloud_step=2, cloud_frame="world", cloud_views=0, cloud_min_views=None,
                 cloud_tol=(1.0, 0.01), save_conf=False, save_map=None, map_min_frames=None, map_slots_log2=None, save_mesh=None,
                 mesh_trunc=None, mesh_min_frames=None, mesh_slots_log2=None, save_fused=False, fused_window=None, fused_interp=None,
                 save_fused_view=False):
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
        if save_fused and save_mesh is None:
            raise ValueError("save_fused needs save_mesh: it renders the mesh's volume")
        if fused_window is not None and (not save_fused or int(fused_window) < 1):
            raise ValueError(f"fused_window needs save_fused and a width >= 1 truncation distances, got {fused_window}")
        if fused_interp is not None and not save_fused:
            raise ValueError(f"fused_interp needs save_fused, got {fused_interp!r}")
        if save_fused_view and not save_fused:
            raise ValueError("save_fused_view needs save_fused: it is the same rendering's picture")
        self.chain = chain = TrajectoryChain(
            save_mesh, mesh_trunc, mesh_min_frames, mesh_slots_log2, near, far, window=fused_window, views=cloud_views,
            min_views=cloud_min_views, tol=cloud_tol, map_voxel=save_map, map_min_frames=map_min_frames,
            map_slots_log2=map_slots_log2, names=_CHAIN_NAMES, interp="nearest" if fused_interp is None else fused_interp)
        for flag, voxel, verb in (("save_map", chain.map_voxel, "map merges"), ("save_mesh", chain.voxel, "mesh fuses")):
            if voxel is not None and cloud_frame != "world":
                raise ValueError(f"{flag} needs cloud_frame='world': a {verb} the frames of a trajectory in one frame")
        if chain.views and not (cloud or chain.map_voxel is not None or chain.voxel is not None):
            raise ValueError("cloud_views needs cloud=True: the check runs on the clouds' pose chain (save_map or save_mesh "
                             "run on it as well)")
        if save_conf and not chain.views:
            raise ValueError("save_conf needs cloud_views >= 1")
        self.cloud, self.cloud_step, self.cloud_frame, self.save_conf = bool(cloud), int(cloud_step), cloud_frame, bool(save_conf)
        self.cloud_views, self.cloud_min_views, self.cloud_tol = chain.views, chain.min_views, chain.tol
        self.save_map, self.map_min_frames, self.map_slots_log2 = chain.map_voxel, chain.map_min_frames, chain.map_slots_log2
        self.save_mesh, self.mesh_trunc, self.mesh_min_frames = chain.voxel, chain.trunc, chain.min_frames
        self.mesh_slots_log2 = chain.slots_log2
        self.save_fused, self.fused_window = bool(save_fused), chain.window
        self.fused_interp, self.save_fused_view = chain.interp, bool(save_fused_view)
        self.fused_pixels = self.fused_cap = self.cloud_kept = self.cloud_cap = 0          # over the finished frames
        self._per_trajectory = self.save_map is not None or self.save_mesh is not None     # map.ply / mesh.ply are written
        self._dirs = None                                  # the directory of every sample's open trajectory, once a step went in
        self.maps = self.map_voxels = self.map_dropped_range = self.map_dropped_full = 0
        self.meshes = self.mesh_vertices = self.mesh_triangles = 0
        self.mesh_dropped_range = self.mesh_dropped_full = self.mesh_quads_dropped = 0
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

    needs_geometry = property(lambda self: self.cloud or self._per_trajectory,
                              doc="Whether the chain runs: ``submit`` then needs ``rgb``, ``rot``, ``trans``, ``camera`` and ``reset``.")

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
        self._slots = [_Slot(self, b, h, w, est.device) for _ in range(self.n_slots)]
        if any(p != "rgb" for p in self.panels):
            self._lut = torch.from_numpy(default_lut()).to(est.device)
        for i in range(self.n_slots):
            self._free.put(i)

    def _finish(self, s):
        """The map and the mesh of sample ``s``'s open trajectory to worker threads (one wait each); the caller clears the
        state on the same stream."""
        if self.save_map is not None:
            keys, vertices, stats = self.chain.extract_map(s)
            self.maps += 1
            self.map_voxels += len(keys)
            self.map_dropped_range += stats["dropped_range"]
            self.map_dropped_full += stats["dropped_full"]
            self._hand_over(s, "map.ply", write_map_ply, (vertices,), (self.save_map, self.map_min_frames, stats))
        if self.save_mesh is not None:
            keys, vertices, triangles, stats = self.chain.extract_volume(s)
            self.meshes += 1
            self.mesh_vertices += len(keys)
            self.mesh_triangles += len(triangles)
            self.mesh_dropped_range += stats["dropped_range"]
            self.mesh_dropped_full += stats["dropped_full"]
            self.mesh_quads_dropped += stats["quads_dropped"]
            self._hand_over(s, "mesh.ply", write_mesh_ply, (vertices, triangles),
                            (self.save_mesh, self.mesh_trunc, self.mesh_min_frames, stats))

    def _hand_over(self, s, file_name, write, arrays, rest):
        """``write(path, *arrays on the host, *rest)`` in a worker thread, once the copies of ``arrays`` have passed."""
        hosts = [torch.empty(a.shape, dtype=a.dtype) for a in arrays]
        for i, a in enumerate(arrays):
            if len(a):                                     # (an empty map or mesh is written too: nothing survived)
                hosts[i] = hosts[i].pin_memory()
                hosts[i].copy_(a, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        self._pool.submit(self._work_product, os.path.join(self._dirs[s], file_name), write, hosts, event, rest)

    def _keep_error(self, e):
        with self._lock:
            if self._error is None:
                self._error = e

    def _work_product(self, rel_path, write, hosts, event, rest):
        try:
            event.synchronize()
            if self.encode:
                path = os.path.join(self.out_dir, rel_path)
                os.makedirs(os.path.dirname(path), exist_ok=True)
                write(path, *(h.numpy() for h in hosts), *rest)
        except BaseException as e:
            self._keep_error(e)

    def _mask(self, slot, reset, first):
        """``reset`` of a submit as (the step's device mask or None, the samples whose trajectory ended with the previous frame).
        The first step resets everybody, so its flags change nothing: host flags are checked and then not even uploaded; a
        device mask costs nothing to pass on and so still gets ``pose_accumulate``'s dtype and shape check."""
        if reset is None:
            return None, ()
        on_device = torch.is_tensor(reset) and reset.is_cuda
        if not on_device:                                  # host flags (the frame's new_traj)
            reset = np.asarray(reset.numpy() if torch.is_tensor(reset) else reset, dtype=bool).reshape(-1)
        n = reset.numel() if on_device else len(reset)
        if n != slot.reset_h.shape[0]:
            raise ValueError(f"reset has {n} samples, the writer {slot.reset_h.shape[0]}")
        if on_device or first:
            return (reset if on_device else None), ()
        slot.reset_h.numpy()[:] = reset                    # through the slot's pinned bytes
        slot.reset_d.copy_(slot.reset_h, non_blocking=True)
        return slot.reset_d, np.nonzero(reset)[0].tolist()

    def _submit_cloud(self, slot, est, rgb, rot, trans, camera, reset, names):
        """The chain's step into ``slot``, on the current stream: what ended goes to the workers, then the launches in the
        chain's order, each followed by the copies of what it made."""
        chain = self.chain
        if rgb is None or rot is None or trans is None or camera is None:
            raise ValueError("a writer with cloud=True or save_map needs rgb, rot, trans and camera at every submit")
        if self._per_trajectory:
            what = "save_map" if self.save_map is not None else "save_mesh"
            if torch.is_tensor(reset) and reset.is_cuda:
                raise ValueError(f"{what} needs host-side reset flags: which trajectory ended is decided on the host")
            dirs = [os.path.dirname(n) for n in names]
            if len(set(dirs)) != len(dirs):
                raise ValueError(f"{what} needs names with one directory per sample and trajectory, got {list(names)}")
        mask, ended = self._mask(slot, reset, first=chain.pose is None)
        for s in ended:
            self._finish(s)
        chain.advance(rot, trans, mask, clear=bool(ended))  # the clear launches only where a trajectory ended
        seen = est                                         # what clouds, maps and meshes see; PNG, panels and guide the estimate
        if chain.views:
            seen = chain.filter(est, camera, counts=slot.conf_d)
            if self.save_conf:
                slot.conf_h.copy_(slot.conf_d, non_blocking=True)
        if self.save_mesh is not None:
            chain.fuse(seen, rgb, camera)
        if self.save_fused:
            slot.hits_d.zero_()
            chain.render(est, camera, out=slot.fused_f, hits=slot.hits_d, view=slot.view_d)
            nops.depth_export(slot.fused_f, self.fmt, depth16=slot.fused_d)
            slot.fused_h.copy_(slot.fused_d, non_blocking=True)
            if slot.view_d is not None:
                slot.view_h.copy_(slot.view_d, non_blocking=True)
            slot.hits_h.copy_(slot.hits_d, non_blocking=True)
        if slot.cloud_d is not None:
            chain.compact(seen, rgb, camera, self.cloud_step, self.cloud_frame == "world", slot.cloud_d, slot.counts_d)
            if self.save_map is not None:
                chain.merge(slot.cloud_d, slot.counts_d)
            if self.cloud:
                slot.cloud_h.copy_(slot.cloud_d, non_blocking=True)
                slot.counts_h.copy_(slot.counts_d, non_blocking=True)
                slot.pose_h.copy_(chain.pose, non_blocking=True)
        if self._per_trajectory:
            self._dirs = dirs

    def submit(self, est, names, gt=None, rgb=None, rot=None, trans=None, camera=None, reset=None):
        """``est`` [b,h,w,1] (+ ``gt`` / ``rgb`` as the panels need) of one step; ``names``: b relative paths without suffix.
        With ``needs_geometry``: ``rgb``, the frame's motion ``rot`` [b,4] / ``trans`` [b,3], ``camera`` {f, c} [b,2] and
        ``reset`` -- which samples start a trajectory with this frame (host flags or a uint8 [b] device mask, None = nobody);
        the first submit resets every sample."""
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
            if self.needs_geometry:
                self._submit_cloud(slot, est, rgb, rot, trans, camera, reset, names)
            slot.event.record()
        except BaseException:
            self._free.put(index)
            raise
        files = (("_depth.png", slot.depth_h, True), ("_panels.png", slot.panels_h, bool(self.panels)), ("_cloud.ply", None, self.cloud),
                 ("_conf.png", slot.conf_h, self.save_conf), ("_fused.png", slot.fused_h, self.save_fused),
                 ("_fused_view.png", slot.view_h, self.save_fused_view))                         # suffix, pinned copy, on
        jobs = [(name + suffix, host, s) for s, name in enumerate(names) for suffix, host, on in files if on]
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
            for s in range(len(self._dirs or ())):         # the open trajectories end here
                self._finish(s)
            self._dirs = None
        except BaseException as e:
            self._keep_error(e)
        if self._slots is not None:
            for _ in range(self.n_slots):
                self._free.get()
        self._pool.shutdown(wait=True)
        if self._error is not None:
            raise self._error

    def summary(self):
        """What was written, as the fragments of the driver's closing line (complete after ``close()``)."""
        said = [self.fmt]
        if self.panels:
            said.append("panels " + ",".join(self.panels))
        if self.cloud:
            said.append(f"clouds at stride {self.cloud_step}")
        if self.cloud_views and self.cloud:
            said.append(f"{self.cloud_views}-view check kept {self.cloud_kept} of {self.cloud_cap} cloud pixels "
                        f"({100.0 * self.cloud_kept / max(self.cloud_cap, 1):.1f} %)")
        if self.save_map is not None:
            said.append(f"{self.maps} voxel maps at {self.save_map:g} m: {self.map_voxels} voxels written, "
                        f"{self.map_dropped_range} vertices dropped out of range, {self.map_dropped_full} dropped by full tables"
                        + (" (raise --map_slots_log2)" if self.map_dropped_full else ""))
        if self.save_mesh is not None:
            said.append(f"{self.meshes} meshes at {self.save_mesh:g} m: {self.mesh_vertices} vertices, "
                        f"{self.mesh_triangles} triangles, {self.mesh_dropped_range} samples dropped out of range, "
                        f"{self.mesh_dropped_full} dropped by full tables"
                        + (" (raise --mesh_slots_log2)" if self.mesh_dropped_full else ""))
        if self.save_fused:
            said.append(f"fused depth rendered on {100.0 * self.fused_pixels / max(self.fused_cap, 1):.1f} % of the pixels"
                        + ("" if self.fused_interp == "nearest" else f" ({self.fused_interp} sampling)")
                        + (", with views" if self.save_fused_view else ""))
        return said
