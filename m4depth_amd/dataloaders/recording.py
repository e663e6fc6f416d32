"""Front end for a user's own camera recording: a folder of frames, a trajectory and a calibration with lens distortion.

    REC/camera.json   width, height, fx, fy, cx, cy,
                      pixel_centre: "integer" (default: OpenCV / Kalibr, pixel centres at integer coordinates; 0.5 is added)
                                    | "half" (pixel centres at integer + 0.5, the convention of get_coords_2d),
                      model: "pinhole" | "radtan" | "equidistant",
                      distortion: [k1,k2,p1,p2,k3] (radtan) | [k1,k2,k3,k4] (equidistant), absent for pinhole,
                      T_body_cam: [qw,qx,qy,qz,tx,ty,tz] optional (camera-to-body; identity if absent),
                      depth_scale: optional, default 5000 (metres = value / depth_scale),
                      zoom: optional, default 1.0
    REC/frames.txt    "timestamp path" per line, '#' comments (TUM rgb.txt)
    REC/poses.txt     "timestamp tx ty tz qx qy qz qw" per line (TUM trajectory, body-to-world)
    REC/depth.txt     optional, "timestamp path" of 16-bit PNGs registered to the colour camera (TUM depth.txt)

The camera frame is x right, y down, z forward.  Everything about poses and timing runs here in numpy float64, once per
recording when it is opened (tens of numbers per frame); the pixels go through the library: the host uploads the decoder's
raw uint8 / uint16 frame and m4d_decode_rgb8_remap / m4d_decode_depth16_remap undistort, cast and resize it in one pass
through the recording's table (m4d_undistort_map, built on first use and kept on the device).
"""
from __future__ import annotations

import ctypes
import json
import os

import numpy as np
import torch

from .._lib import lib, dptr, stream_ptr, check
from .generic import DataLoaderGeneric

MODELS = {"pinhole": 0, "radtan": 1, "equidistant": 2}            # the `model` argument of m4d_undistort_map
DISTORTION_LENGTH = {"pinhole": 0, "radtan": 5, "equidistant": 4}
DEPTH_MAX_DT = 0.02                                               # TUM associate.py's default max_difference


# ---- quaternions (w, x, y, z), float64 ------------------------------------------------------------------------------------------
def quat_mul(a, b):
    """Hamilton product: R(a b) = R(a) R(b)."""
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], np.float64)


def quat_conj(q):
    return np.array([q[0], -q[1], -q[2], -q[3]], np.float64)


def quat_rot(q):
    """Rotation matrix of a unit quaternion (the matrix get_rot_mat writes)."""
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float64)


def slerp(q0, q1, a):
    """Unit quaternion a of the way from q0 to q1 along the short arc."""
    d = float(np.dot(q0, q1))
    if d < 0.0:
        q1, d = -q1, -d
    if d > 1.0 - 1e-12:                                           # nearly the same rotation: the chord is the arc
        q = q0 + a * (q1 - q0)
    else:
        th = np.arccos(d)
        q = (np.sin((1.0 - a) * th) * q0 + np.sin(a * th) * q1) / np.sin(th)
    return q / np.linalg.norm(q)


def compose(T_ab, T_bc):
    """[qw,qx,qy,qz,tx,ty,tz] of T_ab . T_bc (rows of T_ab may be an [N,7] array)."""
    T_ab = np.asarray(T_ab, np.float64)
    if T_ab.ndim == 2:
        return np.stack([compose(T, T_bc) for T in T_ab]) if len(T_ab) else T_ab.reshape(0, 7)
    T_bc = np.asarray(T_bc, np.float64)
    q = quat_mul(T_ab[:4], T_bc[:4])
    return np.concatenate([q / np.linalg.norm(q), quat_rot(T_ab[:4]) @ T_bc[4:] + T_ab[4:]])


# ---- the files ----------------------------------------------------------------------------------------------------------------
def _lines(path):
    """(line number, text) of the non-empty, non-comment lines of a TUM-style text file."""
    with open(path) as fh:
        for no, line in enumerate(fh, 1):
            line = line.split("#", 1)[0].strip()
            if line:
                yield no, line


def _number(text, path, no):
    try:
        v = float(text)
    except ValueError:
        raise ValueError(f"{path}:{no}: {text!r} is not a number") from None
    return v


def _read_stamped_paths(path, root):
    out, last = [], -np.inf
    for no, line in _lines(path):
        f = line.split(None, 1)                                     # the path is the rest of the line: it may hold spaces or commas
        if len(f) < 2:
            raise ValueError(f"{path}:{no}: expected 'timestamp path'")
        t = _number(f[0], path, no)
        if not np.isfinite(t) or t <= last:
            raise ValueError(f"{path}:{no}: timestamps must strictly increase ({t!r} after {last!r})")
        last = t
        out.append((t, f[1] if os.path.isabs(f[1]) else os.path.join(root, f[1])))
    return out


def _read_poses(path):
    times, poses, last = [], [], -np.inf
    for no, line in _lines(path):
        f = line.replace(",", " ").split()
        if len(f) != 8:
            raise ValueError(f"{path}:{no}: expected 'timestamp tx ty tz qx qy qz qw', got {len(f)} fields")
        v = [_number(x, path, no) for x in f]
        if not np.isfinite(v[0]) or v[0] <= last:
            raise ValueError(f"{path}:{no}: timestamps must strictly increase ({v[0]!r} after {last!r})")
        last = v[0]
        q = np.array([v[7], v[4], v[5], v[6]], np.float64)          # file order x y z w -> w x y z
        n = np.linalg.norm(q)
        if not np.isfinite(q).all() or not n > 0.0:
            raise ValueError(f"{path}:{no}: the quaternion is zero or not finite")
        if not np.isfinite(v[1:4]).all():
            raise ValueError(f"{path}:{no}: the translation is not finite")
        times.append(v[0])
        poses.append(np.concatenate([q / n, v[1:4]]))
    if len(times) < 2:
        raise ValueError(f"{path}: at least two poses are needed to interpolate")
    return np.array(times, np.float64), np.array(poses, np.float64)


def read_camera(path):
    """camera.json -> a dict with float64 intrinsics in the HALF-pixel convention, the model, its coefficients, T_body_cam
    [qw,qx,qy,qz,tx,ty,tz], depth_scale and zoom."""
    with open(path) as fh:
        try:
            raw = json.load(fh)
        except json.JSONDecodeError as e:
            raise ValueError(f"{path}:{e.lineno}: not valid json ({e.msg})") from None
    for key in ("width", "height", "fx", "fy", "cx", "cy"):
        if key not in raw:
            raise ValueError(f"{path}: '{key}' is missing")
    model = raw.get("model", "pinhole")
    if model not in MODELS:
        raise ValueError(f"{path}: unknown model {model!r} (one of {', '.join(MODELS)})")
    dist = [float(v) for v in raw.get("distortion") or []]
    if len(dist) != DISTORTION_LENGTH[model]:
        raise ValueError(f"{path}: model {model!r} takes {DISTORTION_LENGTH[model]} distortion coefficients, got {len(dist)}")
    centre = raw.get("pixel_centre", "integer")
    if centre not in ("integer", "half"):
        raise ValueError(f"{path}: pixel_centre must be 'integer' or 'half', got {centre!r}")
    shift = 0.5 if centre == "integer" else 0.0
    T_bc = np.array(raw.get("T_body_cam", [1, 0, 0, 0, 0, 0, 0]), np.float64)
    if T_bc.shape != (7,) or not np.isfinite(T_bc).all() or not np.linalg.norm(T_bc[:4]) > 0:
        raise ValueError(f"{path}: T_body_cam must be [qw,qx,qy,qz,tx,ty,tz] with a non-zero quaternion")
    T_bc[:4] /= np.linalg.norm(T_bc[:4])
    cam = {"width": int(raw["width"]), "height": int(raw["height"]), "fx": float(raw["fx"]), "fy": float(raw["fy"]),
           "cx": float(raw["cx"]) + shift, "cy": float(raw["cy"]) + shift, "model": model, "distortion": dist,
           "T_body_cam": T_bc, "depth_scale": float(raw.get("depth_scale", 5000.0)), "zoom": float(raw.get("zoom", 1.0))}
    if cam["width"] < 1 or cam["height"] < 1 or not cam["fx"] > 0 or not cam["fy"] > 0 or not cam["depth_scale"] > 0 \
            or not cam["zoom"] > 0:
        raise ValueError(f"{path}: width, height, fx, fy, depth_scale and zoom must be positive")
    return cam


class Recording:
    """One recording directory as read_recording leaves it: ``camera`` (read_camera), ``frames`` [(timestamp, path)],
    ``pose_times`` [N], ``poses`` [N,7] body-to-world (qw,qx,qy,qz,tx,ty,tz; unit quaternions), ``depth`` [(timestamp, path)]
    or None without a depth.txt."""

    def __init__(self, root, camera, frames, pose_times, poses, depth):
        self.root, self.camera, self.frames, self.pose_times, self.poses, self.depth = root, camera, frames, pose_times, poses, depth


def read_recording(root):
    """Parses camera.json, frames.txt, poses.txt and the optional depth.txt of one recording.  Refuses, with a ValueError that
    names the file (and the line of a text file): a missing required file, an unknown model, a distortion list of the wrong
    length, timestamps that do not strictly increase, a zero or non-finite quaternion."""
    for name in ("camera.json", "frames.txt", "poses.txt"):
        if not os.path.isfile(os.path.join(root, name)):
            raise ValueError(f"{os.path.join(root, name)}: the file is missing (a recording holds camera.json, frames.txt, "
                             "poses.txt and optionally depth.txt)")
    camera = read_camera(os.path.join(root, "camera.json"))
    frames = _read_stamped_paths(os.path.join(root, "frames.txt"), root)
    if not frames:
        raise ValueError(f"{os.path.join(root, 'frames.txt')}: no frames listed")
    times, poses = _read_poses(os.path.join(root, "poses.txt"))
    dpath = os.path.join(root, "depth.txt")
    depth = _read_stamped_paths(dpath, root) if os.path.isfile(dpath) else None
    return Recording(root, camera, frames, times, poses, depth)


def find_recordings(path):
    """``path`` itself when it holds a camera.json, else its sub-directories that do, sorted."""
    if os.path.isfile(os.path.join(path, "camera.json")):
        return [path]
    subs = sorted(d for d in (os.listdir(path) if os.path.isdir(path) else [])
                  if os.path.isfile(os.path.join(path, d, "camera.json")))
    if not subs:
        raise ValueError(f"{path}: neither a recording (no camera.json) nor a directory of recordings")
    return [os.path.join(path, d) for d in subs]


# ---- association ------------------------------------------------------------------------------------------------------------------
def interpolate_pose(times, poses, t, max_gap=np.inf):
    """The pose [7] at time ``t`` between the two bracketing poses -- translation linear, rotation slerp along the short arc --
    or None when t lies before the first / after the last pose or the bracketing poses are more than ``max_gap`` apart.  At a
    pose's own timestamp the pose itself comes back, whatever the gaps around it."""
    if t < times[0] or t > times[-1]:
        return None
    i = min(int(np.searchsorted(times, t, side="right")) - 1, len(times) - 2)
    if t == times[i]:
        return poses[i].copy()
    if t == times[i + 1]:
        return poses[i + 1].copy()
    dt = times[i + 1] - times[i]
    if dt > max_gap:
        return None
    a = (t - times[i]) / dt
    return np.concatenate([slerp(poses[i, :4], poses[i + 1, :4], a), poses[i, 4:] + a * (poses[i + 1, 4:] - poses[i, 4:])])


def associate_depth(frame_times, depth):
    """Each depth file goes to the frame with the nearest timestamp, within DEPTH_MAX_DT; a frame keeps the closest of the files
    that chose it.  Returns one path or None per frame."""
    out, best = [None] * len(frame_times), [np.inf] * len(frame_times)
    ft = np.asarray(frame_times, np.float64)
    for t, path in depth or []:
        j = int(np.argmin(np.abs(ft - t)))
        d = abs(ft[j] - t)
        if d <= DEPTH_MAX_DT and d < best[j]:
            out[j], best[j] = path, d
    return out


def select_frames(rec, max_gap=0.5, stride=1, min_baseline=0.0, require_depth=False, depth=None):
    """The trajectories of one recording: a list of lists of frames {t, path, depth (path or None), T_wc [7] float64}.
    A frame without a pose (interpolate_pose) is dropped and the next kept frame starts a new trajectory; inside a trajectory
    every ``stride``-th frame is taken, and of those the ones whose camera centre has moved at least ``min_baseline`` metres
    since the last kept frame (a trajectory's first frame is always kept).  ``require_depth``: a frame without an associated
    depth file is left out before the stride is applied -- like a frame the stride skips, it does not break the trajectory:
    the motion to the next kept frame comes from the absolute poses and spans it.  ``depth``: the result of ``associate_depth``
    where the caller already has it."""
    if stride < 1:
        raise ValueError("rec_stride must be >= 1")
    if depth is None:
        depth = associate_depth([t for t, _ in rec.frames], rec.depth)
    runs, run = [], []
    for (t, path), dpath in zip(rec.frames, depth):
        T_wb = interpolate_pose(rec.pose_times, rec.poses, t, max_gap)
        if T_wb is None:
            if run:
                runs.append(run)
            run = []
            continue
        if require_depth and dpath is None:
            continue
        run.append({"t": t, "path": path, "depth": dpath, "T_wc": compose(T_wb, rec.camera["T_body_cam"])})
    if run:
        runs.append(run)
    out = []
    for run in runs:
        kept = []
        for fr in run[::stride]:
            if not kept or np.linalg.norm(fr["T_wc"][4:] - kept[-1]["T_wc"][4:]) >= min_baseline:
                kept.append(fr)
        out.append(kept)
    return out


def relative_motions(T_wc):
    """Camera-to-world poses [N,7] float64 -> the frame-to-frame motions [N,7] float32 (qw,qx,qy,qz,tx,ty,tz) the network takes:
    T_prev^-1 . T_cur, i.e. a point X of the current camera is R X + t in the previous camera (the convention stated at
    m4d_pose_accumulate).  Unit quaternion with w >= 0; float64 throughout, rounded to float32 once at the end; the first
    frame gets the identity."""
    T_wc = np.asarray(T_wc, np.float64).reshape(-1, 7)
    out = np.zeros((len(T_wc), 7), np.float64)
    out[:, 0] = 1.0
    for i in range(1, len(T_wc)):
        qp, qc = T_wc[i - 1, :4] / np.linalg.norm(T_wc[i - 1, :4]), T_wc[i, :4] / np.linalg.norm(T_wc[i, :4])
        q = quat_mul(quat_conj(qp), qc)
        q /= np.linalg.norm(q)
        out[i, :4] = -q if q[0] < 0 else q
        out[i, 4:] = quat_rot(qp).T @ (T_wc[i, 4:] - T_wc[i - 1, 4:])
    return out.astype(np.float32)


def output_camera(cam, H, W):
    """(fx', fy', cx', cy') float64 of the pinhole camera the frames are resampled to at H x W: the source scaled by
    s = max(H/ih, W/iw) * zoom about the image centre.  zoom = 1 fills the frame and crops the excess symmetrically; zoom < 1
    widens the field of view and leaves pixels without a source."""
    ih, iw = float(cam["height"]), float(cam["width"])
    s = max(H / ih, W / iw) * float(cam.get("zoom", 1.0))
    x0, y0 = (iw - W / s) / 2.0, (ih - H / s) / 2.0
    return cam["fx"] * s, cam["fy"] * s, (cam["cx"] - x0) * s, (cam["cy"] - y0) * s


# ---- the loader -------------------------------------------------------------------------------------------------------------------
class DataLoaderRecording(DataLoaderGeneric):
    """Dataloader for recordings in the format of the module's docstring.  ``records_path`` is one recording or a directory of
    recordings (sorted; one or more trajectories each); no dataset root is needed.  Rows are made in memory; intrinsics are per
    sample (every recording has its own camera), so one ``--eval_streams`` step may mix cameras: frames are decoded in groups of
    one recording.  Ground truth: 16-bit PNGs / depth_scale, nearest through the same table.  A sample without ground truth
    cannot be scored, so every use case but predict -- and predict when ``require_depth`` is set (ground-truth panels) -- refuses
    a recording without depth.txt and leaves out the frames no depth file is associated with (``select_frames``): there every
    frame carries a map.  In a plain predict run ground truth is decoded where it exists; in a sequence batch that mixes
    frames with and without it the latter get an all-zero map.  ``allow_missing_depth`` (train only: the photometric loss needs
    no ground truth) lifts the refusal for the 'train' use case in the same way: such frames get the all-zero map.
    ``allow_missing_depth_streams`` lifts it for the 'eval_streams' use case (main.py --consistency, which scores without ground
    truth): every frame is kept, and a step without any ground truth carries no ``depth``."""

    def __init__(self, stride=1, min_baseline=0.0, max_gap=0.5):
        super().__init__("recording")
        self.depth_type = "map"
        self.stride, self.min_baseline, self.max_gap = stride, min_baseline, max_gap
        self.require_depth = False                                  # predict: ground truth needed for every frame (gt / err panels)
        self.allow_missing_depth = False                            # train: a recording without depth.txt is accepted
        self.allow_missing_depth_streams = False                    # eval_streams: the same (main.py --consistency), every frame kept
        self.recordings, self._tables = None, {}

    def _set_output_size(self, out_size=None):
        if out_size is None:
            raise ValueError("the recording loader needs out_size=[height, width]: a recording has no default network size")
        self.out_size = [int(out_size[0]), int(out_size[1])]

    def get_dataset(self, usecase, settings, **kw):
        roots = dict(settings.db_path_config or {})
        roots.setdefault(self.db_name, settings.records_path)       # frame paths are relative to their recording, not to a root
        self.recordings, self._tables = None, {}
        return super().get_dataset(usecase, settings._replace(db_path_config=roots), **kw)

    def has_depth(self, records_path):
        """Whether every recording of ``records_path`` lists ground truth (known before anything is loaded)."""
        return all(os.path.isfile(os.path.join(r, "depth.txt")) for r in find_recordings(records_path))

    def _get_trajectories(self):
        self.recordings = [read_recording(r) for r in find_recordings(self.records_path)]
        need_depth = self.usecase != "predict" or self.require_depth
        if self.usecase == "train" and self.allow_missing_depth:
            need_depth = False
        no_gt = self.usecase == "eval_streams" and self.allow_missing_depth_streams
        if no_gt:
            need_depth = False
        if need_depth:
            for rec in self.recordings:
                if rec.depth is None:
                    raise ValueError(f"{rec.root}: no depth.txt -- the '{self.usecase}' use case scores against ground truth; a "
                                     "recording without it can only be predicted (--mode=predict)")
        trajectories = []
        for ri, rec in enumerate(self.recordings):
            depth = associate_depth([t for t, _ in rec.frames], rec.depth)
            if need_depth and depth.count(None):
                print(f"{rec.root}: {depth.count(None)} of {len(rec.frames)} frames have no depth file within {DEPTH_MAX_DT} s "
                      "and are left out")
            for frames in select_frames(rec, self.max_gap, self.stride, self.min_baseline, require_depth=need_depth, depth=depth):
                motions = relative_motions(np.stack([fr["T_wc"] for fr in frames])) if frames else []
                rows = []
                for i, (fr, m) in enumerate(zip(frames, motions)):
                    # no_gt: the set is scored without ground truth, so none is read (not even where a recording has some)
                    row = {"id": i, "camera_l": fr["path"], "depth": "" if no_gt else fr["depth"] or "", "rec": ri,
                           "timestamp": fr["t"]}
                    row.update(zip(("qw", "qx", "qy", "qz", "tx", "ty", "tz"), (float(v) for v in m)))
                    rows.append(row)
                if rows:
                    trajectories.append(rows)
        if not trajectories:
            raise ValueError(f"{self.records_path}: no frame of any recording lies inside its trajectory file's time span")
        return trajectories

    def _out_cam(self, ri):
        return output_camera(self.recordings[ri].camera, self.out_size[0], self.out_size[1])

    def _camera(self, row):
        fx, fy, cx, cy = (float(np.float32(v)) for v in self._out_cam(row["rec"]))
        return (fx, fy), (cx, cy)

    def _perform_augmentation(self):
        self._augmentation_step_color(invert_color=False)

    # -- host side ----------------------------------------------------------------------------------------------------------
    def _load_raw(self, row):
        from PIL import Image
        cam = self.recordings[row["rec"]].camera
        want = (cam["height"], cam["width"])
        with Image.open(row["camera_l"]) as im:
            rgb = np.asarray(im.convert("RGB"), dtype=np.uint8)
        if rgb.shape[:2] != want:
            raise ValueError(f"{row['camera_l']}: the image is {rgb.shape[0]}x{rgb.shape[1]} (h x w), camera.json says "
                             f"{want[0]}x{want[1]}")
        depth = None
        if row["depth"]:
            depth = self._read_depth(row["depth"])
            if depth.shape != want:
                raise ValueError(f"{row['depth']}: the depth map is {depth.shape[0]}x{depth.shape[1]} (h x w), camera.json says "
                                 f"{want[0]}x{want[1]}: it must be registered to the colour camera")
        return {"rgb": rgb, "depth": depth, "rec": row["rec"]}

    # -- device side --------------------------------------------------------------------------------------------------------
    def _table(self, ri):
        """The undistortion table [oh,ow,2] of recording ``ri`` at the output size: built on first use, kept on the device."""
        if ri not in self._tables:
            cam = self.recordings[ri].camera
            oh, ow = self.out_size
            table = torch.empty((oh, ow, 2), dtype=torch.float32, device=self.device)
            f4 = ctypes.c_float * 4
            dist = (ctypes.c_float * len(cam["distortion"]))(*cam["distortion"]) if cam["distortion"] else None
            check(lib.m4d_undistort_map(MODELS[cam["model"]], dist, f4(cam["fx"], cam["fy"], cam["cx"], cam["cy"]),
                                        f4(*self._out_cam(ri)), cam["height"], cam["width"], oh, ow, dptr(table), stream_ptr()),
                  "m4d_undistort_map")
            self._tables[ri] = table
        return self._tables[ri]

    def _decode_device(self, raws):
        """Raw frames -> (RGB_im [T,h,w,3], depth [T,h,w,1] or None): one launch per modality per recording present."""
        oh, ow = self.out_size
        T = len(raws)
        groups = {}
        for i, r in enumerate(raws):
            groups.setdefault(r["rec"], []).append(i)
        rgb_out = torch.empty((T, oh, ow, 3), dtype=torch.float32, device=self.device)
        any_depth = any(r["depth"] is not None for r in raws)
        all_depth = all(r["depth"] is not None for r in raws)
        dep_out = None
        if any_depth or (self.usecase == "train" and self.allow_missing_depth):      # a training batch always carries a map
            dep_out = (torch.empty if all_depth else torch.zeros)((T, oh, ow, 1), dtype=torch.float32, device=self.device)
        for ri, idx in groups.items():
            cam = self.recordings[ri].camera
            ih, iw = cam["height"], cam["width"]
            table = self._table(ri)
            stack = self._to_device(np.stack([raws[i]["rgb"] for i in idx]))
            dst = rgb_out if len(idx) == T else torch.empty((len(idx), oh, ow, 3), dtype=torch.float32, device=self.device)
            check(lib.m4d_decode_rgb8_remap(dptr(stack, "rgb", torch.uint8), dptr(table), len(idx), ih, iw, oh, ow, dptr(dst),
                                            stream_ptr()), "m4d_decode_rgb8_remap")
            if dst is not rgb_out:
                rgb_out[idx] = dst
            didx = [i for i in idx if raws[i]["depth"] is not None]
            if didx:
                dstack = self._to_device(np.stack([raws[i]["depth"] for i in didx]).view(np.int16))   # no uint16 transfers: same bits
                ddst = dep_out if len(didx) == T else torch.empty((len(didx), oh, ow, 1), dtype=torch.float32, device=self.device)
                check(lib.m4d_decode_depth16_remap(dptr(dstack, "depth", torch.int16), dptr(table),
                                                   float(np.float32(1.0) / np.float32(cam["depth_scale"])), len(didx), ih, iw,
                                                   oh, ow, dptr(ddst), stream_ptr()), "m4d_decode_depth16_remap")
                if ddst is not dep_out:
                    dep_out[didx] = ddst
        return rgb_out, dep_out
