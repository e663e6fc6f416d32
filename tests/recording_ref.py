"""Numpy restatement of m4d_undistort_map, m4d_decode_rgb8_remap and m4d_decode_depth16_remap in the operation order
include/m4depth_hip.h states: the table in float32 (one rounding per operation: every intermediate is a float32 array) and in
float64, the two samplers in float32.  Plus the issue's two fixture cameras and a small recording writer for the tests."""
import json
import os

import numpy as np

F = np.float32

CAMERA_A = {"width": 94, "height": 60, "pixel_centre": "half", "fx": 57.33175, "fy": 57.162, "cx": 45.964375, "cy": 31.109375,
            "model": "radtan", "distortion": [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0]}     # EuRoC cam0 / 8
CAMERA_B = {"width": 64, "height": 64, "pixel_centre": "half", "fx": 23.87225, "fy": 23.871625, "cx": 31.92875, "cy": 32.175,
            "model": "equidistant", "distortion": [0.0034823894, 0.0007150348, -0.0020532361, 0.00020293673]}  # TUM-VI / 8
MODELS = {"pinhole": 0, "radtan": 1, "equidistant": 2}


def undistort_map(model, dist, src_cam, out_cam, ih, iw, oh, ow, dtype=F):
    """[oh,ow,2] table of m4d_undistort_map; ``dtype`` float32 = the device's arithmetic, float64 = the yardstick.  The camera
    numbers are rounded to float32 first in both (the entry point takes float32)."""
    T = dtype
    fx, fy, cx, cy = (T(F(v)) for v in src_cam)
    fxo, fyo, cxo, cyo = (T(F(v)) for v in out_cam)
    k = [T(F(v)) for v in dist]
    col, row = np.meshgrid(np.arange(ow).astype(T), np.arange(oh).astype(T))
    half, one, two = T(0.5), T(1.0), T(2.0)
    x = ((col + half) - cxo) / fxo
    y = ((row + half) - cyo) / fyo
    with np.errstate(all="ignore"):
        if model == "pinhole":
            xd, yd = x, y
        elif model == "radtan":
            k1, k2, p1, p2, k3 = k
            r2 = x * x + y * y
            rad = one + r2 * (k1 + r2 * (k2 + r2 * k3))
            xd = x * rad + ((((two * p1) * x) * y) + p2 * (r2 + (two * x) * x))
            yd = y * rad + (p1 * (r2 + (two * y) * y) + (((two * p2) * x) * y))
        elif model == "equidistant":
            r = np.sqrt(x * x + y * y)
            th = np.arctan(r)
            th2 = th * th
            thd = th * (one + th2 * (k[0] + th2 * (k[1] + th2 * (k[2] + th2 * k[3]))))
            s = np.where(r > T(F(1e-8)), thd / np.where(r > 0, r, one), one)
            xd, yd = x * s, y * s
        else:
            raise ValueError(model)
        u = (xd * fx + cx) - half
        v = (yd * fy + cy) - half
        assert u.dtype == T and v.dtype == T
        ok = (u >= -half) & (u <= T(F(iw) - F(0.5))) & (v >= -half) & (v <= T(F(ih) - F(0.5)))
    out = np.stack([np.where(ok, u, T(-1.0)), np.where(ok, v, T(-1.0))], axis=-1)
    return out.astype(T)


def has_source(table):
    with np.errstate(invalid="ignore"):
        return (table[..., 0] >= F(-0.5)) & (table[..., 1] >= F(-0.5)) & np.isfinite(table).all(axis=-1)


def _axis(src, n):
    src = np.where(np.isfinite(src), src, F(0.0)).astype(F)
    fl = np.floor(src)
    lo = np.clip(fl, 0, n - 1).astype(np.int64)
    hi = np.clip(np.ceil(src), 0, n - 1).astype(np.int64)
    return lo, hi, (src - fl).astype(F)


def decode_rgb8_remap(images, table):
    """uint8 [n,ih,iw,3] through table [oh,ow,2] float32 -> float32 [n,oh,ow,3] (m4d_decode_rgb8_remap)."""
    n, ih, iw, _ = images.shape
    table = table.astype(F)
    ok = has_source(table)
    xlo, xhi, xl = _axis(table[..., 0], iw)
    ylo, yhi, yl = _axis(table[..., 1], ih)
    img = images.astype(F) / F(255.0)
    tl, tr = img[:, ylo, xlo], img[:, ylo, xhi]
    bl, br = img[:, yhi, xlo], img[:, yhi, xhi]
    xl, yl = xl[None, ..., None], yl[None, ..., None]
    top = tl + (tr - tl) * xl
    bot = bl + (br - bl) * xl
    out = top + (bot - top) * yl
    assert out.dtype == F
    return np.where(ok[None, ..., None], out, F(0.0)).astype(F)


def decode_depth16_remap(raw, table, inv_scale):
    """uint16 [n,ih,iw] through table -> float32 [n,oh,ow,1] (m4d_decode_depth16_remap)."""
    n, ih, iw = raw.shape
    table = table.astype(F)
    ok = has_source(table)
    safe = np.where(np.isfinite(table), table, F(0.0)).astype(F)
    xi = np.clip(np.floor(safe[..., 0] + F(0.5)), 0, iw - 1).astype(np.int64)
    yi = np.clip(np.floor(safe[..., 1] + F(0.5)), 0, ih - 1).astype(np.int64)
    q = raw[:, yi, xi]
    out = np.where((q != 0) & ok[None], q.astype(F) * F(inv_scale), F(0.0)).astype(F)
    return out[..., None]


def half_pixel_table(ih, iw, oh, ow):
    """The table of source coordinates m4d_decode_rgb8_resize computes per axis (half_pixel_axis, float32)."""
    sy, sx = F(ih) / F(oh), F(iw) / F(ow)
    v = (np.arange(oh).astype(F) + F(0.5)) * sy - F(0.5)
    u = (np.arange(ow).astype(F) + F(0.5)) * sx - F(0.5)
    return np.stack(np.broadcast_arrays(u[None, :], v[:, None]), axis=-1).astype(F)


# ---- a recording on disk ------------------------------------------------------------------------------------------------------------
def smooth_image(h, w, phase):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    rgb = np.stack([0.5 + 0.5 * np.sin(0.11 * x + 0.07 * y + phase), 0.5 + 0.5 * np.cos(0.05 * x - 0.13 * y + 2 * phase),
                    0.5 + 0.5 * np.sin(0.09 * (x + y) - phase)], axis=-1)
    return (rgb * 255.0).round().astype(np.uint8)


def smooth_depth(h, w, phase, scale=5000.0):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    d = 4.0 + 2.0 * np.sin(0.05 * x + phase) + 1.5 * np.cos(0.08 * y - phase)
    out = (d * scale).round().astype(np.uint16)
    out[::7, ::5] = 0                                            # holes: no measurement
    return out


def trajectory_poses(n, dt=0.1, t0=100.0):
    """Body-to-world poses of a smooth arc: ([n] times, [n,7] w,x,y,z,tx,ty,tz)."""
    times = t0 + dt * np.arange(n)
    out = []
    for i in range(n):
        ang = 0.02 * i
        axis = np.array([0.2, 1.0, 0.1]) / np.linalg.norm([0.2, 1.0, 0.1])
        q = np.concatenate([[np.cos(ang / 2)], axis * np.sin(ang / 2)])
        out.append(np.concatenate([q, [0.05 * i, 0.01 * np.sin(0.5 * i), 0.3 * i]]))
    return times, np.array(out)


def write_recording(root, camera, n_frames, with_depth, extra=None, frame_offset=0.03):
    """A recording directory: ``n_frames`` PNG frames at timestamps strictly inside the span of n_frames + 1 poses, optional
    16-bit depth PNGs at the frames' timestamps.  Returns (frame timestamps, pose times, poses)."""
    from PIL import Image
    os.makedirs(os.path.join(root, "rgb"), exist_ok=True)
    cam = dict(camera)
    cam.update(extra or {})
    with open(os.path.join(root, "camera.json"), "w") as fh:
        json.dump(cam, fh)
    times, poses = trajectory_poses(n_frames + 1)
    with open(os.path.join(root, "poses.txt"), "w") as fh:
        fh.write("# timestamp tx ty tz qx qy qz qw\n")
        for t, p in zip(times, poses):
            fh.write("%.6f " % t + " ".join(repr(float(p[i])) for i in (4, 5, 6, 1, 2, 3, 0)) + "\n")
    h, w = cam["height"], cam["width"]
    stamps = times[:n_frames] + frame_offset
    with open(os.path.join(root, "frames.txt"), "w") as fh:
        fh.write("# timestamp filename\n")
        for i, t in enumerate(stamps):
            Image.fromarray(smooth_image(h, w, 0.2 * i)).save(os.path.join(root, "rgb", f"{i:04d}.png"))
            fh.write("%.6f rgb/%04d.png\n" % (t, i))
    if with_depth:
        os.makedirs(os.path.join(root, "depth"), exist_ok=True)
        with open(os.path.join(root, "depth.txt"), "w") as fh:
            for i, t in enumerate(stamps):
                Image.fromarray(smooth_depth(h, w, 0.2 * i, cam.get("depth_scale", 5000.0))).save(
                    os.path.join(root, "depth", f"{i:04d}.png"))
                fh.write("%.6f depth/%04d.png\n" % (t + 0.004, i))
    return stamps, times, poses


# ---- the pose chain of m4d_pose_accumulate, float64 -----------------------------------------------------------------------------------
def rot_matrix(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float64)


def pose_step(pose, rot, trans):
    """pose [7] float64 (qw,qx,qy,qz,tx,ty,tz) advanced by one float32 frame-to-frame motion: tw <- R(qw) t + tw, qw <- qw q."""
    q = np.asarray(rot, F).astype(np.float64)
    q = q / np.sqrt(q @ q)
    t = rot_matrix(pose[:4]) @ np.asarray(trans, F).astype(np.float64) + pose[4:]
    aw, ax, ay, az = pose[:4]
    bw, bx, by, bz = q
    p = np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                  aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])
    return np.concatenate([p / np.sqrt(p @ p), t])
