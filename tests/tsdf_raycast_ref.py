"""m4d_tsdf_raycast of include/m4depth_hip.h restated in numpy, from the header's statement: one loop per ray over the records of
a ``tsdf_mesh_ref.TsdfVolume`` (a dict keyed by the packed key: nothing here knows about slots or probing).  float64 quantities
are Python floats (IEEE double, one rounding per operation), float32 quantities np.float32."""
import math

import numpy as np

from pose_ref import rot
from voxel_map_ref import HALF
from tsdf_mesh_ref import (F32, F64, PLANE, PLANE_C, PLANE_F, PLANE_NORMAL, PLANE_OFFSET, SPHERE, fuse, look_at_pose,  # noqa: F401
                           plane_frames, plane_poses, render_plane, render_sphere, sphere_frames)

NAN32 = np.array([0x7FC00000], np.uint32).view(F32)[0]          # the miss without a fill


def refused(h, w, near, far, voxel, trunc, min_frames, window=None):
    """The value refusals of the header (the pointer, geometry and stride ones aside), on the float32 arguments."""
    near, far, voxel = F32(near), F32(far), F32(voxel)
    if h < 1 or w < 1 or h * w > 1 << 24 or not (far > near and near > 0):
        return True
    if not (voxel > 0 and np.isfinite(voxel)) or not 2 <= trunc <= 8 or min_frames < 1 or (window is not None and window < 1):
        return True
    return (float(far) - float(near)) / (float(voxel) * 0.5) > float(1 << 20)


def raycast(records, f, c, pose, h, w, voxel, trunc, min_frames, near=1.0, far=80.0, guide=None, window=None, fill=None,
            counters=None):
    """(depth [h,w] float32, hits) of one sample.  ``records``: key -> [S, n, ...] (``TsdfVolume.records``); ``guide`` / ``fill``
    [h,w] float32 or None; ``counters``: a dict that takes ``samples`` (positions sampled, both modes) and ``pixels``."""
    assert not refused(h, w, near, far, voxel, trunc, min_frames, window) and (guide is None) == (window is None)
    out = np.full((h, w), NAN32, F32) if fill is None else np.array(fill, F32).reshape(h, w).copy()
    pose = np.asarray(pose, F64)
    if not np.isfinite(pose).all():
        return out, 0
    R = [[float(v) for v in r] for r in rot(pose)]
    t = [float(v) for v in pose[4:]]
    near32, far32 = F32(near), F32(far)
    voxel = float(F32(voxel))
    hv = voxel * 0.5
    K2 = 2 * int(trunc)
    fx, fy, cx, cy = F32(f[0]), F32(f[1]), F32(c[0]), F32(c[1])
    hits = samples = 0

    def sample(ax, ay, z):
        """(known, D) at depth z of the ray."""
        X, Y = ax * z, ay * z
        cell = []
        for j in range(3):
            fl = math.floor((((R[j][0] * X + R[j][1] * Y) + R[j][2] * z) + t[j]) / voxel)
            if not -HALF <= fl < HALF:
                return False, None
            cell.append(fl + HALF)
        rec = records.get((cell[0] << 42) | (cell[1] << 21) | cell[2])
        if rec is None or rec[1] < min_frames or rec[1] <= 0:
            return False, None
        return True, F32(rec[0]) / F32(rec[1])

    for row in range(h):
        ay = float((F32(row) + F32(0.5) - cy) / fy)
        for col in range(w):
            ax = float((F32(col) + F32(0.5) - cx) / fx)
            z_lo, z_hi = float(near32), float(far32)
            if guide is not None:
                g = F32(guide[row, col])
                if np.isfinite(g) and near32 <= g <= far32:
                    Wd = (float(int(window)) * float(int(trunc))) * voxel
                    z_lo, z_hi = max(float(near32), float(g) - Wd), min(float(far32), float(g) + Wd)
            n_max = math.floor((z_hi - z_lo) / hv)
            i, fine, run, prev = 0, False, 0, None
            while i <= n_max:
                known, D = sample(ax, ay, z_lo + float(i) * hv)
                samples += 1
                if not fine:
                    if not known:
                        i += K2
                        continue
                    i = 0 if i == 0 else i - K2 + 1
                    fine, run, prev = True, 0, None
                    continue
                if not known:
                    prev = None
                    run += 1
                    if run == K2:
                        fine = False
                        i += K2
                    else:
                        i += 1
                    continue
                run = 0
                if prev is not None and prev >= 0 and D < 0:
                    z_prev = z_lo + float(i - 1) * hv
                    out[row, col] = F32(z_prev + hv * float(prev / (prev - D)))
                    hits += 1
                    break
                prev = D
                i += 1
    if counters is not None:
        counters["samples"] = counters.get("samples", 0) + samples
        counters["pixels"] = counters.get("pixels", 0) + h * w
    return out, hits
