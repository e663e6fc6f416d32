"""m4d_tsdf_render of include/m4depth_hip.h restated in numpy, from the header's statement: ``tsdf_raycast_ref.raycast``'s loop per
ray over the records of a ``tsdf_mesh_ref.TsdfVolume`` with the trilinear sample and, at the hit, the normal, the colour and the
shaded byte triple.  Nothing here knows about slots, probing, or which corners a thread keeps.  float64 quantities are Python
floats (IEEE double, one rounding per operation), float32 quantities np.float32."""
import math

import numpy as np

from pose_ref import rot
from voxel_map_ref import HALF
from tsdf_raycast_ref import F32, F64, NAN32, refused          # noqa: F401

INTERP = {"nearest": 0, "trilinear": 1}


def lerp(a, b, t):
    return a + t * (b - a)                                      # np.float32: a subtraction, a product, a sum


def tri(v, fr):
    x00, x10, x01, x11 = lerp(v[0], v[1], fr[0]), lerp(v[2], v[3], fr[0]), lerp(v[4], v[5], fr[0]), lerp(v[6], v[7], fr[0])
    return lerp(lerp(x00, x10, fr[1]), lerp(x01, x11, fr[1]), fr[2])


def rgb_byte(v):
    """m4d_depth_export's rgb rule on one np.float32."""
    return int(np.rint(np.minimum(np.fmax(v, F32(0.0)), F32(1.0)) * F32(255.0)))


def render(records, f, c, pose, h, w, voxel, trunc, min_frames, near=1.0, far=80.0, guide=None, window=None, fill=None,
           interp=0, counters=None):
    """One sample: {"depth" [h,w] float32, "hits", "hit" [h,w] bool, "z_star" [h,w] float64 (NaN at a miss), "normal" / "colour"
    [h,w,3] float32, "view" [h,w,3] uint8}.
    ``records``: key -> [S, n, sr, sg, sb, nc]; ``interp`` 0 nearest, 1 trilinear; the rest as ``tsdf_raycast_ref.raycast``."""
    assert not refused(h, w, near, far, voxel, trunc, min_frames, window) and (guide is None) == (window is None)
    assert interp in (0, 1)
    out = np.full((h, w), NAN32, F32) if fill is None else np.array(fill, F32).reshape(h, w).copy()
    normal, colour = np.full((h, w, 3), NAN32, F32), np.full((h, w, 3), NAN32, F32)
    view = np.zeros((h, w, 3), np.uint8)
    hit = np.zeros((h, w), bool)
    z_stars = np.full((h, w), np.nan, F64)                      # the float64 z* of the hits: where the surface point lies
    res = {"depth": out, "hits": 0, "hit": hit, "z_star": z_stars, "normal": normal, "colour": colour, "view": view}
    pose = np.asarray(pose, F64)
    if not np.isfinite(pose).all():
        return res
    R = [[float(v) for v in r] for r in rot(pose)]
    t = [float(v) for v in pose[4:]]
    near32, far32 = F32(near), F32(far)
    voxel = float(F32(voxel))
    hv = voxel * 0.5
    K2 = 2 * int(trunc)
    fx, fy, cx, cy = F32(f[0]), F32(f[1]), F32(c[0]), F32(c[1])
    hits = samples = 0
    cells = {}                                                  # base cell -> its corners (a cache of this function's only)

    def known_record(cell):
        """The record of the voxel ``cell`` (three unbiased indices) when it is KNOWN, else None."""
        if not all(-HALF <= i < HALF for i in cell):
            return None
        rec = records.get(((cell[0] + HALF) << 42) | ((cell[1] + HALF) << 21) | (cell[2] + HALF))
        if rec is None or rec[1] < min_frames or rec[1] <= 0:
            return None
        return rec

    def quotients(ax, ay, z):
        X, Y = ax * z, ay * z
        return [(((R[j][0] * X + R[j][1] * Y) + R[j][2] * z) + t[j]) / voxel for j in range(3)]

    def corners(q):
        """(the eight KNOWN records or None each, fr) of the base cell of the point with quotients ``q``; None: not finite."""
        g = [v - 0.5 for v in q]
        if not all(math.isfinite(v) for v in g):
            return None
        B = tuple(math.floor(v) for v in g)
        fr = [F32(v - float(b)) for v, b in zip(g, B)]
        if B not in cells:
            cells[B] = [known_record((B[0] + (k & 1), B[1] + ((k >> 1) & 1), B[2] + (k >> 2))) for k in range(8)]
        return cells[B], fr

    def nearest(q):
        if not all(math.isfinite(v) for v in q):
            return None
        return known_record(tuple(math.floor(v) for v in q))

    def sample(ax, ay, z, fine):
        """(known, D) at depth z of the ray."""
        q = quotients(ax, ay, z)
        rec = nearest(q)
        if rec is None:
            return False, None
        D = F32(rec[0]) / F32(rec[1])
        if interp and fine:
            recs, fr = corners(q)
            if all(r is not None for r in recs):
                D = tri([F32(r[0]) / F32(r[1]) for r in recs], fr)
        return True, D

    def mean_colour(rec):
        return [(F32(rec[k]) / F32(rec[5])) / F32(255.0) for k in (2, 3, 4)]

    def surface(row, col, ax, ay, z_star):
        q = quotients(ax, ay, z_star)
        got = corners(q)
        recs, fr = got if got is not None else ([None] * 8, None)
        full = all(r is not None for r in recs)
        n = None
        if full:
            v = [F32(r[0]) / F32(r[1]) for r in recs]
            gx = lerp(lerp(v[1] - v[0], v[3] - v[2], fr[1]), lerp(v[5] - v[4], v[7] - v[6], fr[1]), fr[2])
            gy = lerp(lerp(v[2] - v[0], v[3] - v[1], fr[0]), lerp(v[6] - v[4], v[7] - v[5], fr[0]), fr[2])
            gz = lerp(lerp(v[4] - v[0], v[5] - v[1], fr[0]), lerp(v[6] - v[2], v[7] - v[3], fr[0]), fr[1])
            G = [float(gx), float(gy), float(gz)]
            cam = [(R[0][j] * G[0] + R[1][j] * G[1]) + R[2][j] * G[2] for j in range(3)]
            length = math.sqrt((cam[0] * cam[0] + cam[1] * cam[1]) + cam[2] * cam[2])
            if length > 0.0:
                n = [F32(v / length) for v in cam]
                normal[row, col] = n
        col3 = None
        if full and all(r[5] > 0 for r in recs):
            m = [mean_colour(r) for r in recs]
            col3 = [tri([m[k][ch] for k in range(8)], fr) for ch in range(3)]
        else:
            rec = nearest(q)
            if rec is not None and rec[5] > 0:
                col3 = mean_colour(rec)
        if col3 is not None:
            colour[row, col] = col3
        shade = F32(1.0)
        if n is not None:
            vl = math.sqrt((ax * ax + ay * ay) + 1.0)
            dot = ((float(n[0]) * ax + float(n[1]) * ay) + float(n[2])) / vl
            shade = F32(0.25 + 0.75 * max(0.0, -dot))
        view[row, col] = [rgb_byte((F32(0.5) if col3 is None else col3[ch]) * shade) for ch in range(3)]

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
                known, D = sample(ax, ay, z_lo + float(i) * hv, fine)
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
                    z_star = z_prev + hv * float(prev / (prev - D))
                    out[row, col] = F32(z_star)
                    hit[row, col] = True
                    z_stars[row, col] = z_star
                    surface(row, col, ax, ay, z_star)
                    hits += 1
                    break
                prev = D
                i += 1
    if counters is not None:
        counters["samples"] = counters.get("samples", 0) + samples
        counters["pixels"] = counters.get("pixels", 0) + h * w
    res["hits"] = hits
    return res
