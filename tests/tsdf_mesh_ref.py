"""The TSDF meshes of include/m4depth_hip.h (m4d_tsdf_allocate / _integrate / _extract_vertices / _extract_faces and the host
side of network_ops.tsdf_extract) restated in numpy: a dict keyed by the packed key, float32 and float64 arithmetic exactly as the
header states it, the output sorted as the host sorts it.  Nothing here knows about slots, probing or the 3/4 rule: a volume that
fits its table equals this one bit for bit.  ``exact=True`` is the float64 variant the distance bars of the tests were measured
on: every float32 quantity of the header (the pixel factors, sdf, T, S, D, the crossing sums, the vertex) stays float64."""
import numpy as np

from pose_ref import rot
from voxel_map_ref import HALF, EMPTY, pack, unpack             # the voxel map's keys: csrc/m4d_voxel_hash.h

CELL_MAX = (1 << 21) - 1
F32, F64 = np.float32, np.float64


def _biased(keys):
    """uint64 [m] -> int64 [m,3] biased cell indices 0..2^21-1."""
    k = np.asarray(keys, np.uint64)
    return np.stack([(k >> np.uint64(sh)) & np.uint64(0x1FFFFF) for sh in (42, 21, 0)], axis=-1).astype(np.int64)


def _pack_biased(cells):
    c = np.asarray(cells, np.int64).astype(np.uint64)
    return (c[..., 0] << np.uint64(42)) | (c[..., 1] << np.uint64(21)) | c[..., 2]


def rgb_bytes(rgb):
    """m4d_depth_export's rgb rule: (uint8) rintf(min(max(v, 0), 1) * 255), NaN -> 0."""
    v = np.asarray(rgb, F32)
    return np.rint(np.minimum(np.fmax(v, F32(0.0)), F32(1.0)) * F32(255.0)).astype(np.int64)


class TsdfVolume:
    """``records``: key -> [S, n, sr, sg, sb, nc] (S an np.float32, the rest Python integers); ``dropped_range`` / ``updates``
    as the device counts them (a volume that fits has ``dropped_full`` 0 and ``occupied`` = len(records))."""

    def __init__(self, voxel, trunc, near=1.0, far=80.0, exact=False):
        self.voxel = F32(voxel)
        self.trunc = int(trunc)
        assert np.isfinite(self.voxel) and self.voxel > 0 and 2 <= self.trunc <= 8
        self.near, self.far = F32(near), F32(far)
        self.real = F64 if exact else F32
        self.records = {}
        self.dropped_range = self.updates = 0

    # ---- per frame ---------------------------------------------------------------------------------------------------------------
    def allocate(self, depth, f, c, pose, order=None):
        """``depth`` [h,w] float32, ``f`` / ``c`` the sample's (fx, fy) / (cx, cy), ``pose`` 7 float64; ``order``: a permutation of
        the h*w pixels (the schedule; the result does not depend on it)."""
        depth = np.asarray(depth, F32)
        h, w = depth.shape
        pose = np.asarray(pose, F64)
        if not np.isfinite(pose).all():
            return self
        px = np.arange(h * w) if order is None else np.asarray(order)
        d = depth.reshape(-1)[px]
        with np.errstate(invalid="ignore"):
            keep = np.isfinite(d) & (d >= self.near) & (d <= self.far)
        px, d = px[keep], d[keep]
        row, col = px // w, px % w
        fx, fy, cx, cy = F32(f[0]), F32(f[1]), F32(c[0]), F32(c[1])
        ax = (((col.astype(F32) + F32(0.5)) - cx) / fx).astype(F64)    # float32, m4d_depth_cloud's operand order, then widened
        ay = (((row.astype(F32) + F32(0.5)) - cy) / fy).astype(F64)
        if self.real is F64:                                # the float64 variant: the factors themselves in float64
            ax = ((col.astype(F64) + 0.5) - F64(cx)) / F64(fx)
            ay = ((row.astype(F64) + 0.5) - F64(cy)) / F64(fy)
        R, t = rot(pose), pose[4:]
        voxel = F64(self.voxel)
        hv = voxel * F64(0.5)
        for k in range(-2 * self.trunc, 2 * self.trunc + 1):
            z = d.astype(F64) + F64(k) * hv
            front = z > 0
            X, Y = ax * z, ay * z
            with np.errstate(invalid="ignore", over="ignore"):
                fl = np.stack([np.floor((((R[i][0] * X + R[i][1] * Y) + R[i][2] * z) + t[i]) / voxel) for i in range(3)], axis=-1)
                inside = ((fl >= -HALF) & (fl < HALF)).all(axis=-1)
            self.dropped_range += int((front & ~inside).sum())
            cells = fl[front & inside].astype(np.int64) + HALF
            for key in _pack_biased(cells).tolist():           # in arrival order: the dict's order is the schedule's
                self.records.setdefault(key, [self.real(0.0), 0, 0, 0, 0, 0])
        return self

    def integrate(self, depth, rgb, f, c, pose):
        """``rgb`` [h,w,3] float32 in 0..1."""
        depth = np.asarray(depth, F32)
        h, w = depth.shape
        pose = np.asarray(pose, F64)
        if not np.isfinite(pose).all() or not self.records:
            return self
        keys = np.array(list(self.records), np.uint64)
        cells = _biased(keys) - HALF
        R, t = rot(pose), pose[4:]
        voxel = F64(self.voxel)
        D = [(cells[:, j].astype(F64) + F64(0.5)) * voxel - t[j] for j in range(3)]
        X = [(R[0][j] * D[0] + R[1][j] * D[1]) + R[2][j] * D[2] for j in range(3)]
        z = X[2]
        fx, fy, cx, cy = (F64(F32(v)) for v in (f[0], f[1], c[0], c[1]))
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            u, v = (fx * X[0]) / z + cx, (fy * X[1]) / z + cy
            ok = (z > 0) & (u >= 0) & (u < w) & (v >= 0) & (v < h)
        col = np.where(ok, np.floor(np.where(ok, u, 0.0)), 0).astype(np.int64)
        row = np.where(ok, np.floor(np.where(ok, v, 0.0)), 0).astype(np.int64)
        d = depth[row, col]
        with np.errstate(invalid="ignore"):
            ok &= np.isfinite(d) & (d >= self.near) & (d <= self.far)
            T = self.real(F64(self.trunc) * voxel)
            sdf = (np.where(ok, d, F32(0.0)).astype(F64) - z).astype(self.real)
            upd = ok & (sdf >= -T)
            inc = np.minimum(sdf, T) / T
            coloured = upd & (sdf <= T)
        colour = rgb_bytes(np.asarray(rgb, F32)[row, col])
        for i in np.nonzero(upd)[0].tolist():
            rec = self.records[int(keys[i])]
            rec[0] = self.real(rec[0] + inc[i])
            rec[1] += 1
            if coloured[i]:
                rec[2] += int(colour[i, 0]); rec[3] += int(colour[i, 1]); rec[4] += int(colour[i, 2])
                rec[5] += 1
        self.updates += int(upd.sum())
        return self

    def frame(self, depth, rgb, f, c, pose, order=None):
        return self.allocate(depth, f, c, pose, order).integrate(depth, rgb, f, c, pose)

    def stats(self):
        return {"occupied": len(self.records), "dropped_range": self.dropped_range, "dropped_full": 0, "updates": self.updates}

    # ---- per trajectory ----------------------------------------------------------------------------------------------------------
    def extract(self, min_frames=1):
        """{"keys" uint64 [m] ascending, "xyz" [m,3], "rgba" uint8 [m,4], "vertices" uint8 [m,16] (float32 volumes only),
        "triangles" int32 [2q,3], "quads" int64 [q,4] vertex indices, "quads_dropped", "raw_quads" uint64 [q + dropped, 5] the
        five-word records of m4d_tsdf_extract_faces}: one vertex per sign-changing cell, the quads ordered by (owner key, axis) and
        split along their (0,2) diagonal."""
        real = self.real
        keys = np.array(sorted(self.records), np.uint64)
        m = len(keys)
        empty = {"keys": keys[:0], "xyz": np.zeros((0, 3), real), "rgba": np.zeros((0, 4), np.uint8),
                 "vertices": np.zeros((0, 16), np.uint8), "triangles": np.zeros((0, 3), np.int32),
                 "quads": np.zeros((0, 4), np.int64), "quads_dropped": 0, "raw_quads": np.zeros((0, 5), np.uint64)}
        if not m:
            return empty
        recs = [self.records[int(k)] for k in keys]
        S = np.array([r[0] for r in recs], real)
        n = np.array([r[1] for r in recs], np.int64)
        sums = np.array([r[2:6] for r in recs], np.int64)
        live = n >= int(min_frames)
        with np.errstate(invalid="ignore", divide="ignore"):
            Dv = S / n.astype(real)
        cells = _biased(keys)

        def find(want, ok):
            """Indices into keys of the biased cells ``want`` [..,3] where ``ok``; (index, found)."""
            k = _pack_biased(np.where(ok[..., None], want, 0))
            at = np.minimum(np.searchsorted(keys, k), m - 1)
            return at, ok & (keys[at] == k)

        # vertices
        corner = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)], np.int64)
        want = cells[:, None, :] + corner[None]
        at, found = find(want, (want <= CELL_MAX).all(axis=-1))
        valid = (found & live[at]).all(axis=1)
        D = Dv[at]
        inside = D < 0
        n_in = inside.sum(axis=1)
        emit = valid & (n_in > 0) & (n_in < 8)
        ve = np.nonzero(emit)[0]
        D, inside, at_e = D[ve], inside[ve], at[ve]
        sum_ = np.zeros((len(ve), 3), real)
        count = np.zeros(len(ve), np.int64)
        for axis in range(3):
            for c in range(8):
                if c & (1 << axis):
                    continue
                c2 = c | (1 << axis)
                cross = inside[:, c] != inside[:, c2]
                with np.errstate(invalid="ignore", divide="ignore"):
                    tpar = D[:, c] / (D[:, c] - D[:, c2])
                for j in range(3):
                    add = tpar if j == axis else np.full(len(ve), real((c >> j) & 1))
                    sum_[:, j] = np.where(cross, sum_[:, j] + add, sum_[:, j])
                count += cross
        local = sum_ / count.astype(real)[:, None]
        voxel = F64(self.voxel)
        xyz = ((((cells[ve] - HALF).astype(F64) + F64(0.5)) + local.astype(F64)) * voxel).astype(real)
        tot = sums[at_e].sum(axis=1)                           # [m,4]: sr, sg, sb, nc over the eight corners
        nc = tot[:, 3]
        rgba = np.zeros((len(ve), 4), np.uint8)
        for j in range(3):
            rgba[:, j] = np.where(nc > 0, (2 * tot[:, j] + nc) // np.maximum(2 * nc, 1), 0)
        rgba[:, 3] = np.minimum(255, n[at_e].min(axis=1))
        vkeys = keys[ve]
        vertices = np.zeros((len(ve), 16), np.uint8)
        if real is F32:
            vertices[:, :12] = np.ascontiguousarray(xyz).view(np.uint8).reshape(-1, 12)
            vertices[:, 12:] = rgba

        # faces
        quads = []
        for a in range(3):
            b2, c2 = (a + 1) % 3, (a + 2) % 3
            e = np.eye(3, dtype=np.int64)
            ok = live & (cells[:, a] < CELL_MAX) & (cells[:, b2] >= 1) & (cells[:, c2] >= 1)
            at_n, found_n = find(cells + e[a], ok)
            ok = found_n & live[at_n]
            ok &= (Dv < 0) != (Dv[at_n] < 0)
            own = np.nonzero(ok)[0]
            ring = np.stack([_pack_biased(cells[own] - off) for off in (0 * e[a], e[b2], e[b2] + e[c2], e[c2])], axis=1)
            ring = np.where((Dv[own] < 0)[:, None], ring, ring[:, ::-1])
            quads.append((keys[own], np.full(len(own), a, np.int64), ring, np.where(Dv[own] < 0, a, a | 4).astype(np.uint64)))
        owner = np.concatenate([q[0] for q in quads])
        axis = np.concatenate([q[1] for q in quads])
        ring = np.concatenate([q[2] for q in quads])
        order = np.lexsort((axis, owner))
        ring = ring[order]
        raw_quads = np.concatenate([np.concatenate([q[3] for q in quads])[order][:, None], ring], axis=1)
        if len(vkeys):
            idx = np.minimum(np.searchsorted(vkeys, ring), len(vkeys) - 1)
            have = (vkeys[idx] == ring).all(axis=1)
        else:
            idx, have = np.zeros(ring.shape, np.int64), np.zeros(len(ring), bool)
        q = idx[have].astype(np.int64)
        tri = np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], axis=1).reshape(-1, 3).astype(np.int32)
        return {"keys": vkeys, "xyz": xyz, "rgba": rgba, "vertices": vertices, "triangles": tri, "quads": q,
                "quads_dropped": int((~have).sum()), "raw_quads": raw_quads}


# ---- mesh properties the tests share ---------------------------------------------------------------------------------------------
def edge_counts(quads):
    """The undirected edges of the quads -> how many faces share each (a dict)."""
    q = np.asarray(quads, np.int64)
    e = np.concatenate([np.stack([q[:, i], q[:, (i + 1) % 4]], axis=1) for i in range(4)])
    e = np.sort(e, axis=1)
    uniq, cnt = np.unique(e, axis=0, return_counts=True)
    return uniq, cnt


def quad_normals(xyz, quads):
    """The (unnormalised) normals of the quads: the cross product of their diagonals."""
    p = np.asarray(xyz, F64)[np.asarray(quads, np.int64)]
    return np.cross(p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]), p.mean(axis=1)


# ---- the scenes of the tests -----------------------------------------------------------------------------------------------------
def quat_from_matrix(R):
    """A rotation matrix -> (w, x, y, z), w >= 0."""
    R = np.asarray(R, F64)
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    if w > 1e-6:
        return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
    i = int(np.argmax(np.diag(R)))
    j, k = (i + 1) % 3, (i + 2) % 3
    s = np.sqrt(max(0.0, 1.0 + R[i, i] - R[j, j] - R[k, k])) * 2.0
    q = np.zeros(4)
    q[0] = (R[k, j] - R[j, k]) / s
    q[1 + i] = s / 4.0
    q[1 + j] = (R[j, i] + R[i, j]) / s
    q[1 + k] = (R[k, i] + R[i, k]) / s
    return q / np.linalg.norm(q)


def look_at_pose(eye, target=(0.0, 0.0, 0.0)):
    """The camera-to-world pose (7 float64) of a camera at ``eye`` whose +z axis points at ``target``."""
    eye = np.asarray(eye, F64)
    zc = np.asarray(target, F64) - eye
    zc /= np.linalg.norm(zc)
    up = np.array([0.0, 1.0, 0.0]) if abs(zc[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    xc = np.cross(up, zc)
    xc /= np.linalg.norm(xc)
    yc = np.cross(zc, xc)
    return np.concatenate([quat_from_matrix(np.stack([xc, yc, zc], axis=1)), eye])


def _rays(pose, f, c, h, w):
    R = np.array(rot(pose), F64)
    col, row = np.meshgrid(np.arange(w, dtype=F64), np.arange(h, dtype=F64))
    dirs = np.stack([((col + 0.5) - F64(c[0])) / F64(f[0]), ((row + 0.5) - F64(c[1])) / F64(f[1]), np.ones((h, w))], axis=-1)
    return dirs @ R.T, np.asarray(pose, F64)[4:]


def render_sphere(pose, f, c, h, w, radius=1.0):
    """z-depth [h,w] float32 of the sphere of ``radius`` at the origin, NaN where the ray misses it."""
    dw, o = _rays(pose, f, c, h, w)
    a = (dw * dw).sum(-1)
    b = (dw * o).sum(-1)
    disc = b * b - a * (o @ o - radius * radius)
    with np.errstate(invalid="ignore"):
        z = (-b - np.sqrt(disc)) / a
    return np.where(disc > 0, z, np.nan).astype(F32)


def render_plane(pose, f, c, h, w, normal, offset):
    """z-depth [h,w] float32 of the plane normal . X = offset (world frame)."""
    dw, o = _rays(pose, f, c, h, w)
    normal = np.asarray(normal, F64)
    return ((offset - normal @ o) / (dw @ normal)).astype(F32)


SPHERE = dict(h=48, w=48, f=(48.0, 48.0), c=(24.0, 24.0), voxel=0.125, trunc=2, near=0.5, far=10.0)
SPHERE_DIRS = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)]


def sphere_frames():
    """The 26 (depth, rgb, pose) of the unit sphere seen from 3 m away along {-1,0,1}^3 \\ 0."""
    out = []
    for i, d in enumerate(SPHERE_DIRS):
        eye = 3.0 * np.asarray(d, F64) / np.linalg.norm(d)
        pose = look_at_pose(eye)
        depth = render_sphere(pose, SPHERE["f"], SPHERE["c"], SPHERE["h"], SPHERE["w"])
        rgb = np.random.default_rng(100 + i).random((SPHERE["h"], SPHERE["w"], 3)).astype(F32)
        out.append((depth, rgb, pose))
    return out


PLANE = dict(h=24, w=32, voxel=0.25, trunc=3, near=1.0, far=80.0)
PLANE_NORMAL = np.array([0.3, -0.2, 1.0]) / np.linalg.norm([0.3, -0.2, 1.0])
PLANE_OFFSET = 3.0 * PLANE_NORMAL[2]                           # the plane passes through (0, 0, 3)
PLANE_F, PLANE_C = (27.3, 26.1), (15.7, 12.4)                  # non-dyadic, off-centre


def plane_poses(n=4):
    """``n`` camera-to-world poses: a few degrees of rotation and decimetres of translation per frame, the first the identity."""
    poses = []
    for k in range(n):
        ang = np.deg2rad(np.array([1.5, -2.5, 1.0]) * k)
        q = np.array([1.0, ang[0] / 2, ang[1] / 2, ang[2] / 2])
        q /= np.linalg.norm(q)
        poses.append(np.concatenate([q, np.array([0.21, -0.13, 0.09]) * k]))
    return poses


def plane_frames(f=PLANE_F, c=PLANE_C, n=4, seed=7):
    out = []
    for k, pose in enumerate(plane_poses(n)):
        depth = render_plane(pose, f, c, PLANE["h"], PLANE["w"], PLANE_NORMAL, PLANE_OFFSET)
        rgb = np.random.default_rng(seed + k).random((PLANE["h"], PLANE["w"], 3)).astype(F32)
        out.append((depth, rgb, pose))
    return out


def fuse(frames, f, c, voxel, trunc, near, far, exact=False):
    vol = TsdfVolume(voxel, trunc, near, far, exact=exact)
    for depth, rgb, pose in frames:
        vol.frame(depth, rgb, f, c, pose)
    return vol
