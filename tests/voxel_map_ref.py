"""The voxel map of include/m4depth_hip.h (m4d_voxel_map_integrate / m4d_voxel_map_extract) restated in numpy: a dict keyed by
the packed key, every accumulator a Python integer, the output sorted by key.  Nothing here knows about slots, probing or the
3/4 rule: a map that fits its table equals this one bit for bit."""
import numpy as np

HALF = 1 << 20
EMPTY = (1 << 64) - 1


def axis(x, voxel):
    """One float32 coordinate -> (voxel index, offset bin 0..255), or None when the index leaves [-2^20, 2^20)."""
    g = np.float64(np.float32(x)) / np.float64(np.float32(voxel))
    fl = np.floor(g)
    if not (fl >= -HALF and fl < HALF):
        return None
    return int(fl), min(int(np.floor((g - fl) * np.float64(256.0))), 255)


def pack(ix, iy, iz):
    return ((int(ix) + HALF) << 42) | ((int(iy) + HALF) << 21) | (int(iz) + HALF)


def unpack(key):
    return tuple(((int(key) >> sh) & 0x1FFFFF) - HALF for sh in (42, 21, 0))


class VoxelMap:
    """``records``: key -> [n, sx, sy, sz, sr, sg, sb, last_stamp, frames]; ``observations`` / ``dropped_range`` as the device
    counts them (a map that fits has ``dropped_full`` 0 and ``occupied`` = len(records))."""

    def __init__(self, voxel):
        self.voxel = np.float32(voxel)
        assert np.isfinite(self.voxel) and self.voxel > 0
        self.records = {}
        self.observations = self.dropped_range = 0

    def integrate(self, vertices, stamp):
        """``vertices``: [n,16] uint8 as m4d_depth_cloud writes them; ``stamp`` >= 1."""
        assert stamp >= 1
        raw = np.ascontiguousarray(vertices, np.uint8).reshape(-1, 16)
        xyz = raw[:, :12].copy().view(np.float32).reshape(-1, 3)
        for p, c in zip(xyz, raw[:, 12:15]):
            self.observations += 1
            cells = [axis(v, self.voxel) if np.isfinite(v) else None for v in p]
            if not np.isfinite(p).all() or any(a is None for a in cells):
                self.dropped_range += 1
                continue
            rec = self.records.setdefault(pack(*(a[0] for a in cells)), [0] * 9)
            rec[0] += 1
            for i in range(3):
                rec[1 + i] += cells[i][1]
                rec[4 + i] += int(c[i])
            if rec[7] < stamp:                               # old = max-exchange(last_stamp, stamp); old < stamp: a new frame
                rec[7] = stamp
                rec[8] += 1
        return self

    def extract(self, min_frames=1):
        """(keys uint64 [m] ascending, vertices uint8 [m,16]) of the voxels with frames >= min_frames."""
        keys = sorted(k for k, r in self.records.items() if r[8] >= min_frames)
        out = np.zeros((len(keys), 16), np.uint8)
        voxel = np.float64(self.voxel)
        for row, key in zip(out, keys):
            n, sx, sy, sz, sr, sg, sb, _, frames = self.records[key]
            pos = [np.float32((np.float64(i) + (np.float64(s) / np.float64(n) + np.float64(0.5)) / np.float64(256.0)) * voxel)
                   for i, s in zip(unpack(key), (sx, sy, sz))]
            row[:12] = np.array(pos, np.float32).view(np.uint8)
            row[12:15] = [(2 * s + n) // (2 * n) for s in (sr, sg, sb)]
            row[15] = min(frames, 255)
        return np.array(keys, np.uint64), out

    def stats(self):
        return {"observations": self.observations, "dropped_range": self.dropped_range, "dropped_full": 0,
                "occupied": len(self.records)}


def vertices_of(xyz, rgb):
    """float32 [n,3] + uint8 [n,3] -> the 16-byte vertices of a cloud (alpha 255)."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    rgba = np.concatenate([np.asarray(rgb, np.uint8).reshape(-1, 3), np.full((len(xyz), 1), 255, np.uint8)], axis=1)
    return np.concatenate([xyz.view(np.uint8).reshape(-1, 12), rgba], axis=1)
