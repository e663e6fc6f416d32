"""numpy restatement of m4d_depth_views (include/m4depth_hip.h, "Multi-view depth check"), operation by operation.

Everything is elementwise numpy on float32 / float64 arrays: explicit sums in the header's order, no ``@`` / ``einsum`` / ``dot``
(a BLAS may fuse or reorder).  Besides ``n_views`` it returns what tests need to place thresholds: per (view, pixel) whether the
view tested the pixel and the two residuals the kernel compares.  Also the synthetic scene the tests share: an analytic plane
seen from cameras that move and turn a little more every frame."""
import numpy as np

from pose_ref import rot

F = np.float32
D = np.float64
QNAN_BITS = np.uint32(0x7FC00000)


def relative(pose_k, pose_c):
    """(Rr, tr): Rr = R(qk)^T R(qc), tr = R(qk)^T (tc - tk), sums left to right."""
    with np.errstate(invalid="ignore", over="ignore"):
        rk, rc = rot(pose_k[:4]), rot(pose_c[:4])
        rr = tuple(tuple((rk[0][i] * rc[0][j] + rk[1][i] * rc[1][j]) + rk[2][i] * rc[2][j] for j in range(3)) for i in range(3))
        d = tuple(D(pose_c[4 + i]) - D(pose_k[4 + i]) for i in range(3))
        tr = tuple((rk[0][i] * d[0] + rk[1][i] * d[1]) + rk[2][i] * d[2] for i in range(3))
    return rr, tr


def check_view(depth, f, c, rr, tr, ring):
    """One view over one sample's map: depth, ring [h,w] float32, f / c [2] float32 -> (tested bool, r_px2 float64 =
    (pu-col)^2 + (pv-row)^2, r_z float64 = |Yc.z - d|, zc float64 = d), residuals NaN where the view does not test the pixel
    or Yc.z <= 0 (``back`` false)."""
    h, w = depth.shape
    fx, fy, cx, cy = F(f[0]), F(f[1]), F(c[0]), F(c[1])
    fxd, fyd, cxd, cyd = D(fx), D(fy), D(cx), D(cy)
    rows, cols = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    with np.errstate(all="ignore"):
        valid = np.isfinite(depth) & (depth > F(0.0))
        d = np.where(valid, depth, F(1.0)).astype(F)
        xc = ((((cols.astype(F) + F(0.5)) - cx) / fx) * d).astype(D)
        yc = ((((rows.astype(F) + F(0.5)) - cy) / fy) * d).astype(D)
        zc = d.astype(D)
        X = [((rr[i][0] * xc + rr[i][1] * yc) + rr[i][2] * zc) + tr[i] for i in range(3)]
        z = X[2]
        u = ((fxd * X[0]) / z + cxd) - D(0.5)
        v = ((fyd * X[1]) / z + cyd) - D(0.5)
        inside = valid & (z > 0) & (u >= 0) & (u <= D(w - 1)) & (v >= 0) & (v <= D(h - 1))
        u32 = np.where(inside, u, D(0.0)).astype(F)
        v32 = np.where(inside, v, D(0.0)).astype(F)
        x0 = np.minimum(np.floor(u32).astype(np.int64), w - 2)
        y0 = np.minimum(np.floor(v32).astype(np.int64), h - 2)
        ax, ay = u32 - x0.astype(F), v32 - y0.astype(F)
        tl, tr_, bl, br = ring[y0, x0], ring[y0, x0 + 1], ring[y0 + 1, x0], ring[y0 + 1, x0 + 1]
        taps = np.ones(depth.shape, bool)
        for t in (tl, tr_, bl, br):
            taps &= np.isfinite(t) & (t > F(0.0))
        tested = inside & taps
        top = (tl + ax * (tr_ - tl)).astype(F)
        bot = (bl + ax * (br - bl)).astype(F)
        dk = (top + ay * (bot - top)).astype(F).astype(D)
        e = [(((u + D(0.5)) - cxd) / fxd) * dk - tr[0], (((v + D(0.5)) - cyd) / fyd) * dk - tr[1], dk - tr[2]]
        Y = [(rr[0][i] * e[0] + rr[1][i] * e[1]) + rr[2][i] * e[2] for i in range(3)]
        back = tested & (Y[2] > 0)
        du = (((fxd * Y[0]) / Y[2] + cxd) - D(0.5)) - cols.astype(D)
        dv = (((fyd * Y[1]) / Y[2] + cyd) - D(0.5)) - rows.astype(D)
        r_px2 = np.where(back, du * du + dv * dv, np.nan)
        r_z = np.where(back, np.abs(Y[2] - zc), np.nan)
    return tested, r_px2, r_z, zc


def depth_views(depth, cam_f, cam_c, pose, ring_depth, ring_pose, age_in, head, views, reset=None, force_all=False,
                tol_px=1.0, tol_rel=0.01, min_views=None):
    """One call.  depth [b,h,w] float32, pose [b,7] float64, ring_depth [(K+1),b,h,w], ring_pose [(K+1),b,7], age_in [b].
    The ring arrays are updated in place (slot ``head``).  Returns a dict: n_views [b,h,w] uint8, depth_f [b,h,w] float32,
    age_out [b] int32, and per view j-1 (views not looked at: all False / NaN) tested [K,b,h,w] bool, r_px2, r_z [K,b,h,w]
    float64, confirmed [K,b,h,w] bool, zc [b,h,w] float64."""
    depth = np.asarray(depth, F)
    b, h, w = depth.shape
    K = int(views)
    min_views = min(2, K) if min_views is None else int(min_views)
    tol2, rel = D(F(tol_px)) * D(F(tol_px)), D(F(tol_rel))
    out = {"n_views": np.zeros((b, h, w), np.uint8), "age_out": np.zeros(b, np.int32),
           "tested": np.zeros((K, b, h, w), bool), "confirmed": np.zeros((K, b, h, w), bool),
           "r_px2": np.full((K, b, h, w), np.nan), "r_z": np.full((K, b, h, w), np.nan), "zc": np.zeros((b, h, w), D)}
    for s in range(b):
        fresh = force_all or (reset is not None and bool(reset[s]))
        a = 0 if fresh else min(max(int(age_in[s]), 0), K)
        out["age_out"][s] = min(a + 1, K)
        for j in range(1, a + 1):
            slot = (head - j) % (K + 1)
            rr, tr = relative(ring_pose[slot, s], pose[s])
            tested, r_px2, r_z, zc = check_view(depth[s], cam_f[s], cam_c[s], rr, tr, ring_depth[slot, s])
            with np.errstate(invalid="ignore"):
                confirmed = tested & (r_px2 < tol2) & (r_z < rel * zc)
            out["tested"][j - 1, s], out["r_px2"][j - 1, s], out["r_z"][j - 1, s] = tested, r_px2, r_z
            out["confirmed"][j - 1, s] = confirmed
            out["zc"][s] = zc
            out["n_views"][s] += confirmed.astype(np.uint8)
    keep = out["n_views"] >= min_views
    out["depth_f"] = np.where(keep, depth.view(np.uint32), QNAN_BITS).astype(np.uint32).view(F)
    ring_depth[head] = depth
    ring_pose[head] = pose
    return out


class State:
    """Host-side twin of network_ops.depth_views_state: rings (filled with NaN), ages, head."""

    def __init__(self, b, h, w, views):
        self.views = int(views)
        self.ring_depth = np.full((views + 1, b, h, w), np.nan, F)
        self.ring_pose = np.full((views + 1, b, 7), np.nan, D)
        self.age = np.zeros(b, np.int32)
        self.head = 0

    def step(self, depth, cam_f, cam_c, pose, **kw):
        out = depth_views(depth, cam_f, cam_c, pose, self.ring_depth, self.ring_pose, self.age, self.head, self.views, **kw)
        self.age = out["age_out"].copy()
        self.head = (self.head + 1) % (self.views + 1)
        return out


# ---- the scene -----------------------------------------------------------------------------------------------------------------
H, W, N_POSES = 37, 53, 6
PLANE_N = np.array([0.12, -0.2, 1.0]) / np.linalg.norm([0.12, -0.2, 1.0])     # n . X = d0 in the world (= camera 0) frame
PLANE_D0 = 9.0


def scene_poses(n=N_POSES, scale=1.0):
    """Camera-to-world poses [n,7] float64: translation and rotation grow with the frame index; unit quaternions."""
    poses = np.zeros((n, 7), D)
    axis = np.array([0.3, -0.8, 0.52]) / np.linalg.norm([0.3, -0.8, 0.52])
    for k in range(n):
        ang = np.deg2rad(1.1 * k * scale)
        q = np.concatenate([[np.cos(ang / 2)], axis * np.sin(ang / 2)])
        poses[k, :4] = q / np.sqrt(np.sum(q * q))
        poses[k, 4:] = np.array([0.22, -0.12, 0.15]) * k * scale
    return poses


def render_plane(pose, f, c, h=H, w=W):
    """Depth [h,w] float32 of the plane from a camera: z with n . (R (x z, y z, z) + t) = d0, in float64, rounded once."""
    r = np.array(rot(pose[:4]), D)
    rows, cols = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    x = ((cols + 0.5) - D(F(c[0]))) / D(F(f[0]))
    y = ((rows + 0.5) - D(F(c[1]))) / D(F(f[1]))
    ray = [r[i, 0] * x + r[i, 1] * y + r[i, 2] for i in range(3)]
    den = PLANE_N[0] * ray[0] + PLANE_N[1] * ray[1] + PLANE_N[2] * ray[2]
    z = (PLANE_D0 - np.sum(PLANE_N * pose[4:])) / den
    return z.astype(F)


def smooth_noise(seed, shape, amp):
    """Multiplicative smooth noise 1 + amp * g, g a sum of a few low-frequency sinusoids in [-1, 1]."""
    rng = np.random.default_rng(seed)
    h, w = shape
    rows, cols = np.meshgrid(np.arange(h) / h, np.arange(w) / w, indexing="ij")
    g = np.zeros(shape)
    for _ in range(4):
        fr, fc = rng.uniform(0.5, 3.0, 2)
        g += np.sin(2 * np.pi * (fr * rows + fc * cols) + rng.uniform(0, 2 * np.pi))
    return (1.0 + amp * g / 4.0)


def scene(cam, n=N_POSES, noise=None, h=H, w=W, scale=1.0):
    """(maps [n,b,h,w] float32, poses [n,b,7] float64) of the plane for the b cameras of ``cam`` {f, c} [b,2]; every sample
    follows the same path.  ``noise`` = (seed, amplitude): smooth multiplicative noise, a different field per map."""
    b = len(cam["f"])
    poses = scene_poses(n, scale)
    maps = np.stack([np.stack([render_plane(poses[k], cam["f"][s], cam["c"][s], h, w) for s in range(b)]) for k in range(n)])
    if noise is not None:
        for k in range(n):
            for s in range(b):
                maps[k, s] = (maps[k, s] * smooth_noise(noise[0] + 31 * k + s, (h, w), noise[1])).astype(F)
    return maps, np.ascontiguousarray(np.broadcast_to(poses[:, None], (n, b, 7)))
