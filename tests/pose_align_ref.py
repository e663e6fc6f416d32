"""A numpy restatement of the pose refinement of include/m4depth_hip.h ("Pose refinement"), with a dtype argument.

``dtype=np.float64``: every per-pixel quantity, the pyramid and the pose in double -- the reference.  ``dtype=np.float32``: the
per-pixel arithmetic in float32 in the operation order of csrc/m4d_align.hip (one rounding per operation, the pose rounded to
float32 before the query), products and sums in double -- what a float32 evaluation of the definition costs.  The distance
between the two is the yardstick of tests/test_gpu_pose_align.py.

Test infrastructure, not a fallback: the product has no CPU form of this.
"""
import numpy as np

F = np.float32
NEAR_HUBER = 1e-4          # ``near``: |(|r| - huber)| below this, or
NEAR_BORDER = 1e-3         # a query within this many pixels of the validity border
NEAR_CELL = 2e-5           # ``near_cell``: a query this close to a bilinear cell boundary (the gradient is one-sided there)


# ---- pose algebra (double) -----------------------------------------------------------------------------------------------------
def quat_matrix(q):
    w, x, y, z = (float(v) for v in q)
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]], np.float64)


def unit(q):
    q = np.asarray(q, np.float64)
    return q / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])


def matrix_quat(R):
    """The unit quaternion (w >= 0) of a rotation matrix, the branches of the kernel."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0.0:
        k = np.sqrt(tr + 1.0) * 2.0
        q = [0.25 * k, (R[2, 1] - R[1, 2]) / k, (R[0, 2] - R[2, 0]) / k, (R[1, 0] - R[0, 1]) / k]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        k = np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2.0
        q = [(R[2, 1] - R[1, 2]) / k, 0.25 * k, (R[0, 1] + R[1, 0]) / k, (R[0, 2] + R[2, 0]) / k]
    elif R[1, 1] > R[2, 2]:
        k = np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2.0
        q = [(R[0, 2] - R[2, 0]) / k, (R[0, 1] + R[1, 0]) / k, 0.25 * k, (R[1, 2] + R[2, 1]) / k]
    else:
        k = np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2.0
        q = [(R[1, 0] - R[0, 1]) / k, (R[0, 2] + R[2, 0]) / k, (R[1, 2] + R[2, 1]) / k, 0.25 * k]
    q = unit(q)
    return -q if q[0] < 0.0 else q


def rodrigues(w):
    w = np.asarray(w, np.float64)
    t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    t = np.sqrt(t2)
    if t < 1e-4:
        ka, kb = 1.0 - t2 / 6.0, 0.5 - t2 / 24.0
    else:
        ka, kb = np.sin(t) / t, (1.0 - np.cos(t)) / t2
    return np.array([[1.0 - kb * (w[1] * w[1] + w[2] * w[2]), kb * w[0] * w[1] - ka * w[2], kb * w[0] * w[2] + ka * w[1]],
                     [kb * w[0] * w[1] + ka * w[2], 1.0 - kb * (w[0] * w[0] + w[2] * w[2]), kb * w[1] * w[2] - ka * w[0]],
                     [kb * w[0] * w[2] - ka * w[1], kb * w[1] * w[2] + ka * w[0], 1.0 - kb * (w[0] * w[0] + w[1] * w[1])]])


def rotation_angle(Ra, Rb):
    """The angle of Ra Rb^T."""
    qa, qb = matrix_quat(Ra), matrix_quat(Rb)
    rw = qa @ qb
    rv = -qa[0] * qb[1:] + qb[0] * qa[1:] - np.cross(qa[1:], qb[1:])
    return 2.0 * np.arctan2(np.linalg.norm(rv), abs(rw))


def begin(rot, trans):
    """(A, a) = (R^T, -R^T t) of the given motion (float32 ``rot`` [4], ``trans`` [3]), in double."""
    R = quat_matrix(unit(np.asarray(rot, np.float64)))
    return R.T.copy(), -(R.T @ np.asarray(trans, np.float64))


def given_motion(A, a):
    """float32 (rot, trans) of the network's convention for a previous-to-current pose (A, a)."""
    return matrix_quat(A.T).astype(F), (-(A.T @ a)).astype(F)


# ---- images --------------------------------------------------------------------------------------------------------------------
def box_level(img, dtype):
    """One level of m4d_image_pyramid_box: ((a + b) + (c + d)) * 0.25, a, b on the upper row."""
    x = np.asarray(img, dtype)
    return ((x[0::2, 0::2] + x[0::2, 1::2]) + (x[1::2, 0::2] + x[1::2, 1::2])) * dtype(0.25)


def level_image(img, s, dtype):
    x = np.asarray(img, dtype)
    while s > 1:
        x, s = box_level(x, dtype), s // 2
    return x


def grey(x, dtype):
    return ((x[..., 0] + x[..., 1]) + x[..., 2]) / dtype(3.0)


# ---- one iteration -------------------------------------------------------------------------------------------------------------
def pixel_terms(cur, prev, Dp, f, c, A, a, s, dtype):
    """Everything per level pixel of one sample at stride ``s`` for the pose (A, a): a dict of [h,w] maps (``ok``, ``r``, ``J``
    [h,w,6], the query ``qx``, ``qy`` and alphas).  ``cur`` / ``prev`` [H,W,3] and ``Dp`` [H,W] are the float32 inputs."""
    T = dtype
    H, W = Dp.shape
    hl, wl = H // s, W // s
    Ic, Ip = grey(level_image(cur, s, T), T), grey(level_image(prev, s, T), T)
    fx, fy, cx, cy = T(f[0]) / T(s), T(f[1]) / T(s), T(c[0]) / T(s), T(c[1]) / T(s)
    Af, af = np.asarray(A, np.float64).astype(T), np.asarray(a, np.float64).astype(T)
    draw = np.asarray(Dp, F)[s // 2::s, s // 2::s].astype(T)
    assert draw.shape == (hl, wl)
    d = np.fmin(np.fmax(draw, T(0.01)), T(200.0))
    jj, ii = np.meshgrid(np.arange(hl).astype(T), np.arange(wl).astype(T), indexing="ij")
    mx, my = (ii + T(0.5)) - cx, (jj + T(0.5)) - cy
    ux, uy = mx / fx, my / fy
    X0, X1, X2 = ux * d, uy * d, d
    # m4d_photo_matrix: M = diag(fx, fy, 1) [A | a]; m4d_photo_query: sequential dot products
    Mm = [[fx * Af[0, k] for k in range(3)] + [fx * af[0]], [fy * Af[1, k] for k in range(3)] + [fy * af[1]],
          [Af[2, k] for k in range(3)] + [af[2]]]
    with np.errstate(all="ignore"):
        pr = [((Mm[r][0] * X0 + Mm[r][1] * X1) + Mm[r][2] * X2) + Mm[r][3] * T(1.0) for r in range(3)]
        px, py = pr[0] / pr[2], pr[1] / pr[2]
        qy, qx = jj + (py - my), ii + (px - mx)

        def axis(q, size):
            fl = np.fmin(np.fmax(T(0.0), np.floor(q)), T(size - 2))
            return fl.astype(np.int64), np.fmin(np.fmax(T(0.0), q - fl), T(1.0))
        y0, ay = axis(qy, hl)
        x0, ax = axis(qx, wl)
        ok = (pr[2] > 0) & (qx >= 0) & (qx <= T(wl - 1)) & (qy >= 0) & (qy <= T(hl - 1)) & np.isfinite(draw)
        Yx = ((Af[0, 0] * X0 + Af[0, 1] * X1) + Af[0, 2] * X2) + af[0]
        Yy = ((Af[1, 0] * X0 + Af[1, 1] * X1) + Af[1, 2] * X2) + af[1]
        Yz = ((Af[2, 0] * X0 + Af[2, 1] * X1) + Af[2, 2] * X2) + af[2]
        tl, tr, bl, br = Ic[y0, x0], Ic[y0, x0 + 1], Ic[y0 + 1, x0], Ic[y0 + 1, x0 + 1]
        top = ax * (tr - tl) + tl
        bot = ax * (br - bl) + bl
        r = (ay * (bot - top) + top) - Ip
        gx = (T(1.0) - ay) * (tr - tl) + ay * (br - bl)
        gy = (T(1.0) - ax) * (bl - tl) + ax * (br - tr)
        gfx, gfy = gx * fx, gy * fy
        J0, J1 = gfx / Yz, gfy / Yz
        J2 = -((gfx * Yx + gfy * Yy) / (Yz * Yz))
        J = np.stack([J0, J1, J2, Yy * J2 - Yz * J1, Yz * J0 - Yx * J2, Yx * J1 - Yy * J0], axis=-1)
    return dict(ok=ok, r=r, J=J, qx=qx, qy=qy, ax=ax, ay=ay, finite=np.isfinite(draw), hl=hl, wl=wl)


def sums(cur, prev, Dp, f, c, A, a, s, huber, dtype):
    """H [6,6], b [6], cost, N of one iteration, and ``near`` / ``near_cell``: the pixels at a discontinuity of the definition,
    where float32 and float64 may take different branches."""
    T = dtype
    p = pixel_terms(cur, prev, Dp, f, c, A, a, s, T)
    ok, hl, wl = p["ok"], p["hl"], p["wl"]
    r = p["r"][ok]
    J = p["J"][ok].astype(np.float64)
    with np.errstate(all="ignore"):
        ar = np.abs(r)
        wh = np.where(ar <= T(huber), T(1.0), T(huber) / ar).astype(np.float64)
    rd = r.astype(np.float64)
    Hm = np.zeros((6, 6))
    bv = np.zeros(6)
    for i in range(6):
        wj = wh * J[:, i]
        for k in range(i, 6):
            Hm[i, k] = Hm[k, i] = np.sum(wj * J[:, k])
        bv[i] = np.sum(wj * rd)
    cost = float(np.sum(wh * rd * rd))
    qx, qy = p["qx"].astype(np.float64), p["qy"].astype(np.float64)
    with np.errstate(all="ignore"):
        border = p["finite"] & ((np.abs(qx) < NEAR_BORDER) | (np.abs(qx - (wl - 1)) < NEAR_BORDER) | (np.abs(qy) < NEAR_BORDER)
                                | (np.abs(qy - (hl - 1)) < NEAR_BORDER))
        cell = ok & ((np.abs(qx - np.round(qx)) < NEAR_CELL) | (np.abs(qy - np.round(qy)) < NEAR_CELL))
        hub = ok & (np.abs(np.abs(p["r"].astype(np.float64)) - huber) < NEAR_HUBER)
    return dict(H=Hm, b=bv, cost=cost, N=int(ok.sum()), near=int(border.sum() + hub.sum()), near_cell=int(cell.sum()), hw=hl * wl)


def solve(sm, xi, damping, prior):
    """delta of (H/N + mu diag(H/N) + W) delta = -(b/N + W xi) by the kernel's Cholesky, or None (pivot <= 0 / non-finite)."""
    n = float(sm["N"])
    if n < 1.0:
        return None
    wp = np.array([prior[0]] * 3 + [prior[1]] * 3, np.float64)
    L = sm["H"] / n
    rhs = -(sm["b"] / n + wp * xi)
    L = L.copy()
    for k in range(6):
        L[k, k] = (L[k, k] + damping * L[k, k]) + wp[k]
    for c in range(6):
        d = L[c, c]
        for k in range(c):
            d -= L[c, k] * L[c, k]
        if not (d > 0.0) or not np.isfinite(d):
            return None
        d = np.sqrt(d)
        L[c, c] = d
        for r in range(c + 1, 6):
            v = L[r, c]
            for k in range(c):
                v -= L[r, k] * L[c, k]
            L[r, c] = v / d
    delta = np.zeros(6)
    for r in range(6):
        v = rhs[r]
        for k in range(r):
            v -= L[r, k] * delta[k]
        delta[r] = v / L[r, r]
    for r in range(5, -1, -1):
        v = delta[r]
        for k in range(r + 1, 6):
            v -= L[k, r] * delta[k]
        delta[r] = v / L[r, r]
    return delta if np.isfinite(delta).all() else None


def update(A, a, delta):
    E = rodrigues(delta[3:])
    return E @ A, E @ a + delta[:3]


def iterate(cur, prev, Dp, f, c, A, a, xi, s, huber, damping, prior, dtype):
    """One iteration: (A', a', xi', sums) -- or the pose unchanged and sums["bad"] set."""
    sm = sums(cur, prev, Dp, f, c, A, a, s, huber, dtype)
    delta = solve(sm, xi, damping, prior)
    sm["bad"] = delta is None
    if delta is None:
        return A, a, xi, sm
    A2, a2 = update(A, a, delta)
    return A2, a2, xi + delta, sm


def run(cur, prev, Dp, f, c, rot, trans, strides, iters, huber, damping, prior, dtype, min_cover=0.0, caps=(np.inf, np.inf)):
    """The whole schedule on one sample: dict(A, a, rot, trans, row [8] float32, applied, near, near_cell, counts = N of every iteration)."""
    A, a = begin(rot, trans)
    A0 = A.copy()
    xi, counts = np.zeros(6), []
    bad, n_it, near, near_cell, cost0, cost1, cover, last_s = False, 0, 0, 0, 0.0, 0.0, 0.0, None
    for s in strides:
        for _ in range(iters):
            if bad:
                continue
            A, a, xi, sm = iterate(cur, prev, Dp, f, c, A, a, xi, s, huber, damping, prior, dtype)
            near += sm["near"]
            near_cell += sm["near_cell"]
            counts.append(sm["N"])
            if sm["N"] >= 1:
                cost = sm["cost"] / sm["N"]
                if last_s != s:
                    last_s, cost0 = s, cost
                cost1, cover = cost, sm["N"] / sm["hw"]
            if sm["bad"]:
                bad = True
            else:
                n_it += 1
    R, t = A.T, -(A.T @ a)
    q = matrix_quat(R)
    dt = float(np.linalg.norm(t - np.asarray(trans, np.float64)))
    angle = float(rotation_angle(A, A0))
    applied = (not bad) and n_it >= 1 and cover >= min_cover and cost1 < cost0 and dt <= caps[0] and angle <= caps[1]
    row = np.array([cost0, cost1, cover, dt, angle, n_it, 1.0 if applied else 0.0, 0.0], F)
    return dict(A=A, a=a, rot=q.astype(F) if applied else np.asarray(rot, F), trans=t.astype(F) if applied else np.asarray(trans, F),
                row=row, applied=applied, near=near, near_cell=near_cell, counts=counts)


# ---- scenes --------------------------------------------------------------------------------------------------------------------
def texture(u, v):
    return 0.5 + 0.2 * np.sin(1.3 * u + 0.4) * np.cos(0.9 * v) + 0.15 * np.sin(0.5 * u + 1.1 * v) + 0.1 * np.cos(2.1 * v - 0.3 * u)


def render_plane(h, w, f, c, n, dist, A=None, a=None):
    """The image [h,w,3] (three equal channels) and depth [h,w] of the textured plane n.X = dist (n, X in the previous
    camera's frame) seen from the camera Y = A X + a (default: the previous camera itself), by ray-plane intersection."""
    A = np.eye(3) if A is None else A
    a = np.zeros(3) if a is None else a
    n = np.asarray(n, np.float64) / np.linalg.norm(n)
    e1 = np.cross(n, [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(n, e1)
    jj, ii = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    ray = np.stack([(ii + 0.5 - c[0]) / f[0], (jj + 0.5 - c[1]) / f[1], np.ones_like(ii)], axis=-1)
    lam = (dist + n @ (A.T @ a)) / (ray @ (A @ n))                 # n . A^T (lam ray - a) = dist
    X = (lam[..., None] * ray - a) @ A                             # A^T (Y - a), row vectors
    img = texture(X @ e1, X @ e2)
    return np.repeat(img[..., None], 3, axis=-1).astype(F), lam.astype(F)


RECOVERY = dict(h=48, w=64, f=(52.3, 49.1), c=(30.7, 25.9), n=(0.15, -0.1, 1.0), dist=6.0,
                q_true=(0.9998, 0.004, -0.012, 0.006), a_true=(0.25, -0.08, 0.12),
                d_rot=(0.004, -0.005, 0.003), d_trans=(0.03, 0.02, -0.04),
                strides=(4, 2, 1), iters=5, huber=0.1, damping=1e-9, prior=(0.0, 0.0))


def recovery_scene():
    """The 48 x 64 plane scene: dict(cur, prev, Dp, f, c, A_true, a_true, rot, trans) -- rot / trans the float32 start motion."""
    S = RECOVERY
    A_true, a_true = quat_matrix(unit(S["q_true"])), np.array(S["a_true"], np.float64)
    prev, depth = render_plane(S["h"], S["w"], S["f"], S["c"], S["n"], S["dist"])
    cur, _ = render_plane(S["h"], S["w"], S["f"], S["c"], S["n"], S["dist"], A_true, a_true)
    # the start pose: the true one perturbed as the definition perturbs a pose, Y <- exp(w^) Y + v (``update``)
    A0, a0 = update(A_true, a_true, np.concatenate([S["d_trans"], S["d_rot"]]))
    rot, trans = given_motion(A0, a0)
    return dict(cur=cur, prev=prev, Dp=depth, f=np.array(S["f"], F), c=np.array(S["c"], F), A_true=A_true, a_true=a_true,
                rot=rot, trans=trans)


def pose_errors(A, a, A_true, a_true):
    """(metres, radians) of a previous-to-current pose against the true one."""
    return float(np.linalg.norm(a - a_true)), float(rotation_angle(A, A_true))


def smooth_case(b, h, w, cams, seed):
    """b samples of a smooth scene for the single-iteration comparison: a band-limited RGB texture on a gently curved surface,
    a small motion, per-sample cameras ``cams`` (helpers.cameras_np).  The current image is the texture shifted and scaled, not a
    render: one iteration only needs a residual with structure; a bright patch puts a block of residuals on the Huber branch.  dict of float32 arrays (cur, prev [b,h,w,3], Dp [b,h,w,1],
    rot [b,4], trans [b,3], f, c [b,2])."""
    rng = np.random.default_rng(seed)
    jj, ii = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    out = dict(cur=[], prev=[], Dp=[], rot=[], trans=[])
    for s in range(b):
        ph = rng.uniform(0, 2 * np.pi, [3, 4])
        k = rng.uniform(0.15, 0.45, [3, 4])

        def tex(x, y):
            return np.stack([0.5 + 0.18 * np.sin(k[ch, 0] * x + ph[ch, 0]) * np.cos(k[ch, 1] * y + ph[ch, 1])
                             + 0.12 * np.sin(k[ch, 2] * x + k[ch, 3] * y + ph[ch, 2]) for ch in range(3)], axis=-1)
        out["prev"].append(tex(ii, jj))
        cur = tex(1.01 * ii + 0.7, 0.99 * jj - 0.4) + 0.02
        cur[h // 5:h // 2, w // 2:(4 * w) // 5] += 0.35              # an "occluder": residuals far above the Huber switch
        out["cur"].append(cur)
        out["Dp"].append(6.0 + 1.5 * np.sin(0.11 * ii + ph[0, 3]) * np.cos(0.09 * jj) + 0.02 * jj)
        aa = rng.normal(0.0, 0.004, 3)
        ang = np.linalg.norm(aa)
        out["rot"].append(np.concatenate([[np.cos(ang / 2)], aa / ang * np.sin(ang / 2)]))
        out["trans"].append(rng.normal([0.0, 0.0, 0.1], 0.05, 3))
    case = {k: np.stack(v).astype(F) for k, v in out.items()}
    case["Dp"] = case["Dp"][..., None]
    case["f"], case["c"] = cams["f"].astype(F), cams["c"].astype(F)
    return case


# the single-iteration comparison of tests/test_gpu_pose_align.py: the seed is chosen so that no pixel sits on a discontinuity
# (tests/test_pose_align_ref.py checks it) and both Huber branches are taken at every stride
ONE_ITERATION = dict(b=3, h=24, w=40, seed=15, strides=(1, 2, 4), huber=0.1, damping=1e-6, prior=(0.0, 0.0))


def one_iteration_case():
    from helpers import cameras_np
    c = ONE_ITERATION
    return smooth_case(c["b"], c["h"], c["w"], cameras_np(c["b"], c["h"], c["w"]), c["seed"])
