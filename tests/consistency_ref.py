"""Restatement of the reprojection-consistency score (include/m4depth_hip.h, "Reprojection consistency") on
``photometric_ref.warp`` and ``photometric_ref.photo_error``: the warp in float32 (operation for operation in the kernels'
order: the bitwise reference of `warped` / `valid` / the query), everything after it in float64.

The planted wiring errors (``score(..., planted=...)``): ``camera_of_sample0`` reads sample 0's intrinsics for every sample,
``no_motion`` does not apply the motion, ``dp_at_pixel`` samples the previous estimate at p instead of at the query, ``halo``
sums the geometric term over every tile's 18x18 staging region instead of its own 16x16 pixels.
"""
import functools

import numpy as np
import torch

import photometric_ref as P
from helpers import cameras_np

COLUMNS = ("photo", "photo_id", "better", "geo", "cover", "geo_cover")
TILE = 16
ULP32 = 2.0 ** -23
# The GPU bar, derived: the inputs to the double arithmetic (warped, valid, Pz, Dq) are bit-identical, the double sums differ
# only in their order (relative error ~ n 2^-53, far below float32), and each value is rounded once to float32 at the end:
# half an ulp for the rounding, and a double-precision difference can move a value across one rounding boundary -- within 2 ulps.
GPU_ULPS = 2


def _t(a, dtype):
    return torch.from_numpy(np.asarray(a)).to(dtype)


def score(case, planted=None):
    """case: dict(depth, depth_prev [b,h,w,1], rot, trans, f, c, cur, prev [b,h,w,3]) float32 numpy.  Returns a dict: rows
    [b,6] float64 (unrounded), rows32 [b,6] float32 (rounded once), n, ng [b] int, M [b,h-2,w-2], G, valid [b,h,w] bool,
    warped [b,h,w,3] float32, pe_w, pe_id [b,h-2,w-2] float64, g [b,h,w] float64, pz, dq [b,h,w] float32."""
    f32 = torch.float32
    D, Dp = _t(case["depth"], f32), _t(case["depth_prev"], f32)
    rot, trans = _t(case["rot"], f32), _t(case["trans"], f32)
    f, c, cur, prev = _t(case["f"], f32), _t(case["c"], f32), _t(case["cur"], f32), _t(case["prev"], f32)
    b, h, w, _ = D.shape
    if planted == "no_motion":
        rot = torch.zeros_like(rot)
        if rot.shape[1] == 4:
            rot[:, 0] = 1.0
        trans = torch.zeros_like(trans)
    wp = P.warp(D, rot, trans, f, c, prev, camera_of_sample0=planted == "camera_of_sample0")
    warped, valid, qx, qy, pz = wp["warped"], wp["valid"], wp["qx"], wp["qy"], wp["pz"]
    # the cell and alphas of the image sample (photometric_ref.warp's, float32)
    fly = torch.nan_to_num(torch.clamp(torch.floor(qy), 0.0, float(h - 2)), nan=0.0)
    flx = torch.nan_to_num(torch.clamp(torch.floor(qx), 0.0, float(w - 2)), nan=0.0)
    ay, ax = torch.clamp(qy - fly, 0.0, 1.0), torch.clamp(qx - flx, 0.0, 1.0)
    y0, x0 = fly.long(), flx.long()
    if planted == "dp_at_pixel":
        jj = torch.arange(h).reshape(1, h, 1).expand(b, h, w)
        ii = torch.arange(w).reshape(1, 1, w).expand(b, h, w)
        y0, x0 = torch.clamp(jj, max=h - 2), torch.clamp(ii, max=w - 2)
        ay, ax = (jj - y0).to(f32), (ii - x0).to(f32)
    bi = torch.arange(b).reshape(b, 1, 1).expand(b, h, w)
    d = Dp[..., 0]
    tl, tr, bl, br = d[bi, y0, x0], d[bi, y0, x0 + 1], d[bi, y0 + 1, x0], d[bi, y0 + 1, x0 + 1]
    taps_ok = torch.ones_like(valid)
    for t in (tl, tr, bl, br):
        taps_ok &= torch.isfinite(t) & (t > 0)
    top = ax * (tr - tl) + tl
    bot = ax * (br - bl) + bl
    dq = ay * (bot - top) + top                                    # m4d_lerp2, float32
    G = valid & taps_ok
    g = (pz.double() - dq.double()).abs() / (pz.double() + dq.double())
    f64 = torch.float64
    pe_w = P.photo_error(warped.to(f64), cur.to(f64))
    pe_id = P.photo_error(prev.to(f64), cur.to(f64))
    M = P._win(valid.to(f64)) == 9.0
    weight = torch.ones((h, w), dtype=f64)
    if planted == "halo":                                          # how often a pixel lies in some tile's 18x18 staging region
        weight = torch.zeros((h, w), dtype=f64)
        for ty in range(0, h, TILE):
            for tx in range(0, w, TILE):
                weight[max(ty - 1, 0):min(ty + TILE + 1, h), max(tx - 1, 0):min(tx + TILE + 1, w)] += 1.0
    rows = np.zeros((b, 6), np.float64)
    n, ng = np.zeros(b, np.int64), np.zeros(b, np.int64)
    for s in range(b):
        n[s] = int(M[s].sum())
        ngw = float((G[s].to(f64) * weight).sum())
        ng[s] = int(G[s].sum())
        if n[s] == 0 or ng[s] == 0:
            continue
        rows[s, 0] = float(pe_w[s][M[s]].sum()) / n[s]
        rows[s, 1] = float(pe_id[s][M[s]].sum()) / n[s]
        rows[s, 2] = float((pe_w[s] < pe_id[s])[M[s]].sum()) / n[s]
        rows[s, 3] = float((torch.where(G[s], g[s], torch.zeros_like(g[s])) * weight).sum()) / ngw
        rows[s, 4] = n[s] / float((h - 2) * (w - 2))
        rows[s, 5] = ngw / float(h * w)
    return {"rows": rows, "rows32": rows.astype(np.float32), "n": n, "ng": ng, "M": M, "G": G, "valid": valid,
            "warped": warped, "pe_w": pe_w, "pe_id": pe_id, "g": g, "pz": pz, "dq": dq}


def counted(res, reset=None, active=None):
    """counted [b] bool of the definition from a ``score`` result and the masks (default: nothing reset, everything active)."""
    b = len(res["n"])
    reset = np.zeros(b, bool) if reset is None else np.asarray(reset, bool)
    active = np.ones(b, bool) if active is None else np.asarray(active, bool)
    return active & ~reset & (res["n"] > 0) & (res["ng"] > 0)


def ulps(got, ref64):
    """|got - ref| in units of the float32 ulp of |ref| (ref the unrounded float64 value); 0 where both are exactly 0."""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    mag = np.maximum(np.abs(ref64), np.finfo(np.float32).tiny)
    return np.abs(got - ref64) / (2.0 ** np.floor(np.log2(mag)) * ULP32)


# ---- the cases the CPU and the GPU tests share ----------------------------------------------------------------------------------
def random_case(name):
    """A geometry of photometric_ref.CASES plus a random previous estimate in [4,12]."""
    case = P.make_case(name)
    h, w, _, seed = P.CASES[name]
    rng = np.random.default_rng(77000 + 1000 * h + 10 * w + seed)
    case["depth_prev"] = rng.uniform(4.0, 12.0, case["depth"].shape).astype(np.float32)
    return case


def big_case(h=33, w=35, b=3, seed=5):
    """33 x 35 at b = 3: three tiles per axis, the last one 1 and 3 pixels wide; per-sample cameras, quaternions."""
    rng = np.random.default_rng(seed)
    cam = cameras_np(b, h, w)
    aa = rng.normal(0.0, 0.01, [b, 3])
    ang = np.linalg.norm(aa, axis=1, keepdims=True)
    rot = np.concatenate([np.cos(ang / 2), aa / np.maximum(ang, 1e-12) * np.sin(ang / 2)], axis=1)
    trans = rng.normal([0.35, -0.1, 0.05], 0.03, [b, 3]) * np.array([[1.0], [-1.3], [0.7]])[:b]
    u = lambda lo, hi, shape: rng.uniform(lo, hi, shape).astype(np.float32)
    return {"name": "33x35", "depth": u(4.0, 12.0, [b, h, w, 1]), "depth_prev": u(4.0, 12.0, [b, h, w, 1]),
            "rot": rot.astype(np.float32), "trans": trans.astype(np.float32), "f": cam["f"], "c": cam["c"],
            "cur": u(0.0, 1.0, [b, h, w, 3]), "prev": u(0.0, 1.0, [b, h, w, 3])}


RANDOM_CASES = tuple(P.CASES) + ("33x35",)


@functools.lru_cache(maxsize=None)
def case_and_ref(name):
    """(case, score(case)) of a shared case, computed once and never modified."""
    if name == "33x35":
        case = big_case()
    elif name == "exact":
        case = exact_scene()
    elif name == "hostile":
        case = hostile_case()
    elif name == "out-of-view":
        case = out_of_view_case()
    else:
        case = random_case(name)
    return case, score(case)


def exact_scene(h=12, w=20, k=2, scale=1.0, forward=0.0, seed=3):
    """A fronto-parallel plane at z0 = 8, identity rotation, dyadic camera f = (16, 8), c = (w/2, h/2).  With ``forward`` = 0
    the translation is sideways, tx = k z0 / fx, so the flow is exactly k pixels along x and every intermediate is exact in
    float32: Px = 8 mx + 16 k / 2 ... = z0 (mx + k), Pz = z0.  The images hold multiples of 1/256 (the one column read with
    alpha 1 from the cell before, a (r - l) + l, is then exact too); prev(y, x) = cur(y, x - k), columns x < k random.
    ``scale`` multiplies the estimate D (not the translation), ``forward`` > 0 replaces the translation by (0, 0, forward) and
    scales the previous estimate as well."""
    rng = np.random.default_rng(seed)
    z0, fx, fy = 8.0, 16.0, 8.0
    cur = (rng.integers(0, 257, [1, h, w, 3]) / 256.0).astype(np.float32)
    prev = (rng.integers(0, 257, [1, h, w, 3]) / 256.0).astype(np.float32)
    prev[:, :, k:] = cur[:, :, :w - k]
    trans = [0.0, 0.0, forward] if forward else [k * z0 / fx, 0.0, 0.0]
    return {"name": "exact", "depth": np.full([1, h, w, 1], z0 * scale, np.float32),
            "depth_prev": np.full([1, h, w, 1], z0 * (scale if forward else 1.0), np.float32),
            "rot": np.array([[1.0, 0.0, 0.0, 0.0]], np.float32), "trans": np.array([trans], np.float32),
            "f": np.array([[fx, fy]], np.float32), "c": np.array([[w / 2.0, h / 2.0]], np.float32), "cur": cur, "prev": prev}


def hostile_case():
    """random_case('13x21-angle') with NaN, +Inf, 0 and negative pixels planted in D and Dp."""
    case = random_case("13x21-angle")
    case["depth"] = case["depth"].copy()
    case["depth"][0, 2, 3:8, 0] = [np.nan, np.inf, 0.0, -3.0, -np.inf]
    case["depth"][1, 6, 9:13, 0] = [np.nan, 0.0, -0.5, np.inf]
    case["depth_prev"][0, 7, 10:14, 0] = [np.nan, np.inf, 0.0, -2.0]
    case["depth_prev"][1, 3, 2:5, 0] = [-1.0, np.nan, 0.0]
    case["name"] = "hostile"
    return case


def out_of_view_case():
    """Sample 0 of random_case('13x21-quat') thrown out of view (N = Ng = 0) beside an ordinary sample 1."""
    case = random_case("13x21-quat")
    case["trans"] = case["trans"].copy()
    case["trans"][0] = [400.0, 0.0, 0.0]
    case["name"] = "out-of-view"
    return case
