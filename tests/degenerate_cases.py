"""The degenerate inputs of DESIGN.md "Degenerate inputs" (rules R1-R4): one table for the GPU tests
(tests/test_gpu_degenerate.py) and for the CPU guard that keeps every case on its edge (tests/test_degenerate_oracle.py).

Every input built here is FINITE; the non-finite values (0/0 queries, x / sqrt(0) features, 1 / 0 parallaxes) arise inside the
code under test.  A case is two samples -- the degenerate one beside a neighbour, so that R4 (a sample's degenerate data never
changes another sample's bits) is checked by the same comparison -- on one of the geometries below.

  kind            sample 0                                             sample 1
  "stationary"    trans = 0: s = |delta| = 0 on every pixel            moving
  "epipole"       identity rotation, trans = (0, 0, tz): s = 0 on the one pixel whose centre is the principal point (both;
                  odd h and w only: with helpers.camera_np the principal point of an even map lies between pixels)
  "zero_cut"      moving; planted all-zero feature cuts: one cut of one c1 pixel, one cut of a 2x3 block of c2 and every
                  cut of c2[1, 0, 0]
  "far_query"     sideways motion, parallaxes planted at +-2e6 and     trans ~ 1e-30: delta is a normal number, delta^2
                  -10 so that hypotheses sit on both clamps of         underflows to 0, so s = 0 and delta / (s / p) = +-Inf
                  clip(disp + n, 1e-6, 1e6): queries 1e6 pixels away   on every pixel
  "prev_d2para"   moving; depth_prev_t == tz on planted pixels: prev_d2para's denominator is 0 there (both samples)

Backward only (BACKWARD_CASES = CASES + these; the forward tests keep their table):
  "clamped_corner" identity rotation, motion up and to the left (tz = 0): every hypothesis of pixel (0, 0) leaves the map over
                  BOTH edges, so both alphas are clamped and the query gradient is selected to 0 (R5) -- while the four cells
                  it reads hold a NaN feature cut (sample 0: cut 0 of f2[0, 0, 0] is all zero) or an infinite warped parallax
                  (sample 1: depth_prev_t[1, 0, 0] == tz).  The alpha gradients are NaN / Inf there, g_disp is exactly 0: the
                  one place where a clamp gradient written as a PRODUCT with a 0/1 mask gives another answer (NaN).
"""
from collections import namedtuple

import numpy as np

from helpers import F, camera_np, motion_np

Geom = namedtuple("Geom", "h w C k t_scale note")

GEOMS = {
    "13x21": Geom(13, 21, 32, 2, 3.0, "odd both ways, C = 32 / 2 cuts"),
    "12x20": Geom(12, 20, 32, 2, 3.0, "even: the principal point lies between pixels"),
    "37x45": Geom(37, 45, 16, 1, 3.0, "C = 16 / 1 cut: ragged tiles of the fused front in both directions"),
    "21x19": Geom(21, 19, 96, 4, 3.0, "C = 96 / 4 cuts of 24"),
    "6x20": Geom(6, 20, 192, 8, 3.0, "C = 192 / 8 cuts: the coarsest level"),
    "20x44": Geom(20, 44, 16, 1, 40.0, "large flows: the LDS-window variants fall back to global gathers"),
}

KINDS = ("stationary", "epipole", "zero_cut", "far_query", "prev_d2para")

Case = namedtuple("Case", "kind geom")

# every kind on the two small maps; the route-specific geometries take the kinds that reach a query (the zero-cut and
# prev_d2para patterns do not depend on the tiling of the gathers)
CASES = [Case(k, g) for g in ("13x21", "12x20") for k in KINDS if not (k == "epipole" and g == "12x20")]
CASES += [Case("stationary", "37x45"), Case("epipole", "37x45"), Case("far_query", "37x45"),
          Case("stationary", "21x19"), Case("epipole", "21x19"), Case("zero_cut", "21x19"),
          Case("stationary", "6x20"), Case("far_query", "6x20"), Case("zero_cut", "6x20"),
          Case("stationary", "20x44"), Case("far_query", "20x44")]

B = 2               # samples per case
DSCV_RANGE = 4      # m4depth_network.py:221
SNCV_RANGE = 3      # m4depth_network.py:232


def case_id(c):
    return f"{c.kind}-{c.geom}"


BACKWARD_ONLY_KINDS = ("clamped_corner",)
BACKWARD_CASES = CASES + [Case("clamped_corner", "13x21"), Case("clamped_corner", "37x45")]


def _seed(case):
    return 7000 + 100 * (KINDS + BACKWARD_ONLY_KINDS).index(case.kind) + sorted(GEOMS).index(case.geom)


def far_plant(h, w):
    """Pixels of the far-query case whose parallax is planted at the upper / lower clamp, spread over the map."""
    up = [(0, 0), (h // 2, w // 3), (h - 1, w - 1), (1, w - 2)]
    lo = [(0, w - 1), (h // 2, 2 * w // 3), (h - 1, 0)]
    return up, lo


def zero_plant(h, w, k):
    """(c1 pixel, cut), (c2 block origin, cut) of the zero-cut case; the block is 2 rows x 3 columns."""
    return ((h // 3, w // 2), k - 1), ((h // 2, w // 4), 0)


def d2para_plant(h, w):
    return [(0, 0), (h // 2, w // 2), (h - 2, w - 3), (h - 1, w - 1)]


def make(case):
    """The finite inputs of ``case``: raw feature maps f1 (current frame) and f2 (previous), the depth memory, the coarser
    parallax ``disp``, the motion and the camera, as float32 numpy arrays."""
    g = GEOMS[case.geom]
    h, w, C, k = g.h, g.w, g.C, g.k
    rng = np.random.default_rng(_seed(case))
    cam = camera_np(B, h, w)
    rot, trans = motion_np(rng, B, t_scale=(g.t_scale, g.t_scale, 1.0))
    f1 = rng.standard_normal([B, h, w, C]).astype(F)
    f2 = rng.standard_normal([B, h, w, C]).astype(F)
    disp = (0.2 + 6.0 * rng.random([B, h, w, 1])).astype(F)
    depth_prev_t = (1.0 + 50.0 * rng.random([B, h, w, 1])).astype(F)
    nc = C // k
    if case.kind == "stationary":
        trans[0] = 0.0
    elif case.kind == "epipole":
        assert h % 2 == 1 and w % 2 == 1, case
        rot = np.tile(np.array([[1.0, 0.0, 0.0, 0.0]], F), [B, 1])
        trans = np.array([[0.0, 0.0, 0.3], [0.0, 0.0, -0.45]], F)
    elif case.kind == "zero_cut":
        ((j1, i1), k1), ((j2, i2), k2) = zero_plant(h, w, k)
        f1[0, j1, i1, k1 * nc:(k1 + 1) * nc] = 0.0
        f2[0, j2:j2 + 2, i2:i2 + 3, k2 * nc:(k2 + 1) * nc] = 0.0
        f2[1, 0, 0, :] = 0.0
    elif case.kind == "far_query":
        rot[0] = np.array([1.0, 0.0, 0.0, 0.0], F)
        trans[0] = np.array([0.3, 0.0, 0.0], F)
        trans[1] = np.array([1e-30, -2e-30, 0.0], F)
        up, lo = far_plant(h, w)
        for n, (j, i) in enumerate(up):
            disp[:, j, i, 0] = F(2e6) if n % 2 == 0 else F(1e6 - 2.0)     # every hypothesis on the clamp / only the upper ones
        for n, (j, i) in enumerate(lo):
            disp[:, j, i, 0] = F(-10.0) if n % 2 == 0 else F(-2.0)         # every hypothesis on the clamp / only the lower ones
    elif case.kind == "prev_d2para":
        for (j, i) in d2para_plant(h, w):
            depth_prev_t[:, j, i, 0] = trans[:, 2]
    elif case.kind == "clamped_corner":
        rot = np.tile(np.array([[1.0, 0.0, 0.0, 0.0]], F), [B, 1])
        trans = np.array([[-0.3, -0.2, 0.0], [-0.25, -0.35, 0.0]], F)
        f2[0, 0, 0, :nc] = 0.0
        depth_prev_t[1, 0, 0, 0] = trans[1, 2]
    else:
        raise ValueError(case.kind)
    return dict(f1=f1, f2=f2, disp=disp, depth_prev_t=depth_prev_t, rot=rot, trans=trans, cam=cam, h=h, w=w, C=C, k=k)


def sweep_queries(O, d):
    """The (row, col) query points [b, h, w, 2r+1, 2] of the DSCV sweep of a case, in the oracle's arithmetic
    (oracle get_parallax_sweeping_cv, utils/depth_operations.py:235-264 and dense_image_warp.py:244)."""
    b, h, w = d["disp"].shape[:3]
    m = O.motion_factors(b, h, w, d["rot"], d["trans"], d["cam"])
    jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    out = np.zeros([b, h, w, 2 * DSCV_RANGE + 1, 2], F)
    with np.errstate(all="ignore"):
        for t in range(2 * DSCV_RANGE + 1):
            p = np.fmin(np.fmax(d["disp"][..., 0] + F(t - DSCV_RANGE), F(1e-6)), F(1e6))
            divider = m["sqrt"] / p
            fx = (m["proj_x"] + m["delta_x"] / divider) - m["start_x"]
            fy = (m["proj_y"] + m["delta_y"] / divider) - m["start_y"]
            out[..., t, 0] = jj.astype(F)[None] + fy
            out[..., t, 1] = ii.astype(F)[None] + fx
    return out


def reproject_depth(d):
    """The depth map the cases hand to ``reproject``: the depth memory with three zeros planted (with trans = 0 the projected
    z is then 0 and the projection 0/0)."""
    depth = d["depth_prev_t"].copy()
    h, w = d["h"], d["w"]
    for (j, i) in [(0, 1), (h // 2, w // 2), (h - 1, w - 2)]:
        depth[:, j, i, 0] = 0.0
    return depth


_REFERENCE = {}


def reference(case):
    """Everything the rule-bearing oracle computes for ``case``, evaluated once per process and shared (read-only) by the tests:
    the op-level outputs of part 3a, keyed by name."""
    if case in _REFERENCE:
        return _REFERENCE[case]
    from oracle import m4depth_oracle as O
    d = make(case)
    k, rot, trans, cam = d["k"], d["rot"], d["trans"], d["cam"]
    r = {}
    with np.errstate(all="ignore"):
        r["c1"] = O.normalize_cuts(d["f1"], k)
        r["c2"] = O.normalize_cuts(d["f2"], k)
        r["p2d"] = O.parallax2depth(d["disp"], rot, trans, cam)
        r["d2p"] = O.depth2parallax(d["depth_prev_t"], rot, trans, cam)
        r["pd2p"] = O.prev_d2para(d["depth_prev_t"], rot, trans, cam)
        r["recompute"] = O.recompute_depth(d["depth_prev_t"], rot, trans, cam)
        rp, (pmr, rotc) = O.reproject(r["c2"][..., :4], reproject_depth(d), rot, trans, cam)
        r["reproject"], r["reproject_pmr"], r["reproject_rotc"] = rp, pmr, rotc
        for acc in ("fp32_round", "fp16_seq"):
            cv, pd, y0, x0 = O.get_parallax_sweeping_cv(r["c1"], r["c2"], r["pd2p"], d["disp"], rot, trans, cam, DSCV_RANGE, k,
                                                        cv_accum=acc, return_index=True)
            r[f"cv_{acc}"] = cv
        r["prev_disp"], r["idx"] = pd, np.stack([y0, x0], -1)
        r["sncv_auto"] = O.cost_volume(r["c1"], r["c1"], SNCV_RANGE, nbre_cuts=k)
        r["sncv"] = O.cost_volume(r["c1"], r["c2"], SNCV_RANGE, nbre_cuts=k)
        # the two gathers whose query IS their input: the centre and the last hypothesis of the case's own sweep
        q = sweep_queries(O, d)
        b, h, w = q.shape[:3]
        grid = np.stack(np.meshgrid(np.arange(h), np.arange(w), indexing="ij"), -1).astype(F)[None]
        r["queries"] = q
        r["flow"] = (q[..., 2 * DSCV_RANGE, :] - grid).astype(F)
        r["warp"], wy, wx = O.dense_image_warp(r["c2"], r["flow"], return_index=True)
        r["warp_idx"] = np.stack([wy, wx], -1)
        r["points"] = q[..., DSCV_RANGE, :].reshape(b, h * w, 2)
        r["interp"], iy, ix = O.interpolate_bilinear(r["c2"], r["points"], return_index=True)
        r["interp_idx"] = np.stack([iy, ix], -1)
    for v in r.values():
        v.setflags(write=False)
    r["inputs"] = d
    _REFERENCE[case] = r
    return r


# ---- the backward on the same cases (rules R5, R6): fixed upstream gradients and autodiff of the rule-bearing restatement
BACKWARD_TENSORS = ("dscv_g_c1", "dscv_g_c2", "dscv_g_disp_prev_t", "dscv_g_disp", "sncv_auto_g_c1", "sncv_g_c1", "sncv_g_c2", "norm_g_f1")
# the tensors whose graph has no float16 step: their non-finite masks are the same in float32 and float64
NO_HALF_TENSORS = ("dscv_g_disp_prev_t", "sncv_auto_g_c1", "sncv_g_c1", "sncv_g_c2", "norm_g_f1")


def backward_upstream(case):
    """The upstream gradients of a case (finite, drawn once per case): of cv, of the warped parallax, of the SNCV output and of
    the normalised features."""
    g = GEOMS[case.geom]
    rng = np.random.default_rng(50000 + _seed(case))
    ncp, mo2 = 2 * DSCV_RANGE + 1, (2 * SNCV_RANGE + 1) ** 2
    return dict(g_cv=rng.standard_normal([B, g.h, g.w, g.k * ncp]).astype(F),
                g_prev_disp=rng.standard_normal([B, g.h, g.w, ncp]).astype(F),
                g_sncv=rng.standard_normal([B, g.h, g.w, mo2 * g.k]).astype(F),
                g_feat=rng.standard_normal([B, g.h, g.w, g.C]).astype(F))


_BACKWARD = {}


def backward_reference(case, double=False):
    """Autodiff of oracle/m4depth_oracle_train.py on ``case``, evaluated once per process and shared read-only: the gradients
    BACKWARD_TENSORS and the forward outputs (cv, prev_disp, sncv_auto, sncv, c1n) they were taken through.  The cost volumes
    take the numpy oracle's normalised features and prev_d2para as their leaves (what the kernels are handed); the normalisation
    takes the raw f1.  ``double``: the float32 inputs evaluated in float64, the DSCV correlation without its float16 step."""
    key = (case, double)
    if key in _BACKWARD:
        return _BACKWARD[key]
    import torch
    from oracle import m4depth_oracle_train as OT
    r = reference(case)
    d, u = r["inputs"], backward_upstream(case)
    k = d["k"]
    dt = torch.float64 if double else torch.float32
    T = lambda a: torch.from_numpy(np.array(a)).to(dt)
    leaf = lambda a: T(a).requires_grad_(True)
    cam = {n: np.asarray(v, np.float64 if double else F) for n, v in d["cam"].items()}
    out = {}
    c1, c2, dpt, disp = leaf(r["c1"]), leaf(r["c2"]), leaf(r["pd2p"]), leaf(d["disp"])
    cv, pd = OT.get_parallax_sweeping_cv(c1, c2, dpt, disp, T(d["rot"]), T(d["trans"]), cam, DSCV_RANGE, nbre_cuts=k, half=not double)
    ((cv * T(u["g_cv"])).sum() + (pd * T(u["g_prev_disp"])).sum()).backward()
    out.update(cv=cv, prev_disp=pd, dscv_g_c1=c1.grad, dscv_g_c2=c2.grad, dscv_g_disp_prev_t=dpt.grad, dscv_g_disp=disp.grad)
    a = leaf(r["c1"])
    sn = OT.cost_volume(a, a, SNCV_RANGE, nbre_cuts=k)
    (sn * T(u["g_sncv"])).sum().backward()
    out.update(sncv_auto=sn, sncv_auto_g_c1=a.grad)
    a, b_ = leaf(r["c1"]), leaf(r["c2"])
    sn = OT.cost_volume(a, b_, SNCV_RANGE, nbre_cuts=k)
    (sn * T(u["g_sncv"])).sum().backward()
    out.update(sncv=sn, sncv_g_c1=a.grad, sncv_g_c2=b_.grad)
    f1 = leaf(d["f1"])
    c1n = OT.normalize_cuts(f1, k)
    (c1n * T(u["g_feat"])).sum().backward()
    out.update(c1n=c1n, norm_g_f1=f1.grad)
    out = {n: v.detach().numpy() for n, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    _BACKWARD[key] = out
    return out


DSCV_BWD_WINDOW_FLOATS = 48 * 256    # the default LDS budget of m4d_dscv_bwd (csrc/m4d_grad.hip, the launcher)


def dscv_bwd_blocks(idx, C):
    """(private [b, blocks_y, blocks_x] bool, block height, block width): which pixel blocks of dscv_bwd_kernel keep their g_c2
    window in LDS, from the forward's (y0, x0) grid [b, h, w, 2r+1, 2] -- the block shape of the launcher and the window
    test of the kernel, per block (tests/test_gpu_grad.py::dscv_window_mix gives the two totals)."""
    b, h, w = idx.shape[:3]
    ppw = 64 // (C // 4)
    p2 = 0
    while (2 << p2) <= 4 * ppw:
        p2 += 1
    bh, bw = 1 << (p2 // 2), 1 << (p2 - p2 // 2)
    ph, pw = -(-h // bh) * bh, -(-w // bw) * bw
    pad = np.pad(idx, ((0, 0), (0, ph - h), (0, pw - w), (0, 0), (0, 0)), mode="edge")
    blk = pad.reshape(b, ph // bh, bh, pw // bw, bw, -1, 2)
    lo, hi = blk.min(axis=(2, 4, 5)), blk.max(axis=(2, 4, 5))
    cells = (hi[..., 0] - lo[..., 0] + 2).astype(np.int64) * (hi[..., 1] - lo[..., 1] + 2)
    return cells * C <= DSCV_BWD_WINDOW_FLOATS, bh, bw


def blocks_with(pixels, bh, bw):
    """[b, blocks_y, blocks_x] bool: the blocks holding a True pixel of ``pixels`` [b, h, w]."""
    b, h, w = pixels.shape
    ph, pw = -(-h // bh) * bh, -(-w // bw) * bw
    return np.pad(pixels, ((0, 0), (0, ph - h), (0, pw - w))).reshape(b, ph // bh, bh, pw // bw, bw).any(axis=(2, 4))


PARITY_OUTPUTS = ("p2d", "d2p", "pd2p", "recompute", "reproject", "cv_fp32_round", "cv_fp16_seq", "prev_disp", "sncv_auto", "sncv",
                  "warp", "interp")


# ---- model-level cases: sample independence (R4) and recovery after a stationary frame (R2), M4Depth.stream_step
MODEL_LEVELS, MODEL_H, MODEL_W = 3, 64, 96
STATIONARY_FRAME = 2
ORACLE_K = 1        # frames after motion resumes until ``O.M4Depth`` is wholly finite again (tests/test_degenerate_oracle.py)


def model_sequence(batch, frames, seed=9):
    """(weights, samples, camera): He-normal weights and a lateral-motion trajectory; every stream moves on every frame."""
    from m4depth_amd import synthetic as S
    weights = S.init_weights(MODEL_LEVELS, seed=21)
    samples, cam = S.make_sequence(batch, frames, MODEL_H, MODEL_W, seed=seed, motion="lateral")
    return weights, samples, cam


def make_stationary(samples, frame, rows):
    """The same trajectory with trans = 0 for the samples ``rows`` at ``frame``."""
    out = [dict(s) for s in samples]
    tr = out[frame]["trans"].copy()
    tr[rows] = 0.0
    out[frame]["trans"] = tr
    return out


def first_recovered(finite_per_frame):
    """Frames after STATIONARY_FRAME until everything is finite again, given one bool per frame."""
    for t in range(STATIONARY_FRAME + 1, len(finite_per_frame)):
        if finite_per_frame[t]:
            return t - STATIONARY_FRAME
    return None
