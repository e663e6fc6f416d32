"""Restatement of the photometric loss's two options (include/m4depth_hip.h, "Full-resolution terms and the minimum over two
sources") with torch CPU tensors, on top of tests/photometric_ref.py: the half-pixel upsampling U_s, the inverse motion, the
per-pixel minimum over the previous and the next frame.  Autodiff stands for the backward (the adjoint U_s^T included); the
dtype is a parameter (float64 = the reference, float32 = the yardstick and, operation for operation, the bitwise reference of
U_s).

Two margins join those of photometric_ref: ``select`` = |pe_0 - pe_1| where both sources are ok (a local kink: the pixel's
window changes source) and ``automask`` = |m - id| where some source is ok (global: a flipped bit changes N).

The ``smooth`` margin leaves out the pairs of fine pixels that U_s makes equal BY CONSTRUCTION: inside the clamped band of an
axis (src <= 0, or the upper tap clamped onto the lower one) two neighbours along that axis read the same coarse samples with
the same weights, so their difference is exactly 0 in every precision and sign(0) = 0 carries no gradient anywhere -- nothing
a rounding error could flip.
"""
import functools

import numpy as np
import torch

import photometric_ref as R
from helpers import cameras_np

MARGIN = R.MARGIN


# ---- U_s ------------------------------------------------------------------------------------------------------------------------
def _axis(n, s, dtype, mode):
    """(i0, i1 [N] long, a [N] dtype, clamped [N] bool) of one axis: N = n s outputs over n inputs."""
    N = n * s
    Y = torch.arange(N, dtype=dtype)
    if mode == "half_pixel":
        raw = (Y + 0.5) / s - 0.5
    elif mode == "align_corners":
        raw = Y * (float(n - 1) / float(max(N - 1, 1)))
    elif mode == "legacy_v1":
        raw = Y / s
    else:
        raise ValueError(mode)
    src = torch.clamp(raw, min=0.0)
    i0 = torch.clamp(torch.floor(src).long(), max=n - 1)
    i1 = torch.clamp(i0 + 1, max=n - 1)
    return i0, i1, src - i0.to(dtype), (raw <= 0) | (i1 == i0)


def upsample_hp(x, s, mode="half_pixel", adjoint_no_clamp=False):
    """[b,h,w,c] -> [b, h s, w s, c]: bilinear, half-pixel centres, edge clamp; m4d_lerp2's operation order.  ``mode``: the
    planted conventions ``align_corners`` and ``legacy_v1``; ``adjoint_no_clamp`` (planted): the fine pixels of the clamped
    border rows and columns hand no gradient back."""
    b, h, w, _ = x.shape
    y0, y1, ay, cy = _axis(h, s, x.dtype, mode)
    x0, x1, ax, cx = _axis(w, s, x.dtype, mode)
    ay, ax = ay.reshape(1, -1, 1, 1), ax.reshape(1, 1, -1, 1)
    tl, tr = x[:, y0][:, :, x0], x[:, y0][:, :, x1]
    bl, br = x[:, y1][:, :, x0], x[:, y1][:, :, x1]
    top = ax * (tr - tl) + tl
    bot = ax * (br - bl) + bl
    out = ay * (bot - top) + top
    if adjoint_no_clamp:
        out = torch.where((cy.reshape(-1, 1) | cx.reshape(1, -1)).reshape(1, h * s, w * s, 1), out.detach(), out)
    return out


def structurally_equal(h, w, s):
    """(along x [H, W-1], along y [H-1, W]) bool: neighbours that U_s makes equal by construction (see the module docstring)."""
    _, _, _, cy = _axis(h, s, torch.float64, "half_pixel")
    _, _, _, cx = _axis(w, s, torch.float64, "half_pixel")
    H, W = h * s, w * s
    ex = (cx[1:] & cx[:-1]).reshape(1, W - 1).expand(H, W - 1)
    ey = (cy[1:] & cy[:-1]).reshape(H - 1, 1).expand(H - 1, W)
    return ex, ey


def motion_inverse(rot, trans):
    """Quaternion motion x -> R(rot) x + trans  ->  its inverse: rot' = (w, -x, -y, -z), trans' = -(R(rot') trans)."""
    assert rot.shape[1] == 4
    inv = rot * torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=rot.dtype)
    r = R.rot_mat(inv)
    t0, t1, t2 = trans.unbind(-1)
    out = torch.stack([(r[0] * t0 + r[1] * t1) + r[2] * t2, (r[3] * t0 + r[4] * t1) + r[5] * t2,
                       (r[6] * t0 + r[7] * t1) + r[8] * t2], dim=-1)
    return inv, -out


def apply_motion(rot, trans, x):
    """R(rot) x + trans for points x [b,3]."""
    r = R.rot_mat(rot)
    return torch.stack([(r[0] * x[:, 0] + r[1] * x[:, 1]) + r[2] * x[:, 2], (r[3] * x[:, 0] + r[4] * x[:, 1]) + r[5] * x[:, 2],
                        (r[6] * x[:, 0] + r[7] * x[:, 1]) + r[8] * x[:, 2]], dim=-1) + trans


# ---- one term ---------------------------------------------------------------------------------------------------------------------
def multi_term(depth, s, rot0, trans0, f, c, cur, src0, src1=None, rot1=None, trans1=None, smooth=1e-3, automask=True, sel=None,
               **planted):
    """One term with the options.  ``depth`` [b,h,w,1]; ``s`` = 1 (scale level) or the upsampling factor (scale full: images
    and camera at [h s, w s]); source 0 = ``src0`` with (rot0, trans0); source 1 (optional) = ``src1`` with the INVERSE of
    (rot1, trans1), the motion of frame t+1.  ``sel`` (optional, [b,H,W] uint8) replaces the computed selection.  Planted
    errors: only_prev, identity_prev_only, next_not_inverted, align_corners, legacy_v1, adjoint_no_clamp."""
    if planted.get("only_prev"):
        src1 = None
    mode = "align_corners" if planted.get("align_corners") else "legacy_v1" if planted.get("legacy_v1") else "half_pixel"
    D = upsample_hp(depth, s, mode, planted.get("adjoint_no_clamp", False)) if s > 1 else depth
    b, H, W, _ = D.shape
    dt = D.dtype
    wp0 = R.warp(D, rot0, trans0, f, c, src0)
    pe0 = R.photo_error(wp0["warped"], cur)
    ok0 = R._win(wp0["valid"].to(dt)) == 9.0
    pe_id = R.photo_error(src0, cur)
    wps = [wp0]
    if src1 is None:
        m, chosen = pe0, ok0
        choice_in = ok0.to(torch.uint8)
        both_ok = torch.zeros_like(ok0)
        pe1 = None
    else:
        r1, t1 = (rot1, trans1) if planted.get("next_not_inverted") else motion_inverse(rot1, trans1)
        wp1 = R.warp(D, r1, t1, f, c, src1)
        wps.append(wp1)
        pe1 = R.photo_error(wp1["warped"], cur)
        ok1 = R._win(wp1["valid"].to(dt)) == 9.0
        take1 = ok1 & (~ok0 | (pe1.detach() < pe0.detach()))               # a tie keeps the previous frame
        m = torch.where(take1, pe1, pe0)
        chosen = ok0 | ok1
        choice_in = torch.where(take1, 2, 1).to(torch.uint8) * chosen.to(torch.uint8)
        both_ok = ok0 & ok1
        if not planted.get("identity_prev_only"):
            pe_id = torch.minimum(pe_id, R.photo_error(src1, cur))
    m_in = chosen & (m.detach() < pe_id) if automask else chosen
    computed = torch.zeros((b, H, W), dtype=torch.uint8)
    computed[:, 1:-1, 1:-1] = choice_in * m_in.to(torch.uint8)
    used = computed if sel is None else sel
    u_in = used[:, 1:-1, 1:-1]
    if src1 is None:
        mf = (u_in != 0).to(dt)
        n = mf.sum()
        photo = (mf * pe0).sum() / torch.clamp(n, min=1.0)
    else:
        n = (u_in != 0).to(dt).sum()
        photo = ((u_in == 1).to(dt) * pe0 + (u_in == 2).to(dt) * pe1).sum() / torch.clamp(n, min=1.0)
    ld = torch.log(wp0["dc"])
    ex = torch.exp(-(cur[:, :, 1:] - cur[:, :, :-1]).abs().mean(dim=-1))
    ey = torch.exp(-(cur[:, 1:] - cur[:, :-1]).abs().mean(dim=-1))
    dx, dy = ld[:, :, 1:] - ld[:, :, :-1], ld[:, 1:] - ld[:, :-1]
    sm = ((dx.abs() * ex).sum() + (dy.abs() * ey).sum()) / float(b * H * W)
    term = photo + smooth * sm
    # ---- margins
    inf = torch.full((b, H, W), float("inf"), dtype=torch.float64)
    cell, absdiff = inf.clone(), inf.clone()
    for wp in wps:
        qx, qy = wp["qx"].double(), wp["qy"].double()
        cl = torch.minimum((qx - torch.round(qx)).abs(), (qy - torch.round(qy)).abs())
        cl = torch.minimum(cl, wp["pz"].double().abs())
        cell = torch.minimum(cell, torch.where(torch.isfinite(cl), cl, torch.zeros_like(cl)))
        absdiff = torch.minimum(absdiff, (wp["warped"].detach() - cur).abs().min(dim=-1).values.double())
    am, se = inf.clone(), inf.clone()
    if automask:
        am[:, 1:-1, 1:-1] = torch.where(chosen, (m.detach() - pe_id).abs().double(), inf[:, 1:-1, 1:-1])
    if src1 is not None:
        se[:, 1:-1, 1:-1] = torch.where(both_ok, (pe0.detach() - pe1.detach()).abs().double(), inf[:, 1:-1, 1:-1])
    adx, ady = dx.detach().abs().double(), dy.detach().abs().double()
    if s > 1:
        eqx, eqy = structurally_equal(H // s, W // s, s)
        adx = torch.where(eqx.unsqueeze(0), inf[:, :, 1:], adx)
        ady = torch.where(eqy.unsqueeze(0), inf[:, 1:], ady)
    sd = inf.clone()
    sd[:, :, :-1] = torch.minimum(sd[:, :, :-1], adx)
    sd[:, :, 1:] = torch.minimum(sd[:, :, 1:], adx)
    sd[:, :-1] = torch.minimum(sd[:, :-1], ady)
    sd[:, 1:] = torch.minimum(sd[:, 1:], ady)
    d0 = D[..., 0].detach().double()
    clip = torch.minimum((d0 - 0.01).abs(), (d0 - 200.0).abs())
    clip = torch.where(torch.isfinite(clip), clip, inf)
    return {"term": term, "photo": photo, "smooth": sm, "n": n, "sel": computed, "D": D, "pe_id": pe_id,
            "valid": [wp["valid"] for wp in wps], "warped": [wp["warped"] for wp in wps],
            "margins": {"cell": cell, "absdiff": absdiff, "automask": am, "select": se, "smooth": sd, "clip": clip}}


def well_conditioned(margins):
    """[b,H,W] bool at the resolution of D: no local kink within MARGIN (``select`` included; ``automask`` is global)."""
    return R.well_conditioned(margins) & (margins["select"] >= MARGIN)


def coarse_well(well, s):
    """[b,H,W] -> [b,h,w]: a coarse pixel is well conditioned when every fine pixel whose stencil can hold it is (the at most
    2s x 2s window of U_s^T)."""
    if s == 1:
        return well
    bad = (~well).double().unsqueeze(1)
    k = 2 * s
    bad = torch.nn.functional.max_pool2d(torch.nn.functional.pad(bad, (s // 2,) * 4), kernel_size=k, stride=s)
    return bad[:, 0] == 0


# ---- cases ------------------------------------------------------------------------------------------------------------------------
# name -> (full H, full W, s (1 = scale level), seed); b = 2, quaternions, helpers.cameras_np.  The seeds are the first per size
# that meet the conditions tests/test_photometric_full_ref.py asserts.
CASES = {"12x16-s2": (12, 16, 2, 0), "24x40-s2": (24, 40, 2, 0), "32x48-s8": (32, 48, 8, 0), "48x80-s16": (48, 80, 16, 4),
         "24x40-level": (24, 40, 1, 0)}
UPSAMPLE_SHAPES = [(6, 8, 2), (3, 5, 16), (1, 3, 8), (6, 6, 64)]


def _quat(aa):
    ang = np.linalg.norm(aa, axis=1, keepdims=True)
    return np.concatenate([np.cos(ang / 2), aa / np.maximum(ang, 1e-12) * np.sin(ang / 2)], axis=1)


def make_case(name, b=2, seed=None):
    """Random images in [0,1], a coarse depth in [4,12], small rotations, mostly sideways translations (the camera keeps moving:
    the motion of frame t+1 resembles that of frame t, so the two sources see the scene from opposite sides)."""
    H, W, s, sd = CASES[name]
    sd = sd if seed is None else seed
    rng = np.random.default_rng(1000 * H + 10 * W + 100000 * s + sd)
    cam = cameras_np(b, H, W)
    sign = np.array([[1.0], [-1.3]])[:b]
    img = lambda: rng.uniform(0.0, 1.0, [b, H, W, 3]).astype(np.float32)
    f32 = lambda a: np.asarray(a, np.float32)
    return {"name": name, "s": s, "depth": rng.uniform(4.0, 12.0, [b, H // s, W // s, 1]).astype(np.float32),
            "rot0": f32(_quat(rng.normal(0.0, 0.01, [b, 3]))), "trans0": f32(rng.normal([0.35, -0.1, 0.05], 0.03, [b, 3]) * sign),
            "rot1": f32(_quat(rng.normal(0.0, 0.01, [b, 3]))), "trans1": f32(rng.normal([0.3, 0.12, 0.04], 0.03, [b, 3]) * sign),
            "f": cam["f"], "c": cam["c"], "cur": img(), "prev": img(), "next": img()}


def case_tensors(case, dtype):
    return {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in case.items() if k not in ("name", "s", "true")}


def term_and_grad(case, dtype, smooth=1e-3, automask=True, sel=None, two=True, **planted):
    """(result dict, g_depth [b,h,w,1], g_D [b,H,W,1]) of multi_term on a case, in ``dtype``; ``two`` = both sources."""
    t = case_tensors(case, dtype)
    depth = t["depth"].clone().requires_grad_(True)
    extra = dict(src1=t["next"], rot1=t["rot1"], trans1=t["trans1"]) if two else {}
    res = multi_term(depth, case["s"], t["rot0"], t["trans0"], t["f"], t["c"], t["cur"], t["prev"], smooth=smooth, automask=automask,
                     sel=sel, **extra, **planted)
    if case["s"] > 1:
        g, g_D = torch.autograd.grad(res["term"], [depth, res["D"]])
    else:
        g, = torch.autograd.grad(res["term"], depth)
        g_D = g
    return res, g, g_D


def term_and_grad_free(case, dtype, automask=True):
    """multi_term on a case with both sources and no gradient (for cases whose restated term is not finite: torch.clamp keeps
    a NaN that the kernels' fmaxf / fminf clip to 0.01, so only validity, selection and N are compared there)."""
    t = case_tensors(case, dtype)
    with torch.no_grad():
        return multi_term(t["depth"], case["s"], t["rot0"], t["trans0"], t["f"], t["c"], t["cur"], t["prev"], src1=t["next"],
                          rot1=t["rot1"], trans1=t["trans1"], automask=automask)


def yardstick_of(case, two=True):
    """photometric_ref.yardstick for a case of this file: ``loss`` = the float32 restatement's largest relative error of (term,
    photo, smooth) over both auto-mask settings, ``grad`` / ``grad_D`` = its largest |g32 - g64| / max |g64| over the
    well-conditioned coarse / fine pixels of both.  ``ref[automask]`` = (result, g_depth, g_D, coarse well, fine well), float64."""
    out = {"loss": 0.0, "grad": 0.0, "grad_D": 0.0, "ref": {}, "case": case}
    for am in (True, False):
        r64, g64, gD64 = term_and_grad(case, torch.float64, automask=am, two=two)
        r32, g32, gD32 = term_and_grad(case, torch.float32, automask=am, two=two)
        well = well_conditioned(r64["margins"])
        cw = coarse_well(well, case["s"])
        for k in ("term", "photo", "smooth"):
            if r64[k].item() == 0.0:                   # nothing in view: photo is exactly 0 on both sides
                assert r32[k].item() == 0.0
                continue
            out["loss"] = max(out["loss"], abs(r32[k].item() - r64[k].item()) / abs(r64[k].item()))
        out["grad"] = max(out["grad"], ((g32.double() - g64).abs()[..., 0][cw].max() / g64.abs().max()).item())
        out["grad_D"] = max(out["grad_D"], ((gD32.double() - gD64).abs()[..., 0][well].max() / gD64.abs().max()).item())
        out["ref"][am] = (r64, g64, gD64, cw, well)
    return out


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """``yardstick_of`` the named case of CASES, both sources; computed once and shared."""
    return yardstick_of(make_case(name))


def out_of_view(case, which):
    """``which`` = "next" or "both": a 400-unit translation throws every query of that source out of the image.  The next
    frame's motion is inverted, so its translation is given the other sign."""
    case = dict(case)
    far = np.array([[400.0, 0.0, 0.0], [0.0, -300.0, 0.0]], np.float32)
    case["trans1"] = -far
    if which == "both":
        case["trans0"] = far
    case["name"] = case["name"] + "-" + which + "-out-of-view"
    return case


def hostile_case():
    """photometric_ref.hostile_depth_case's depths (0.001, 250, -3, +-Inf, 0, 1e-6, 1e4) in a 6x10 map upsampled by 8 (48x80),
    with its motions: part of sample 0 out of view, part of sample 1 behind the camera."""
    rng = np.random.default_rng(77)
    b, h, w, s = 2, 6, 10, 8
    cam = cameras_np(b, h * s, w * s)
    d = rng.uniform(4.0, 12.0, [b, h, w, 1]).astype(np.float32)
    d[0, 2, 3:9, 0] = [0.001, 250.0, -3.0, np.inf, 0.0, -np.inf]
    d[1, 4, 1:5, 0] = [1e-6, 1e4, -0.5, np.inf]
    img = lambda: rng.uniform(0.0, 1.0, [b, h * s, w * s, 3]).astype(np.float32)
    ident = np.array([[1.0, 0.0, 0.0, 0.0]] * b, np.float32)
    return {"name": "hostile", "s": s, "depth": d, "rot0": ident, "trans0": np.array([[3.0, 0.4, 0.2], [0.2, -0.1, -7.0]], np.float32),
            "rot1": ident, "trans1": np.array([[0.3, 0.1, 0.05], [-0.4, 0.1, 0.0]], np.float32), "f": cam["f"], "c": cam["c"],
            "cur": img(), "prev": img(), "next": img()}


# ---- the whole loss -----------------------------------------------------------------------------------------------------------------
def loss(samples, depths, camera, smooth=1e-3, automask=True, dtype=torch.float64, scale="level", sources="prev", **planted):
    """training.photometric_loss with its options; as photometric_ref.loss otherwise."""
    T = len(samples)
    cv = lambda a: a.to(dtype) if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a)).to(dtype)
    L = len(depths[1])
    frames = [cv(s["RGB_im"]) for s in samples]
    pyrs = [R.image_pyramid(fr, L) for fr in frames] if scale == "level" else None
    total, results = 0.0, {}
    for t in range(1, T):
        for i in range(L):
            k = 2 ** (i + 1)
            if scale == "level":
                f, c, s, img = cv(camera["f"]) / float(k), cv(camera["c"]) / float(k), 1, lambda u: pyrs[u][i]
            else:
                f, c, s, img = cv(camera["f"]), cv(camera["c"]), k, lambda u: frames[u]
            extra = {}
            if sources == "both" and t < T - 1:
                extra = dict(src1=img(t + 1), rot1=cv(samples[t + 1]["rot"]), trans1=cv(samples[t + 1]["trans"]))
            res = multi_term(cv(depths[t][i]), s, cv(samples[t]["rot"]), cv(samples[t]["trans"]), f, c, img(t), img(t - 1),
                             smooth=smooth, automask=automask, **extra, **planted)
            total = total + res["term"] * ((0.64 / 2.0 ** (i - 1)) / float(T - 1))
            results[(t, i)] = res
    return total, results


# (scale, sources) -> (levels, seed) of the end-to-end cases: the first seed whose every term meets the conditions
LOSS_CASES = {("full", "both"): (3, 19), ("full", "prev"): (2, 17), ("level", "both"): (2, 0), ("level", "prev"): (2, 0)}


def loss_case(scale="full", sources="both", b=2, T=3, H=48, W=80):
    """The end-to-end case: T random frames, per-sample cameras, small quaternion motions, depths in [4,12] for every level."""
    L, seed = LOSS_CASES[(scale, sources)]
    rng = np.random.default_rng(500 + seed)
    cam = cameras_np(b, H, W)
    samples = []
    for t in range(T):
        samples.append({"RGB_im": rng.uniform(0.0, 1.0, [b, H, W, 3]).astype(np.float32),
                        "rot": _quat(rng.normal(0.0, 0.01, [b, 3])).astype(np.float32),
                        "trans": rng.normal([0.3, 0.1, 0.05], 0.03, [b, 3]).astype(np.float32)})
    depths = [[rng.uniform(4.0, 12.0, [b, H >> (i + 1), W >> (i + 1), 1]).astype(np.float32) for i in range(L)] for t in range(T)]
    return samples, depths, cam


def loss_and_grads(samples, depths, camera, dtype, **kw):
    """(loss, {(t, i): g_depth}, {(t, i): result}) of ``loss`` in ``dtype`` by autodiff."""
    leaves = [[torch.from_numpy(d).to(dtype).requires_grad_(True) for d in lv] for lv in depths]
    total, results = loss(samples, leaves, camera, dtype=dtype, **kw)
    keys = sorted(results)
    grads = torch.autograd.grad(total, [leaves[t][i] for t, i in keys])
    return total.detach(), dict(zip(keys, grads)), results


# ---- the optimisation scene ---------------------------------------------------------------------------------------------------------
def learn_scene(s, b=2, H=48, W=80):
    """A textured 3-D plane n . X = d0 (in the current camera's frame) rendered analytically into the previous, the current and
    the next camera by ray-plane intersection, float64.  The texture is a smooth sum of sinusoids of the plane point's (X, Y).
    ``true`` is the plane's depth at the centres of the coarse pixels ([b, H/s, W/s, 1]); the start is 1.25 x that."""
    cam = cameras_np(b, H, W)
    f, c = cam["f"].astype(np.float64), cam["c"].astype(np.float64)
    normals = np.array([[-0.10, -0.06, 1.0], [0.08, -0.05, 1.0]])[:b]
    d0 = np.array([6.0, 7.8])[:b]
    ident = np.array([[1.0, 0.0, 0.0, 0.0]] * b)
    rot0, trans0 = ident, np.array([[0.35, 0.03, 0.0], [-0.33, 0.05, 0.01]])[:b]
    rot1, trans1 = _quat(np.array([[0.0, 0.004, 0.0], [0.002, 0.0, 0.0]])[:b]), np.array([[0.33, -0.04, 0.01], [-0.35, 0.03, 0.0]])[:b]
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    inv1 = [a.numpy() for a in motion_inverse(t64(rot1), t64(trans1))]

    def texture(X, Y):
        return np.stack([0.5 + 0.25 * np.sin(2.2 * X + 0.3 * k) * np.cos(1.9 * Y - 0.2 * k) + 0.2 * np.sin(0.9 * (X + Y) + k)
                         for k in range(3)], axis=-1)

    def render(rot, trans, h, w, fk, ck):
        """(image [b,h,w,3], depth of the plane along the camera's own z [b,h,w]) of the camera X_cam = R X_cur + t."""
        jj, ii = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        imgs, zs = [], []
        for bi in range(b):
            Rm = np.array([r[bi].item() for r in R.rot_mat(t64(rot))]).reshape(3, 3)
            ray = np.stack([(ii + 0.5 - ck[bi, 0]) / fk[bi, 0], (jj + 0.5 - ck[bi, 1]) / fk[bi, 1], np.ones_like(ii)], axis=-1)
            n_cam = Rm @ normals[bi]                                   # n . R^T v = (R n) . v
            lam = (d0[bi] + n_cam @ trans[bi]) / (ray @ n_cam)
            Xc = (lam[..., None] * ray - trans[bi]) @ Rm               # R^T (lam r - t), row-vector form
            imgs.append(texture(Xc[..., 0], Xc[..., 1]))
            zs.append(lam)
        return np.stack(imgs, 0), np.stack(zs, 0)

    zero = np.zeros([b, 3])
    cur, _ = render(ident, zero, H, W, f, c)
    prev, _ = render(rot0, trans0, H, W, f, c)
    nxt, _ = render(inv1[0], inv1[1], H, W, f, c)
    _, true = render(ident, zero, H // s, W // s, f / s, c / s)
    f32 = lambda a: np.asarray(a, np.float32)
    true = true[..., None]
    return {"name": f"learn-s{s}", "s": s, "depth": f32(1.25 * true), "true": f32(true), "rot0": f32(rot0), "trans0": f32(trans0),
            "rot1": f32(rot1), "trans1": f32(trans1), "f": cam["f"], "c": cam["c"], "cur": f32(cur), "prev": f32(prev), "next": f32(nxt)}
