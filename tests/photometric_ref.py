"""Restatement of the photometric reprojection loss (include/m4depth_hip.h, "Photometric reprojection loss") with torch CPU
tensors.  Autodiff stands for the backward; the dtype is a parameter (float64 = the reference, float32 = the yardstick of
float32's own error, and -- operation for operation in the kernels' order -- the bitwise reference of `warped` / `valid`).

Besides the loss it returns per-pixel *conditioning margins*: how far the inputs are from a kink of the definition (a cell
border of the bilinear sample, |warped - cur| = 0, the auto-mask comparison, a zero smoothness difference, the clip bounds).
A kink is local -- a flipped cell, |.| sign or `inside` changes only that pixel's gradient -- except the mask: a flipped mask
bit changes N and with it every gradient.
"""
import functools

import numpy as np
import torch

from helpers import cameras_np

C1, C2 = 0.01 ** 2, 0.03 ** 2
MARGIN = 1e-5


def rot_mat(rot):
    """m4d_load_motion's rotation, same operation order: [b,3] small angle or [b,4] quaternion (w,x,y,z) -> 9 x [b]."""
    one = torch.ones_like(rot[:, 0])
    if rot.shape[1] == 3:
        r0, r1, r2 = rot.unbind(-1)
        return (one, -r2, r1, r2, one, -r0, -r1, r0, one)
    w, x, y, z = rot.unbind(-1)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return (1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx, txz - twy, tyz + twx,
            1.0 - (txx + tyy))


def image_pyramid(img, levels):
    """[n,H,W,3] -> list of levels, each the 2x2 mean ((a + b) + (c + d)) * 0.25 of the one before."""
    out = []
    for _ in range(levels):
        a, b = img[:, 0::2, 0::2], img[:, 0::2, 1::2]
        c, d = img[:, 1::2, 0::2], img[:, 1::2, 1::2]
        img = ((a + b) + (c + d)) * 0.25
        out.append(img)
    return out


def warp(depth, rot, trans, f, c, prev, drop_px_c=False, camera_of_sample0=False):
    """depth [b,h,w,1], prev [b,h,w,3] -> dict(warped, valid, qx, qy, pz, dc).  The planted errors: ``drop_px_c`` detaches the
    Px C term of dq/ddc; ``camera_of_sample0`` reads sample 0's intrinsics for every sample."""
    b, h, w, _ = depth.shape
    dt = depth.dtype
    if camera_of_sample0:
        f, c = f[:1].expand(b, 2), c[:1].expand(b, 2)
    v = lambda t: t.reshape(b, 1, 1)
    r00, r01, r02, r10, r11, r12, r20, r21, r22 = [v(r) for r in rot_mat(rot)]
    fx, fy, cx, cy = v(f[:, 0]), v(f[:, 1]), v(c[:, 0]), v(c[:, 1])
    tx, ty, tz = v(trans[:, 0]), v(trans[:, 1]), v(trans[:, 2])
    dc = torch.clamp(depth[..., 0], 0.01, 200.0)
    jj = torch.arange(h, dtype=dt).reshape(1, h, 1)
    ii = torch.arange(w, dtype=dt).reshape(1, 1, w)
    mx = (ii + 0.5) - cx
    my = (jj + 0.5) - cy
    pos0, pos1, pos2 = (mx / fx) * dc, (my / fy) * dc, 1.0 * dc
    rows = ((fx * r00, fx * r01, fx * r02, fx * tx), (fy * r10, fy * r11, fy * r12, fy * ty), (r20, r21, r22, tz))
    pr = [((m0 * pos0 + m1 * pos1) + m2 * pos2) + m3 * 1.0 for m0, m1, m2, m3 in rows]
    pz_den = pr[2].detach() if drop_px_c else pr[2]
    px, py = pr[0] / pz_den, pr[1] / pz_den
    qy = jj + (py - my)
    qx = ii + (px - mx)
    fly = torch.clamp(torch.floor(qy.detach()), 0.0, float(h - 2))
    flx = torch.clamp(torch.floor(qx.detach()), 0.0, float(w - 2))
    fly, flx = torch.nan_to_num(fly, nan=0.0), torch.nan_to_num(flx, nan=0.0)      # fmaxf(0, NaN) = 0 in the kernels
    ay = torch.clamp(qy - fly, 0.0, 1.0).unsqueeze(-1)
    ax = torch.clamp(qx - flx, 0.0, 1.0).unsqueeze(-1)
    y0, x0 = fly.long(), flx.long()
    bi = torch.arange(b).reshape(b, 1, 1).expand(b, h, w)
    tl, tr = prev[bi, y0, x0], prev[bi, y0, x0 + 1]
    bl, br = prev[bi, y0 + 1, x0], prev[bi, y0 + 1, x0 + 1]
    top = ax * (tr - tl) + tl
    bot = ax * (br - bl) + bl
    warped = ay * (bot - top) + top
    valid = ((pr[2] > 0) & (qx >= 0) & (qx <= w - 1) & (qy >= 0) & (qy <= h - 1) & torch.isfinite(depth[..., 0])).detach()
    return {"warped": warped, "valid": valid, "qx": qx.detach(), "qy": qy.detach(), "pz": pr[2].detach(), "dc": dc}


def _win(t):
    """Sum over the 3x3 window at the interior pixels: [b,h,w,...] -> [b,h-2,w-2,...]."""
    h, w = t.shape[1:3]
    s = 0.0
    for dy in range(3):
        for dx in range(3):
            s = s + t[:, dy:h - 2 + dy, dx:w - 2 + dx]
    return s


def photo_error(x, y, drop_mu=False):
    """pe(x, y) at the interior pixels, [b,h-2,w-2].  ``drop_mu`` (planted error): the window means carry no gradient."""
    mx, my = _win(x) / 9.0, _win(y) / 9.0
    if drop_mu:
        mx = mx.detach()
    vx, vy = _win(x * x) / 9.0 - mx * mx, _win(y * y) / 9.0 - my * my
    cxy = _win(x * y) / 9.0 - mx * my
    ssim = ((2.0 * mx * my + C1) * (2.0 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    l1 = (x - y).abs()[:, 1:-1, 1:-1]
    return (0.85 * (1.0 - ssim) / 2.0 + 0.15 * l1).mean(dim=-1)


def level_term(depth, rot, trans, f, c, cur, prev, smooth=1e-3, automask=True, mask=None, ignore_valid=False, **planted):
    """One level's term and everything the tests compare.  ``mask`` (optional, [b,h,w] bool) replaces the computed one."""
    b, h, w, _ = depth.shape
    wp = warp(depth, rot, trans, f, c, prev, **{k: v for k, v in planted.items() if k != "drop_mu"})
    pe_w = photo_error(wp["warped"], cur, drop_mu=planted.get("drop_mu", False))
    pe_p = photo_error(prev, cur)
    all9 = _win(wp["valid"].to(depth.dtype)) == 9.0
    if ignore_valid:
        all9 = torch.ones_like(all9)
    m_in = all9 & (pe_w.detach() < pe_p) if automask else all9
    computed = torch.zeros((b, h, w), dtype=torch.bool)
    computed[:, 1:-1, 1:-1] = m_in
    used = computed if mask is None else mask
    mf = used[:, 1:-1, 1:-1].to(depth.dtype)
    n = mf.sum()
    photo = (mf * pe_w).sum() / torch.clamp(n, min=1.0)
    ld = torch.log(wp["dc"])
    ex = torch.exp(-(cur[:, :, 1:] - cur[:, :, :-1]).abs().mean(dim=-1))
    ey = torch.exp(-(cur[:, 1:] - cur[:, :-1]).abs().mean(dim=-1))
    dx, dy = ld[:, :, 1:] - ld[:, :, :-1], ld[:, 1:] - ld[:, :-1]
    sm = ((dx.abs() * ex).sum() + (dy.abs() * ey).sum()) / float(b * h * w)
    term = photo + smooth * sm
    # ---- margins
    inf = torch.full((b, h, w), float("inf"), dtype=torch.float64)
    qx, qy = wp["qx"].double(), wp["qy"].double()
    cell = torch.minimum((qx - torch.round(qx)).abs(), (qy - torch.round(qy)).abs())
    cell = torch.minimum(cell, wp["pz"].double().abs())
    cell = torch.where(torch.isfinite(cell), cell, torch.zeros_like(cell))
    absdiff = (wp["warped"].detach() - cur).abs().min(dim=-1).values.double()
    am = inf.clone()
    if automask:
        am[:, 1:-1, 1:-1] = torch.where(all9, (pe_w.detach() - pe_p).abs().double(), inf[:, 1:-1, 1:-1])
    sd = inf.clone()
    adx, ady = dx.detach().abs().double(), dy.detach().abs().double()
    sd[:, :, :-1] = torch.minimum(sd[:, :, :-1], adx)
    sd[:, :, 1:] = torch.minimum(sd[:, :, 1:], adx)
    sd[:, :-1] = torch.minimum(sd[:, :-1], ady)
    sd[:, 1:] = torch.minimum(sd[:, 1:], ady)
    d0 = depth[..., 0].detach().double()
    clip = torch.minimum((d0 - 0.01).abs(), (d0 - 200.0).abs())
    clip = torch.where(torch.isfinite(clip), clip, inf)
    return {"term": term, "photo": photo, "smooth": sm, "n": n, "mask": computed, "warped": wp["warped"], "valid": wp["valid"],
            "pe_w": pe_w, "pe_p": pe_p,
            "margins": {"cell": cell, "absdiff": absdiff, "automask": am, "smooth": sd, "clip": clip}}


def well_conditioned(margins):
    """[b,h,w] bool: no local kink within MARGIN of the pixel (the auto-mask margin is global and asserted separately)."""
    return ((margins["cell"] >= MARGIN) & (margins["absdiff"] >= MARGIN) & (margins["smooth"] >= MARGIN)
            & (margins["clip"] >= MARGIN))


def term_and_grad(case, dtype, smooth=1e-3, automask=True, mask=None, **planted):
    """(result dict, g_depth [b,h,w,1]) of level_term on a case of make_case, in ``dtype``."""
    t = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in case.items() if k not in ("name",)}
    depth = t["depth"].clone().requires_grad_(True)
    res = level_term(depth, t["rot"], t["trans"], t["f"], t["c"], t["cur"], t["prev"], smooth, automask, mask, **planted)
    g, = torch.autograd.grad(res["term"], depth)
    return res, g


def loss(samples, depths, camera, smooth=1e-3, automask=True, dtype=torch.float64):
    """photometric_loss: samples[t] = dict(RGB_im [b,H,W,3], rot, trans), depths[t][i] [b,h_i,w_i,1] (torch, may require
    grad), camera = dict(f, c) full resolution.  Level i weighs (0.64 / 2**(i-1)) / (T-1)."""
    T = len(samples)
    cv = lambda a: a.to(dtype) if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a)).to(dtype)
    L = len(depths[1])
    pyrs = [image_pyramid(cv(s["RGB_im"]), L) for s in samples]
    total, results = 0.0, {}
    for t in range(1, T):
        for i in range(L):
            k = 2.0 ** (i + 1)
            res = level_term(cv(depths[t][i]), cv(samples[t]["rot"]), cv(samples[t]["trans"]), cv(camera["f"]) / k,
                             cv(camera["c"]) / k, pyrs[t][i], pyrs[t - 1][i], smooth, automask)
            total = total + res["term"] * ((0.64 / 2.0 ** (i - 1)) / float(T - 1))
            results[(t, i)] = res
    return total, results


def loss_case(seed=7, b=2, T=3, H=48, W=80, L=2):
    """The end-to-end case: T random frames, per-sample cameras, small motions, depths [4,12] for every level of every frame."""
    rng = np.random.default_rng(seed)
    cam = cameras_np(b, H, W)
    samples = []
    for t in range(T):
        aa = rng.normal(0.0, 0.01, [b, 3])
        samples.append({"RGB_im": rng.uniform(0.0, 1.0, [b, H, W, 3]).astype(np.float32), "rot": aa.astype(np.float32),
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


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """The float32 restatement's error to the float64 one on case ``name``: the bars of the GPU tests are 4 x these.  A case is
    a geometry; both auto-mask settings belong to it, and the loss has three reported parts, so ``loss`` is the largest
    relative error of (term, photo, smooth) over both settings and ``grad`` the largest |g32 - g64| / max |g64| over the
    well-conditioned pixels of both.  Also returns the float64 results: ``ref[automask]`` = (result, g_depth, well)."""
    case = make_case(name) if name in CASES else {"out-of-view": out_of_view_case}[name]()
    out = {"loss": 0.0, "grad": 0.0, "ref": {}, "case": case}
    for am in (True, False):
        r64, g64 = term_and_grad(case, torch.float64, automask=am)
        r32, g32 = term_and_grad(case, torch.float32, automask=am)
        well = well_conditioned(r64["margins"])
        for k in ("term", "photo", "smooth"):
            if r64[k].item() == 0.0:                   # nothing in view: photo is exactly 0 on both sides
                assert r32[k].item() == 0.0
                continue
            out["loss"] = max(out["loss"], abs(r32[k].item() - r64[k].item()) / abs(r64[k].item()))
        out["grad"] = max(out["grad"], ((g32.double() - g64).abs()[..., 0][well].max() / g64.abs().max()).item())
        out["ref"][am] = (r64, g64, well)
    return out


# ---- the cases the CPU and the GPU tests share ------------------------------------------------------------------------------
# name -> (h, w, quaternion?, seed).  The seeds are chosen (tests/test_photometric_ref.py asserts it) so that the float64
# restatement has no pixel with an auto-mask margin below MARGIN and at most 1 % of pixels with any other margin below it.
CASES = {"6x8-quat": (6, 8, True, 0), "6x8-angle": (6, 8, False, 1), "13x21-quat": (13, 21, True, 0),
         "13x21-angle": (13, 21, False, 1), "24x40-quat": (24, 40, True, 0), "24x40-angle": (24, 40, False, 1)}


def make_case(name, b=2):
    """Random images in [0,1], depth in [4,12], a small rotation, a mostly sideways translation scaled with the map so that
    the flow is a few tenths of a pixel to a few pixels; per-sample off-centre cameras (helpers.cameras_np)."""
    h, w, quat, seed = CASES[name]
    rng = np.random.default_rng(1000 * h + 10 * w + seed)
    cam = cameras_np(b, h, w)
    aa = rng.normal(0.0, 0.01, [b, 3])
    if quat:
        ang = np.linalg.norm(aa, axis=1, keepdims=True)
        rot = np.concatenate([np.cos(ang / 2), aa / np.maximum(ang, 1e-12) * np.sin(ang / 2)], axis=1)
    else:
        rot = aa
    trans = rng.normal([0.35, -0.1, 0.05], 0.03, [b, 3]) * np.array([[1.0], [-1.3]])[:b]
    return {"name": name, "depth": rng.uniform(4.0, 12.0, [b, h, w, 1]).astype(np.float32),
            "rot": rot.astype(np.float32), "trans": trans.astype(np.float32), "f": cam["f"], "c": cam["c"],
            "cur": rng.uniform(0.0, 1.0, [b, h, w, 3]).astype(np.float32),
            "prev": rng.uniform(0.0, 1.0, [b, h, w, 3]).astype(np.float32)}


def out_of_view_case(h=13, w=21, b=2):
    """Everything out of view: a translation that throws every query far outside the image (N = 0)."""
    case = make_case("13x21-quat", b)
    case["trans"] = np.array([[400.0, 0.0, 0.0], [0.0, -300.0, 0.0]], np.float32)[:b]
    case["name"] = "out-of-view"
    return case


def hostile_depth_case():
    """make_case('13x21-angle') with depths outside [0.01, 200], negative and infinite ones, and a motion that pushes part of
    the image out of view (sample 0) and part of it behind the camera, Pz <= 0 (sample 1)."""
    case = make_case("13x21-angle")
    d = case["depth"]
    d[0, 2, 3:9, 0] = [0.001, 250.0, -3.0, np.inf, 0.0, -np.inf]
    d[1, 5, 1:5, 0] = [1e-6, 1e4, -0.5, np.inf]
    case["trans"] = np.array([[3.0, 0.4, 0.2], [0.2, -0.1, -7.0]], np.float32)
    case["name"] = "hostile"
    return case


def stationary_case(h=13, w=21):
    """make_case('13x21-quat') with sample 0 STATIONARY -- identity rotation, zero translation, the case of a hovering drone --
    beside the moving sample 1.  Sample 0's camera is dyadic (f = (16, 8), c = (10.25, 6.75)) and its depths are powers of two
    (2^(1 + (j + 2 i) mod 4): no two neighbours equal, so the smoothness term sits on no kink), which makes its projection
    EXACT in float32 and float64 alike: every query is the pixel's own centre, every pixel is valid, d query / d depth is exactly
    0, and ``warped`` is ``prev`` bit for bit except in the last row and column (read with weight 1 from the cell before:
    a * (r - l) + l is r to an ulp).  Without that the validity of the border pixels (q >= 0 against q = 0 -+ one
    ulp) is decided by last-bit noise and no two evaluations agree on the mask.  The weight of the bilinear cell is 0 / 1 on a
    cell border everywhere (the ``cell`` margin is 0), but with d query / d depth = 0 the choice of cell carries no gradient:
    ``stationary_well`` leaves the cell margin out for sample 0."""
    case = make_case("13x21-quat")
    jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    case["depth"][0, ..., 0] = 2.0 ** (1 + (jj + 2 * ii) % 4)
    case["rot"][0] = [1.0, 0.0, 0.0, 0.0]
    case["trans"][0] = 0.0
    case["f"], case["c"] = case["f"].copy(), case["c"].copy()
    case["f"][0], case["c"][0] = [16.0, 8.0], [10.25, 6.75]
    case["name"] = "stationary"
    return case


def stationary_well(margins):
    """``well_conditioned`` for stationary_case: sample 0 without the cell margin (see there)."""
    well = well_conditioned(margins)
    well[0] = ((margins["absdiff"] >= MARGIN) & (margins["smooth"] >= MARGIN) & (margins["clip"] >= MARGIN))[0]
    return well


@functools.lru_cache(maxsize=None)
def stationary_yardstick():
    """``yardstick`` for stationary_case with ``automask=False`` (with the auto-mask sample 0's mask compares pe(warped, cur)
    with pe(prev, cur) where warped == prev: nothing to compare it with)."""
    case = stationary_case()
    r64, g64 = term_and_grad(case, torch.float64, automask=False)
    r32, g32 = term_and_grad(case, torch.float32, automask=False)
    well = stationary_well(r64["margins"])
    out = {"case": case, "ref": (r64, g64, well), "r32": r32}
    out["loss"] = max(abs(r32[k].item() - r64[k].item()) / abs(r64[k].item()) for k in ("term", "photo", "smooth"))
    out["grad"] = ((g32.double() - g64).abs()[..., 0][well].max() / g64.abs().max()).item()
    return out


def learn_case(b=2, h=24, w=40):
    """The optimisation setup: prev a smooth sinusoid texture, cur = prev warped with a sloped plane (6 + 0.08 x + 0.05 y,
    second sample x 1.3), translation about 0.35 sideways, start 1.25 x the true depth."""
    cam = cameras_np(b, h, w)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    prev = np.stack([0.5 + 0.25 * np.sin(0.55 * xx + 0.3 * k) * np.cos(0.45 * yy - 0.2 * k) + 0.2 * np.sin(0.23 * (xx + yy) + k)
                     for k in range(3)], axis=-1)
    prev = np.stack([prev, prev[:, ::-1].copy()], 0)[:b]
    true = (6.0 + 0.08 * xx + 0.05 * yy)[None, :, :, None] * np.array([1.0, 1.3])[:b].reshape(b, 1, 1, 1)
    rot = np.zeros([b, 3])
    trans = np.array([[0.35, 0.03, 0.0], [-0.33, 0.05, 0.01]])[:b]
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    cur = warp(t64(true), t64(rot), t64(trans), t64(cam["f"]), t64(cam["c"]), t64(prev))["warped"].numpy()
    f32 = lambda a: np.asarray(a, np.float32)
    return {"name": "learn", "depth": f32(1.25 * true), "true": f32(true), "rot": f32(rot), "trans": f32(trans), "f": cam["f"],
            "c": cam["c"], "cur": f32(cur), "prev": f32(prev)}


def median_error(depth, true, border=2):
    """Median and 90th percentile of |depth / true - 1| over the pixels more than ``border`` from the border."""
    e = np.abs(np.asarray(depth, np.float64) / np.asarray(true, np.float64) - 1.0)[:, border + 1:-border - 1, border + 1:-border - 1]
    return float(np.median(e)), float(np.percentile(e, 90))


def optimise(case, term_fn, dtype=torch.float64, dev="cpu", steps=100, lr=0.02):
    """Adam on log depth, no network: ``term_fn(depth [b,h,w,1] requiring grad) -> scalar``.  Returns the final depth (numpy)."""
    ld =torch.log(torch.from_numpy(case["depth"]).to(dtype)).to(dev).requires_grad_(True)
    opt = torch.optim.Adam([ld], lr=lr)
    for _ in range(steps):
        opt.zero_grad()
        term_fn(torch.exp(ld)).backward()
        opt.step()
    return torch.exp(ld).detach().cpu().numpy()
