"""The training graph: M4Depth.call(training=True), m4depth_loss and train_step
(m4depth_network.py:278-323, 351-365, 371-431, 491-536).

Division of labour.  The reference lets tf.GradientTape differentiate its whole Python graph.
Here torch autograd records the graph, and the nodes that carry the work are HIP:

  * cost volumes: ``get_parallax_sweeping_cv`` / ``cost_volume`` forward and backward kernels
    (m4d_dscv_fwd/bwd, m4d_sncv_fwd/bwd);
  * convolutions: forward = the fp32-MFMA implicit GEMM with fused bias + leaky_relu (every layer, the 3-channel
    image layer included); data gradient = the SAME kernel run on the 180-degree-rotated, transposed
    weights (a 3x3 'SAME' stride-1 correlation is its own adjoint up to that re-packing; for a stride-2
    layer the incoming gradient is first spread onto the input grid, m4d_dilate2); weight gradient = the
    fp32-MFMA kernel of csrc/m4d_wgrad.hip (K = pixels, fixed-order two-stage reduction).  No MIOpen /
    framework convolution is left in the training step;
  * the per-pixel glue (upsampling, log/exp, parallax<->depth) is a handful of elementwise
    torch ops on the device -- they are < 1 % of a training step.

There is no CPU path: every tensor must live on the MI355X.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from . import network_ops as nops
from ._lib import lib, dptr, stream_ptr, check, as_f32
from .depth_operations import get_parallax_sweeping_cv, cost_volume, prev_d2para, depth2parallax

def _same_pads(h, w, s):
    ph = max((-(-h // s) - 1) * s + 3 - h, 0)
    pw = max((-(-w // s) - 1) * s + 3 - w, 0)
    return ph // 2, ph - ph // 2, pw // 2, pw - pw // 2


def _packed(cache, weight, transpose):
    """(wp, n_pad) of the live parameter, re-packed by one HIP kernel per optimizer step."""
    key = ("bwd" if transpose else "fwd", weight.data_ptr(), weight._version)
    hit = cache.get(key)
    if hit is None:
        O, I = weight.shape[0], weight.shape[1]
        w_ohwi = weight.detach().permute(0, 2, 3, 1).contiguous()      # a view of the channels-last parameter
        K, N = (O, I) if transpose else (I, O)
        n_pad = -(-N // 32) * 32
        wp = torch.empty((-(-K // 16), 9, n_pad, 16), dtype=torch.float32, device=weight.device)
        check(lib.m4d_pack_conv_weights(dptr(w_ohwi, "weight"), O, I, int(transpose), dptr(wp), stream_ptr()),
              "m4d_pack_conv_weights")
        hit = (wp, n_pad)
        cache[key] = hit
    return hit


def _packed_lat(cache, weight, transpose):
    """The parameter in m4d_conv3x3_lat's fragment-major bf16-split layout (int16 bits), re-packed on the device per step."""
    key = ("bwd_lat" if transpose else "fwd_lat", weight.data_ptr(), weight._version)
    hit = cache.get(key)
    if hit is None:
        O, I = weight.shape[0], weight.shape[1]
        w_ohwi = weight.detach().permute(0, 2, 3, 1).contiguous()
        K, N = (O, I) if transpose else (I, O)
        hit = torch.empty((-(-N // 32), -(-K // 16), 9, 3, 64, 8), dtype=torch.int16, device=weight.device)
        check(lib.m4d_pack_conv_weights_lat(dptr(w_ohwi, "weight"), O, I, int(transpose), dptr(hit, "wp", torch.int16), stream_ptr()),
              "m4d_pack_conv_weights_lat")
        cache[key] = hit
    return hit


def _lat_ok(b, h, w, cin, stride):
    """Small maps (the coarse levels of a training crop) run forward and data gradient on the latency-first kernel
    (csrc/m4d_convlat.hip: float32 operands as exact 3 x bf16 splits) instead of the fp32-MFMA split-K pair."""
    from . import network as net
    return (stride == 1 and net.conv_arith in net._SPLIT_ARITHS and cin >= 16 and cin % 4 == 0 and b * h * w <= net.lat_conv_max_pixels
            and train_lat_convs)


import os as _os
train_lat_convs = _os.environ.get("M4D_TRAIN_LAT_CONVS", "1") == "1"


class _ConvBiasAct(torch.autograd.Function):
    """leaky_relu(conv3x3_same_tf(x, w) + bias, slope) on NHWC activations, OIHW weights (channels-last strides)."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, slope, cache):
        cout = weight.shape[0]
        b, h, w, cin = x.shape
        if _lat_ok(b, h, w, cin, stride):
            out = nops.conv3x3_lat(x, _packed_lat(cache, weight, False), bias.detach(), cout, slope, final=True)
        else:
            wp, n_pad = _packed(cache, weight, False)
            out = nops.conv3x3_bias_act(x, wp, bias.detach(), cout, n_pad, slope, stride=stride)
        ctx.save_for_backward(x, weight, out)
        ctx.cfg = (stride, slope, cache)
        return out

    @staticmethod
    def backward(ctx, g):
        x, weight, out = ctx.saved_tensors
        stride, slope, cache = ctx.cfg
        b, h, w, cin = x.shape
        cout = weight.shape[0]
        oh, ow = out.shape[1:3]
        g = as_f32(g, "grad")
        rows = g.numel() // cout
        # epilogue backward: leaky_relu mask (tf.nn.leaky_relu: features > 0 ? g : alpha*g) + bias gradient, one pass
        gp = torch.empty_like(g)
        g_bias = torch.empty(cout, dtype=torch.float32, device=g.device)
        ws = nops._workspace("bias_bwd", 4 * int(lib.m4d_bias_act_bwd_workspace_floats(rows, cout)), g.device)
        check(lib.m4d_bias_act_bwd(dptr(g, "grad"), dptr(out), rows, cout, float(slope), dptr(gp), dptr(g_bias), dptr(ws),
                                   stream_ptr()), "m4d_bias_act_bwd")
        g = gp
        g_x = None
        if ctx.needs_input_grad[0]:
            # adjoint of a 'SAME' 3x3 correlation = the stride-1 correlation with k'[ky,kx,o,i] = k[2-ky,2-kx,i,o] of the
            # gradient (stride 2: of the gradient spread onto the input grid with zeros in between)
            zero = cache.get(("zero", cin))
            if zero is None:
                zero = torch.zeros(cin, dtype=torch.float32, device=x.device)
                cache[("zero", cin)] = zero
            gd = g
            if stride == 2:
                gd = torch.empty((b, h, w, cout), dtype=torch.float32, device=g.device)
                check(lib.m4d_dilate2(dptr(g), b, oh, ow, cout, h, w, dptr(gd), stream_ptr()), "m4d_dilate2")
            if _lat_ok(b, h, w, cout, 1) and stride == 1:
                g_x = nops.conv3x3_lat(gd, _packed_lat(cache, weight, True), zero, cin, 1.0, final=True)
            else:
                wp, n_pad = _packed(cache, weight, True)
                g_x = nops.conv3x3_bias_act(gd, wp, zero, cin, n_pad, 1.0, stride=1)
        g_w = None
        if ctx.needs_input_grad[1]:
            # gradient in the parameter's own memory layout: OIHW tensor with channels-last strides = [O][ky][kx][I]
            g_w = torch.empty_strided(tuple(weight.shape), (9 * cin, 1, 3 * cin, cin), dtype=torch.float32, device=x.device)
            n_ws = int(lib.m4d_conv3x3_wgrad_workspace_floats(b, h, w, cin, cout, stride))
            wsg = nops._workspace("wgrad", 4 * n_ws, x.device)
            check(lib.m4d_conv3x3_wgrad(dptr(x), dptr(g), b, h, w, cin, cout, stride, dptr(wsg), n_ws,
                                        ctypes.c_void_p(g_w.data_ptr()), stream_ptr()), "m4d_conv3x3_wgrad")
        return g_x, g_w, g_bias, None, None, None


def conv_bias_act(conv, x, slope, cache):
    """Differentiable twin of network._Conv3x3SameTF.forward."""
    if conv.weight is None:
        conv._build(x.shape[-1], x.device)
    return _ConvBiasAct.apply(as_f32(x, "x"), conv.weight, conv.bias, conv.stride, 1.0 if slope is None else slope, cache)


# ------------------------------------------------------------------------------- glue
class _UpsampleV1(torch.autograd.Function):
    """tf.compat.v1.image.resize_bilinear(x, [h, w]) * mul (legacy coordinates, m4depth_network.py:202-204)."""

    @staticmethod
    def forward(ctx, x, h, w, mul):
        ctx.cfg = (tuple(x.shape), h, w, mul)
        return nops.resize_bilinear_v1(x, h, w, mul)

    @staticmethod
    def backward(ctx, g):
        (b, ih, iw, c), h, w, mul = ctx.cfg
        g = as_f32(g, "grad")
        g_in = torch.empty((b, ih, iw, c), dtype=torch.float32, device=g.device)
        check(lib.m4d_resize_bilinear_v1_bwd(dptr(g, "grad"), b, ih, iw, c, h, w, float(mul), dptr(g_in), stream_ptr()),
              "m4d_resize_bilinear_v1_bwd")
        return g_in, None, None, None


def _upsample2_v1(x, h, w, mul=1.0):
    return _UpsampleV1.apply(as_f32(x, "x"), int(h), int(w), float(mul))


class _NormalizeCuts(torch.autograd.Function):
    """Per-cut tf.linalg.normalize (m4depth_network.py:179-189)."""

    @staticmethod
    def forward(ctx, x, k):
        ctx.save_for_backward(x)
        ctx.k = k
        return nops.normalize_cuts(x, k)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        b, h, w, c = x.shape
        g = as_f32(g, "grad")
        gx = torch.empty_like(x)
        check(lib.m4d_normalize_cuts_bwd(dptr(x), dptr(g, "grad"), b, h, w, c, ctx.k, dptr(gx), stream_ptr()),
              "m4d_normalize_cuts_bwd")
        return gx, None


def _normalize_cuts(x, k):
    return _NormalizeCuts.apply(as_f32(x, "x"), int(k))


class _LevelPost(torch.autograd.Function):
    """The level tail (m4depth_network.py:247-251): refiner output -> parallax = exp(clip)/2^m,
    depth = parallax2depth(parallax), other."""

    @staticmethod
    def forward(ctx, ro, rot, trans, f, c, scale):
        para, depth, other = nops.level_post(ro, rot, trans, {"f": f, "c": c}, scale)
        ctx.save_for_backward(ro, rot, trans, f, c)
        ctx.scale = scale
        return para, depth, other

    @staticmethod
    def backward(ctx, g_para, g_depth, g_other):
        ro, rot, trans, f, c = ctx.saved_tensors
        b, h, w, _ = ro.shape
        gs = [None if g is None else as_f32(g, "grad") for g in (g_para, g_depth, g_other)]
        g_ro = torch.empty_like(ro)
        check(lib.m4d_level_post_bwd(dptr(ro), dptr(gs[0]), dptr(gs[1]), dptr(gs[2]), dptr(rot, "rot"), rot.shape[1],
                                     dptr(trans), dptr(f), dptr(c), b, h, w, float(ctx.scale), dptr(g_ro), stream_ptr()),
              "m4d_level_post_bwd")
        return g_ro, None, None, None, None, None


class _LevelL1(torch.autograd.Function):
    """One level's unweighted term of m4depth_loss (m4depth_network.py:503-533)."""

    @staticmethod
    def forward(ctx, pred, gt, velodyne):
        b, h, w, _ = pred.shape
        H, W = gt.shape[1:3]
        ws = nops._workspace("loss", 4 * int(lib.m4d_loss_workspace_floats()), pred.device)
        out2 = torch.empty(2, dtype=torch.float32, device=pred.device)
        check(lib.m4d_loss_level_fwd(dptr(pred, "pred"), dptr(gt, "gt"), b, h, w, H, W, int(velodyne), dptr(ws), dptr(out2),
                                     stream_ptr()), "m4d_loss_level_fwd")
        ctx.save_for_backward(pred, gt, out2)
        ctx.velodyne = velodyne
        return out2[0]

    @staticmethod
    def backward(ctx, g):
        pred, gt, out2 = ctx.saved_tensors
        b, h, w, _ = pred.shape
        H, W = gt.shape[1:3]
        g = as_f32(g, "grad").reshape(1)
        g_pred = torch.empty_like(pred)
        check(lib.m4d_loss_level_bwd(dptr(pred), dptr(gt), dptr(out2), dptr(g, "grad"), b, h, w, H, W, int(ctx.velodyne),
                                     dptr(g_pred), stream_ptr()), "m4d_loss_level_bwd")
        return g_pred, None, None


class _LevelPhoto(torch.autograd.Function):
    """One level's unweighted term of the photometric reprojection loss (include/m4depth_hip.h, "Photometric reprojection
    loss"): photo + smooth * smoothness of the predicted depth of frame t against the level images of frames t and t-1.
    The images are data; the gradient goes through the warp into the depth (m4d_photo_loss_bwd, a gather)."""

    @staticmethod
    def forward(ctx, depth, rot, trans, f, c, cur, prev, smooth, automask):
        warped, dwarp, valid = nops.photo_warp_fwd(depth, rot, trans, f, c, prev)
        out4, mask = nops.photo_loss_fwd(depth, warped, valid, cur, prev, smooth, automask)
        ctx.save_for_backward(depth, warped, dwarp, cur, mask, out4)
        ctx.smooth = smooth
        return out4[0]

    @staticmethod
    def backward(ctx, g):
        depth, warped, dwarp, cur, mask, out4 = ctx.saved_tensors
        return (nops.photo_loss_bwd(depth, warped, dwarp, cur, mask, out4, g, ctx.smooth),) + (None,) * 8


class _MultiPhoto(torch.autograd.Function):
    """One level's unweighted term with the loss's options (include/m4depth_hip.h, "Full-resolution terms and the minimum over
    two sources"): ``s`` > 1 upsamples the level depth to the images' resolution first (U_s, m4d_upsample_hp_fwd), ``src1`` adds
    the next frame, warped with the inverse motion ``rot1`` / ``trans1``; ``pe_id`` (nops.photo_identity, None = auto-masking
    off) is shared by the levels of a frame at scale full.  The backward is two gathers: m4d_photo_min_bwd, then U_s^T."""

    @staticmethod
    def forward(ctx, depth, rot0, trans0, rot1, trans1, f, c, cur, src0, src1, pe_id, s, smooth):
        D = nops.upsample_hp(depth, s) if s > 1 else depth
        warped0, dwarp0, valid0 = nops.photo_warp_fwd(D, rot0, trans0, f, c, src0)
        warped1 = dwarp1 = valid1 = None
        if src1 is not None:
            warped1, dwarp1, valid1 = nops.photo_warp_fwd(D, rot1, trans1, f, c, src1)
        out4, sel = nops.photo_min_fwd(D, warped0, valid0, warped1, valid1, cur, pe_id, smooth)
        ctx.save_for_backward(D, warped0, dwarp0, warped1, dwarp1, cur, sel, out4)
        ctx.smooth, ctx.s = smooth, s
        return out4[0]

    @staticmethod
    def backward(ctx, g):
        D, warped0, dwarp0, warped1, dwarp1, cur, sel, out4 = ctx.saved_tensors
        g_D = nops.photo_min_bwd(D, warped0, dwarp0, warped1, dwarp1, cur, sel, out4, g, ctx.smooth)
        return (nops.upsample_hp_bwd(g_D, ctx.s) if ctx.s > 1 else g_D,) + (None,) * 12


def motion_inverse(rot, trans):
    """The inverse of a quaternion motion x -> R(rot) x + trans: rot' = (w, -x, -y, -z), trans' = -(R(rot') trans), with
    m4d_load_motion's rotation matrix.  Torch ops on the device (7 numbers per sample), capturable."""
    if rot.shape[-1] != 4:
        raise ValueError("photometric loss, sources='both': the inverse motion needs quaternion rotations (w,x,y,z); a small-angle "
                         "rotation I + [r]x has no exact inverse of that form")
    inv = torch.cat([rot[..., :1], -rot[..., 1:]], dim=-1)           # no host constant: the capture takes no copy from the host
    w, x, y, z = inv.unbind(-1)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    t0, t1, t2 = trans.unbind(-1)
    out = torch.stack([((1.0 - (tyy + tzz)) * t0 + (txy - twz) * t1) + (txz + twy) * t2,
                       ((txy + twz) * t0 + (1.0 - (txx + tzz)) * t1) + (tyz - twx) * t2,
                       ((txz - twy) * t0 + (tyz + twx) * t1) + (1.0 - (txx + tyy)) * t2], dim=-1)
    return inv.contiguous(), (-out).contiguous()


def level_forward_train(level, curr_f_maps, prev_l_est, rot, trans, camera, prev_f_maps, prev_t_depth, cache):
    """DepthEstimatorLevel.call with is_training=True (m4depth_network.py:167-262)."""
    b, h, w, c = curr_f_maps.shape
    dev = curr_f_maps.device
    k = level.nbre_cuts
    vp = (lambda t: _normalize_cuts(t, k)) if level.ablation.normalize_features else (lambda t: t)
    curr_f = vp(curr_f_maps)
    if prev_l_est is None:                                                           # :196-200
        para_prev_l = torch.ones((b, h, w, 1), device=dev)
        depth_prev_l = torch.full((b, h, w, 1), 1000., device=dev)
        other_prev_l = torch.zeros((b, h, w, 4), device=dev)
    else:                                                                            # :202-204
        other_prev_l = _upsample2_v1(prev_l_est["other"], h, w)
        para_prev_l = _upsample2_v1(prev_l_est["parallax"], h, w, 2.)
        depth_prev_l = _upsample2_v1(prev_l_est["depth"], h, w)
    if prev_t_depth is None:                                                         # :208-214
        return {"depth": depth_prev_l, "parallax": para_prev_l, "other": other_prev_l}
    prev_f = vp(prev_f_maps)
    scale = float(2.0 ** level.lvl_mul)
    with torch.no_grad():                                                            # tf.stop_gradient, depth_operations.py:215
        para_prev_t = prev_d2para(prev_t_depth.detach().contiguous(), rot, trans, camera)
    cv, para_reproj = get_parallax_sweeping_cv(curr_f.contiguous(), prev_f.contiguous(), para_prev_t,
                                               para_prev_l.contiguous(), rot, trans, camera, level.dscv_range,
                                               nbre_cuts=k, cv_accum=level.cv_accum)
    feats = [cv, torch.log(para_prev_l * scale)]                                      # :224
    if level.ablation.level_memory:
        feats.append(other_prev_l)
    if level.ablation.SNCV:
        cf = curr_f.contiguous()
        feats.append(cost_volume(cf, cf, level.sncv_range, nbre_cuts=k))             # :232
    if level.ablation.time_recurr:
        r = level.dscv_range
        feats.append(torch.log(para_reproj[..., r:r + 1] * scale))                   # :238
    x = torch.cat(feats, dim=3)
    convs = list(level.disp_refiner.prep_conv_layers) + list(level.disp_refiner.est_d_conv_layers)
    for i, conv in enumerate(convs):
        x = conv_bias_act(conv, x, 0.1 if i < len(convs) - 1 else None, cache)
    rot_t = as_f32(rot, "rot")
    para_curr, depth, other = _LevelPost.apply(x, rot_t, as_f32(trans, "trans").reshape(b, 3),
                                               as_f32(camera["f"], "f").reshape(b, 2),
                                               as_f32(camera["c"], "c").reshape(b, 2), scale)   # :247-251
    return {"other": other, "depth": depth, "parallax": para_curr}


def dinl_autograd(dn, f_map):
    """DomainNormalization (m4depth_network.py:24-48) as the node the TRAINING graph records: (x - mean_hw) / (var_hw + 1e-12),
    l2-normalised over the channels, scale and bias -- torch autograd ops standing where tf.GradientTape stands (the
    inference forward runs the HIP kernel m4d_dinl_fwd_padded instead, network.DomainNormalization.forward)."""
    mean = f_map.mean(dim=(1, 2), keepdim=True)
    centred = f_map - mean
    var = (centred * centred).mean(dim=(1, 2), keepdim=True)
    n = centred / (var + 1e-12)
    ss = (n * n).sum(dim=-1, keepdim=True)
    n = n * torch.rsqrt(torch.clamp_min(ss, 1e-12))               # tf.math.l2_normalize
    return dn.scale * n + dn.bias


def encoder_forward_train(encoder, images, cache):
    """FeaturePyramid.call (m4depth_network.py:76-90), recorded by autograd."""
    fm = as_f32(images, "images")
    outs = []
    for i, (c1, c2, dn) in enumerate(zip(encoder.conv_layers_s1, encoder.conv_layers_s2, encoder.dn_layers)):
        if encoder.use_dinl and i == 0:
            t = conv_bias_act(c1, fm, None, cache)
            if dn.scale is None:
                dn._build(t.shape[-1], t.device)
            t = F.leaky_relu(dinl_autograd(dn, t), 0.1)
        else:
            t = conv_bias_act(c1, fm, 0.1, cache)
        fm = conv_bias_act(c2, t, 0.1, cache)
        outs.append(fm)
    return outs


def model_forward_train(model, traj_samples, camera):
    """M4Depth.call(training=True): returns d_est_seq[seq][level, fine -> coarse] (m4depth_network.py:351-365)."""
    cache = model.__dict__.setdefault("_train_cache", {})
    for key in [k for k in cache if k[0] in ("fwd", "bwd")]:
        del cache[key]                                 # weights may have been stepped since the last call
    pyrs = [encoder_forward_train(model.encoder, s["RGB_im"], cache) for s in traj_samples]
    levels = model.d_estimator.levels
    L = len(levels)
    cams = [{"f": as_f32(camera["f"], "f") / 2. ** (lvl + 1), "c": as_f32(camera["c"], "c") / 2. ** (lvl + 1)}
            for lvl in range(L)]
    d_est_seq = []
    for seq_i, (f_pyr, sample) in enumerate(zip(pyrs, traj_samples)):
        d_est_curr = None
        for l in range(L):
            lvl = L - 1 - l
            f_prev = d_prev = None
            if seq_i != 0:                                                           # :297-299
                f_prev = pyrs[seq_i - 1][lvl]
                d_prev = d_est_seq[-1][lvl]["depth"]
            prev = None if d_est_curr is None else dict(d_est_curr[-1])
            est = level_forward_train(levels[lvl], f_pyr[lvl], prev, sample["rot"], sample["trans"], cams[lvl],
                                      f_prev, d_prev, cache)
            d_est_curr = [est] if d_est_curr is None else d_est_curr + [est]
        d_est_seq.append(d_est_curr[::-1])
    return d_est_seq


def m4depth_loss(gts, preds, depth_type="map"):
    """M4Depth.m4depth_loss (m4depth_network.py:491-536): log-depth L1 over every level of every
    frame but the first, level i weighted 0.64 / 2**(i-1); one fused HIP kernel per level."""
    l1_loss = 0.
    velodyne = depth_type == "velodyne"
    for gt, pred_pyr in zip(gts[1:], preds[1:]):
        gt_d = as_f32(gt["depth"], "gt depth")
        for i, pred in enumerate(pred_pyr):
            term = _LevelL1.apply(as_f32(pred["depth"], "pred depth"), gt_d, velodyne)
            l1_loss = l1_loss + term * ((0.64 / (2. ** (i - 1))) / float(len(gts) - 1))
    return l1_loss


LOSSES = ("supervised", "photometric")
PHOTO_SCALES = ("level", "full")
PHOTO_SOURCES = ("prev", "both")


def photometric_loss(samples, preds, camera, smooth=1e-3, automask=True, scale="level", sources="prev"):
    """Training without ground-truth depth: the photometric reprojection loss (SSIM + L1 error between frame t and frame t-1
    warped with the PREDICTED depth and the data's exact relative pose, validity mask, auto-masking, edge-aware smoothness:
    Godard et al., ICCV 2019; the definition is in include/m4depth_hip.h).  One term per level of every frame but the first,
    with the level weights of ``m4depth_loss``.  ``samples[t]`` = {"RGB_im" [b,H,W,3] in [0,1], "rot", "trans"}, ``preds`` as
    ``model_forward_train`` returns them, ``camera`` the full-resolution intrinsics.  The image pyramid of every frame is built
    once, by one call.

    ``scale``: ``level`` = each term at its level's resolution against the image pyramid; ``full`` = the level depth upsampled to
    the input resolution (half-pixel bilinear) and compared there against the frames themselves (Monodepth2's form).
    ``sources``: ``prev`` = frame t-1 only; ``both`` = the per-pixel minimum over frame t-1 and frame t+1 (the last frame has
    the previous one only), which needs quaternion rotations.  The defaults take ``_LevelPhoto``; anything else ``_MultiPhoto``."""
    if scale not in PHOTO_SCALES:
        raise ValueError(f"scale: expected one of {PHOTO_SCALES}, got {scale!r}")
    if sources not in PHOTO_SOURCES:
        raise ValueError(f"sources: expected one of {PHOTO_SOURCES}, got {sources!r}")
    if scale != "level" or sources != "prev":
        return _photometric_loss_multi(samples, preds, camera, float(smooth), bool(automask), scale, sources)
    T = len(samples)
    L = len(preds[-1])
    b = samples[0]["RGB_im"].shape[0]
    frames = torch.stack([as_f32(s["RGB_im"], "RGB_im") for s in samples], dim=0)               # [T,b,H,W,3]
    with torch.no_grad():
        pyr = [lvl.view(T, b, *lvl.shape[1:]) for lvl in nops.image_pyramid_box(frames.view(T * b, *frames.shape[2:]), L)]
    f, c = as_f32(camera["f"], "f").reshape(b, 2), as_f32(camera["c"], "c").reshape(b, 2)
    cams = [(f / 2. ** (i + 1), c / 2. ** (i + 1)) for i in range(L)]
    loss = 0.
    for t in range(1, T):
        rot, trans = as_f32(samples[t]["rot"], "rot"), as_f32(samples[t]["trans"], "trans").reshape(b, 3)
        for i, pred in enumerate(preds[t]):
            term = _LevelPhoto.apply(as_f32(pred["depth"], "pred depth"), rot, trans, cams[i][0], cams[i][1], pyr[i][t], pyr[i][t - 1],
                                     float(smooth), bool(automask))
            loss = loss + term * ((0.64 / (2. ** (i - 1))) / float(T - 1))
    return loss


def _photometric_loss_multi(samples, preds, camera, smooth, automask, scale, sources):
    """photometric_loss with ``scale`` / ``sources`` other than the defaults."""
    T = len(samples)
    L = len(preds[-1])
    b = samples[0]["RGB_im"].shape[0]
    both = sources == "both"
    if both and any(s["rot"].shape[-1] != 4 for s in samples):
        raise ValueError("photometric loss, sources='both': the inverse motion needs quaternion rotations (w,x,y,z); a small-angle "
                         "rotation I + [r]x has no exact inverse of that form")
    images = [as_f32(s["RGB_im"], "RGB_im") for s in samples]
    f, c = as_f32(camera["f"], "f").reshape(b, 2), as_f32(camera["c"], "c").reshape(b, 2)
    if scale == "full":
        H, W = images[0].shape[1:3]
        if H % (1 << L) or W % (1 << L):
            raise ValueError(f"photometric loss, scale='full': {H}x{W} is no multiple of 2^{L}")
        level_images = [images] * L                                   # level i, frame t: the frames themselves
        cams = [(f, c)] * L
    else:
        with torch.no_grad():
            frames = torch.stack(images, dim=0)
            pyr = [lvl.view(T, b, *lvl.shape[1:]) for lvl in nops.image_pyramid_box(frames.view(T * b, *frames.shape[2:]), L)]
        level_images = [[pyr[i][t] for t in range(T)] for i in range(L)]
        cams = [(f / 2. ** (i + 1), c / 2. ** (i + 1)) for i in range(L)]
    loss = 0.
    for t in range(1, T):
        rot0, trans0 = as_f32(samples[t]["rot"], "rot"), as_f32(samples[t]["trans"], "trans").reshape(b, 3)
        nxt = both and t < T - 1
        rot1 = trans1 = None
        if nxt:
            with torch.no_grad():
                rot1, trans1 = motion_inverse(as_f32(samples[t + 1]["rot"], "rot"), as_f32(samples[t + 1]["trans"], "trans").reshape(b, 3))
        pe_id = None
        for i, pred in enumerate(preds[t]):
            img = level_images[i]
            src1 = img[t + 1] if nxt else None
            if automask and (pe_id is None or scale == "level"):       # at scale full one identity error serves every level
                with torch.no_grad():
                    pe_id = nops.photo_identity(img[t], img[t - 1], src1)
            term = _MultiPhoto.apply(as_f32(pred["depth"], "pred depth"), rot0, trans0, rot1, trans1, cams[i][0], cams[i][1], img[t],
                                     img[t - 1], src1, pe_id, 2 ** (i + 1) if scale == "full" else 1, smooth)
            loss = loss + term * ((0.64 / (2. ** (i - 1))) / float(T - 1))
    return loss


def _loss_of(model, loss, gts, samples, preds, camera):
    """The training loss ``loss`` names: ``supervised`` = m4depth_loss against ground truth, ``photometric`` = photometric_loss
    (its settings are per-model: ``model.photo_smooth``, ``model.photo_automask``, ``model.photo_scale``, ``model.photo_sources``)."""
    if loss == "supervised":
        return m4depth_loss(gts, preds, model.depth_type)
    if loss == "photometric":
        return photometric_loss(samples, preds, camera, getattr(model, "photo_smooth", 1e-3), getattr(model, "photo_automask", True),
                                getattr(model, "photo_scale", "level"), getattr(model, "photo_sources", "prev"))
    raise ValueError(f"loss: expected one of {LOSSES}, got {loss!r}")


def unstack_sequence(data):
    """The sample re-arrangement at the top of train_step / test_step (m4depth_network.py:377-385)."""
    T = data["depth"].shape[1]
    out = [{} for _ in range(T)]
    for key in ("depth", "RGB_im", "new_traj", "rot", "trans"):
        for i in range(T):
            out[i][key] = data[key][:, i]
    return out


def set_trainable(model, flag=True):
    """Keras marks every conv kernel / bias and the DINL scale / bias trainable; the inference
    build keeps them frozen (requires_grad=False) so that no autograd graph is ever recorded."""
    for p in model.parameters():
        p.requires_grad_(flag)
    return model


def train_step(model, data, optimizer, grad_sync=None, loss="supervised"):
    """M4Depth.train_step (m4depth_network.py:371-431): loss, gradients, optimizer update, metrics
    of the last frame.  ``data`` holds [b,T,...] device tensors (+ data['camera']).  ``grad_sync``
    (optional) runs between backward and the update -- dist.all_reduce_gradients for data-parallel
    training over RCCL.  ``loss``: ``supervised`` (m4depth_loss, the reference's) or ``photometric`` (photometric_loss: the
    ground truth is then read by the metric only)."""
    from .metrics import RootMeanSquaredLogError
    if loss not in LOSSES:
        raise ValueError(f"loss: expected one of {LOSSES}, got {loss!r}")
    loss_name = loss
    traj_samples = unstack_sequence(data)
    with torch.no_grad():
        gts = [{"depth": s["depth"], "parallax": depth2parallax(s["depth"], s["rot"], s["trans"], data["camera"])}
               for s in traj_samples]
    with torch.enable_grad():
        preds = model_forward_train(model, traj_samples, data["camera"])
        loss = _loss_of(model, loss_name, gts, traj_samples, preds, data["camera"])
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    if grad_sync is not None:
        grad_sync([p for g in optimizer.param_groups for p in g["params"]])
    optimizer.step()
    model.step_counter += 1
    model.last_pyramid = [lvl["depth"].detach() for lvl in preds[-1]]                # what :410-415 draw, finest first
    with torch.no_grad():                                                            # :418-427
        gt = gts[-1]["depth"]
        est = nops.resize_nearest(preds[-1][0]["depth"].detach().contiguous(), gt.shape[1], gt.shape[2])
        gt_c = torch.clamp(gt, 0.0, 80.)
        est_c = torch.clamp(est, 0.001, 80.)
        if not getattr(model, "compiled_metrics", None):
            model.compiled_metrics = [RootMeanSquaredLogError()]
        for m in model.compiled_metrics:
            m.update_state(gt_c, est_c)
    out = {m.name: m.result() for m in model.compiled_metrics}
    out["loss"] = loss.detach()
    return out


class GraphedTrainStep:
    """One whole ``train_step`` -- forward, loss, backward, Adam update -- captured in a hipGraph.

    Eagerly a 384x384 / batch-3 / 4-frame step is several thousand kernel launches (most of them
    the few-microsecond elementwise nodes of the autograd graph) and the GPU idles two thirds of
    the time waiting for the host (profiles/r01_train_steady_state_eager.txt).  The step has no
    host synchronisation and fixed shapes, so it is captured once and replayed: the host then
    only copies the next batch into the static input buffers.

    ``pyramid``: the last frame's depth estimate of every level, finest first (``est is pyramid[0]``), static tensors of the
    capture like ``loss`` -- what ``summaries.TrainSummaryWriter.images`` draws as ``depth_lvl_i``.

    ``loss``: as in ``train_step``; the photometric loss's pyramid and loss launches are nodes of the capture like the rest (no
    host synchronisation: the mask count N stays on the device).

    ``step_log`` (optional, a ``TrainStepLog``): every step, the warm-up steps included, ends with its device-side log
    entry, so the host reads losses and metrics only when it wants to.

    Requirements: an optimizer whose step is capturable (``torch.optim.Adam(..., capturable=True)``),
    the batch layout of ``example`` for every later call, ``new_traj`` = first frame only (it is
    host-side control flow baked into the capture).  The eager warm-up steps (packed-weight and
    workspace allocation) are REAL optimizer steps on ``example``."""

    def __init__(self, model, example, optimizer, warmup=3, grad_sync=None, step_log=None, loss="supervised"):
        if loss not in LOSSES:
            raise ValueError(f"loss: expected one of {LOSSES}, got {loss!r}")
        self.loss_name = loss
        self.model, self.optimizer = model, optimizer
        self.step_log = step_log
        self.static = {k: example[k].clone() for k in ("depth", "RGB_im", "rot", "trans")}
        self.camera = {k: v.clone() for k, v in example["camera"].items()}
        self.new_traj = example["new_traj"]
        self.grad_sync = grad_sync
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            warm = None
            for _ in range(warmup):
                warm = self._step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        optimizer.zero_grad(set_to_none=True)
        self.graph = torch.cuda.CUDAGraph()
        from ._lib import framework_copies_in_capture
        with framework_copies_in_capture(), torch.cuda.graph(self.graph):      # the autograd graph's own nodes are framework kernels
            self.loss, self.pyramid = self._step()
        self.est = self.pyramid[0]
        if warm is not None:                           # capturing ran nothing: until the first replay the static outputs hold the
            self.loss.copy_(warm[0])                   # last warm-up step's, the step the caller has just taken
            for dst, src in zip(self.pyramid, warm[1]):
                dst.copy_(src)

    def _data(self):
        d = dict(self.static)
        d["new_traj"] = self.new_traj
        d["camera"] = self.camera
        return d

    def _step(self):
        data = self._data()
        samples = unstack_sequence(data)
        gts = [{"depth": s["depth"]} for s in samples]
        preds = model_forward_train(self.model, samples, self.camera)
        loss = _loss_of(self.model, self.loss_name, gts, samples, preds, self.camera)
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        if self.grad_sync is not None:
            self.grad_sync([p for g in self.optimizer.param_groups for p in g["params"]])
        self.optimizer.step()
        loss, pyramid = loss.detach(), [lvl["depth"].detach() for lvl in preds[-1]]
        if self.step_log is not None:                  # the last node of the step: warm-up steps are logged too
            self.step_log.record(loss, self.static["depth"][:, -1], pyramid[0])
        return loss, pyramid

    def __call__(self, data=None):
        """Copies ``data`` into the static buffers, replays the step; returns (loss, finest depth
        estimate of the last frame) -- static device tensors, overwritten by the next replay."""
        if data is not None:
            for k in self.static:
                if data[k].data_ptr() != self.static[k].data_ptr():
                    self.static[k].copy_(data[k], non_blocking=True)
            for k in self.camera:
                if data["camera"][k].data_ptr() != self.camera[k].data_ptr():
                    self.camera[k].copy_(data["camera"][k], non_blocking=True)
        self.graph.replay()
        self.model.step_counter += 1
        return self.loss, self.est


class TrainStepLog:
    """Device-side log of training steps (m4d_train_log_step): ``rows`` x [loss, RMSE_log] in a ring, a step counter and the
    sticky index of the first non-finite loss, written by one fused launch pair at the end of each step and read by the host
    only at ``read()`` -- the replayed step (``GraphedTrainStep``) then never synchronises."""

    def __init__(self, rows, device):
        self.rows = int(rows)
        if self.rows < 1:
            raise ValueError("TrainStepLog: rows must be >= 1")
        self.log = torch.zeros((self.rows, 2), dtype=torch.float32, device=device)
        self.counter = torch.zeros(1, dtype=torch.int64, device=device)
        self.first_bad = torch.full((1,), -1, dtype=torch.int64, device=device)
        self.read_up_to = 0                                    # steps already handed to the host

    def record(self, loss, gt, est):
        nops.train_log_step(loss, gt, est, self.log, self.counter, self.first_bad)

    def read(self):
        """(rows [n,2] float32 numpy of the steps logged since the last read, in step order; first_bad or -1).  Raises when
        more than ``rows`` steps went by unread (the ring overwrote some)."""
        log, counter, first_bad = self.log.cpu().numpy(), int(self.counter.item()), int(self.first_bad.item())
        n = counter - self.read_up_to
        if n > self.rows:
            raise RuntimeError(f"TrainStepLog: {n} steps since the last read overflow the {self.rows}-row log")
        idx = [(self.read_up_to + i) % self.rows for i in range(n)]
        self.read_up_to = counter
        return log[idx], first_bad
