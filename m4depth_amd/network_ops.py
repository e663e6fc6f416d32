"""DepthEstimatorLevel glue kernels (m4depth_network.py:179-204, 218, 224-260)
exposed as tensor functions.  All dispatch to libm4depth_hip.so.
"""
from __future__ import annotations

import ctypes

import torch

from ._lib import lib, dptr, stream_ptr, check, as_f32
from .depth_operations import _CV_ACCUM


def normalize_cuts(x, nbre_cuts, out=None):
    """Per-cut tf.linalg.normalize of m4depth_network.py:179-189 (no epsilon)."""
    x = as_f32(x, "x")
    b, h, w, C = x.shape
    if C % nbre_cuts != 0:
        raise ValueError(f"nbre_cuts={nbre_cuts} does not divide the {C} feature channels")
    if out is None:
        out = torch.empty_like(x)
    check(lib.m4d_normalize_cuts(dptr(x, "x"), b, h, w, C, int(nbre_cuts), dptr(out, "out"), stream_ptr()),
          "m4d_normalize_cuts")
    return out


def resize_bilinear_v1(x, out_h, out_w, mul=1.0):
    """tf.compat.v1.image.resize_bilinear with its defaults (legacy coordinates:
    no half-pixel offset), m4depth_network.py:202-204."""
    x = as_f32(x, "x")
    b, ih, iw, c = x.shape
    out = torch.empty((b, out_h, out_w, c), dtype=torch.float32, device=x.device)
    check(lib.m4d_resize_bilinear_v1(dptr(x, "x"), b, ih, iw, c, int(out_h), int(out_w), float(mul), dptr(out),
                                     stream_ptr()), "m4d_resize_bilinear_v1")
    return out


def resize_nearest(x, out_h, out_w, out=None):
    """tf.image.resize(method=NEAREST_NEIGHBOR), m4depth_network.py:368; ``out`` (optional): the [b,out_h,out_w,c] destination."""
    x = as_f32(x, "x")
    b, ih, iw, c = x.shape
    if out is None:
        out = torch.empty((b, out_h, out_w, c), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (b, out_h, out_w, c):
        raise ValueError(f"resize_nearest: out has shape {tuple(out.shape)}, expected {(b, out_h, out_w, c)}")
    check(lib.m4d_resize_nearest(dptr(x, "x"), b, ih, iw, c, int(out_h), int(out_w), dptr(out), stream_ptr()),
          "m4d_resize_nearest")
    return out


def level_pre(prev_l_est, depth_prev_t, trans, camera, b, h, w, device, f_input=None, log_scale=1.0, normalize=None,
              depth_state_reset=None):
    """Fused upsample of the coarser level's estimate (+ prev_d2para of the
    temporal depth state, + the log-parallax / level-memory features written
    straight into ``f_input``, a ``RefinerInput``, at its ``log_off`` / ``other_off``).  Returns (para_prev_l, depth_prev_l,
    other_prev_l, para_prev_t or None).  ``normalize`` = (raw features [b,h,w,C], cuts, out): the per-cut
    normalisation of the level's current features rides in the same launch (m4d_level_pre_normalize).
    ``depth_state_reset`` [b,h,w,1] (reset branch, m4depth_network.py:209) is set to 1000 in the same pass."""
    para = torch.empty((b, h, w, 1), dtype=torch.float32, device=device)
    depth = torch.empty_like(para)
    other = torch.empty((b, h, w, 4), dtype=torch.float32, device=device)
    para_t = torch.empty_like(para) if depth_prev_t is not None else None
    if prev_l_est is not None:
        pd = as_f32(prev_l_est["depth"], "prev_l_est['depth']")
        pp = as_f32(prev_l_est["parallax"], "prev_l_est['parallax']")
        po = as_f32(prev_l_est["other"], "prev_l_est['other']")
        ph, pw = pd.shape[1:3]
    else:
        pd = pp = po = None
        ph = pw = 0
    tr = f = c = None
    if depth_prev_t is not None:
        tr = as_f32(trans, "trans").reshape(b, 3)
        f = as_f32(camera["f"], "camera['f']").reshape(b, 2)
        c = as_f32(camera["c"], "camera['c']").reshape(b, 2)
    fin_buf, f_stride, log_off, other_off = (None, 0, 0, -1) if f_input is None else (
        f_input.buf, f_input.f_stride, f_input.log_off, f_input.other_off)
    if normalize is not None:
        raw, cuts, nout = normalize
        raw = as_f32(raw, "curr_f_maps")
        check(lib.m4d_level_pre_normalize(dptr(pd), dptr(pp), dptr(po), ph, pw, dptr(depth_prev_t, "depth_prev_t"), dptr(tr),
                                          dptr(f), dptr(c), b, h, w, dptr(para), dptr(depth), dptr(other), dptr(para_t),
                                          dptr(fin_buf, "f_input"), f_stride, int(log_off), int(other_off), float(log_scale),
                                          dptr(depth_state_reset, "depth_state_reset"), dptr(raw, "curr_f_maps"), int(raw.shape[-1]), int(cuts), dptr(nout, "normalised features"),
                                          stream_ptr()), "m4d_level_pre_normalize")
        return para, depth, other, para_t
    check(lib.m4d_level_pre(dptr(pd), dptr(pp), dptr(po), ph, pw, dptr(depth_prev_t, "depth_prev_t"), dptr(tr),
                            dptr(f), dptr(c), b, h, w, dptr(para), dptr(depth), dptr(other), dptr(para_t),
                            dptr(fin_buf, "f_input"), f_stride, int(log_off), int(other_off), float(log_scale),
                            dptr(depth_state_reset, "depth_state_reset"), stream_ptr()), "m4d_level_pre")
    return para, depth, other, para_t


class RefinerInput:
    """The refiner-input rows of one level call and the only place that does address arithmetic on them: ``buf``
    [b,h,w,f_stride] (``f_stride`` >= ``f_in``, the width the refiner was built for) and the channel offsets of the log-parallax
    feature, the level-memory features, the SNCV and the time-recurrence feature (-1 = the level has none)."""

    def __init__(self, buf, f_in, log_off=0, other_off=-1, sncv_off=-1, recurr_off=-1):
        self.buf, self.f_in, self.f_stride = buf, f_in, buf.shape[-1]
        self.log_off, self.other_off, self.sncv_off, self.recurr_off = log_off, other_off, sncv_off, recurr_off

    @classmethod
    def for_level(cls, key, b, h, w, f_in, f_stride, dscv_channels, level_memory, time_recurr, device):
        """The rows of m4depth_network.py:224-242 (DSCV | log parallax | memory | SNCV | time recurrence).  ``f_stride`` > ``f_in``:
        the persistent zeroed workspace of ``key``, whose padding channels nothing ever writes."""
        if f_stride > f_in:
            buf = zeroed_workspace(("f_input", key), (b, h, w, f_stride), device)
        else:
            buf = torch.empty((b, h, w, f_in), dtype=torch.float32, device=device)
        mem = 4 if level_memory else 0
        return cls(buf, f_in, dscv_channels, dscv_channels + 1 if level_memory else -1, dscv_channels + 1 + mem,
                   f_in - 1 if time_recurr else -1)

    def at(self, channel):
        """Address of ``channel`` of the first row; None (NULL) for a channel the level does not have."""
        return None if channel < 0 else ctypes.c_void_p(self.buf.data_ptr() + 4 * channel)

    def dscv_into(self, log_scale):
        return self.at(0), self.f_stride, self.at(self.recurr_off), self.f_stride, log_scale

    def sncv_into(self):
        return self.at(self.sncv_off), self.f_stride

    def rows(self):
        """The reference-width view (inspection / tests)."""
        return self.buf if self.f_stride == self.f_in else self.buf[..., :self.f_in]


def level_front_supported(c, cuts, dscv_range, sncv_range, f_stride):
    return bool(lib.m4d_level_front_supported(c, cuts, dscv_range, sncv_range, f_stride))


def level_front_small_supported(c, cuts, dscv_range, sncv_range):
    return bool(lib.m4d_level_front_small_supported(c, cuts, dscv_range, sncv_range))


def pyramid_reset_supported(c, cuts):
    return bool(lib.m4d_pyramid_reset_supported(c, cuts))


def _coarser_estimate(prev_l_est):
    """(parallax, other, their height, width) of the coarser level's estimate, which the front kernels upsample themselves; NULL
    at the coarsest level."""
    if prev_l_est is None:
        return None, None, 0, 0
    pp = as_f32(prev_l_est["parallax"], "prev_l_est['parallax']")
    return pp, as_f32(prev_l_est["other"], "prev_l_est['other']"), pp.shape[1], pp.shape[2]


def level_front(raw, curr_f, prev_f, depth_prev_t, prev_l_est, motion, cuts, dscv_range, sncv_range, cv_accum, f_input, scale):
    """The whole level front in one launch: ``level_pre``, DSCV and SNCV -> complete rows of ``f_input`` (a ``RefinerInput``), with
    the per-cut normalisation of ``raw`` into ``curr_f`` (m4d_level_front_r) or, ``raw`` None, on a ``curr_f`` normalised ahead of
    the level (m4d_level_front_small).  ``motion`` = (rot, trans [b,3], f [b,2], c [b,2])."""
    rot, tr, cf, cc = motion
    pp, po, ph, pw = _coarser_estimate(prev_l_est)
    b, h, w, c = curr_f.shape
    name, head = ("m4d_level_front_small", ()) if raw is None else ("m4d_level_front_r", (dptr(raw, "curr_f_maps"),))
    check(getattr(lib, name)(*head, dptr(curr_f), dptr(prev_f), dptr(depth_prev_t, "prev_t_depth"), dptr(pp), dptr(po), ph, pw,
                             dptr(rot), rot.shape[1], dptr(tr), dptr(cf), dptr(cc), b, h, w, c, cuts, dscv_range, sncv_range,
                             _CV_ACCUM[cv_accum], f_input.at(0), f_input.f_stride, scale, stream_ptr()), name)


def dscv_sncv(curr_f, prev_f, para_prev_t, para_prev_l, motion, cuts, dscv_range, sncv_range, cv_accum, f_input, scale):
    """Both cost volumes of a small map in one launch (m4d_dscv_sncv_fwd), into the rows of ``f_input``."""
    rot, tr, cf, cc = motion
    b, h, w, c = curr_f.shape
    cv, stride, log, log_stride, log_scale = f_input.dscv_into(scale)
    sncv, sncv_stride = f_input.sncv_into()
    check(lib.m4d_dscv_sncv_fwd(dptr(curr_f), dptr(prev_f), dptr(para_prev_t), dptr(para_prev_l), dptr(rot), rot.shape[1],
                                dptr(tr), dptr(cf), dptr(cc), b, h, w, c, dscv_range, cuts, _CV_ACCUM[cv_accum], cv, stride, None,
                                log, log_stride, log_scale, sncv_range, sncv, sncv_stride, stream_ptr()), "m4d_dscv_sncv_fwd")


def pyramid_reset(levels, b):
    """The reset frame of every level in one launch (m4d_pyramid_reset).  ``levels`` = coarse -> fine list of dicts
    ``features`` [b,h,w,C] raw, ``cuts``, ``state_features`` (receives the normalised features), ``depth_state`` [b,h,w,1].
    Returns the per-level estimates (coarse -> fine) ``{"depth", "parallax", "other"}``: the constant maps the x2 upsampling
    chain of m4depth_network.py:198-204 produces on a new trajectory."""
    from ._lib import ResetLevel
    n = len(levels)
    arr = (ResetLevel * n)()
    ests = []
    pv = 1.0
    for i, lv in enumerate(levels):
        f = as_f32(lv["features"], "curr_f_maps")
        bb, h, w, c = f.shape
        if bb != b:
            raise ValueError("pyramid_reset: batch mismatch")
        para = torch.empty((b, h, w, 1), dtype=torch.float32, device=f.device)
        depth = torch.empty_like(para)
        other = torch.empty((b, h, w, 4), dtype=torch.float32, device=f.device)
        arr[i] = ResetLevel(dptr(f, "curr_f_maps").value, dptr(lv["state_features"], "state_features").value,
                            dptr(lv["depth_state"], "depth_state").value, dptr(para).value, dptr(depth).value, dptr(other).value,
                            h, w, c, int(lv["cuts"]), pv)
        ests.append({"depth": depth, "parallax": para, "other": other})
        pv *= 2.0                                    # :203, exact
    check(lib.m4d_pyramid_reset(arr, n, int(b), stream_ptr()), "m4d_pyramid_reset")
    return ests


def normalize_levels(maps, outs=None):
    """The per-cut normalisation of several feature maps in ONE launch (m4d_normalize_levels; the bits of ``normalize_cuts``).
    ``maps`` = [(tensor [n,h,w,C], cuts), ...] (at most 8); returns the normalised tensors in the same order.  ``outs``
    (optional): one destination per map (the streaming path writes straight into each level's own state buffer)."""
    from ._lib import NormLevel
    n = len(maps)
    arr = (NormLevel * n)()
    dests, outs = outs, []
    for i, (x, cuts) in enumerate(maps):
        x = as_f32(x, "features")
        out = torch.empty_like(x) if dests is None else dests[i]
        if tuple(out.shape) != tuple(x.shape):
            raise ValueError(f"normalize_levels: destination {i} has shape {tuple(out.shape)}, the map {tuple(x.shape)}")
        arr[i] = NormLevel(dptr(x, "features").value, dptr(out).value, int(x.shape[0] * x.shape[1] * x.shape[2]), int(x.shape[3]), int(cuts))
        outs.append(out)
    check(lib.m4d_normalize_levels(arr, n, stream_ptr()), "m4d_normalize_levels")
    return outs


def _reset_mask(reset, b, depth_state):
    """The uint8 [b] device mask of a masked level close (``reset`` bool or uint8); the masked kernels need ``depth_state``."""
    if reset.dtype == torch.bool:
        reset = reset.view(torch.uint8)
    if tuple(reset.shape) != (b,):
        raise ValueError(f"reset mask must have shape ({b},), got {tuple(reset.shape)}")
    if depth_state is None:
        raise ValueError("a masked level close writes the reset samples' depth_state: depth_state is required")
    return dptr(reset, "reset", torch.uint8)


def level_post(refiner_out, rot, trans, camera, scale, depth_state=None, reset=None, reset_parallax=1.0):
    """Fused tail of a level (m4depth_network.py:247-260): returns (parallax,
    depth, other); ``depth_state`` (optional) receives the depth as well.  ``reset`` (streaming): a [b] device mask -- masked
    samples get the reset constants (m4d_level_post_m: parallax ``reset_parallax``, depth 1000, other 0, depth_state 1000)."""
    ro = as_f32(refiner_out, "refiner_out")
    b, h, w, five = ro.shape
    if five != 5:
        raise ValueError(f"refiner output must have 5 channels, got {five}")
    rot = as_f32(rot, "rot")
    tr = as_f32(trans, "trans").reshape(b, 3)
    f = as_f32(camera["f"], "camera['f']").reshape(b, 2)
    c = as_f32(camera["c"], "camera['c']").reshape(b, 2)
    para = torch.empty((b, h, w, 1), dtype=torch.float32, device=ro.device)
    depth = torch.empty_like(para)
    other = torch.empty((b, h, w, 4), dtype=torch.float32, device=ro.device)
    if reset is not None:
        rp = _reset_mask(reset, b, depth_state)
        check(lib.m4d_level_post_m(dptr(ro), dptr(rot, "rot"), rot.shape[1], dptr(tr), dptr(f), dptr(c), b, h, w,
                                   float(scale), dptr(para), dptr(depth), dptr(other), dptr(depth_state, "depth_state"),
                                   rp, float(reset_parallax), stream_ptr()), "m4d_level_post_m")
        return para, depth, other
    check(lib.m4d_level_post(dptr(ro), dptr(rot, "rot"), rot.shape[1], dptr(tr), dptr(f), dptr(c), b, h, w,
                             float(scale), dptr(para), dptr(depth), dptr(other), dptr(depth_state, "depth_state"),
                             stream_ptr()), "m4d_level_post")
    return para, depth, other


def bias_act_(x, bias, slope=0.1):
    """In-place convolution epilogue on an NHWC tensor: x = leaky_relu(x + bias, slope)
    (slope = 1.0: bias add only)."""
    C = x.shape[-1]
    rows = x.numel() // C
    check(lib.m4d_bias_act(dptr(x, "x"), dptr(bias, "bias"), rows, C, float(slope), dptr(x, "x"), stream_ptr()),
          "m4d_bias_act")
    return x


_ws_cache = {}


def _workspace(key, nbytes, device):
    """Scratch buffer per (purpose, device, stream): kernels of different streams may run
    concurrently (the level pipeline of DepthEstimatorPyramid), so they must not share scratch."""
    k = (key, device, torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0)
    ws = _ws_cache.get(k)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
        _ws_cache[k] = ws
    return ws


_zero_ws_cache = {}


class private_workspaces:
    """Inside: every workspace of ``_workspace`` / ``zeroed_workspace`` is a fresh one, and on exit the caches are restored as
    they were.  For a second model run in a process that holds a captured graph (the in-process validation of a replayed
    training step): it neither writes into nor re-sizes a buffer the graph has baked in, whatever stream handles it gets.
    The caller synchronises before leaving (the buffers made inside are dropped on exit)."""

    def __enter__(self):
        self._saved = (dict(_ws_cache), dict(_zero_ws_cache))
        _ws_cache.clear()
        _zero_ws_cache.clear()
        return self

    def __exit__(self, *exc):
        for cache, saved in zip((_ws_cache, _zero_ws_cache), self._saved):
            cache.clear()
            cache.update(saved)
        return False


def zeroed_workspace(key, shape, device):
    """A persistent float32 buffer of ``shape`` per (purpose, shape, device, stream), zero-filled ONCE when it is created:
    for buffers whose padding elements are never written (the channel-padded refiner input).  Created outside any
    hipGraph capture by the eager warm-up pass; replays only reuse it."""
    k = (key, tuple(shape), device, torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0)
    buf = _zero_ws_cache.get(k)
    if buf is None:
        buf = torch.zeros(tuple(shape), dtype=torch.float32, device=device)
        _zero_ws_cache[k] = buf
    return buf


def dinl_act(x, scale, bias, slope=1.0, out=None, offset=(0, 0)):
    """DomainNormalization (m4depth_network.py:44-48) fused with leaky_relu(slope)
    (slope = 1.0: normalisation alone).  x [b,h,w,C], C in (16, 32).  ``out`` may be a larger
    zero-bordered [b,H',W',C] buffer; the result is then written at ``offset`` (row, col)."""
    x = as_f32(x, "x")
    b, h, w, C = x.shape
    ws = _workspace("dinl", 4 * int(lib.m4d_dinl_workspace_floats(b, C)), x.device)
    if out is None:
        out = torch.empty_like(x)
    check(lib.m4d_dinl_fwd_padded(dptr(x, "x"), dptr(scale.reshape(-1), "scale"), dptr(bias.reshape(-1), "bias"),
                                  b, h, w, C, float(slope), dptr(ws), dptr(out, "out"), out.shape[1], out.shape[2],
                                  int(offset[0]), int(offset[1]), stream_ptr()), "m4d_dinl_fwd_padded")
    return out


def bias_act_padded(x, bias, slope, out, offset=(0, 0)):
    """leaky_relu(x + bias, slope) written into the zero-bordered buffer ``out`` [b,H',W',C] at
    ``offset``: the activation arrives already TF-'SAME'-padded for the stride-2 convolution."""
    b, h, w, C = x.shape
    check(lib.m4d_bias_act_padded(dptr(x, "x"), dptr(bias, "bias"), b, h, w, C, float(slope), dptr(out, "out"),
                                  out.shape[1], out.shape[2], int(offset[0]), int(offset[1]), stream_ptr()),
          "m4d_bias_act_padded")
    return out


def depth_metrics(gt, est, max_d=80.0, total=None, count=0, mean=None):
    """The 7 metrics of metrics.py for one batch, one pass: returns a [7] device tensor
    (AbsRel, SqRel, RMSE, RMSE_log, Delta1, Delta2, Delta3); clipping as in test_step.
    ``total`` [7] (Keras-Mean totals) is incremented and ``mean`` [7] = total / count written in the same launch."""
    est = as_f32(est, "est")
    if gt.numel() != est.numel():
        raise ValueError(f"gt {tuple(gt.shape)} and est {tuple(est.shape)} differ in size")
    ws = _workspace("metrics", int(lib.m4d_metrics_workspace_bytes()), est.device)
    out = torch.empty(7, dtype=torch.float32, device=est.device)
    if (gt.is_cuda and gt.dtype == torch.float32 and gt.dim() >= 2 and not gt.is_contiguous() and gt[0].is_contiguous()
            and gt.stride(0) >= gt[0].numel()):
        # dense images at a batch stride: data["depth"][:, -1] of a [b,T,H,W,1] sequence batch, read in place
        check(lib.m4d_depth_metrics_strided(ctypes.c_void_p(gt.data_ptr()), gt[0].numel(), gt.stride(0), dptr(est, "est"),
                                            gt.numel(), float(max_d), dptr(ws), dptr(out), dptr(total, "total"), float(count),
                                            dptr(mean, "mean"), stream_ptr()), "m4d_depth_metrics_strided")
        return out
    gt = as_f32(gt, "gt")
    check(lib.m4d_depth_metrics(dptr(gt, "gt"), dptr(est, "est"), gt.numel(), float(max_d), dptr(ws), dptr(out),
                                dptr(total, "total"), float(count), dptr(mean, "mean"), stream_ptr()), "m4d_depth_metrics")
    return out


def _batch_stride(t, name):
    """Batch stride of a [b, ...] float32 device tensor whose images are dense (t[0] contiguous) -- a slice such as
    ``depth[:, -1]`` of a sequence batch is read in place."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise TypeError(f"{name}: expected a float32 device tensor")
    if t.dim() < 2 or not t[0].is_contiguous() or (t.shape[0] > 1 and t.stride(0) < t[0].numel()):
        raise ValueError(f"{name}: expected [b, ...] with dense images at a batch stride, got strides {t.stride()}")
    return t.stride(0) if t.shape[0] > 1 else t[0].numel()


def depth_metrics_per_sample(gt, est, new_traj, active, max_d=80.0, rows=None, counted=None):
    """The 7 metrics of ``depth_metrics`` for every sample of a batch on its own, in one launch pair: returns (rows [b,7] float32,
    counted [b] uint8), device tensors; row s is bit for bit ``depth_metrics(gt[s:s+1], est[s:s+1])``.  ``counted[s]`` =
    active[s] and not new_traj[s], computed on the device (uint8 [b] masks, never read by the host); nothing synchronises.
    ``rows`` / ``counted`` may be views into a preallocated log (one step's row of an [n_steps,b,7] / [n_steps,b] tensor)."""
    b = est.shape[0]
    per_image = est[0].numel()
    if gt.shape[0] != b or gt[0].numel() != per_image:
        raise ValueError(f"gt {tuple(gt.shape)} and est {tuple(est.shape)} differ in size")
    for name, m in (("new_traj", new_traj), ("active", active)):
        if not isinstance(m, torch.Tensor) or m.dtype not in (torch.uint8, torch.bool) or tuple(m.shape) != (b,):
            raise ValueError(f"{name}: expected a uint8 / bool [{b}] device tensor")
    new_traj = new_traj.view(torch.uint8) if new_traj.dtype == torch.bool else new_traj
    active = active.view(torch.uint8) if active.dtype == torch.bool else active
    gs, es = _batch_stride(gt, "gt"), _batch_stride(est, "est")
    if rows is None:
        rows = torch.empty((b, 7), dtype=torch.float32, device=est.device)
    if counted is None:
        counted = torch.empty(b, dtype=torch.uint8, device=est.device)
    if tuple(rows.shape) != (b, 7) or tuple(counted.shape) != (b,):
        raise ValueError(f"rows must be [{b},7] and counted [{b}], got {tuple(rows.shape)} and {tuple(counted.shape)}")
    ws = _workspace("metrics_ps", int(lib.m4d_metrics_per_sample_workspace_bytes(b)), est.device)
    check(lib.m4d_depth_metrics_per_sample(ctypes.c_void_p(gt.data_ptr()), gs, ctypes.c_void_p(est.data_ptr()), es, b, per_image,
                                           float(max_d), dptr(new_traj, "new_traj", torch.uint8),
                                           dptr(active, "active", torch.uint8), dptr(ws), dptr(rows, "rows"),
                                           dptr(counted, "counted", torch.uint8), stream_ptr()),
          "m4d_depth_metrics_per_sample")
    return rows, counted


def consistency_per_sample(est, est_prev, cur, prev, rot, trans, f, c, reset, active, rows=None, counted=None):
    """The reprojection-consistency score (include/m4depth_hip.h, "Reprojection consistency") of every sample of a batch in one
    launch pair: returns (rows [b,6] float32 = photo, photo_id, better, geo, cover, geo_cover; counted [b] uint8), device tensors.
    ``est`` / ``est_prev`` [b,H,W,1] are the estimates of the current and the previous frame, ``cur`` / ``prev`` [b,H,W,3] the two
    images (dense images at a batch stride: a frame slice of a [B,T,...] tensor is read in place), ``rot`` [b,3|4] / ``trans``
    [b,3] the current frame's motion, ``f`` / ``c`` [b,2] the per-sample full-resolution cameras.  ``counted[s]`` = active[s] and
    not reset[s] and N > 0 and Ng > 0, decided on the device (uint8 / bool [b] masks, never read by the host); an uncounted row is
    six zeros and a masked-off sample's images and maps are not read.  Nothing synchronises.  ``rows`` / ``counted`` may be views
    into a preallocated log (one step's row of an [n_steps,b,6] / [n_steps,b] tensor)."""
    if est.dim() != 4 or est.shape[3] != 1:
        raise ValueError(f"est: expected [b,H,W,1], got {tuple(est.shape)}")
    b, h, w, _ = est.shape
    if tuple(est_prev.shape) != (b, h, w, 1):
        raise ValueError(f"est_prev: expected {(b, h, w, 1)}, got {tuple(est_prev.shape)}")
    for name, t in (("cur", cur), ("prev", prev)):
        if tuple(t.shape) != (b, h, w, 3):
            raise ValueError(f"{name}: expected {(b, h, w, 3)}, got {tuple(t.shape)}")
    for name, m in (("reset", reset), ("active", active)):
        if not isinstance(m, torch.Tensor) or m.dtype not in (torch.uint8, torch.bool) or tuple(m.shape) != (b,):
            raise ValueError(f"{name}: expected a uint8 / bool [{b}] device tensor")
    reset = reset.view(torch.uint8) if reset.dtype == torch.bool else reset
    active = active.view(torch.uint8) if active.dtype == torch.bool else active
    rot = as_f32(rot, "rot")
    if rot.dim() != 2 or rot.shape[0] != b or rot.shape[1] not in (3, 4):
        raise ValueError('Rotation must be expressed as a small angle (x,y,z) or a quaternion (w,x,y,z)')
    trans, f, c = as_f32(trans, "trans").reshape(b, 3), as_f32(f, "f").reshape(b, 2), as_f32(c, "c").reshape(b, 2)
    strides = [_batch_stride(t, n) for t, n in ((est, "est"), (est_prev, "est_prev"), (cur, "cur"), (prev, "prev"))]
    if rows is None:
        rows = torch.empty((b, 6), dtype=torch.float32, device=est.device)
    if counted is None:
        counted = torch.empty(b, dtype=torch.uint8, device=est.device)
    if tuple(rows.shape) != (b, 6) or tuple(counted.shape) != (b,):
        raise ValueError(f"rows must be [{b},6] and counted [{b}], got {tuple(rows.shape)} and {tuple(counted.shape)}")
    nbytes = int(lib.m4d_consistency_workspace_bytes(b, h, w))
    if nbytes < 0:
        raise ValueError(f"consistency: a {b}x{h}x{w} batch is refused (h, w >= 3, h*w <= 2^24, b <= 65535)")
    ws = _workspace("consistency", nbytes + 8, est.device)
    ws_ptr = ctypes.c_void_p((ws.data_ptr() + 7) // 8 * 8)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    check(lib.m4d_consistency_per_sample(vp(est), strides[0], vp(est_prev), strides[1], vp(cur), strides[2], vp(prev), strides[3],
                                         dptr(rot, "rot"), rot.shape[1], dptr(trans, "trans"), dptr(f, "f"), dptr(c, "c"),
                                         dptr(reset, "reset", torch.uint8), dptr(active, "active", torch.uint8), b, h, w, ws_ptr,
                                         dptr(rows, "rows"), dptr(counted, "counted", torch.uint8), stream_ptr()),
          "m4d_consistency_per_sample")
    return rows, counted


POSE_ALIGN_STATE = 64        # doubles per sample at the head of the pose-alignment workspace (include/m4depth_hip.h)


def _mask(m, name, b, optional=False):
    """A per-sample device mask as the library reads it: uint8 [b] (a bool mask reinterpreted), or None where it is optional."""
    if m is None and optional:
        return None
    if not isinstance(m, torch.Tensor) or m.dtype not in (torch.uint8, torch.bool) or tuple(m.shape) != (b,):
        raise ValueError(f"{name}: expected a uint8 / bool [{b}] device tensor")
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def _masks(reset, active, b):
    return _mask(reset, "reset", b), _mask(active, "active", b)


def _check_pose7(pose, b):
    if not isinstance(pose, torch.Tensor) or pose.dtype != torch.float64 or tuple(pose.shape) != (b, 7):
        raise ValueError(f"pose: expected a [{b},7] float64 device tensor")


def _check_camera(cam_f, cam_c, b):
    if tuple(cam_f.shape) != (b, 2) or tuple(cam_c.shape) != (b, 2):
        raise ValueError(f"cam_f / cam_c: expected [{b},2], got {tuple(cam_f.shape)} and {tuple(cam_c.shape)}")


def _pose(rot, trans):
    rot = as_f32(rot, "rot")
    if rot.dim() != 2 or rot.shape[1] != 4:
        raise ValueError(f"pose alignment needs quaternion rotations [b,4], got {tuple(rot.shape)}")
    return rot, as_f32(trans, "trans").reshape(rot.shape[0], 3)


def pose_align_begin(rot, trans, h, w):
    """Opens the pose refinement of one frame (include/m4depth_hip.h, "Pose refinement"): the workspace of a [b,h,w] batch,
    a float64 device tensor whose first ``b * POSE_ALIGN_STATE`` values are the per-sample state ((A, a) = (R^T, -R^T t) of
    ``rot`` [b,4] / ``trans`` [b,3], xi_acc = 0).  One launch; the buffer is shared by the frames of a stream."""
    rot, trans = _pose(rot, trans)
    b = rot.shape[0]
    nbytes = int(lib.m4d_pose_align_workspace_bytes(b, int(h), int(w)))
    if nbytes < 0:
        raise ValueError(f"pose alignment: a {b}x{h}x{w} batch is refused (h, w >= 3, h*w <= 2^24, b <= 65535)")
    ws = _workspace("pose_align", nbytes, rot.device)[:nbytes // 4].view(torch.float64)
    check(lib.m4d_pose_align_begin(dptr(rot, "rot"), 4, dptr(trans, "trans"), b, int(h), int(w), dptr(ws, "workspace", torch.float64),
                                   stream_ptr()), "m4d_pose_align_begin")
    return ws


def pose_align_iterate(ws, cur, prev, est_prev, f, c, reset, active, stride, huber, damping=0.0, prior=(0.0, 0.0)):
    """One Gauss-Newton iteration at ``stride``: ``cur`` / ``prev`` [b, H/stride, W/stride, 3] are the level images (the frames
    themselves at stride 1, else the box-pyramid level), ``est_prev`` [b,H,W,1] the previous frame's full-resolution estimate
    (all three dense images at a batch stride), ``f`` / ``c`` [b,2] the full-resolution cameras.  Two launches; updates ``ws``."""
    if est_prev.dim() != 4 or est_prev.shape[3] != 1:
        raise ValueError(f"est_prev: expected [b,H,W,1], got {tuple(est_prev.shape)}")
    b, h, w, _ = est_prev.shape
    stride = int(stride)
    for name, t in (("cur", cur), ("prev", prev)):
        if stride < 1 or tuple(t.shape) != (b, h // stride, w // stride, 3):
            raise ValueError(f"{name}: expected {(b, h // max(stride, 1), w // max(stride, 1), 3)} at stride {stride}, got {tuple(t.shape)}")
    reset, active = _masks(reset, active, b)
    f, c = as_f32(f, "f").reshape(b, 2), as_f32(c, "c").reshape(b, 2)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    check(lib.m4d_pose_align_iterate(vp(cur), _batch_stride(cur, "cur"), vp(prev), _batch_stride(prev, "prev"), vp(est_prev),
                                     _batch_stride(est_prev, "est_prev"), dptr(f, "f"), dptr(c, "c"),
                                     dptr(reset, "reset", torch.uint8), dptr(active, "active", torch.uint8), b, h, w, stride,
                                     float(huber), float(damping), float(prior[0]), float(prior[1]),
                                     dptr(ws, "workspace", torch.float64), stream_ptr()), "m4d_pose_align_iterate")
    return ws


def pose_align_end(ws, rot, trans, reset, active, h, w, min_cover, caps, rot_out=None, trans_out=None, rows=None):
    """Closes the refinement: the rejection rules decided on the device, then (rot_out [b,4], trans_out [b,3], rows [b,8]) --
    the refined motion, or the given one bit for bit where the result is rejected; ``caps`` = (metres, radians).  ``rows`` may
    be a view into a log.  One launch."""
    rot, trans = _pose(rot, trans)
    b = rot.shape[0]
    reset, active = _masks(reset, active, b)
    rot_out = torch.empty_like(rot) if rot_out is None else rot_out
    trans_out = torch.empty_like(trans) if trans_out is None else trans_out
    rows = torch.empty((b, 8), dtype=torch.float32, device=rot.device) if rows is None else rows
    if tuple(rot_out.shape) != (b, 4) or tuple(trans_out.shape) != (b, 3) or tuple(rows.shape) != (b, 8):
        raise ValueError(f"expected rot_out [{b},4], trans_out [{b},3] and rows [{b},8]")
    check(lib.m4d_pose_align_end(dptr(rot, "rot"), 4, dptr(trans, "trans"), dptr(reset, "reset", torch.uint8),
                                 dptr(active, "active", torch.uint8), b, int(h), int(w), float(min_cover), float(caps[0]),
                                 float(caps[1]), dptr(ws, "workspace", torch.float64), dptr(rot_out, "rot_out"),
                                 dptr(trans_out, "trans_out"), dptr(rows, "rows"), stream_ptr()), "m4d_pose_align_end")
    return rot_out, trans_out, rows


EXPORT_FORMATS = {None: 0, "kitti16": 1, "midair16": 2}          # the `format` argument of m4d_depth_export
EXPORT_PANELS = {"rgb": 0, "est": 1, "gt": 2, "err": 3}          # its panel kinds


def depth_export(est, fmt, panels=(), gt=None, rgb=None, lut=None, near=1.0, far=80.0, err_max=0.5, depth16=None,
                 panels_out=None):
    """The estimate of a frame batch in its on-disk forms, one launch (m4d_depth_export): returns (depth16, panels).

    ``est`` [b,h,w,1], ``gt`` [b,h,w,1], ``rgb`` [b,h,w,3]: float32 device tensors with dense images at a batch stride (a
    frame slice of a sequence batch is read in place).  ``fmt`` 'kitti16' | 'midair16' | None -> ``depth16`` [b,h,w] int16
    holding the uint16 bits (torch moves no uint16: ``.numpy().view(np.uint16)`` on the host), None without a format.
    ``panels``: up to four of 'rgb', 'est', 'gt', 'err' -> [b, len(panels)*h, w, 3] uint8, None when empty; ``lut`` [257,3]
    uint8 device tensor (export.default_lut), row 256 the invalid colour.  ``depth16`` / ``panels_out``: destinations to
    write into (the slot buffers of export.PredictionWriter).  Nothing synchronises."""
    if fmt not in EXPORT_FORMATS:
        raise ValueError(f"fmt: expected one of {[k for k in EXPORT_FORMATS if k]} or None, got {fmt!r}")
    panels = tuple(panels)
    unknown = [p for p in panels if p not in EXPORT_PANELS]
    if unknown or len(panels) > 4:
        raise ValueError(f"panels: up to four of {list(EXPORT_PANELS)}, got {panels}")
    if est.dim() != 4 or est.shape[3] != 1:
        raise ValueError(f"est: expected [b,h,w,1], got {tuple(est.shape)}")
    b, h, w = est.shape[:3]
    dev = est.device
    strides = {"est": _batch_stride(est, "est")}
    for name, t, c, kinds in (("gt", gt, 1, ("gt", "err")), ("rgb", rgb, 3, ("rgb",))):
        if t is None:
            if any(p in kinds for p in panels):
                raise ValueError(f"panels {panels} need {name}")
            strides[name] = 0
            continue
        if tuple(t.shape[:3]) != (b, h, w) or t[0].numel() != h * w * c:
            raise ValueError(f"{name} {tuple(t.shape)} does not belong to est {tuple(est.shape)}")
        strides[name] = _batch_stride(t, name)
    if any(p != "rgb" for p in panels):
        if not isinstance(lut, torch.Tensor) or lut.dtype != torch.uint8 or tuple(lut.shape) != (257, 3):
            raise ValueError("lut: expected a [257,3] uint8 device tensor (export.default_lut)")
    else:
        lut = None
    if fmt is None:
        depth16 = None
    elif depth16 is None:
        depth16 = torch.empty((b, h, w), dtype=torch.int16, device=dev)
    elif tuple(depth16.shape) != (b, h, w):
        raise ValueError(f"depth16: expected {(b, h, w)}, got {tuple(depth16.shape)}")
    if not panels:
        panels_out = None
    elif panels_out is None:
        panels_out = torch.empty((b, len(panels) * h, w, 3), dtype=torch.uint8, device=dev)
    elif tuple(panels_out.shape) != (b, len(panels) * h, w, 3):
        raise ValueError(f"panels_out: expected {(b, len(panels) * h, w, 3)}, got {tuple(panels_out.shape)}")
    kinds = (ctypes.c_int * 4)(*[EXPORT_PANELS[p] for p in panels])
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())          # noqa: E731  (views: checked above)
    check(lib.m4d_depth_export(ptr(est), strides["est"], ptr(gt), strides["gt"], ptr(rgb), strides["rgb"], b, h, w,
                               EXPORT_FORMATS[fmt], dptr(depth16, "depth16", torch.int16), len(panels), kinds,
                               dptr(lut, "lut", torch.uint8), float(near), float(far), float(err_max),
                               dptr(panels_out, "panels_out", torch.uint8), stream_ptr()), "m4d_depth_export")
    return depth16, panels_out


def pose_accumulate(rot, trans, pose, reset=None, force_all=False):
    """One step of the per-sample camera-to-world pose kept on the device (m4d_pose_accumulate): ``pose`` [b,7] float64
    (qw qx qy qz tx ty tz) is updated in place and returned.  ``rot`` [b,4] quaternions, ``trans`` [b,3]: the frame's motion
    as the network gets it; a small-angle ``rot`` [b,3] is refused (it has no exact composition).  ``reset``: uint8 / bool [b]
    device mask of the samples that start a trajectory (identity pose), ``force_all``: all of them.  Nothing synchronises."""
    if not isinstance(pose, torch.Tensor) or pose.dtype != torch.float64 or pose.dim() != 2 or pose.shape[1] != 7:
        raise ValueError("pose: expected a [b,7] float64 device tensor")
    b = pose.shape[0]
    if tuple(rot.shape) == (b, 3):
        raise ValueError("rot: small-angle rotations [b,3] cannot be accumulated into a pose; quaternions [b,4] only")
    if tuple(rot.shape) != (b, 4) or tuple(trans.shape) != (b, 3):
        raise ValueError(f"expected rot [{b},4] and trans [{b},3], got {tuple(rot.shape)} and {tuple(trans.shape)}")
    reset = _mask(reset, "reset", b, optional=True)
    check(lib.m4d_pose_accumulate(dptr(reset, "reset", torch.uint8), int(bool(force_all)), dptr(as_f32(rot, "rot"), "rot"),
                                  dptr(as_f32(trans, "trans"), "trans"), b, dptr(pose, "pose", torch.float64), stream_ptr()),
          "m4d_pose_accumulate")
    return pose


def cloud_capacity(h, w, step):
    """Vertices per sample a [h,w] map can give at ``step``: the size of ``depth_cloud``'s buffer."""
    return -(-int(h) // int(step)) * -(-int(w) // int(step))


def depth_cloud(depth, rgb, cam_f, cam_c, step=2, near=1.0, far=80.0, pose=None, vertices=None, counts=None):
    """The depth maps of a frame batch as dense lists of coloured vertices (m4d_depth_cloud): returns (vertices
    [b,cap,16] uint8, counts [b] int32), cap = ``cloud_capacity(h, w, step)``.  ``depth`` [b,h,w,1], ``rgb`` [b,h,w,3]: float32
    device tensors with dense images at a batch stride; ``cam_f`` / ``cam_c`` [b,2]; ``pose`` [b,7] float64 as
    ``pose_accumulate`` keeps it (world frame) or None (camera frame).  Every ``step``-th pixel of every ``step``-th row with
    a finite depth in [near, far] gives a vertex -- float32 x, y, z and uint8 r, g, b, a -- written densely in raster order;
    the bytes beyond ``counts[s]`` vertices of sample s are left as they were.  ``vertices`` / ``counts``: destinations (the
    slot buffers of export.PredictionWriter).  Nothing synchronises."""
    if depth.dim() != 4 or depth.shape[3] != 1:
        raise ValueError(f"depth: expected [b,h,w,1], got {tuple(depth.shape)}")
    b, h, w = depth.shape[:3]
    step = int(step)
    if step < 1:
        raise ValueError(f"step must be >= 1, got {step}")
    if not float(far) > float(near):
        raise ValueError(f"need near < far, got {near}, {far}")
    if tuple(rgb.shape) != (b, h, w, 3):
        raise ValueError(f"rgb {tuple(rgb.shape)} does not belong to depth {tuple(depth.shape)}")
    _check_camera(cam_f, cam_c, b)
    if pose is not None:
        _check_pose7(pose, b)
    ds, rs = _batch_stride(depth, "depth"), _batch_stride(rgb, "rgb")
    cap = cloud_capacity(h, w, step)
    dev = depth.device
    if vertices is None:
        vertices = torch.empty((b, cap, 16), dtype=torch.uint8, device=dev)
    elif tuple(vertices.shape) != (b, cap, 16):
        raise ValueError(f"vertices: expected {(b, cap, 16)}, got {tuple(vertices.shape)}")
    if counts is None:
        counts = torch.empty(b, dtype=torch.int32, device=dev)
    elif tuple(counts.shape) != (b,):
        raise ValueError(f"counts: expected [{b}], got {tuple(counts.shape)}")
    ws = _workspace("depth_cloud", 4 * int(lib.m4d_depth_cloud_workspace_ints(b, h, w, step)), dev).view(torch.int32)
    check(lib.m4d_depth_cloud(ctypes.c_void_p(depth.data_ptr()), ds, ctypes.c_void_p(rgb.data_ptr()), rs,
                              dptr(as_f32(cam_f, "cam_f"), "cam_f"), dptr(as_f32(cam_c, "cam_c"), "cam_c"),
                              dptr(pose, "pose", torch.float64), b, h, w, step, float(near), float(far),
                              dptr(vertices, "vertices", torch.uint8), dptr(counts, "counts", torch.int32),
                              dptr(ws, "workspace", torch.int32), stream_ptr()), "m4d_depth_cloud")
    return vertices, counts


VIEWS_MAX = 8                                                   # m4d_depth_views: at most this many earlier frames


def depth_views_state(b, h, w, views, device):
    """The state ``depth_views`` keeps between frames: {"ring_depth" [(views+1),b,h,w] float32, "ring_pose" [(views+1),b,7]
    float64, "age" [two [b] int32 buffers, zeroed: in, out], "head": 0, "views": views}.  The ring tensors start uninitialised:
    a slot is read only after it was written (age counts the written ones)."""
    b, h, w, views = int(b), int(h), int(w), int(views)
    if lib.m4d_depth_views_ring_floats(b, h, w, views) < 0:
        raise ValueError(f"depth_views_state: need b in 1..65535, h, w >= 2, h*w <= 2^24 and views in 1..{VIEWS_MAX}, got "
                         f"b {b}, h {h}, w {w}, views {views}")
    return {"ring_depth": torch.empty((views + 1, b, h, w), dtype=torch.float32, device=device),
            "ring_pose": torch.empty((views + 1, b, 7), dtype=torch.float64, device=device),
            "age": [torch.zeros(b, dtype=torch.int32, device=device), torch.zeros(b, dtype=torch.int32, device=device)],
            "head": 0, "views": views}


def depth_views(depth, cam_f, cam_c, pose, state, reset=None, force_all=False, tol_px=1.0, tol_rel=0.01, min_views=None,
                n_views=None, depth_f=None):
    """The multi-view depth check of one frame batch (m4d_depth_views): returns (n_views [b,h,w] uint8, depth_f [b,h,w,1]
    float32).  ``depth`` [b,h,w,1] float32 device tensor with dense images at a batch stride; ``cam_f`` / ``cam_c`` [b,2];
    ``pose`` [b,7] float64 as ``pose_accumulate`` keeps it; ``state`` from ``depth_views_state`` -- this call writes the frame
    into ring slot ``state["head"]``, then advances the head and swaps the age buffers on the host.  ``reset``: uint8 / bool [b]
    device mask of the samples that start a trajectory, ``force_all``: all of them.  ``n_views`` counts the earlier frames (up
    to ``state["views"]``) that confirm a pixel within ``tol_px`` pixels and ``tol_rel`` relative depth; ``depth_f`` is
    ``depth`` with NaN where fewer than ``min_views`` (default min(2, views)) do; both may be given as destinations (the
    buffers of export.PredictionWriter).  Nothing synchronises."""
    if depth.dim() != 4 or depth.shape[3] != 1:
        raise ValueError(f"depth: expected [b,h,w,1], got {tuple(depth.shape)}")
    b, h, w = depth.shape[:3]
    views = int(state["views"])
    min_views = min(2, views) if min_views is None else int(min_views)
    if not 1 <= min_views <= views:
        raise ValueError(f"min_views must be in 1..{views}, got {min_views}")
    if not (float(tol_px) > 0 and float(tol_rel) > 0):
        raise ValueError(f"need tol_px > 0 and tol_rel > 0, got {tol_px}, {tol_rel}")
    _check_camera(cam_f, cam_c, b)
    _check_pose7(pose, b)
    ring_depth, ring_pose, (age_in, age_out) = state["ring_depth"], state["ring_pose"], state["age"]
    if tuple(ring_depth.shape) != (views + 1, b, h, w) or tuple(ring_pose.shape) != (views + 1, b, 7) \
            or tuple(age_in.shape) != (b,) or tuple(age_out.shape) != (b,) or not 0 <= int(state["head"]) <= views:
        raise ValueError(f"state: not a depth_views_state of {(b, h, w)} with {views} views")
    reset = _mask(reset, "reset", b, optional=True)
    ds = _batch_stride(depth, "depth")
    dev = depth.device
    if n_views is None:
        n_views = torch.empty((b, h, w), dtype=torch.uint8, device=dev)
    elif tuple(n_views.shape) != (b, h, w):
        raise ValueError(f"n_views: expected {(b, h, w)}, got {tuple(n_views.shape)}")
    if depth_f is None:
        depth_f = torch.empty((b, h, w, 1), dtype=torch.float32, device=dev)
    elif tuple(depth_f.shape) != (b, h, w, 1):
        raise ValueError(f"depth_f: expected {(b, h, w, 1)}, got {tuple(depth_f.shape)}")
    check(lib.m4d_depth_views(ctypes.c_void_p(depth.data_ptr()), ds, dptr(as_f32(cam_f, "cam_f"), "cam_f"),
                              dptr(as_f32(cam_c, "cam_c"), "cam_c"), dptr(pose, "pose", torch.float64),
                              dptr(reset, "reset", torch.uint8), int(bool(force_all)), b, h, w, views, int(state["head"]),
                              dptr(ring_depth, "ring_depth"), dptr(ring_pose, "ring_pose", torch.float64),
                              dptr(age_in, "age_in", torch.int32), dptr(age_out, "age_out", torch.int32), float(tol_px),
                              float(tol_rel), min_views, dptr(n_views, "n_views", torch.uint8), dptr(depth_f, "depth_f"),
                              stream_ptr()), "m4d_depth_views")
    state["head"] = (int(state["head"]) + 1) % (views + 1)
    state["age"] = [age_out, age_in]
    return n_views, depth_f


VOXEL_MAP_STATS = ("observations", "dropped_range", "dropped_full", "occupied")   # the statistics words of m4d_voxel_map_*
VOXEL_MAP_RECORD = 10                                           # words of a table record: key, n, sx sy sz, sr sg sb, last_stamp, frames


def voxel_map_state(b, slots_log2, device):
    """The state of ``b`` voxel maps with 2^``slots_log2`` slots each (include/m4depth_hip.h), cleared: {"words": the int64
    buffer the library works on, "stats": its [b,4] head, "table": its [b, 2^L, 10] records, "b", "slots_log2", and the scratch
    of ``voxel_map_extract`` once it has run}.  The words are unsigned on the device; torch shows them as int64."""
    b, slots_log2 = int(b), int(slots_log2)
    words = int(lib.m4d_voxel_map_state_words(b, slots_log2))
    if words < 0:
        raise ValueError(f"voxel_map_state: need b in 1..65535 and slots_log2 in 6..26, got b {b}, slots_log2 {slots_log2}")
    buf = torch.empty(words, dtype=torch.int64, device=device)
    state = {"words": buf, "stats": buf[:4 * b].view(b, 4), "table": buf[4 * b:].view(b, 1 << slots_log2, VOXEL_MAP_RECORD),
             "b": b, "slots_log2": slots_log2}
    return voxel_map_clear(state)


def _hashed_check(state, noun, state_words, voxel=None):
    """(b, slots_log2) of a ``voxel_map_state`` / ``tsdf_state`` (``noun``: which; ``state_words``: the library's size of one)."""
    b, slots_log2 = int(state["b"]), int(state["slots_log2"])
    if state["words"].numel() != state_words(b, slots_log2):
        raise ValueError(f"state: not a {noun} of {b} samples with 2^{slots_log2} slots")
    if voxel is not None and not (float(voxel) > 0 and float(voxel) < float("inf")):
        raise ValueError(f"voxel must be a finite edge length > 0, got {voxel}")
    return b, slots_log2


def _hashed_clear(state, mask, check_state, clear, entry):
    b, slots_log2 = check_state(state)
    mask = _mask(mask, "mask", b, optional=True)
    check(clear(dptr(state["words"], "state", torch.int64), dptr(mask, "mask", torch.uint8), b, slots_log2, stream_ptr()), entry)
    return state


def _voxel_map_check(state, voxel=None):
    return _hashed_check(state, "voxel_map_state", lib.m4d_voxel_map_state_words, voxel)


def voxel_map_integrate(vertices, counts, voxel, stamp, state):
    """The compacted vertices of one step into the maps (m4d_voxel_map_integrate): ``vertices`` [b,cap,16] uint8 and ``counts``
    [b] int32 as ``depth_cloud`` left them on the device, ``voxel`` the edge length in metres, ``stamp`` >= 1 the step's number
    (the frames a voxel was seen in are counted by distinct stamps).  One launch, nothing synchronises."""
    b, slots_log2 = _voxel_map_check(state, voxel)
    if vertices.dim() != 3 or vertices.shape[0] != b or vertices.shape[2] != 16 or tuple(counts.shape) != (b,):
        raise ValueError(f"expected vertices [{b},cap,16] and counts [{b}], got {tuple(vertices.shape)} and {tuple(counts.shape)}")
    if int(stamp) < 1:
        raise ValueError(f"stamp must be >= 1, got {stamp}")
    check(lib.m4d_voxel_map_integrate(dptr(vertices, "vertices", torch.uint8), dptr(counts, "counts", torch.int32), b,
                                      vertices.shape[1], float(voxel), int(stamp), dptr(state["words"], "state", torch.int64),
                                      slots_log2, stream_ptr()), "m4d_voxel_map_integrate")
    return state


def voxel_map_extract(state, s, min_frames, voxel):
    """The map of sample ``s`` (m4d_voxel_map_extract): (keys [n] int64 ascending, vertices [n,16] uint8, stats) -- one vertex
    per voxel that at least ``min_frames`` frames observed, sorted by key on the device (``torch.sort`` + a gather); ``stats``:
    the sample's {observations, dropped_range, dropped_full, occupied} as Python integers.  Waits for the device once, to
    read the count and the statistics.  Once per trajectory: not a hot path."""
    b, slots_log2 = _voxel_map_check(state, voxel)
    s, min_frames = int(s), int(min_frames)
    if not 0 <= s < b or min_frames < 1:
        raise ValueError(f"need s in 0..{b - 1} and min_frames >= 1, got s {s}, min_frames {min_frames}")
    dev, cap = state["words"].device, 1 << slots_log2
    if "keys_out" not in state:                                 # every slot may qualify: sized once, kept with the state
        state["keys_out"] = torch.empty(cap, dtype=torch.int64, device=dev)
        state["vertices_out"] = torch.empty((cap, 16), dtype=torch.uint8, device=dev)
        state["count"] = torch.empty(1, dtype=torch.int64, device=dev)
    state["count"].zero_()
    check(lib.m4d_voxel_map_extract(dptr(state["words"], "state", torch.int64), b, slots_log2, s, min_frames, float(voxel),
                                    dptr(state["keys_out"], "keys_out", torch.int64),
                                    dptr(state["vertices_out"], "vertices_out", torch.uint8), cap,
                                    dptr(state["count"], "count", torch.int64), stream_ptr()), "m4d_voxel_map_extract")
    host = torch.cat([state["count"], state["stats"][s]]).cpu().tolist()          # the one wait
    n = host[0]
    keys, order = torch.sort(state["keys_out"][:n])             # keys stay below 2^63: int64 order is the unsigned order
    return keys, state["vertices_out"][:n][order], dict(zip(VOXEL_MAP_STATS, host[1:]))


def voxel_map_clear(state, mask=None):
    """Empties the maps of the samples with ``mask[s]`` set (uint8 / bool [b] device tensor; None: all of them) and zeroes
    their statistics (m4d_voxel_map_clear).  One launch."""
    return _hashed_clear(state, mask, _voxel_map_check, lib.m4d_voxel_map_clear, "m4d_voxel_map_clear")


TSDF_STATS = ("occupied", "dropped_range", "dropped_full", "updates")   # the statistics words of m4d_tsdf_*
TSDF_TRUNC = (2, 8)                                             # the truncation distance in voxels m4d_tsdf_* accept


def tsdf_state(b, slots_log2, device):
    """The state of ``b`` TSDF volumes with 2^``slots_log2`` slots each (include/m4depth_hip.h), cleared: {"words": the int64
    buffer the library works on, "stats": its [b,4] head, "keys": its [b, 2^L] keys, "recs": its [b, 2^L, 6] int32 records (S is
    float32: view column 0), "b", "slots_log2"}.  Keys and counters are unsigned on the device; torch shows them signed."""
    b, slots_log2 = int(b), int(slots_log2)
    words = int(lib.m4d_tsdf_state_words(b, slots_log2))
    if words < 0:
        raise ValueError(f"tsdf_state: need b in 1..65535 and slots_log2 in 6..26, got b {b}, slots_log2 {slots_log2}")
    return tsdf_clear(tsdf_state_views(torch.empty(words, dtype=torch.int64, device=device), b, slots_log2))


def tsdf_state_views(buf, b, slots_log2):
    """The dict of ``tsdf_state`` over an int64 buffer of m4d_tsdf_state_words(b, slots_log2) words, as it is (not cleared)."""
    slots = 1 << slots_log2
    return {"words": buf, "stats": buf[:4 * b].view(b, 4), "keys": buf[4 * b:4 * b + b * slots].view(b, slots),
            "recs": buf[4 * b + b * slots:].view(torch.int32).view(b, slots, 6), "b": b, "slots_log2": slots_log2}


def _tsdf_check(state, voxel=None):
    return _hashed_check(state, "tsdf_state", lib.m4d_tsdf_state_words, voxel)


def tsdf_integrate(depth, rgb, cam_f, cam_c, pose, voxel, trunc, state, near=1.0, far=80.0):
    """One frame batch into the TSDF volumes: m4d_tsdf_allocate (every pixel's ray over the truncation band claims its voxels),
    then m4d_tsdf_integrate (every allocated voxel the frame sees takes its truncated signed distance and colour).  ``depth``
    [b,h,w,1], ``rgb`` [b,h,w,3]: float32 device tensors with dense images at a batch stride; ``cam_f`` / ``cam_c`` [b,2];
    ``pose`` [b,7] float64 as ``pose_accumulate`` keeps it; ``voxel`` the edge in metres, ``trunc`` the truncation distance in
    voxels (2..8).  Two launches, nothing synchronises."""
    b, slots_log2 = _tsdf_check(state, voxel)
    trunc = int(trunc)
    if not TSDF_TRUNC[0] <= trunc <= TSDF_TRUNC[1]:
        raise ValueError(f"trunc must be in {TSDF_TRUNC[0]}..{TSDF_TRUNC[1]} voxels, got {trunc}")
    if depth.dim() != 4 or depth.shape[3] != 1 or depth.shape[0] != b:
        raise ValueError(f"depth: expected [{b},h,w,1], got {tuple(depth.shape)}")
    h, w = depth.shape[1:3]
    if not float(far) > float(near):
        raise ValueError(f"need near < far, got {near}, {far}")
    if tuple(rgb.shape) != (b, h, w, 3):
        raise ValueError(f"rgb {tuple(rgb.shape)} does not belong to depth {tuple(depth.shape)}")
    _check_camera(cam_f, cam_c, b)
    _check_pose7(pose, b)
    ds, rs = _batch_stride(depth, "depth"), _batch_stride(rgb, "rgb")
    f, c = dptr(as_f32(cam_f, "cam_f"), "cam_f"), dptr(as_f32(cam_c, "cam_c"), "cam_c")
    words = dptr(state["words"], "state", torch.int64)
    check(lib.m4d_tsdf_allocate(ctypes.c_void_p(depth.data_ptr()), ds, f, c, dptr(pose, "pose", torch.float64), b, h, w,
                                float(near), float(far), float(voxel), trunc, words, slots_log2, stream_ptr()), "m4d_tsdf_allocate")
    check(lib.m4d_tsdf_integrate(ctypes.c_void_p(depth.data_ptr()), ds, ctypes.c_void_p(rgb.data_ptr()), rs, f, c,
                                 dptr(pose, "pose", torch.float64), b, h, w, float(near), float(far), float(voxel), trunc, words,
                                 slots_log2, stream_ptr()), "m4d_tsdf_integrate")
    return state


def _tsdf_ray_args(state, cam_f, cam_c, pose, h, w, voxel, trunc, min_frames, near, far, guide, window, fill, out, hits):
    """What ``tsdf_raycast`` and ``tsdf_render`` check alike: (b, slots_log2, trunc, min_frames, h, w, near, far, out, strides)."""
    b, slots_log2 = _tsdf_check(state, voxel)
    trunc, min_frames, h, w = int(trunc), int(min_frames), int(h), int(w)
    if not TSDF_TRUNC[0] <= trunc <= TSDF_TRUNC[1]:
        raise ValueError(f"trunc must be in {TSDF_TRUNC[0]}..{TSDF_TRUNC[1]} voxels, got {trunc}")
    if min_frames < 1:
        raise ValueError(f"min_frames must be >= 1, got {min_frames}")
    if h < 1 or w < 1 or h * w > 1 << 24:
        raise ValueError(f"need h, w >= 1 and h*w <= 2^24, got {h}x{w}")
    near, far = float(near), float(far)
    if not (far > near and near > 0):
        raise ValueError(f"need 0 < near < far, got {near}, {far}")
    f32 = lambda v: ctypes.c_float(v).value                    # noqa: E731  (the library's float arguments)
    if (f32(far) - f32(near)) / (f32(voxel) * 0.5) > 1 << 20:
        raise ValueError(f"[{near}, {far}] holds more than 2^20 half voxels of {voxel}: the march's bound")
    if (guide is None) != (window is None):
        raise ValueError("guide and window come together or not at all")
    if window is not None and int(window) < 1:
        raise ValueError(f"window must be >= 1 truncation distances, got {window}")
    _check_camera(cam_f, cam_c, b)
    _check_pose7(pose, b)
    if hits is not None and (not isinstance(hits, torch.Tensor) or tuple(hits.shape) != (b,)):
        raise ValueError(f"hits: expected an int64 [{b}] device tensor")
    if out is None:
        out = torch.empty((b, h, w, 1), dtype=torch.float32, device=state["words"].device)
    strides = {}
    for name, t in (("guide", guide), ("fill", fill), ("out", out)):
        if t is None:
            strides[name] = 0
            continue
        strides[name] = _batch_stride(t, name)
        if tuple(t.shape) != (b, h, w, 1):
            raise ValueError(f"{name}: expected [{b},{h},{w},1], got {tuple(t.shape)}")
    if fill is not None and fill.data_ptr() == out.data_ptr() and strides["fill"] != strides["out"]:
        raise ValueError("out may be fill itself only at the same batch stride")
    return b, slots_log2, trunc, min_frames, h, w, near, far, out, strides


def tsdf_raycast(state, cam_f, cam_c, pose, h, w, voxel, trunc, min_frames, near=1.0, far=80.0, guide=None, window=None,
                 fill=None, out=None, hits=None):
    """The TSDF volumes rendered into the cameras ``pose`` (m4d_tsdf_raycast): returns depth [b,h,w,1] float32, the z-depth of
    the first front-face zero crossing of the field along every pixel's ray over [near, far], marched coarse to fine in half
    voxels.  ``state`` as ``tsdf_integrate`` left it (only read); ``cam_f`` / ``cam_c`` [b,2]; ``pose`` [b,7] float64; ``voxel``,
    ``trunc`` the volume's; a voxel counts once ``min_frames`` frames updated it.  ``guide`` [b,h,w,1] with ``window`` (>= 1; both
    or neither): a pixel with a finite guide depth in [near, far] marches only ``window`` truncation distances around it.
    ``fill`` [b,h,w,1]: what a pixel without a surface gets (None: NaN).  ``guide``, ``fill`` and ``out`` are float32 device
    tensors with dense images at a batch stride; ``out`` (the destination, the caller's) may be ``fill`` itself.  ``hits``: int64
    [b] the launch adds every sample's rendered pixels to (the caller zeroes it; a row of a log is fine).  One launch, nothing
    synchronises."""
    b, slots_log2, trunc, min_frames, h, w, near, far, out, strides = _tsdf_ray_args(
        state, cam_f, cam_c, pose, h, w, voxel, trunc, min_frames, near, far, guide, window, fill, out, hits)
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())          # noqa: E731  (views: checked above)
    check(lib.m4d_tsdf_raycast(dptr(state["words"], "state", torch.int64), b, slots_log2, dptr(as_f32(cam_f, "cam_f"), "cam_f"),
                               dptr(as_f32(cam_c, "cam_c"), "cam_c"), dptr(pose, "pose", torch.float64), h, w, near, far,
                               float(voxel), trunc, min_frames, ptr(guide), strides["guide"], 0 if window is None else int(window),
                               ptr(fill), strides["fill"], ptr(out), strides["out"], dptr(hits, "hits", torch.int64),
                               stream_ptr()), "m4d_tsdf_raycast")
    return out


TSDF_INTERP = {"nearest": 0, "trilinear": 1}                    # how m4d_tsdf_render samples the field


def tsdf_render(state, cam_f, cam_c, pose, h, w, voxel, trunc, min_frames, near=1.0, far=80.0, guide=None, window=None,
                fill=None, interp="nearest", out=None, normal=None, colour=None, view=None, hits=None):
    """``tsdf_raycast`` with a choice of the sample and the surface's looks (m4d_tsdf_render): returns depth [b,h,w,1] float32.
    ``interp``: "nearest" (the depth and the hits are ``tsdf_raycast``'s bit for bit) or "trilinear" (a fine-mode sample blends
    the eight voxels around it when all are known: no half-voxel staircase).  Optional destinations, written for every pixel:
    ``normal`` [b,h,w,3] float32, the unit gradient of the interpolant at the hit in the camera frame, towards the camera (NaN at
    a miss or next to an unknown voxel); ``colour`` [b,h,w,3] float32 in [0,1], the blended mean colour (NaN at a miss);
    ``view`` [b,h,w,3] uint8, the colour under a headlight (0 at a miss).  ``fill`` applies to the depth only.  Every tensor is
    a device tensor with dense images at a batch stride.  The other arguments are ``tsdf_raycast``'s.  One launch, nothing
    synchronises."""
    if interp not in TSDF_INTERP:
        raise ValueError(f"interp must be one of {', '.join(TSDF_INTERP)}, got {interp!r}")
    b, slots_log2, trunc, min_frames, h, w, near, far, out, strides = _tsdf_ray_args(
        state, cam_f, cam_c, pose, h, w, voxel, trunc, min_frames, near, far, guide, window, fill, out, hits)
    for name, t in (("normal", normal), ("colour", colour), ("view", view)):
        if t is None:
            strides[name] = 0
        elif name == "view":
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8:
                raise TypeError("view: expected a uint8 device tensor")
            if t.dim() < 2 or not t[0].is_contiguous() or (t.shape[0] > 1 and t.stride(0) < t[0].numel()):
                raise ValueError(f"view: expected [b, ...] with dense images at a batch stride, got strides {t.stride()}")
            strides[name] = t.stride(0) if t.shape[0] > 1 else t[0].numel()
        else:
            strides[name] = _batch_stride(t, name)
        if t is not None and tuple(t.shape) != (b, h, w, 3):
            raise ValueError(f"{name}: expected [{b},{h},{w},3], got {tuple(t.shape)}")
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())          # noqa: E731  (views: checked above)
    check(lib.m4d_tsdf_render(dptr(state["words"], "state", torch.int64), b, slots_log2, dptr(as_f32(cam_f, "cam_f"), "cam_f"),
                              dptr(as_f32(cam_c, "cam_c"), "cam_c"), dptr(pose, "pose", torch.float64), h, w, near, far,
                              float(voxel), trunc, min_frames, ptr(guide), strides["guide"], 0 if window is None else int(window),
                              ptr(fill), strides["fill"], TSDF_INTERP[interp], ptr(out), strides["out"], ptr(normal),
                              strides["normal"], ptr(colour), strides["colour"], ptr(view), strides["view"],
                              dptr(hits, "hits", torch.int64), stream_ptr()), "m4d_tsdf_render")
    return out


def tsdf_extract_raw(state, s, min_frames, voxel, vertex_cap, quad_cap, out=None):
    """The two extraction launches of sample ``s``: (keys [vertex_cap] int64, vertices [vertex_cap,16] uint8, quads [quad_cap,5]
    int64, counts [2] int64 = records found by each launch -- beyond a capacity they are counted, not written), in the order
    the waves arrived.  ``out``: these four as destinations (counts zeroed by the caller); fresh buffers otherwise."""
    b, slots_log2 = _tsdf_check(state, voxel)
    s, min_frames = int(s), int(min_frames)
    if not 0 <= s < b or min_frames < 1:
        raise ValueError(f"need s in 0..{b - 1} and min_frames >= 1, got s {s}, min_frames {min_frames}")
    dev = state["words"].device
    vertex_cap, quad_cap = max(int(vertex_cap), 1), max(int(quad_cap), 1)
    if out is None:
        out = (torch.empty(vertex_cap, dtype=torch.int64, device=dev), torch.empty((vertex_cap, 16), dtype=torch.uint8, device=dev),
               torch.empty((quad_cap, 5), dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev))
    keys, vertices, quads, counts = out
    if tuple(keys.shape) != (vertex_cap,) or tuple(vertices.shape) != (vertex_cap, 16) or tuple(quads.shape) != (quad_cap, 5) \
            or tuple(counts.shape) != (2,):
        raise ValueError(f"out: expected keys [{vertex_cap}], vertices [{vertex_cap},16], quads [{quad_cap},5] and counts [2]")
    words = dptr(state["words"], "state", torch.int64)
    check(lib.m4d_tsdf_extract_vertices(words, b, slots_log2, s, min_frames, float(voxel), dptr(keys, "keys_out", torch.int64),
                                        dptr(vertices, "vertices_out", torch.uint8), vertex_cap,
                                        dptr(counts[0:1], "count", torch.int64), stream_ptr()), "m4d_tsdf_extract_vertices")
    check(lib.m4d_tsdf_extract_faces(words, b, slots_log2, s, min_frames, dptr(quads, "quads_out", torch.int64), quad_cap,
                                     dptr(counts[1:2], "count", torch.int64), stream_ptr()), "m4d_tsdf_extract_faces")
    return keys, vertices, quads, counts


def tsdf_extract(state, s, min_frames, voxel):
    """The surface of sample ``s`` by naive surface nets: (keys [n] int64 ascending, vertices [n,16] uint8, triangles [2q,3] int32,
    stats) -- one vertex per sign-changing cell whose eight voxels at least ``min_frames`` frames updated, one quad per
    sign-changing grid edge, ordered by (owner key, axis) and split along its (0,2) diagonal; ``stats``: the sample's {occupied,
    dropped_range, dropped_full, updates} and ``quads_dropped``, the quads that named a cell without a vertex (the rim of an open
    surface).  The outputs are sized from ``occupied`` (vertices <= occupied, quads <= 3 occupied), which is read with one wait; the
    launches' own counts are read with a second one.  Sorting (``torch.sort``) and the key -> index mapping
    (``torch.searchsorted``) run on the device.  Once per trajectory: not a hot path."""
    _tsdf_check(state, voxel)
    if not 0 <= int(s) < int(state["b"]):
        raise ValueError(f"need s in 0..{int(state['b']) - 1}, got {s}")
    stats = dict(zip(TSDF_STATS, state["stats"][int(s)].cpu().tolist()))      # the wait of the trajectory
    slots = 1 << int(state["slots_log2"])
    occupied = min(stats["occupied"], slots)
    keys, vertices, quads, counts = tsdf_extract_raw(state, s, min_frames, voxel, occupied, 3 * occupied)
    n_v, n_q = (min(n, cap) for n, cap in zip(counts.cpu().tolist(), (keys.shape[0], quads.shape[0])))
    keys, vertices, triangles, stats["quads_dropped"] = tsdf_order(keys[:n_v], vertices[:n_v], quads[:n_q])
    return keys, vertices, triangles, stats


def tsdf_order(keys, vertices, quads):
    """What the extraction launches found, in arrival order, as a mesh: (keys ascending, vertices in that order, triangles [2q,3]
    int32, quads dropped for naming a cell without a vertex).  Device tensors in, device tensors out."""
    n_v, n_q = keys.shape[0], quads.shape[0]
    keys, order = torch.sort(keys)                              # keys stay below 2^63: int64 order is the unsigned order
    vertices = vertices[order]
    flags, ring = quads[:, 0], quads[:, 1:]
    owner = torch.where(flags >= 4, ring[:, 3], ring[:, 0])
    first = torch.sort(flags & 3, stable=True)[1]               # by axis, then stably by owner: (owner key, axis)
    order = first[torch.sort(owner[first], stable=True)[1]]
    ring = ring[order]
    if n_v:
        at = torch.searchsorted(keys, ring.contiguous()).clamp_(max=n_v - 1)
        have = (keys[at] == ring).all(dim=1)
    else:
        at, have = torch.zeros_like(ring), torch.zeros(ring.shape[0], dtype=torch.bool, device=ring.device)
    q = at[have]
    triangles = torch.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], dim=1).reshape(-1, 3).to(torch.int32)
    return keys, vertices, triangles, int(n_q - q.shape[0])


def tsdf_clear(state, mask=None):
    """Empties the volumes of the samples with ``mask[s]`` set (uint8 / bool [b] device tensor; None: all of them) and zeroes
    their statistics (m4d_tsdf_clear).  One launch."""
    return _hashed_clear(state, mask, _tsdf_check, lib.m4d_tsdf_clear, "m4d_tsdf_clear")


SUMMARY_KINDS = {"unit": 0, "log_depth": 1}                   # the `kind` argument of m4d_summary_images
SUMMARY_MAX_MAPS = 16


def summary_layout(shapes, n):
    """(byte offsets, total bytes) of the images ``summary_images`` writes for maps of ``shapes`` [(h, w, c), ...]: map m's
    [n,h,w,c] block starts at a multiple of 16 bytes."""
    offsets, total = [], 0
    for h, w, c in shapes:
        offsets.append(total)
        total += -(-(int(n) * h * w * c) // 16) * 16
    return offsets, total


def summary_images(maps, kinds, n, out=None):
    """The first ``n`` images of every map as uint8, one launch for all of them (m4d_summary_images): returns a list of
    [n,h,w,c] uint8 tensors, views of one buffer.

    ``maps``: up to 16 float32 device tensors [b,h,w,c], c 1 or 3, b >= n, of any sizes, with dense images at a batch stride
    (a frame slice such as ``data["RGB_im"][:, -1]`` is read in place).  ``kinds``: per map 'unit' (values in [0,1]: colour) or
    'log_depth' (log(clip(d, 1, 200)) / log(200)).  ``out``: the flat uint8 device buffer to write into, at least
    ``summary_layout(...)[1]`` bytes (a slot of summaries.TrainSummaryWriter); allocated when None.  Nothing synchronises."""
    maps, kinds, n = list(maps), list(kinds), int(n)
    if not 1 <= len(maps) <= SUMMARY_MAX_MAPS or len(kinds) != len(maps):
        raise ValueError(f"summary_images: 1..{SUMMARY_MAX_MAPS} maps with one kind each, got {len(maps)} maps, {len(kinds)} kinds")
    unknown = [k for k in kinds if k not in SUMMARY_KINDS]
    if unknown:
        raise ValueError(f"kinds: expected {list(SUMMARY_KINDS)}, got {unknown}")
    strides = []
    for i, t in enumerate(maps):
        strides.append(_batch_stride(t, f"maps[{i}]"))
        if t.dim() != 4 or t.shape[3] not in (1, 3) or t.shape[0] < n or n < 1:
            raise ValueError(f"maps[{i}]: expected [b >= {n},h,w,1 or 3] with n >= 1, got {tuple(t.shape)}")
    shapes = [tuple(t.shape[1:]) for t in maps]
    offsets, total = summary_layout(shapes, n)
    if out is None:
        out = torch.empty(total, dtype=torch.uint8, device=maps[0].device)
    elif out.dim() != 1 or out.numel() < total:
        raise ValueError(f"out: expected a flat uint8 buffer of at least {total} bytes, got {tuple(out.shape)}")
    m = len(maps)
    ints = lambda vals: (ctypes.c_int * m)(*vals)                                   # noqa: E731
    longs = lambda vals: (ctypes.c_longlong * m)(*vals)                             # noqa: E731
    check(lib.m4d_summary_images(m, (ctypes.c_void_p * m)(*[t.data_ptr() for t in maps]), longs(strides),
                                 ints([s[0] for s in shapes]), ints([s[1] for s in shapes]), ints([s[2] for s in shapes]),
                                 ints([SUMMARY_KINDS[k] for k in kinds]), longs(offsets), n, dptr(out, "out", torch.uint8),
                                 stream_ptr()), "m4d_summary_images")
    return [out[o:o + n * h * w * c].view(n, h, w, c) for o, (h, w, c) in zip(offsets, shapes)]


def train_log_step(loss, gt, est, log, counter, first_bad):
    """The step log of a training step (m4d_train_log_step): [loss, RMSE_log of the last frame] into row ``counter % rows`` of
    ``log`` [rows, 2] float32, ``counter`` += 1, ``first_bad`` latched to the step index of the first non-finite loss -- all on
    the device, nothing synchronises, so it can be the last node of a captured step.  ``loss`` [] / [1] float32, ``gt`` the
    last frame's full-resolution ground truth [b,H,W(,1)] (a frame slice such as ``depth[:, -1]`` is read in place), ``est``
    the finest estimate [b,h,w,1]; ``counter`` / ``first_bad`` int64 [1] device tensors."""
    if not isinstance(loss, torch.Tensor) or loss.numel() != 1:
        raise ValueError("loss: expected a one-element float32 device tensor")
    est = as_f32(est, "est")
    b, h, w = est.shape[:3]
    if est.dim() != 4 or est.shape[3] != 1:
        raise ValueError(f"est: expected [b,h,w,1], got {tuple(est.shape)}")
    gs = _batch_stride(gt, "gt")
    if gt.shape[0] != b or gt.dim() not in (3, 4) or (gt.dim() == 4 and gt.shape[3] != 1):
        raise ValueError(f"gt {tuple(gt.shape)} is not the [b,H,W,1] ground truth of est {tuple(est.shape)}")
    H, W = gt.shape[1:3]
    if log.dim() != 2 or log.shape[1] != 2:
        raise ValueError(f"log: expected [rows, 2], got {tuple(log.shape)}")
    for name, t in (("counter", counter), ("first_bad", first_bad)):
        if not isinstance(t, torch.Tensor) or t.numel() != 1:
            raise ValueError(f"{name}: expected a one-element int64 device tensor")
    ws = _workspace("train_log", int(lib.m4d_train_log_workspace_bytes()), est.device)
    check(lib.m4d_train_log_step(dptr(loss.reshape(1), "loss"), ctypes.c_void_p(gt.data_ptr()), gs, dptr(est, "est"), b, H, W,
                                 h, w, dptr(log, "log"), log.shape[0], dptr(counter, "counter", torch.int64),
                                 dptr(first_bad, "first_bad", torch.int64), dptr(ws), stream_ptr()), "m4d_train_log_step")
    return log

def pack_conv_weights(kernel_hwio):
    """Re-pack a TF HWIO [3,3,Cin,Cout] kernel for m4d_conv3x3_bias_act:
    [ceil(Cin/16)][9][CoutPad][16], CoutPad = Cout rounded up to 32, the 16 input channels of a
    chunk stored even-first, zero padded.  numpy in, numpy out (host side, once per model)."""
    import numpy as np
    k = np.asarray(kernel_hwio, dtype=np.float32)
    assert k.shape[:2] == (3, 3)
    cin, cout = k.shape[2], k.shape[3]
    nch = -(-cin // 16)
    cpad = -(-cout // 32) * 32
    full = np.zeros((3, 3, nch * 16, cpad), np.float32)
    full[:, :, :cin, :cout] = k
    perm = np.array([0, 2, 4, 6, 8, 10, 12, 14, 1, 3, 5, 7, 9, 11, 13, 15])
    w = full.reshape(9, nch, 16, cpad)[:, :, perm, :]            # [tap][chunk][16p][n]
    return np.ascontiguousarray(w.transpose(1, 0, 3, 2)), cpad    # [chunk][tap][n][16p]


def conv3x3_bias_act(x, wp, bias, cout, cout_pad, slope=0.1, stride=1, split_batch=None):
    """3x3 TF-'SAME' convolution (stride 1 or 2) + bias + leaky_relu(slope) on the matrix cores.  ``split_batch``: the batch the
    split-K factor (= the summation order) is decided for, when it is not the batch of this launch: the encoder runs a layer on
    one frame or on several stacked frames and must get the same bits per image either way."""
    x = as_f32(x, "x")
    b, h, w, cin = x.shape
    split_b = b if split_batch is None else int(split_batch)
    oh, ow = -(-h // stride), -(-w // stride)
    out = torch.empty((b, oh, ow, cout), dtype=torch.float32, device=x.device)
    ws = None
    ws_floats = 0
    if split_b * oh * ow <= 16384:                       # coarse levels: allow split-K through a workspace
        ws_floats = int(lib.m4d_conv3x3_workspace_floats(b, oh, ow, int(cout_pad)))
        ws = _workspace("conv_splitk", 4 * ws_floats, x.device)
    if split_batch is None:
        check(lib.m4d_conv3x3s_bias_act_ws(dptr(x, "x"), dptr(wp, "wp"), dptr(bias, "bias"), b, h, w, cin, int(cout),
                                           int(cout_pad), int(stride), float(slope), dptr(out), dptr(ws), ws_floats,
                                           stream_ptr()), "m4d_conv3x3s_bias_act_ws")
    else:
        check(lib.m4d_conv3x3s_bias_act_wsb(dptr(x, "x"), dptr(wp, "wp"), dptr(bias, "bias"), b, split_b, h, w, cin, int(cout),
                                            int(cout_pad), int(stride), float(slope), dptr(out), dptr(ws), ws_floats,
                                            stream_ptr()), "m4d_conv3x3s_bias_act_wsb")
    return out


def conv3x3_small_bias_act(x, wp, bias, cout, cout_pad, slope=0.1, stride=1):
    """The convolution for small maps (stride 1 or 2): one launch, K split over the waves of a workgroup (no split-K reduce)."""
    x = as_f32(x, "x")
    b, h, w, cin = x.shape
    out = torch.empty((b, -(-h // stride), -(-w // stride), cout), dtype=torch.float32, device=x.device)
    check(lib.m4d_conv3x3s_small_bias_act(dptr(x, "x"), dptr(wp, "wp"), dptr(bias, "bias"), b, h, w, cin, int(cout),
                                          int(cout_pad), int(stride), float(slope), dptr(out), stream_ptr()),
          "m4d_conv3x3s_small_bias_act")
    return out


_WINO_G = [[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]]


_WINO_SKEW = 64


def pack_conv_weights_winograd(kernel_hwio, chunk=16):
    """Winograd F(2x2,3x3) filter transform U = G g G^T of a TF HWIO [3,3,Cin,Cout] kernel (in float64, rounded
    once to float32), packed for m4d_conv3x3_wino_bias_act (chunk = 16) / m4d_conv3x3_wino2_bias_act (chunk = 8):
    [ceil(Cin/chunk)][16 positions][CoutPad][chunk channels], zero padded; for chunk = 8 every position block is
    followed by 64 floats of padding (kWSkew in m4d_wino.hip: the 16 position blocks of a chunk, 4 KB apart at
    CoutPad = 128, otherwise all start on the same L2 channel).  numpy in, numpy out."""
    import numpy as np
    k = np.asarray(kernel_hwio, dtype=np.float64)
    assert k.shape[:2] == (3, 3)
    cin, cout = k.shape[2], k.shape[3]
    G = np.array(_WINO_G, np.float64)
    U = np.einsum('ij,jkco,lk->ilco', G, k, G)                   # [4,4,Cin,Cout]
    nch = -(-cin // chunk)
    cpad = -(-cout // 32) * 32
    full = np.zeros((16, nch * chunk, cpad), np.float32)
    full[:, :cin, :cout] = U.reshape(16, cin, cout).astype(np.float32)
    w = np.ascontiguousarray(full.reshape(16, nch, chunk, cpad).transpose(1, 0, 3, 2))    # [chunk][pos][n][channels]
    if chunk == 8:
        skewed = np.zeros((nch, 16, cpad * chunk + _WINO_SKEW), np.float32)
        skewed[:, :, :cpad * chunk] = w.reshape(nch, 16, cpad * chunk)
        return skewed, cpad
    return w, cpad


def conv3x3_wino_bias_act(x, wu, bias, cout, cout_pad, slope=0.1):
    """3x3 stride-1 TF-'SAME' convolution + bias + leaky_relu(slope), Winograd F(2x2,3x3) on the matrix cores."""
    x = as_f32(x, "x")
    b, h, w, cin = x.shape
    out = torch.empty((b, h, w, cout), dtype=torch.float32, device=x.device)
    check(lib.m4d_conv3x3_wino_bias_act(dptr(x, "x"), dptr(wu, "wu"), dptr(bias, "bias"), b, h, w, cin, int(cout),
                                        int(cout_pad), float(slope), dptr(out), stream_ptr()), "m4d_conv3x3_wino_bias_act")
    return out


def conv3x3_wino2_bias_act(x, wu8, bias, cout, cout_pad, slope=0.1):
    """Winograd variant 2 (16x16 workgroup tile, 8-channel chunks; weights packed with chunk=8)."""
    x = as_f32(x, "x")
    b, h, w, cin = x.shape
    out = torch.empty((b, h, w, cout), dtype=torch.float32, device=x.device)
    check(lib.m4d_conv3x3_wino2_bias_act(dptr(x, "x"), dptr(wu8, "wu8"), dptr(bias, "bias"), b, h, w, cin, int(cout),
                                         int(cout_pad), float(slope), dptr(out), stream_ptr()), "m4d_conv3x3_wino2_bias_act")
    return out


def split_bf16x3(v):
    """float32 array -> uint16 [3, ...]: three bf16 bit patterns p1, p2, p3 (round to nearest even) with
    v == p1 + p2 + p3 EXACTLY (8 + 8 + 8 significand bits; the residuals of a rounding are exact in float32)."""
    import numpy as np

    def bf16_rn(x):
        u = x.view(np.uint32).astype(np.uint64)
        return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)

    def widen(b):
        return (b.astype(np.uint32) << 16).view(np.float32)
    v = np.ascontiguousarray(v, dtype=np.float32)
    if not np.isfinite(v).all():
        raise ValueError("split_bf16x3: non-finite float32 value (NaN / Inf weights cannot be split into bf16 terms)")
    # below 2^-110 the third residual would fall into bf16's denormal range and stop being exact: such magnitudes are
    # 30 orders below anything a float32 accumulation of activations x weights can resolve -- flushed to zero
    v = np.where(np.abs(v) < np.float32(2.0 ** -110), np.float32(0.0), v)
    p1 = bf16_rn(v)
    r1 = v - widen(p1)
    p2 = bf16_rn(r1)
    r2 = r1 - widen(p2)
    p3 = bf16_rn(r2)
    if not np.array_equal(widen(p3), r2):
        raise ValueError("split_bf16x3: a float32 value is not the exact sum of three bf16 terms")
    return np.stack([p1, p2, p3])


def pack_conv_weights_wino6(kernel_hwio):
    """Winograd F(2x2,3x3) filter transform U = G g G^T (float64, rounded once to float32 -- the same U as
    pack_conv_weights_winograd), every value split exactly into three bf16 terms, in the MFMA B-fragment order of
    m4d_conv3x3_wino6_bias_act: [Cin/16][CoutPad/64][16 positions][2 N-tiles][3 parts][64 lanes][8] bf16 (uint16 bits),
    lane = k_half * 32 + cout % 32, element e = channel 8 k_half + e of the chunk.  Cin is zero-padded to a multiple of
    16, Cout to a multiple of 64.  numpy in, (numpy uint16, CoutPad) out."""
    import numpy as np
    k = np.asarray(kernel_hwio, dtype=np.float64)
    assert k.shape[:2] == (3, 3)
    cin, cout = k.shape[2], k.shape[3]
    G = np.array(_WINO_G, np.float64)
    U = np.einsum('ij,jkco,lk->ilco', G, k, G)                   # [4,4,Cin,Cout]
    nch, ng = -(-cin // 16), -(-cout // 64)
    cpad = ng * 64
    full = np.zeros((16, nch * 16, cpad), np.float32)
    full[:, :cin, :cout] = U.reshape(16, cin, cout).astype(np.float32)
    parts = split_bf16x3(full)                                   # [3][pos][cin][cout]
    parts = parts.reshape(3, 16, nch, 2, 8, ng, 2, 32)           # part, pos, chunk, k_half, e, n-group, n-tile, j
    w = np.ascontiguousarray(parts.transpose(2, 5, 1, 6, 0, 3, 7, 4))   # chunk, group, pos, n-tile, part, k_half, j, e
    return w.reshape(nch, ng, 16, 2, 3, 64, 8), cpad


def pack_conv_weights_winof16(kernel_hwio):
    """The filter transform U of pack_conv_weights_wino6 (the same float32 values), scaled per output channel n by 2^t_n
    (|2^t_n U| < 2^15, exact) and split into two fp16 terms (round to nearest: hi = fp16(u), lo = fp16(u - hi)) in the
    B-fragment order of m4d_conv3x3_winof16_bias_act_ks: [Cin/16][CoutPad/64][16 positions][2 N-tiles][2 parts][64 lanes][8]
    fp16 bits, followed by the CoutPad exponents t_n as int16.  numpy in, (flat numpy uint16, CoutPad) out."""
    import numpy as np
    k = np.asarray(kernel_hwio, dtype=np.float64)
    assert k.shape[:2] == (3, 3)
    cin, cout = k.shape[2], k.shape[3]
    G = np.array(_WINO_G, np.float64)
    U = np.einsum('ij,jkco,lk->ilco', G, k, G)                   # [4,4,Cin,Cout]
    nch, ng = -(-cin // 16), -(-cout // 64)
    cpad = ng * 64
    full = np.zeros((16, nch * 16, cpad), np.float32)
    full[:, :cin, :cout] = U.reshape(16, cin, cout).astype(np.float32)
    if not np.isfinite(full).all():
        raise ValueError("pack_conv_weights_winof16: non-finite weight")
    amax = np.abs(full).max(axis=(0, 1)).astype(np.float64)      # [cpad]
    texp = np.where(amax > 0, 15 - np.frexp(amax)[1], 0).astype(np.int64)   # amax < 2^E  ->  2^t amax < 2^15
    scaled = full.astype(np.float64) * np.ldexp(1.0, texp)[None, None, :]    # exact: a power of two
    hi = scaled.astype(np.float16)
    lo = (scaled - hi.astype(np.float64)).astype(np.float16)
    parts = np.stack([hi, lo]).view(np.uint16)                   # [2][pos][cin][cout]
    parts = parts.reshape(2, 16, nch, 2, 8, ng, 2, 32)           # part, pos, chunk, k_half, e, n-group, n-tile, j
    w = np.ascontiguousarray(parts.transpose(2, 5, 1, 6, 0, 3, 7, 4))   # chunk, group, pos, n-tile, part, k_half, j, e
    return np.concatenate([w.reshape(-1), texp.astype(np.int16).view(np.uint16)]), cpad


def pack_conv_weights_small6(kernel_hwio):
    """A TF HWIO [3,3,Cin,Cout] kernel split exactly into three bf16 terms per weight, for m4d_conv3x3_small6_bias_act:
    [ceil(Cin/16)][9 taps][CoutPad][3 parts][16 channels] bf16 (uint16 bits), Cin zero-padded to a multiple of 16, CoutPad = Cout
    rounded up to 32.  numpy in, (numpy uint16, CoutPad) out."""
    import numpy as np
    k = np.asarray(kernel_hwio, dtype=np.float32)
    assert k.shape[:2] == (3, 3)
    cin, cout = k.shape[2], k.shape[3]
    nch = -(-cin // 16)
    cpad = -(-cout // 32) * 32
    full = np.zeros((9, nch * 16, cpad), np.float32)
    full[:, :cin, :cout] = k.reshape(9, cin, cout)
    parts = split_bf16x3(full).reshape(3, 9, nch, 16, cpad)       # part, tap, chunk, channel, n
    return np.ascontiguousarray(parts.transpose(2, 1, 4, 0, 3)), cpad   # chunk, tap, n, part, channel


def pack_conv_weights_lat(kernel_hwio):
    """A TF HWIO [3,3,Cin,Cout] kernel split exactly into three bf16 terms per weight, in the MFMA B-fragment order
    m4d_conv3x3_lat loads straight into operand registers: [ceil(Cout/32)][ceil(Cin/16)][9 taps][3 parts][64 lanes][8] bf16
    (uint16 bits); lane = k_half * 32 + cout % 32, element e = channel 8 k_half + e of the chunk.  Zero padded.
    numpy in, numpy uint16 out."""
    import numpy as np
    k = np.asarray(kernel_hwio, dtype=np.float32)
    assert k.shape[:2] == (3, 3)
    cin, cout = k.shape[2], k.shape[3]
    nch, ng = -(-cin // 16), -(-cout // 32)
    full = np.zeros((9, nch * 16, ng * 32), np.float32)
    full[:, :cin, :cout] = k.reshape(9, cin, cout)
    parts = split_bf16x3(full).reshape(3, 9, nch, 2, 8, ng, 32)   # part, tap, chunk, k_half, e, group, n
    return np.ascontiguousarray(parts.transpose(5, 2, 1, 0, 3, 6, 4)).reshape(ng, nch, 9, 3, 64, 8)


def pack_conv_weights_lat_f16(kernel_hwio):
    """The TF HWIO [3,3,Cin,Cout] kernel of pack_conv_weights_lat scaled per output channel n by 2^t_n (|2^t_n w| < 2^15,
    exact) and split into two fp16 terms (round to nearest: hi = fp16(w), lo = fp16(w - hi)) in the B-fragment order
    m4d_conv3x3_lat_f16 loads into operand registers: [ceil(Cout/32)][ceil(Cin/16)][9 taps][2 parts][64 lanes][8] fp16 bits
    (lane = k_half * 32 + cout % 32, element e = channel 8 k_half + e of the chunk; zero padded), followed by the
    ceil(Cout/32) * 32 exponents t_n as int16.  numpy in, flat numpy uint16 out."""
    import numpy as np
    k = np.asarray(kernel_hwio, dtype=np.float32)
    assert k.shape[:2] == (3, 3)
    cin, cout = k.shape[2], k.shape[3]
    nch, ng = -(-cin // 16), -(-cout // 32)
    full = np.zeros((9, nch * 16, ng * 32), np.float32)
    full[:, :cin, :cout] = k.reshape(9, cin, cout)
    if not np.isfinite(full).all():
        raise ValueError("pack_conv_weights_lat_f16: non-finite weight")
    amax = np.abs(full).max(axis=(0, 1)).astype(np.float64)      # [ng * 32]
    texp = np.where(amax > 0, 15 - np.frexp(amax)[1], 0).astype(np.int64)   # amax < 2^E  ->  2^t amax < 2^15
    scaled = full.astype(np.float64) * np.ldexp(1.0, texp)[None, None, :]    # exact: a power of two
    hi = scaled.astype(np.float16)
    lo = (scaled - hi.astype(np.float64)).astype(np.float16)
    parts = np.stack([hi, lo]).view(np.uint16).reshape(2, 9, nch, 2, 8, ng, 32)   # part, tap, chunk, k_half, e, group, n
    w = np.ascontiguousarray(parts.transpose(5, 2, 1, 0, 3, 6, 4))               # group, chunk, tap, part, k_half, n, e
    return np.concatenate([w.reshape(-1), texp.astype(np.int16).view(np.uint16)])


class PartialAct:
    """An activation that exists as K-slice partial sums: ``slabs`` [S,b,h,w,C] raw sums of m4d_conv3x3_lat's K slices, to be
    added in slab order, + ``bias``, leaky_relu(``slope``) -- which the consuming m4d_conv3x3_lat does while it stages its
    input.  ``dense()`` = the finished [b,h,w,C] tensor (one HIP launch, m4d_partial_finish: same order, same bits)."""

    def __init__(self, slabs, bias, slope):
        self.slabs, self.bias, self.slope = slabs, bias, 1.0 if slope is None else float(slope)

    @property
    def shape(self):
        return self.slabs.shape[1:]

    @property
    def is_cuda(self):
        return self.slabs.is_cuda

    @property
    def device(self):
        return self.slabs.device

    def dense(self):
        S, b, h, w, C = self.slabs.shape
        out = torch.empty((b, h, w, C), dtype=torch.float32, device=self.slabs.device)
        check(lib.m4d_partial_finish(dptr(self.slabs, "slabs"), S, b * h * w * C, dptr(self.bias, "bias"), self.slope,
                                     b * h * w, C, dptr(out), stream_ptr()), "m4d_partial_finish")
        return out


def _lat_halo_pixels(mt, stride):
    mtx, mty = (2 if mt >= 4 else 1), (2 if mt >= 2 else 1)
    return ((8 * mtx - 1) * stride + 3) * ((4 * mty - 1) * stride + 3)


import os as _os
# grid cap of the latency-first small-map convolution (workgroups): 256 = one per CU
lat_max_workgroups = int(_os.environ.get("M4D_LAT_MAX_WG", "256"))


def lat_config(b, h, w, cin, cout, final=False, stride=1):
    """(mt, kw, s_out) of m4d_conv3x3_lat / m4d_conv3x3s_lat for a layer -- the rule the sweep of tools/bench_lat_convs.py
    reads out (profiles/r05_lat_conv_sweep.txt): as many K slices over workgroups as there can be (s_out <= 4 partial slabs, no
    empty slice; ``final`` forces 1: the consumer cannot add slabs), one chunk per wave where the slice allows it (kw = 1 / 2 /
    4 K sub-slices over the waves of a workgroup), and a grid of at most one workgroup per CU: on larger maps first the waves
    stop splitting K (kw -> 1: four cout groups share one staged halo), then a wave takes 2 / 4 M-tiles.  (h, w) = the INPUT
    size; two staged rounds of kw chunks must fit the 160 KB of LDS."""
    n_chunks, n_groups = -(-cin // 16), -(-cout // 32)
    oh, ow = -(-h // stride), -(-w // stride)
    s_out = 1 if final else min(4, n_chunks)
    while s_out > 1 and (s_out - 1) * (-(-n_chunks // s_out)) >= n_chunks:
        s_out -= 1                                      # no empty K slice
    cps = -(-n_chunks // s_out)
    kw = 1 if cps <= 1 else (2 if cps <= 2 else 4)

    def wgs(mt, kw):
        mtx, mty = (2 if mt == 4 else 1), (2 if mt >= 2 else 1)
        tiles = b * (-(-oh // (4 * mty))) * (-(-ow // (8 * mtx)))
        return tiles * (-(-n_groups // (4 // kw))) * s_out

    def fits(mt, kw):
        return 2 * kw * _lat_halo_pixels(mt, stride) * 96 <= 160 * 1024
    mt = 1
    while (wgs(mt, kw) > lat_max_workgroups or not fits(mt, kw)) and kw > 1:
        kw //= 2
    while wgs(mt, kw) > lat_max_workgroups and mt < 4 and fits(mt * 2, kw):
        mt *= 2
    return mt, kw, s_out


def conv3x3_lat(x, wp, bias, cout, slope=0.1, final=False, config=None, stride=1):
    """m4d_conv3x3_lat / m4d_conv3x3s_lat: ``x`` a finished [b,h,w,Cin] tensor or a ``PartialAct``; returns a finished tensor
    (s_out == 1) or a ``PartialAct`` the next call finishes while staging.  ``config`` = (mt, kw, s_out) overrides lat_config;
    ``stride`` 1 or 2 (TF 'SAME')."""
    if isinstance(x, PartialAct):
        xs, s_in, x_bias, x_slope = x.slabs, x.slabs.shape[0], x.bias, x.slope
        b, h, w, cin = x.shape
        slab = b * h * w * cin
    else:
        xs = as_f32(x, "x")
        s_in, x_bias, x_slope = 1, None, 1.0
        b, h, w, cin = xs.shape
        slab = 0
    mt, kw, s_out = config if config is not None else lat_config(b, h, w, cin, cout, final, stride)
    act = 1.0 if slope is None else float(slope)
    oh, ow = -(-h // stride), -(-w // stride)
    out = torch.empty((s_out, b, oh, ow, cout), dtype=torch.float32, device=xs.device)
    check(lib.m4d_conv3x3s_lat(dptr(xs, "x"), s_in, slab, dptr(x_bias, "x_bias"), float(x_slope), dptr(wp, "wp", torch.int16),
                               dptr(bias, "bias"), b, h, w, cin, int(cout), int(stride), act, mt, kw, s_out, dptr(out),
                               b * oh * ow * int(cout), stream_ptr()), "m4d_conv3x3s_lat")
    return out[0] if s_out == 1 else PartialAct(out, bias, act)


def conv3x3_lat_f16(x, wp, bias, cout, slope=0.1, final=False, config=None):
    """conv3x3_lat (stride 1) on m4d_conv3x3_lat_f16: float32 operands scaled by powers of two and split into two fp16 terms,
    three fp16 MFMA products per term pair (csrc/m4d_convlat_f16.hip).  ``wp`` = pack_conv_weights_lat_f16 on the device
    (int16).  Takes and returns what conv3x3_lat does: its ``PartialAct`` slabs are the same raw float32 partial sums."""
    if isinstance(x, PartialAct):
        xs, s_in, x_bias, x_slope = x.slabs, x.slabs.shape[0], x.bias, x.slope
        b, h, w, cin = x.shape
        slab = b * h * w * cin
    else:
        xs = as_f32(x, "x")
        s_in, x_bias, x_slope = 1, None, 1.0
        b, h, w, cin = xs.shape
        slab = 0
    mt, kw, s_out = config if config is not None else lat_config(b, h, w, cin, cout, final)
    act = 1.0 if slope is None else float(slope)
    out = torch.empty((s_out, b, h, w, cout), dtype=torch.float32, device=xs.device)
    check(lib.m4d_conv3x3_lat_f16(dptr(xs, "x"), s_in, slab, dptr(x_bias, "x_bias"), float(x_slope), dptr(wp, "wp", torch.int16),
                                  dptr(bias, "bias"), b, h, w, cin, int(cout), act, mt, kw, s_out, dptr(out),
                                  b * h * w * int(cout), stream_ptr()), "m4d_conv3x3_lat_f16")
    return out[0] if s_out == 1 else PartialAct(out, bias, act)


def conv3x3_small6_bias_act(x, wp6, bias, cout, cout_pad, slope=0.1):
    """The one-launch small-map convolution with float32 operands split into three bf16 terms (csrc/m4d_conv.hip,
    conv3x3_small6_kernel): float32 accuracy at 2.7x less matrix-core time per wave."""
    x = as_f32(x, "x")
    b, h, w, cin = x.shape
    out = torch.empty((b, h, w, cout), dtype=torch.float32, device=x.device)
    check(lib.m4d_conv3x3_small6_bias_act(dptr(x, "x"), dptr(wp6, "wp6", torch.int16), dptr(bias, "bias"), b, h, w, cin, int(cout),
                                          int(cout_pad), float(slope), dptr(out), stream_ptr()), "m4d_conv3x3_small6_bias_act")
    return out


class ActMaxima:
    """A finished activation ``tensor`` [b,h,w,C] together with ``maxima`` [b,h,w,ceil(C/64)] (int32 bits), per pixel and
    group of 64 channels the largest finite |value| as the fp16 Winograd kernel that wrote the tensor saw it
    (m4d_conv3x3_winof16_bias_act_pm, ``pm_out``).  The next such layer derives its input scales from them instead of scanning
    its halo; every other consumer takes ``dense()``, the tensor itself (no launch)."""

    def __init__(self, tensor, maxima):
        self.tensor, self.maxima = tensor, maxima

    @property
    def shape(self):
        return self.tensor.shape

    @property
    def is_cuda(self):
        return self.tensor.is_cuda

    @property
    def device(self):
        return self.tensor.device

    def dense(self):
        return self.tensor


def conv3x3_winof16_bias_act(x, wuh, bias, cout, cout_pad, slope=0.1, stagger_us=0, stagger_phases=16, want_maxima=False):
    """The convolution of conv3x3_wino6_bias_act with float32 operands split into two fp16 terms after a power-of-two scale
    (per Winograd tile / per output channel), three fp16 MFMA products per term pair, float32 accumulation
    (csrc/m4d_wino_f16.hip).  ``wuh`` = pack_conv_weights_winof16 on the device (int16).  ``x`` an ``ActMaxima``: the input
    scales come from its maxima, not from a scan of the halo; ``want_maxima``: returns an ``ActMaxima`` for the next layer
    (allocated like the output).  The same bits either way."""
    pm_in = None
    if isinstance(x, ActMaxima):
        x, pm_in = x.tensor, x.maxima
    x = as_f32(x, "x")
    b, h, w, cin = x.shape
    out = torch.empty((b, h, w, cout), dtype=torch.float32, device=x.device)
    if pm_in is None and not want_maxima:
        check(lib.m4d_conv3x3_winof16_bias_act_ks(dptr(x, "x"), dptr(wuh, "wuh", torch.int16), dptr(bias, "bias"), b, h, w, cin,
                                                  int(cout), int(cout_pad), float(slope), dptr(out), int(stagger_us),
                                                  int(stagger_phases), stream_ptr()),
              "m4d_conv3x3_winof16_bias_act_ks")
        return out
    if pm_in is not None and tuple(pm_in.shape) != (b, h, w, -(-cin // 64)):
        raise ValueError(f"conv3x3_winof16_bias_act: maxima {tuple(pm_in.shape)} do not belong to an input {tuple(x.shape)}")
    pm_out = torch.empty((b, h, w, int(cout_pad) // 64), dtype=torch.int32, device=x.device) if want_maxima else None
    check(lib.m4d_conv3x3_winof16_bias_act_pm(dptr(x, "x"), dptr(wuh, "wuh", torch.int16), dptr(bias, "bias"), b, h, w, cin,
                                              int(cout), int(cout_pad), float(slope), dptr(out), dptr(pm_in, "maxima", torch.int32),
                                              dptr(pm_out, "maxima", torch.int32), int(stagger_us), int(stagger_phases), stream_ptr()),
          "m4d_conv3x3_winof16_bias_act_pm")
    return ActMaxima(out, pm_out) if want_maxima else out


def conv3x3_wino6_bias_act(x, wu6, bias, cout, cout_pad, slope=0.1, kernel=0, stagger_us=0, stagger_phases=16, arith="bf16x3",
                           want_maxima=False):
    """3x3 stride-1 TF-'SAME' convolution + bias + leaky_relu(slope): Winograd F(2x2,3x3), float32 operands split into
    three bf16 terms, six bf16 MFMA products per term pair, float32 accumulation.  ``kernel``: 0 = chosen from the grid,
    1 = one workgroup per (tile, 64 couts) (csrc/m4d_wino6.hip), 2 = persistent workgroups (csrc/m4d_wino6p.hip); same bits.
    ``stagger_us`` > 0: the one-workgroup-per-unit kernel starts its first round of workgroups in ``stagger_phases`` groups spread
    over that many microseconds (a per-launch ARGUMENT, m4d_conv3x3_wino6_bias_act_ks; same bits).  ``arith`` = "f16x2": the
    same layer on the fp16 two-term kernel (conv3x3_winof16_bias_act; ``wu6`` = pack_conv_weights_winof16, ``kernel`` ignored;
    an ``ActMaxima`` input and ``want_maxima`` are that kernel's alone)."""
    if arith == "f16x2":
        return conv3x3_winof16_bias_act(x, wu6, bias, cout, cout_pad, slope, stagger_us=stagger_us, stagger_phases=stagger_phases,
                                        want_maxima=want_maxima)
    if want_maxima or isinstance(x, ActMaxima):
        raise ValueError("conv3x3_wino6_bias_act: pixel maxima are handed on by the f16x2 kernel only")
    x = as_f32(x, "x")
    b, h, w, cin = x.shape
    out = torch.empty((b, h, w, cout), dtype=torch.float32, device=x.device)
    check(lib.m4d_conv3x3_wino6_bias_act_ks(dptr(x, "x"), dptr(wu6, "wu6", torch.int16), dptr(bias, "bias"), b, h, w, cin,
                                            int(cout), int(cout_pad), float(slope), dptr(out), int(kernel), int(stagger_us),
                                            int(stagger_phases), stream_ptr()),
          "m4d_conv3x3_wino6_bias_act_ks")
    return out


class FrameStack:
    """``frames`` [bsz,T',H,W,3]-shaped VIEW into a sequence batch [bsz,T,H,W,3] (frames t0..t1 of every sequence): what
    M4Depth.call hands the encoder so that all frames are encoded in one launch, frame-major (image t*bsz + i), read in
    place.  Only the fused encoder head understands it; ``dense()`` materialises the stacked batch for any other layer."""

    def __init__(self, frames):
        if frames.dim() != 5 or frames.dtype != torch.float32 or not frames[0, 0].is_contiguous():
            raise ValueError("FrameStack: expected a float32 [b,T,H,W,3] view with dense frames")
        self.frames = frames

    @property
    def shape(self):
        bsz, t, h, w, c = self.frames.shape
        return (bsz * t, h, w, c)

    @property
    def is_cuda(self):
        return self.frames.is_cuda

    @property
    def device(self):
        return self.frames.device

    def dense(self):
        bsz, t, h, w, c = self.frames.shape
        return self.frames.transpose(0, 1).reshape(bsz * t, h, w, c)


def encoder_head(images, w_hwio, bias1, dn_scale, dn_bias, wp2, bias2, cout2, cout2_pad, slope=0.1):
    """Encoder level 0 with DINL (m4depth_network.py:79-87) in two fused calls: conv3x3(3->16) + bias + DINL statistics,
    then the stride-2 convolution reading the raw map and normalising it on the fly.  Returns [b, h/2, w/2, cout2].
    ``images``: a dense [b,h,w,3] tensor or a ``FrameStack``."""
    if isinstance(images, FrameStack):
        fr = images.frames
        bsz = fr.shape[0]
        stride_b, stride_t = fr.stride(0), fr.stride(1)
        b, h, w, c3 = images.shape
        img_ptr = ctypes.c_void_p(fr.data_ptr())
        if not fr.is_cuda:
            raise RuntimeError("images: m4depth_amd ops run on the MI355X only; there is no CPU fallback")
        images_dev = fr.device
    else:
        images = as_f32(images, "images")
        b, h, w, c3 = images.shape
        bsz, stride_b, stride_t = b, h * w * c3, 0
        img_ptr = dptr(images, "images")
        images_dev = images.device
    if c3 != 3:
        raise ValueError(f"encoder_head expects RGB images, got {c3} channels")
    C = bias1.numel()
    ws = _workspace("dinl", 4 * int(lib.m4d_dinl_workspace_floats(b, C)), images_dev)
    raw = torch.empty((b, h, w, C), dtype=torch.float32, device=images_dev)
    check(lib.m4d_enc_head_fwd(img_ptr, int(bsz), int(stride_b), int(stride_t), dptr(w_hwio, "w_hwio"), dptr(bias1, "bias"),
                               b, h, w, C, dptr(ws), dptr(raw), stream_ptr()), "m4d_enc_head_fwd")
    total = int(lib.m4d_dinl_workspace_floats(b, C))     # [partials | mean b*C | var b*C]
    mean = ws[total - 2 * b * C: total - b * C]
    var = ws[total - b * C: total]
    oh, ow = -(-h // 2), -(-w // 2)
    out = torch.empty((b, oh, ow, cout2), dtype=torch.float32, device=images_dev)
    check(lib.m4d_conv3x3s2_dinl_bias_act(dptr(raw), dptr(mean), dptr(var), dptr(dn_scale.reshape(-1), "dn_scale"),
                                          dptr(dn_bias.reshape(-1), "dn_bias"), float(slope), dptr(wp2, "wp"), dptr(bias2, "bias"),
                                          b, h, w, int(cout2), int(cout2_pad), float(slope), dptr(out), stream_ptr()),
          "m4d_conv3x3s2_dinl_bias_act")
    return out


def _image_batch_address(images):
    """(pointer, bsz, stride_b, stride_t, (b, h, w, c), device) of a dense [b,h,w,3] batch or a ``FrameStack`` read in place."""
    if isinstance(images, FrameStack):
        fr = images.frames
        if not fr.is_cuda:
            raise RuntimeError("images: m4depth_amd ops run on the MI355X only; there is no CPU fallback")
        return ctypes.c_void_p(fr.data_ptr()), fr.shape[0], fr.stride(0), fr.stride(1), tuple(images.shape), fr.device
    images = as_f32(images, "images")
    b, h, w, c3 = images.shape
    return dptr(images, "images"), b, h * w * c3, 0, (b, h, w, c3), images.device


def encoder_level0_stats(images, w1_hwio, bias1):
    """The DINL statistics of encoder level 0 (m4depth_network.py:44-48 on the 3 -> 16 convolution's output, which is never
    written): (mean, var), each [b,16], per image.  ``images`` may hold MORE frames than the ``encoder_level0`` call that
    consumes a slice of the rows: the statistics of a whole sequence ride in the first encoder batch's launches."""
    img_ptr, bsz, stride_b, stride_t, (b, h, w, c3), dev = _image_batch_address(images)
    if c3 != 3 or bias1.numel() != 16:
        raise ValueError("encoder_level0_stats expects RGB images and a 3->16 convolution")
    ws = _workspace("dinl", 4 * int(lib.m4d_dinl_workspace_floats(b, 16)), dev)
    mean = torch.empty((b, 16), dtype=torch.float32, device=dev)
    var = torch.empty((b, 16), dtype=torch.float32, device=dev)
    check(lib.m4d_enc_level0_stats(img_ptr, int(bsz), int(stride_b), int(stride_t), dptr(w1_hwio, "w1_hwio"), dptr(bias1, "bias1"),
                                   b, h, w, dptr(ws), dptr(mean), dptr(var), stream_ptr()), "m4d_enc_level0_stats")
    return mean, var


def encoder_level0(images, w1_hwio, bias1, dn_scale, dn_bias, w2_hwio, bias2, slope=0.1, stats=None):
    """Encoder level 0 with DINL (m4depth_network.py:79-87) in one call that never writes the [b,h,w,16] map: the 3 -> 16
    convolution is recomputed from the images on the matrix cores in each pass (sums, squared deviations, normalise +
    stride-2 convolution).  16 -> 16 channels only (the reference's level 0).  ``images``: dense [b,h,w,3] or a ``FrameStack``.
    ``stats`` = (mean, var) [b,16] of these images from ``encoder_level0_stats``: only the last pass runs."""
    img_ptr, bsz, stride_b, stride_t, (b, h, w, c3), images_dev = _image_batch_address(images)
    if c3 != 3 or bias1.numel() != 16 or bias2.numel() != 16 or tuple(w2_hwio.shape) != (3, 3, 16, 16):
        raise ValueError("encoder_level0 expects RGB images and 3->16 / 16->16 convolutions")
    out = torch.empty((b, -(-h // 2), -(-w // 2), 16), dtype=torch.float32, device=images_dev)
    if stats is not None:
        mean, var = stats
        if tuple(mean.shape) != (b, 16) or tuple(var.shape) != (b, 16):
            raise ValueError(f"encoder_level0: statistics of {tuple(mean.shape)} for {b} images")
        check(lib.m4d_enc_level0_apply(img_ptr, int(bsz), int(stride_b), int(stride_t), dptr(w1_hwio, "w1_hwio"), dptr(bias1, "bias1"),
                                       dptr(mean, "mean"), dptr(var, "var"), dptr(dn_scale.reshape(-1), "dn_scale"),
                                       dptr(dn_bias.reshape(-1), "dn_bias"), float(slope), dptr(w2_hwio, "w2_hwio"),
                                       dptr(bias2, "bias2"), float(slope), b, h, w, dptr(out), stream_ptr()), "m4d_enc_level0_apply")
        return out
    ws = _workspace("dinl", 4 * int(lib.m4d_dinl_workspace_floats(b, 16)), images_dev)
    check(lib.m4d_enc_level0_fwd(img_ptr, int(bsz), int(stride_b), int(stride_t), dptr(w1_hwio, "w1_hwio"), dptr(bias1, "bias1"),
                                 dptr(dn_scale.reshape(-1), "dn_scale"), dptr(dn_bias.reshape(-1), "dn_bias"), float(slope),
                                 dptr(w2_hwio, "w2_hwio"), dptr(bias2, "bias2"), float(slope), b, h, w, dptr(ws), dptr(out),
                                 stream_ptr()), "m4d_enc_level0_fwd")
    return out


def pack_refiner_tail_weights(k6_hwio, k7_hwio):
    """Weights of the fused level tail (m4d_refiner_tail): conv6 [3,3,32,16] -> [9][16][32], conv7 [3,3,16,5] -> [9][16][16]
    (output rows 5..15 zero).  numpy in, numpy out."""
    import numpy as np
    k6 = np.asarray(k6_hwio, np.float32)
    k7 = np.asarray(k7_hwio, np.float32)
    assert k6.shape == (3, 3, 32, 16) and k7.shape == (3, 3, 16, 5), (k6.shape, k7.shape)
    w6 = np.ascontiguousarray(k6.reshape(9, 32, 16).transpose(0, 2, 1))
    w7 = np.zeros((9, 16, 16), np.float32)
    w7[:, :5, :] = k7.reshape(9, 16, 5).transpose(0, 2, 1)
    return w6, w7


def pack_refiner_tail_weights6(k6_hwio, k7_hwio):
    """Weights of the bf16-split fused level tail (m4d_refiner_tail6) as MFMA B fragments, every weight split exactly into
    three bf16 terms: conv6 [3,3,32,16] -> [9 taps][3 parts][64 lanes = (k-quarter, cout)][8 channels 8 kq .. 8 kq + 7];
    conv7 [3,3,16,5] -> [5 K-steps][3 parts][4 k-quarters][8 couts][8]: k-quarter kq = channels 8 (kq & 1) .. + 7 of tap
    2 j + (kq >> 1), zeros for the tenth tap and couts 5..7.  numpy in, numpy uint16 out."""
    import numpy as np
    k6 = np.asarray(k6_hwio, np.float32)
    k7 = np.asarray(k7_hwio, np.float32)
    assert k6.shape == (3, 3, 32, 16) and k7.shape == (3, 3, 16, 5), (k6.shape, k7.shape)
    p6 = split_bf16x3(k6.reshape(9, 4, 8, 16))                      # part, tap, kq, e, n
    w6 = np.ascontiguousarray(p6.transpose(1, 0, 2, 4, 3)).reshape(9, 3, 64, 8)        # tap, part, (kq, n), e
    full7 = np.zeros((10, 16, 8), np.float32)
    full7[:9, :, :5] = k7.reshape(9, 16, 5)
    p7 = split_bf16x3(full7.reshape(5, 2, 2, 8, 8))                 # part, j, tap parity, channel half, e, n
    w7 = np.ascontiguousarray(p7.transpose(1, 0, 2, 3, 5, 4)).reshape(5, 3, 4, 8, 8)   # j, part, kq = (parity, half), n, e
    return w6, w7


def refiner_tail6(x32, w6f, b6, w7f, b7, rot, trans, camera, scale, depth_state=None, reset=None, reset_parallax=1.0):
    """refiner_tail with float32 operands split into three bf16 terms on the bf16 matrix cores (csrc/m4d_tail6.hip);
    w6f / w7f from pack_refiner_tail_weights6 (int16 views on the device).  ``reset``: as ``level_post`` (m4d_refiner_tail6_m)."""
    x = as_f32(x32, "x32")
    b, h, w, c = x.shape
    if c != 32:
        raise ValueError(f"refiner_tail6 expects the 32-channel refiner activation, got {c} channels")
    rot = as_f32(rot, "rot")
    tr = as_f32(trans, "trans").reshape(b, 3)
    f = as_f32(camera["f"], "camera['f']").reshape(b, 2)
    cc = as_f32(camera["c"], "camera['c']").reshape(b, 2)
    para = torch.empty((b, h, w, 1), dtype=torch.float32, device=x.device)
    depth = torch.empty_like(para)
    other = torch.empty((b, h, w, 4), dtype=torch.float32, device=x.device)
    if reset is not None:
        rp = _reset_mask(reset, b, depth_state)
        check(lib.m4d_refiner_tail6_m(dptr(x, "x32"), dptr(w6f, "w6f", torch.int16), dptr(b6, "b6"), dptr(w7f, "w7f", torch.int16),
                                      dptr(b7, "b7"), dptr(rot, "rot"), rot.shape[1], dptr(tr), dptr(f), dptr(cc), b, h, w, float(scale),
                                      dptr(para), dptr(depth), dptr(other), dptr(depth_state, "depth_state"), rp,
                                      float(reset_parallax), stream_ptr()), "m4d_refiner_tail6_m")
        return para, depth, other
    check(lib.m4d_refiner_tail6(dptr(x, "x32"), dptr(w6f, "w6f", torch.int16), dptr(b6, "b6"), dptr(w7f, "w7f", torch.int16),
                                dptr(b7, "b7"), dptr(rot, "rot"), rot.shape[1], dptr(tr), dptr(f), dptr(cc), b, h, w, float(scale),
                                dptr(para), dptr(depth), dptr(other), dptr(depth_state, "depth_state"), stream_ptr()),
          "m4d_refiner_tail6")
    return para, depth, other


def refiner_tail(x32, w6p, b6, w7p, b7, rot, trans, camera, scale, depth_state=None, reset=None, reset_parallax=1.0):
    """conv(32->16)+lrelu, conv(16->5) and the level tail (level_post) in one launch: returns (parallax, depth, other).
    ``reset``: as ``level_post`` (m4d_refiner_tail_m)."""
    x = as_f32(x32, "x32")
    b, h, w, c = x.shape
    if c != 32:
        raise ValueError(f"refiner_tail expects the 32-channel refiner activation, got {c} channels")
    rot = as_f32(rot, "rot")
    tr = as_f32(trans, "trans").reshape(b, 3)
    f = as_f32(camera["f"], "camera['f']").reshape(b, 2)
    cc = as_f32(camera["c"], "camera['c']").reshape(b, 2)
    para = torch.empty((b, h, w, 1), dtype=torch.float32, device=x.device)
    depth = torch.empty_like(para)
    other = torch.empty((b, h, w, 4), dtype=torch.float32, device=x.device)
    if reset is not None:
        rp = _reset_mask(reset, b, depth_state)
        check(lib.m4d_refiner_tail_m(dptr(x, "x32"), dptr(w6p, "w6p"), dptr(b6, "b6"), dptr(w7p, "w7p"), dptr(b7, "b7"),
                                     dptr(rot, "rot"), rot.shape[1], dptr(tr), dptr(f), dptr(cc), b, h, w, float(scale),
                                     dptr(para), dptr(depth), dptr(other), dptr(depth_state, "depth_state"), rp,
                                     float(reset_parallax), stream_ptr()), "m4d_refiner_tail_m")
        return para, depth, other
    check(lib.m4d_refiner_tail(dptr(x, "x32"), dptr(w6p, "w6p"), dptr(b6, "b6"), dptr(w7p, "w7p"), dptr(b7, "b7"),
                               dptr(rot, "rot"), rot.shape[1], dptr(tr), dptr(f), dptr(cc), b, h, w, float(scale),
                               dptr(para), dptr(depth), dptr(other), dptr(depth_state, "depth_state"), stream_ptr()),
          "m4d_refiner_tail")
    return para, depth, other


def camera_pyramid(camera, levels):
    """Level-local intrinsics of DepthEstimatorPyramid.call (m4depth_network.py:300-302): a list (finest level first) of
    {"f": [b,2], "c": [b,2]} = camera / 2^(l+1), all levels from one launch."""
    f = as_f32(camera["f"], "camera['f']")
    c = as_f32(camera["c"], "camera['c']")
    b = f.shape[0]
    out = torch.empty((2, levels, b, 2), dtype=torch.float32, device=f.device)
    check(lib.m4d_camera_pyramid(dptr(f.reshape(b, 2), "camera['f']"), dptr(c.reshape(b, 2), "camera['c']"), b, int(levels),
                                 dptr(out[0]), dptr(out[1]), stream_ptr()), "m4d_camera_pyramid")
    return [{"f": out[0, l], "c": out[1, l]} for l in range(levels)]


def stream_prepare(new_traj, force_all, rot, trans):
    """One streamed frame's reset mask and pose (m4d_stream_prepare): ``new_traj`` [b] bool / uint8 on the device, ``force_all``
    a host bool.  Returns (reset uint8 [b], rot [b,rot_c], trans [b,3]) -- reset samples carry identity rotation and
    translation (0,0,1) in the pose copy, continuing samples their own pose."""
    rot = as_f32(rot, "rot")
    tr = as_f32(trans, "trans")
    if rot.dim() != 2 or rot.shape[1] not in (3, 4):
        raise ValueError('Rotation must be expressed as a small angle (x,y,z) or a quaternion (w,x,y,z)')
    b = rot.shape[0]
    if tuple(tr.shape) != (b, 3):
        raise ValueError(f"stream_prepare: trans must have shape ({b}, 3), got {tuple(tr.shape)}")
    nt = new_traj.view(torch.uint8) if new_traj.dtype == torch.bool else new_traj
    if tuple(nt.shape) != (b,):
        raise ValueError(f"stream_prepare: new_traj must have shape ({b},), got {tuple(nt.shape)}")
    reset = torch.empty((b,), dtype=torch.uint8, device=rot.device)
    rot_out = torch.empty_like(rot)
    tr_out = torch.empty_like(tr)
    check(lib.m4d_stream_prepare(dptr(nt, "new_traj", torch.uint8), int(bool(force_all)), dptr(rot, "rot"), rot.shape[1],
                                 dptr(tr, "trans"), b, dptr(reset, "reset", torch.uint8), dptr(rot_out), dptr(tr_out), stream_ptr()),
          "m4d_stream_prepare")
    return reset, rot_out, tr_out


# ---- photometric reprojection loss (csrc/m4d_photo.hip; the definition: include/m4depth_hip.h) ------------------------------
def image_pyramid_box(images, levels):
    """The image pyramid of the photometric loss (m4d_image_pyramid_box): ``images`` [n,H,W,3] in [0,1] -> list of ``levels``
    maps, level i = [n, H >> (i+1), W >> (i+1), 3], each the 2x2 mean of the one before -- views of one buffer, one call."""
    images = as_f32(images, "images")
    if images.dim() != 4 or images.shape[3] != 3:
        raise ValueError(f"images: expected [n,H,W,3], got {tuple(images.shape)}")
    n, H, W, _ = images.shape
    total = int(lib.m4d_image_pyramid_floats(n, H, W, int(levels)))
    if total < 0:
        raise ValueError(f"image_pyramid_box: {H}x{W} is no multiple of 2^{levels}")
    buf = torch.empty(total, dtype=torch.float32, device=images.device)
    check(lib.m4d_image_pyramid_box(dptr(images, "images"), n, H, W, int(levels), dptr(buf), stream_ptr()), "m4d_image_pyramid_box")
    out, off = [], 0
    for i in range(1, int(levels) + 1):
        h, w = H >> i, W >> i
        out.append(buf[off:off + n * h * w * 3].view(n, h, w, 3))
        off += n * h * w * 3
    return out


def _photo_motion(depth, rot, trans, f, c):
    depth = as_f32(depth, "depth")
    if depth.dim() != 4 or depth.shape[3] != 1:
        raise ValueError(f"depth: expected [b,h,w,1], got {tuple(depth.shape)}")
    b = depth.shape[0]
    rot = as_f32(rot, "rot")
    if rot.dim() != 2 or rot.shape[0] != b or rot.shape[1] not in (3, 4):
        raise ValueError('Rotation must be expressed as a small angle (x,y,z) or a quaternion (w,x,y,z)')
    return depth, rot, as_f32(trans, "trans").reshape(b, 3), as_f32(f, "f").reshape(b, 2), as_f32(c, "c").reshape(b, 2)


def _photo_image(img, name, b, h, w):
    img = as_f32(img, name)
    if tuple(img.shape) != (b, h, w, 3):
        raise ValueError(f"{name}: expected {(b, h, w, 3)}, got {tuple(img.shape)}")
    return img


def photo_warp_fwd(depth, rot, trans, f, c, prev):
    """m4d_photo_warp_fwd: (warped [b,h,w,3] = reproject(prev, clip(depth), ...)[0] bit for bit, dwarp [b,h,w,3] = d warped /
    d clip(depth), valid [b,h,w,1] uint8); ``f`` / ``c`` are the per-sample level cameras [b,2]."""
    depth, rot, trans, f, c = _photo_motion(depth, rot, trans, f, c)
    b, h, w, _ = depth.shape
    prev = _photo_image(prev, "prev", b, h, w)
    warped = torch.empty_like(prev)
    dwarp = torch.empty_like(prev)
    valid = torch.empty((b, h, w, 1), dtype=torch.uint8, device=depth.device)
    check(lib.m4d_photo_warp_fwd(dptr(depth, "depth"), dptr(rot, "rot"), rot.shape[1], dptr(trans), dptr(f), dptr(c), dptr(prev), b, h, w,
                                 dptr(warped), dptr(dwarp), dptr(valid, "valid", torch.uint8), stream_ptr()), "m4d_photo_warp_fwd")
    return warped, dwarp, valid


def photo_loss_fwd(depth, warped, valid, cur, prev, smooth, automask):
    """m4d_photo_loss_fwd: (out4 = (term, photo, smooth, N) float32 [4], mask [b,h,w,1] uint8)."""
    depth = as_f32(depth, "depth")
    b, h, w, _ = depth.shape
    warped, cur, prev = (_photo_image(t, n, b, h, w) for t, n in ((warped, "warped"), (cur, "cur"), (prev, "prev")))
    nbytes = int(lib.m4d_photo_workspace_bytes(b, h, w))
    if nbytes < 0:
        raise ValueError(f"photometric loss: a {b}x{h}x{w} map is refused (h, w >= 3 and b*h*w <= 2^24)")
    ws = _workspace("photo", nbytes + 8, depth.device)
    ws_ptr = ctypes.c_void_p((ws.data_ptr() + 7) // 8 * 8)
    out4 = torch.empty(4, dtype=torch.float32, device=depth.device)
    mask = torch.empty((b, h, w, 1), dtype=torch.uint8, device=depth.device)
    check(lib.m4d_photo_loss_fwd(dptr(depth, "depth"), dptr(warped), dptr(valid, "valid", torch.uint8), dptr(cur), dptr(prev), b, h, w,
                                 float(smooth), int(bool(automask)), ws_ptr, dptr(out4), dptr(mask, "mask", torch.uint8), stream_ptr()),
          "m4d_photo_loss_fwd")
    return out4, mask


def photo_loss_bwd(depth, warped, dwarp, cur, mask, out4, g_out, smooth):
    """m4d_photo_loss_bwd: g_depth [b,h,w,1] from the scalar gradient ``g_out`` (device, [1]) with the forward's mask and out4."""
    depth = as_f32(depth, "depth")
    b, h, w, _ = depth.shape
    warped, dwarp, cur = (_photo_image(t, n, b, h, w) for t, n in ((warped, "warped"), (dwarp, "dwarp"), (cur, "cur")))
    g_depth = torch.empty_like(depth)
    check(lib.m4d_photo_loss_bwd(dptr(depth, "depth"), dptr(warped), dptr(dwarp), dptr(cur), dptr(mask, "mask", torch.uint8),
                                 dptr(out4, "out4"), dptr(as_f32(g_out, "g_out").reshape(1)), b, h, w, float(smooth), dptr(g_depth),
                                 stream_ptr()), "m4d_photo_loss_bwd")
    return g_depth


# ---- full-resolution terms, minimum over two sources (include/m4depth_hip.h, "Full-resolution terms ...") -------------------
UPSAMPLE_HP_SCALES = (2, 4, 8, 16, 32, 64)


def _hp_map(x, name):
    x = as_f32(x, name)
    if x.dim() != 4 or x.shape[3] != 1:
        raise ValueError(f"{name}: expected [b,h,w,1], got {tuple(x.shape)}")
    return x


def upsample_hp(x, s):
    """m4d_upsample_hp_fwd: ``x`` [b,h,w,1] -> [b, h s, w s, 1], bilinear with half-pixel centres and edge clamp (the bits of
    the header's definition; ``interpolate(mode="bilinear", align_corners=False)`` to rounding)."""
    x = _hp_map(x, "x")
    b, h, w, _ = x.shape
    s = int(s)
    if s not in UPSAMPLE_HP_SCALES or b * h * s * w * s > 1 << 24:
        raise ValueError(f"upsample_hp: scale {s} of a {b}x{h}x{w} map is refused (s in {UPSAMPLE_HP_SCALES}, b (h s)(w s) <= 2^24)")
    out = torch.empty((b, h * s, w * s, 1), dtype=torch.float32, device=x.device)
    check(lib.m4d_upsample_hp_fwd(dptr(x, "x"), b, h, w, s, dptr(out), stream_ptr()), "m4d_upsample_hp_fwd")
    return out


def upsample_hp_bwd(g_out, s):
    """m4d_upsample_hp_bwd: the exact adjoint of ``upsample_hp``: ``g_out`` [b, h s, w s, 1] -> [b,h,w,1]; the same bits
    every run."""
    g_out = _hp_map(g_out, "g_out")
    b, H, W, _ = g_out.shape
    s = int(s)
    if s not in UPSAMPLE_HP_SCALES or H % s or W % s or b * H * W > 1 << 24 or H == 0 or W == 0:
        raise ValueError(f"upsample_hp_bwd: scale {s} of a {b}x{H}x{W} gradient is refused (s in {UPSAMPLE_HP_SCALES}, H and W "
                         "multiples of s, b H W <= 2^24)")
    g_x = torch.empty((b, H // s, W // s, 1), dtype=torch.float32, device=g_out.device)
    check(lib.m4d_upsample_hp_bwd(dptr(g_out, "g_out"), b, H // s, W // s, s, dptr(g_x), stream_ptr()), "m4d_upsample_hp_bwd")
    return g_x


def _photo_cur(cur):
    cur = as_f32(cur, "cur")
    if cur.dim() != 4 or cur.shape[3] != 3:
        raise ValueError(f"cur: expected [b,h,w,3], got {tuple(cur.shape)}")
    return cur


def photo_identity(cur, src0, src1=None):
    """m4d_photo_identity_fwd: pe_id [b,h,w] float32 = min over the given sources of pe(source, cur) at the interior pixels
    (0 elsewhere): the right-hand side of the auto-mask, independent of the depth."""
    cur = _photo_cur(cur)
    b, h, w, _ = cur.shape
    src0 = _photo_image(src0, "src0", b, h, w)
    src1 = None if src1 is None else _photo_image(src1, "src1", b, h, w)
    if int(lib.m4d_photo_min_workspace_bytes(b, h, w)) < 0:
        raise ValueError(f"photometric loss: a {b}x{h}x{w} map is refused (h, w >= 3 and b*h*w <= 2^24)")
    pe_id = torch.empty((b, h, w), dtype=torch.float32, device=cur.device)
    check(lib.m4d_photo_identity_fwd(dptr(cur, "cur"), dptr(src0), dptr(src1), b, h, w, dptr(pe_id), stream_ptr()),
          "m4d_photo_identity_fwd")
    return pe_id


def _photo_source(warped, valid, names, b, h, w):
    """One source's pair (warped [b,h,w,3], valid [b,h,w,1] uint8), both or neither."""
    if (warped is None) != (valid is None):
        raise ValueError(f"{names[0]} and {names[1]}: give both or neither")
    if warped is None:
        return None, None
    if tuple(valid.shape) != (b, h, w, 1):
        raise ValueError(f"{names[1]}: expected {(b, h, w, 1)}, got {tuple(valid.shape)}")
    return _photo_image(warped, names[0], b, h, w), valid


def photo_min_fwd(depth, warped0, valid0, warped1, valid1, cur, pe_id, smooth):
    """m4d_photo_min_fwd: (out4 = (term, photo, smooth, N) float32 [4], sel [b,h,w,1] uint8: 0 = not in the mask, 1 = source
    0, 2 = source 1).  ``warped1`` / ``valid1`` None = one source; ``pe_id`` (photo_identity) None = auto-masking off."""
    depth = _hp_map(depth, "depth")
    b, h, w, _ = depth.shape
    cur = _photo_image(cur, "cur", b, h, w)
    warped0, valid0 = _photo_source(warped0, valid0, ("warped0", "valid0"), b, h, w)
    if warped0 is None:
        raise ValueError("warped0 and valid0: source 0 is required")
    warped1, valid1 = _photo_source(warped1, valid1, ("warped1", "valid1"), b, h, w)
    if pe_id is not None and tuple(pe_id.shape) != (b, h, w):
        raise ValueError(f"pe_id: expected {(b, h, w)}, got {tuple(pe_id.shape)}")
    nbytes = int(lib.m4d_photo_min_workspace_bytes(b, h, w))
    if nbytes < 0:
        raise ValueError(f"photometric loss: a {b}x{h}x{w} map is refused (h, w >= 3 and b*h*w <= 2^24)")
    ws = _workspace("photo", nbytes + 8, depth.device)
    ws_ptr = ctypes.c_void_p((ws.data_ptr() + 7) // 8 * 8)
    out4 = torch.empty(4, dtype=torch.float32, device=depth.device)
    sel = torch.empty((b, h, w, 1), dtype=torch.uint8, device=depth.device)
    check(lib.m4d_photo_min_fwd(dptr(depth, "depth"), dptr(warped0), dptr(valid0, "valid0", torch.uint8), dptr(warped1),
                                dptr(valid1, "valid1", torch.uint8), dptr(cur), dptr(pe_id, "pe_id"), b, h, w, float(smooth), ws_ptr,
                                dptr(out4), dptr(sel, "sel", torch.uint8), stream_ptr()), "m4d_photo_min_fwd")
    return out4, sel


def photo_min_bwd(depth, warped0, dwarp0, warped1, dwarp1, cur, sel, out4, g_out, smooth):
    """m4d_photo_min_bwd: g_depth [b,h,w,1] from the scalar gradient ``g_out`` (device, [1]) with the forward's sel and out4,
    one gather over both sources."""
    depth = _hp_map(depth, "depth")
    b, h, w, _ = depth.shape
    cur = _photo_image(cur, "cur", b, h, w)
    warped0, dwarp0 = _photo_image(warped0, "warped0", b, h, w), _photo_image(dwarp0, "dwarp0", b, h, w)
    if (warped1 is None) != (dwarp1 is None):
        raise ValueError("warped1 and dwarp1: give both or neither")
    if warped1 is not None:
        warped1, dwarp1 = _photo_image(warped1, "warped1", b, h, w), _photo_image(dwarp1, "dwarp1", b, h, w)
    if tuple(sel.shape) != (b, h, w, 1):
        raise ValueError(f"sel: expected {(b, h, w, 1)}, got {tuple(sel.shape)}")
    g_depth = torch.empty_like(depth)
    check(lib.m4d_photo_min_bwd(dptr(depth, "depth"), dptr(warped0), dptr(dwarp0), dptr(warped1), dptr(dwarp1), dptr(cur),
                                dptr(sel, "sel", torch.uint8), dptr(out4, "out4"), dptr(as_f32(g_out, "g_out").reshape(1)), b, h, w,
                                float(smooth), dptr(g_depth), stream_ptr()), "m4d_photo_min_bwd")
    return g_depth
