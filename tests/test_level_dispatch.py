"""The launches of ``DepthEstimatorLevel.forward`` against a recorded trace.

``tests/golden/level_dispatch_snapshot.json`` was recorded on an MI355X from ``DepthEstimatorLevel.forward`` at commit 4aa959b,
BEFORE its launch choice moved into ``DepthEstimatorLevel.plan``: the expected values come from that code path, never from
``plan``.  A recorder stands in for every launch entry point of the one ``_lib.lib`` object (the ``m4d_*`` functions that take a
stream; the ``*_supported`` queries launch nothing and are left alone) and passes the call on.  Per launch a row holds the
symbol, every scalar argument verbatim and every pointer argument as ``null`` or ``[label, byte offset]``: a label names a
tensor the test knows -- the level's two state buffers, its depth state, the refiner-input buffer, the inputs, the two
parallax maps ``level_pre`` hands to the cost volumes -- and any other pointer is ``"tmp"``.

Every case runs ONE level: a reset call, then one full step.  The GPU test replays the cases through today's ``forward`` and
wants the recorded rows; the CPU test wants ``plan`` to name, for every case, what the recorded launches imply."""
import contextlib
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from m4depth_amd import _lib
from m4depth_amd import network as N
from m4depth_amd import network_ops as nops
from m4depth_amd.synthetic import ENCODER_CHANNELS

SNAPSHOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "level_dispatch_snapshot.json")
ABLATIONS = ("SNCV", "time_recurr", "normalize_features", "level_memory")
SWITCHES = ("fused_front", "fused_refiner_tail", "tail_split")


def _case(ranges=(4, 3), depth=2, shape=(1, 64, 64), mode="plain", off=None, switch=None, arith=None, training=False,
          hand_prenormalized=True):
    return {"ranges": ranges, "depth": depth, "shape": shape, "mode": mode, "off": off, "switch": switch, "arith": arith,
            "training": training, "hand_prenormalized": hand_prenormalized}


def _cases():
    """name -> case.  ``mode``: "plain" (reset call, full step), "masked" (the step carries ``reset_mask`` [1, 0]), "explicit"
    (the step carries ``prev_f_maps`` / ``prev_t_depth``).  ``off``: an ablation switched off; ``switch``: a module switch
    switched off; ``arith``: the convolution arithmetic; ``hand_prenormalized``: hand the level per-cut normalised features
    whenever it ``wants_prenormalized`` them."""
    out = {}
    for ranges, depths, hw in [((4, 3), (1, 2, 3), 64), ((4, 3), (4, 5, 6), 64), ((4, 3), (4, 5, 6), 80),
                               ((2, 2), range(1, 7), 64), ((2, 2), range(1, 7), 80), ((6, 6), (4, 5), 64), ((6, 6), (6,), 80)]:
        for d in depths:
            out[f"r{ranges[0]}{ranges[1]}_d{d}_{hw}x{hw}"] = _case(ranges, d, (1, hw, hw))
    for d in (4, 5, 6):                               # a coarse level whose caller did not normalise ahead of it
        out[f"raw_d{d}_64x64"] = _case(depth=d, hand_prenormalized=False)
    for d in (2, 5):
        for b, h, w in ((2, 32, 64), (2, 40, 80)):
            out[f"masked_d{d}_{h}x{w}"] = _case(depth=d, shape=(b, h, w), mode="masked")
        for training in (False, True):
            out[f"explicit_d{d}_{'training' if training else 'inference'}"] = _case(depth=d, mode="explicit", training=training)
        for ab in ABLATIONS:
            out[f"no_{ab}_d{d}"] = _case(depth=d, off=ab)
        for sw in SWITCHES:
            out[f"{sw}_off_d{d}"] = _case(depth=d, switch=sw)
        for arith in ("f32", "bf16x3"):
            out[f"{arith}_d{d}"] = _case(depth=d, arith=arith)
    return out


CASES = _cases()


@contextlib.contextmanager
def _configured(case):
    """The module switch and the arithmetic of a case, restored on exit."""
    old = {sw: getattr(N, sw) for sw in SWITCHES}
    try:
        if case["switch"] is not None:
            setattr(N, case["switch"], False)
        with N.conv_arithmetic(case["arith"] or "f16x2"):
            yield
    finally:
        for sw, v in old.items():
            setattr(N, sw, v)


def _level(case):
    ablation = N.M4depthAblationParameters(**({case["off"]: False} if case["off"] else {}))
    settings = {"nbre_lvls": 6, "is_training": case["training"], "ablation": ablation, "dscv_range": case["ranges"][0],
                "sncv_range": case["ranges"][1]}
    torch.manual_seed(0)
    return N.DepthEstimatorLevel(settings, case["depth"])


def _map_shape(case):
    b, h, w = case["shape"]
    return b, h, w, ENCODER_CHANNELS[case["depth"] - 1]


def _launch_symbols():
    return [n for n in _lib._SIGNATURES if not n.endswith("_supported")]


@contextlib.contextmanager
def _recording(log):
    """Every launch entry point of ``_lib.lib`` logs (symbol, raw arguments) into ``log`` and runs."""
    real = {n: getattr(_lib.lib, n) for n in _launch_symbols()}

    def recorder(name, fn):
        def rec(*args):
            row = []
            for a, t in zip(args, fn.argtypes):
                if t is ctypes.c_void_p and (a is None or isinstance(a, (int, ctypes.c_void_p))):
                    row.append(("ptr", (a.value if isinstance(a, ctypes.c_void_p) else a) or None))
                elif isinstance(a, (int, float)):
                    row.append(("scalar", a))
                else:               # a host array: the structs of m4d_pyramid_reset / m4d_normalize_levels, a ``dims[6]``
                    row.append(("scalar", type(a).__name__))
            log.append((name, row))
            return fn(*args)
        return rec
    try:
        for n, fn in real.items():
            setattr(_lib.lib, n, recorder(n, fn))
        yield
    finally:
        for n, fn in real.items():
            setattr(_lib.lib, n, fn)


def _resolve(log, labels):
    """The rows of a call: pointers as null, [label, byte offset] or "tmp"."""
    spans = [(name, t.untyped_storage().data_ptr(), t.untyped_storage().nbytes()) for name, t in labels.items()
             if isinstance(t, torch.Tensor) and t.is_cuda]

    def pointer(p):
        if p is None:
            return None
        for name, base, nbytes in spans:
            if base <= p < base + nbytes:
                return [name, p - base]
        return "tmp"
    return [[name] + [pointer(v) if kind == "ptr" else v for kind, v in row] for name, row in log]


def record_case(case, dev):
    """{"prenormalized": were normalised features handed in, "calls": [rows of the reset call, rows of the step]}."""
    b, h, w, c = _map_shape(case)
    gen = torch.Generator().manual_seed(1234)

    def rand(*shape, lo=None, hi=None):
        x = torch.randn(*shape, generator=gen) if lo is None else lo + (hi - lo) * torch.rand(*shape, generator=gen)
        return x.to(dev)
    with _configured(case), torch.no_grad():
        level = _level(case).to(dev)
        camera = {"f": torch.tensor([[float(w), float(w)]] * b, device=dev), "c": torch.tensor([[w / 2., h / 2.]] * b, device=dev)}
        hand = case["hand_prenormalized"] and bool(level.wants_prenormalized(b, h, w, c))
        calls, state = [], {}
        for step in (0, 1):
            inputs = {"curr_f_maps": rand(b, h, w, c), "rot": 0.01 * rand(b, 3), "trans": rand(b, 3), "cam_f": camera["f"],
                      "cam_c": camera["c"]}
            prev_l = None
            if case["depth"] < 6:                     # (the coarsest level of a pyramid has no coarser estimate)
                ph, pw = (h + 1) // 2, (w + 1) // 2
                prev_l = {"depth": rand(b, ph, pw, 1, lo=1., hi=50.), "parallax": rand(b, ph, pw, 1, lo=.2, hi=2.),
                          "other": rand(b, ph, pw, 4)}
                inputs.update({f"prev_l.{k}": v for k, v in prev_l.items()})
            kw = {}
            if hand:
                kw["curr_f_normalized"] = inputs["curr_f_normalized"] = nops.normalize_cuts(inputs["curr_f_maps"], level.nbre_cuts)
            new_traj = np.full([b], step == 0)
            if step == 1 and case["mode"] == "masked":
                new_traj = None
                kw["reset_mask"] = inputs["reset_mask"] = torch.tensor([1, 0], dtype=torch.uint8, device=dev)
                kw["reset_parallax"] = 4.0
            if step == 1 and case["mode"] == "explicit":
                kw["prev_f_maps"] = inputs["prev_f_maps"] = state["features"]
                kw["prev_t_depth"] = inputs["prev_t_depth"] = state["depth"]
            log = []
            with _recording(log):
                est = level(inputs["curr_f_maps"], prev_l, inputs["rot"], inputs["trans"], camera, new_traj, **kw)
            torch.cuda.synchronize()
            state = {"features": inputs["curr_f_maps"], "depth": est["depth"]}
            labels = dict(inputs)
            if level._own is not None:
                labels.update({"state0": level._own[0], "state1": level._own[1], "depth_state": level.depth_prev_t})
            if step == 1:                             # (both live from the top of the call to its end: no address is reused)
                labels["f_input"] = level.last_f_input
                labels["para_prev_t"], labels["para_prev_l"] = level.last_cv_inputs[2:4]
            calls.append(_resolve(log, labels))
    return {"prenormalized": hand, "calls": calls}


def snapshot(dev):
    return {"recorded_at": "4aa959b", "row": ["symbol", "arguments in ABI order: scalar | null | [label, byte offset] | 'tmp'"],
            "cases": {name: record_case(case, dev) for name, case in CASES.items()}}


@functools.lru_cache(maxsize=None)
def _load():
    with open(SNAPSHOT) as fh:
        return json.load(fh)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_forward_launches_the_recorded_trace(dev, name):
    want = _load()["cases"][name]
    got = json.loads(json.dumps(record_case(CASES[name], dev)))
    assert got["prenormalized"] == want["prenormalized"]
    for call, (g_rows, w_rows) in enumerate(zip(got["calls"], want["calls"])):
        assert [r[0] for r in g_rows] == [r[0] for r in w_rows], (name, call)
        for g, w in zip(g_rows, w_rows):
            assert g == w, (name, call, g, w)


# -- what a recorded call says about the plan: the mapping from launch names and arguments to ``LevelPlan`` fields ----------
_ROUTE = {"m4d_level_front_r": "front", "m4d_level_front_small": "front_small", "m4d_dscv_sncv_fwd": "dscv_sncv",
          "m4d_dscv_fwd": "dscv+sncv"}                # (with SNCV ablated the second launch of "dscv+sncv" does not exist)
_TAIL = {"m4d_refiner_tail6": "tail6", "m4d_refiner_tail6_m": "tail6", "m4d_refiner_tail": "tail", "m4d_refiner_tail_m": "tail",
         "m4d_level_post": "post", "m4d_level_post_m": "post"}
# position of the refiner-input row stride among the arguments of the launch that opens a full step
_STRIDE_ARG = {"m4d_level_front_r": 22, "m4d_level_front_small": 21, "m4d_level_pre": 17, "m4d_level_pre_normalize": 17}


def implied_plan(rows):
    """(route, normalize, f_stride, tail) of a recorded call."""
    symbols = [r[0] for r in rows]
    routes = [_ROUTE[s] for s in symbols if s in _ROUTE]
    tails = [_TAIL[s] for s in symbols if s in _TAIL]
    assert len(routes) <= 1 and len(tails) <= 1, symbols
    if "m4d_level_pre_normalize" in symbols:
        normalize = "with_pre"
    else:
        normalize = {"front": "in_front", "front_small": "prenormalized"}.get(routes[0] if routes else None, "separate")
    if not routes:                                    # the reset branch: level_pre alone (and the separate normalisation)
        assert set(symbols) <= {"m4d_level_pre", "m4d_level_pre_normalize", "m4d_normalize_cuts"}, symbols
        return "reset", normalize, None, None
    opening = next(r for r in rows if r[0] in _STRIDE_ARG)
    return routes[0], normalize, opening[1 + _STRIDE_ARG[opening[0]]], tails[0]


def test_plan_names_what_the_recorded_launches_imply():
    recorded = _load()["cases"]
    assert set(recorded) == set(CASES)
    for name, case in CASES.items():
        with _configured(case):
            level = _level(case)
            for step, rows in enumerate(recorded[name]["calls"]):
                own_state = not case["training"] and not (step == 1 and case["mode"] == "explicit")
                # a masked call never reads new_traj; a training level without a previous depth takes the reset branch
                reset = step == 0
                p = level.plan(*_map_shape(case), gpu=True, own_state=own_state, reset=reset,
                               prenormalized=recorded[name]["prenormalized"])
                route, normalize, f_stride, tail = implied_plan(rows)
                assert (p.route, p.normalize) == (route, normalize), (name, step, p, route, normalize)
                if route != "reset":
                    assert (p.f_stride, p.tail) == (f_stride, tail), (name, step, p, f_stride, tail)
