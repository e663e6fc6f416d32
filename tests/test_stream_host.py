"""Streaming inference, host side (no GPU): the entry points of the masked level close and of the per-frame prepare kernel are
declared in include/m4depth_hip.h, bound by m4depth_amd/_lib.py and exported by the library; their argument validation returns
hipErrorInvalidValue (1) without touching a device; main.py's --stream flag parses and is refused outside --mode=predict."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_SYMBOLS = ["m4d_refiner_tail6_m", "m4d_refiner_tail_m", "m4d_level_post_m", "m4d_stream_prepare"]


def _declared():
    txt = open(os.path.join(ROOT, "include", "m4depth_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(m4d_[a-z0-9_]+)\s*\(", txt))


def test_stream_symbols_declared_bound_exported():
    from m4depth_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    declared = _declared()
    for s in STREAM_SYMBOLS:
        assert s in declared, f"{s} not declared in include/m4depth_hip.h"
        assert s in _lib.EXPORTED_SYMBOLS, f"{s} not bound in m4depth_amd/_lib.py"
        assert hasattr(raw, s), f"{s} not exported by the library"
    # one more argument each than the unmasked entry points: the mask and the reset parallax (the stream stays last)
    for masked, plain in (("m4d_refiner_tail6_m", "m4d_refiner_tail6"), ("m4d_refiner_tail_m", "m4d_refiner_tail"),
                          ("m4d_level_post_m", "m4d_level_post")):
        a, p = _lib.SIGNATURES[masked][1], _lib.SIGNATURES[plain][1]
        assert a[:-1] == p[:-1] + (ctypes.c_void_p, ctypes.c_float) and a[-1] == p[-1]
    assert _lib.lib.m4d_abi_version() == 6


def test_stream_entry_points_validate_without_device():
    from m4depth_amd._lib import lib
    fake = ctypes.c_void_p(4096)            # never dereferenced: validation fails first
    # m4d_stream_prepare: null pointers, b <= 0, a rotation that is neither small-angle nor quaternion
    assert lib.m4d_stream_prepare(None, 0, None, 3, None, 1, None, None, None, None) == 1
    assert lib.m4d_stream_prepare(fake, 0, fake, 3, fake, 1, None, fake, fake, None) == 1
    assert lib.m4d_stream_prepare(fake, 1, fake, 3, fake, 0, fake, fake, fake, None) == 1
    assert lib.m4d_stream_prepare(fake, 1, fake, 5, fake, 2, fake, fake, fake, None) == 1
    # the masked closes need the mask and the depth state
    for fn in (lib.m4d_refiner_tail6_m, lib.m4d_refiner_tail_m):
        assert fn(None, None, None, None, None, None, 4, None, None, None, 1, 8, 8, 1.0, None, None, None, None, None, 1.0, None) == 1
        assert fn(fake, fake, fake, fake, fake, fake, 4, fake, fake, fake, 1, 8, 8, 1.0, fake, fake, fake, fake, None, 1.0, None) == 1
        assert fn(fake, fake, fake, fake, fake, fake, 4, fake, fake, fake, 1, 8, 8, 1.0, fake, fake, fake, None, fake, 1.0, None) == 1
        assert fn(fake, fake, fake, fake, fake, fake, 4, fake, fake, fake, 0, 8, 8, 1.0, fake, fake, fake, fake, fake, 1.0, None) == 1
    assert lib.m4d_level_post_m(fake, fake, 4, fake, fake, fake, 1, 8, 8, 1.0, fake, fake, fake, fake, None, 1.0, None) == 1
    assert lib.m4d_level_post_m(fake, fake, 4, fake, fake, fake, 1, 8, 8, 1.0, fake, fake, fake, None, fake, 1.0, None) == 1
    assert lib.m4d_level_post_m(fake, fake, 5, fake, fake, fake, 1, 8, 8, 1.0, fake, fake, fake, fake, fake, 1.0, None) == 1


def test_stream_flag_parses_and_is_predict_only():
    from m4depth_amd import main as MN
    args = MN.build_parser().parse_args(["--mode=predict", "--stream", "--graph"])
    assert args.stream and args.graph
    assert not MN.build_parser().parse_args(["--mode=predict"]).stream          # default off: existing runs unchanged
    for mode in ("eval", "train", "validation", "finetune"):
        with pytest.raises(SystemExit) as e:
            MN.main([f"--mode={mode}", "--stream"])
        assert e.value.code == 2


def test_stream_step_refuses_cpu_frames_and_training_models():
    """The streaming entry points never fall back to the host: a CPU frame and a training-mode model are refused before any
    kernel is launched."""
    import torch
    import m4depth_amd as M
    model = M.M4Depth(nbre_levels=2)
    frame = {"RGB_im": torch.zeros(2, 16, 16, 3), "rot": torch.zeros(2, 4), "trans": torch.zeros(2, 3),
             "new_traj": torch.zeros(2, dtype=torch.bool), "camera": {"f": torch.ones(2, 2), "c": torch.ones(2, 2)}}
    with pytest.raises(RuntimeError, match="device"):
        model.stream_step(frame)
    with pytest.raises(RuntimeError, match="is_training=False"):
        M.M4Depth(nbre_levels=2, is_training=True).stream_step(frame)
    bad = dict(frame, trans=torch.zeros(2, 4))
    with pytest.raises(ValueError, match="trans"):
        model.stream_step(bad)
    with pytest.raises(ValueError, match="RGB_im"):
        model.stream_step(dict(frame, RGB_im=torch.zeros(16, 16, 3)))
