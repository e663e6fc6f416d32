"""Host side of the photometric loss's two options (``--photo_scale``, ``--photo_sources``): the parser and its refusals, the
new entry points declared, bound and exported, their argument validation, the wrappers' refusals.  No GPU."""
import ctypes
import os
import re

import pytest


def _parse(argv, world=1):
    from m4depth_amd import main as M
    parser = M.build_parser()
    args = parser.parse_args(argv)
    M.check_train_args(parser, args, world)
    return args


def test_options_parse_and_default_to_today():
    a = _parse(["--mode", "train", "--loss", "photometric"])
    assert (a.photo_scale, a.photo_sources) == (None, None)              # unset: the model gets "level" / "prev"
    for scale in ("level", "full"):
        for sources in ("prev", "both"):
            for graph in ([], ["--graph"]):
                a = _parse(["--mode", "train", "--loss", "photometric", "--photo_scale", scale, "--photo_sources", sources] + graph)
                assert (a.photo_scale, a.photo_sources, a.graph) == (scale, sources, bool(graph))
    from m4depth_amd import training as TR
    assert TR.LOSSES == ("supervised", "photometric")
    assert TR.PHOTO_SCALES == ("level", "full") and TR.PHOTO_SOURCES == ("prev", "both")


def test_option_refusals(capsys):
    for bad, message in ((["--mode", "train", "--photo_scale", "full"], "--photo_scale needs --loss=photometric"),
                         (["--mode", "train", "--photo_scale", "level"], "--photo_scale needs --loss=photometric"),
                         (["--mode", "train", "--photo_sources", "both"], "--photo_sources needs --loss=photometric"),
                         (["--mode", "train", "--loss", "photometric", "--photo_scale", "half"], "invalid choice"),
                         (["--mode", "train", "--loss", "photometric", "--photo_sources", "next"], "invalid choice"),
                         (["--mode", "eval", "--loss", "photometric", "--photo_scale", "full"], "--loss=photometric is a --mode=train option")):
        with pytest.raises(SystemExit):
            _parse(bad)
        assert re.search(message, capsys.readouterr().err), bad


def test_loss_of_reads_the_model_settings():
    """_loss_of hands model.photo_scale / model.photo_sources on (defaults level / prev); an unknown value is refused before
    anything is launched."""
    from m4depth_amd import training as TR

    class Model:
        depth_type = "map"
    m = Model()
    m.photo_scale = "half"
    with pytest.raises(ValueError, match="scale: expected one of"):
        TR._loss_of(m, "photometric", None, [], [], {})
    m.photo_scale, m.photo_sources = "full", "next"
    with pytest.raises(ValueError, match="sources: expected one of"):
        TR._loss_of(m, "photometric", None, [], [], {})


def test_motion_inverse_on_the_host():
    import torch
    from m4depth_amd import training as TR
    rot = torch.tensor([[0.9689124, 0.1, -0.2, 0.1], [1.0, 0.0, 0.0, 0.0]])
    rot = rot / rot.norm(dim=1, keepdim=True)
    trans = torch.tensor([[0.3, -0.1, 0.05], [1.0, 2.0, 3.0]])
    ri, ti = TR.motion_inverse(rot, trans)
    rr, tt = TR.motion_inverse(ri, ti)
    assert torch.allclose(rr, rot) and torch.allclose(tt, trans, atol=1e-6)
    assert torch.equal(ti[1], -trans[1])
    with pytest.raises(ValueError, match="quaternion"):
        TR.motion_inverse(torch.zeros(2, 3), trans)


NAMES = ["m4d_upsample_hp_fwd", "m4d_upsample_hp_bwd", "m4d_photo_identity_fwd", "m4d_photo_min_workspace_bytes", "m4d_photo_min_fwd",
         "m4d_photo_min_bwd"]


def test_abi_declared_bound_exported():
    from m4depth_amd import _lib, network_ops as nops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "m4depth_hip.h")).read()
    for n in NAMES:
        assert n in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, n) and re.search(r"\b%s\s*\(" % n, header), n
    assert _lib.lib.m4d_abi_version() == 6
    for n in ("upsample_hp", "upsample_hp_bwd", "photo_identity", "photo_min_fwd", "photo_min_bwd"):
        assert callable(getattr(nops, n))


def test_argument_validation_without_gpu():
    from m4depth_amd._lib import lib
    fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)      # never dereferenced: validation fails first
    for fn in (lib.m4d_upsample_hp_fwd, lib.m4d_upsample_hp_bwd):
        assert fn(None, 2, 6, 8, 2, fake, None) == 1 and fn(fake, 2, 6, 8, 2, None, None) == 1
        for b, h, w, s in ((2, 6, 8, 3), (2, 6, 8, 128), (2, 6, 8, 1), (2, 6, 8, 0), (2, 6, 8, -2), (2, 0, 8, 2), (2, 6, 0, 2), (0, 6, 8, 2),
                           (1 << 10, 64, 64, 4), (1, 1 << 12, 1 << 12, 64)):
            assert fn(fake, b, h, w, s, fake, None) == 1, (b, h, w, s)
    ident = lambda **kw: lib.m4d_photo_identity_fwd(*[kw.get(k, d) for k, d in (
        ("cur", fake), ("src0", fake), ("src1", None), ("b", 2), ("h", 6), ("w", 8), ("pe_id", fake))], None)
    for ptr in ("cur", "src0", "pe_id"):
        assert ident(**{ptr: None}) == 1, ptr
    assert ident(h=2) == 1 and ident(w=2) == 1 and ident(b=0) == 1 and ident(b=1 << 12, h=1 << 7, w=1 << 7) == 1
    assert lib.m4d_photo_min_workspace_bytes(2, 24, 40) == lib.m4d_photo_workspace_bytes(2, 24, 40) == 2 * 2 * 3 * 3 * 8
    assert lib.m4d_photo_min_workspace_bytes(2, 2, 40) == -1 and lib.m4d_photo_min_workspace_bytes(1 << 12, 1 << 7, 1 << 7) == -1
    fwd = lambda **kw: lib.m4d_photo_min_fwd(*[kw.get(k, d) for k, d in (
        ("depth", fake), ("warped0", fake), ("valid0", fake), ("warped1", fake), ("valid1", fake), ("cur", fake), ("pe_id", fake),
        ("b", 2), ("h", 6), ("w", 8), ("smooth", 1e-3), ("ws", fake), ("out4", fake), ("sel", fake))], None)
    for ptr in ("depth", "warped0", "valid0", "cur", "ws", "out4", "sel", "warped1", "valid1"):     # one half of source 1: refused
        assert fwd(**{ptr: None}) == 1, ptr
    assert fwd(ws=odd) == 1 and fwd(h=2) == 1 and fwd(w=1) == 1 and fwd(b=-1) == 1
    bwd = lambda **kw: lib.m4d_photo_min_bwd(*[kw.get(k, d) for k, d in (
        ("depth", fake), ("warped0", fake), ("dwarp0", fake), ("warped1", fake), ("dwarp1", fake), ("cur", fake), ("sel", fake),
        ("out4", fake), ("g_out", fake), ("b", 2), ("h", 6), ("w", 8), ("smooth", 1e-3), ("g_depth", fake))], None)
    for ptr in ("depth", "warped0", "dwarp0", "cur", "sel", "out4", "g_out", "g_depth", "warped1", "dwarp1"):
        assert bwd(**{ptr: None}) == 1, ptr
    assert bwd(h=2) == 1 and bwd(w=2) == 1 and bwd(b=0) == 1


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    import torch
    from m4depth_amd import network_ops as nops
    with pytest.raises(ValueError, match=r"x: expected \[b,h,w,1\]"):
        nops.upsample_hp(torch.zeros(1, 8, 8), 2)
    with pytest.raises(ValueError, match="scale 3"):
        nops.upsample_hp(torch.zeros(1, 8, 8, 1), 3)
    with pytest.raises(ValueError, match="multiples of s"):
        nops.upsample_hp_bwd(torch.zeros(1, 9, 8, 1), 2)
    with pytest.raises(RuntimeError, match="MI355X only"):
        nops.upsample_hp(torch.zeros(1, 8, 8, 1), 2)
    with pytest.raises(ValueError, match=r"cur: expected \[b,h,w,3\]"):
        nops.photo_identity(torch.zeros(1, 8, 8, 1), torch.zeros(1, 8, 8, 3))
    with pytest.raises(ValueError, match="src1: expected"):
        nops.photo_identity(torch.zeros(1, 8, 8, 3), torch.zeros(1, 8, 8, 3), torch.zeros(1, 8, 9, 3))
    d, img, v = torch.zeros(1, 8, 8, 1), torch.zeros(1, 8, 8, 3), torch.zeros(1, 8, 8, 1, dtype=torch.uint8)
    with pytest.raises(ValueError, match="give both or neither"):
        nops.photo_min_fwd(d, img, v, img, None, img, None, 1e-3)
    with pytest.raises(ValueError, match="pe_id: expected"):
        nops.photo_min_fwd(d, img, v, None, None, img, torch.zeros(1, 8, 9), 1e-3)
    with pytest.raises(ValueError, match="give both or neither"):
        nops.photo_min_bwd(d, img, img, img, None, img, v, torch.zeros(4), torch.zeros(1), 1e-3)
    with pytest.raises(ValueError, match="sel: expected"):
        nops.photo_min_bwd(d, img, img, None, None, img, torch.zeros(1, 8, 8, dtype=torch.uint8), torch.zeros(4), torch.zeros(1), 1e-3)
