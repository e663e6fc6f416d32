"""Host side of the multi-view depth check: the header's declarations, argument validation of m4d_depth_views without a device,
the ring-size helper, the wrappers', the writer's and the driver's refusals and defaults, the confidence PNG round trip."""
import ctypes
import os

import numpy as np
import pytest

FAKE = ctypes.c_void_p(4096)                 # never dereferenced: validation fails first
FAKE2 = ctypes.c_void_p(8192)


def _views(**over):
    from m4depth_amd._lib import lib
    a = dict(depth=FAKE, depth_stride=12, cam_f=FAKE, cam_c=FAKE, pose=FAKE, reset=FAKE, force_all=0, b=2, h=3, w=4, views=4,
             head=0, ring_depth=FAKE, ring_pose=FAKE, age_in=FAKE, age_out=FAKE2, tol_px=1.0, tol_rel=0.01, min_views=2,
             n_views=FAKE, depth_f=FAKE)
    a.update(over)
    return lib.m4d_depth_views(a["depth"], a["depth_stride"], a["cam_f"], a["cam_c"], a["pose"], a["reset"], a["force_all"],
                               a["b"], a["h"], a["w"], a["views"], a["head"], a["ring_depth"], a["ring_pose"], a["age_in"],
                               a["age_out"], a["tol_px"], a["tol_rel"], a["min_views"], a["n_views"], a["depth_f"], None)


REFUSED = {
    "null depth": dict(depth=None), "null cam_f": dict(cam_f=None), "null cam_c": dict(cam_c=None), "null pose": dict(pose=None),
    "null ring_depth": dict(ring_depth=None), "null ring_pose": dict(ring_pose=None), "null age_in": dict(age_in=None),
    "null age_out": dict(age_out=None), "null n_views": dict(n_views=None),
    "empty batch": dict(b=0), "negative batch": dict(b=-1), "batch above the grid": dict(b=65536),
    "one row": dict(h=1), "one column": dict(w=1), "no rows": dict(h=0), "negative columns": dict(w=-4),
    "too many pixels": dict(h=4097, w=4096, depth_stride=4097 * 4096),
    "no views": dict(views=0), "nine views": dict(views=9, min_views=2), "negative views": dict(views=-1),
    "head negative": dict(head=-1), "head above views": dict(head=5),
    "min_views zero": dict(min_views=0), "min_views above views": dict(min_views=5),
    "tol_px zero": dict(tol_px=0.0), "tol_px negative": dict(tol_px=-1.0), "tol_px nan": dict(tol_px=float("nan")),
    "tol_rel zero": dict(tol_rel=0.0), "tol_rel negative": dict(tol_rel=-0.01), "tol_rel nan": dict(tol_rel=float("nan")),
    "ages alias": dict(age_out=FAKE),
    "depth stride": dict(depth_stride=11),
    "misaligned depth": dict(depth=ctypes.c_void_p(4098)), "misaligned cam_f": dict(cam_f=ctypes.c_void_p(4097)),
    "misaligned cam_c": dict(cam_c=ctypes.c_void_p(4099)), "misaligned pose": dict(pose=ctypes.c_void_p(4100)),
    "misaligned ring_depth": dict(ring_depth=ctypes.c_void_p(4098)), "misaligned ring_pose": dict(ring_pose=ctypes.c_void_p(4100)),
    "misaligned age_in": dict(age_in=ctypes.c_void_p(4098)), "misaligned age_out": dict(age_out=ctypes.c_void_p(8193)),
    "misaligned depth_f": dict(depth_f=ctypes.c_void_p(4098)),
}


@pytest.mark.parametrize("why", sorted(REFUSED))
def test_depth_views_refuses_without_a_device(why):
    from m4depth_amd._lib import lib
    n0 = lib.m4d_launch_count()
    assert _views(**REFUSED[why]) == 1, why
    assert lib.m4d_launch_count() == n0, "a refusal must not launch"


def test_ring_floats():
    from m4depth_amd._lib import lib
    for b, h, w, k in ((1, 2, 2, 1), (3, 37, 53, 4), (8, 384, 512, 8), (1, 4096, 4096, 8), (65535, 2, 2, 1)):
        assert lib.m4d_depth_views_ring_floats(b, h, w, k) == (k + 1) * b * h * w
    for b, h, w, k in ((0, 4, 4, 1), (1, 1, 4, 1), (1, 4, 1, 1), (1, 4, 4, 0), (1, 4, 4, 9), (1, 4097, 4096, 1), (65536, 4, 4, 1)):
        assert lib.m4d_depth_views_ring_floats(b, h, w, k) == -1


def test_header_declares_the_entry_points():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "m4depth_hip.h")).read()
    for decl in ("int m4d_depth_views(", "long long m4d_depth_views_ring_floats("):
        assert decl in txt, decl
    section = txt[txt.index("Multi-view depth check"):txt.index("int m4d_depth_views(")]
    for word in ("get_rot_mat", "R(qk)^T R(qc)", "0x7FC00000", "age_out[s] = min(a + 1, K)", "ABI 6 unchanged"):
        assert word in section, word
    assert "#define M4D_ABI_VERSION 6 " in txt
    from m4depth_amd._lib import SIGNATURES
    restype, argtypes, names = SIGNATURES["m4d_depth_views"]
    assert restype is ctypes.c_int and len(argtypes) == 22 and names[-1] == "stream" and names[0] == "depth"
    assert argtypes[1] is ctypes.c_longlong and argtypes[16] is ctypes.c_float and argtypes[5] is ctypes.c_void_p


def test_wrappers_refuse_before_any_pointer_is_taken():
    import torch
    from m4depth_amd import network_ops as nops
    for bad in (dict(b=0), dict(h=1), dict(views=0), dict(views=9)):
        with pytest.raises(ValueError, match="depth_views_state"):
            nops.depth_views_state(**dict(dict(b=2, h=3, w=4, views=4, device="cpu"), **bad))
    st = nops.depth_views_state(2, 3, 4, 4, "cpu")
    assert st["ring_depth"].shape == (5, 2, 3, 4) and st["ring_depth"].dtype == torch.float32
    assert st["ring_pose"].shape == (5, 2, 7) and st["ring_pose"].dtype == torch.float64
    assert st["head"] == 0 and st["views"] == 4 and len(st["age"]) == 2
    assert all(a.dtype == torch.int32 and a.shape == (2,) and not a.any() for a in st["age"])
    assert st["age"][0].data_ptr() != st["age"][1].data_ptr()
    depth, f, pose = torch.zeros(2, 3, 4, 1), torch.ones(2, 2), torch.zeros((2, 7), dtype=torch.float64)
    with pytest.raises(ValueError, match=r"\[b,h,w,1\]"):
        nops.depth_views(torch.zeros(2, 3, 4), f, f, pose, st)
    with pytest.raises(ValueError, match="min_views"):
        nops.depth_views(depth, f, f, pose, st, min_views=5)
    with pytest.raises(ValueError, match="tol_px"):
        nops.depth_views(depth, f, f, pose, st, tol_px=0.0)
    with pytest.raises(ValueError, match="cam_f"):
        nops.depth_views(depth, torch.ones(2, 3), f, pose, st)
    with pytest.raises(ValueError, match="float64"):
        nops.depth_views(depth, f, f, pose.float(), st)
    with pytest.raises(ValueError, match="reset"):
        nops.depth_views(depth, f, f, pose, st, reset=torch.zeros(3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="reset"):
        nops.depth_views(depth, f, f, pose, st, reset=torch.zeros(2))
    with pytest.raises(ValueError, match="state"):
        nops.depth_views(torch.zeros(2, 5, 4, 1), f, f, pose, st)
    with pytest.raises(TypeError, match="float32 device tensor"):
        nops.depth_views(depth, f, f, pose, st)
    assert st["head"] == 0                                                      # a refused call advances nothing


def test_writer_refuses_bad_options(tmp_path):
    from m4depth_amd.export import PredictionWriter
    out = str(tmp_path)
    for kw, match in ((dict(cloud=True, cloud_views=9), "cloud_views"), (dict(cloud=True, cloud_views=-1), "cloud_views"),
                      (dict(cloud_views=2), "needs cloud=True"), (dict(cloud=True, save_conf=True), "save_conf needs cloud_views"),
                      (dict(cloud=True, cloud_min_views=1), "cloud_min_views needs cloud_views"),
                      (dict(cloud=True, cloud_views=2, cloud_min_views=3), "cloud_min_views"),
                      (dict(cloud=True, cloud_views=2, cloud_min_views=0), "cloud_min_views"),
                      (dict(cloud=True, cloud_views=2, cloud_tol=(0.0, 0.01)), "cloud_tol"),
                      (dict(cloud=True, cloud_views=2, cloud_tol=(1.0, float("nan"))), "cloud_tol"),
                      (dict(cloud=True, cloud_views=2, cloud_tol=(1.0,)), "cloud_tol")):
        with pytest.raises(ValueError, match=match):
            PredictionWriter(out, "kitti16", **kw)
    w = PredictionWriter(out, "kitti16")
    assert (w.cloud_views, w.save_conf, w.cloud_tol) == (0, False, (1.0, 0.01))
    w.close()
    for k, want in ((1, 1), (2, 2), (8, 2)):
        w = PredictionWriter(out, "kitti16", cloud=True, cloud_views=k)
        assert (w.cloud_views, w.cloud_min_views) == (k, want)
        w.close()


def _refused(argv, capsys, match):
    from m4depth_amd import main as MAIN
    with pytest.raises(SystemExit) as e:
        MAIN.main(argv)
    assert e.value.code == 2
    assert match in capsys.readouterr().err


def test_driver_refusals(tmp_path, capsys):
    out = str(tmp_path / "out")
    base = ["--mode", "predict", "--save_dir", out]
    _refused(["--mode", "predict", "--cloud_views", "4"], capsys, "--cloud_views needs --save_cloud")
    _refused(base + ["--cloud_views", "4"], capsys, "--cloud_views needs --save_cloud")
    _refused(base + ["--cloud_min_views", "1"], capsys, "--cloud_min_views needs --save_cloud")
    _refused(base + ["--cloud_tol", "1", "0.01"], capsys, "--cloud_tol needs --save_cloud")
    _refused(base + ["--save_conf"], capsys, "--save_conf needs --save_cloud")
    _refused(["--mode", "predict", "--save_cloud", "--cloud_views", "4"], capsys, "--save_cloud needs --save_dir")
    cloud = base + ["--save_cloud"]
    _refused(cloud + ["--save_conf"], capsys, "--save_conf needs --cloud_views")
    _refused(cloud + ["--cloud_min_views", "1"], capsys, "--cloud_min_views needs --cloud_views")
    _refused(cloud + ["--cloud_tol", "1", "0.01"], capsys, "--cloud_tol needs --cloud_views")
    _refused(cloud + ["--cloud_views", "0", "--save_conf"], capsys, "--save_conf needs --cloud_views")
    _refused(cloud + ["--cloud_views", "9"], capsys, "--cloud_views must be 0 (off) or 1..8")
    _refused(cloud + ["--cloud_views", "-1"], capsys, "--cloud_views must be 0 (off) or 1..8")
    _refused(cloud + ["--cloud_views", "4", "--cloud_min_views", "5"], capsys, "--cloud_min_views must be in 1..4")
    _refused(cloud + ["--cloud_views", "4", "--cloud_min_views", "0"], capsys, "--cloud_min_views must be in 1..4")
    _refused(cloud + ["--cloud_views", "4", "--cloud_tol", "0", "0.01"], capsys, "--cloud_tol PX REL needs PX > 0 and REL > 0")
    _refused(cloud + ["--cloud_views", "4", "--cloud_tol", "1", "-0.01"], capsys, "--cloud_tol PX REL needs PX > 0 and REL > 0")
    assert not os.path.exists(out)


def test_driver_defaults():
    from m4depth_amd import main as MAIN
    parser = MAIN.build_parser()
    args = parser.parse_args(["--mode", "predict", "--save_dir", "x", "--save_cloud"])
    MAIN.check_save_args(parser, args)
    assert args.cloud_views == 0 and not args.save_conf and args.cloud_tol == (1.0, 0.01) and args.cloud_min_views is None
    for k, want in ((1, 1), (4, 2), (8, 2)):
        args = parser.parse_args(["--mode", "predict", "--save_dir", "x", "--save_cloud", "--cloud_views", str(k)])
        MAIN.check_save_args(parser, args)
        assert (args.cloud_views, args.cloud_min_views, args.cloud_tol, args.save_conf) == (k, want, (1.0, 0.01), False)
    args = parser.parse_args(["--mode", "predict", "--save_dir", "x", "--save_cloud", "--cloud_views", "3", "--cloud_min_views", "3",
                              "--cloud_tol", "0.5", "0.02", "--save_conf"])
    MAIN.check_save_args(parser, args)
    assert (args.cloud_views, args.cloud_min_views, args.cloud_tol, args.save_conf) == (3, 3, (0.5, 0.02), True)
    args = parser.parse_args(["--mode", "predict"])
    MAIN.check_save_args(parser, args)
    assert args.cloud_views == 0 and not args.save_conf


@pytest.mark.parametrize("views", [1, 3, 4, 7, 8])
def test_conf_png_round_trip(tmp_path, views):
    from PIL import Image
    from m4depth_amd.export import read_conf_png
    rng = np.random.default_rng(views)
    counts = rng.integers(0, views + 1, (9, 13)).astype(np.uint8)
    counts[0, :views + 1] = np.arange(views + 1)
    path = str(tmp_path / "c_conf.png")
    Image.fromarray((counts.astype(np.uint16) * 255 // views).astype(np.uint8)).save(path, format="PNG")
    got = read_conf_png(path, views)
    assert got.dtype == np.uint8 and np.array_equal(got, counts)
    with pytest.raises(ValueError, match="views"):
        read_conf_png(path, 0)
    if views == 4:
        Image.fromarray(np.full((4, 4), 100, np.uint8)).save(path, format="PNG")
        with pytest.raises(ValueError, match="not the confirmation counts"):
            read_conf_png(path, 4)
        Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(path, format="PNG")
        with pytest.raises(ValueError, match="8-bit grey"):
            read_conf_png(path, 4)
