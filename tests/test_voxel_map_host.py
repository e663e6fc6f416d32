"""Host side of the voxel maps (main.py --save_map): the option refusals, the writer's refusals, the map file's round trip and
the C entries' argument checks -- nothing here launches a kernel."""
import ctypes
import os

import numpy as np
import pytest
import torch

from voxel_map_ref import VoxelMap, vertices_of


def _refused(argv, capsys, match):
    from m4depth_amd import main as MAIN
    with pytest.raises(SystemExit) as e:
        MAIN.main(argv)
    assert e.value.code == 2
    assert match in capsys.readouterr().err


def _checked(argv):
    from m4depth_amd import main as MAIN
    parser = MAIN.build_parser()
    args = parser.parse_args(argv)
    MAIN.check_save_args(parser, args)
    return args


def test_driver_refusals(tmp_path, capsys):
    out = str(tmp_path / "out")
    base = ["--mode", "predict", "--save_dir", out]
    _refused(["--mode", "predict", "--save_map", "0.05"], capsys, "--save_map needs --save_dir")
    _refused(["--mode", "predict", "--map_min_frames", "2"], capsys, "--map_min_frames needs --save_map")
    _refused(base + ["--map_min_frames", "2"], capsys, "--map_min_frames needs --save_map")
    _refused(base + ["--save_cloud", "--map_slots_log2", "20"], capsys, "--map_slots_log2 needs --save_map")
    _refused(["--mode", "eval", "--save_dir", out, "--save_map", "0.05"], capsys, "--save_dir is a --mode=predict option")
    _refused(base + ["--save_map", "0.05", "--cloud_frame", "camera"], capsys, "--save_map needs --cloud_frame world")
    _refused(base + ["--save_map", "0.05", "--save_cloud", "--cloud_frame", "camera"], capsys, "--save_map needs --cloud_frame world")
    for bad in ("0", "-1", "nan", "inf"):
        _refused(base + ["--save_map", bad], capsys, "--save_map VOXEL needs a finite edge length > 0")
    _refused(base + ["--save_map", "0.05", "--map_min_frames", "0"], capsys, "--map_min_frames must be >= 1")
    for bad in ("15", "27"):
        _refused(base + ["--save_map", "0.05", "--map_slots_log2", bad], capsys, "--map_slots_log2 must be in 16..26")
    # what the clouds' options still refuse without either of the two
    _refused(base + ["--cloud_stride", "2"], capsys, "--cloud_stride needs --save_cloud")
    _refused(base + ["--cloud_views", "4"], capsys, "--cloud_views needs --save_cloud")
    _refused(base + ["--save_map", "0.05", "--cloud_min_views", "1"], capsys, "--cloud_min_views needs --cloud_views")
    _refused(base + ["--save_map", "0.05", "--cloud_stride", "0"], capsys, "--cloud_stride must be >= 1")
    assert not os.path.exists(out)


def test_driver_defaults_and_companions():
    a = _checked(["--mode", "predict", "--save_dir", "x", "--save_map", "0.05"])
    assert a.save_map == 0.05 and a.map_min_frames == 2 and a.map_slots_log2 == 21 and not a.save_cloud
    assert a.cloud_stride == 2 and a.cloud_frame == "world" and a.cloud_views == 0 and a.save_range == (1.0, 80.0)
    a = _checked(["--mode", "predict", "--save_dir", "x", "--save_map", "0.1", "--map_min_frames", "3", "--map_slots_log2", "16",
                  "--cloud_stride", "1", "--cloud_frame", "world", "--cloud_views", "4", "--cloud_min_views", "3", "--cloud_tol", "2",
                  "0.02", "--save_conf", "--save_range", "2", "40"])
    assert (a.save_map, a.map_min_frames, a.map_slots_log2, a.cloud_stride, a.cloud_views, a.cloud_min_views) == (0.1, 3, 16, 1, 4, 3)
    assert a.cloud_tol == (2.0, 0.02) and a.save_conf and a.save_range == (2.0, 40.0) and not a.save_cloud
    a = _checked(["--mode", "predict", "--save_dir", "x", "--save_cloud"])                 # without the option: nothing of it
    assert a.save_map is None and a.map_min_frames is None and a.map_slots_log2 is None
    from m4depth_amd import main as MAIN
    plain = vars(MAIN.build_parser().parse_args(["--mode", "predict"]))                    # absent from the namespace until given
    assert not {"save_map", "map_min_frames", "map_slots_log2"} & set(plain)


def test_writer_refusals(tmp_path):
    from m4depth_amd.export import PredictionWriter
    out = str(tmp_path)
    with pytest.raises(ValueError, match="save_map needs cloud_frame='world'"):
        PredictionWriter(out, "kitti16", save_map=0.05, cloud_frame="camera")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel edge"):
            PredictionWriter(out, "kitti16", save_map=bad)
    with pytest.raises(ValueError, match="map_min_frames"):
        PredictionWriter(out, "kitti16", save_map=0.05, map_min_frames=0)
    for bad in (5, 27):
        with pytest.raises(ValueError, match="map_slots_log2"):
            PredictionWriter(out, "kitti16", save_map=0.05, map_slots_log2=bad)
    with pytest.raises(ValueError, match="cloud_views needs cloud=True"):
        PredictionWriter(out, "kitti16", cloud_views=2)
    w = PredictionWriter(out, "kitti16", save_map=0.05, cloud_views=2)              # the filter serves the map alone too
    assert (w.cloud, w.save_map, w.map_min_frames, w.map_slots_log2) == (False, float(np.float32(0.05)), 2, 21)
    w.close()
    w = PredictionWriter(out, "kitti16")
    assert w.save_map is None and w.maps == 0
    w.close()
    w = PredictionWriter(out, "kitti16", save_map=None, map_min_frames=None, map_slots_log2=None)    # as the driver passes them
    assert w.save_map is None and (w.map_min_frames, w.map_slots_log2) == (2, 21)
    w.close()
    assert not os.listdir(out)


def test_map_file_round_trip(tmp_path):
    from m4depth_amd.export import write_map_ply, read_map_ply, read_cloud_ply
    rng = np.random.default_rng(3)
    m = VoxelMap(0.25)
    for stamp in (1, 2, 3):
        m.integrate(vertices_of(rng.uniform(-2, 2, (300, 3)), rng.integers(0, 256, (300, 3))), stamp)
    keys, vertices = m.extract(2)
    assert 10 < len(keys) < len(m.records)
    stats = dict(m.stats(), dropped_full=12345678901234)
    path = str(tmp_path / "map.ply")
    write_map_ply(path, vertices, np.float32(0.25), 2, stats)
    xyz, rgba, pose = read_cloud_ply(path)                                          # the per-frame clouds' reader reads it
    assert np.array_equal(np.concatenate([xyz.view(np.uint8).reshape(-1, 12), rgba], axis=1), vertices)
    assert np.array_equal(pose, [1, 0, 0, 0, 0, 0, 0])
    xyz2, rgba2, info = read_map_ply(path)
    assert np.array_equal(xyz2, xyz) and np.array_equal(rgba2, rgba)
    assert info == dict(stats, voxel=0.25, min_frames=2)
    with open(path, "rb") as fh:
        head = fh.read().split(b"end_header\n")[0].decode("ascii").splitlines()
    assert "comment pose 1 0 0 0 0 0 0" in head
    assert ("comment voxel_map voxel 0.25 min_frames 2 observations 900 dropped_range 0 dropped_full 12345678901234 occupied %d"
            % len(m.records)) in head
    write_map_ply(path, vertices[:0], np.float32(0.05), 1, m.stats())               # an empty map is a file too
    xyz, rgba, info = read_map_ply(path)
    assert xyz.shape == (0, 3) and rgba.shape == (0, 4) and np.float32(info["voxel"]) == np.float32(0.05) and info["min_frames"] == 1
    from m4depth_amd.export import write_cloud_ply
    write_cloud_ply(path, vertices, [1, 0, 0, 0, 0, 0, 0])
    with pytest.raises(ValueError, match="not a voxel map"):
        read_map_ply(path)


def test_entries_refuse_bad_arguments_without_a_launch():
    """Every refusal include/m4depth_hip.h lists, on host pointers that are never dereferenced; the size query."""
    from m4depth_amd._lib import lib
    assert lib.m4d_voxel_map_state_words(2, 12) == 2 * (4 + 10 * 4096)
    assert lib.m4d_voxel_map_state_words(1, 26) == 4 + 10 * (1 << 26)
    for b, L in ((0, 12), (65536, 12), (1, 5), (1, 27)):
        assert lib.m4d_voxel_map_state_words(b, L) == -1
    buf = (ctypes.c_ulonglong * 64)()
    p = ctypes.addressof(buf)
    assert p % 16 == 0 or (p + 8) % 16 == 0
    p += p % 16                                                                     # 16-byte aligned
    ok = dict(vertices=p, counts=p, b=1, cap=4, voxel=0.05, stamp=1, state=p, L=6)

    def integrate(**kw):
        a = dict(ok, **kw)
        return lib.m4d_voxel_map_integrate(a["vertices"], a["counts"], a["b"], a["cap"], a["voxel"], a["stamp"], a["state"], a["L"], None)

    for bad in (dict(vertices=None), dict(counts=None), dict(state=None), dict(b=0), dict(b=65536), dict(cap=0), dict(cap=(1 << 24) + 1),
                dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=float("nan")), dict(voxel=float("inf")), dict(stamp=0), dict(stamp=-3),
                dict(L=5), dict(L=27), dict(vertices=p + 8), dict(counts=p + 2), dict(state=p + 4)):
        assert integrate(**bad) == 1, bad

    def extract(**kw):
        a = dict(dict(state=p, b=2, L=6, s=1, min_frames=1, voxel=0.05, keys=p, out=p, out_cap=4, count=p), **kw)
        return lib.m4d_voxel_map_extract(a["state"], a["b"], a["L"], a["s"], a["min_frames"], a["voxel"], a["keys"], a["out"],
                                         a["out_cap"], a["count"], None)

    for bad in (dict(state=None), dict(keys=None), dict(out=None), dict(count=None), dict(b=0), dict(L=5), dict(L=27), dict(s=-1),
                dict(s=2), dict(min_frames=0), dict(voxel=0.0), dict(voxel=float("nan")), dict(voxel=float("inf")), dict(out_cap=0),
                dict(state=p + 4), dict(keys=p + 4), dict(count=p + 4), dict(out=p + 8)):
        assert extract(**bad) == 1, bad
    for state, b, L in ((None, 1, 6), (p, 0, 6), (p, 1, 5), (p, 1, 27), (p + 4, 1, 6)):
        assert lib.m4d_voxel_map_clear(state, None, b, L, None) == 1


def test_ops_refuse_bad_arguments():
    from m4depth_amd import network_ops as nops
    with pytest.raises(ValueError, match="slots_log2 in 6..26"):
        nops.voxel_map_state(1, 5, "cpu")
    with pytest.raises(ValueError, match="slots_log2 in 6..26"):
        nops.voxel_map_state(0, 12, "cpu")
    words = torch.zeros(4 + 10 * 64, dtype=torch.int64)
    state = {"words": words, "stats": words[:4].view(1, 4), "table": words[4:].view(1, 64, 10), "b": 1, "slots_log2": 6}
    v, c = torch.zeros((1, 8, 16), dtype=torch.uint8), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="voxel must be"):
        nops.voxel_map_integrate(v, c, 0.0, 1, state)
    with pytest.raises(ValueError, match="stamp must be >= 1"):
        nops.voxel_map_integrate(v, c, 0.05, 0, state)
    with pytest.raises(ValueError, match="expected vertices"):
        nops.voxel_map_integrate(v[0], c, 0.05, 1, state)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nops.voxel_map_integrate(v, c, 0.05, 1, state)
    with pytest.raises(ValueError, match="min_frames >= 1"):
        nops.voxel_map_extract(state, 0, 0, 0.05)
    with pytest.raises(ValueError, match="s in 0..0"):
        nops.voxel_map_extract(state, 1, 1, 0.05)
    with pytest.raises(ValueError, match="mask"):
        nops.voxel_map_clear(state, torch.zeros(2, dtype=torch.uint8))
    with pytest.raises(ValueError, match="not a voxel_map_state"):
        nops.voxel_map_clear(dict(state, slots_log2=7))


def test_header_states_the_contract():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "m4depth_hip.h")).read()
    for decl in ("int m4d_voxel_map_integrate(", "int m4d_voxel_map_extract(", "int m4d_voxel_map_clear(",
                 "long long m4d_voxel_map_state_words("):
        assert decl in txt, decl
    section = txt[txt.index("The map of a trajectory is the voxel-grid reduction"):txt.index("int m4d_voxel_map_integrate(")]
    for phrase in ("nothing is recomputed from depth", "agent-scope atomics only", "dropped_full", "3/4 of the slots", "ABI 6 unchanged"):
        assert phrase in section, phrase
    assert "#define M4D_ABI_VERSION 6 " in txt
    mk = open(os.path.join(root, "m4depth_amd", "csrc", "Makefile")).read()
    assert "m4d_voxelmap.hip" in mk.split("SRCS")[1].splitlines()[0]
