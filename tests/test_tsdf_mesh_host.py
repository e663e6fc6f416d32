"""Host side of the TSDF meshes (main.py --save_mesh): the option refusals, the writer's refusals, the mesh file's round trip and
the C entries' argument checks -- nothing here launches a kernel."""
import ctypes
import os

import numpy as np
import pytest
import torch

import tsdf_mesh_ref as T

MESH_OPTIONS = {"save_mesh", "mesh_trunc", "mesh_min_frames", "mesh_slots_log2"}


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
    _refused(["--mode", "predict", "--save_mesh", "0.05"], capsys, "--save_mesh needs --save_dir")
    for opt in ("--mesh_trunc", "--mesh_min_frames", "--mesh_slots_log2"):
        _refused(["--mode", "predict", opt, "20"], capsys, opt + " needs --save_mesh")
        _refused(base + ["--save_cloud", "--save_map", "0.05", opt, "20"], capsys, opt + " needs --save_mesh")
    _refused(["--mode", "eval", "--save_dir", out, "--save_mesh", "0.05"], capsys, "--save_dir is a --mode=predict option")
    _refused(base + ["--save_mesh", "0.05", "--cloud_frame", "camera"], capsys, "--save_mesh needs --cloud_frame world")
    _refused(base + ["--save_mesh", "0.05", "--save_cloud", "--cloud_frame", "camera"], capsys, "--save_mesh needs --cloud_frame world")
    for bad in ("0", "-1", "nan", "inf"):
        _refused(base + ["--save_mesh", bad], capsys, "--save_mesh VOXEL needs a finite edge length > 0")
    for bad in ("1", "9"):
        _refused(base + ["--save_mesh", "0.05", "--mesh_trunc", bad], capsys, "--mesh_trunc must be in 2..8")
    _refused(base + ["--save_mesh", "0.05", "--mesh_min_frames", "0"], capsys, "--mesh_min_frames must be >= 1")
    for bad in ("15", "27"):
        _refused(base + ["--save_mesh", "0.05", "--mesh_slots_log2", bad], capsys, "--mesh_slots_log2 must be in 16..26")
    _refused(base + ["--cloud_views", "4"], capsys, "--cloud_views needs --save_cloud")           # still refused without a consumer
    _refused(base + ["--save_mesh", "0.05", "--cloud_min_views", "1"], capsys, "--cloud_min_views needs --cloud_views")
    assert not os.path.exists(out)


def test_several_ranks_are_refused(tmp_path, monkeypatch):
    """Like every --save_dir run (the refusal comes before anything touches a GPU)."""
    from m4depth_amd import main as MAIN
    from m4depth_amd import dist as D
    monkeypatch.setattr(D, "init_from_env", lambda: (0, 2, 0, torch.device("cpu")))
    with pytest.raises(SystemExit, match="run it on one rank"):
        MAIN.main(["--mode", "predict", "--save_dir", str(tmp_path / "out"), "--save_mesh", "0.05"])


def test_driver_defaults_and_companions():
    a = _checked(["--mode", "predict", "--save_dir", "x", "--save_mesh", "0.05"])
    assert (a.save_mesh, a.mesh_trunc, a.mesh_min_frames, a.mesh_slots_log2) == (0.05, 4, 2, 22)
    assert not a.save_cloud and a.save_map is None and a.cloud_frame == "world" and a.cloud_views == 0 and a.save_range == (1.0, 80.0)
    a = _checked(["--mode", "predict", "--save_dir", "x", "--save_mesh", "0.1", "--mesh_trunc", "2", "--mesh_min_frames", "3",
                  "--mesh_slots_log2", "16", "--cloud_views", "4", "--cloud_min_views", "3", "--save_range", "2", "40"])
    assert (a.save_mesh, a.mesh_trunc, a.mesh_min_frames, a.mesh_slots_log2, a.cloud_views, a.cloud_min_views) == (0.1, 2, 3, 16, 4, 3)
    assert a.save_range == (2.0, 40.0) and not a.save_cloud and a.save_map is None                # the views check serves the mesh alone
    a = _checked(["--mode", "predict", "--save_dir", "x", "--save_mesh", "0.1", "--mesh_trunc", "8", "--save_cloud", "--save_map", "0.2"])
    assert (a.save_mesh, a.mesh_trunc, a.save_map, a.save_cloud) == (0.1, 8, 0.2, True)
    a = _checked(["--mode", "predict", "--save_dir", "x", "--save_cloud"])                        # without the option: nothing of it
    assert all(getattr(a, f) is None for f in MESH_OPTIONS)
    from m4depth_amd import main as MAIN
    plain = vars(MAIN.build_parser().parse_args(["--mode", "predict"]))                           # absent from the namespace until given
    assert not MESH_OPTIONS & set(plain)


def test_writer_refusals(tmp_path):
    from m4depth_amd.export import PredictionWriter
    out = str(tmp_path)
    with pytest.raises(ValueError, match="save_mesh needs cloud_frame='world'"):
        PredictionWriter(out, "kitti16", save_mesh=0.05, cloud_frame="camera")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="save_mesh: the voxel edge"):
            PredictionWriter(out, "kitti16", save_mesh=bad)
    for bad in (dict(mesh_trunc=1), dict(mesh_trunc=9), dict(mesh_min_frames=0), dict(mesh_slots_log2=5), dict(mesh_slots_log2=27)):
        with pytest.raises(ValueError, match="mesh_trunc in 2..8, mesh_min_frames >= 1 and mesh_slots_log2 in 6..26"):
            PredictionWriter(out, "kitti16", save_mesh=0.05, **bad)
    with pytest.raises(ValueError, match="cloud_views needs cloud=True: the check runs on the clouds' pose chain"):
        PredictionWriter(out, "kitti16", cloud_views=2)
    w = PredictionWriter(out, "kitti16", save_mesh=0.05, cloud_views=2)                 # the filter serves the mesh alone too
    assert (w.cloud, w.save_map, w.save_mesh, w.mesh_trunc, w.mesh_min_frames, w.mesh_slots_log2) == \
        (False, None, float(np.float32(0.05)), 4, 2, 22)
    w.close()
    w = PredictionWriter(out, "kitti16")
    assert w.save_mesh is None and w.meshes == 0 and w.mesh_vertices == 0 and w.mesh_triangles == 0
    w.close()
    w = PredictionWriter(out, "kitti16", save_mesh=None, mesh_trunc=None, mesh_min_frames=None, mesh_slots_log2=None)
    assert w.save_mesh is None and (w.mesh_trunc, w.mesh_min_frames, w.mesh_slots_log2) == (4, 2, 22)       # as the driver passes them
    w.close()
    assert not os.listdir(out)


def test_mesh_file_round_trip(tmp_path):
    from m4depth_amd.export import write_mesh_ply, read_mesh_ply, read_cloud_ply, write_cloud_ply, PLY_FACE
    P = T.PLANE
    vol = T.fuse(T.plane_frames(), T.PLANE_F, T.PLANE_C, P["voxel"], P["trunc"], P["near"], P["far"])
    m = vol.extract(2)
    assert len(m["keys"]) > 100 and len(m["triangles"]) > 200
    stats = dict(vol.stats(), dropped_full=12345678901234, quads_dropped=m["quads_dropped"])
    path = str(tmp_path / "mesh.ply")
    write_mesh_ply(path, m["vertices"], m["triangles"], np.float32(P["voxel"]), P["trunc"], 2, stats)
    xyz, rgba, tri, info = read_mesh_ply(path)
    assert np.array_equal(np.concatenate([xyz.view(np.uint8).reshape(-1, 12), rgba], axis=1), m["vertices"])
    assert tri.dtype == np.int32 and np.array_equal(tri, m["triangles"])
    assert info == dict(stats, voxel=0.25, trunc=3, min_frames=2)
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    head = head.decode("ascii").splitlines()
    assert head[:3] == ["ply", "format binary_little_endian 1.0", "comment pose 1 0 0 0 0 0 0"]
    assert head[3] == ("comment tsdf_mesh voxel 0.25 trunc 3 min_frames 2 occupied %d dropped_range 0 dropped_full 12345678901234 "
                       "updates %d quads_dropped %d" % (len(vol.records), vol.updates, m["quads_dropped"]))
    assert head[4] == "element vertex %d" % len(xyz) and head[-2:] == ["element face %d" % len(tri),
                                                                       "property list uchar int vertex_indices"]
    assert PLY_FACE.itemsize == 13 and len(body) == 16 * len(xyz) + 13 * len(tri)
    assert body[16 * len(xyz)] == 3 and body[16 * len(xyz) + 1:16 * len(xyz) + 13] == m["triangles"][0].astype("<i4").tobytes()
    with pytest.raises(ValueError, match="not a point cloud"):                       # a mesh is no cloud: the cloud reader says so
        read_cloud_ply(path)
    write_mesh_ply(path, m["vertices"][:0], m["triangles"][:0], np.float32(0.05), 4, 1, dict(vol.stats(), quads_dropped=0))
    xyz, rgba, tri, info = read_mesh_ply(path)                                       # an empty mesh is a file too
    assert xyz.shape == (0, 3) and rgba.shape == (0, 4) and tri.shape == (0, 3) and np.float32(info["voxel"]) == np.float32(0.05)
    assert (info["trunc"], info["min_frames"]) == (4, 1)
    with pytest.raises(ValueError, match="names a vertex outside"):
        write_mesh_ply(path, m["vertices"][:3], np.array([[0, 1, 3]], np.int32), 0.05, 4, 1, dict(vol.stats(), quads_dropped=0))
    write_cloud_ply(path, m["vertices"], [1, 0, 0, 0, 0, 0, 0])
    with pytest.raises(ValueError, match="not a TSDF mesh"):
        read_mesh_ply(path)


def test_host_ordering_of_shuffled_records():
    """network_ops.tsdf_order on the restatement's records in a shuffled order (pure torch: it runs on the CPU too)."""
    from m4depth_amd import network_ops as nops
    P = T.PLANE
    m = T.fuse(T.plane_frames(), T.PLANE_F, T.PLANE_C, P["voxel"], P["trunc"], P["near"], P["far"]).extract(2)
    rng = np.random.default_rng(1)
    pv, pq = rng.permutation(len(m["keys"])), rng.permutation(len(m["raw_quads"]))
    keys, vertices, triangles, dropped = nops.tsdf_order(torch.from_numpy(m["keys"][pv].view(np.int64)),
                                                         torch.from_numpy(m["vertices"][pv]),
                                                         torch.from_numpy(m["raw_quads"][pq].view(np.int64)))
    assert np.array_equal(keys.numpy().view(np.uint64), m["keys"]) and np.array_equal(vertices.numpy(), m["vertices"])
    assert triangles.dtype == torch.int32 and np.array_equal(triangles.numpy(), m["triangles"])
    assert dropped == m["quads_dropped"] > 0
    none = nops.tsdf_order(torch.zeros(0, dtype=torch.int64), torch.zeros((0, 16), dtype=torch.uint8),
                           torch.from_numpy(m["raw_quads"][:5].view(np.int64)))
    assert none[2].shape == (0, 3) and none[3] == 5


def test_entries_refuse_bad_arguments_without_a_launch():
    """Every refusal include/m4depth_hip.h lists, on host pointers that are never dereferenced; the size query."""
    from m4depth_amd._lib import lib
    assert lib.m4d_tsdf_state_words(2, 12) == 2 * (4 + 4 * 4096)
    assert lib.m4d_tsdf_state_words(1, 26) == 4 + 4 * (1 << 26) and 8 * (4 * (1 << 22)) == 32 << 22
    for b, L in ((0, 12), (65536, 12), (1, 5), (1, 27)):
        assert lib.m4d_tsdf_state_words(b, L) == -1
    buf = (ctypes.c_ulonglong * 64)()
    p = ctypes.addressof(buf)
    p += p % 16                                                                     # 16-byte aligned
    ok = dict(depth=p, ds=12, rgb=p, rs=36, f=p, c=p, pose=p, b=1, h=3, w=4, near=1.0, far=80.0, voxel=0.05, trunc=4, state=p, L=6)
    frame_bad = (dict(depth=None), dict(f=None), dict(c=None), dict(pose=None), dict(state=None), dict(b=0), dict(b=65536),
                 dict(h=0), dict(w=0), dict(h=4097, w=4097, ds=1 << 25, rs=1 << 27), dict(far=1.0), dict(far=float("nan")),
                 dict(near=float("nan")), dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=float("nan")), dict(voxel=float("inf")),
                 dict(trunc=1), dict(trunc=9), dict(ds=11), dict(L=5), dict(L=27), dict(depth=p + 2), dict(f=p + 2), dict(c=p + 2),
                 dict(pose=p + 4), dict(state=p + 4))

    def allocate(**kw):
        a = dict(ok, **kw)
        return lib.m4d_tsdf_allocate(a["depth"], a["ds"], a["f"], a["c"], a["pose"], a["b"], a["h"], a["w"], a["near"], a["far"],
                                     a["voxel"], a["trunc"], a["state"], a["L"], None)

    def integrate(**kw):
        a = dict(ok, **kw)
        return lib.m4d_tsdf_integrate(a["depth"], a["ds"], a["rgb"], a["rs"], a["f"], a["c"], a["pose"], a["b"], a["h"], a["w"],
                                      a["near"], a["far"], a["voxel"], a["trunc"], a["state"], a["L"], None)

    for bad in frame_bad:
        assert allocate(**bad) == 1, bad
        assert integrate(**bad) == 1, bad
    for bad in (dict(rgb=None), dict(rs=35), dict(rgb=p + 2)):
        assert integrate(**bad) == 1, bad

    def vertices(**kw):
        a = dict(dict(state=p, b=2, L=6, s=1, min_frames=1, voxel=0.05, keys=p, out=p, out_cap=4, count=p), **kw)
        return lib.m4d_tsdf_extract_vertices(a["state"], a["b"], a["L"], a["s"], a["min_frames"], a["voxel"], a["keys"], a["out"],
                                             a["out_cap"], a["count"], None)

    for bad in (dict(state=None), dict(keys=None), dict(out=None), dict(count=None), dict(b=0), dict(L=5), dict(L=27), dict(s=-1),
                dict(s=2), dict(min_frames=0), dict(voxel=0.0), dict(voxel=float("nan")), dict(voxel=float("inf")), dict(out_cap=0),
                dict(state=p + 4), dict(keys=p + 4), dict(count=p + 4), dict(out=p + 8)):
        assert vertices(**bad) == 1, bad

    def faces(**kw):
        a = dict(dict(state=p, b=2, L=6, s=1, min_frames=1, quads=p, out_cap=4, count=p), **kw)
        return lib.m4d_tsdf_extract_faces(a["state"], a["b"], a["L"], a["s"], a["min_frames"], a["quads"], a["out_cap"], a["count"], None)

    for bad in (dict(state=None), dict(quads=None), dict(count=None), dict(b=0), dict(L=5), dict(L=27), dict(s=-1), dict(s=2),
                dict(min_frames=0), dict(out_cap=0), dict(state=p + 4), dict(quads=p + 4), dict(count=p + 4)):
        assert faces(**bad) == 1, bad
    for state, b, L in ((None, 1, 6), (p, 0, 6), (p, 1, 5), (p, 1, 27), (p + 4, 1, 6)):
        assert lib.m4d_tsdf_clear(state, None, b, L, None) == 1


def test_ops_refuse_bad_arguments():
    from m4depth_amd import network_ops as nops
    with pytest.raises(ValueError, match="slots_log2 in 6..26"):
        nops.tsdf_state(1, 5, "cpu")
    with pytest.raises(ValueError, match="slots_log2 in 6..26"):
        nops.tsdf_state(0, 12, "cpu")
    state = nops.tsdf_state_views(torch.zeros(4 + 4 * 64, dtype=torch.int64), 1, 6)
    assert state["stats"].shape == (1, 4) and state["keys"].shape == (1, 64) and state["recs"].shape == (1, 64, 6)
    assert state["recs"].dtype == torch.int32 and state["recs"].data_ptr() == state["words"].data_ptr() + 8 * (4 + 64)
    depth, rgb = torch.zeros((1, 3, 4, 1)), torch.zeros((1, 3, 4, 3))
    cam, pose = torch.ones((1, 2)), torch.zeros((1, 7), dtype=torch.float64)
    with pytest.raises(ValueError, match="voxel must be"):
        nops.tsdf_integrate(depth, rgb, cam, cam, pose, 0.0, 4, state)
    for bad in (1, 9):
        with pytest.raises(ValueError, match="trunc must be in 2..8"):
            nops.tsdf_integrate(depth, rgb, cam, cam, pose, 0.05, bad, state)
    with pytest.raises(ValueError, match="depth: expected"):
        nops.tsdf_integrate(depth[..., 0], rgb, cam, cam, pose, 0.05, 4, state)
    with pytest.raises(ValueError, match="rgb .* does not belong"):
        nops.tsdf_integrate(depth, rgb[:, :2], cam, cam, pose, 0.05, 4, state)
    with pytest.raises(ValueError, match="near < far"):
        nops.tsdf_integrate(depth, rgb, cam, cam, pose, 0.05, 4, state, near=2.0, far=2.0)
    with pytest.raises(ValueError, match="pose: expected"):
        nops.tsdf_integrate(depth, rgb, cam, cam, pose.float(), 0.05, 4, state)
    with pytest.raises(TypeError, match="float32 device tensor"):
        nops.tsdf_integrate(depth, rgb, cam, cam, pose, 0.05, 4, state)
    with pytest.raises(ValueError, match="min_frames >= 1"):
        nops.tsdf_extract_raw(state, 0, 0, 0.05, 4, 12)
    with pytest.raises(ValueError, match="s in 0..0"):
        nops.tsdf_extract(state, 1, 1, 0.05)
    with pytest.raises(ValueError, match="mask"):
        nops.tsdf_clear(state, torch.zeros(2, dtype=torch.uint8))
    with pytest.raises(ValueError, match="not a tsdf_state"):
        nops.tsdf_clear(dict(state, slots_log2=7))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nops.tsdf_clear(state)


def test_header_states_the_contract_and_the_library_exports_it():
    from m4depth_amd._lib import lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "m4depth_hip.h")).read()
    for decl in ("int m4d_tsdf_allocate(", "int m4d_tsdf_integrate(", "int m4d_tsdf_extract_vertices(", "int m4d_tsdf_extract_faces(",
                 "int m4d_tsdf_clear(", "long long m4d_tsdf_state_words("):
        assert decl in txt, decl
        name = decl.split()[-1][:-1]
        assert callable(getattr(lib, name)) and getattr(lib, name).argtypes, name        # exported, signature from the header
    section = txt[txt.index("Truncated-signed-distance fusion"):txt.index("int m4d_tsdf_allocate(")]
    for phrase in ("structure of arrays", "3/4 of the slots", "at most 128 trips", "touched by its owner only", "t = D_a / (D_a - D_b)",
                   "the owner key", "dropped_full", "ABI 6 unchanged"):
        assert phrase in section, phrase
    assert "#define M4D_ABI_VERSION 6 " in txt
    mk = open(os.path.join(root, "m4depth_amd", "csrc", "Makefile")).read()
    assert "m4d_tsdf.hip" in mk.split("SRCS")[1].splitlines()[0]
    src = open(os.path.join(root, "m4depth_amd", "csrc", "m4d_tsdf.hip")).read()
    assert "getenv" not in src and "hipMemset" not in src
