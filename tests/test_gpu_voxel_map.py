"""Voxel maps on the GPU (m4d_voxel_map_integrate / _extract / _clear, export.PredictionWriter(save_map=...), main.py --save_map)
against the numpy restatement tests/voxel_map_ref.py, bit for bit.

Every accumulator is an integer and the extraction is a fixed float64 expression rounded once, so there is no tolerance anywhere:
the device's records (read straight from the table, sorted by key) equal the restatement's dict, and the extracted vertices equal
its extraction byte for byte.  The state and the vertex buffers live inside sentinel-filled allocations with guard words on both
sides (as the arenas of test_gpu_degenerate.py): a store outside the state shows as a changed guard."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

from helpers import F, npy, cameras_np, make_fake_dataset
from voxel_map_ref import VoxelMap, vertices_of, EMPTY
import depth_views_ref as DV

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A
GUARD = 512                                                                     # 64-bit guard words on both sides


# ---- guarded buffers -------------------------------------------------------------------------------------------------------------
class Guarded:
    """A voxel_map_state whose words lie between guard words; ``check()`` holds the guards."""

    def __init__(self, b, L, dev):
        from m4depth_amd import network_ops as nops
        from m4depth_amd._lib import lib
        words = int(lib.m4d_voxel_map_state_words(b, L))
        self.flat = torch.full((GUARD + words + GUARD,), SENTINEL, dtype=torch.int64, device=dev)
        buf = self.flat[GUARD:GUARD + words]
        self.state = {"words": buf, "stats": buf[:4 * b].view(b, 4), "table": buf[4 * b:].view(b, 1 << L, 10), "b": b,
                      "slots_log2": L}
        nops.voxel_map_clear(self.state)

    def check(self):
        torch.cuda.synchronize()
        assert bool((self.flat[:GUARD] == SENTINEL).all()) and bool((self.flat[-GUARD:] == SENTINEL).all()), \
            "words outside the state overwritten"


def guarded_vertices(vertices, dev, cap=None):
    """[b] lists of [n,16] uint8 -> (vertices [b,cap,16] device view between guards, counts [b] int32, the flat buffer); the
    tail beyond a sample's count is filled with a NaN-coordinate pattern no map may ever see."""
    b = len(vertices)
    cap = cap or max(1, max(len(v) for v in vertices))
    flat = torch.full((GUARD * 8 + b * cap * 16 + GUARD * 8,), 0xFF, dtype=torch.uint8, device=dev)
    view = flat[GUARD * 8:GUARD * 8 + b * cap * 16].view(b, cap, 16)
    for s, v in enumerate(vertices):
        if len(v):
            view[s, :len(v)] = torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    counts = torch.tensor([len(v) for v in vertices], dtype=torch.int32, device=dev)
    return view, counts, flat


def records(state, s):
    """The occupied records of sample s straight from the table: key -> the nine other words, as Python integers."""
    table = npy(state["table"][s]).view(np.uint64)
    rows = table[table[:, 0] != np.uint64(EMPTY)]
    assert len(set(rows[:, 0].tolist())) == len(rows), "a key lives in two slots"
    return {int(r[0]): [int(v) for v in r[1:]] for r in rows}


def stats_of(state, s):
    return dict(zip(("observations", "dropped_range", "dropped_full", "occupied"), npy(state["stats"][s]).tolist()))


def assert_map_equals(state, s, ref, voxel, what):
    from m4depth_amd import network_ops as nops
    got = records(state, s)
    assert got == {k: list(v) for k, v in ref.records.items()}, what
    assert stats_of(state, s) == ref.stats(), what
    for min_frames in (1, 2):
        keys, vertices, stats = nops.voxel_map_extract(state, s, min_frames, voxel)
        want_keys, want = ref.extract(min_frames)
        assert np.array_equal(npy(keys).view(np.uint64), want_keys), (what, min_frames)
        assert np.array_equal(npy(vertices), want), (what, min_frames)
        assert stats == ref.stats(), what


# ---- 1: the kernels on clouds of m4d_depth_cloud ---------------------------------------------------------------------------------
B, H, W, FRAMES, VOXEL = 2, 20, 52, 3, 0.75


def _cloud_frames(dev):
    """Three frames of the tilted plane of depth_views_ref from a moving camera, per-sample cameras, a few pixels invalid or out
    of range: the compacted world-frame vertices as m4d_depth_cloud leaves them, [frame] of (vertices, counts) on the device."""
    from m4depth_amd import network_ops as nops
    cam = cameras_np(B, H, W)
    maps, poses = DV.scene(cam, n=FRAMES, h=H, w=W, scale=1.5)
    rng = np.random.default_rng(77)
    out = []
    for k in range(FRAMES):
        depth = maps[k].copy()
        holes = rng.random(depth.shape) < 0.1
        depth[holes] = rng.choice(np.array([np.nan, 0.5, 500.0, np.inf], F), int(holes.sum()))
        rgb = rng.random((B, H, W, 3)).astype(F)
        v, n = nops.depth_cloud(torch.from_numpy(depth[..., None]).to(dev), torch.from_numpy(rgb).to(dev),
                                torch.from_numpy(cam["f"]).to(dev), torch.from_numpy(cam["c"]).to(dev), step=1, near=1.0, far=80.0,
                                pose=torch.from_numpy(poses[k].copy()).to(dev))
        out.append((v, n))
    return out


@pytest.fixture(scope="module")
def cloud_frames(dev):
    frames = _cloud_frames(dev)
    torch.cuda.synchronize()
    host = [[npy(v[s, :int(n[s])]) for s in range(B)] for v, n in frames]
    refs = []
    for s in range(B):
        ref = VoxelMap(VOXEL)
        for k in range(FRAMES):
            ref.integrate(host[k][s], k + 1)
        refs.append(ref)
    return frames, host, refs


def test_maps_match_the_restatement_byte_for_byte(dev, cloud_frames):
    """Batch 2, 20 x 52 at stride 1 (1040 candidates: five workgroups, the last ragged), three frames, L = 12."""
    from m4depth_amd import network_ops as nops
    frames, host, refs = cloud_frames
    assert frames[0][0].shape == (B, 1040, 16)
    for s, ref in enumerate(refs):                                              # the scene is what the issue asks for
        recs = list(ref.records.values())
        assert 700 < len(host[0][s]) < 1040 and ref.dropped_range == 0
        assert np.mean([r[0] > 1 for r in recs]) > 0.5 and np.mean([r[8] > 1 for r in recs]) > 0.5, "most voxels: several pixels, frames"
        xyz = np.concatenate([h[s][:, :12].copy().view(F).reshape(-1, 3) for h in host])
        assert (xyz < 0).any(axis=0).sum() >= 2, "negative coordinates"
        assert 40 < len(recs) < 2000
    g = Guarded(B, 12, dev)
    for k, (v, n) in enumerate(frames):
        nops.voxel_map_integrate(v, n, VOXEL, k + 1, g.state)
    for s, ref in enumerate(refs):
        assert_map_equals(g.state, s, ref, VOXEL, f"sample {s}")
    g.check()


# ---- 2 + 3: a table of 64 slots --------------------------------------------------------------------------------------------------
def _box_vertices(seed, n, lo, hi):
    rng = np.random.default_rng(seed)
    return vertices_of(rng.uniform(lo, hi, (n, 3)).astype(F), rng.integers(0, 256, (n, 3)))


def _home(key, L):
    return ((key * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)) >> (64 - L)


def _occupied_slots(keys, L):
    """(The slots linear probing ends up occupying, the probe steps beyond the home slots summed over the keys): both are the
    same for every insertion order."""
    taken = set()
    steps = 0
    for k in keys:
        slot = _home(k, L)
        while slot in taken:
            slot = (slot + 1) % (1 << L)
            steps += 1
        taken.add(slot)
    return taken, steps


def test_long_probes_and_wrap_around(dev):
    """L = 6 and 40 distinct voxels (a 4 x 5 x 2 box, negative cells included): every one stored, byte for byte, nothing dropped.
    The slots they occupy are the ones linear probing must give for any order, and they wrap past the table's end."""
    from m4depth_amd import network_ops as nops
    voxel, L = 0.5, 6
    v = _box_vertices(11, 700, [-2.0, -1.5, 2.0], [0.0, 1.0, 3.0])
    ref = VoxelMap(voxel).integrate(v[:400], 1).integrate(v[400:], 2)
    assert 30 < len(ref.records) <= 40 and ref.dropped_range == 0                # checked on the CPU before the launch
    want_slots, want_steps = _occupied_slots(ref.records, L)
    assert want_steps >= 10, "no probing to speak of in this scene"
    homes = [_home(k, L) for k in ref.records]
    assert len(set(homes)) < len(homes), "no two keys share a home slot: nothing to probe"
    g = Guarded(1, L, dev)
    for stamp, part in ((1, v[:400]), (2, v[400:])):
        vd, nd, flat = guarded_vertices([part], dev, cap=450)
        nops.voxel_map_integrate(vd, nd, voxel, stamp, g.state)
    assert_map_equals(g.state, 0, ref, voxel, "64 slots")
    assert stats_of(g.state, 0)["dropped_full"] == 0
    table = npy(g.state["table"][0]).view(np.uint64)
    got_slots = set(np.nonzero(table[:, 0] != np.uint64(EMPTY))[0].tolist())
    assert got_slots == want_slots
    moved = [(slot - _home(int(table[slot, 0]), L)) % 64 for slot in got_slots]
    assert sum(moved) == want_steps
    assert any(slot < _home(int(table[slot, 0]), L) for slot in got_slots), "no probe wrapped past the end of the table"
    g.check()


def test_overflow_returns_and_keeps_its_books(dev):
    """L = 6 and some 500 voxels: the call returns, every vertex is accounted for, what is stored is a subset of the truth."""
    from m4depth_amd import network_ops as nops
    voxel, L = 0.5, 6
    v = _box_vertices(12, 3000, [-2.0, -2.0, 1.0], [2.0, 2.0, 5.0])
    v[5, :4] = np.array([np.nan], F).view(np.uint8)                             # and two the range drops
    v[77, 4:8] = np.array([3e38], F).view(np.uint8)
    ref = VoxelMap(voxel).integrate(v, 1)
    assert len(ref.records) > 48 and ref.dropped_range == 2
    g = Guarded(1, L, dev)
    vd, nd, _ = guarded_vertices([v], dev)
    nops.voxel_map_integrate(vd, nd, voxel, 1, g.state)
    g.check()
    got, st = records(g.state, 0), stats_of(g.state, 0)
    assert st["observations"] == 3000 and st["dropped_range"] == 2 and st["dropped_full"] > 0
    assert sum(r[0] for r in got.values()) + st["dropped_full"] + st["dropped_range"] == st["observations"]
    assert st["occupied"] == len(got) and 48 <= len(got) <= 64
    for key, rec in got.items():
        assert key in ref.records and 1 <= rec[0] <= ref.records[key][0], key
        assert all(a <= b for a, b in zip(rec[:7], ref.records[key][:7])) and rec[7:] == [1, 1]
    nops.voxel_map_integrate(vd, nd, voxel, 2, g.state)                          # a full table takes what it knows, no more
    again = records(g.state, 0)
    assert set(again) == set(got) and stats_of(g.state, 0)["observations"] == 6000
    st = stats_of(g.state, 0)
    assert sum(r[0] for r in again.values()) + st["dropped_full"] + st["dropped_range"] == 6000
    g.check()


# ---- 4: sample independence ------------------------------------------------------------------------------------------------------
def test_batch_launch_equals_per_sample_launches(dev, cloud_frames):
    from m4depth_amd import network_ops as nops
    _, host, refs = cloud_frames
    L = 12
    per_sample = [host[0][0], np.zeros((0, 16), np.uint8), host[0][1], host[1][0]]      # sample 1: counts = 0
    g = Guarded(4, L, dev)
    vd, nd, _ = guarded_vertices(per_sample, dev, cap=1040)
    nops.voxel_map_integrate(vd, nd, VOXEL, 1, g.state)
    g.check()
    fresh = npy(Guarded(1, L, dev).state["words"])
    for s, v in enumerate(per_sample):
        alone = Guarded(1, L, dev)
        v1, n1, _ = guarded_vertices([v], dev, cap=1040)
        nops.voxel_map_integrate(v1, n1, VOXEL, 1, alone.state)
        alone.check()
        assert records(g.state, s) == records(alone.state, 0) and stats_of(g.state, s) == stats_of(alone.state, 0), s
        assert records(g.state, s) == {k: list(r) for k, r in VoxelMap(VOXEL).integrate(v, 1).records.items()}, s
    assert np.array_equal(npy(g.state["table"][1]).reshape(-1), fresh[4:]) and not npy(g.state["stats"][1]).any(), \
        "a sample without vertices was touched"


# ---- 5: stamps -------------------------------------------------------------------------------------------------------------------
def test_stamps_count_frames_not_calls(dev, cloud_frames):
    from m4depth_amd import network_ops as nops
    frames, host, _ = cloud_frames
    v, n = frames[0]
    once, twice, two_stamps = (Guarded(B, 12, dev) for _ in range(3))
    nops.voxel_map_integrate(v, n, VOXEL, 5, once.state)
    for stamp, g in ((5, twice), (5, twice), (5, two_stamps), (6, two_stamps)):
        nops.voxel_map_integrate(v, n, VOXEL, stamp, g.state)
    for s in range(B):
        a, b2, c = records(once.state, s), records(twice.state, s), records(two_stamps.state, s)
        assert set(a) == set(b2) == set(c) and len(a) > 20
        for key, rec in a.items():
            assert b2[key] == [2 * x for x in rec[:7]] + [5, 1], key
            assert c[key] == [2 * x for x in rec[:7]] + [6, 2], key
            assert rec[7:] == [5, 1]
    for g in (once, twice, two_stamps):
        g.check()


# ---- 6: clear --------------------------------------------------------------------------------------------------------------------
def test_masked_clear_restores_the_fresh_state(dev, cloud_frames):
    from m4depth_amd import network_ops as nops
    _, host, _ = cloud_frames
    g = Guarded(3, 10, dev)
    fresh = npy(g.state["words"]).copy()
    assert (fresh[:12] == 0).all() and (fresh[12::10].view(np.uint64) == np.uint64(EMPTY)).all()
    assert not np.delete(fresh[12:].reshape(-1, 10), 0, axis=1).any()
    vd, nd, _ = guarded_vertices([host[0][0], host[1][1], host[2][0]], dev)
    nops.voxel_map_integrate(vd, nd, VOXEL, 1, g.state)
    full = npy(g.state["words"]).copy()
    tables = lambda w: w[12:].reshape(3, -1)
    assert all((tables(full)[s] != tables(fresh)[s]).any() and full[4 * s] > 0 for s in range(3))
    nops.voxel_map_clear(g.state, torch.tensor([1, 0, 1], dtype=torch.uint8, device=dev))
    got = npy(g.state["words"])
    for s in (0, 2):
        assert np.array_equal(tables(got)[s], tables(fresh)[s]) and not got[4 * s:4 * s + 4].any(), s
    assert np.array_equal(tables(got)[1], tables(full)[1]) and np.array_equal(got[4:8], full[4:8])
    nops.voxel_map_clear(g.state, torch.tensor([False, False, False], device=dev))
    assert np.array_equal(npy(g.state["words"]), got)
    nops.voxel_map_clear(g.state)
    assert np.array_equal(npy(g.state["words"]), fresh)
    g.check()


# ---- 7: the writer ---------------------------------------------------------------------------------------------------------------
def _map_of_clouds(directory, voxel, min_frames):
    """The restatement applied to the ``_cloud.ply`` files of one trajectory directory, frame k stamped k (any increasing
    stamps give the same map)."""
    from m4depth_amd.export import read_cloud_ply
    ref = VoxelMap(voxel)
    clouds = sorted(f for f in os.listdir(directory) if f.endswith("_cloud.ply"))
    for k, name in enumerate(clouds):
        xyz, rgba, _ = read_cloud_ply(os.path.join(directory, name))
        ref.integrate(np.concatenate([xyz.view(np.uint8).reshape(-1, 12), rgba], axis=1), k + 1)
    return ref, len(clouds)


def _check_map_files(out, voxel, min_frames, want_dirs):
    from m4depth_amd.export import read_map_ply
    dirs = sorted(os.listdir(out))
    assert dirs == sorted(want_dirs)
    sizes = {}
    for d in dirs:
        ref, n_clouds = _map_of_clouds(os.path.join(out, d), voxel, min_frames)
        assert n_clouds == want_dirs[d], d
        xyz, rgba, info = read_map_ply(os.path.join(out, d, "map.ply"))
        _, want = ref.extract(min_frames)
        assert np.array_equal(np.concatenate([xyz.view(np.uint8).reshape(-1, 12), rgba], axis=1), want), d
        assert info == dict(ref.stats(), voxel=float("%.9g" % np.float32(voxel)), min_frames=min_frames), d
        sizes[d] = len(want)
    return sizes


@pytest.mark.parametrize("views", [0, 2])
def test_prediction_writer_maps(dev, tmp_path, views):
    """Batch 2 on the rendered plane, seven steps through a ring of two slots; slot 1 starts a second trajectory at step 3.
    Every map.ply is the restatement of its trajectory's _cloud.ply files."""
    from m4depth_amd.export import PredictionWriter, FrameNamer
    b, h, w, steps, voxel = 2, 24, 40, 7, 1.0
    cam = {"f": np.tile(np.array([[20.0, 12.0]], F), (b, 1)), "c": np.tile(np.array([[20.3, 11.6]], F), (b, 1))}
    poses = np.zeros((steps, 7))
    poses[:, 0] = 1.0
    poses[:, 4:] = np.array([0.22, -0.12, 0.15])[None] * np.arange(steps)[:, None]       # translation only: rot is the identity
    camera = {k: torch.from_numpy(v).to(dev) for k, v in cam.items()}
    rng = np.random.default_rng(9)
    flags = [[k == 0, k in (0, 3)] for k in range(steps)]
    namer = FrameNamer(b)
    out = str(tmp_path / "out")
    with PredictionWriter(out, "kitti16", near=2.0, far=40.0, slots=2, cloud=True, cloud_step=1, cloud_views=views,
                          save_map=voxel, map_min_frames=2, map_slots_log2=12) as writer:
        for k in range(steps):
            depth = np.stack([DV.render_plane(poses[k], cam["f"][s], cam["c"][s], h, w) for s in range(b)])
            est = torch.from_numpy(depth[..., None]).to(dev)
            rgb = torch.from_numpy(rng.random((b, h, w, 3)).astype(F)).to(dev)
            rot = torch.tensor([[1.0, 0.0, 0.0, 0.0]] * b, device=dev)
            trans = torch.from_numpy(np.tile((poses[k, 4:] - poses[max(k - 1, 0), 4:]).astype(F), (b, 1))).to(dev)
            writer.submit(est, namer(flags[k]), rgb=rgb, rot=rot, trans=trans, camera=camera, reset=np.array(flags[k]))
        with pytest.raises(ValueError, match="host-side reset flags"):
            writer.submit(est, namer([False, False]), rgb=rgb, rot=rot, trans=trans, camera=camera,
                          reset=torch.zeros(b, dtype=torch.uint8, device=dev))
    sizes = _check_map_files(out, voxel, 2, {"s00_t0000": 7, "s01_t0000": 3, "s01_t0001": 4})
    assert writer.maps == 3 and writer.map_voxels == sum(sizes.values())
    assert writer.map_dropped_full == 0 and writer.map_dropped_range == 0
    assert sizes["s00_t0000"] > 100 and sizes["s01_t0001"] > 50
    if views:                                # three frames under the strict two-view rule: one cloud with vertices, no voxel seen twice
        assert sizes["s01_t0000"] == 0
    else:
        assert sizes["s01_t0000"] > 50


# ---- 8: the driver ---------------------------------------------------------------------------------------------------------------
N_TRAJ, N_FRAMES, SIZE = 2, 8, 64
_runs = {}


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("voxel_map"))
    db, rec = make_fake_dataset(root, "midair", n_traj=N_TRAJ, n_frames=N_FRAMES, size=(SIZE, SIZE))
    cfg = os.path.join(root, "datasets_location.json")
    with open(cfg, "w") as fh:
        json.dump({"midair": "./db"}, fh)
    return {"root": root, "rec": rec, "cfg": cfg}


def run_driver(dataset, key, extra):
    if key not in _runs:
        from m4depth_amd import main as MAIN
        out = os.path.join(dataset["root"], key)
        printed = io.StringIO()
        with contextlib.redirect_stdout(printed):
            assert MAIN.main(["--mode", "predict", "--dataset", "midair", "--db_path_config", dataset["cfg"], "--records_path",
                              dataset["rec"], "--arch_depth", "2", "--height", str(SIZE), "--width", str(SIZE), "--ckpt_dir",
                              out + "_ckpt"] + [a.replace("OUT", out) for a in extra]) == 0
        _runs[key] = (out, printed.getvalue())
    return _runs[key]


def map_run(dataset, key, extra):
    out, _ = run_driver(dataset, "plain", [])
    preds = np.load(out + "_ckpt/predictions.npy")
    near, far = (float(F(v)) for v in np.percentile(preds, [20, 80]))
    voxel = float(F((far - near) / 6.0))
    assert 0 < near < far and voxel > 0
    return run_driver(dataset, key, extra + ["--save_dir", "OUT", "--save_range", repr(near), repr(far), "--cloud_stride", "2",
                                             "--save_map", repr(voxel), "--map_slots_log2", "16"]) + (voxel,)


def test_driver_paths_write_identical_maps(dev, dataset):
    plain, printed, voxel = map_run(dataset, "frames", ["--save_cloud"])
    graphed, _, _ = map_run(dataset, "stream-graph", ["--save_cloud", "--stream", "--graph"])
    want_dirs = {f"s00_t{t:04d}": N_FRAMES for t in range(N_TRAJ)}
    sizes = _check_map_files(plain, voxel, 2, want_dirs)
    assert all(n > 20 for n in sizes.values()), sizes
    for d in want_dirs:
        files = sorted(os.listdir(os.path.join(plain, d)))
        assert files == sorted(os.listdir(os.path.join(graphed, d))) and len(files) == 2 * N_FRAMES + 1
        for name in files:
            with open(os.path.join(plain, d, name), "rb") as a, open(os.path.join(graphed, d, name), "rb") as b2:
                assert a.read() == b2.read(), (d, name)
    (line,) = [l for l in printed.splitlines() if l.startswith("predict: wrote")]
    assert (f"{N_TRAJ} voxel maps at {voxel:g} m: {sum(sizes.values())} voxels written, 0 vertices dropped out of range, "
            "0 dropped by full tables") in line


def test_driver_map_alone_writes_no_clouds(dev, dataset):
    with_clouds, _, voxel = map_run(dataset, "frames", ["--save_cloud"])
    alone, _, _ = map_run(dataset, "alone", [])
    for d in sorted(os.listdir(with_clouds)):
        files = sorted(os.listdir(os.path.join(alone, d)))
        assert files == sorted([f"{k:06d}_depth.png" for k in range(N_FRAMES)] + ["map.ply"]), files
        with open(os.path.join(with_clouds, d, "map.ply"), "rb") as a, open(os.path.join(alone, d, "map.ply"), "rb") as b2:
            assert a.read() == b2.read(), d
