"""TSDF meshes on the GPU (m4d_tsdf_allocate / _integrate / _extract_vertices / _extract_faces / _clear,
export.PredictionWriter(save_mesh=...), main.py --save_mesh) against the numpy restatement tests/tsdf_mesh_ref.py, bit for bit.

The key set does not depend on the schedule, a record has one owner, and the extraction is a fixed sequence of float32 / float64
operations rounded once each, so there is no tolerance anywhere: the device's records (read straight from the state, keyed by the
packed key) equal the restatement's dict, and the extracted vertices and triangles equal its extraction byte for byte.  Every raw
buffer a kernel reads or writes lies inside a sentinel-filled allocation with guards on both sides: a store outside shows as a
changed guard."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

from helpers import F, npy, cameras_np, make_fake_dataset
import tsdf_mesh_ref as T
import depth_views_ref as DV

pytestmark = pytest.mark.gpu

GUARD = 4096                                                                    # guard bytes on both sides
SENTINEL = 0x5A


# ---- guarded buffers -------------------------------------------------------------------------------------------------------------
class Guarded:
    """A device tensor of ``shape`` / ``dtype`` between guard bytes, filled from ``array`` (or with the sentinel);
    ``check()`` holds the guards."""

    def __init__(self, dev, shape, dtype, array=None):
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        self.flat = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
        self.t = self.flat[GUARD:GUARD + n].view(dtype).view(*shape)
        if array is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(array)).view(dtype).view(*shape))

    def check(self):
        torch.cuda.synchronize()
        assert bool((self.flat[:GUARD] == SENTINEL).all()) and bool((self.flat[-GUARD:] == SENTINEL).all()), \
            "bytes outside a buffer overwritten"


class GuardedState(Guarded):
    """A tsdf_state whose words lie between guards, cleared."""

    def __init__(self, b, L, dev):
        from m4depth_amd import network_ops as nops
        from m4depth_amd._lib import lib
        super().__init__(dev, (int(lib.m4d_tsdf_state_words(b, L)),), torch.int64)
        self.state = nops.tsdf_clear(nops.tsdf_state_views(self.t, b, L))


class Frame:
    """The inputs of one tsdf_integrate call, each between guards."""

    def __init__(self, dev, depth, rgb, cam, poses):
        b, h, w = depth.shape
        self.bufs = [Guarded(dev, (b, h, w, 1), torch.float32, depth.astype(F)),
                     Guarded(dev, (b, h, w, 3), torch.float32, rgb.astype(F)),
                     Guarded(dev, (b, 2), torch.float32, cam["f"].astype(F)), Guarded(dev, (b, 2), torch.float32, cam["c"].astype(F)),
                     Guarded(dev, (b, 7), torch.float64, np.asarray(poses, np.float64))]

    def into(self, g, voxel, trunc, near, far):
        from m4depth_amd import network_ops as nops
        depth, rgb, f, c, pose = (x.t for x in self.bufs)
        nops.tsdf_integrate(depth, rgb, f, c, pose, voxel, trunc, g.state, near=near, far=far)

    def check(self):
        for x in self.bufs:
            x.check()


def records(state, s):
    """The occupied records of sample s straight from the state: key -> [bits of S, n, sr, sg, sb, nc]."""
    keys = npy(state["keys"][s]).view(np.uint64)
    recs = npy(state["recs"][s]).view(np.uint32)
    used = keys != np.uint64(T.EMPTY)
    assert len(set(keys[used].tolist())) == int(used.sum()), "a key lives in two slots"
    assert not recs[~used].any(), "a record without a key"
    return {int(k): [int(v) for v in r] for k, r in zip(keys[used], recs[used])}


def ref_records(vol):
    return {k: [np.float32(r[0]).view(np.uint32).item()] + r[1:] for k, r in vol.records.items()}


def stats_of(state, s):
    return dict(zip(("occupied", "dropped_range", "dropped_full", "updates"), npy(state["stats"][s]).tolist()))


def extract_guarded(g, s, min_frames, voxel, vertex_cap=None, quad_cap=None):
    """The two extraction launches into guarded buffers, then the host's ordering: (keys uint64, vertices [n,16] uint8, triangles
    int32, quads dropped, raw counts)."""
    from m4depth_amd import network_ops as nops
    dev = g.state["words"].device
    occupied = stats_of(g.state, s)["occupied"]
    vcap = max(occupied if vertex_cap is None else vertex_cap, 1)
    qcap = max(3 * occupied if quad_cap is None else quad_cap, 1)
    out = [Guarded(dev, (vcap,), torch.int64), Guarded(dev, (vcap, 16), torch.uint8), Guarded(dev, (qcap, 5), torch.int64),
           Guarded(dev, (2,), torch.int64, np.zeros(2, np.int64))]
    nops.tsdf_extract_raw(g.state, s, min_frames, voxel, vcap, qcap, out=tuple(x.t for x in out))
    for x in out:
        x.check()
    g.check()
    n_v, n_q = npy(out[3].t).tolist()
    keys, vertices, tri, dropped = nops.tsdf_order(out[0].t[:min(n_v, vcap)], out[1].t[:min(n_v, vcap)], out[2].t[:min(n_q, qcap)])
    return npy(keys).view(np.uint64), npy(vertices), npy(tri), dropped, (n_v, n_q)


def assert_mesh_equals(g, s, vol, voxel, what, min_frames=(1, 2)):
    from m4depth_amd import network_ops as nops
    for m in min_frames:
        want = vol.extract(m)
        keys, vertices, tri, dropped, counts = extract_guarded(g, s, m, voxel)
        assert counts == (len(want["keys"]), len(want["raw_quads"])), (what, m)
        assert np.array_equal(keys, want["keys"]), (what, m)
        assert np.array_equal(vertices, want["vertices"]), (what, m)
        assert np.array_equal(tri, want["triangles"]) and dropped == want["quads_dropped"], (what, m)
        k2, v2, t2, stats = nops.tsdf_extract(g.state, s, m, voxel)                # the wrapper the writer calls: the same mesh
        assert np.array_equal(npy(k2).view(np.uint64), keys) and np.array_equal(npy(v2), vertices) and np.array_equal(npy(t2), tri)
        assert stats == dict(vol.stats(), quads_dropped=dropped), (what, m)
    return want


# ---- 1 + 2: the plane, batch 2 ---------------------------------------------------------------------------------------------------
B, H, W, L = 2, T.PLANE["h"], T.PLANE["w"], 12
VOXEL, TRUNC, NEAR, FAR = T.PLANE["voxel"], T.PLANE["trunc"], 1.0, 3.25         # far cuts the wide camera's rim: the table fits


def _plane_inputs():
    """Five frames for two samples with their own cameras: the four plane poses and a fifth frame with a NaN hole and a depth
    step; sample 1 sees the poses in another order.  [frame] of (depth [B,H,W], rgb [B,H,W,3], poses [B,7])."""
    cam = cameras_np(B, H, W)
    poses = T.plane_poses(5)
    rng = np.random.default_rng(21)
    frames = []
    for k in range(5):
        ps = [poses[k], poses[(k + 2) % 5]]
        depth = np.stack([T.render_plane(ps[s], cam["f"][s], cam["c"][s], H, W, T.PLANE_NORMAL, T.PLANE_OFFSET) for s in range(B)])
        if k == 4:
            depth[:, 5:9, 7:12] = np.nan
            depth[:, 12:, 20:] -= F(1.0)
        frames.append((depth, rng.random((B, H, W, 3)).astype(F), np.stack(ps)))
    return cam, frames


@pytest.fixture(scope="module")
def plane(dev):
    """The device state after every frame (host copies of records and statistics), the final guarded state, and the restatement's
    volumes after every frame."""
    import copy
    cam, frames = _plane_inputs()
    vols = [T.TsdfVolume(VOXEL, TRUNC, NEAR, FAR) for _ in range(B)]
    g = GuardedState(B, L, dev)
    got, want = [], []
    for depth, rgb, poses in frames:
        fr = Frame(dev, depth, rgb, cam, poses)
        fr.into(g, VOXEL, TRUNC, NEAR, FAR)
        fr.check()
        g.check()
        got.append([(records(g.state, s), stats_of(g.state, s)) for s in range(B)])
        for s in range(B):
            vols[s].frame(depth[s], rgb[s], cam["f"][s], cam["c"][s], poses[s])
        want.append([(ref_records(vols[s]), copy.deepcopy(vols[s].stats())) for s in range(B)])
    return {"cam": cam, "frames": frames, "g": g, "got": got, "want": want, "vols": vols}


def test_state_after_every_frame_equals_the_restatement(plane):
    """24 x 32 pixels (three workgroups of allocate), 4096 slots (sixteen of integrate), batch 2, five frames."""
    mark = (1 << L) - (1 << (L - 2))
    for vol in plane["vols"]:                                                    # checked for the inputs as they are
        assert 500 < len(vol.records) < mark and vol.dropped_range == 0 and vol.updates > 2000
        n = np.array([r[1] for r in vol.records.values()])
        nc = np.array([r[5] for r in vol.records.values()])
        assert (n > 1).mean() > 0.3 and (n == 0).any() and (nc < n).any(), "several frames per voxel, unseen voxels, free space"
    for k, (got, want) in enumerate(zip(plane["got"], plane["want"])):
        for s in range(B):
            assert set(got[s][0]) == set(want[s][0]), (k, s, "key set")
            assert got[s][0] == want[s][0], (k, s, "records")
            assert got[s][1] == want[s][1], (k, s, "statistics")


def test_plane_extraction_equals_the_restatement(plane):
    for s, vol in enumerate(plane["vols"]):
        want = assert_mesh_equals(plane["g"], s, vol, VOXEL, f"sample {s}")
        assert len(want["keys"]) > 50 and len(want["triangles"]) > 80
    # a capacity too small: counted, not written, the guards intact
    keys, _, _, _, counts = extract_guarded(plane["g"], 0, 1, VOXEL, vertex_cap=10, quad_cap=7)
    want = plane["vols"][0].extract(1)
    assert counts == (len(want["keys"]), len(want["raw_quads"])) and len(keys) == 10 and set(keys.tolist()) <= set(want["keys"].tolist())


def test_sphere_extraction_is_closed_and_equals_the_restatement(dev):
    """26 frames of the unit sphere, L = 13: 3944 voxels against the 6144-slot mark."""
    S = T.SPHERE
    frames = T.sphere_frames()
    vol = T.fuse(frames, S["f"], S["c"], S["voxel"], S["trunc"], S["near"], S["far"])
    assert len(vol.records) == 3944 < (1 << 13) - (1 << 11)
    cam = {"f": np.array([S["f"]], F), "c": np.array([S["c"]], F)}
    g = GuardedState(1, 13, dev)
    for depth, rgb, pose in frames:
        Frame(dev, depth[None], rgb[None], cam, pose[None]).into(g, S["voxel"], S["trunc"], S["near"], S["far"])
    g.check()
    assert records(g.state, 0) == ref_records(vol) and stats_of(g.state, 0) == vol.stats()
    want = assert_mesh_equals(g, 0, vol, S["voxel"], "sphere")
    keys, vertices, tri, dropped, _ = extract_guarded(g, 0, 2, S["voxel"])
    xyz = vertices[:, :12].copy().view(F).reshape(-1, 3)
    quads = np.concatenate([tri[0::2], tri[1::2, 2:]], axis=1)                    # (0,1,2) + (0,2,3) -> the quad
    assert dropped == 0 and (len(keys), len(quads)) == (1250, 1248)
    edges, shared = T.edge_counts(quads)
    assert (shared == 2).all() and len(keys) - len(edges) + len(quads) == 2
    normal, centre = T.quad_normals(xyz, quads)
    assert ((normal * centre).sum(axis=1) > 0).all()
    assert np.array_equal(quads, want["quads"])


# ---- 3: long probes and wrap-around ----------------------------------------------------------------------------------------------
def _home(key, L2):
    return ((key * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)) >> (64 - L2)


def _insert(keys, L2):
    """Linear probing as the device inserts: slot -> key."""
    table = {}
    for k in keys:
        slot = _home(k, L2)
        while slot in table:
            slot = (slot + 1) % (1 << L2)
        table[slot] = k
    return table


def _lookup_trips(table, key, L2):
    """(trips of the read-only probe for ``key``, whether it passed the table's end)."""
    slot, trips, wrapped = _home(key, L2), 1, False
    while slot in table and table[slot] != key:
        wrapped |= slot == (1 << L2) - 1
        slot = (slot + 1) % (1 << L2)
        trips += 1
    return trips, wrapped


def _crafted_block():
    """A 3 x 3 x 4 block of voxels and 40 lone ones (76 of 128 slots, below the 96-slot mark).  Fibonacci hashing spreads
    neighbouring voxels evenly, so long probes are made on purpose: the lone voxels, inserted first, all hash into the last 24
    slots and pile up across the table's end, and the block's origin is chosen, by a fixed search, so that several of its voxels
    hash into the head of that pile.  The corner look-ups of the extraction then probe for dozens of trips and across the end.
    S and n are drawn so that most cells change sign and some voxels fall below min_frames."""
    L2 = 7
    slots = 1 << L2
    rng = np.random.default_rng(5)
    cells = []
    while len(cells) < 40:
        c = tuple(int(v) for v in rng.integers(-1000, 1000, 3))
        if slots - 24 <= _home(T.pack(*c), L2) and c not in cells:
            cells.append(c)
    while True:
        o = rng.integers(-1000, 1000, 3)
        block = [(int(o[0]) + x, int(o[1]) + y, int(o[2]) + z) for x in range(3) for y in range(3) for z in range(4)]
        if sum(slots - 24 <= _home(T.pack(*c), L2) < slots - 12 for c in block) >= 6 and not set(block) & set(cells):
            break
    cells += block
    keys = [T.pack(*c) for c in cells]
    table = _insert(keys, L2)
    looks = [_lookup_trips(table, T.pack(c[0] + dx, c[1] + dy, c[2] + dz), L2)
             for c in cells for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)]
    assert sum(w for _, w in looks) >= 10, "too few look-ups pass the table's end"
    recs = {}
    for k in keys:
        n = int(rng.integers(2, 6)) if rng.random() < 0.85 else 1
        nc = int(rng.integers(0, n + 1))
        recs[k] = [F(rng.uniform(-1.0, 1.0) * n), n] + [int(rng.integers(0, 256)) * nc for _ in range(3)] + [nc]
    return L2, table, recs, max(t for t, _ in looks)


def test_long_probes_and_wrap_around(dev):
    L2, table, recs, longest = _crafted_block()
    assert longest >= 24 and len(table) == 76 < 96 and L2 == 7
    vol = T.TsdfVolume(0.5, 2)
    vol.records = {k: list(r) for k, r in recs.items()}
    g = GuardedState(1, L2, dev)
    keys = np.full(1 << L2, T.EMPTY, np.uint64)
    rows = np.zeros((1 << L2, 6), np.uint32)
    for slot, k in table.items():
        keys[slot] = k
        rows[slot] = [np.float32(recs[k][0]).view(np.uint32)] + recs[k][1:]
    g.state["keys"][0].copy_(torch.from_numpy(keys.view(np.int64)))
    g.state["recs"][0].copy_(torch.from_numpy(rows.view(np.int32)))
    g.state["stats"][0, 0] = len(table)
    assert records(g.state, 0) == ref_records(vol)
    for m in (1, 2, 3):
        want = vol.extract(m)
        got_keys, vertices, tri, dropped, counts = extract_guarded(g, 0, m, 0.5)
        assert counts == (len(want["keys"]), len(want["raw_quads"])) and np.array_equal(got_keys, want["keys"]), m
        assert np.array_equal(vertices, want["vertices"]) and np.array_equal(tri, want["triangles"]), m
        assert dropped == want["quads_dropped"], m
    assert len(vol.extract(1)["keys"]) >= 8 and len(vol.extract(1)["raw_quads"]) >= 20
    assert len(vol.extract(3)["keys"]) < len(vol.extract(1)["keys"])


# ---- 4: overflow -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L2", [6, 7, 8])
def test_overflow_returns_and_keeps_its_books(plane, dev, L2):
    from m4depth_amd import network_ops as nops
    slots, mark = 1 << L2, (1 << L2) - (1 << (L2 - 2))
    g = GuardedState(B, L2, dev)
    for depth, rgb, poses in plane["frames"][:2]:
        fr = Frame(dev, depth, rgb, plane["cam"], poses)
        fr.into(g, VOXEL, TRUNC, NEAR, FAR)                                      # a refused entry would raise
        fr.check()
    g.check()
    for s in range(B):
        st, got = stats_of(g.state, s), records(g.state, s)
        assert st["dropped_full"] > 0 and st["dropped_range"] == 0
        assert st["occupied"] == len(got) and mark <= len(got) <= min(slots, mark + H * W)    # the mark + the claims in flight
        assert set(got) <= set(plane["want"][1][s][0]), "a key the frames never touched"
        keys, vertices, tri, stats = nops.tsdf_extract(g.state, s, 1, VOXEL)
        assert len(keys) <= len(got) and (len(tri) == 0 or (0 <= int(tri.min()) and int(tri.max()) < len(keys)))
        assert stats["occupied"] == len(got)
    g.check()


# ---- 5: sample independence ------------------------------------------------------------------------------------------------------
def test_batch_launch_equals_per_sample_launches(plane, dev):
    """Four samples: a plane frame, a NaN pose, an all-NaN depth, another plane frame -- two frames each."""
    cam2, frames = plane["cam"], plane["frames"][:2]
    pick = [0, 1, 0, 1]
    cam = {k: v[pick] for k, v in cam2.items()}
    batch = []
    for depth, rgb, poses in frames:
        d, c, p = depth[pick].copy(), rgb[pick].copy(), poses[pick].copy()
        p[1, 2] = np.nan
        d[2] = np.nan
        batch.append((d, c, p))
    g = GuardedState(4, L, dev)
    fresh = npy(GuardedState(1, L, dev).t)
    for d, c, p in batch:
        fr = Frame(dev, d, c, cam, p)
        fr.into(g, VOXEL, TRUNC, NEAR, FAR)
        fr.check()
    g.check()
    for s in range(4):
        alone = GuardedState(1, L, dev)
        for d, c, p in batch:
            Frame(dev, d[s:s + 1], c[s:s + 1], {k: v[s:s + 1] for k, v in cam.items()}, p[s:s + 1]).into(alone, VOXEL, TRUNC, NEAR, FAR)
        alone.check()
        assert records(g.state, s) == records(alone.state, 0) and stats_of(g.state, s) == stats_of(alone.state, 0), s
        a, b2 = extract_guarded(g, s, 1, VOXEL), extract_guarded(alone, 0, 1, VOXEL)
        assert all(np.array_equal(x, y) for x, y in zip(a[:3], b2[:3])) and a[3:] == b2[3:], s
        if s in (1, 2):
            assert not npy(g.state["stats"][s]).any() and np.array_equal(npy(alone.t), fresh), "a sample without input was touched"
            assert (npy(g.state["keys"][s]).view(np.uint64) == np.uint64(T.EMPTY)).all() and not npy(g.state["recs"][s]).any()
            assert a[4] == (0, 0)
        else:
            assert records(g.state, s) == plane["got"][1][pick[s]][0] and a[4][0] > 20


# ---- 6: clear --------------------------------------------------------------------------------------------------------------------
def test_masked_clear_restores_the_fresh_state(plane, dev):
    from m4depth_amd import network_ops as nops
    L2, slots = 11, 1 << 11
    g = GuardedState(3, L2, dev)
    fresh = npy(g.t).copy()
    assert not fresh[:12].any() and (fresh[12:12 + 3 * slots].view(np.uint64) == np.uint64(T.EMPTY)).all() and not fresh[12 + 3 * slots:].any()
    depth, rgb, poses = plane["frames"][0]
    pick = [0, 0, 0]
    Frame(dev, depth[pick], rgb[pick], {k: v[pick] for k, v in plane["cam"].items()}, poses[pick]).into(g, VOXEL, TRUNC, NEAR, FAR)
    full = {k: npy(g.state[k]).copy() for k in ("stats", "keys", "recs")}
    assert all(full["stats"][s, 0] > 100 and full["stats"][s, 3] > 100 and full["recs"][s].any() for s in range(3))
    nops.tsdf_clear(g.state, torch.tensor([1, 0, 1], dtype=torch.uint8, device=dev))
    got = {k: npy(g.state[k]).copy() for k in ("stats", "keys", "recs")}
    for s in (0, 2):
        assert not got["stats"][s].any() and (got["keys"][s].view(np.uint64) == np.uint64(T.EMPTY)).all() and not got["recs"][s].any(), s
    assert all(np.array_equal(got[k][1], full[k][1]) for k in got)
    nops.tsdf_clear(g.state, torch.tensor([False, False, False], device=dev))
    assert all(np.array_equal(npy(g.state[k]), got[k]) for k in got)
    nops.tsdf_clear(g.state)
    assert np.array_equal(npy(g.t), fresh)
    g.check()


# ---- 7: the writer ---------------------------------------------------------------------------------------------------------------
def _writer_run(dev, out, views, **kw):
    """Batch 2 on the rendered plane of depth_views_ref, seven steps through a ring of two slots; slot 1 starts a second
    trajectory at step 3.  Returns (writer, per step: the depths the mesh saw [b,h,w], rgb, poses [b,7], flags)."""
    from m4depth_amd.export import PredictionWriter, FrameNamer
    from m4depth_amd import network_ops as nops
    b, h, w, steps = 2, 24, 40, 7
    cam = {"f": np.tile(np.array([[20.0, 12.0]], F), (b, 1)), "c": np.tile(np.array([[20.3, 11.6]], F), (b, 1))}
    poses = np.zeros((steps, 7))
    poses[:, 0] = 1.0
    poses[:, 4:] = np.array([0.22, -0.12, 0.15])[None] * np.arange(steps)[:, None]
    camera = {k: torch.from_numpy(v).to(dev) for k, v in cam.items()}
    rng = np.random.default_rng(9)
    flags = [[k == 0, k in (0, 3)] for k in range(steps)]
    namer = FrameNamer(b)
    # the chain the writer runs, run again here: the poses it accumulates and the depths its views check lets through
    pose = torch.empty((b, 7), dtype=torch.float64, device=dev)
    vstate = nops.depth_views_state(b, h, w, views, dev) if views else None
    seen = []
    with PredictionWriter(out, "kitti16", near=2.0, far=40.0, slots=2, cloud_step=1, cloud_views=views, **kw) as writer:
        for k in range(steps):
            depth = np.stack([DV.render_plane(poses[k], cam["f"][s], cam["c"][s], h, w) for s in range(b)])
            est = torch.from_numpy(depth[..., None]).to(dev)
            rgb = rng.random((b, h, w, 3)).astype(F)
            rot = torch.tensor([[1.0, 0.0, 0.0, 0.0]] * b, device=dev)
            trans = torch.from_numpy(np.tile((poses[k, 4:] - poses[max(k - 1, 0), 4:]).astype(F), (b, 1))).to(dev)
            writer.submit(est, namer(flags[k]), rgb=torch.from_numpy(rgb).to(dev), rot=rot, trans=trans, camera=camera,
                          reset=np.array(flags[k]))
            mask = torch.tensor(flags[k], dtype=torch.uint8, device=dev)
            nops.pose_accumulate(rot, trans, pose, reset=mask, force_all=k == 0)
            mine = est
            if views:
                _, mine = nops.depth_views(est, camera["f"], camera["c"], pose, vstate, reset=mask, force_all=k == 0)
            seen.append((npy(mine)[..., 0].copy(), rgb, npy(pose).copy(), flags[k]))
    return writer, cam, seen


def _check_mesh_files(out, cam, seen, voxel, trunc, min_frames, near, far):
    from m4depth_amd.export import read_mesh_ply
    vols, dirs, traj = {}, {}, [-1, -1]
    for depth, rgb, pose, flags in seen:
        for s in range(2):
            if flags[s]:
                traj[s] += 1
                vols[f"s{s:02d}_t{traj[s]:04d}"] = T.TsdfVolume(voxel, trunc, near, far)
            vols[f"s{s:02d}_t{traj[s]:04d}"].frame(depth[s], rgb[s], cam["f"][s], cam["c"][s], pose[s])
    sizes = {}
    for d, vol in vols.items():
        want = vol.extract(min_frames)
        xyz, rgba, tri, info = read_mesh_ply(os.path.join(out, d, "mesh.ply"))
        assert np.array_equal(np.concatenate([xyz.view(np.uint8).reshape(-1, 12), rgba], axis=1), want["vertices"]), d
        assert np.array_equal(tri, want["triangles"]), d
        assert info == dict(vol.stats(), voxel=float("%.9g" % np.float32(voxel)), trunc=trunc, min_frames=min_frames,
                            quads_dropped=want["quads_dropped"]), d
        sizes[d] = (len(xyz), len(tri))
    return sizes


@pytest.mark.parametrize("views", [0, 2])
def test_prediction_writer_meshes(dev, tmp_path, views):
    """Every mesh.ply is the restatement of the depths its trajectory's frames gave; the mesh alone writes nothing else, and
    beside the clouds and the map it changes none of their bytes."""
    voxel, trunc = 0.5, 3
    mesh = dict(save_mesh=voxel, mesh_trunc=trunc, mesh_min_frames=2, mesh_slots_log2=14)
    alone, both, without = (str(tmp_path / n) for n in ("alone", "both", "without"))
    writer, cam, seen = _writer_run(dev, alone, views, **mesh)
    want_dirs = ["s00_t0000", "s01_t0000", "s01_t0001"]
    assert sorted(os.listdir(alone)) == want_dirs
    sizes = _check_mesh_files(alone, cam, seen, voxel, trunc, 2, 2.0, 40.0)
    assert writer.meshes == 3 and writer.mesh_vertices == sum(v for v, _ in sizes.values())
    assert writer.mesh_triangles == sum(t for _, t in sizes.values()) and writer.mesh_dropped_full == 0 and writer.mesh_dropped_range == 0
    assert sizes["s00_t0000"][0] > 100 and sizes["s00_t0000"][1] > 100
    if views:                                   # three frames under the strict two-view rule: one frame with depths, no voxel seen twice
        assert sizes["s01_t0000"] == (0, 0)
    else:
        assert sizes["s01_t0000"][0] > 50
    for d, n in zip(want_dirs, (7, 3, 4)):
        assert sorted(os.listdir(os.path.join(alone, d))) == sorted([f"{k:06d}_depth.png" for k in range(n)] + ["mesh.ply"]), d
    w2, _, _ = _writer_run(dev, both, views, cloud=True, save_map=1.0, map_slots_log2=12, **mesh)
    w3, _, _ = _writer_run(dev, without, views, cloud=True, save_map=1.0, map_slots_log2=12)
    assert w2.maps == w3.maps == 3 and w2.meshes == 3 and w3.meshes == 0
    for d in want_dirs:
        files = sorted(os.listdir(os.path.join(both, d)))
        assert files == sorted(os.listdir(os.path.join(without, d)) + ["mesh.ply"]) and "map.ply" in files
        for name in files:
            twin = os.path.join(alone if name == "mesh.ply" else without, d, name)
            with open(os.path.join(both, d, name), "rb") as a, open(twin, "rb") as b2:
                assert a.read() == b2.read(), (d, name)


def test_writer_refuses_device_flags(dev, tmp_path):
    from m4depth_amd.export import PredictionWriter
    b, h, w = 1, 8, 8
    with PredictionWriter(str(tmp_path), "kitti16", save_mesh=0.5, mesh_slots_log2=8) as writer:
        with pytest.raises(ValueError, match="save_mesh needs host-side reset flags"):
            writer.submit(torch.ones((b, h, w, 1), device=dev), ["s00_t0000/000000"], rgb=torch.zeros((b, h, w, 3), device=dev),
                          rot=torch.tensor([[1.0, 0, 0, 0]], device=dev), trans=torch.zeros((b, 3), device=dev),
                          camera={"f": torch.ones((b, 2), device=dev), "c": torch.ones((b, 2), device=dev)},
                          reset=torch.zeros(b, dtype=torch.uint8, device=dev))


# ---- 8: the driver ---------------------------------------------------------------------------------------------------------------
N_TRAJ, N_FRAMES = 2, 8
_runs = {}


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("tsdf_mesh"))
    db, rec = make_fake_dataset(root, "midair", n_traj=N_TRAJ, n_frames=N_FRAMES)          # 48 x 64
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
                              dataset["rec"], "--arch_depth", "2", "--height", "48", "--width", "64", "--ckpt_dir",
                              out + "_ckpt"] + [a.replace("OUT", out) for a in extra]) == 0
        _runs[key] = (out, printed.getvalue())
    return _runs[key]


def mesh_run(dataset, key, extra):
    out, _ = run_driver(dataset, "plain", [])
    preds = np.load(out + "_ckpt/predictions.npy")
    near, far = (float(F(v)) for v in np.percentile(preds, [10, 90]))
    voxel = float(F((far - near) / 8.0))
    assert 0 < near < far and voxel > 0
    return run_driver(dataset, key, extra + ["--save_dir", "OUT", "--save_range", repr(near), repr(far), "--save_mesh", repr(voxel),
                                             "--mesh_trunc", "2", "--mesh_min_frames", "1", "--mesh_slots_log2", "16"]) + (voxel,)


def test_driver_paths_write_identical_meshes(dev, dataset):
    from m4depth_amd.export import read_mesh_ply
    frames, printed, voxel = mesh_run(dataset, "frames", [])
    others = [mesh_run(dataset, "stream", ["--stream"])[0], mesh_run(dataset, "stream-graph", ["--stream", "--graph"])[0],
              mesh_run(dataset, "sequences", ["--db_seq_len", str(N_FRAMES), "--seq_len", str(N_FRAMES), "--batch_size", "1"])[0]]
    want_dirs = [f"s00_t{t:04d}" for t in range(N_TRAJ)]
    assert sorted(os.listdir(frames)) == want_dirs
    totals = [0, 0]
    for d in want_dirs:
        assert sorted(os.listdir(os.path.join(frames, d))) == sorted([f"{k:06d}_depth.png" for k in range(N_FRAMES)] + ["mesh.ply"])
        xyz, rgba, tri, info = read_mesh_ply(os.path.join(frames, d, "mesh.ply"))
        assert info["occupied"] > 100 and info["updates"] > 100 and info["dropped_full"] == 0
        assert len(xyz) > 20 and len(tri) > 20, "an estimate of a random network still has a surface"
        totals[0] += len(xyz)
        totals[1] += len(tri)
        with open(os.path.join(frames, d, "mesh.ply"), "rb") as fh:
            want = fh.read()
        for other in others:
            with open(os.path.join(other, d, "mesh.ply"), "rb") as fh:
                assert fh.read() == want, (other, d)
    for key, extra in (("refine", ["--stream", "--refine_pose"]), ("refine-graph", ["--stream", "--graph", "--refine_pose"])):
        refined = mesh_run(dataset, key, extra)[0]                               # other poses, so other meshes: they are written
        for d in want_dirs:
            xyz, rgba, tri, info = read_mesh_ply(os.path.join(refined, d, "mesh.ply"))
            assert info["occupied"] > 100 and info["updates"] > 100 and len(xyz) > 20 and len(tri) > 20, (key, d)
    (line,) = [l for l in printed.splitlines() if l.startswith("predict: wrote")]
    assert f"{N_TRAJ} meshes at {voxel:g} m: {totals[0]} vertices, {totals[1]} triangles, 0 samples dropped out of range, " \
           "0 dropped by full tables)" in line


def test_driver_mesh_beside_clouds_and_map(dev, dataset):
    """--save_mesh with --save_cloud, --save_map and --cloud_views: the same clouds and map as without it; a full table is
    reported with the hint."""
    base = ["--save_cloud", "--cloud_views", "2", "--save_map", "0.5", "--map_slots_log2", "16", "--stream"]
    out, _ = run_driver(dataset, "plain", [])
    with_mesh, printed, voxel = mesh_run(dataset, "all", base)
    preds = np.load(out + "_ckpt/predictions.npy")
    near, far = (repr(float(F(v))) for v in np.percentile(preds, [10, 90]))
    without, _ = run_driver(dataset, "no-mesh", base + ["--save_dir", "OUT", "--save_range", near, far])
    for d in sorted(os.listdir(without)):
        files = sorted(os.listdir(os.path.join(without, d)))
        assert sorted(files + ["mesh.ply"]) == sorted(os.listdir(os.path.join(with_mesh, d))) and "map.ply" in files
        for name in files:
            with open(os.path.join(without, d, name), "rb") as a, open(os.path.join(with_mesh, d, name), "rb") as b2:
                assert a.read() == b2.read(), (d, name)
    assert "raise --mesh_slots_log2" not in printed
