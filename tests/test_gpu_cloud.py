"""Point-cloud export (m4d_pose_accumulate, m4d_depth_cloud, export.PredictionWriter(cloud=True), main.py --save_cloud) against
a numpy restatement of the formulas in include/m4depth_hip.h.

Camera-frame vertices are + - * / on float32, one rounding per operation, and the compaction is a pure reordering: counts and
bytes are compared exactly.  World-frame vertices are + - * on float64 in the kernel's operand order (tests/pose_ref.py) and one
rounding to float32: the kernel's own bytes are compared exactly too.  The pose chain adds float64 sqrt and /, which IEEE 754
rounds correctly on both sides: every state of the 200 steps is compared bit for bit.  (The writer and driver tests, whose
poses travel through files, keep the one-ulp / 1e-12 bounds they had.)"""
import csv
import json
import os

import numpy as np
import pytest
import torch

from helpers import F, npy, make_fake_dataset
from pose_ref import rot as rot_matrix, apply_pose

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 64                                                                      # bytes before and after the vertex buffer


# ---- the restatement -----------------------------------------------------------------------------------------------------
def pose_step(pose, rot, trans, reset):
    """m4d_pose_accumulate of one sample: pose [7] float64, rot [4] / trans [3] float32."""
    if reset:
        return np.array([1, 0, 0, 0, 0, 0, 0], np.float64)
    w, x, y, z = (np.float64(v) for v in rot)
    n = np.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    pw, px, py, pz = pose[:4]
    t = apply_pose(pose, *(np.float64(v) for v in trans))
    rw = ((pw * w - px * x) - py * y) - pz * z
    rx = ((pw * x + px * w) + py * z) - pz * y
    ry = ((pw * y - px * z) + py * w) + pz * x
    rz = ((pw * z + px * y) - py * x) + pz * w
    m = np.sqrt(((rw * rw + rx * rx) + ry * ry) + rz * rz)
    return np.array([rw / m, rx / m, ry / m, rz / m, t[0], t[1], t[2]], np.float64)


def rgb_bytes(v):
    v = np.asarray(v, F)
    v = np.where(np.isnan(v), F(0.0), v)
    return np.rint(np.minimum(np.maximum(v, F(0.0)), F(1.0)) * F(255.0)).astype(np.uint8)


def cloud_of(depth, colours, f, c, step, near, far, pose=None):
    """One sample: depth [h,w] float32, colours [h,w,3] uint8, f / c [2] float32 -> (xyz float32 [n,3], rgba uint8 [n,4]) in
    raster order."""
    depth = np.asarray(depth, F)
    keep = np.zeros(depth.shape, bool)
    with np.errstate(invalid="ignore"):
        keep[::step, ::step] = (np.isfinite(depth) & (depth >= F(near)) & (depth <= F(far)))[::step, ::step]
    rows, cols = np.nonzero(keep)                                               # row-major = raster order
    d = depth[rows, cols]
    x = (((cols.astype(F) + F(0.5)) - F(c[0])) / F(f[0])) * d
    y = (((rows.astype(F) + F(0.5)) - F(c[1])) / F(f[1])) * d
    xyz = np.stack([x, y, d], axis=1).astype(F).reshape(-1, 3)
    if pose is not None:
        xyz = np.stack([v.astype(F) for v in apply_pose(pose, x, y, d)], axis=1).reshape(-1, 3)
    rgba = np.concatenate([colours[rows, cols], np.full((len(rows), 1), 255, np.uint8)], axis=1)
    return xyz, rgba


def as_bytes(xyz, rgba):
    return np.concatenate([np.ascontiguousarray(xyz, F).view(np.uint8).reshape(-1, 12), rgba], axis=1)


def within_one_ulp(got, want):
    got, want = np.asarray(got, F), np.asarray(want, F)
    return (got == want) | (got == np.nextafter(want, F(np.inf))) | (got == np.nextafter(want, F(-np.inf)))


# ---- 1 + 2: the kernel -------------------------------------------------------------------------------------------------------
B, H, W = 3, 37, 53
NEAR, FAR = 1.5, 60.0
FULL_ROWS, EMPTY_ROWS = slice(9, 22), slice(22, 37)      # whole waves (step 1: whole workgroups) full, then empty, at every step


def _case():
    """Sample 0: about half of the pixels kept, every kind of dropped value sprinkled in, then 13 rows that are all kept and
    15 rows that are all dropped; sample 1 all dropped; sample 2 all kept (the bounds themselves included)."""
    rng = np.random.default_rng(2024)
    bad = np.array([np.nan, np.inf, -np.inf, -3.0, 0.0, 1.4999999, 60.000004, 1e-30, 3e38], F)
    depth = np.empty((B, H, W), F)
    inside = rng.uniform(NEAR, FAR, (H, W)).astype(F)
    outside = np.where(rng.random((H, W)) < 0.5, rng.uniform(0.0, NEAR * 0.99, (H, W)), rng.uniform(FAR * 1.01, 500.0, (H, W)))
    depth[0] = np.where(rng.random((H, W)) < 0.5, inside, outside.astype(F))
    spots = rng.permutation(9 * W)[:4 * len(bad)]
    depth[0].reshape(-1)[spots] = np.tile(bad, 4)
    depth[0, FULL_ROWS] = rng.uniform(NEAR, FAR, (13, W)).astype(F)
    depth[0, EMPTY_ROWS] = rng.choice(bad, (15, W))
    depth[1] = rng.choice(bad, (H, W))
    depth[2] = rng.uniform(NEAR, FAR, (H, W)).astype(F)
    depth[2, 0, 0], depth[2, -1, -1], depth[2, 18, 26] = F(NEAR), F(FAR), F(NEAR)
    rgb = rng.uniform(-0.2, 1.2, (B, H, W, 3)).astype(F)
    rgb.reshape(-1)[rng.permutation(rgb.size)[:40]] = np.tile(np.array([np.nan, -5.0, 7.0, 0.5], F), 10)
    f = np.array([[0.55 * W, 0.45 * H], [0.5 * W, 0.5 * H], [31.25, 17.5]], F)
    c = np.array([[0.5 * W + 0.3, 0.5 * H - 0.7], [0.5 * W, 0.5 * H], [20.0, 21.5]], F)
    ang = rng.uniform(-np.pi, np.pi, B)
    axis = rng.normal(size=(B, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    q = np.concatenate([np.cos(ang / 2)[:, None], axis * np.sin(ang / 2)[:, None]], axis=1)
    pose = np.concatenate([q / np.linalg.norm(q, axis=1, keepdims=True), rng.uniform(-5.0, 5.0, (B, 3))], axis=1)
    return depth, rgb, f, c, pose.astype(np.float64)


CASE = _case()
for _a in CASE:
    _a.setflags(write=False)


def _run(dev, step, pose, strided):
    from m4depth_amd import network_ops as nops
    depth, rgb, f, c, _ = CASE
    cap = nops.cloud_capacity(H, W, step)
    d = torch.from_numpy(depth.reshape(B, H, W, 1).copy()).to(dev)
    r = torch.from_numpy(rgb.copy()).to(dev)
    if strided:                                                                 # frame slices of taller buffers, read in place
        tall_d = torch.full((B, H + 2, W, 1), float("nan"), device=dev)
        tall_r = torch.full((B, H + 5, W, 3), float("nan"), device=dev)
        tall_d[:, :H], tall_r[:, :H] = d, r
        d, r = tall_d[:, :H], tall_r[:, :H]
    flat = torch.full((GUARD + B * cap * 16 + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    vertices = flat[GUARD:GUARD + B * cap * 16].view(B, cap, 16)
    counts = torch.full((B,), -7, dtype=torch.int32, device=dev)
    pose_d = None if pose is None else torch.from_numpy(pose.copy()).to(dev)
    got_v, got_c = nops.depth_cloud(d, r, torch.from_numpy(f.copy()).to(dev), torch.from_numpy(c.copy()).to(dev), step=step,
                                    near=NEAR, far=FAR, pose=pose_d, vertices=vertices, counts=counts)
    torch.cuda.synchronize()
    assert got_v is vertices and got_c is counts
    flat = npy(flat)
    assert (flat[:GUARD] == SENTINEL).all() and (flat[-GUARD:] == SENTINEL).all(), "bytes outside the vertex buffer overwritten"
    return npy(vertices), npy(counts), cap


@pytest.mark.parametrize("step", [1, 2, 3])
def test_compaction_matches_the_restatement_byte_for_byte(dev, step):
    depth, rgb, f, c, _ = CASE
    got, counts, cap = _run(dev, step, None, strided=(step == 2))
    colours = rgb_bytes(rgb)
    assert cap == -(-H // step) * -(-W // step)
    assert step == 3 or (cap > 256 and cap % 256)                               # several workgroups per sample, the last partial
    for s in range(B):
        want = as_bytes(*cloud_of(depth[s], colours[s], f[s], c[s], step, NEAR, FAR))
        print(f"step {step} sample {s}: {counts[s]} of {cap} kept")
        assert counts[s] == len(want), (s, counts[s], len(want))
        bad = np.argwhere(got[s, :len(want)] != want)
        assert len(bad) == 0, f"sample {s}: {len(bad)} bytes differ; first at vertex {bad[0][0]}, byte {bad[0][1]}"
        assert (got[s, len(want):] == SENTINEL).all(), f"sample {s}: bytes beyond the count were written"
    assert counts[1] == 0 and counts[2] == cap and 0.3 * cap < counts[0] < 0.7 * cap


@pytest.mark.parametrize("step", [1, 2, 3])
def test_world_frame_within_one_ulp_of_float64(dev, step):
    depth, rgb, f, c, pose = CASE
    got, counts, cap = _run(dev, step, pose, strided=False)
    colours = rgb_bytes(rgb)
    for s in range(B):
        xyz, rgba = cloud_of(depth[s], colours[s], f[s], c[s], step, NEAR, FAR, pose=pose[s])
        n = len(xyz)
        assert counts[s] == n
        got_xyz = got[s, :n, :12].copy().view(F)
        assert np.array_equal(got[s, :n, 12:], rgba), f"sample {s}: colours or order differ"
        bad = np.argwhere(got_xyz.view(np.uint32) != xyz.view(np.uint32))
        print(f"step {step} sample {s}: {len(bad)} of {3 * n} coordinates differ from numpy; "
              f"{int((~within_one_ulp(got_xyz, xyz)).sum())} by more than one ulp")
        assert len(bad) == 0, f"sample {s}: {len(bad)} coordinates differ in their bits; first at {bad[0]}"
        assert (got[s, n:] == SENTINEL).all()


def test_cloud_replays_from_a_captured_graph(dev):
    """Both entry points are plain launches: captured once, replayed on new poses and depths."""
    from m4depth_amd import network_ops as nops
    depth, rgb, f, c, pose = CASE
    d = torch.from_numpy(depth.reshape(B, H, W, 1).copy()).to(dev)
    r, fd, cd = (torch.from_numpy(a.copy()).to(dev) for a in (rgb, f, c))
    state = torch.from_numpy(pose.copy()).to(dev)
    rot = torch.tensor([[1.0, 0, 0, 0]] * B, device=dev)
    trans = torch.tensor([[0.5, -1.0, 2.0]] * B, device=dev)
    vertices = torch.zeros((B, nops.cloud_capacity(H, W, 2), 16), dtype=torch.uint8, device=dev)
    counts = torch.zeros(B, dtype=torch.int32, device=dev)
    nops.depth_cloud(d, r, fd, cd, step=2, near=NEAR, far=FAR, pose=state, vertices=vertices, counts=counts)   # eager warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        nops.pose_accumulate(rot, trans, state)
        nops.depth_cloud(d, r, fd, cd, step=2, near=NEAR, far=FAR, pose=state, vertices=vertices, counts=counts)
    state.copy_(torch.from_numpy(pose.copy()))
    graph.replay()
    torch.cuda.synchronize()
    want_pose = np.stack([pose_step(pose[s], [1, 0, 0, 0], [0.5, -1.0, 2.0], False) for s in range(B)])
    assert np.abs(npy(state) - want_pose).max() <= 1e-12
    colours = rgb_bytes(rgb)
    for s in (0, 2):
        xyz, rgba = cloud_of(depth[s], colours[s], f[s], c[s], 2, NEAR, FAR, pose=npy(state)[s])
        n = int(npy(counts)[s])
        assert n == len(xyz) and within_one_ulp(npy(vertices)[s, :n, :12].copy().view(F), xyz).all()


# ---- 3: the pose chain -------------------------------------------------------------------------------------------------------
def test_pose_chain_follows_float64_numpy(dev):
    from m4depth_amd import network_ops as nops
    b, steps = 4, 200
    rng = np.random.default_rng(7)
    ang = np.deg2rad(rng.uniform(0.0, 4.0, (steps, b)))
    axis = rng.normal(size=(steps, b, 3))
    axis /= np.linalg.norm(axis, axis=2, keepdims=True)
    rot = np.concatenate([np.cos(ang / 2)[..., None], axis * np.sin(ang / 2)[..., None]], axis=2)
    rot = (rot * rng.uniform(0.7, 1.4, (steps, b, 1))).astype(F)                # not unit: the kernel normalises
    trans = rng.normal(0.0, 1.0, (steps, b, 3)).astype(F)
    reset = np.zeros((steps, b), bool)
    reset[0] = True
    reset[[37, 150], 1] = True
    reset[90, 2] = True
    reset[199, 3] = True                                                        # on the last step: the final state is a reset one
    force = {120}
    rot_d, trans_d, reset_d = (torch.from_numpy(a).to(dev) for a in (rot, trans, reset.view(np.uint8)))
    state = torch.full((b, 7), float("nan"), dtype=torch.float64, device=dev)
    trace = torch.empty((steps, b, 7), dtype=torch.float64, device=dev)
    for k in range(steps):
        nops.pose_accumulate(rot_d[k], trans_d[k], state, reset=reset_d[k] if k % 2 else reset_d[k].bool(), force_all=k in force)
        trace[k].copy_(state)
    got = npy(trace)
    want = np.empty((steps, b, 7))
    pose = np.full((b, 7), np.nan)
    for k in range(steps):
        pose = np.stack([pose_step(pose[s], rot[k, s], trans[k, s], reset[k, s] or k in force) for s in range(b)])
        want[k] = pose
    err = np.abs(got - want).max()
    differ = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    norm = np.abs(np.linalg.norm(got[..., :4], axis=-1) - 1.0).max()
    print(f"pose chain: max |device - numpy| {err:.3e}, {len(differ)} of {got.size} values differ in their bits, "
          f"max |norm - 1| {norm:.3e}, |t| up to {np.abs(want[..., 4:]).max():.1f}")
    assert np.isfinite(got).all() and err <= 1e-12
    assert len(differ) == 0, f"first difference at (step, sample, word) {differ[0]}"
    assert norm <= 1e-15
    identity = np.array([1, 0, 0, 0, 0, 0, 0], np.float64)
    for k, s in list(zip(*np.nonzero(reset))) + [(120, s) for s in range(b)]:
        assert np.array_equal(got[k, s], identity), (k, s)
    assert np.array_equal(got[199, 3], identity) and not np.array_equal(got[199, 0], identity)
    nops.pose_accumulate(rot_d[0], trans_d[0], state)                          # no mask at all: nobody resets
    torch.cuda.synchronize()
    assert not (npy(state) == identity).all(axis=1).any()


# ---- 4: the convention, tied to the library's own warp -----------------------------------------------------------------------
def test_world_points_project_where_reproject_flow_says(dev):
    """A point X of the current camera is R(rot) X + trans in the previous camera: the cloud of the current frame, posed by one
    m4d_pose_accumulate step from the identity, is in the previous camera's frame, and projecting it with f must give the
    coordinates m4d_reproject_flow warps with (proj = flow[..., ::-1] + mesh).  About 20 float32 roundings apart on coordinates
    <= 64 px with pz >= 1: of order 1e-4 px; 1e-3 px leaves a decade.  The inverse pose misses by pixels."""
    from m4depth_amd import network_ops as nops
    from m4depth_amd._lib import lib, dptr, stream_ptr, check
    h, w = 32, 48
    rng = np.random.default_rng(99)
    depth = rng.uniform(2.0, 50.0, (1, h, w, 1)).astype(F)
    ang = np.deg2rad(5.0)
    axis = np.array([0.3, -0.8, 0.52]) / np.linalg.norm([0.3, -0.8, 0.52])
    rot = np.concatenate([[np.cos(ang / 2)], axis * np.sin(ang / 2)]).astype(F)[None]
    trans = np.array([[0.3, -0.25, 0.3]], F)
    assert np.linalg.norm(trans) <= 0.5
    f, c = np.array([[0.5 * w, 0.5 * h]], F), np.array([[0.5 * w - 0.25, 0.5 * h + 0.5]], F)
    d, rot_d, trans_d, fd, cd = (torch.from_numpy(a).to(dev) for a in (depth, rot, trans, f, c))
    flow = torch.empty((1, h, w, 2), dtype=torch.float32, device=dev)
    check(lib.m4d_reproject_flow(dptr(d), dptr(rot_d), 4, dptr(trans_d), dptr(fd), dptr(cd), 1, h, w, dptr(flow), None, None,
                                 stream_ptr()), "m4d_reproject_flow")
    state = torch.empty((1, 7), dtype=torch.float64, device=dev)
    nops.pose_accumulate(rot_d, trans_d, state, force_all=True)
    nops.pose_accumulate(rot_d, trans_d, state)
    rgb = torch.zeros((1, h, w, 3), device=dev)
    posed, counts = nops.depth_cloud(d, rgb, fd, cd, step=1, near=1.0, far=80.0, pose=state)
    plain, _ = nops.depth_cloud(d, rgb, fd, cd, step=1, near=1.0, far=80.0)
    torch.cuda.synchronize()
    assert int(counts[0]) == h * w                                              # every pixel kept: vertex k is pixel k
    rows, cols = np.divmod(np.arange(h * w), w)
    mesh = np.stack([(cols + 0.5) - np.float64(c[0, 0]), (rows + 0.5) - np.float64(c[0, 1])], axis=1)
    want = npy(flow).reshape(h * w, 2)[:, ::-1].astype(np.float64) + mesh

    def project(xyz):
        xyz = xyz.astype(np.float64)
        return np.stack([f[0, 0] * xyz[:, 0] / xyz[:, 2], f[0, 1] * xyz[:, 1] / xyz[:, 2]], axis=1)

    P = npy(posed)[0, :, :12].copy().view(F)
    assert P[:, 2].min() >= 1.0
    err = np.abs(project(P) - want).max()
    X = npy(plain)[0, :, :12].copy().view(F).astype(np.float64)                 # the same through numpy: R X + t of the vertices
    by_hand = np.stack(apply_pose(np.concatenate([rot[0] / np.linalg.norm(rot[0].astype(np.float64)), trans[0]]), *X.T), axis=1)
    err_hand = np.abs(project(by_hand) - want).max()
    R = np.array(rot_matrix(rot[0].astype(np.float64) / np.linalg.norm(rot[0].astype(np.float64))))
    inverse = (X - trans[0].astype(np.float64)) @ R                             # R^T (X - t): the pose the other way round
    err_inverse = np.abs(project(inverse) - want).max()
    print(f"projection of the posed cloud against reproject_flow: {err:.3e} px (numpy transform {err_hand:.3e} px; "
          f"inverse pose {err_inverse:.3e} px)")
    assert err <= 1e-3 and err_hand <= 1e-3
    assert err_inverse > 0.5


# ---- the writer --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", ["world", "camera"])
def test_prediction_writer_clouds(dev, tmp_path, frame):
    """Three samples over seven steps through a ring of two slots: every file equals the kernels' own output for that step."""
    from m4depth_amd import network_ops as nops
    from m4depth_amd.export import PredictionWriter, FrameNamer, read_cloud_ply
    b, h, w, steps, step = 3, 24, 40, 7, 2
    rng = np.random.default_rng(31)
    camera = {"f": torch.tensor([[20.0, 12.0]] * b, device=dev), "c": torch.tensor([[20.0, 12.0]] * b, device=dev)}
    flags = [[k == 0, k in (0, 3), k in (0, 5)] for k in range(steps)]
    namer, want = FrameNamer(b), {}
    state = torch.empty((b, 7), dtype=torch.float64, device=dev)
    out = str(tmp_path / "out")
    with PredictionWriter(out, "kitti16", near=2.0, far=40.0, slots=2, cloud=True, cloud_step=step, cloud_frame=frame) as writer:
        for k in range(steps):
            est = torch.from_numpy(rng.uniform(0.5, 80.0, (b, h, w, 1)).astype(F)).to(dev)
            rgb = torch.from_numpy(rng.random((b, h, w, 3)).astype(F)).to(dev)
            rot = torch.from_numpy(np.concatenate([np.ones((b, 1)), rng.normal(0, 0.02, (b, 3))], 1).astype(F)).to(dev)
            trans = torch.from_numpy(rng.normal(0, 0.5, (b, 3)).astype(F)).to(dev)
            names = namer(flags[k])
            reset = torch.tensor(flags[k]) if k % 2 else np.array(flags[k])    # host tensor or array, as the loaders give it
            writer.submit(est, names, rgb=rgb, rot=rot, trans=trans, camera=camera, reset=reset)
            nops.pose_accumulate(rot, trans, state, reset=torch.tensor(flags[k], device=dev), force_all=k == 0)
            v, n = nops.depth_cloud(est, rgb, camera["f"], camera["c"], step=step, near=2.0, far=40.0,
                                    pose=state if frame == "world" else None)
            for s, name in enumerate(names):
                want[name] = (npy(v[s, :int(n[s])]), npy(state[s]))
    found = sorted(os.path.relpath(os.path.join(r, f), out) for r, _, fs in os.walk(out) for f in fs)
    assert found == sorted(n + s for n in want for s in ("_cloud.ply", "_depth.png")) and len(found) == 42
    for name, (v, pose) in want.items():
        xyz, rgba, got_pose = read_cloud_ply(os.path.join(out, name + "_cloud.ply"))
        assert 0 < len(v) < 240 and np.array_equal(as_bytes(xyz, rgba), v), name
        assert np.array_equal(got_pose, pose), name
        if name.endswith("/000000"):
            assert np.array_equal(got_pose, [1, 0, 0, 0, 0, 0, 0]), name
    with pytest.raises(ValueError, match="needs rgb, rot, trans and camera"):
        with PredictionWriter(out, "kitti16", cloud=True) as writer:
            writer.submit(est, names, rgb=rgb)


# ---- 5: the driver -------------------------------------------------------------------------------------------------------------
PATHS = {"frames": [], "stream": ["--stream"], "stream-graph": ["--stream", "--graph"]}
N_TRAJ, N_FRAMES, SIZE = 2, 8, 64
_runs = {}


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("cloud"))
    db, rec = make_fake_dataset(root, "midair", n_traj=N_TRAJ, n_frames=N_FRAMES, size=(SIZE, SIZE))
    cfg = os.path.join(root, "datasets_location.json")
    with open(cfg, "w") as fh:
        json.dump({"midair": "./db"}, fh)
    return {"root": root, "rec": rec, "cfg": cfg}


def run_driver(dataset, key, extra):
    """One ``main`` run per distinct option list of the module: (output directory, library launches it issued)."""
    if key not in _runs:
        from m4depth_amd import main as MAIN
        from m4depth_amd._lib import lib
        out = os.path.join(dataset["root"], key)
        n0 = lib.m4d_launch_count()
        assert MAIN.main(["--mode", "predict", "--dataset", "midair", "--db_path_config", dataset["cfg"], "--records_path",
                          dataset["rec"], "--arch_depth", "2", "--height", str(SIZE), "--width", str(SIZE), "--ckpt_dir",
                          out + "_ckpt"] + [a.replace("OUT", out) for a in extra]) == 0
        _runs[key] = (out, lib.m4d_launch_count() - n0)
    return _runs[key]


def predictions(dataset):
    """The plain predict run's depths [16,64,64] and the depth range the cloud runs keep: its 20th to 80th percentile."""
    out, _ = run_driver(dataset, "plain", [])
    preds = np.load(out + "_ckpt/predictions.npy")[..., 0]
    assert preds.shape == (N_TRAJ * N_FRAMES, SIZE, SIZE) and np.isfinite(preds).all()
    near, far = (float(F(v)) for v in np.percentile(preds, [20, 80]))
    assert 0 < near < far
    return preds, near, far


def cloud_run(dataset, path, frame, stride):
    _, near, far = predictions(dataset)
    return run_driver(dataset, f"{path}_{frame}_{stride}",
                      PATHS[path] + ["--save_dir", "OUT", "--save_cloud", "--cloud_frame", frame, "--cloud_stride", str(stride),
                                     "--save_range", repr(near), repr(far), "--save_panels", "rgb"])


def csv_pose_chain(dataset, traj):
    """Camera-to-world poses of a trajectory's frames from its csv, chained in numpy float64 (the loader hands the network
    float32 rot / trans; the first frame starts the trajectory)."""
    with open(os.path.join(dataset["rec"], f"set_{traj}", f"traj_{traj:04d}.csv"), newline="") as fh:
        rows = list(csv.DictReader(fh, delimiter="\t"))
    poses, pose = [], None
    for k, row in enumerate(rows):
        rot = np.array([row[c] for c in ("qw", "qx", "qy", "qz")], np.float64).astype(F)
        trans = np.array([row[c] for c in ("tx", "ty", "tz")], np.float64).astype(F)
        pose = pose_step(pose, rot, trans, k == 0)
        poses.append(pose)
    return poses


def check_cloud_files(dataset, out, frame, stride):
    from PIL import Image
    from m4depth_amd.export import read_cloud_ply
    preds, near, far = predictions(dataset)
    files = sorted(os.path.join(d, f) for d in sorted(os.listdir(out)) for f in os.listdir(os.path.join(out, d)))
    depth_files = [f for f in files if f.endswith("_depth.png")]
    assert len(depth_files) == N_TRAJ * N_FRAMES and len(files) == 3 * len(depth_files)
    kept = 0
    for i, name in enumerate(depth_files):
        stem = os.path.join(out, name[:-len("_depth.png")])
        assert os.path.isfile(stem + "_cloud.ply"), name                        # one cloud next to every depth map
        xyz, rgba, pose = read_cloud_ply(stem + "_cloud.ply")
        traj, k = divmod(i, N_FRAMES)
        want_pose = csv_pose_chain(dataset, traj)[k]
        # the csv's chain against the device's: the same float64 arithmetic in the same order, so the bound is the one the
        # pose chain of test 3 holds to (1e-12 absolute), not a looser one
        assert np.abs(pose - want_pose).max() <= 1e-12, (name, pose, want_pose)
        if k == 0:
            assert np.array_equal(pose, [1, 0, 0, 0, 0, 0, 0]), name
        # the frame's colours from the dataset's own file, not from anything the run wrote: the loader's u8 / 255 (frames are
        # stored at the network's size, so its bilinear resize is the identity) under the restated byte rule
        with Image.open(os.path.join(dataset["root"], "db", f"traj_{traj}", "color", f"{k:06d}.JPEG")) as im:
            colours = rgb_bytes(np.asarray(im.convert("RGB"), F) / F(255.0))
        f = c = np.array([0.5 * SIZE, 0.5 * SIZE], F)
        want_xyz, want_rgba = cloud_of(preds[i], colours, f, c, stride, near, far, pose=pose if frame == "world" else None)
        assert len(xyz) == len(want_xyz) and np.array_equal(rgba, want_rgba), name
        if frame == "camera":
            assert np.array_equal(as_bytes(xyz, rgba), as_bytes(want_xyz, want_rgba)), name
        else:
            assert within_one_ulp(xyz, want_xyz).all(), name
        kept += len(xyz)
    cap = (-(-SIZE // stride)) ** 2 * len(depth_files)
    assert 0.4 * cap < kept < 0.8 * cap                                         # the 20th to 80th percentile of the lattice
    return files


@pytest.mark.parametrize("path", list(PATHS))
def test_driver_writes_world_clouds(dev, dataset, path):
    out, _ = cloud_run(dataset, path, "world", 2)
    check_cloud_files(dataset, out, "world", 2)


def test_driver_camera_frame_clouds_are_exact(dev, dataset):
    out, _ = cloud_run(dataset, "frames", "camera", 3)
    check_cloud_files(dataset, out, "camera", 3)


def test_driver_paths_write_identical_files(dev, dataset):
    outs = [cloud_run(dataset, path, "world", 2)[0] for path in PATHS]
    names = sorted(os.path.join(d, f) for d in sorted(os.listdir(outs[0])) for f in os.listdir(os.path.join(outs[0], d)))
    assert len(names) == 3 * N_TRAJ * N_FRAMES
    for other in outs[1:]:
        for name in names:
            with open(os.path.join(outs[0], name), "rb") as a, open(os.path.join(other, name), "rb") as b:
                assert a.read() == b.read(), (other, name)


def test_driver_without_the_option_is_unchanged(dev, dataset):
    """No .ply, and the launches of a --save_dir run stay what they were: the forward's plus one m4d_depth_export per frame.
    With --save_cloud each frame adds three (the pose step and the two compaction passes)."""
    _, near, far = predictions(dataset)
    _, plain = run_driver(dataset, "plain", [])
    saved, with_save = run_driver(dataset, "saved", ["--save_dir", "OUT", "--save_range", repr(near), repr(far), "--save_panels", "rgb"])
    _, with_cloud = cloud_run(dataset, "frames", "world", 2)
    files = [f for _, _, fs in os.walk(saved) for f in fs]
    assert len(files) == 2 * N_TRAJ * N_FRAMES and not [f for f in files if f.endswith(".ply")]
    assert with_save - plain == N_TRAJ * N_FRAMES
    assert with_cloud - with_save == 3 * N_TRAJ * N_FRAMES
