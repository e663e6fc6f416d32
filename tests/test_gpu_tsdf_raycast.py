"""m4d_tsdf_raycast on the GPU (network_ops.tsdf_raycast, fusion.FusedDepth, main.py --fused) against the numpy restatement
tests/tsdf_raycast_ref.py, bit for bit -- NaN positions and hit counts included.  The march is a fixed sequence of float32 /
float64 operations rounded once each on a state that is only read, so there is no tolerance anywhere; what the restatement itself
is worth is measured in tests/test_tsdf_raycast_ref.py.  The volumes are built on the device with network_ops.tsdf_integrate
(held to tsdf_mesh_ref.TsdfVolume by tests/test_gpu_tsdf_mesh.py) and in the restatement from the same frames.  Every buffer the
launch reads or writes lies between sentinel guards."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

from helpers import F, npy, cameras_np, make_fake_dataset
import tsdf_mesh_ref as T
import tsdf_raycast_ref as RC
from test_gpu_tsdf_mesh import Guarded, GuardedState, Frame, records, ref_records

pytestmark = pytest.mark.gpu

B, H, W, L = 2, T.PLANE["h"], T.PLANE["w"], 14
VOXEL, TRUNC, NEAR, FAR = T.PLANE["voxel"], T.PLANE["trunc"], 1.0, 20.0          # 153 positions per ray


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _plane_inputs():
    """Four frames for two samples with their own off-centre cameras; sample 1 sees the poses in another order.  The render
    poses: sample 0 a fused one, sample 1 a novel one."""
    cam = cameras_np(B, H, W)
    poses = T.plane_poses(6)
    rng = np.random.default_rng(5)
    frames = []
    for k in range(4):
        ps = [poses[k], poses[(2, 0, 3, 1)[k]]]
        depth = np.stack([T.render_plane(ps[s], cam["f"][s], cam["c"][s], H, W, T.PLANE_NORMAL, T.PLANE_OFFSET) for s in range(B)])
        frames.append((depth, rng.random((B, H, W, 3)).astype(F), np.stack(ps)))
    return cam, frames, np.stack([poses[3], poses[5]])


@pytest.fixture(scope="module")
def plane(dev):
    cam, frames, render = _plane_inputs()
    vols = [T.TsdfVolume(VOXEL, TRUNC, NEAR, FAR) for _ in range(B)]
    g = GuardedState(B, L, dev)
    for depth, rgb, poses in frames:
        fr = Frame(dev, depth, rgb, cam, poses)
        fr.into(g, VOXEL, TRUNC, NEAR, FAR)
        fr.check()
        for s in range(B):
            vols[s].frame(depth[s], rgb[s], cam["f"][s], cam["c"][s], poses[s])
    g.check()
    mark = (1 << L) - (1 << (L - 2))
    for s, vol in enumerate(vols):
        assert 500 < len(vol.records) < mark, "the table stays below the 3/4 mark"
        assert records(g.state, s) == ref_records(vol)
    truth = np.stack([T.render_plane(render[s], cam["f"][s], cam["c"][s], H, W, T.PLANE_NORMAL, T.PLANE_OFFSET) for s in range(B)])
    guide = truth.copy()                                        # the guide: the analytic depth with holes of every kind
    guide[:, 3:6, 4:9] = np.nan
    guide[:, 10, :] = np.inf
    guide[:, 15:17, 20:] = F(0.5)                               # below near
    guide[:, 20:, :6] = F(25.0)                                 # beyond far
    guide[0, 12, 12] = np.nextafter(F(NEAR), F(0))
    return {"cam": cam, "g": g, "vols": vols, "render": render, "guide": guide, "ref": {}}


def reference(plane, min_frames, window, pose=None):
    """(depth [B,H,W], hits [B]) of the restatement, computed once per case."""
    key = (min_frames, window, None if pose is None else np.asarray(pose).tobytes())
    if key not in plane["ref"]:
        cam, poses = plane["cam"], plane["render"] if pose is None else pose
        out = [RC.raycast(plane["vols"][s].records, cam["f"][s], cam["c"][s], poses[s], H, W, VOXEL, TRUNC, min_frames, NEAR, FAR,
                          guide=plane["guide"][s] if window else None, window=window) for s in range(B)]
        plane["ref"][key] = (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int64))
    return plane["ref"][key]


class Launch:
    """The inputs of one raycast between guards; ``out`` a [B,H,W,1] slice at batch stride ``out_stride`` of a guarded buffer."""

    def __init__(self, dev, plane, poses=None, fill=None, fill_stride=None, out_stride=None, hits0=None):
        cam = plane["cam"]
        poses = plane["render"] if poses is None else poses
        self.f, self.c = Guarded(dev, (B, 2), torch.float32, cam["f"]), Guarded(dev, (B, 2), torch.float32, cam["c"])
        self.pose = Guarded(dev, (B, 7), torch.float64, np.asarray(poses, np.float64))
        self.guide = Guarded(dev, (B, H, W, 1), torch.float32, plane["guide"][..., None])
        image = H * W
        out_stride = image if out_stride is None else out_stride
        self.out_buf = Guarded(dev, (B * out_stride,), torch.float32)
        self.out = self.out_buf.t.as_strided((B, H, W, 1), (out_stride, W, 1, 1))
        self.fill = self.fill_buf = None
        if fill is not None:
            fill_stride = image if fill_stride is None else fill_stride
            host = np.zeros((B, fill_stride), F)
            host[:, :image] = fill.reshape(B, image)
            self.fill_buf = Guarded(dev, (B * fill_stride,), torch.float32, host.reshape(-1))
            self.fill = self.fill_buf.t.as_strided((B, H, W, 1), (fill_stride, W, 1, 1))
        self.hits = Guarded(dev, (B,), torch.int64, np.zeros(B, np.int64) if hits0 is None else np.asarray(hits0, np.int64))
        self.bufs = [x for x in (self.f, self.c, self.pose, self.guide, self.out_buf, self.fill_buf, self.hits) if x is not None]

    def run(self, state, min_frames, window):
        from m4depth_amd import network_ops as nops
        got = nops.tsdf_raycast(state, self.f.t, self.c.t, self.pose.t, H, W, VOXEL, TRUNC, min_frames, near=NEAR, far=FAR,
                                guide=self.guide.t if window else None, window=window, fill=self.fill, out=self.out,
                                hits=self.hits.t)
        assert got is self.out
        for x in self.bufs:
            x.check()
        return npy(self.out)[..., 0], npy(self.hits.t)


@pytest.mark.parametrize("min_frames", [1, 2])
@pytest.mark.parametrize("window", [None, 1, 2])
def test_plane_equals_the_restatement(dev, plane, min_frames, window):
    """24 x 32 pixels: two 16-pixel tile rows and columns per sample, batch 2, per-sample off-centre cameras and poses."""
    want, want_hits = reference(plane, min_frames, window)
    assert (want_hits > 100).all() and np.isnan(want).any(), "surface and misses in every sample"
    before = npy(plane["g"].t).copy()
    got, hits = Launch(dev, plane).run(plane["g"].state, min_frames, window)
    assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:5]
    assert np.array_equal(hits, want_hits)
    plane["g"].check()
    assert np.array_equal(npy(plane["g"].t), before), "the launch only reads the state"


def test_windowed_march_differs_from_the_whole_range_only_where_the_guide_says(plane):
    """What the guide's holes are there for (on the restatement: the device equals it above)."""
    whole, _ = reference(plane, 1, None)
    near_guide, _ = reference(plane, 1, 1)
    unguided = ~(np.isfinite(plane["guide"]) & (plane["guide"] >= F(NEAR)) & (plane["guide"] <= F(FAR)))
    assert np.array_equal(bits(whole)[unguided], bits(near_guide)[unguided]) and np.isfinite(whole[unguided]).any()
    assert (bits(whole) != bits(near_guide)).any(), "a window starts its half-voxel positions elsewhere"


def test_a_sample_with_a_nan_pose_is_all_misses(dev, plane):
    poses = plane["render"].copy()
    poses[0, 2] = np.nan
    want, want_hits = reference(plane, 1, None)
    fill = np.random.default_rng(8).random((B, H, W)).astype(F) + F(2.0)
    got, hits = Launch(dev, plane, poses=poses).run(plane["g"].state, 1, None)
    assert (bits(got[0]) == 0x7FC00000).all() and np.array_equal(bits(got[1]), bits(want[1]))
    assert hits.tolist() == [0, int(want_hits[1])]
    got, hits = Launch(dev, plane, poses=poses, fill=fill).run(plane["g"].state, 1, None)
    assert np.array_equal(bits(got[0]), bits(fill[0])) and hits[0] == 0


def test_fill_strides_and_counters(dev, plane):
    """Misses take the fill's bits at a batch stride larger than an image, the output lies at a stride of its own between guards
    and inside its buffer's slack, and the hit counts add to what the words held."""
    want, want_hits = reference(plane, 2, None)
    rng = np.random.default_rng(9)
    fill = (rng.random((B, H, W)) + 2.0).astype(F)
    fill[:, 0, :5] = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40], F)          # bits, not values
    run = Launch(dev, plane, fill=fill, fill_stride=H * W + 37, out_stride=H * W + 101, hits0=[7, 1 << 40])
    got, hits = run.run(plane["g"].state, 2, None)
    miss = np.isnan(want)
    assert np.array_equal(bits(got)[miss], bits(fill)[miss]) and np.array_equal(bits(got)[~miss], bits(want)[~miss])
    assert hits.tolist() == [7 + int(want_hits[0]), (1 << 40) + int(want_hits[1])]
    slack = npy(run.out_buf.t).reshape(B, -1)[:, H * W:]
    assert (slack.view(np.uint8) == 0x5A).all(), "the elements between the images of the output stay as they were"
    # in place: the output is the fill
    from m4depth_amd import network_ops as nops
    buf = Guarded(dev, (B, H, W, 1), torch.float32, fill[..., None])
    nops.tsdf_raycast(plane["g"].state, run.f.t, run.c.t, run.pose.t, H, W, VOXEL, TRUNC, 2, near=NEAR, far=FAR, fill=buf.t, out=buf.t)
    buf.check()
    assert np.array_equal(bits(npy(buf.t)[..., 0]), bits(got))


def test_capturable(dev, plane):
    from m4depth_amd import network_ops as nops
    run = Launch(dev, plane)
    eager, eager_hits = run.run(plane["g"].state, 1, 2)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        nops.tsdf_raycast(plane["g"].state, run.f.t, run.c.t, run.pose.t, H, W, VOXEL, TRUNC, 1, near=NEAR, far=FAR,
                          guide=run.guide.t, window=2, out=run.out, hits=run.hits.t)
    run.out_buf.t.zero_()
    run.hits.t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(npy(run.out)[..., 0]), bits(eager)) and np.array_equal(npy(run.hits.t), eager_hits)
    for x in run.bufs:
        x.check()


def test_sphere_equals_the_restatement(dev):
    """48 x 48 pixels (nine tiles), batch 1, 26 frames, L = 14; a fused and a novel view."""
    from m4depth_amd import network_ops as nops
    from test_tsdf_raycast_ref import NOVEL_SPHERE_EYE
    S = T.SPHERE
    frames = T.sphere_frames()
    vol = T.fuse(frames, S["f"], S["c"], S["voxel"], S["trunc"], S["near"], S["far"])
    cam = {"f": np.array([S["f"]], F), "c": np.array([S["c"]], F)}
    g = GuardedState(1, 14, dev)
    for depth, rgb, pose in frames:
        Frame(dev, depth[None], rgb[None], cam, pose[None]).into(g, S["voxel"], S["trunc"], S["near"], S["far"])
    assert records(g.state, 0) == ref_records(vol)
    f, c = torch.from_numpy(cam["f"]).to(dev), torch.from_numpy(cam["c"]).to(dev)
    for pose in (frames[0][2], T.look_at_pose(NOVEL_SPHERE_EYE)):
        want, want_hits = RC.raycast(vol.records, S["f"], S["c"], pose, S["h"], S["w"], S["voxel"], S["trunc"], 2, S["near"], S["far"])
        out = Guarded(dev, (1, S["h"], S["w"], 1), torch.float32)
        hits = torch.zeros(1, dtype=torch.int64, device=dev)
        nops.tsdf_raycast(g.state, f, c, torch.from_numpy(pose[None].copy()).to(dev), S["h"], S["w"], S["voxel"], S["trunc"], 2,
                          near=S["near"], far=S["far"], out=out.t, hits=hits)
        out.check()
        g.check()
        assert want_hits > 900 and np.array_equal(bits(npy(out.t)[0, ..., 0]), bits(want)) and int(hits[0]) == want_hits


def test_refusals(dev, plane):
    """Every refusal of the header's list: the op raises, the raw entry returns 1 -- on device pointers, without a launch."""
    from m4depth_amd import network_ops as nops
    from m4depth_amd._lib import lib
    run = Launch(dev, plane, fill=np.ones((B, H, W), F))
    st = plane["g"].state
    ok = dict(h=H, w=W, voxel=VOXEL, trunc=TRUNC, min_frames=1, near=NEAR, far=FAR, out=run.out)
    for kw in (dict(voxel=0.0), dict(voxel=float("inf")), dict(voxel=float("nan")), dict(trunc=1), dict(trunc=9), dict(min_frames=0),
               dict(h=0), dict(w=0), dict(far=NEAR), dict(far=float("nan")), dict(near=0.0), dict(near=-1.0), dict(near=float("nan")),
               dict(voxel=1e-5), dict(window=1), dict(guide=run.guide.t), dict(guide=run.guide.t, window=0),
               dict(guide=run.guide.t[:, :-1], window=1), dict(fill=run.fill[:, :, :-1]), dict(out=run.out[:1]),
               dict(hits=torch.zeros(B + 1, dtype=torch.int64, device=dev)), dict(out=run.out.transpose(1, 2))):
        with pytest.raises(ValueError):
            nops.tsdf_raycast(st, run.f.t, run.c.t, run.pose.t, **dict(ok, **kw))
    with pytest.raises(TypeError):
        nops.tsdf_raycast(st, run.f.t, run.c.t, run.pose.t, **dict(ok, hits=torch.zeros(B, dtype=torch.int32, device=dev)))
    with pytest.raises(ValueError, match="not a tsdf_state"):
        nops.tsdf_raycast(dict(st, slots_log2=L + 1), run.f.t, run.c.t, run.pose.t, **ok)
    p = dict(state=st["words"].data_ptr(), b=B, L=L, f=run.f.t.data_ptr(), c=run.c.t.data_ptr(), pose=run.pose.t.data_ptr(), h=H, w=W,
             near=NEAR, far=FAR, voxel=VOXEL, trunc=TRUNC, min_frames=1, guide=None, gs=0, window=0, fill=None, fs=0,
             out=run.out.data_ptr(), os=H * W, hits=None)

    def raw(**kw):
        a = dict(p, **kw)
        return lib.m4d_tsdf_raycast(a["state"], a["b"], a["L"], a["f"], a["c"], a["pose"], a["h"], a["w"], a["near"], a["far"],
                                    a["voxel"], a["trunc"], a["min_frames"], a["guide"], a["gs"], a["window"], a["fill"], a["fs"],
                                    a["out"], a["os"], a["hits"], None)

    n0 = lib.m4d_launch_count()
    gd, fl, hp = run.guide.t.data_ptr(), run.fill.data_ptr(), run.hits.t.data_ptr()
    for kw in (dict(state=None), dict(f=None), dict(c=None), dict(pose=None), dict(out=None), dict(b=0), dict(b=65536), dict(L=5),
               dict(L=27), dict(h=0), dict(w=0), dict(h=4097, w=4097, os=1 << 25), dict(far=NEAR), dict(far=float("nan")),
               dict(near=float("nan")), dict(near=0.0), dict(near=-1.0), dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=float("nan")),
               dict(voxel=float("inf")), dict(trunc=1), dict(trunc=9), dict(min_frames=0), dict(guide=gd, gs=H * W, window=0),
               dict(voxel=1e-5), dict(os=H * W - 1), dict(guide=gd, gs=H * W - 1, window=1), dict(fill=fl, fs=H * W - 1),
               dict(f=p["f"] + 2), dict(c=p["c"] + 2), dict(out=p["out"] + 2), dict(guide=gd + 2, gs=H * W, window=1),
               dict(fill=fl + 2, fs=H * W), dict(state=p["state"] + 4), dict(pose=p["pose"] + 4), dict(hits=hp + 4)):
        assert raw(**kw) == 1, kw
    assert lib.m4d_launch_count() == n0
    for x in run.bufs:
        x.check()


# ---- fusion.FusedDepth -----------------------------------------------------------------------------------------------------------
def _motion(prev, cur):
    """The float32 frame-to-frame motion (rot [4], trans [3]) that takes the camera-to-world pose ``prev`` to ``cur``."""
    from pose_ref import rot
    a, b = np.asarray(prev, np.float64), np.asarray(cur, np.float64)
    aw, ax, ay, az = a[0], -a[1], -a[2], -a[3]
    bw, bx, by, bz = b[:4]
    q = np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                  aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])
    R = np.array(rot(a), np.float64)
    return q.astype(F), (R.T @ (b[4:] - a[4:])).astype(F)


def test_fused_depth_steps_equal_the_restatement(dev):
    """Three plane frames as estimates through FusedDepth.step at batch 2, then a frame at which sample 1 restarts (device mask):
    every step equals clear + fuse + raycast of the restatement at the pose chain the device keeps (m4d_pose_accumulate has tests
    of its own), sample 1 has a volume of its own from its reset on and sample 0 is unaffected by it."""
    from m4depth_amd.fusion import FusedDepth
    cam = cameras_np(B, H, W)
    chain = T.plane_poses(4)
    order = [(0, 0), (1, 2), (2, 3), (3, 1)]                                      # (pose of sample 0, of sample 1) per step
    fd = FusedDepth(VOXEL, trunc=TRUNC, min_frames=1, slots_log2=L, near=NEAR, far=FAR, window=None)
    fdw = FusedDepth(VOXEL, trunc=TRUNC, min_frames=2, slots_log2=L, near=NEAR, far=FAR, window=2)
    vols = [T.TsdfVolume(VOXEL, TRUNC, NEAR, FAR) for _ in range(B)]
    f, c = torch.from_numpy(cam["f"]).to(dev), torch.from_numpy(cam["c"]).to(dev)
    hits = torch.zeros((len(order), B), dtype=torch.int64, device=dev)
    hits_w = torch.zeros_like(hits)
    rng = np.random.default_rng(12)
    ident = np.array([1, 0, 0, 0, 0, 0, 0], np.float64)
    prev = [ident, ident]
    for k, ps in enumerate(order):
        reset = np.array([k == 0, k == 0 or k == 3], np.uint8)
        cur = [ident if reset[s] else chain[ps[s]] for s in range(B)]
        motion = [_motion(prev[s], cur[s]) for s in range(B)]
        prev = cur
        est = np.stack([T.render_plane(cur[s], cam["f"][s], cam["c"][s], H, W, T.PLANE_NORMAL, T.PLANE_OFFSET) for s in range(B)])
        est[:, 2, 3] = np.nan
        rgb = rng.random((B, H, W, 3)).astype(F)
        args = (torch.from_numpy(est[..., None]).to(dev), torch.from_numpy(rgb).to(dev),
                torch.from_numpy(np.stack([m[0] for m in motion])).to(dev), torch.from_numpy(np.stack([m[1] for m in motion])).to(dev),
                {"f": f, "c": c}, torch.from_numpy(reset).to(dev))
        got = npy(fd.step(*args, hits=hits[k]))[..., 0]
        got_w = npy(fdw.step(*args, hits=hits_w[k]))[..., 0]
        poses = npy(fd.pose)
        assert np.array_equal(poses, npy(fdw.pose)) and np.abs(poses - np.stack(cur)).max() < 1e-6
        before_reset = len(vols[1].records)
        for s in range(B):
            if reset[s]:
                vols[s] = T.TsdfVolume(VOXEL, TRUNC, NEAR, FAR)
                assert np.array_equal(poses[s], ident)
            vols[s].frame(est[s], rgb[s], cam["f"][s], cam["c"][s], poses[s])
            for g, h_log, m, win in ((got, hits, 1, None), (got_w, hits_w, 2, 2)):
                want, n = RC.raycast(vols[s].records, cam["f"][s], cam["c"][s], poses[s], H, W, VOXEL, TRUNC, m, NEAR, FAR,
                                     guide=est[s] if win else None, window=win, fill=est[s])
                assert np.array_equal(bits(g[s]), bits(want)), (k, s, m)
                assert int(h_log[k, s]) == n and (n > 300 or m == 2 and (k == 0 or reset[s])), (k, s, m, n)
    stats = fd.stats()
    assert [st["occupied"] for st in stats] == [len(v.records) for v in vols] and all(st["dropped_full"] == 0 for st in stats)
    assert len(vols[1].records) < before_reset, "sample 1 holds one frame since its reset"
    with pytest.raises(ValueError, match="device mask"):
        fd.step(*args[:5], np.zeros(B, np.uint8))


# ---- the driver ------------------------------------------------------------------------------------------------------------------
LENGTHS = [5, 3, 6, 1]
SIZE = 64
ARCH = ["--arch_depth", "4", "--height", str(SIZE), "--width", str(SIZE)]
FUSED = ["--fused", "0.5", "--fused_slots_log2", "20"]


@pytest.fixture(scope="module")
def midair_set(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("fused_eval"))
    db, rec = make_fake_dataset(root, "midair", n_traj=len(LENGTHS), n_frames=max(LENGTHS), size=(SIZE, SIZE), seed=29)
    for t, n in enumerate(LENGTHS):
        path = os.path.join(rec, f"set_{t}", f"traj_{t:04d}.csv")
        lines = open(path).read().splitlines()
        with open(path, "w") as fh:
            fh.write("\n".join(lines[:1 + n]) + "\n")
    cfg = os.path.join(root, "datasets_location.json")
    with open(cfg, "w") as fh:
        json.dump({"midair": db}, fh)
    return cfg, rec, root


_runs = {}


def _eval(dataset_set, *extra, where=False):
    """One main.py --mode=eval run (cached per flag set): ({file name: bytes} of its ckpt_dir, what it printed), or with
    ``where`` the ckpt_dir."""
    from m4depth_amd import main as MAIN
    if extra not in _runs:
        cfg, rec, root = dataset_set
        ck = os.path.join(root, "ckpt_" + str(len(_runs)))
        argv = ["--mode", "eval", "--dataset", "midair", "--db_path_config", cfg, "--records_path", rec, "--ckpt_dir", ck]
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            assert MAIN.main(argv + ARCH + list(extra)) == 0
        _runs[extra] = ({n: open(os.path.join(ck, n), "rb").read() for n in sorted(os.listdir(ck)) if n.endswith(".txt")},
                        out.getvalue(), ck)
    return _runs[extra][2] if where else _runs[extra][:2]


def test_driver_scores_the_fused_depth_beside_the_raw(dev, midair_set):
    from m4depth_amd import fusion as FU
    plain, _ = _eval(midair_set, "--eval_streams", "3")
    fused, said = _eval(midair_set, "--eval_streams", "3", *FUSED)
    assert set(plain) == {"perfs-midair.txt"} and set(fused) == {"perfs-midair.txt", "perfs-fused-midair.txt", "fused-frames-midair.txt"}
    assert fused["perfs-midair.txt"] == plain["perfs-midair.txt"], "the raw metrics are what they are without the flag"
    ck = _eval(midair_set, "--eval_streams", "3", *FUSED, where=True)
    means = FU.read_perfs(FU.perfs_path(ck, "midair"))
    frames = FU.read_frames(FU.frames_path(ck, "midair"))
    assert means.shape == (7,) and np.isfinite(means).all()
    assert [(t, f) for t, f, _ in frames] == [(t, f) for t, n in enumerate(LENGTHS) for f in range(1, n)]
    rows = np.stack([r for _, _, r in frames])
    assert np.isfinite(rows).all() and (rows[:, 0] >= 0).all() and (rows[:, 0] <= 1).all()
    raw = np.loadtxt(os.path.join(ck, "perfs-midair.txt")).astype(F)
    assert abs(rows[:, 1].astype(np.float64).mean() - raw[0]) < 1e-5 * raw[0] and abs(rows[:, 2].astype(np.float64).mean() - means[0]) < 1e-5 * means[0]
    assert "fused depth at 0.5 m (K 4, min_frames 2, whole range)" in said and " 0 samples dropped by full tables" in said


def test_driver_schedule_and_graph_independence(dev, midair_set):
    base, _ = _eval(midair_set, "--eval_streams", "3", *FUSED)
    for extra in (("--eval_streams_policy", "arrival"), ("--graph",)):
        other, _ = _eval(midair_set, "--eval_streams", "3", *FUSED, *extra)
        assert other == base, extra


def test_driver_windowed_and_companions(dev, midair_set):
    got, said = _eval(midair_set, "--eval_streams", "3", "--fused", "0.5", "--fused_slots_log2", "20", "--fused_window", "1",
                      "--fused_trunc", "2", "--fused_min_frames", "1")
    base, _ = _eval(midair_set, "--eval_streams", "3")
    assert got["perfs-midair.txt"] == base["perfs-midair.txt"] and "(K 2, min_frames 1, window 1)" in said


# ---- predict: export.PredictionWriter(save_fused=True), main.py --save_fused ---------------------------------------------------------
def _kitti16(d):
    """m4d_depth_export's kitti16 of a float32 map: rint(d * 256) clamped to 1..65535, 0 for a depth that is not finite and > 0."""
    d = np.asarray(d, F)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(d) & (d > 0)
        return np.where(valid, np.clip(np.rint(np.where(valid, d, F(1)) * F(256.0)), 1, 65535), 0).astype(np.uint16)


@pytest.mark.parametrize("window", [None, 2])
def test_prediction_writer_fused(dev, tmp_path, window):
    """Every <frame>_fused.png is the restatement's rendering of the trajectory's volume right after the frame went in, encoded
    as the estimate is; every other file is what the writer writes without the option."""
    from PIL import Image
    from test_gpu_tsdf_mesh import _writer_run
    voxel, trunc, near, far = 0.5, 3, 2.0, 40.0
    mesh = dict(save_mesh=voxel, mesh_trunc=trunc, mesh_min_frames=2, mesh_slots_log2=14)
    with_fused, without = str(tmp_path / "fused"), str(tmp_path / "plain")
    writer, cam, seen = _writer_run(dev, with_fused, 0, save_fused=True, fused_window=window, **mesh)
    _writer_run(dev, without, 0, **mesh)
    vols, traj, count, rendered = {}, [-1, -1], {}, 0
    for depth, rgb, pose, flags in seen:
        for s in range(2):
            if flags[s]:
                traj[s] += 1
                vols[s] = T.TsdfVolume(voxel, trunc, near, far)
            d = f"s{s:02d}_t{traj[s]:04d}"
            vols[s].frame(depth[s], rgb[s], cam["f"][s], cam["c"][s], pose[s])
            h, w = depth[s].shape
            want, hits = RC.raycast(vols[s].records, cam["f"][s], cam["c"][s], pose[s], h, w, voxel, trunc, 2, near, far,
                                    guide=depth[s] if window else None, window=window)
            k = count[d] = count.get(d, -1) + 1
            got = np.asarray(Image.open(os.path.join(with_fused, d, f"{k:06d}_fused.png")))
            assert got.dtype == np.uint16 and np.array_equal(got, _kitti16(want)), (d, k)
            assert (got == 0).sum() == h * w - hits
            rendered += hits
    assert rendered > 2000 and (writer.fused_pixels, writer.fused_cap) == (rendered, 14 * 24 * 40)
    for d in sorted(os.listdir(without)):
        files = sorted(os.listdir(os.path.join(without, d)))
        assert sorted(files + [f"{k:06d}_fused.png" for k in range(count[d] + 1)]) == sorted(os.listdir(os.path.join(with_fused, d)))
        for name in files:
            with open(os.path.join(without, d, name), "rb") as a, open(os.path.join(with_fused, d, name), "rb") as b2:
                assert a.read() == b2.read(), (d, name)


def test_driver_predict_writes_fused_maps(dev, tmp_path):
    """main.py --mode=predict --save_mesh --save_fused on the streaming and the graphed path: the same files, a <frame>_fused.png
    beside every <frame>_depth.png, the closing line's share."""
    from PIL import Image
    from m4depth_amd import main as MAIN
    root = str(tmp_path)
    db, rec = make_fake_dataset(root, "midair", n_traj=1, n_frames=5)                      # 48 x 64
    cfg = os.path.join(root, "datasets_location.json")
    with open(cfg, "w") as fh:
        json.dump({"midair": "./db"}, fh)
    outs = []
    for extra in (["--stream"], ["--stream", "--graph"]):
        out = os.path.join(root, "out%d" % len(outs))
        printed = io.StringIO()
        with contextlib.redirect_stdout(printed):
            assert MAIN.main(["--mode", "predict", "--dataset", "midair", "--db_path_config", cfg, "--records_path", rec,
                              "--arch_depth", "2", "--height", "48", "--width", "64", "--ckpt_dir", out + "_ckpt", "--save_dir", out,
                              "--save_range", "0.01", "1000", "--save_mesh", "2.0", "--mesh_min_frames", "1", "--mesh_slots_log2", "18",
                              "--save_fused"] + extra) == 0
        assert "fused depth rendered on" in printed.getvalue()
        outs.append(out)
    names = sorted(os.listdir(os.path.join(outs[0], "s00_t0000")))
    assert names == sorted([f"{k:06d}_{kind}.png" for k in range(5) for kind in ("depth", "fused")] + ["mesh.ply"])
    for name in names:
        with open(os.path.join(outs[0], "s00_t0000", name), "rb") as a, open(os.path.join(outs[1], "s00_t0000", name), "rb") as b2:
            assert a.read() == b2.read(), name
    im = np.asarray(Image.open(os.path.join(outs[0], "s00_t0000", "000004_fused.png")))
    assert im.dtype == np.uint16 and im.shape == (48, 64)
