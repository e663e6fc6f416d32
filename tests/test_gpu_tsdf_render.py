"""m4d_tsdf_render on the GPU (network_ops.tsdf_render, fusion.FusedDepth(interp=...), main.py --fused_interp / --save_fused_view)
against the numpy restatement tests/tsdf_render_ref.py, bit for bit: depth, normal, colour, view, NaN positions and hit counts.
Every quantity is a fixed sequence of float32 / float64 operations rounded once each on a state that is only read, so there is no
tolerance anywhere; what the restatement itself is worth is measured in tests/test_tsdf_render_ref.py.  The volumes are built on
the device with network_ops.tsdf_integrate (held to tsdf_mesh_ref.TsdfVolume by tests/test_gpu_tsdf_mesh.py) and in the
restatement from the same frames.  Every buffer the launch reads or writes lies between sentinel guards, every output at a batch
stride with slack behind each image."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

from helpers import F, npy, cameras_np, make_fake_dataset
import tsdf_mesh_ref as T
import tsdf_render_ref as RR
from test_gpu_tsdf_mesh import Guarded, GuardedState, Frame, records, ref_records, SENTINEL
from test_tsdf_render_ref import NOVEL_SPHERE_EYE, LINEAR, column_case

pytestmark = pytest.mark.gpu

B, H, W, L = 3, T.PLANE["h"], T.PLANE["w"], 14                                  # 24 rows: one and a half 16-row tiles
VOXEL, TRUNC, NEAR, FAR = T.PLANE["voxel"], T.PLANE["trunc"], 1.0, 20.0
INTERPS = ("nearest", "trilinear")
OUTPUTS = ("depth", "normal", "colour", "view")


def bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.uint8 else a.astype(F, copy=False).view(np.uint32)


def _plane_inputs():
    """Four frames for three samples with their own off-centre cameras and their own order of the poses.  The render poses:
    sample 0 a fused one, sample 1 a novel one, sample 2 one that holds a NaN."""
    cam = cameras_np(B, H, W)
    poses = T.plane_poses(6)
    rng = np.random.default_rng(5)
    frames = []
    for k in range(4):
        ps = [poses[k], poses[(2, 0, 3, 1)[k]], poses[(1, 3, 0, 2)[k]]]
        depth = np.stack([T.render_plane(ps[s], cam["f"][s], cam["c"][s], H, W, T.PLANE_NORMAL, T.PLANE_OFFSET) for s in range(B)])
        frames.append((depth, rng.random((B, H, W, 3)).astype(F), np.stack(ps)))
    broken = poses[4].copy()
    broken[2] = np.nan
    return cam, frames, np.stack([poses[3], poses[5], broken])


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
    for s, vol in enumerate(vols):
        assert 500 < len(vol.records) < (1 << L) - (1 << (L - 2)), "the table stays below the 3/4 mark"
        assert records(g.state, s) == ref_records(vol)
    truth = np.stack([T.render_plane(render[min(s, 1)], cam["f"][s], cam["c"][s], H, W, T.PLANE_NORMAL, T.PLANE_OFFSET) for s in range(B)])
    guide = truth.copy()                                        # the guide: the analytic depth with holes of every kind
    guide[:, 3:6, 4:9] = np.nan
    guide[:, 10, :] = np.inf
    guide[:, 15:17, 20:] = F(0.5)                               # below near
    guide[:, 20:, :6] = F(25.0)                                 # beyond far
    fill = (np.random.default_rng(9).random((B, H, W)) + 2.0).astype(F)
    fill[:, 0, :5] = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40], F)          # bits, not values
    return {"cam": cam, "g": g, "vols": vols, "render": render, "guide": guide, "fill": fill, "ref": {}}


def reference(plane, min_frames, window, interp, fill):
    """The restatement's outputs stacked over the samples ({name: [B,...]}, hits [B], hit [B,H,W]), computed once per case."""
    key = (min_frames, window, interp, fill)
    if key not in plane["ref"]:
        cam = plane["cam"]
        out = [RR.render(plane["vols"][s].records, cam["f"][s], cam["c"][s], plane["render"][s], H, W, VOXEL, TRUNC, min_frames, NEAR,
                         FAR, guide=plane["guide"][s] if window else None, window=window, fill=plane["fill"][s] if fill else None,
                         interp=RR.INTERP[interp]) for s in range(B)]
        plane["ref"][key] = ({k: np.stack([o[k] for o in out]) for k in OUTPUTS}, np.array([o["hits"] for o in out], np.int64),
                             np.stack([o["hit"] for o in out]))
    return plane["ref"][key]


class Launch:
    """The inputs and outputs of one render between guards; every image tensor a [B,H,W,c] view at a batch stride of its own
    with slack behind each image."""

    PAD = {"guide": 13, "fill": 37, "depth": 101, "normal": 7, "colour": 50, "view": 29}

    def __init__(self, dev, plane, fill=True, outputs=OUTPUTS[1:], hits0=None):
        cam = plane["cam"]
        self.f, self.c = Guarded(dev, (B, 2), torch.float32, cam["f"]), Guarded(dev, (B, 2), torch.float32, cam["c"])
        self.pose = Guarded(dev, (B, 7), torch.float64, np.asarray(plane["render"], np.float64))
        self.hits = Guarded(dev, (B,), torch.int64, np.zeros(B, np.int64) if hits0 is None else np.asarray(hits0, np.int64))
        self.bufs, self.views = [self.f, self.c, self.pose, self.hits], {}
        for name, c, dtype, host in (("guide", 1, torch.float32, plane["guide"]), ("fill", 1, torch.float32, plane["fill"] if fill else None),
                                     ("depth", 1, torch.float32, None), ("normal", 3, torch.float32, None),
                                     ("colour", 3, torch.float32, None), ("view", 3, torch.uint8, None)):
            if (name == "fill" and not fill) or (name in OUTPUTS[1:] and name not in outputs):
                self.views[name] = None
                continue
            image, stride = H * W * c, H * W * c + self.PAD[name]
            init = None
            if host is not None:
                init = np.full((B, stride), F(-7.0), F)
                init[:, :image] = host.reshape(B, image)
            buf = Guarded(dev, (B * stride,), dtype, None if init is None else init.reshape(-1))
            self.bufs.append(buf)
            self.views[name] = buf.t.as_strided((B, H, W, c), (stride, W * c, c, 1))
            setattr(self, name + "_buf", buf)

    def run(self, state, min_frames, window, interp):
        from m4depth_amd import network_ops as nops
        v = self.views
        got = nops.tsdf_render(state, self.f.t, self.c.t, self.pose.t, H, W, VOXEL, TRUNC, min_frames, near=NEAR, far=FAR,
                               guide=v["guide"] if window else None, window=window, fill=v["fill"], interp=interp, out=v["depth"],
                               normal=v["normal"], colour=v["colour"], view=v["view"], hits=self.hits.t)
        assert got is v["depth"]
        return self.results()

    def results(self):
        """({name: the output as numpy [B,H,W,c]}, hits); holds the guards and the slack behind every output image."""
        for x in self.bufs:
            x.check()
        out = {}
        for name in OUTPUTS:
            if self.views[name] is None:
                continue
            out[name] = npy(self.views[name])
            c = out[name].shape[-1]
            slack = npy(getattr(self, name + "_buf").t).reshape(B, -1)[:, H * W * c:]
            assert (slack.view(np.uint8) == SENTINEL).all(), f"{name}: the elements between the images stay as they were"
        out["depth"] = out["depth"][..., 0]
        return out, npy(self.hits.t)


def assert_equal(got, want, what):
    for name in OUTPUTS:
        if name in got:
            diff = np.argwhere(bits(got[name]) != bits(want[name]))
            assert not len(diff), (what, name, len(diff), diff[:5].tolist())


@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("min_frames", [1, 2])
@pytest.mark.parametrize("window", [None, 1, 2])
def test_plane_equals_the_restatement(dev, plane, min_frames, window, interp):
    """24 x 32 pixels: two 16-pixel tile rows (the second half empty) and columns per sample; two samples with cameras and
    poses of their own, a third whose pose holds a NaN.  With a fill and every output at a padded stride; then without a fill
    and with no optional output: the same depth."""
    want, want_hits, hit = reference(plane, min_frames, window, interp, True)
    assert (want_hits[:2] > 100).all() and want_hits[2] == 0 and not hit[:2].all(), "surface and misses in both rendered samples"
    assert np.isfinite(want["normal"]).any() and np.isfinite(want["colour"]).any() and want["view"].any()
    before = npy(plane["g"].t).copy()
    got, hits = Launch(dev, plane, hits0=[7, 1 << 40, 3]).run(plane["g"].state, min_frames, window, interp)
    assert_equal(got, want, (min_frames, window, interp))
    assert hits.tolist() == [7 + int(want_hits[0]), (1 << 40) + int(want_hits[1]), 3]
    assert np.array_equal(bits(got["depth"][2]), bits(plane["fill"][2])) and (bits(got["normal"][2]) == 0x7FC00000).all()
    assert (bits(got["colour"][2]) == 0x7FC00000).all() and not got["view"][2].any()
    bare, hits = Launch(dev, plane, fill=False, outputs=()).run(plane["g"].state, min_frames, window, interp)
    assert np.array_equal(bits(bare["depth"])[hit], bits(want["depth"])[hit]) and (bits(bare["depth"])[~hit] == 0x7FC00000).all()
    assert np.array_equal(hits, want_hits)
    plane["g"].check()
    assert np.array_equal(npy(plane["g"].t), before), "the launch only reads the state"


def test_trilinear_differs_from_nearest(plane):
    """On the restatement (the device equals it above): the two rules hit nearly the same pixels at other depths."""
    near, _, hit_n = reference(plane, 1, None, "nearest", True)
    tri, _, hit_t = reference(plane, 1, None, "trilinear", True)
    both = hit_n & hit_t
    # a pixel next to unknown space falls back to the nearest rule and keeps its depth; one with all eight voxels around its
    # samples does not -- those are the pixels that have a normal, at least 0.75 of the hits (tests/test_tsdf_render_ref.py)
    assert both.sum() > 0.95 * hit_n.sum() and (bits(near["depth"])[both] != bits(tri["depth"])[both]).mean() > 0.75


@pytest.mark.parametrize("window", [None, 2])
def test_nearest_equals_tsdf_raycast(dev, plane, window):
    from m4depth_amd import network_ops as nops
    run = Launch(dev, plane, hits0=[0, 0, 0])
    got, hits = run.run(plane["g"].state, 2, window, "nearest")
    out = Guarded(dev, (B, H, W, 1), torch.float32)
    hits_r = torch.zeros(B, dtype=torch.int64, device=dev)
    nops.tsdf_raycast(plane["g"].state, run.f.t, run.c.t, run.pose.t, H, W, VOXEL, TRUNC, 2, near=NEAR, far=FAR,
                      guide=run.views["guide"] if window else None, window=window, fill=run.views["fill"], out=out.t, hits=hits_r)
    out.check()
    assert np.array_equal(bits(npy(out.t)[..., 0]), bits(got["depth"])) and np.array_equal(npy(hits_r), hits) and hits[:2].min() > 100


@pytest.mark.parametrize("interp", INTERPS)
def test_depth_may_alias_the_fill(dev, plane, interp):
    from m4depth_amd import network_ops as nops
    want, want_hits, _ = reference(plane, 2, None, interp, True)
    run = Launch(dev, plane)
    buf = Guarded(dev, (B, H, W, 1), torch.float32, plane["fill"][..., None])
    nops.tsdf_render(plane["g"].state, run.f.t, run.c.t, run.pose.t, H, W, VOXEL, TRUNC, 2, near=NEAR, far=FAR, fill=buf.t, out=buf.t,
                     interp=interp, view=run.views["view"])
    buf.check()
    assert np.array_equal(bits(npy(buf.t)[..., 0]), bits(want["depth"]))
    assert np.array_equal(npy(run.views["view"]), want["view"])


def test_capturable(dev, plane):
    from m4depth_amd import network_ops as nops
    run = Launch(dev, plane, hits0=[0, 0, 0])
    eager, eager_hits = run.run(plane["g"].state, 1, 2, "trilinear")
    torch.cuda.synchronize()
    v = run.views
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        nops.tsdf_render(plane["g"].state, run.f.t, run.c.t, run.pose.t, H, W, VOXEL, TRUNC, 1, near=NEAR, far=FAR, guide=v["guide"],
                         window=2, fill=v["fill"], interp="trilinear", out=v["depth"], normal=v["normal"], colour=v["colour"],
                         view=v["view"], hits=run.hits.t)
    for _ in range(2):
        for name in OUTPUTS:
            v[name].zero_()
        run.hits.t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for name in OUTPUTS:
            got = npy(v[name])[..., 0] if name == "depth" else npy(v[name])
            assert np.array_equal(bits(got), bits(eager[name])), name
        assert np.array_equal(npy(run.hits.t), eager_hits)
    for x in run.bufs:
        x.check()


def test_sphere_equals_the_restatement(dev):
    """48 x 48 pixels (nine tiles), batch 1, 26 frames, L = 14; a fused and a novel view, both rules, every output."""
    from m4depth_amd import network_ops as nops
    S = T.SPHERE
    frames = T.sphere_frames()
    vol = T.fuse(frames, S["f"], S["c"], S["voxel"], S["trunc"], S["near"], S["far"])
    cam = {"f": np.array([S["f"]], F), "c": np.array([S["c"]], F)}
    g = GuardedState(1, 14, dev)
    for depth, rgb, pose in frames:
        Frame(dev, depth[None], rgb[None], cam, pose[None]).into(g, S["voxel"], S["trunc"], S["near"], S["far"])
    assert records(g.state, 0) == ref_records(vol)
    f, c = torch.from_numpy(cam["f"]).to(dev), torch.from_numpy(cam["c"]).to(dev)
    h, w = S["h"], S["w"]
    for pose in (frames[0][2], T.look_at_pose(NOVEL_SPHERE_EYE)):
        for interp in INTERPS:
            want = RR.render(vol.records, S["f"], S["c"], pose, h, w, S["voxel"], S["trunc"], 2, S["near"], S["far"], interp=RR.INTERP[interp])
            outs = {"depth": Guarded(dev, (1, h, w, 1), torch.float32), "normal": Guarded(dev, (1, h, w, 3), torch.float32),
                    "colour": Guarded(dev, (1, h, w, 3), torch.float32), "view": Guarded(dev, (1, h, w, 3), torch.uint8)}
            hits = torch.zeros(1, dtype=torch.int64, device=dev)
            nops.tsdf_render(g.state, f, c, torch.from_numpy(pose[None].copy()).to(dev), h, w, S["voxel"], S["trunc"], 2, near=S["near"],
                             far=S["far"], interp=interp, out=outs["depth"].t, normal=outs["normal"].t, colour=outs["colour"].t,
                             view=outs["view"].t, hits=hits)
            g.check()
            got = {}
            for name, buf in outs.items():
                buf.check()
                got[name] = npy(buf.t)[0, ..., 0] if name == "depth" else npy(buf.t)[0]
            assert want["hits"] > 900 and int(hits[0]) == want["hits"]
            assert np.isfinite(want["normal"][want["hit"]]).all() and np.isfinite(want["colour"][want["hit"]]).all()
            assert_equal(got, want, interp)


def test_the_grid_ends_and_the_origin(dev):
    """The hand-made columns of tests/test_tsdf_render_ref.py as device states: a base cell that straddles the world origin, one
    whose low corners lie at cell -2^20 - 1 (with a copy of the column where a wrapped index would look) and one whose high
    corners lie at 2^20."""
    from m4depth_amd import network_ops as nops
    from tsdf_mesh_ref import F32
    half = float(1 << 20)
    cases = [dict(), dict(shift=(3, 2, 0)), dict(shift=(0, 0, -9)), dict(drop=[(0, 1, 5)]), dict(x0=-half + 0.25, wrapped=True),
             dict(x0=-half + 1.25), dict(x0=half - 0.25)]
    for kw in cases:
        rec, (f, c, pose, h, w, voxel, trunc, min_frames) = column_case(LINEAR, **kw)
        st = nops.tsdf_state(1, 8, dev)
        mask = (1 << 8) - 1
        keys, recs = npy(st["keys"]).copy().view(np.uint64), npy(st["recs"]).copy()
        for key, r in rec.items():                             # the insertion's probe sequence on the host
            slot = ((key * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)) >> (64 - 8)
            while keys[0, slot] != np.uint64(T.EMPTY):
                slot = (slot + 1) & mask
            keys[0, slot] = np.uint64(key)
            recs[0, slot] = [int(F32(r[0]).view(np.int32))] + r[1:]
        st["keys"].copy_(torch.from_numpy(keys.view(np.int64)))
        st["recs"].copy_(torch.from_numpy(recs))
        dv = lambda a, t: torch.tensor([a], dtype=t, device=dev)                   # noqa: E731
        for interp in INTERPS:
            want = RR.render(rec, f, c, pose, h, w, voxel, trunc, min_frames, near=1.0, far=20.0, interp=RR.INTERP[interp])
            outs = {"normal": torch.zeros((1, 1, 1, 3), device=dev), "colour": torch.zeros((1, 1, 1, 3), device=dev),
                    "view": torch.zeros((1, 1, 1, 3), dtype=torch.uint8, device=dev)}
            depth = nops.tsdf_render(st, dv(f, torch.float32), dv(c, torch.float32), dv(pose, torch.float64), h, w, voxel, trunc,
                                     min_frames, near=1.0, far=20.0, interp=interp, **outs)
            got = dict({k: npy(v)[0] for k, v in outs.items()}, depth=npy(depth)[0, ..., 0])
            assert want["hits"] == 1
            assert_equal(got, want, (kw, interp))


def test_refusals(dev, plane):
    """What the op and the entry refuse beyond m4d_tsdf_raycast's list (tests/test_tsdf_render_ref.py has all of it on host
    pointers): on device pointers, without a launch."""
    from m4depth_amd import network_ops as nops
    from m4depth_amd._lib import lib
    run = Launch(dev, plane)
    st, v = plane["g"].state, run.views
    ok = dict(h=H, w=W, voxel=VOXEL, trunc=TRUNC, min_frames=1, near=NEAR, far=FAR, out=v["depth"])
    for kw in (dict(interp="cubic"), dict(interp=0), dict(normal=v["normal"][:, :-1]), dict(colour=v["colour"][:1]),
               dict(view=v["view"][..., :2]), dict(normal=v["depth"]), dict(view=v["view"].transpose(1, 2)), dict(trunc=9), dict(near=0.0)):
        with pytest.raises(ValueError):
            nops.tsdf_render(st, run.f.t, run.c.t, run.pose.t, **dict(ok, **kw))
    for kw in (dict(view=v["colour"]), dict(normal=v["view"]), dict(colour=v["colour"].double())):
        with pytest.raises(TypeError):
            nops.tsdf_render(st, run.f.t, run.c.t, run.pose.t, **dict(ok, **kw))
    image = H * W
    p = dict(state=st["words"].data_ptr(), f=run.f.t.data_ptr(), c=run.c.t.data_ptr(), pose=run.pose.t.data_ptr(), interp=1,
             out=v["depth"].data_ptr(), os=image, normal=v["normal"].data_ptr(), ns=3 * image, colour=v["colour"].data_ptr(),
             cs=3 * image, view=v["view"].data_ptr(), vs=3 * image)

    def raw(**kw):
        a = dict(p, **kw)
        return lib.m4d_tsdf_render(a["state"], B, L, a["f"], a["c"], a["pose"], H, W, NEAR, FAR, VOXEL, TRUNC, 1, None, 0, 0, None, 0,
                                   a["interp"], a["out"], a["os"], a["normal"], a["ns"], a["colour"], a["cs"], a["view"], a["vs"],
                                   None, None)

    n0 = lib.m4d_launch_count()
    for kw in (dict(interp=2), dict(interp=-1), dict(ns=3 * image - 1), dict(cs=3 * image - 1), dict(vs=3 * image - 1), dict(os=image - 1),
               dict(normal=p["normal"] + 2), dict(colour=p["colour"] + 2), dict(out=None), dict(state=p["state"] + 4)):
        assert raw(**kw) == 1, kw
    assert lib.m4d_launch_count() == n0
    for x in run.bufs:
        x.check()


# ---- fusion.FusedDepth -----------------------------------------------------------------------------------------------------------
def test_fused_depth_steps_equal_the_restatement(dev):
    """Plane frames as estimates through FusedDepth(interp="trilinear").step at batch 2, sample 1 restarting in the middle (device
    mask): every step equals clear + fuse + render of the restatement at the pose chain the device keeps; the optional outputs
    pass through; interp="nearest" without them is the raycast's launch."""
    from m4depth_amd.fusion import FusedDepth
    from test_gpu_tsdf_raycast import _motion
    b = 2
    cam = cameras_np(b, H, W)
    chain = T.plane_poses(4)
    order = [(0, 0), (1, 2), (2, 1), (3, 3)]                                      # (pose of sample 0, of sample 1) per step
    fd = FusedDepth(VOXEL, trunc=TRUNC, min_frames=1, slots_log2=L, near=NEAR, far=FAR, window=2, interp="trilinear")
    plain = FusedDepth(VOXEL, trunc=TRUNC, min_frames=1, slots_log2=L, near=NEAR, far=FAR, window=2)
    vols = [T.TsdfVolume(VOXEL, TRUNC, NEAR, FAR) for _ in range(b)]
    f, c = torch.from_numpy(cam["f"]).to(dev), torch.from_numpy(cam["c"]).to(dev)
    hits = torch.zeros((len(order), b), dtype=torch.int64, device=dev)
    outs = {"normal": torch.empty((b, H, W, 3), device=dev), "colour": torch.empty((b, H, W, 3), device=dev),
            "view": torch.empty((b, H, W, 3), dtype=torch.uint8, device=dev)}
    rng = np.random.default_rng(12)
    ident = np.array([1, 0, 0, 0, 0, 0, 0], np.float64)
    prev = [ident, ident]
    differs = 0
    for k, ps in enumerate(order):
        reset = np.array([k == 0, k == 0 or k == 2], np.uint8)
        cur = [ident if reset[s] else chain[ps[s]] for s in range(b)]
        motion = [_motion(prev[s], cur[s]) for s in range(b)]
        prev = cur
        est = np.stack([T.render_plane(cur[s], cam["f"][s], cam["c"][s], H, W, T.PLANE_NORMAL, T.PLANE_OFFSET) for s in range(b)])
        est[:, 2, 3] = np.nan
        rgb = rng.random((b, H, W, 3)).astype(F)
        args = (torch.from_numpy(est[..., None]).to(dev), torch.from_numpy(rgb).to(dev),
                torch.from_numpy(np.stack([m[0] for m in motion])).to(dev), torch.from_numpy(np.stack([m[1] for m in motion])).to(dev),
                {"f": f, "c": c}, torch.from_numpy(reset).to(dev))
        from m4depth_amd._lib import lib
        n0 = lib.m4d_launch_count()
        got_plain = npy(plain.step(*args))[..., 0]
        n1 = lib.m4d_launch_count()
        got = npy(fd.step(*args, hits=hits[k], **(outs if k % 2 else {})))[..., 0]
        assert lib.m4d_launch_count() - n1 == n1 - n0, "the same number of launches either way"
        poses = npy(fd.pose)
        for s in range(b):
            if reset[s]:
                vols[s] = T.TsdfVolume(VOXEL, TRUNC, NEAR, FAR)
            vols[s].frame(est[s], rgb[s], cam["f"][s], cam["c"][s], poses[s])
            for interp, g in (("trilinear", got), ("nearest", got_plain)):
                want = RR.render(vols[s].records, cam["f"][s], cam["c"][s], poses[s], H, W, VOXEL, TRUNC, 1, NEAR, FAR, guide=est[s],
                                 window=2, fill=est[s], interp=RR.INTERP[interp])
                assert np.array_equal(bits(g[s]), bits(want["depth"])), (k, s, interp)
                if interp == "trilinear":
                    assert int(hits[k, s]) == want["hits"] > 300
                    if k % 2:
                        assert_equal({n: npy(t)[s] for n, t in outs.items()}, want, (k, s))
            differs += int((bits(got[s]) != bits(got_plain[s])).sum())
    assert differs > 1000


# ---- the driver ------------------------------------------------------------------------------------------------------------------
LENGTHS = [5, 3, 6, 1]
SIZE = 64
ARCH = ["--arch_depth", "4", "--height", str(SIZE), "--width", str(SIZE)]
FUSED = ["--fused", "0.5", "--fused_slots_log2", "20"]
TRILINEAR = FUSED + ["--fused_interp", "trilinear"]


@pytest.fixture(scope="module")
def midair_set(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("fused_interp_eval"))
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


def _eval(dataset_set, *extra):
    """One main.py --mode=eval run (cached per flag set): ({file name: bytes} of its ckpt_dir, what it printed)."""
    from m4depth_amd import main as MAIN
    if extra not in _runs:
        cfg, rec, root = dataset_set
        ck = os.path.join(root, "ckpt_" + str(len(_runs)))
        argv = ["--mode", "eval", "--dataset", "midair", "--db_path_config", cfg, "--records_path", rec, "--ckpt_dir", ck]
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            assert MAIN.main(argv + ARCH + list(extra)) == 0
        _runs[extra] = ({n: open(os.path.join(ck, n), "rb").read() for n in sorted(os.listdir(ck)) if n.endswith(".txt")}, out.getvalue())
    return _runs[extra]


def test_driver_scores_the_trilinear_fused_depth(dev, midair_set):
    plain, _ = _eval(midair_set, "--eval_streams", "3")
    fused, said = _eval(midair_set, "--eval_streams", "3", *TRILINEAR)
    assert set(fused) == {"perfs-midair.txt", "perfs-fused-midair.txt", "fused-frames-midair.txt"}
    assert fused["perfs-midair.txt"] == plain["perfs-midair.txt"], "the raw metrics are what they are without the flag"
    assert "fused depth at 0.5 m (K 4, min_frames 2, whole range, trilinear sampling)" in said
    nearest, said = _eval(midair_set, "--eval_streams", "3", *FUSED)
    assert "(K 4, min_frames 2, whole range)" in said and nearest["perfs-midair.txt"] == plain["perfs-midair.txt"]
    assert nearest["perfs-fused-midair.txt"] != fused["perfs-fused-midair.txt"]
    assert nearest["fused-frames-midair.txt"] != fused["fused-frames-midair.txt"]
    for extra in (("--eval_streams_policy", "arrival"), ("--graph",)):
        other, _ = _eval(midair_set, "--eval_streams", "3", *TRILINEAR, *extra)
        assert other == fused, extra


# ---- predict: export.PredictionWriter(fused_interp=..., save_fused_view=True) ------------------------------------------------------
def test_prediction_writer_fused_view(dev, tmp_path):
    """Every <frame>_fused_view.png is the restatement's view of the trajectory's volume right after the frame went in and
    <frame>_fused.png its depth; every other file is what the writer writes without the new keywords, which write what they
    wrote before."""
    from PIL import Image
    from test_gpu_tsdf_mesh import _writer_run
    from test_gpu_tsdf_raycast import _kitti16
    voxel, trunc, near, far = 0.5, 3, 2.0, 40.0
    mesh = dict(save_mesh=voxel, mesh_trunc=trunc, mesh_min_frames=2, mesh_slots_log2=14, save_fused=True)
    dirs = {k: str(tmp_path / k) for k in ("view", "plain", "named")}
    writer, cam, seen = _writer_run(dev, dirs["view"], 0, fused_interp="trilinear", save_fused_view=True, **mesh)
    _writer_run(dev, dirs["plain"], 0, **mesh)
    _writer_run(dev, dirs["named"], 0, fused_interp="nearest", **mesh)
    assert "trilinear sampling" in " ".join(writer.summary())
    vols, traj, count, rendered, differs = {}, [-1, -1], {}, 0, 0
    for depth, rgb, pose, flags in seen:
        for s in range(2):
            if flags[s]:
                traj[s] += 1
                vols[s] = T.TsdfVolume(voxel, trunc, near, far)
            d = f"s{s:02d}_t{traj[s]:04d}"
            vols[s].frame(depth[s], rgb[s], cam["f"][s], cam["c"][s], pose[s])
            h, w = depth[s].shape
            want = RR.render(vols[s].records, cam["f"][s], cam["c"][s], pose[s], h, w, voxel, trunc, 2, near, far, interp=1)
            k = count[d] = count.get(d, -1) + 1
            got = np.asarray(Image.open(os.path.join(dirs["view"], d, f"{k:06d}_fused.png")))
            assert got.dtype == np.uint16 and np.array_equal(got, _kitti16(want["depth"])), (d, k)
            view = np.asarray(Image.open(os.path.join(dirs["view"], d, f"{k:06d}_fused_view.png")))
            assert view.dtype == np.uint8 and view.shape == (h, w, 3) and np.array_equal(view, want["view"]), (d, k)
            differs += int((got != np.asarray(Image.open(os.path.join(dirs["plain"], d, f"{k:06d}_fused.png")))).sum())
            rendered += want["hits"]
    # a tenth of a voxel between the two rules is a dozen steps of the 16-bit code: most rendered pixels differ
    assert rendered > 2000 and writer.fused_pixels == rendered and differs > rendered // 2
    for d in sorted(os.listdir(dirs["plain"])):
        files = sorted(os.listdir(os.path.join(dirs["plain"], d)))
        assert files == sorted(os.listdir(os.path.join(dirs["named"], d)))
        assert sorted(files + [f"{k:06d}_fused_view.png" for k in range(count[d] + 1)]) == sorted(os.listdir(os.path.join(dirs["view"], d)))
        for name in files:
            blobs = [open(os.path.join(dirs[k], d, name), "rb").read() for k in ("plain", "named", "view")]
            assert blobs[0] == blobs[1], (d, name)
            assert blobs[0] == blobs[2] or name.endswith("_fused.png"), (d, name)


def test_driver_predict_writes_fused_views(dev, tmp_path):
    """main.py --mode=predict --save_mesh --save_fused --fused_interp trilinear --save_fused_view on the streaming and the graphed
    path: the same files, a <frame>_fused_view.png beside every <frame>_fused.png, the closing line names the sampling."""
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
                              "--save_fused", "--fused_interp", "trilinear", "--save_fused_view"] + extra) == 0
        assert "(trilinear sampling), with views" in printed.getvalue()
        outs.append(out)
    names = sorted(os.listdir(os.path.join(outs[0], "s00_t0000")))
    assert names == sorted([f"{k:06d}_{kind}.png" for k in range(5) for kind in ("depth", "fused", "fused_view")] + ["mesh.ply"])
    for name in names:
        with open(os.path.join(outs[0], "s00_t0000", name), "rb") as a, open(os.path.join(outs[1], "s00_t0000", name), "rb") as b2:
            assert a.read() == b2.read(), name
    im = np.asarray(Image.open(os.path.join(outs[0], "s00_t0000", "000004_fused_view.png")))
    assert im.dtype == np.uint8 and im.shape == (48, 64, 3)
