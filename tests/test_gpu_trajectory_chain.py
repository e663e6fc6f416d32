"""The per-step launch budget of fusion.TrajectoryChain's two consumers: a steady-state PredictionWriter.submit and a steady-state
FusedDepth.step issue exactly the library launches their options imply -- the sum of what each network_ops wrapper issues on its
own, measured here through m4d_launch_count, never a number written down -- and a writer step that ends a trajectory adds the
clears and the extractions, nothing else.  What the launches compute is held to the numpy restatements in test_gpu_cloud,
test_gpu_depth_views, test_gpu_voxel_map, test_gpu_tsdf_mesh and test_gpu_tsdf_raycast."""
import numpy as np
import pytest
import torch

from helpers import F
import depth_views_ref as DV

pytestmark = pytest.mark.gpu

B, H, W, L = 2, 24, 40, 12
VOXEL, TRUNC, MIN_FRAMES, NEAR, FAR = 0.5, 4, 2, 2.0, 40.0
STEPS = 4                                                        # the third is the steady state, the fourth ends sample 1's trajectory
FLAGS = [[True, True], [False, False], [False, False], [False, True]]


def _launches(fn):
    from m4depth_amd._lib import lib
    n0 = lib.m4d_launch_count()
    fn()
    return lib.m4d_launch_count() - n0


@pytest.fixture(scope="module")
def frames(dev):
    """STEPS frame batches of a camera that slides along the rendered plane: (est, rgb, rot, trans) per step, and the camera."""
    cam = {"f": np.tile(np.array([[20.0, 12.0]], F), (B, 1)), "c": np.tile(np.array([[20.3, 11.6]], F), (B, 1))}
    rng = np.random.default_rng(3)
    step = np.array([0.22, -0.12, 0.15])
    out = []
    for k in range(STEPS):
        pose = np.array([1.0, 0, 0, 0, *(step * k)])
        depth = np.stack([DV.render_plane(pose, cam["f"][s], cam["c"][s], H, W) for s in range(B)])
        assert np.isfinite(depth).all() and depth.min() > NEAR and depth.max() < FAR
        out.append((torch.from_numpy(depth[..., None].astype(F)).to(dev), torch.from_numpy(rng.random((B, H, W, 3)).astype(F)).to(dev),
                    torch.tensor([[1.0, 0.0, 0.0, 0.0]] * B, device=dev),
                    torch.from_numpy(np.tile((step * (k > 0)).astype(F), (B, 1))).to(dev)))
    return out, {k: torch.from_numpy(v).to(dev) for k, v in cam.items()}


@pytest.fixture(scope="module")
def unit(dev, frames):
    """Launches of every wrapper the chain calls, each measured on its own."""
    from m4depth_amd import network_ops as nops
    (est, rgb, rot, trans), camera = frames[0][0], frames[1]
    f, c = camera["f"], camera["c"]
    pose = torch.empty((B, 7), dtype=torch.float64, device=dev)
    views, volume, vmap = nops.depth_views_state(B, H, W, 2, dev), nops.tsdf_state(B, L, dev), nops.voxel_map_state(B, L, dev)
    mask = torch.tensor([0, 1], dtype=torch.uint8, device=dev)
    cloud = []
    n = {"pose_accumulate": _launches(lambda: nops.pose_accumulate(rot, trans, pose, force_all=True)),
         "depth_views": _launches(lambda: nops.depth_views(est, f, c, pose, views, force_all=True)),
         "tsdf_integrate": _launches(lambda: nops.tsdf_integrate(est, rgb, f, c, pose, VOXEL, TRUNC, volume, near=NEAR, far=FAR)),
         "tsdf_raycast": _launches(lambda: nops.tsdf_raycast(volume, f, c, pose, H, W, VOXEL, TRUNC, MIN_FRAMES, near=NEAR, far=FAR)),
         "depth_export": _launches(lambda: nops.depth_export(est, "kitti16")),
         "depth_cloud": _launches(lambda: cloud.extend(nops.depth_cloud(est, rgb, f, c, step=2, near=NEAR, far=FAR, pose=pose)))}
    n["voxel_map_integrate"] = _launches(lambda: nops.voxel_map_integrate(cloud[0], cloud[1], VOXEL, 1, vmap))
    n["tsdf_extract"] = _launches(lambda: nops.tsdf_extract(volume, 1, MIN_FRAMES, VOXEL))
    n["voxel_map_extract"] = _launches(lambda: nops.voxel_map_extract(vmap, 1, MIN_FRAMES, VOXEL))
    n["tsdf_clear"] = _launches(lambda: nops.tsdf_clear(volume, mask))
    n["voxel_map_clear"] = _launches(lambda: nops.voxel_map_clear(vmap, mask))
    torch.cuda.synchronize()
    assert all(v >= 1 for v in n.values()), n
    return n


def _implied(unit, cloud=False, cloud_views=0, save_map=None, save_mesh=None, save_fused=False, **_):
    """(launches of a steady-state submit, launches a step adds per ended trajectory, launches it adds once) by the options."""
    vertices = cloud or save_map is not None
    names = ["depth_export"]
    if vertices or save_mesh is not None:
        names += ["pose_accumulate"] + ["depth_views"] * bool(cloud_views)
    if save_mesh is not None:
        names += ["tsdf_integrate"] + ["tsdf_raycast", "depth_export"] * bool(save_fused)
    if vertices:
        names += ["depth_cloud"] + ["voxel_map_integrate"] * (save_map is not None)
    ended = ["voxel_map_extract"] * (save_map is not None) + ["tsdf_extract"] * (save_mesh is not None)
    clears = ["voxel_map_clear"] * (save_map is not None) + ["tsdf_clear"] * (save_mesh is not None)
    return tuple(sum(unit[k] for k in ks) for ks in (names, ended, clears))


OPTION_SETS = {"plain": {}, "cloud": dict(cloud=True), "cloud_views": dict(cloud=True, cloud_views=2), "map": dict(save_map=VOXEL),
               "mesh": dict(save_mesh=VOXEL), "mesh_fused": dict(save_mesh=VOXEL, save_fused=True),
               "everything": dict(cloud=True, cloud_views=2, save_conf=True, save_map=VOXEL, save_mesh=VOXEL, save_fused=True)}


@pytest.mark.parametrize("key", list(OPTION_SETS))
def test_writer_submit_issues_what_its_options_imply(dev, tmp_path, frames, unit, key):
    from m4depth_amd.export import PredictionWriter, FrameNamer
    options = OPTION_SETS[key]
    steps, camera = frames
    namer, got = FrameNamer(B), []
    with PredictionWriter(str(tmp_path), "kitti16", near=NEAR, far=FAR, slots=2, encode=False, map_slots_log2=L, mesh_slots_log2=L,
                          mesh_trunc=TRUNC, mesh_min_frames=MIN_FRAMES, map_min_frames=MIN_FRAMES, **options) as writer:
        for (est, rgb, rot, trans), flags in zip(steps, FLAGS):
            motion = dict(rgb=rgb, rot=rot, trans=trans, camera=camera, reset=np.array(flags)) if writer.needs_geometry else {}
            got.append(_launches(lambda: writer.submit(est, namer(flags), **motion)))
        assert writer.needs_geometry == (key != "plain")
    steady, per_ended, clears = _implied(unit, **options)
    assert got[2] == steady, (key, got, steady)
    assert got[1] == steady, "the second submit is a steady one too: only the first differs (nothing to clear, nobody to extract)"
    assert got[3] == steady + per_ended * sum(FLAGS[3]) + clears, (key, got, steady, per_ended, clears)
    assert (writer.maps, writer.meshes) == (3 * ("save_map" in options), 3 * ("save_mesh" in options)), "one ended, two closed"


def test_fused_depth_step_issues_clear_pose_integrate_raycast(dev, frames, unit):
    from m4depth_amd.fusion import FusedDepth
    steps, camera = frames
    fd = FusedDepth(VOXEL, trunc=TRUNC, min_frames=MIN_FRAMES, slots_log2=L, near=NEAR, far=FAR)
    got = []
    for (est, rgb, rot, trans), flags in zip(steps, FLAGS):
        mask = torch.tensor(flags, dtype=torch.uint8, device=dev)
        got.append(_launches(lambda: fd.step(est, rgb, rot, trans, camera, mask)))
    torch.cuda.synchronize()
    step = unit["tsdf_clear"] + unit["pose_accumulate"] + unit["tsdf_integrate"] + unit["tsdf_raycast"]
    assert got[1:] == [step] * 3, "every step after the first (which allocates) clears by the device mask, set or not"
