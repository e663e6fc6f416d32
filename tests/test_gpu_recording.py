"""The recording front end on the GPU: m4d_undistort_map, m4d_decode_rgb8_remap and m4d_decode_depth16_remap against the numpy
restatement of include/m4depth_hip.h (tests/recording_ref.py), with guard bytes around every raw call, then the driver end to
end on two small recordings (radtan with ground truth, equidistant without)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import recording_ref as RR
from recording_ref import CAMERA_A, CAMERA_B

pytestmark = pytest.mark.gpu
F = np.float32
GUARD, FILL = 4096, 0xA5                 # guard bytes on either side of every region, and their value


def assert_bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = got.view(np.uint32) != want.view(np.uint32)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} values differ, first at {np.argwhere(diff)[0]}"


class Guarded:
    """Device regions with GUARD sentinel bytes before and after: a write past an output changes a guard, a read past an input
    stays inside the test's own memory.  ``check()`` asserts every guard and every input is intact."""

    def __init__(self, dev):
        self.dev, self.regions = dev, []

    def _region(self, nbytes, data=None):
        buf = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=self.dev)
        view = buf[GUARD:GUARD + nbytes]
        if data is not None:
            view.copy_(torch.from_numpy(data.reshape(-1).view(np.uint8).copy()).to(self.dev))
        self.regions.append((buf, nbytes, None if data is None else view.clone()))
        return view

    def put(self, array):
        array = np.ascontiguousarray(array)
        return self._region(array.nbytes, array)

    def out(self, shape, dtype=F):
        return self._region(int(np.prod(shape)) * np.dtype(dtype).itemsize)

    def check(self, what):
        for buf, nbytes, data in self.regions:
            assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + nbytes:] == FILL).all()), f"{what}: a guard byte changed"
            if data is not None:
                assert bool((buf[GUARD:GUARD + nbytes] == data).all()), f"{what}: an input changed"


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def as_array(view, shape, dtype=F):
    return view.cpu().numpy().view(dtype).reshape(shape)


def camera_numbers(cam):
    return cam["fx"], cam["fy"], cam["cx"], cam["cy"]


def output_camera(cam, oh, ow, zoom=1.0):
    from m4depth_amd.dataloaders.recording import output_camera as oc
    return oc(dict(cam, zoom=zoom), oh, ow)


def device_map(dev, cam, out_cam, oh, ow):
    from m4depth_amd._lib import lib, check, stream_ptr
    g = Guarded(dev)
    table = g.out((oh, ow, 2))
    f4 = ctypes.c_float * 4
    dist = (ctypes.c_float * len(cam.get("distortion", [])))(*cam.get("distortion", [])) if cam.get("distortion") else None
    check(lib.m4d_undistort_map(RR.MODELS[cam["model"]], dist, f4(*camera_numbers(cam)), f4(*out_cam), cam["height"], cam["width"],
                                oh, ow, P(table), stream_ptr()), "m4d_undistort_map")
    torch.cuda.synchronize()
    g.check("m4d_undistort_map")
    return as_array(table, (oh, ow, 2))


def reference_maps(cam, out_cam, oh, ow):
    args = (cam["model"], cam.get("distortion", []), camera_numbers(cam), out_cam, cam["height"], cam["width"], oh, ow)
    return RR.undistort_map(*args, dtype=F), RR.undistort_map(*args, dtype=np.float64)


# ---- the table ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zoom", [1.0, 0.6])
def test_map_radtan_is_bit_exact(dev, zoom):
    out_cam = output_camera(CAMERA_A, 40, 56, zoom)
    m32, m64 = reference_maps(CAMERA_A, out_cam, 40, 56)
    got = device_map(dev, CAMERA_A, out_cam, 40, 56)
    assert_bits_equal(got, m32, f"radtan table at zoom {zoom}")
    none = ~RR.has_source(got)
    assert np.array_equal(none, m64[..., 0] < -0.5), "float32 and float64 disagree on an entry's validity"
    assert np.array_equal(got[none], np.full((int(none.sum()), 2), -1.0, F))
    share = none.mean()
    print(f"zoom {zoom}: {100 * share:.1f} % of the entries have no source")
    if zoom == 1.0:
        assert share == 0.0
    else:
        assert 0.30 < share < 0.40                               # the branch is exercised and does not swallow the image


def test_map_pinhole_is_the_half_pixel_resize(dev):
    cam = dict(CAMERA_A, model="pinhole", distortion=[])
    out_cam = output_camera(cam, 30, 47)
    assert out_cam == pytest.approx((cam["fx"] / 2, cam["fy"] / 2, cam["cx"] / 2, cam["cy"] / 2), abs=1e-12)
    m32, _ = reference_maps(cam, out_cam, 30, 47)
    got = device_map(dev, cam, out_cam, 30, 47)
    assert_bits_equal(got, m32, "pinhole table")
    want = RR.half_pixel_table(60, 94, 30, 47).astype(np.float64)   # (o + 0.5) * 2 - 0.5, through the division and the product
    assert np.abs(got - want).max() <= 8 * 2.0 ** -18              # at most 8 float32 roundings, each <= half an ulp below 128


def test_map_equidistant_against_float64(dev):
    """The device's atanf / sqrtf need not round like numpy's: the yardstick is the float64 restatement, the bound four times the
    float32 restatement's own distance from it (a device atanf a couple of ulp off)."""
    out_cam = output_camera(CAMERA_B, 40, 56)
    m32, m64 = reference_maps(CAMERA_B, out_cam, 40, 56)
    own = np.hypot(*np.moveaxis(m32 - m64, -1, 0)).max()
    assert 1e-6 < own < 2e-5                                       # 5.5e-6 px expected: a float32 at magnitude 64
    got = device_map(dev, CAMERA_B, out_cam, 40, 56)
    assert np.array_equal(RR.has_source(got), m64[..., 0] >= -0.5), "validity differs from float64"
    ok = RR.has_source(got)
    dist = np.hypot(*np.moveaxis(got.astype(np.float64) - m64, -1, 0))[ok].max()
    print(f"equidistant table: device {dist:.3e} px from float64, float32 restatement {own:.3e} px, bound {4 * own:.3e} px")
    assert dist <= 4 * own


# ---- the samplers ---------------------------------------------------------------------------------------------------------------------
def edge_rows(ih, iw):
    """Two hand-made table rows: the four edge coordinates of u (at an interior v), the same four of v, an integer coordinate
    (ceil == floor) and a (-1, -1) entry; a third row of entries that are no source by the header's rule (infinite, NaN, below
    -0.5) and one finite coordinate far past the image, which samples the border."""
    us = [-0.5, 0.0, iw - 1.0, iw - 0.5]
    vs = [-0.5, 0.0, ih - 1.0, ih - 0.5]
    row0 = [(u, 7.25) for u in us] + [(11.5, v) for v in vs]
    row1 = [(u, v) for u, v in zip(us, vs)] + [(13.0, 9.0), (-1.0, -1.0), (us[3], vs[0]), (20.75, 30.125)]
    row2 = [(np.inf, 3.0), (3.0, np.inf), (np.nan, 3.0), (3.0, np.nan), (-np.inf, 3.0), (-0.75, 3.0), (3.0, -0.75), (1e30, 3.0)]
    return np.array([row0, row1, row2], F)


def run_rgb(dev, images, table):
    from m4depth_amd._lib import lib, check, stream_ptr
    n, ih, iw, _ = images.shape
    oh, ow = table.shape[:2]
    g = Guarded(dev)
    img, tab, out = g.put(images), g.put(table), g.out((n, oh, ow, 3))
    check(lib.m4d_decode_rgb8_remap(P(img), P(tab), n, ih, iw, oh, ow, P(out), stream_ptr()), "m4d_decode_rgb8_remap")
    torch.cuda.synchronize()
    g.check("m4d_decode_rgb8_remap")
    return as_array(out, (n, oh, ow, 3))


def run_depth(dev, raw, table, inv_scale):
    from m4depth_amd._lib import lib, check, stream_ptr
    n, ih, iw = raw.shape
    oh, ow = table.shape[:2]
    g = Guarded(dev)
    src, tab, out = g.put(raw), g.put(table), g.out((n, oh, ow, 1))
    check(lib.m4d_decode_depth16_remap(P(src), P(tab), float(inv_scale), n, ih, iw, oh, ow, P(out), stream_ptr()),
          "m4d_decode_depth16_remap")
    torch.cuda.synchronize()
    g.check("m4d_decode_depth16_remap")
    return as_array(out, (n, oh, ow, 1))


@pytest.fixture(scope="module")
def tables():
    """Camera A's table at zoom 0.6 (a third of it without a source) and the hand-made edge rows, from the restatement."""
    m32, _ = reference_maps(CAMERA_A, output_camera(CAMERA_A, 40, 56, 0.6), 40, 56)
    return {"zoom": m32, "edges": edge_rows(60, 94)}


@pytest.mark.parametrize("which", ["zoom", "edges"])
def test_rgb_remap_is_bit_exact(dev, tables, which):
    table = tables[which]
    images = np.random.default_rng(11).integers(0, 256, (3, 60, 94, 3), dtype=np.uint8)     # n = 3, odd sizes: the image stride
    got = run_rgb(dev, images, table)
    assert_bits_equal(got, RR.decode_rgb8_remap(images, table), f"rgb through the {which} table")
    none = ~RR.has_source(table)
    assert none.any() and not got[:, none].any() and got[:, ~none].any()
    assert len({got[i].tobytes() for i in range(3)}) == 3          # three distinct frames came out
    if which == "edges":                                           # the edge taps, by hand: u = -0.5 / iw - 0.5 clamp to the border
        img = images.astype(F) / F(255.0)
        assert_bits_equal(got[:, 1, 4], img[:, 9, 13], "an integer coordinate is the pixel itself")
        assert_bits_equal(got[:, 1, 0], img[:, 0, 0], "(-0.5, -0.5) is the corner pixel")
        assert_bits_equal(got[:, 1, 3], img[:, 59, 93], "(iw - 0.5, ih - 0.5) is the opposite corner")
        assert_bits_equal(got[:, 1, 6], img[:, 0, 93], "(iw - 0.5, -0.5)")
        assert none[2, :7].all() and not none[2, 7]                # infinite, NaN and below -0.5: no source, zeros, never NaN
        assert_bits_equal(got[:, 2, 7], img[:, 3, 93], "a finite coordinate far past the image samples the border")


@pytest.mark.parametrize("shape", [(60, 94, 24, 40), (24, 40, 60, 94)], ids=["down", "up"])
def test_rgb_remap_equals_the_resize_kernel(dev, shape):
    """With the table ((o + 0.5) * scale - 0.5) the remap IS m4d_decode_rgb8_resize: bit for bit, both directions."""
    from m4depth_amd._lib import lib, check, stream_ptr, dptr
    ih, iw, oh, ow = shape
    images = np.random.default_rng(12).integers(0, 256, (3, ih, iw, 3), dtype=np.uint8)
    table = RR.half_pixel_table(ih, iw, oh, ow)
    assert RR.has_source(table).all() and table[..., 0].max() <= iw - 0.5 and table[..., 1].max() <= ih - 0.5
    got = run_rgb(dev, images, table)
    src = torch.from_numpy(images).to(dev)
    want = torch.empty((3, oh, ow, 3), dtype=torch.float32, device=dev)
    check(lib.m4d_decode_rgb8_resize(dptr(src, "rgb", torch.uint8), 3, ih, iw, oh, ow, dptr(want), stream_ptr()),
          "m4d_decode_rgb8_resize")
    assert_bits_equal(got, want.cpu().numpy(), f"remap against resize {ih}x{iw} -> {oh}x{ow}")


@pytest.mark.parametrize("which", ["zoom", "edges"])
def test_depth_remap_is_bit_exact(dev, tables, which):
    table = tables[which]
    rng = np.random.default_rng(13)
    raw = rng.integers(1, 65536, (3, 60, 94), dtype=np.uint16)
    raw[rng.random(raw.shape) < 0.2] = 0                           # holes
    raw[:, 0, 0] = 0
    inv_scale = F(1.0) / F(5000.0)
    got = run_depth(dev, raw, table, inv_scale)
    want = RR.decode_depth16_remap(raw, table, inv_scale)
    assert_bits_equal(got, want, f"depth through the {which} table")
    none = ~RR.has_source(table)
    assert not got[:, none].any()
    # zero-valued source pixels give exactly 0, every other pixel with a source a positive depth
    safe = np.where(none[..., None], F(0.0), table)
    xi = np.clip(np.floor(safe[..., 0] + F(0.5)), 0, 93).astype(int)
    yi = np.clip(np.floor(safe[..., 1] + F(0.5)), 0, 59).astype(int)
    hole = raw[:, yi, xi] == 0
    assert hole[:, ~none].any() and np.array_equal(got[..., 0] == 0, hole | none[None])
    if which == "edges":
        assert not got[:, 1, 0].any()                              # raw[:, 0, 0] = 0 at (-0.5, -0.5)
        assert_bits_equal(got[:, 1, 4, 0], raw[:, 9, 13].astype(F) * inv_scale, "an integer coordinate")
        assert_bits_equal(got[:, 1, 7, 0], raw[:, 30, 21].astype(F) * inv_scale, "(20.75, 30.125) rounds to (21, 30)")


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
SIZE = ["--arch_depth", "2", "--height", "64", "--width", "64"]


@pytest.fixture(scope="module")
def recordings(tmp_path_factory):
    """mixed/: a (camera A, 8 frames, ground truth) and b (camera B, 6 frames, none); gt/: a and c (camera B with ground truth)."""
    root = str(tmp_path_factory.mktemp("recordings"))
    extra = {"T_body_cam": [0.5, 0.5, -0.5, 0.5, 0.05, -0.02, 0.1], "zoom": 0.8}
    for group, name, cam, n, depth in (("mixed", "a", CAMERA_A, 8, True), ("mixed", "b", CAMERA_B, 6, False),
                                       ("gt", "a", CAMERA_A, 8, True), ("gt", "c", CAMERA_B, 6, True)):
        RR.write_recording(os.path.join(root, group, name), cam, n, depth, extra=extra if cam is CAMERA_A else None)
    return root


def loader_rows(path):
    """The rows the loader makes of ``path`` (host work only)."""
    from m4depth_amd import dataloaders as dl
    loader = dl.get_loader("recording")
    loader.get_dataset("predict", dl.DataloaderParameters(None, path, None, None, False), batch_size=1, out_size=[64, 64],
                       device="cpu")
    return loader, loader._get_trajectories()


def test_predict_writes_depth_maps_and_posed_clouds(dev, recordings):
    from m4depth_amd import main as MAIN
    from m4depth_amd.export import read_cloud_ply
    out = os.path.join(recordings, "predict")
    assert MAIN.main(["--mode", "predict", "--dataset", "recording", "--records_path", os.path.join(recordings, "mixed"), "--stream",
                      "--save_dir", out, "--save_cloud", "--ckpt_dir", out + "_ckpt"] + SIZE) == 0
    assert sorted(os.listdir(out)) == ["s00_t0000", "s00_t0001"]
    for folder, n in (("s00_t0000", 8), ("s00_t0001", 6)):
        assert sorted(os.listdir(os.path.join(out, folder))) == sorted(f"{k:06d}_{s}" for k in range(n)
                                                                        for s in ("depth.png", "cloud.ply"))
    _, trajs = loader_rows(os.path.join(recordings, "mixed"))
    pose = np.array([1, 0, 0, 0, 0, 0, 0], np.float64)
    for k, row in enumerate(trajs[0]):
        if k:
            pose = RR.pose_step(pose, [row[c] for c in ("qw", "qx", "qy", "qz")], [row[c] for c in ("tx", "ty", "tz")])
        got = read_cloud_ply(os.path.join(out, "s00_t0000", f"{k:06d}_cloud.ply"))[2]
        assert np.abs(got - pose).max() <= 1e-9, (k, got, pose)
    assert np.abs(pose[4:] - [0, 0, 0]).max() > 0.5                # the camera did move


def test_eval_on_a_recording_with_ground_truth(dev, recordings):
    from m4depth_amd import main as MAIN
    ck = os.path.join(recordings, "eval_ckpt")
    assert MAIN.main(["--mode", "eval", "--dataset", "recording", "--records_path", os.path.join(recordings, "mixed", "a"),
                      "--ckpt_dir", ck] + SIZE) == 0
    perfs = np.loadtxt(os.path.join(ck, "perfs-recording.txt"))
    assert perfs.shape == (7,) and np.all(np.isfinite(perfs))


def test_eval_streams_mixes_cameras_and_refuses_recordings_without_ground_truth(dev, recordings):
    """Two slots, two recordings with different cameras and source sizes in every step.  A sample without ground truth cannot
    be scored (m4d_depth_metrics_per_sample reads a ground-truth map for every slot), so the scoring use cases refuse a
    recording without depth.txt."""
    from m4depth_amd import main as MAIN
    ck = os.path.join(recordings, "streams_ckpt")
    common = ["--mode", "eval", "--dataset", "recording", "--eval_streams", "2", "--ckpt_dir", ck] + SIZE
    assert MAIN.main(common + ["--records_path", os.path.join(recordings, "gt")]) == 0
    perfs = np.loadtxt(os.path.join(ck, "perfs-recording.txt"))
    assert perfs.shape == (7,) and np.all(np.isfinite(perfs))
    with pytest.raises(ValueError, match=r"b: no depth\.txt -- the 'eval_streams' use case scores against ground truth"):
        MAIN.main(common + ["--records_path", os.path.join(recordings, "mixed")])
    with pytest.raises(ValueError, match=r"b: no depth\.txt -- the 'eval' use case"):
        MAIN.main(["--mode", "eval", "--dataset", "recording", "--ckpt_dir", ck, "--records_path",
                   os.path.join(recordings, "mixed")] + SIZE)


def test_loader_frame_equals_the_restatement(dev, recordings):
    from PIL import Image
    from m4depth_amd import dataloaders as dl
    loader = dl.get_loader("recording")
    path = os.path.join(recordings, "mixed")
    ds = loader.get_dataset("predict", dl.DataloaderParameters(None, path, None, None, False), batch_size=1, out_size=[64, 64],
                            device=dev)
    frames = [b for _, b in zip(range(9), ds)]                      # frames 0..7 of a, frame 0 of b
    cam = loader.recordings[0].camera
    out_cam = output_camera(cam, 64, 64, cam["zoom"])
    m32, _ = reference_maps(cam, out_cam, 64, 64)
    assert (~RR.has_source(m32)).mean() > 0.05                      # zoom 0.8: a border without a source
    with Image.open(os.path.join(path, "a", "rgb", "0002.png")) as im:
        rgb = np.asarray(im.convert("RGB"), np.uint8)
    with Image.open(os.path.join(path, "a", "depth", "0002.png")) as im:
        raw = np.asarray(im, np.uint16)
    assert tuple(frames[2]["RGB_im"].shape) == (1, 64, 64, 3)
    assert_bits_equal(frames[2]["RGB_im"].cpu().numpy(), RR.decode_rgb8_remap(rgb[None], m32), "the loader's RGB_im")
    assert_bits_equal(frames[2]["depth"].cpu().numpy(), RR.decode_depth16_remap(raw[None], m32, F(1.0) / F(5000.0)),
                      "the loader's depth")
    assert frames[2]["camera"]["f"].cpu().numpy().tolist() == [[float(F(out_cam[0])), float(F(out_cam[1]))]]
    assert [bool(f["new_traj"].item()) for f in frames] == [True] + [False] * 7 + [True]
    assert "depth" not in frames[8] and frames[8]["camera"]["f"].cpu().numpy().tolist() == \
        [[float(F(CAMERA_B["fx"])), float(F(CAMERA_B["fy"]))]]
    assert sorted(loader._tables) == [0, 1]                        # one table per recording, kept on the device


def test_training_batch_from_a_recording(dev, recordings):
    """The train use case comes with the base class: one augmented batch of seq_len 4 feeds train_step."""
    import m4depth_amd as M
    from m4depth_amd import dataloaders as dl, synthetic, training as TR
    loader = dl.get_loader("recording")
    ds = loader.get_dataset("train", dl.DataloaderParameters(None, os.path.join(recordings, "mixed", "a"), 4, 4, True),
                            batch_size=1, out_size=[64, 64], device=dev, seed=3)
    model = M.M4Depth(depth_type=loader.depth_type, nbre_levels=2, is_training=True, dscv_range=2, sncv_range=2)
    model.load_numpy_weights(synthetic.init_weights(nbre_levels=2, seed=1, dscv_range=2, sncv_range=2), dev)
    TR.set_trainable(model)
    model.compile(optimizer=torch.optim.Adam(model.parameters(), lr=1e-4, eps=1e-7))
    batch = next(iter(ds))
    assert tuple(batch["RGB_im"].shape) == (1, 4, 64, 64, 3) and tuple(batch["depth"].shape) == (1, 4, 64, 64, 1)
    assert batch["new_traj"].tolist() == [[True, False, False, False]]
    assert np.isfinite(float(model.train_step(batch)["loss"]))
