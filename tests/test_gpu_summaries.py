"""Training summaries on the MI355X: m4d_summary_images against a restatement written here (colour bytes in numpy float32,
which reproduces the single multiply exactly; log-depth bytes against float64), summaries.TrainSummaryWriter on a real
replayed training step, and ``main --mode train --log_dir`` eager and graphed.

Log-depth tolerance: the kernel's float32 logf and divide are a few ulp of a value <= 255.5 (one ulp there is 1.5e-5), below
1e-4 in units of the byte scale.  A byte may therefore differ from the float64 byte only where the float64 ``x * 255.5`` lies
within 1e-3 of an integer, and then by exactly 1; with uniform fractional parts 0.2 % of the pixels lie that close, and the
tests allow 1 % of the log-depth pixels of a call.  Depths clipped to 1 or to 200 (a tenth of the log-uniform inputs; NaN, 0
and negative values too) are exact in both precisions -- log(1) = 0, and 255.5 is far from an integer -- so they are never
excused: their bytes must be 0 and 255."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest
import torch

from helpers import to_dev
from summary_reader import read_events, png_pixels
from m4depth_amd import synthetic

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 0xA5
SIZES = [(37, 53, 3), (37, 53, 3), (37, 53, 1), (19, 27, 1), (5, 3, 1), (1, 2, 1)]
KINDS = [0, 0, 1, 1, 1, 1]


# ------------------------------------------------------------------------------ the restatement
def colour_bytes(v):
    """q(v) in float32: numpy's float32 multiply is the kernel's."""
    v = np.asarray(v, F)
    with np.errstate(invalid="ignore", over="ignore"):
        t = v * F(255.5)
        out = np.where(t >= F(255.0), 255, np.where(t < 0, 0, np.trunc(np.where(np.isfinite(t), t, 0)))).astype(np.int64)
    return np.where(np.isnan(v), 0, out).astype(np.uint8)


def log_depth_f64(d):
    """(bytes, near) of kind 1 in float64: near marks the unclipped pixels whose x * 255.5 lies within 1e-3 of an integer."""
    d = np.asarray(d, np.float64)
    d = np.where(np.isnan(d), 1.0, d)                        # fmaxf(NaN, 1) = 1
    t = np.log(np.clip(d, 1.0, 200.0)) / np.log(200.0) * 255.5
    near = (np.abs(t - np.rint(t)) <= 1e-3) & (d > 1.0) & (d < 200.0)
    return np.where(t >= 255.0, 255, np.trunc(t)).astype(np.uint8), near


def check_log_depth(got, d, what, tally):
    """Asserts the bytes ``got`` of the depths ``d``; adds (pixels near a boundary, pixels) to ``tally`` for ``check_tally``."""
    want, near = log_depth_f64(d)
    diff = got.astype(int) - want.astype(int)
    print(f"{what}: {near.sum()} of {near.size} pixels near a byte boundary, {np.count_nonzero(diff)} bytes differ")
    assert not (diff != 0)[~near].any(), f"{what}: a byte differs away from a boundary"
    assert np.abs(diff).max(initial=0) <= 1, f"{what}: a byte differs by more than 1"
    tally[0] += int(near.sum())
    tally[1] += near.size


def check_tally(tally):
    print(f"near a byte boundary: {tally[0]} of {tally[1]} log-depth pixels ({100.0 * tally[0] / tally[1]:.3f} %)")
    assert tally[0] <= 0.01 * tally[1], "the tolerance excuses more than 1 % of the log-depth pixels"


def make_maps(b, seed):
    """The six maps of the kernel test for a batch of ``b``: colour and ground truth as frame slices of [b,3,H,W,c] batches
    (batch stride = 3 images), the three coarser maps dense."""
    rng = np.random.default_rng(seed)
    H, W = SIZES[0][:2]
    rgb = rng.uniform(-0.1, 1.1, (b, 3, H, W, 3)).astype(F)
    depth = np.exp(rng.uniform(np.log(0.5), np.log(400.0), (b, 3, H, W, 1))).astype(F)
    small = [np.exp(rng.uniform(np.log(0.5), np.log(400.0), (b,) + s)).astype(F) for s in SIZES[3:]]
    planted_c = [np.nan, np.inf, -np.inf, 0.0, -3.0, 1.0, 0.999, 254.999 / 255.5, 255.0 / 255.5]
    planted_d = [np.nan, np.inf, -np.inf, 0.0, -3.0, 1.0, 200.0, 199.99, 1.0000001]
    for i in range(min(b, 3)):
        rgb[i, -1].reshape(-1)[7 + i:7 + i + len(planted_c)] = planted_c
        rgb[i, -2].reshape(-1)[-len(planted_c) - i:rgb[i, -2].size - i] = planted_c
        depth[i, -1].reshape(-1)[11 + i:11 + i + len(planted_d)] = planted_d
        small[0][i].reshape(-1)[3:3 + len(planted_d)] = planted_d
        small[1][i].reshape(-1)[:len(planted_d)] = planted_d
    small[2][0].reshape(-1)[:] = [np.nan, 200.0]
    return rgb, depth, small


def run_kernel(maps, kinds, n, offsets, out):
    from m4depth_amd._lib import lib, stream_ptr
    m = len(maps)
    ints = lambda v: (ctypes.c_int * m)(*v)                                         # noqa: E731
    longs = lambda v: (ctypes.c_longlong * m)(*v)                                   # noqa: E731
    return lib.m4d_summary_images(m, (ctypes.c_void_p * m)(*[t.data_ptr() for t in maps]),
                                  longs([t.stride(0) for t in maps]), ints([t.shape[1] for t in maps]),
                                  ints([t.shape[2] for t in maps]), ints([t.shape[3] for t in maps]), ints(kinds),
                                  longs(offsets), n, ctypes.c_void_p(out.data_ptr()), stream_ptr())


def guarded_layout(n, lead):
    """Offsets with 48 guard bytes behind every range; ``lead`` shifts the first range (odd: every packed store misaligned)."""
    offsets, pos = [], lead
    for h, w, c in SIZES:
        offsets.append(pos)
        pos += n * h * w * c + 48
    return offsets, pos


@pytest.mark.parametrize("b,n,lead", [(4, 3, 16), (2, 2, 5)])
def test_summary_images_against_the_restatement(dev, b, n, lead):
    rgb, depth, small = make_maps(b, seed=20 + b)
    rgb_d, depth_d = torch.from_numpy(rgb).to(dev), torch.from_numpy(depth).to(dev)
    maps = [rgb_d[:, -1], rgb_d[:, -2], depth_d[:, -1]] + [torch.from_numpy(s).to(dev) for s in small]
    host = [rgb[:, -1], rgb[:, -2], depth[:, -1]] + small
    assert maps[0].stride(0) == 3 * 37 * 53 * 3 and maps[2].stride(0) == 3 * 37 * 53
    offsets, total = guarded_layout(n, lead)
    out = torch.full((total,), GUARD, dtype=torch.uint8, device=dev)
    assert run_kernel(maps, KINDS, n, offsets, out) == 0
    got = out.cpu().numpy()
    written, tally = np.zeros(total, bool), [0, 0]
    for m, (off, (h, w, c)) in enumerate(zip(offsets, SIZES)):
        size = n * h * w * c
        written[off:off + size] = True
        image = got[off:off + size].reshape(n, h, w, c)
        if KINDS[m] == 0:
            assert np.array_equal(image, colour_bytes(host[m][:n])), f"map {m}"
        else:
            check_log_depth(image, host[m][:n], f"map {m} (b {b})", tally)
    check_tally(tally)
    assert (got[~written] == GUARD).all(), "a byte outside the n images was written"        # guards, and no image i >= n
    # the planted values, spelled out
    first = got[offsets[0]:offsets[0] + 37 * 53 * 3][7:15]
    assert first.tolist() == [0, 255, 0, 0, 0, 255, 255, 254]
    d0 = got[offsets[2]:offsets[2] + 37 * 53][11:18]
    assert d0.tolist() == [0, 255, 0, 0, 0, 0, 255]
    assert got[offsets[5]:offsets[5] + 2].tolist() == [0, 255]
    # deterministic
    again = torch.full((total,), GUARD, dtype=torch.uint8, device=dev)
    assert run_kernel(maps, KINDS, n, offsets, again) == 0
    assert torch.equal(out, again)
    # the wrapper: the same bytes as views of one buffer, in its own layout
    from m4depth_amd import network_ops as nops
    views = nops.summary_images(maps, ["unit", "unit", "log_depth", "log_depth", "log_depth", "log_depth"], n)
    base = views[0].data_ptr()
    lay, lay_total = nops.summary_layout(SIZES, n)
    for v, off, lo, (h, w, c) in zip(views, offsets, lay, SIZES):
        assert v.dtype == torch.uint8 and tuple(v.shape) == (n, h, w, c) and v.data_ptr() - base == lo and lo % 16 == 0
        assert np.array_equal(v.cpu().numpy().reshape(-1), got[off:off + n * h * w * c])
    with pytest.raises(ValueError):
        nops.summary_images(maps, ["unit"] * 6, b + 1)                              # more images than the batch holds
    with pytest.raises(ValueError):
        nops.summary_images(maps, ["unit"] * 5 + ["depth"], n)
    with pytest.raises(ValueError):
        nops.summary_images(maps, ["unit"] * 6, n, out=torch.empty(lay_total - 1, dtype=torch.uint8, device=dev))


def test_summary_images_refusals_leave_out_untouched(dev):
    from m4depth_amd._lib import lib, stream_ptr
    src = torch.rand(4 * 3 * 4 * 3 + 8, device=dev)
    out = torch.full((512,), GUARD, dtype=torch.uint8, device=dev)

    def call(**over):
        a = dict(n_maps=2, src=[src.data_ptr(), src.data_ptr() + 4], stride=[40, 12], h=[3, 3], w=[4, 4], c=[3, 1],
                 kind=[0, 1], off=[0, 80], n=2, out=out.data_ptr())
        a.update(over)
        m = len(a["src"])
        return lib.m4d_summary_images(a["n_maps"], (ctypes.c_void_p * m)(*a["src"]), (ctypes.c_longlong * m)(*a["stride"]),
                                      (ctypes.c_int * m)(*a["h"]), (ctypes.c_int * m)(*a["w"]), (ctypes.c_int * m)(*a["c"]),
                                      (ctypes.c_int * m)(*a["kind"]), (ctypes.c_longlong * m)(*a["off"]), a["n"],
                                      ctypes.c_void_p(a["out"]) if a["out"] else None, stream_ptr())
    refused = [dict(n_maps=0), dict(n_maps=17), dict(n=0), dict(n=-1), dict(out=None), dict(src=[src.data_ptr(), None]),
               dict(c=[2, 1]), dict(c=[3, 0]), dict(kind=[0, 2]), dict(kind=[-1, 0]), dict(stride=[35, 12]),
               dict(stride=[40, 11]), dict(src=[src.data_ptr() + 2, src.data_ptr()]), dict(h=[0, 3]), dict(off=[0, 71]),
               dict(off=[23, 0]), dict(off=[-8, 80])]
    for over in refused:
        assert call(**over) == 1, over
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == GUARD).all()
    assert call() == 0                                       # the call they were all derived from is a valid one
    got = out.cpu().numpy()
    assert (got[72:80] == GUARD).all() and (got[104:] == GUARD).all() and not (got[:72] == GUARD).all()


# ------------------------------------------------------------------------------ the writer on a real step
L, H, W, T, B = 2, 64, 64, 3, 2                              # test_gpu_train_workflow.py's geometry
TAGS = ["RGB_im", "camera_prev_t_reproj", "depth_gt", "depth_lvl_0", "depth_lvl_1"]


def _data(seed):
    samples, cam = synthetic.make_sequence(B, T, H, W, seed=seed)
    data = {k: np.stack([s[k] for s in samples], axis=1) for k in ("RGB_im", "depth", "rot", "trans", "new_traj")}
    data["camera"] = cam
    return data


def _model(dev):
    import m4depth_amd as M
    from m4depth_amd import training as TR
    wts = synthetic.init_weights(nbre_levels=L, seed=5, dscv_range=2, sncv_range=2)
    model = M.M4Depth(nbre_levels=L, is_training=True, dscv_range=2, sncv_range=2).load_numpy_weights(wts, dev)
    return TR.set_trainable(model), TR


def _image_events(events):
    return [e for e in events if any("image" in v for v in e["values"])]


def _images_of(event):
    """{tag: [n,h,w,c] uint8} of an image event, checking every Summary.Image's header against its PNG."""
    out = {}
    for v in event["values"]:
        tag, _, index = v["tag"].partition("/image")
        pix = png_pixels(v["image"]["png"])
        pix = pix[..., None] if pix.ndim == 2 else pix
        assert (v["image"]["height"], v["image"]["width"], v["image"]["colorspace"]) == pix.shape
        assert index == "/%d" % len(out.setdefault(tag, []))
        out[tag].append(pix)
    return {k: np.stack(v) for k, v in out.items()}


def test_writer_reads_the_step_before_the_next_replay_overwrites_it(dev, tmp_path):
    from m4depth_amd.summaries import TrainSummaryWriter
    from m4depth_amd.depth_operations import reproject
    model, TR = _model(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, eps=1e-7, capturable=True)
    model.compile(optimizer=opt)
    batches = [to_dev(_data(70 + i), dev) for i in range(3)]
    runner = TR.GraphedTrainStep(model, batches[0], opt, warmup=1)
    assert runner.pyramid[0] is runner.est and len(runner.pyramid) == L
    assert [tuple(p.shape) for p in runner.pyramid] == [(B, H // 2, W // 2, 1), (B, H // 4, W // 4, 1)]
    runner(batches[1])
    kept = {k: v.cpu().numpy() for k, v in runner.static.items()}
    kept_pyr = [p.cpu().numpy() for p in runner.pyramid]
    kept_cam = {k: v.clone() for k, v in runner.camera.items()}
    writer = TrainSummaryWriter(str(tmp_path))
    writer.images(11, runner.static, runner.pyramid, runner.camera)
    runner(batches[2])                                       # overwrites every static tensor the summary was made of
    writer.scalars(12, 1.0, 2.0)
    writer.close()
    assert not np.array_equal(kept["RGB_im"], runner.static["RGB_im"].cpu().numpy())
    assert not np.array_equal(kept_pyr[1], runner.pyramid[1].cpu().numpy())
    assert np.array_equal(kept["RGB_im"], batches[1]["RGB_im"].cpu().numpy())

    events = read_events(writer.path)
    assert [e["step"] for e in events] == [0, 11, 12]
    got = _images_of(events[1])
    assert list(got) == TAGS and all(len(v) == B for v in got.values())
    assert np.array_equal(got["RGB_im"], colour_bytes(kept["RGB_im"][:, -1]))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                # noqa: E731
    warped, _ = reproject(up(kept["RGB_im"][:, -2]), up(kept["depth"][:, -1]), up(kept["rot"][:, -1]), up(kept["trans"][:, -1]),
                          kept_cam)
    assert np.array_equal(got["camera_prev_t_reproj"], colour_bytes(warped.cpu().numpy()))
    assert not np.array_equal(got["camera_prev_t_reproj"], got["RGB_im"])
    tally = [0, 0]
    check_log_depth(got["depth_gt"], kept["depth"][:, -1], "depth_gt", tally)
    for i in range(L):
        assert got[f"depth_lvl_{i}"].shape == (B, H >> (i + 1), W >> (i + 1), 1)
        check_log_depth(got[f"depth_lvl_{i}"], kept_pyr[i], f"depth_lvl_{i}", tally)
    check_tally(tally)


def test_eager_step_keeps_the_pyramid(dev):
    model, TR = _model(dev)
    model.compile(optimizer=torch.optim.Adam(model.parameters(), lr=1e-3, eps=1e-7))
    out = model.train_step(to_dev(_data(75), dev))
    assert sorted(out) == ["RMSE_log", "loss"]               # no new key: callers iterate the dict
    pyr = model.last_pyramid
    assert [tuple(p.shape) for p in pyr] == [(B, H // 2, W // 2, 1), (B, H // 4, W // 4, 1)]
    assert all(not p.requires_grad and torch.isfinite(p).all() for p in pyr)


# ------------------------------------------------------------------------------ the driver
SYN = ["--arch_depth", "2", "--height", str(H), "--width", str(W), "--seq_len", str(T), "--batch_size", str(B),
       "--learning_rate", "1e-3"]


def _printed(out):
    return [(int(m.group(1)), float(m.group(2)), float(m.group(3)))
            for m in re.finditer(r"^step (\d+): loss (\S+)  RMSE_log (\S+)", out, re.M)]


@pytest.mark.parametrize("graph", [False, True])
def test_driver_writes_scalars_every_step_and_images_at_the_interval(dev, tmp_path, capsys, graph):
    from m4depth_amd import main as MAIN
    logs = str(tmp_path / "logs")
    argv = ["--mode", "train", "--n_batches", "5", "--ckpt_dir", str(tmp_path / "ck"), "--summary_interval", "2",
            "--log_dir", logs] + SYN + (["--graph"] if graph else [])
    assert MAIN.main(argv) == 0
    printed = _printed(capsys.readouterr().out)
    assert [s for s, _, _ in printed] == [1, 2, 3, 4, 5]
    files = os.listdir(logs)
    assert len(files) == 1 and files[0].startswith("events.out.tfevents.")
    events = read_events(os.path.join(logs, files[0]))
    assert events[0]["file_version"] == "brain.Event:2"
    steps = [e["step"] for e in events[1:]]
    assert steps == sorted(steps), "steps must not decrease within the file"
    scalars = [e for e in events[1:] if e not in _image_events(events)]
    assert [e["step"] for e in scalars] == [1, 2, 3, 4, 5]
    for e, (step, loss, rmse) in zip(scalars, printed):
        assert [v["tag"] for v in e["values"]] == ["loss", "RMSE_log"]
        vals = [float(np.uint32(v["simple_value_bits"]).view(F)) for v in e["values"]]
        # to the printed precision: the printed value is rounded to 6 decimals (5e-7), the stored one to float32 (2^-24 relative)
        print(f"step {step}: file loss {vals[0]!r} RMSE_log {vals[1]!r}, printed {loss} {rmse}")
        for got, shown in zip(vals, (loss, rmse)):
            assert np.isfinite(got) and abs(got - shown) <= 5e-7 + 2.0 ** -24 * abs(shown) + 1e-12, (step, got, shown)
    images = _image_events(events)
    assert [e["step"] for e in images] == [2, 4]
    for e in images:
        got = _images_of(e)
        assert list(got) == TAGS
        assert [v.shape for v in got.values()] == [(B, H, W, 3), (B, H, W, 3), (B, H, W, 1), (B, H // 2, W // 2, 1),
                                                   (B, H // 4, W // 4, 1)]
    assert not np.array_equal(_images_of(images[0])["RGB_im"], _images_of(images[1])["RGB_im"])   # each its own batch


def test_driver_writes_no_event_file_without_log_dir(dev, tmp_path, capsys):
    from m4depth_amd import main as MAIN
    assert MAIN.main(["--mode", "train", "--n_batches", "1", "--ckpt_dir", str(tmp_path / "ck")] + SYN) == 0
    capsys.readouterr()
    assert not glob.glob(str(tmp_path / "**" / "events.out*"), recursive=True)
