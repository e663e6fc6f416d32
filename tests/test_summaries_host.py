"""Host side of the training summaries (m4depth_amd.summaries): the event-file format read back by the tests' own reader
(summary_reader.py: its own record framing and protocol-buffer wire decode; only crc32c is shared with the writer), the ring of TrainSummaryWriter with
stand-ins for the device work, argument validation of m4d_summary_images without a device, and the driver's refusal."""
import ctypes
import os
import re
import socket
import struct
import threading

import numpy as np
import pytest

from m4depth_amd.tf_checkpoint import crc32c
from summary_reader import mask, read_records, read_events, png_pixels, bits


# ------------------------------------------------------------------------------ the format
def test_crc32c_andmask():
    from m4depth_amd.tf_checkpoint import masked_crc32c
    assert crc32c(b"123456789") == 0xE3069283
    assert masked_crc32c(b"123456789") == mask(0xE3069283)


def _write_small_file(log_dir, rng):
    from m4depth_amd.summaries import EventFileWriter
    grey = rng.integers(0, 256, (1, 5, 7, 1), dtype=np.uint8)
    colour = rng.integers(0, 256, (2, 4, 3, 3), dtype=np.uint8)
    with EventFileWriter(log_dir) as w:
        w.add_scalars(1, {"loss": 0.25, "RMSE_log": 1.0 / 3.0})
        w.add_scalars(2, {"loss": float("nan"), "RMSE_log": 3e38})
        w.add_images(2, [("depth_gt", grey), ("RGB_im", colour)])
        w.add_scalars(2 ** 40, {"loss": -0.0})
        path = w.path
    return path, grey, colour


def test_event_file_reads_back(tmp_path):
    log_dir = str(tmp_path / "a" / "b")                     # created by the writer
    path, grey, colour = _write_small_file(log_dir, np.random.default_rng(3))
    assert os.listdir(log_dir) == [os.path.basename(path)]
    assert re.fullmatch(r"events\.out\.tfevents\.\d{10}\.%s\.%d\.0" % (re.escape(socket.gethostname()), os.getpid()),
                        os.path.basename(path))
    events = read_events(path)                               # both CRCs of every record verify
    assert len(events) == 5
    assert events[0]["file_version"] == "brain.Event:2" and events[0]["values"] == [] and events[0]["wall_time"] > 1e9
    assert [e["step"] for e in events[1:]] == [1, 2, 2, 2 ** 40]
    assert all("file_version" not in e and e["wall_time"] > 1e9 for e in events[1:])
    assert events[1]["values"] == [{"tag": "loss", "simple_value_bits": bits(0.25)},
                                   {"tag": "RMSE_log", "simple_value_bits": bits(1.0 / 3.0)}]
    assert events[2]["values"] == [{"tag": "loss", "simple_value_bits": bits(float("nan"))},
                                   {"tag": "RMSE_log", "simple_value_bits": bits(3e38)}]
    assert events[4]["values"] == [{"tag": "loss", "simple_value_bits": 0x80000000}]
    images = events[3]["values"]
    assert [v["tag"] for v in images] == ["depth_gt/image", "RGB_im/image/0", "RGB_im/image/1"]
    im = images[0]["image"]
    assert (im["height"], im["width"], im["colorspace"]) == (5, 7, 1)
    assert np.array_equal(png_pixels(im["png"]), grey[0, :, :, 0])
    for i in (0, 1):
        im = images[1 + i]["image"]
        assert (im["height"], im["width"], im["colorspace"]) == (4, 3, 3)
        assert np.array_equal(png_pixels(im["png"]), colour[i])


def test_reader_catches_a_flipped_byte(tmp_path):
    path, _, _ = _write_small_file(str(tmp_path), np.random.default_rng(4))
    blob = open(path, "rb").read()
    first = 12 + struct.unpack_from("<Q", blob, 0)[0] + 4    # where the second record starts
    for offset in (first + 3, first + 14, len(blob) - 2, 9):  # a length byte, a payload byte, a data CRC byte, a length CRC byte
        bad = bytearray(blob)
        bad[offset] ^= 0x10
        with pytest.raises(ValueError):
            read_records(bytes(bad))
    with pytest.raises(ValueError):
        read_records(blob[:-1])
    assert len(read_records(blob)) == 5


def test_writer_flushes_and_refuses_after_close(tmp_path):
    from m4depth_amd.summaries import EventFileWriter
    w = EventFileWriter(str(tmp_path))
    assert len(read_events(w.path)) == 1                      # the version record is on disk at once
    w.add_scalars(7, {"loss": 1.5})
    w.flush()
    assert [e["step"] for e in read_events(w.path)] == [0, 7]
    second = EventFileWriter(str(tmp_path))                  # the same second, the same process: another file
    assert second.path != w.path
    second.close()
    w.close()
    w.close()
    with pytest.raises(RuntimeError):
        w.add_scalars(8, {"loss": 1.0})


def test_tensorboard_reads_the_file(tmp_path):
    """Skipped where no tensorboard package exists (the build environment): the format is then only checked by the reader
    above."""
    pytest.importorskip("tensorboard")
    from tensorboard.backend.event_processing.event_accumulator import EventAccumulator
    path, grey, colour = _write_small_file(str(tmp_path), np.random.default_rng(5))
    acc = EventAccumulator(path, size_guidance={"images": 0, "scalars": 0})
    acc.Reload()
    assert sorted(acc.Tags()["scalars"]) == ["RMSE_log", "loss"]
    assert sorted(acc.Tags()["images"]) == ["RGB_im/image/0", "RGB_im/image/1", "depth_gt/image"]
    assert [(s.step, s.value) for s in acc.Scalars("RMSE_log")][0] == (1, float(np.float32(1.0 / 3.0)))
    im = acc.Images("depth_gt/image")[0]
    assert (im.step, im.height, im.width) == (2, 5, 7)
    assert np.array_equal(png_pixels(im.encoded_image_string), grey[0, :, :, 0])


# ------------------------------------------------------------------------------ the ring, with stand-ins for the device
class _Gate:
    """Stands in for the slot's device event: ``synchronize`` returns when the test opens the gate."""

    def __init__(self):
        self.open = threading.Event()

    def synchronize(self):
        assert self.open.wait(30), "the test never opened the gate"


class _Shape:
    def __init__(self, *shape):
        self.shape = shape


def _standin_writer(tmp_path, monkeypatch, **kw):
    """A TrainSummaryWriter whose device side is replaced: a slot is a numpy buffer with a gate, rendering fills every map of
    the slot with the step number; ``rendered`` collects the gate of every rendering."""
    from m4depth_amd import summaries as SM
    made, rendered = [], []

    class Slot:
        def __init__(self, nbytes, dev):
            self.host = np.zeros(nbytes, np.uint8)
            self.event = _Gate()
            made.append(self)

    def render(self, slot, data, pyramid, camera, n):
        _, shapes = self._geometry(data, pyramid)
        slot.event = data.get("gate") or _Gate()
        rendered.append(slot.event)
        return [np.full((n,) + s, data["step"], np.uint8) for s in shapes]

    monkeypatch.setattr(SM.TrainSummaryWriter, "_make_slot", lambda self, nbytes, dev: Slot(nbytes, dev))
    monkeypatch.setattr(SM.TrainSummaryWriter, "_render", render)
    return SM.TrainSummaryWriter(str(tmp_path), **kw), made, rendered


def _batch(step, b=4):
    return {"RGB_im": _Shape(b, 3, 6, 8, 3), "step": step}


PYRAMID = [_Shape(4, 3, 4, 1), _Shape(4, 2, 2, 1)]


def test_ring_is_bounded_ordered_and_drained(tmp_path, monkeypatch):
    writer, made, rendered = _standin_writer(tmp_path, monkeypatch, slots=2, threads=2)
    writer.scalars(1, 0.5, 0.25)
    writer.images(1, _batch(1), PYRAMID, None)
    writer.scalars(2, 0.4, 0.2)
    writer.images(2, _batch(2), PYRAMID, None)
    writer.scalars(3, 0.3, 0.1)
    assert len(made) == 2 and len(rendered) == 2
    assert made[0].host.nbytes == sum(-(-3 * h * w * c // 16) * 16 for h, w, c in ((6, 8, 3), (6, 8, 3), (6, 8, 1), (3, 4, 1), (2, 2, 1)))
    gates = list(rendered)

    # a third images() finds the ring full: it blocks until a slot comes back, and allocates nothing
    third = threading.Thread(target=lambda: writer.images(3, _batch(3), PYRAMID, None))
    third.start()
    third.join(0.3)
    assert third.is_alive() and len(rendered) == 2 and len(made) == 2

    # the second step's copy finishes first: its worker is done, but its event waits for its turn in the file
    gates[1].open.set()
    third.join(10)
    assert not third.is_alive() and len(rendered) == 3 and len(made) == 2
    writer.events.flush()
    assert [(e["step"], len(e["values"])) for e in read_events(writer.path)[1:]] == [(1, 2)]
    gates[0].open.set()
    rendered[2].open.set()
    writer.close()                                           # drains the ring
    writer.close()
    events = read_events(writer.path)[1:]
    assert [(e["step"], len(e["values"])) for e in events] == [(1, 2), (1, 15), (2, 2), (2, 15), (3, 2), (3, 15)]
    tags = [v["tag"] for v in events[1]["values"]]
    assert tags == [f"{t}/image/{i}" for t in ("RGB_im", "camera_prev_t_reproj", "depth_gt", "depth_lvl_0", "depth_lvl_1")
                    for i in range(3)]
    sizes = [(v["image"]["height"], v["image"]["width"], v["image"]["colorspace"]) for v in events[1]["values"][::3]]
    assert sizes == [(6, 8, 3), (6, 8, 3), (6, 8, 1), (3, 4, 1), (2, 2, 1)]
    for e in events[1::2]:
        assert all(np.all(png_pixels(v["image"]["png"]) == e["step"]) for v in e["values"])
    assert events[0]["values"] == [{"tag": "loss", "simple_value_bits": bits(0.5)},
                                   {"tag": "RMSE_log", "simple_value_bits": bits(0.25)}]
    with pytest.raises(RuntimeError):
        writer.scalars(4, 0.0, 0.0)


def test_one_sample_batch_and_worker_errors(tmp_path, monkeypatch):
    writer, made, rendered = _standin_writer(tmp_path, monkeypatch, max_outputs=3, slots=1, threads=1)
    writer.images(5, _batch(5, b=1), [_Shape(1, 3, 4, 1)], None)
    rendered[0].open.set()
    writer.scalars(5, 1.0, 1.0)
    with pytest.raises(ValueError):                          # another geometry than the ring was sized for
        writer.images(6, _batch(6, b=1), [_Shape(1, 5, 4, 1)], None)

    class Broken:
        def synchronize(self):
            raise OSError("the copy failed")
    writer.images(7, dict(_batch(7, b=1), gate=Broken()), [_Shape(1, 3, 4, 1)], None)
    writer.scalars(7, 2.0, 2.0)
    with pytest.raises(OSError):                             # close() drains, then re-raises what the worker hit
        writer.close()
    events = read_events(writer.path)[1:]
    assert [(e["step"], len(e["values"])) for e in events] == [(5, 4), (5, 2), (7, 2)]       # the failed event is left out, order kept
    assert [v["tag"] for v in events[0]["values"]] == ["RGB_im/image", "camera_prev_t_reproj/image", "depth_gt/image",
                                                       "depth_lvl_0/image"]


# ------------------------------------------------------------------------------ m4d_summary_images without a device
def _summary_call(**over):
    from m4depth_amd._lib import lib
    a = dict(n_maps=2, src=[4096, 8192], stride=[40, 12], h=[3, 3], w=[4, 4], c=[3, 1], kind=[0, 1], off=[0, 80], n=2,
             out=ctypes.c_void_p(4096), null=())
    a.update(over)
    m = len(a["src"])
    arrays = {"src": (ctypes.c_void_p * m)(*a["src"]), "stride": (ctypes.c_longlong * m)(*a["stride"]),
              "h": (ctypes.c_int * m)(*a["h"]), "w": (ctypes.c_int * m)(*a["w"]), "c": (ctypes.c_int * m)(*a["c"]),
              "kind": (ctypes.c_int * m)(*a["kind"]), "off": (ctypes.c_longlong * m)(*a["off"])}
    for name in a["null"]:
        arrays[name] = None
    return lib.m4d_summary_images(a["n_maps"], arrays["src"], arrays["stride"], arrays["h"], arrays["w"], arrays["c"],
                                  arrays["kind"], arrays["off"], a["n"], a["out"], None)


SUMMARY_REFUSED = {
    "no maps": dict(n_maps=0),
    "seventeen maps": dict(n_maps=17, src=[4096] * 17, stride=[12] * 17, h=[3] * 17, w=[4] * 17, c=[1] * 17, kind=[0] * 17,
                           off=[32 * i for i in range(17)]),
    "no images": dict(n=0),
    "null out": dict(out=None),
    "null source": dict(src=[4096, None]),
    "null source list": dict(null=("src",)),
    "null stride list": dict(null=("stride",)),
    "null kind list": dict(null=("kind",)),
    "null offset list": dict(null=("off",)),
    "two channels": dict(c=[2, 1]),
    "four channels": dict(c=[3, 4]),
    "unknown kind": dict(kind=[0, 2]),
    "negative kind": dict(kind=[-1, 1]),
    "stride below an image": dict(stride=[35, 12]),
    "misaligned source": dict(src=[4098, 8192]),
    "empty rows": dict(w=[0, 4], stride=[40, 12]),
    "overlapping outputs": dict(off=[0, 71]),
    "overlapping outputs, reversed": dict(off=[23, 0]),
    "negative offset": dict(off=[-72, 80]),
}


@pytest.mark.parametrize("why", sorted(SUMMARY_REFUSED))
def test_summary_images_refuses_without_a_device(why):
    assert _summary_call(**SUMMARY_REFUSED[why]) == 1, why


def test_driver_refuses_log_dir_outside_training(tmp_path, capsys):
    from m4depth_amd import main as MAIN
    out = str(tmp_path / "logs")
    for mode in ("eval", "predict", "validation"):
        with pytest.raises(SystemExit) as e:
            MAIN.main(["--mode", mode, "--log_dir", out])
        assert e.value.code == 2 and "--log_dir is a --mode=train" in capsys.readouterr().err
    assert not os.path.exists(out)
    assert MAIN.build_parser().parse_args([]).log_dir is None
