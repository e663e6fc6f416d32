"""Training summaries -- the counterpart of the reference's ``tf.summary`` calls in ``train_step``
(m4depth_network.py:401-415) and of the Keras TensorBoard callback of its training driver (main.py:86-89, ``--log_dir``,
m4depth_options.py:43): the loss and ``RMSE_log`` curves, the last frame's image, the previous image re-projected with the
ground-truth depth and pose (``camera_prev_t_reproj``), the ground-truth log depth and every pyramid level's estimate
(``depth_lvl_i``), written as a TensorBoard event file.

``EventFileWriter`` is pure Python, written against the format itself (no ``tensorboard`` / ``tensorflow`` package exists in the
build environment; ``tf_checkpoint.py`` reads the neighbouring bundle format the same way and its crc32c is reused):

* file name ``events.out.tfevents.<unix seconds, 10 digits>.<hostname>.<pid>.0`` in ``log_dir``;
* a file is a sequence of records: ``uint64 LE length``, ``uint32 LE masked_crc32c(the 8 length bytes)``, the payload,
  ``uint32 LE masked_crc32c(payload)``, with mask(c) = ((c >> 15 | c << 17) + 0xA282EAD8) mod 2^32;
* a payload is a serialised ``Event`` protocol buffer; the first one is ``Event{wall_time, file_version="brain.Event:2"}``;
* field numbers (hand-encoded below: varints and length-delimited fields, no generated ``_pb2`` module):

      Event          wall_time double = 1, step int64 = 2, file_version string = 3, summary Summary = 5
      Summary        repeated value Summary.Value = 1
      Summary.Value  tag string = 1, simple_value float = 2, image Summary.Image = 4
      Summary.Image  height int32 = 1, width int32 = 2, colorspace int32 = 3 (1 grey, 3 RGB),
                     encoded_image_string bytes = 4 (a PNG)

* image tags follow the v1 convention of ``tf.summary.image``: ``<tag>/image`` for one image, else ``<tag>/image/0``,
  ``<tag>/image/1``, ...

The format has been read back only by the independent reader of tests/test_summaries_host.py: it has NOT been opened in
TensorBoard here.

``TrainSummaryWriter`` keeps the training loop free of host waits, the way ``export.PredictionWriter`` does for predictions: one
``network_ops.summary_images`` launch turns all maps of a step into uint8 on the device, the bytes are copied asynchronously
into a ring of pinned buffers, and host threads compress them to PNG and append the event while the next steps run.
"""
from __future__ import annotations

import io
import os
import queue
import socket
import struct
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .tf_checkpoint import masked_crc32c

FILE_VERSION = "brain.Event:2"


# ------------------------------------------------------------------------------ protocol buffer wire format
def _varint(v):
    v &= (1 << 64) - 1                                     # int32 / int64 fields: negative values as 64-bit two's complement
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _key(field, wire_type):
    return _varint((field << 3) | wire_type)


def _int_field(field, v):
    return _key(field, 0) + _varint(int(v))


def _bytes_field(field, data):
    if isinstance(data, str):
        data = data.encode("utf-8")
    return _key(field, 2) + _varint(len(data)) + bytes(data)


def scalar_value(tag, value):
    """A serialised ``Summary.Value{tag, simple_value}``."""
    return _bytes_field(1, tag) + _key(2, 5) + np.float32(value).tobytes()


def image_value(tag, height, width, colorspace, png):
    """A serialised ``Summary.Value{tag, image}`` around the PNG bytes ``png``."""
    image = _int_field(1, height) + _int_field(2, width) + _int_field(3, colorspace) + _bytes_field(4, png)
    return _bytes_field(1, tag) + _bytes_field(4, image)


def image_tags(tag, n):
    return [tag + "/image"] if n == 1 else [f"{tag}/image/{i}" for i in range(n)]


def encode_event(wall_time, step=None, values=None, file_version=None):
    """A serialised ``Event``: ``values`` is a list of serialised ``Summary.Value`` messages."""
    out = _key(1, 1) + struct.pack("<d", float(wall_time))
    if step is not None:
        out += _int_field(2, step)
    if file_version is not None:
        out += _bytes_field(3, file_version)
    if values is not None:
        out += _bytes_field(5, b"".join(_bytes_field(1, v) for v in values))
    return out


def encode_png(image):
    """[h,w,1] or [h,w,3] uint8 -> PNG bytes (PIL)."""
    from PIL import Image
    arr = np.ascontiguousarray(image)
    if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] not in (1, 3):
        raise ValueError(f"encode_png: expected [h,w,1 or 3] uint8, got {arr.dtype} {arr.shape}")
    buf = io.BytesIO()
    Image.fromarray(arr[..., 0] if arr.shape[2] == 1 else arr).save(buf, format="PNG")
    return buf.getvalue()


class EventFileWriter:
    """Appends ``Event`` records to one new event file of ``log_dir`` (created if needed).  ``flush()`` and ``close()`` push the
    buffered records to the file; a context manager.  Calls may come from several threads."""

    def __init__(self, log_dir):
        os.makedirs(log_dir, exist_ok=True)
        stem = os.path.join(str(log_dir), "events.out.tfevents.%010d.%s.%d" % (int(time.time()), socket.gethostname(), os.getpid()))
        uid = 0
        while os.path.exists(f"{stem}.{uid}"):             # a second writer of this process within the same second
            uid += 1
        self.path = f"{stem}.{uid}"
        self._lock = threading.Lock()
        self._file = open(self.path, "wb")
        self.add_record(encode_event(time.time(), file_version=FILE_VERSION))
        self.flush()

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        self.close()
        return False

    def add_record(self, payload):
        header = struct.pack("<Q", len(payload))
        record = header + struct.pack("<I", masked_crc32c(header)) + payload + struct.pack("<I", masked_crc32c(payload))
        with self._lock:
            if self._file is None:
                raise RuntimeError("EventFileWriter: write after close()")
            self._file.write(record)

    def add_event(self, step, values, wall_time=None):
        self.add_record(encode_event(time.time() if wall_time is None else wall_time, step=step, values=values))

    def add_scalars(self, step, scalars, wall_time=None):
        """One event holding ``scalars`` = {tag: value}."""
        self.add_event(step, [scalar_value(t, v) for t, v in scalars.items()], wall_time)

    def add_images(self, step, images, wall_time=None):
        """One event holding ``images`` = [(tag, [n,h,w,1 or 3] uint8), ...], each tag as its n images."""
        self.add_event(step, image_values(images), wall_time)

    def flush(self):
        with self._lock:
            if self._file is not None:
                self._file.flush()

    def close(self):
        with self._lock:
            if self._file is not None:
                self._file.close()
                self._file = None


def image_values(images):
    values = []
    for tag, batch in images:
        batch = np.asarray(batch)
        for name, im in zip(image_tags(tag, len(batch)), batch):
            values.append(image_value(name, im.shape[0], im.shape[1], im.shape[2], encode_png(im)))
    return values


# ------------------------------------------------------------------------------ the training loop's writer
class _Slot:
    """One entry of the ring: the kernel's device buffer, its pinned host copy and the event that says the copy is done."""

    def __init__(self, nbytes, dev):
        import torch
        self.dev = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        self.event = torch.cuda.Event()


class TrainSummaryWriter:
    """The summaries of a training run in one event file of ``log_dir``.

    ``scalars(step, loss, rmse_log)`` appends the tags ``loss`` and ``RMSE_log``.  ``images(step, data, pyramid, camera)``
    draws, for the first ``max_outputs`` samples of the batch, ``RGB_im`` (the last frame), ``camera_prev_t_reproj`` (the
    previous frame warped by ``depth_operations.reproject`` with the last frame's ground-truth depth and pose), ``depth_gt`` and
    ``depth_lvl_i`` of every level of ``pyramid`` (finest first, each at its own resolution; both log-depth images are
    log(clip(d, 1, 200)) / log(200)).  It enqueues the warp, one ``summary_images`` launch, the copy into a pinned slot and an
    event on the caller's current stream and returns: once it has, the caller may overwrite the tensors it passed (the next
    graph replay) on that stream.  One of ``threads`` host threads waits for the event, compresses and appends ONE event with
    all images of the step.  The ring has ``slots`` entries and does not grow: ``images`` blocks while all are in flight.
    Events reach the file in the order of the calls, whichever thread finishes first.  ``close()`` drains the ring and
    re-raises the first exception a worker hit.  All calls must come from one thread and one stream, with one geometry."""

    def __init__(self, log_dir, max_outputs=3, slots=2, threads=2):
        if max_outputs < 1 or slots < 1 or threads < 1:
            raise ValueError("max_outputs, slots and threads must be >= 1")
        self.max_outputs, self.n_slots = int(max_outputs), int(slots)
        self.events = EventFileWriter(log_dir)
        self.path = self.events.path
        self._pool = ThreadPoolExecutor(max_workers=int(threads), thread_name_prefix="m4d-summary")
        self._free = queue.Queue()
        self._slots = None                                 # allocated at the first images() (the geometry is the step's)
        self._shapes = None
        self._lock = threading.Lock()
        self._tickets = 0                                  # events handed in so far, in call order
        self._next = 0                                     # the ticket the file waits for
        self._done = {}                                    # ticket -> record payload (None: dropped) finished out of turn
        self._error = None
        self._closed = False

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:                                              # the body's exception wins; still leave nothing in flight
            try:
                self.close()
            except Exception:
                pass
        return False

    def _ticket(self):
        if self._closed:
            raise RuntimeError("TrainSummaryWriter: write after close()")
        t = self._tickets
        self._tickets += 1
        return t

    def _emit(self, ticket, payload):
        """Hands the finished event of ``ticket`` over; it and every finished successor goes to the file once its turn comes."""
        with self._lock:
            self._done[ticket] = payload
            while self._next in self._done:
                ready = self._done.pop(self._next)
                self._next += 1
                if ready is not None:
                    self.events.add_record(ready)

    def scalars(self, step, loss, rmse_log=None):
        """``rmse_log`` None: the batch has no ground truth, only the loss is written."""
        values = [scalar_value("loss", loss)] + ([] if rmse_log is None else [scalar_value("RMSE_log", rmse_log)])
        self._emit(self._ticket(), encode_event(time.time(), step=int(step), values=values))

    # -- the device side: replaced by stand-ins in the host tests
    def _make_slot(self, nbytes, dev):
        return _Slot(nbytes, dev)

    @staticmethod
    def _geometry(data, pyramid, has_gt=True):
        """(tags, [(h, w, c), ...]) of the step's maps; without ground truth the two images made of it are left out."""
        H, W = data["RGB_im"].shape[2:4]
        gt_tags, gt_shapes = (["camera_prev_t_reproj", "depth_gt"], [(H, W, 3), (H, W, 1)]) if has_gt else ([], [])
        tags = ["RGB_im"] + gt_tags + [f"depth_lvl_{i}" for i in range(len(pyramid))]
        return tags, [(H, W, 3)] + gt_shapes + [tuple(p.shape[1:]) for p in pyramid]

    def _render(self, slot, data, pyramid, camera, n, has_gt=True):
        """Enqueues the step's images into ``slot`` on the current stream and records its event; returns the host views
        [n,h,w,c] uint8 of the maps, valid once the event has completed."""
        from . import network_ops as nops
        from .depth_operations import reproject
        rgb, depth = data["RGB_im"], data["depth"]
        if not has_gt:
            maps = [rgb[:, -1]] + list(pyramid)
            nops.summary_images(maps, ["unit"] + ["log_depth"] * len(pyramid), n, out=slot.dev)
            slot.host.copy_(slot.dev, non_blocking=True)
            slot.event.record()
            offsets, _ = nops.summary_layout([tuple(m.shape[1:]) for m in maps], n)
            return [slot.host[o:o + n * m[0].numel()].view(n, *m.shape[1:]) for o, m in zip(offsets, maps)]
        reproj, _ = reproject(rgb[:n, -2], depth[:n, -1], data["rot"][:n, -1], data["trans"][:n, -1],
                              {k: v[:n] for k, v in camera.items()})                 # m4depth_network.py:405-406
        maps = [rgb[:, -1], reproj, depth[:, -1]] + list(pyramid)
        nops.summary_images(maps, ["unit", "unit", "log_depth"] + ["log_depth"] * len(pyramid), n, out=slot.dev)
        slot.host.copy_(slot.dev, non_blocking=True)
        slot.event.record()
        offsets, _ = nops.summary_layout([tuple(m.shape[1:]) for m in maps], n)
        return [slot.host[o:o + n * m[0].numel()].view(n, *m.shape[1:]) for o, m in zip(offsets, maps)]

    def images(self, step, data, pyramid, camera, has_gt=True):
        """``data``: the step's [b,T,...] device batch (``RGB_im``, ``depth``, ``rot``, ``trans``), T >= 2; ``pyramid``: the last
        frame's depth estimates [b,h_i,w_i,1], finest first; ``camera``: {'f', 'c'} [b,2].  ``has_gt`` False (a batch without
        ground truth): ``RGB_im`` and ``depth_lvl_i`` only -- ``camera_prev_t_reproj`` and ``depth_gt`` are made of it."""
        shape = tuple(data["RGB_im"].shape)
        if len(shape) != 5 or shape[1] < 2 or not 1 <= len(pyramid) <= 13:
            raise ValueError(f"images: expected a [b,T>=2,H,W,3] batch and 1..13 levels, got RGB_im {shape}, {len(pyramid)} levels")
        n = min(self.max_outputs, shape[0])
        tags, shapes = self._geometry(data, pyramid, has_gt)
        if self._slots is None:
            from .network_ops import summary_layout
            nbytes = summary_layout(shapes, n)[1]
            self._slots = [self._make_slot(nbytes, getattr(data["RGB_im"], "device", None)) for _ in range(self.n_slots)]
            self._shapes = shapes
            for i in range(self.n_slots):
                self._free.put(i)
        if shapes != self._shapes:
            raise ValueError(f"images: maps of sizes {shapes}, the writer was sized for {self._shapes}")
        ticket = self._ticket()
        index = self._free.get()                           # back-pressure: waits while every slot is in flight
        try:
            # (the sixth argument only when it is not the default: stand-ins of _render keep the five-argument form)
            views = self._render(self._slots[index], data, pyramid, camera, n, *(() if has_gt else (False,)))
        except BaseException:
            self._free.put(index)
            self._emit(ticket, None)
            raise
        self._pool.submit(self._work, index, ticket, int(step), time.time(), list(zip(tags, views)))

    def _work(self, index, ticket, step, wall_time, views):
        payload = None
        try:
            self._slots[index].event.synchronize()
            payload = encode_event(wall_time, step=step, values=image_values(views))
        except BaseException as e:                         # kept for close(); the slot is freed and the turn passed on all the same
            with self._lock:
                if self._error is None:
                    self._error = e
        finally:
            self._free.put(index)
            try:
                self._emit(ticket, payload)
                self.events.flush()
            except BaseException as e:
                with self._lock:
                    if self._error is None:
                        self._error = e

    def close(self):
        """Waits for every slot, stops the workers, closes the file and re-raises the first worker exception."""
        if self._closed:
            return
        self._closed = True
        if self._slots is not None:
            for _ in range(self.n_slots):
                self._free.get()
        self._pool.shutdown(wait=True)
        self.events.close()
        if self._error is not None:
            raise self._error
