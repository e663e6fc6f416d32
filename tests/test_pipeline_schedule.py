"""The issue order of ``DepthEstimatorPyramid._forward_pipelined`` against a recorded snapshot (CPU only).

Streams, events, the levels, the encoder and the pyramid reset are replaced by stand-ins that log what the method does with
them: the ordered list of level / encoder / reset launches with their stream, and every ``Event.record`` and
``Stream.wait_event``.  That order IS the capture order of the hipGraph every benchmark number comes from.
``tests/golden/pipeline_schedule_snapshot.json`` was recorded this way at commit 60d4868 (default settings)."""
import contextlib
import json
import os

import numpy as np
import torch

from m4depth_amd import network as N

SNAPSHOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipeline_schedule_snapshot.json")
# name: (levels, new_traj per frame, frames encoded before the decoder)
CASES = {
    "reset_full_full_full": (6, [True, False, False, False], 2),
    "reset_in_the_middle": (6, [True, False, True, False], 2),
    "no_reset_3_levels": (3, [False, False, False, False], 2),
    "whole_encoder_up_front": (6, [True, False, False, False], 4),
    "reset_then_two": (6, [True, False, False], 2),
}


def record_schedule(n_lvls, resets, split, monkeypatch):
    log = []
    counter = {"stream": 0, "event": 0}

    class Stream:
        def __init__(self):
            self.id = counter["stream"]
            counter["stream"] += 1

        def wait_event(self, ev):
            log.append(["wait", self.id, ev.id])

    class Event:
        def __init__(self, **_kw):
            self.id = counter["event"]
            counter["event"] += 1

        def record(self, stream=None):
            log.append(["record", self.id, (stream or current[-1]).id])

    current = [Stream()]                              # stream 0 = the calling stream

    @contextlib.contextmanager
    def on_stream(st):
        current.append(st)
        try:
            yield
        finally:
            current.pop()
    monkeypatch.setattr(torch.cuda, "Stream", Stream)
    monkeypatch.setattr(torch.cuda, "Event", Event)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: current[-1])
    monkeypatch.setattr(torch.cuda, "stream", on_stream)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)

    class Maps:
        """A stacked feature map of frames first, first + 1, ...: a batch slice names its frame."""
        def __init__(self, first, lvl):
            self.first, self.lvl = first, lvl

        def __getitem__(self, s):
            return ("f", self.first + s.start, self.lvl)

    def level_forward(self, curr_f_maps, prev_l_est, rot, trans, camera, new_traj, **kw):
        assert curr_f_maps[2] == self.lvl_depth - 1
        assert (prev_l_est is None) == (self.lvl_depth == n_lvls)
        log.append(["level", curr_f_maps[1], self.lvl_depth, current[-1].id])
        return {"depth": (curr_f_maps[1], self.lvl_depth)}
    monkeypatch.setattr(N.DepthEstimatorLevel, "forward", level_forward)
    pyr = N.DepthEstimatorPyramid({"nbre_lvls": n_lvls, "is_training": False, "ablation": N.M4depthAblationParameters()})

    def reset_all(f_pyr, new_traj):
        if not bool(np.asarray(new_traj).reshape(-1)[0]):
            return None
        log.append(["reset", f_pyr[0][1], current[-1].id])
        return [{"depth": (f_pyr[0][1], n_lvls - l)} for l in range(n_lvls)]
    pyr._reset_all_levels = reset_all
    pyr.prenormalize = lambda tail, bsz: None
    n_fr = len(resets)
    samples = [{"RGB_im": torch.full((1, 2, 2, 3), float(t)), "rot": None, "trans": None, "new_traj": np.array([r])}
               for t, r in enumerate(resets)]

    def encoder(images):
        first = int(images[0, 0, 0, 0])
        log.append(["encoder", first, images.shape[0], current[-1].id])
        return [Maps(first, lvl) for lvl in range(n_lvls)]
    f_pyrs = [[("f", t, lvl) for lvl in range(n_lvls)] for t in range(split)] + [None] * (n_fr - split)
    out = pyr._forward_pipelined(f_pyrs, samples, [None] * n_lvls, n_fr, encoder, None)
    return {"log": log, "estimates": [[list(est["depth"]) for est in ests] for ests in out]}


def test_pipelined_forward_issues_the_recorded_schedule(monkeypatch):
    with open(SNAPSHOT) as fh:
        want = json.load(fh)
    assert sorted(want) == sorted(CASES)
    for name, (n_lvls, resets, split) in CASES.items():
        with monkeypatch.context() as mp:
            got = record_schedule(n_lvls, resets, split, mp)
        assert got["estimates"] == want[name]["estimates"], name
        for i, (g, w) in enumerate(zip(got["log"], want[name]["log"])):
            assert g == w, (name, i, g, w)
        assert len(got["log"]) == len(want[name]["log"]), name
