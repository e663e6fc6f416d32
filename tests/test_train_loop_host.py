"""The training loop of the driver (main.train_loop) on stand-ins for the stepper, the checkpoint writer and the summary
writer: the order of steps, log reads, reports, images and saves.  No GPU; the real steppers are held to the same interface by
tests/test_gpu_train_workflow.py and tests/test_gpu_summaries.py."""
import os

import numpy as np
import pytest
import torch

from m4depth_amd import main as M


def _args(*extra):
    return M.build_parser().parse_args(["--mode", "train", "--summary_interval", "2", "--save_every", "3", *extra])


def _epochs(n=2, per_epoch=4):
    return n, lambda epoch: iter(range(per_epoch))


class Stepper:
    """graph=False: every step returns its row, or marks itself bad.  graph=True: the rows wait for ``read``, which drops those
    from the bad step on and is silent afterwards, as the device-side log is."""
    mode, n_timed = "stand-in", 0

    def __init__(self, ev, graph, step0=0, bad_step=None):
        self.ev, self.graph, self.bad_step, self.bad = ev, graph, bad_step, None
        self.taken = self.logged = step0

    def _rows(self, steps):
        good = [s for s in steps if self.bad_step is None or s < self.bad_step]
        if len(good) < len(steps):
            self.bad = self.bad_step
        return [(s, 1.0 / s, 0.5) for s in good]

    def step(self, data):
        self.taken += 1
        self.ev.append(("step", self.taken))
        return [] if self.graph else self._rows([self.taken])

    def read(self):
        if not self.graph or self.bad is not None:
            return []
        rows = self._rows(range(self.logged + 1, self.taken + 1))
        self.logged = self.taken
        self.ev.append(("read", tuple(r[0] for r in rows)))
        return rows

    def images(self, summary, step):
        summary.images(step)


class Ckpts:
    def __init__(self, ev):
        self.ev, self.saved = ev, set()

    def path(self, step):
        return f"ckpt-{step}"

    def save(self, step):
        if step in self.saved:
            return None
        self.saved.add(step)
        self.ev.append(("save", step))
        return self.path(step)


class Summary:
    def __init__(self, ev):
        self.ev = ev

    def scalars(self, step, loss, rmse):
        self.ev.append(("report", step, loss, rmse))

    def images(self, step):
        self.ev.append(("images", step))


def _run(graph, step0=0, bad_step=None, validate=None, args=None):
    ev = []
    rc = M.train_loop(args or _args(), Stepper(ev, graph, step0, bad_step), Ckpts(ev), Summary(ev), _epochs(), step0, 0, validate)
    return rc, [e[:2] for e in ev]


def _of(ev, kind):
    return [e[1] for e in ev if e[0] == kind]


def test_graph_cadence(capsys):
    rc, ev = _run(graph=True)
    assert rc == 0
    assert ev == [("step", 1), ("step", 2), ("read", (1, 2)), ("report", 1), ("report", 2), ("images", 2),
                  ("step", 3), ("read", (3,)), ("report", 3), ("save", 3),
                  ("step", 4), ("read", (4,)), ("report", 4), ("images", 4), ("read", ()),
                  ("step", 5), ("step", 6), ("read", (5, 6)), ("report", 5), ("report", 6), ("images", 6), ("save", 6),
                  ("step", 7), ("step", 8), ("read", (7, 8)), ("report", 7), ("report", 8), ("images", 8), ("read", ()),
                  ("save", 8)]
    out = capsys.readouterr().out.splitlines()
    assert out == [M.format_step(s, 1.0 / s, 0.5) for s in range(1, 9)]        # printed with the values the summary got


def test_eager_cadence():
    rc, ev = _run(graph=False)
    assert rc == 0
    assert ev == [("step", 1), ("report", 1), ("step", 2), ("report", 2), ("images", 2), ("step", 3), ("report", 3), ("save", 3),
                  ("step", 4), ("report", 4), ("images", 4), ("step", 5), ("report", 5), ("step", 6), ("report", 6),
                  ("images", 6), ("save", 6), ("step", 7), ("report", 7), ("step", 8), ("report", 8), ("images", 8), ("save", 8)]


def test_graph_non_finite_step(capsys):
    rc, ev = _run(graph=True, bad_step=5)
    assert rc == 1
    assert ev[-3:] == [("step", 5), ("step", 6), ("read", ())]               # the read after step 6 reports nothing
    assert (_of(ev, "report"), _of(ev, "images"), _of(ev, "save")) == ([1, 2, 3, 4], [2, 4], [3])
    assert capsys.readouterr().out.splitlines()[-1] == \
        "step 5: non-finite loss, training stopped (TerminateOnNaN): nothing of epoch 2 is saved"


def test_eager_non_finite_step(capsys):
    rc, ev = _run(graph=False, bad_step=5)
    assert rc == 1
    assert ev[-1] == ("step", 5)
    assert (_of(ev, "report"), _of(ev, "images"), _of(ev, "save")) == ([1, 2, 3, 4], [2, 4], [3])
    assert "step 5: non-finite loss, training stopped (TerminateOnNaN): nothing of epoch 2 is saved" in capsys.readouterr().out


def test_resumed_run_counts_reads_from_step0_and_saves_from_zero():
    rc, ev = _run(graph=True, step0=7)
    assert rc == 0
    assert _of(ev, "step") == list(range(8, 16))
    # reads: (step - 7) % 2 == 0 at 9, 11, 13, 15; save_every 3 divides 9, 12, 15; the epochs end after 11 and 15
    assert _of(ev, "read") == [(8, 9), (10, 11), (), (12,), (13,), (14, 15), ()]
    assert _of(ev, "images") == [9, 11, 13, 15]
    assert _of(ev, "save") == [9, 12, 15]                                     # 15 was just saved: no final save
    assert ev.index(("read", (8, 9))) < ev.index(("images", 9)) < ev.index(("save", 9))


def test_validation_gets_each_epochs_checkpoint_once():
    seen = []
    rc, ev = _run(graph=True, validate=seen.append)
    assert rc == 0
    assert seen == ["ckpt-4", "ckpt-8"]
    assert _of(ev, "save") == [3, 4, 6, 8]                                    # the final save of step 8 is not repeated
    seen.clear()
    rc, ev = _run(graph=False, validate=seen.append, args=_args("--save_every", "4"))
    assert (rc, seen, _of(ev, "save")) == (0, ["ckpt-4", "ckpt-8"], [4, 8])   # already saved: the path is named, nothing rewritten


class Model:
    def __init__(self, value):
        self.w = torch.full((3,), value)

    def parameters(self):
        return [self.w]

    def numpy_weights(self):
        return {"w": self.w.numpy()}


class Optimizer:
    def state_dict(self):
        return {"state": {}}


@pytest.mark.parametrize("graph", [False, True])
def test_non_finite_parameters_at_a_save_write_nothing(tmp_path, capsys, graph):
    """The real checkpoint writer: finite parameters are written once per step, non-finite ones stop the run at the first due
    save, on every rank, with nothing on disk."""
    args = _args("--ckpt_dir", str(tmp_path / "ok"))
    model, opt = Model(1.0), Optimizer()
    ev = []
    assert M.train_loop(args, Stepper(ev, graph), M.CheckpointWriter(args, model, opt, 0), None, _epochs()) == 0
    assert sorted(os.listdir(tmp_path / "ok" / "train")) == sorted(f"ckpt-{s}{e}" for s in (3, 6, 8) for e in (".npz", ".opt.pt"))
    assert np.array_equal(np.load(tmp_path / "ok" / "train" / "ckpt-8.npz")["w"], np.ones(3, np.float32))
    capsys.readouterr()
    for rank in (0, 1):
        args = _args("--ckpt_dir", str(tmp_path / f"nan{rank}"))
        ev = []
        rc = M.train_loop(args, Stepper(ev, graph), M.CheckpointWriter(args, Model(float("nan")), opt, rank), None, _epochs(),
                          0, rank)
        assert rc == 1 and _of(ev, "step") == [1, 2, 3]
        assert capsys.readouterr().out.splitlines()[-1] == \
            "step 3: non-finite parameters, training stopped: no checkpoint of this state is written"
        assert not os.path.exists(tmp_path / f"nan{rank}")
