"""Batched streaming evaluation: whole trajectories dealt into B parallel slots (host logic, no device).

The reference evaluates Mid-Air and TartanAir by streaming: every trajectory is fed one frame at a time, the network state
carries over from frame to frame, and each frame's 7 metrics are added to a Keras ``Mean`` unless the frame opens a trajectory
(m4depth_network.py:433-474, dataloaders/generic.py:128-146).  Sample s of ``M4Depth.stream_step`` is exactly a stream of its
own, so B trajectories can run side by side:

  * ``schedule`` deals the trajectories into B slots.  A slot whose trajectory ends takes the next unassigned one at the next
    step; the first frame of every assignment gets a forced reset.  Once no trajectory is left, an idle slot repeats its last
    frame with the reset set and ``active`` clear: the batch keeps its size (a change of geometry would reset every sample and
    re-capture the graphs) and nothing is decoded for it.
  * The device scores every sample of every step on its own (``network_ops.depth_metrics_per_sample``) into an
    [n_steps, B, 7] log, with a per-cell ``counted`` flag = active and not the frame's own new_traj (csv ``id == 0``).
  * ``fold`` walks that log in the sequential run's order -- trajectory in csv order, frame in order -- and sums the counted
    rows in float32, as the metric kernel adds each frame to the Keras-Mean totals: the same (total, count), bit for bit.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

POLICIES = ("lpt", "arrival")

# cells [n_steps, B, 2] int64: (trajectory, frame) scored at (step, slot), -1 for an idle slot
# feed  [n_steps, B, 2] int64: the frame the slot is fed -- the cell itself, or the slot's last frame when it is idle
# reset [n_steps, B] bool: the forced reset of the first frame of each assignment, and every idle cell
Schedule = namedtuple("Schedule", ("cells", "feed", "reset", "n_slots", "order"))


def _order(lengths, policy):
    idx = [i for i, n in enumerate(lengths) if n > 0]
    if policy == "lpt":                              # longest first (stable: ties keep csv order) -- shortens the tail
        return sorted(idx, key=lambda i: -lengths[i])
    if policy == "arrival":
        return idx
    raise ValueError(f"schedule: policy must be one of {POLICIES}, got {policy!r}")


def schedule(traj_lengths, n_slots, policy="lpt"):
    """Deal trajectories of ``traj_lengths`` frames into ``min(n_slots, n_traj)`` slots.  Returns a ``Schedule``; its
    ``cells`` table holds every (trajectory, frame) exactly once, frames in order within a slot, idle cells only after a
    slot's last assignment.  Trajectories of length 0 are skipped."""
    lengths = [int(n) for n in traj_lengths]
    if any(n < 0 for n in lengths):
        raise ValueError("schedule: negative trajectory length")
    if int(n_slots) < 1:
        raise ValueError(f"schedule: n_slots must be >= 1, got {n_slots}")
    order = _order(lengths, policy)
    B = min(int(n_slots), len(order))
    if B == 0:
        empty = np.zeros((0, 0, 2), np.int64)
        return Schedule(empty, empty.copy(), np.zeros((0, 0), bool), 0, order)
    # list scheduling: each slot's (trajectory, start step) assignments; a slot frees at the end of its trajectory
    free_at = [0] * B
    assign = [[] for _ in range(B)]
    for t in order:
        s = min(range(B), key=lambda k: (free_at[k], k))
        assign[s].append((t, free_at[s]))
        free_at[s] += lengths[t]
    n_steps = max(free_at)
    cells = np.full((n_steps, B, 2), -1, np.int64)
    feed = np.empty((n_steps, B, 2), np.int64)
    reset = np.zeros((n_steps, B), bool)
    for s in range(B):
        for t, start in assign[s]:
            n = lengths[t]
            cells[start:start + n, s, 0] = t
            cells[start:start + n, s, 1] = np.arange(n)
            reset[start, s] = True
        end = free_at[s]
        feed[:end, s] = cells[:end, s]
        feed[end:, s] = cells[end - 1, s]            # idle tail: the slot's last frame again, reset, not active
        reset[end:, s] = True
    return Schedule(cells, feed, reset, B, order)


def makespan(sched):
    return int(sched.cells.shape[0])


def fold(rows, counted, cells, traj_order=None):
    """The Keras ``Mean`` state of the sequential run from the per-sample log: ``rows`` [n_steps,B,7] float32, ``counted``
    [n_steps,B] (nonzero = counted), ``cells`` the schedule's [n_steps,B,2] table.  Walks (trajectory in ``traj_order``,
    default ascending = csv order; frame in order) and sums the counted rows as ``total = float32(total + v)`` -- what
    metrics_finalize_kernel does once per frame.  Returns (total float32 [7], count); the result is
    ``float32(total) / float32(count)``."""
    rows = np.asarray(rows, np.float32)
    counted = np.asarray(counted)
    cells = np.asarray(cells)
    if rows.shape[:2] != cells.shape[:2] or counted.shape != cells.shape[:2] or rows.shape[2:] != (7,):
        raise ValueError(f"fold: rows {rows.shape}, counted {counted.shape} and cells {cells.shape} disagree")
    live = cells[..., 0] >= 0
    st, sl = np.nonzero(live)
    tr, fr = cells[st, sl, 0], cells[st, sl, 1]
    if traj_order is None:
        rank = tr
    else:
        pos = {int(t): i for i, t in enumerate(traj_order)}
        rank = np.array([pos[int(t)] for t in tr], np.int64)
    walk = np.lexsort((fr, rank))                    # trajectory, then frame
    total = np.zeros(7, np.float32)
    count = 0
    for k in walk:
        if counted[st[k], sl[k]]:
            total = (total + rows[st[k], sl[k]]).astype(np.float32)
            count += 1
    return total, count


def fold_consistency(rows, counted, cells, traj_order=None):
    """``fold`` for the 6-column log of ``consistency.ConsistencyScorer`` (``consistency.COLUMNS``): the same sequential walk
    (trajectory in ``traj_order``, default ascending = csv order; frame in order), the counted rows summed as ``total =
    float32(total + v)``.  Returns (total float32 [6], count, frames) with ``frames`` the counted (trajectory, frame, row)
    triples in the walk's order -- the per-frame file of ``main.py --consistency``."""
    rows = np.asarray(rows, np.float32)
    counted = np.asarray(counted)
    cells = np.asarray(cells)
    if rows.shape[:2] != cells.shape[:2] or counted.shape != cells.shape[:2] or rows.shape[2:] != (6,):
        raise ValueError(f"fold: rows {rows.shape}, counted {counted.shape} and cells {cells.shape} disagree")
    live = cells[..., 0] >= 0
    st, sl = np.nonzero(live)
    tr, fr = cells[st, sl, 0], cells[st, sl, 1]
    if traj_order is None:
        rank = tr
    else:
        pos = {int(t): i for i, t in enumerate(traj_order)}
        rank = np.array([pos[int(t)] for t in tr], np.int64)
    walk = np.lexsort((fr, rank))                    # trajectory, then frame
    total = np.zeros(6, np.float32)
    count = 0
    frames = []
    for k in walk:
        if counted[st[k], sl[k]]:
            total = (total + rows[st[k], sl[k]]).astype(np.float32)
            count += 1
            frames.append((int(tr[k]), int(fr[k]), rows[st[k], sl[k]].copy()))
    return total, count, frames


def fold_fused(rows, rows_f, hits, counted, cells, pixels, traj_order=None):
    """The per-frame rows of ``main.py --fused`` from the raw and the fused 7-column logs (``rows``, ``rows_f`` [n_steps,B,7]) and
    the [n_steps,B] log of rendered pixels, in the same sequential walk (trajectory in ``traj_order``, default ascending = csv
    order; frame in order): the counted (trajectory, frame, float32 [coverage = hits / pixels, AbsRel raw, AbsRel fused])
    triples -- the frames the seven metrics count."""
    rows, rows_f = np.asarray(rows, np.float32), np.asarray(rows_f, np.float32)
    hits, counted, cells = np.asarray(hits), np.asarray(counted), np.asarray(cells)
    if rows.shape != rows_f.shape or rows.shape[:2] != cells.shape[:2] or rows.shape[2:] != (7,) \
            or counted.shape != cells.shape[:2] or hits.shape != cells.shape[:2]:
        raise ValueError(f"fold: rows {rows.shape} / {rows_f.shape}, hits {hits.shape}, counted {counted.shape} and cells "
                         f"{cells.shape} disagree")
    st, sl = np.nonzero(cells[..., 0] >= 0)
    tr, fr = cells[st, sl, 0], cells[st, sl, 1]
    if traj_order is None:
        rank = tr
    else:
        pos = {int(t): i for i, t in enumerate(traj_order)}
        rank = np.array([pos[int(t)] for t in tr], np.int64)
    walk = np.lexsort((fr, rank))                    # trajectory, then frame
    return [(int(tr[k]), int(fr[k]), np.array([np.float32(hits[st[k], sl[k]]) / np.float32(pixels), rows[st[k], sl[k], 0],
                                               rows_f[st[k], sl[k], 0]], np.float32))
            for k in walk if counted[st[k], sl[k]]]


def fold_pose_refine(rows, cells, traj_order=None):
    """The per-frame rows of ``pose_refine.PoseRefiner`` (``pose_refine.COLUMNS``) from its [n_steps,B,8] log, in the same
    sequential walk (trajectory in ``traj_order``, default ascending = csv order; frame in order): the (trajectory, frame, row)
    triples of every frame but a trajectory's first, which has no frame before it -- the frames ``--consistency`` scores."""
    rows = np.asarray(rows, np.float32)
    cells = np.asarray(cells)
    if rows.shape[:2] != cells.shape[:2] or rows.shape[2:] != (8,):
        raise ValueError(f"fold: rows {rows.shape} and cells {cells.shape} disagree")
    st, sl = np.nonzero((cells[..., 0] >= 0) & (cells[..., 1] >= 1))
    tr, fr = cells[st, sl, 0], cells[st, sl, 1]
    if traj_order is None:
        rank = tr
    else:
        pos = {int(t): i for i, t in enumerate(traj_order)}
        rank = np.array([pos[int(t)] for t in tr], np.int64)
    walk = np.lexsort((fr, rank))                    # trajectory, then frame
    return [(int(tr[k]), int(fr[k]), rows[st[k], sl[k]].copy()) for k in walk]


def fold_result(total, count):
    """``float32(total) / float32(count)`` (count 0 -> the totals themselves, as the writer's clamp to 1 gives)."""
    return (np.asarray(total, np.float32) / np.float32(max(int(count), 1))).astype(np.float32)
