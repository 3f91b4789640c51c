"""The rule of mnav_fleet_timed_traffic (include/mnav.h) in numpy, on top of tests/fleet_model.py:
FM.run gives every robot its code, potential and path; the fields carry dist.  A contributor visits its own vertex and every
id of its path down to the seed; each visit falls into the window of the time at which the robot reaches it -- float32 steps
written one by one -- adds the robot's weight to the cell and lowers the cell's holder to the robot's key.  The report is taken
on the cells as they stand after all adds.  tests/test_timed_traffic_model.py pins the header's host mirror against it,
tests/test_gpu_timed_traffic.py the device."""
from __future__ import annotations

import numpy as np

from tests import fleet_model as FM
from tests import traffic_model as TM

MAX_TOTAL = TM.MAX_TOTAL
MAX_WINDOWS = 1024
NONE = FM.NONE
F = np.float32


class Cells:
    """the context's state: V x B cells and holders (None before the first call), their configuration and T"""

    def __init__(self, V: int):
        self.V, self.B, self.tau, self.T = V, 0, None, 0
        self.cell = self.holder = None

    @property
    def peak(self):
        return np.zeros(self.V, np.uint32) if self.cell is None else self.cell.max(axis=1).astype(np.uint32)

    @property
    def window(self):
        """the smallest window that attains the peak, NONE where the peak is 0"""
        if self.cell is None:
            return np.full(self.V, NONE, np.uint32)
        return np.where(self.peak > 0, self.cell.argmax(axis=1), NONE).astype(np.uint32)


def visit_time(P, d_u, depart, pace):
    """t of a visit: float32 arrays (or scalars), one operation at a time"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        dt = np.fmax((np.asarray(P, F) - np.asarray(d_u, F)).astype(F), F(0)).astype(F)
        along = (dt * np.asarray(pace, F)).astype(F)
        return (np.asarray(depart, F) + along).astype(F)


def window_of(t, tau, B: int):
    """(in the horizon, window) of float32 times: q = t / (float) tau, in iff q < (float) B, window = trunc(q)"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        q = (np.asarray(t, F) / F(tau)).astype(F)
    inside = q < F(B)
    return inside, np.where(inside, q, F(0)).astype(np.uint32)


def refused(state: Cells, n, weights, depart, pace, B, tau, accumulate) -> bool:
    if not 1 <= B <= MAX_WINDOWS:
        return True
    with np.errstate(over="ignore", under="ignore"):
        tf = np.float64(tau).astype(F)
    if not np.isfinite(tf) or not tf > 0:
        return True
    if depart is not None and not (np.isfinite(depart) & (np.asarray(depart) >= 0)).all():
        return True
    if pace is not None and not (np.isfinite(pace) & (np.asarray(pace) > 0)).all():
        return True
    if accumulate and state.cell is not None and (state.B != B or state.tau != tf):
        return True
    total = n if weights is None else int(np.asarray(weights, np.uint32).astype(np.uint64).sum())
    return total + (state.T if accumulate else 0) > MAX_TOTAL


def timed(state: Cells, fields, slots, vtx, weights=None, depart=None, pace=None, key=None, B=64, tau=1.0, free_count=0, accumulate=False, run=None):
    """one mnav_fleet_timed_traffic call on `state`.  Returns None (state untouched) where the call refuses, else the
    call's outputs and statistics.  run: FM.run(fields, V, slots, vtx) when the caller has it already."""
    n, V = len(slots), state.V
    if refused(state, n, weights, depart, pace, B, tau, accumulate):
        return None
    with np.errstate(over="ignore", under="ignore"):
        tf = np.float64(tau).astype(F)
    w = np.ones(n, np.uint32) if weights is None else np.asarray(weights, np.uint32)
    dep = np.zeros(n, F) if depart is None else np.asarray(depart, F)
    pc = np.ones(n, F) if pace is None else np.asarray(pace, F)
    ky = np.arange(n, dtype=np.uint32) if key is None else np.asarray(key, np.uint32)
    r = FM.run(fields, V, slots, vtx) if run is None else run
    on = TM.contributes(r["codes"], r["potential"]) & (w > 0)
    off = r["offsets"].astype(np.int64)
    # the visits of the contributors, robot by robot, each from its vertex down to the seed
    who, us, ds = [], [], []
    for i in np.flatnonzero(on):
        path = np.concatenate(([int(vtx[i])], r["ids"][off[i]:off[i + 1]][::-1])).astype(np.int64)
        who.append(np.full(path.size, i, np.int64))
        us.append(path)
        ds.append(np.asarray(fields[int(slots[i])].dist, F)[path])
    who, us = (np.concatenate(a) if a else np.zeros(0, np.int64) for a in (who, us))
    ds = np.concatenate(ds) if ds else np.zeros(0, F)
    t = visit_time(r["potential"][who], ds, dep[who], pc[who])
    inside, k = window_of(t, tf, B)
    if accumulate and state.cell is not None:
        cell, holder, T = state.cell.astype(np.int64).ravel(), state.holder.copy().ravel(), state.T
    else:
        cell, holder, T = np.zeros(V * B, np.int64), np.full(V * B, NONE, np.uint32), 0
    idx = us[inside] * B + k[inside].astype(np.int64)
    np.add.at(cell, idx, w[who[inside]].astype(np.int64))
    np.minimum.at(holder, idx, ky[who[inside]])
    assert cell.max(initial=0) <= MAX_TOTAL
    state.cell, state.holder = cell.astype(np.uint32).reshape(V, B), holder.reshape(V, B)
    state.B, state.tau, state.T = B, tf, T + int(w[on].sum())
    # the report, on the cells as they now stand
    over = state.cell.ravel()[idx] > np.uint32(free_count)
    yields = over & (state.holder.ravel()[idx] != ky[who[inside]])
    robot = who[inside]
    conflict = np.bincount(robot[over], minlength=n).astype(np.uint32)
    yl = np.bincount(robot[yields], minlength=n).astype(np.uint32)
    fv, fw, ft = np.full(n, NONE, np.uint32), np.full(n, NONE, np.uint32), np.full(n, np.inf, F)
    first_robot, first_at = np.unique(robot[yields], return_index=True)       # visits are in robot order, then in visit order
    at = np.flatnonzero(yields)[first_at]
    fv[first_robot], fw[first_robot], ft[first_robot] = us[inside][at], k[inside][at], t[inside][at]
    return dict(codes=r["codes"], potential=r["potential"], conflict_hops=conflict, yield_hops=yl, first_yield_vertex=fv, first_yield_window=fw,
                first_yield_time=ft, contributing=int(on.sum()), adds=int(inside.sum()), beyond_horizon=int((~inside).sum()), weight=int(w[on].sum()),
                total_weight=state.T, occupied_cells=int((state.cell > 0).sum()), over_cells=int((state.cell > np.uint32(free_count)).sum()),
                largest_cell=int(state.cell.max(initial=0)), yielding=int((yl > 0).sum()), windows=B)
