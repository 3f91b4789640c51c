"""The rules of mnav_fleet_traffic and mnav_layer_traffic (include/mnav.h) in numpy, on top of
tests/fleet_model.py: a robot contributes iff the fleet rule serves it with a finite potential; it adds its weight to its
own vertex and to every id of its path.  tests/test_traffic_model.py pins the header's host mirror against it,
tests/test_gpu_traffic.py the device."""
from __future__ import annotations

import numpy as np

from tests import fleet_model as FM

MAX_TOTAL = 2 ** 32 - 1


class Counts:
    """the context's state: V uint32 counts and T, the total of the accumulated weight"""

    def __init__(self, V: int):
        self.V, self.c, self.T = V, np.zeros(V, np.uint32), 0


def contributes(codes, potential):
    return (np.asarray(codes) == FM.SUCCESS) & np.isfinite(np.asarray(potential, np.float32))


def traffic(state: Counts, fields, slots, vtx, weights=None, accumulate=False):
    """one mnav_fleet_traffic call on `state`.  Returns None (state untouched) when the weights do not fit the counters,
    else dict(codes, potential, contributing, adds, total_weight, occupied, peak) -- the call's outputs and statistics."""
    n = len(slots)
    w = np.ones(n, np.uint32) if weights is None else np.asarray(weights, np.uint32)
    if int(w.astype(np.uint64).sum()) + (state.T if accumulate else 0) > MAX_TOTAL:
        return None
    r = FM.run(fields, state.V, slots, vtx)
    on = contributes(r["codes"], r["potential"]) & (w > 0)
    off = r["offsets"].astype(np.int64)
    c = state.c.astype(np.int64) if accumulate else np.zeros(state.V, np.int64)
    vt = np.asarray(vtx, np.int64)
    np.add.at(c, vt[on], w[on])                                          # the robots' own vertices
    per_id = np.repeat(np.where(on, w, 0).astype(np.int64), np.diff(off))
    np.add.at(c, r["ids"].astype(np.int64), per_id)                      # every id of their paths
    assert c.max(initial=0) <= MAX_TOTAL
    state.c = c.astype(np.uint32)
    state.T = (state.T if accumulate else 0) + int(w[on].sum())
    return dict(codes=r["codes"], potential=r["potential"], contributing=int(on.sum()),
                adds=int((r["path_len"].astype(np.int64)[on] + 1).sum()), weight=int(w[on].sum()), total_weight=state.T,
                occupied=int((state.c > 0).sum()), peak=int(state.c.max(initial=0)))


def cost(counts, free_count: int, gain: float, cap: float):
    """the cost rule: e = c - free_count where c is above it; 0.0f for e == 0, else fminf((float) e * (float) gain, (float) cap)"""
    c = np.asarray(counts, np.uint32)
    e = np.where(c > np.uint32(free_count), c - np.uint32(free_count), np.uint32(0)).astype(np.uint32)
    with np.errstate(over="ignore", under="ignore"):
        x = np.minimum(e.astype(np.float32) * np.float64(gain).astype(np.float32), np.float64(cap).astype(np.float32)).astype(np.float32)
    return np.where(e == 0, np.float32(0), x).astype(np.float32)


def changed(old_cost, old_lethal, new_cost, fresh: bool):
    """the ascending ids mnav_layer_traffic reports: every vertex of a fresh slot, else where the cost bits or the flag differ"""
    if fresh:
        return np.arange(len(new_cost), dtype=np.uint32)
    diff = (FM.bits(old_cost) != FM.bits(new_cost)) | (np.asarray(old_lethal) != 0)
    return np.flatnonzero(diff).astype(np.uint32)
