"""The rule of mnav_fleet_paths (include/mnav.h) in numpy, over (dist, pred, seed, target,
offset) of each plan: rules 1 to 6, the hop walk, the packed output.  tests/test_fleet_model.py pins it against fresh
plans of the CPU oracle and pins the header's host mirror against it; tests/test_gpu_fleet.py uses it for the robots the
device may call MNAV_BEYOND_FIELD."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

SUCCESS, INVALID_START, INVALID_GOAL, NO_PATH_FOUND, INTERNAL_ERROR, BEYOND_FIELD = 0, 52, 53, 54, 60, 70
NONE = 0xFFFFFFFF
INF = np.float32(np.inf)
BLOCK = 256                 # robots per block of the device's scan (mnav_fleet.h kFleetBlock)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@dataclass
class Field:
    """One plan as the robots see it.  dist None: the plan never reached the device, `code` is its own code."""
    dist: np.ndarray | None
    pred: np.ndarray | None
    seed: int
    target: int
    offset: float
    code: int = SUCCESS


def plan_code(seed: int, target: int, V: int) -> int:
    """what the plan call gives a plan it does not run"""
    return INVALID_START if seed >= V else INVALID_GOAL if target >= V else SUCCESS


def cut_of(dist, target: int, offset: float) -> np.float32:
    """goal_cut(dist[target], offset, target).cut of mnav_eval.h: float(dt + offset) in double, dt itself when that rounds
    below dt, +inf when dt is"""
    dt = np.float32(dist[target])
    if not dt < INF:
        return INF
    goal = np.float32(np.float64(dt) + np.float64(offset))
    return dt if goal < dt else goal


def classify(f: Field, V: int, v: int):
    """(code, path seed first ... pred[v], potential) of one robot on vertex v"""
    none = np.zeros(0, np.uint32)
    if v >= V:
        return INVALID_GOAL, none, INF                                  # rule 1
    if f.dist is None:
        return f.code, none, INF                                        # rule 2
    if v == f.seed:
        return SUCCESS, none, np.float32(0)                             # rule 3
    d = np.float32(f.dist[v])
    cut = cut_of(f.dist, f.target, f.offset)
    if d < cut or v == f.target:                                        # rule 4
        u = int(f.pred[v])
        if u == v:
            return NO_PATH_FOUND, none, d
        hops = [u]
        while u != f.seed:
            w = int(f.pred[u]) if u < V else u
            if w == u or len(hops) >= V:
                return INTERNAL_ERROR, none, INF
            u = w
            hops.append(u)
        return SUCCESS, np.array(hops[::-1], np.uint32), d
    if not d < INF and (not cut < INF or not (np.isfinite(f.dist) & (f.dist >= cut)).any()):
        return NO_PATH_FOUND, none, INF                                 # rule 5: the wave ran out (no reached vertex at or above the cut)
    return BEYOND_FIELD, none, INF                                      # rule 6


def run(fields, V: int, slots, vtx):
    """the whole call: dict(codes, path_len, potential, offsets (n + 1, uint64), ids, counts = served / beyond / no path / invalid)"""
    n = len(slots)
    codes, lens = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    pot = np.zeros(n, np.float32)
    rows = []
    for i in range(n):
        c, p, d = classify(fields[int(slots[i])], V, int(vtx[i]))
        codes[i], lens[i], pot[i] = c, p.size, d
        rows.append(p)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(lens.astype(np.uint64))
    ids = np.concatenate(rows) if rows else np.zeros(0, np.uint32)
    counts = [int((codes == SUCCESS).sum()), int((codes == BEYOND_FIELD).sum()), int((codes == NO_PATH_FOUND).sum())]
    counts.append(n - sum(counts))
    return dict(codes=codes, path_len=lens, potential=pot, offsets=off, ids=ids.astype(np.uint32), counts=counts)


def robots_of(field: Field, V: int, rng, n_random: int):
    """robot vertices for one field: the seed, the target, vertices on the tentative ring (finite, at or above the cut),
    beyond it (never reached although the wave stopped), unreached with an infinite cut, and n_random random ones"""
    d = field.dist
    cut = cut_of(d, field.target, field.offset)
    fin = np.isfinite(d)
    ring = np.flatnonzero(fin & (d >= cut))
    out = np.flatnonzero(~fin)
    pick = [field.seed, field.target]
    for group in (ring, out):
        if group.size:
            pick += list(rng.choice(group, min(4, group.size), replace=False))
    pick += list(rng.integers(0, V, n_random))
    return np.array(pick, np.uint32)
