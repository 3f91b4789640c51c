"""The fleet rollout (mnav_fleet_rollout) in Python / numpy, written from its specification (include/mnav.h), NOT from
mnav_fleet_rollout.h: departures and the separation check.  What tests/test_separation_model.py (CPU, against the header
compiled for the host) and tests/test_gpu_fleet_rollout.py (device) compare with.

Departures: robots are independent, so robot i of a call over `ticks` ticks with start tick s is robot i of
tests/rollout_model.py run for ticks - min(s, ticks) ticks, its trace moved down by s rows.  The check: O(n^2) brute force
over positions and presence, float32 with every operation rounded on its own."""
import numpy as np

from tests import follow_model as FM
from tests import rollout_model as RM

F32 = np.float32
NONE = 0xFFFFFFFF
WAITING_PRESENT, REACHED_PRESENT = 1, 2
SEP_KEYS = ("near_checks", "max_partners", "first_near_tick", "first_near_robot", "min_sep2", "min_sep_tick", "min_sep_robot")


def departures(model, cfg, fields, robots, goals, dt, ticks, dist_tol, ang_tol, start_tick=None):
    """The state outputs (RM.KEYS) of a fleet rollout, `trace`: (n, ticks, 3) at stride 1, `how`, and `status_at`:
    (n, ticks) = the status of every robot after every call tick."""
    n = robots["pos"].shape[0]
    start = np.zeros(n, np.int64) if start_tick is None else np.minimum(np.asarray(start_tick, np.int64), ticks)
    out = dict(status=np.zeros(n, np.int32), ticks=np.zeros(n, np.uint32), pos=np.array(robots["pos"], F32), dir=np.array(robots["dir"], F32),
               face=np.array(robots["face_in"], np.uint32), travel=np.zeros(n), cost_integral=np.zeros(n), min_goal_dist=np.full(n, np.inf, F32),
               trace=np.repeat(np.array(robots["pos"], F32)[:, None, :], ticks, axis=1), how=np.zeros(5, np.int64))
    status_at = np.zeros((n, ticks), np.int32)
    for s in np.unique(start):
        own = int(ticks - s)
        if own == 0:
            continue                                                  # comes back as it went in
        g = np.nonzero(start == s)[0]
        sub = {k: (None if v is None else np.asarray(v)[g]) for k, v in robots.items()}
        r = RM.run(model, cfg, fields, sub, None if goals is None else (goals[0][g], goals[1][g]), dt, own, dist_tol, ang_tol, trace_stride=1)
        for k in RM.KEYS:
            out[k][g] = r[k]
        out["trace"][g, s:] = r["trace"]
        out["how"] += r["how"]
        k = np.arange(1, own + 1)[None, :]                            # a robot that stopped did so at its last tick
        status_at[g, s:] = np.where((r["status"][:, None] != RM.RUNNING) & (k >= r["ticks"][:, None].astype(np.int64)), r["status"][:, None], RM.RUNNING)
    out["status_at"] = status_at
    return out


def thin(trace, stride):
    """the trace at another stride: the rows after every stride-th tick"""
    return trace[:, stride - 1::stride][:, : trace.shape[1] // stride]


def present(status, waiting, flags, pos):
    finite = np.isfinite(pos).all(axis=1)
    run = (status == RM.RUNNING) & (~waiting | bool(flags & WAITING_PRESENT))
    stranded = (status == RM.OUT_OF_MAP) | (status == RM.NO_FIELD)
    return finite & (run | stranded | ((status == RM.REACHED) & bool(flags & REACHED_PRESENT)))


def d2_matrix(pos):
    p = np.asarray(pos, F32)
    with np.errstate(all="ignore"):
        dx, dy, dz = (p[:, None, k] - p[None, :, k] for k in range(3))
        return (dx * dx + dy * dy) + dz * dz


def start_rows(n):
    return dict(near_checks=np.zeros(n, np.uint32), max_partners=np.zeros(n, np.uint32), first_near_tick=np.full(n, NONE, np.uint32),
                first_near_robot=np.full(n, NONE, np.uint32), min_sep2=np.full(n, np.inf, F32), min_sep_tick=np.full(n, NONE, np.uint32),
                min_sep_robot=np.full(n, NONE, np.uint32))


def check(rows, pos, is_present, radius, tick):
    """one check at call tick `tick`, folded into `rows`; returns the near matrix"""
    n = pos.shape[0]
    r2 = F32(F32(radius) * F32(radius))
    d2 = d2_matrix(pos)
    with np.errstate(all="ignore"):
        near = is_present[:, None] & is_present[None, :] & ~np.eye(n, dtype=bool) & (d2 <= r2)
    partners = near.sum(axis=1)
    d2n = np.where(near, d2, F32(np.inf))
    who = np.argmin(d2n, axis=1)                                      # the first minimum: ties to the smallest index
    best = d2n[np.arange(n), who]
    for i in np.nonzero(partners)[0]:
        rows["near_checks"][i] += 1
        rows["max_partners"][i] = max(rows["max_partners"][i], partners[i])
        if rows["first_near_tick"][i] == NONE:
            rows["first_near_tick"][i], rows["first_near_robot"][i] = tick, who[i]
        if best[i] < rows["min_sep2"][i]:
            rows["min_sep2"][i], rows["min_sep_tick"][i], rows["min_sep_robot"][i] = best[i], tick, who[i]
    return near


def separation(trace, status_at, start_tick, radius, check_stride, flags):
    """The separation outputs of a call from its stride-1 trace (n, ticks, 3) and statuses (n, ticks): SEP_KEYS, `pairs`
    (near pairs per check), `partner_of` (n, bool: the robot was somebody's partner at some check) and the statistics."""
    n, ticks = trace.shape[0], trace.shape[1]
    start = np.zeros(n, np.int64) if start_tick is None else np.asarray(start_tick, np.int64)
    rows = start_rows(n)
    pairs, was_partner = [], np.zeros(n, bool)
    for t in range(check_stride, ticks + 1, check_stride):
        near = check(rows, trace[:, t - 1], present(status_at[:, t - 1], t <= start, flags, trace[:, t - 1]), radius, t)
        pairs.append(int(near.sum()) // 2)
        was_partner |= near.any(axis=0)
    out = dict(rows, pairs=np.array(pairs, np.int64), partner_of=was_partner)
    out["stats"] = stats(out, check_stride)
    return out


def stats(out, check_stride):
    """what mnav_fleet_rollout_stats tells of the checks, from the model's outputs (no check skipped)"""
    pairs, m = out["pairs"], out["min_sep2"]
    st = dict(checks_run=len(pairs), checks_skipped=0, first_skipped_tick=NONE, robots_near=int((out["near_checks"] > 0).sum()), near_pairs=int(pairs.sum()),
              max_pairs=int(pairs.max()) if len(pairs) else 0, max_pairs_tick=(int(np.argmax(pairs)) + 1) * check_stride if len(pairs) else NONE)
    i = int(np.argmin(m)) if len(m) else 0
    near = len(m) and np.isfinite(m[i])
    st["min_sep2"] = m[i] if near else F32(np.inf)
    st["min_pair"] = (i, int(out["min_sep_robot"][i])) if near else (NONE, NONE)
    return st


def assert_same_rows(got, want, what=""):
    for k in SEP_KEYS:
        g, w = np.asarray(got[k] if isinstance(got, dict) else getattr(got, k)), np.asarray(want[k])
        assert g.dtype == w.dtype and FM.same_bits(g, w), (what, k, np.nonzero(g != w)[0][:8], g[g != w][:4], w[g != w][:4])
