"""The yielding fleet rollout (mnav_fleet_rollout_yield) in Python / numpy, written from its specification (include/mnav.h),
NOT from mnav_fleet_yield.h.  What tests/test_yield_model.py (CPU, against the header compiled for the host) and
tests/test_gpu_fleet_yield.py (device) compare with.

Robots are no longer independent, so the loop is tick-synchronous: per call tick rollout_model.one_tick for every robot that
has a tick (RUNNING, departed, not held), then the trace row, then -- after every check_stride-th tick -- an O(n^2) check:
separation_model.present and d2_matrix, the separation rows through separation_model.check, and the right-of-way predicate in
numpy float32, every operation rounded on its own in the stated order."""
import numpy as np

from tests import follow_model as FM
from tests import rollout_model as RM
from tests import separation_model as SM

F32 = np.float32
NONE = SM.NONE
YIELD_KEYS = ("hold", "hold_checks", "held_ticks", "first_hold_tick", "first_hold_robot")


def start_yrows(n):
    return dict(hold_checks=np.zeros(n, np.uint32), held_ticks=np.zeros(n, np.uint32), first_hold_tick=np.full(n, NONE, np.uint32),
                first_hold_robot=np.full(n, NONE, np.uint32))


def ahead(pos, direction, d2, ahead_cos):
    """A[i, j]: j is ahead of i"""
    p, d = np.asarray(pos, F32), np.asarray(direction, F32)
    c = F32(ahead_cos)
    c2 = F32(c * c)
    with np.errstate(all="ignore"):
        ex, ey, ez = (p[None, :, k] - p[:, None, k] for k in range(3))
        dot = (d[:, None, 0] * ex + d[:, None, 1] * ey) + d[:, None, 2] * ez
        return (dot > F32(0)) & (dot * dot >= c2 * d2)


def decide(pos, direction, status, waiting, is_present, near, d2, ahead_cos, priority=None):
    """one check's decision: yields[i, j] = the present mover i yields to its partner j"""
    n = pos.shape[0]
    mover = (np.asarray(status) == RM.RUNNING) & ~waiting
    A = ahead(pos, direction, d2, ahead_cos)
    prio = np.zeros(n, np.int64) if priority is None else np.asarray(priority, np.int64)
    idx = np.arange(n)
    before = (prio[None, :] < prio[:, None]) | ((prio[None, :] == prio[:, None]) & (idx[None, :] < idx[:, None]))     # before[i, j] = before(j, i)
    to_standing = ~mover[None, :] & A
    to_mover = mover[None, :] & A & (~A.T | before)
    return near & (is_present & mover)[:, None] & (to_standing | to_mover)


def check(rows, yrows, pos, direction, status, waiting, flags, radius, ahead_cos, priority, tick):
    """one check at call tick `tick` folded into the separation rows and the yield rows; returns (hold, near, yields)"""
    n = pos.shape[0]
    is_present = SM.present(np.asarray(status), waiting, flags, pos)
    near = SM.check(rows, pos, is_present, radius, tick)
    d2 = SM.d2_matrix(pos)
    yields = decide(pos, direction, status, waiting, is_present, near, d2, ahead_cos, priority)
    hold = yields.any(axis=1)
    d2y = np.where(yields, d2, F32(np.inf))
    who = np.argmin(d2y, axis=1)                                      # the first minimum: ties to the smallest index
    for i in np.nonzero(hold)[0]:
        yrows["hold_checks"][i] += 1
        if yrows["first_hold_tick"][i] == NONE:
            yrows["first_hold_tick"][i], yrows["first_hold_robot"][i] = tick, who[i]
    return hold.astype(np.uint8), near, yields


def run(model, cfg, fields, robots, goals, dt, ticks, dist_tol, ang_tol, start_tick, radius, check_stride, flags, ahead_cos, priority=None, hold_in=None,
        skip_checks=()):
    """The whole call.  Returns RM.KEYS, `trace` (n, ticks, 3) at stride 1, SM.SEP_KEYS, YIELD_KEYS, `held_at` (checks, n:
    the flags every check left), `had_tick` (n, ticks), `pairs`, `stats` (mnav_fleet_yield_stats) and `sep_stats`.
    skip_checks: ticks whose check the guard skips (nothing compared, every hold cleared)."""
    n = robots["pos"].shape[0]
    start = np.zeros(n, np.int64) if start_tick is None else np.asarray(start_tick, np.int64)
    states = [RM.start(robots["pos"][i], robots["dir"][i], robots["up"][i], robots["face_in"][i]) for i in range(n)]
    has = {}
    for i in range(n):
        key = (int(robots["slot"][i]), FM.NONE if robots.get("seed_face") is None else int(robots["seed_face"][i]))
        if key not in has:
            has[key] = FM.has_vector(model, fields[key[0]], key[1])
    hold = np.zeros(n, np.uint8) if hold_in is None else (np.asarray(hold_in) != 0).astype(np.uint8)
    rows, yrows = SM.start_rows(n), start_yrows(n)
    trace, had_tick = np.zeros((n, ticks, 3), F32), np.zeros((n, ticks), bool)
    how = np.zeros(5, np.int64)
    held_at, pairs, skipped = [], [], []
    for t in range(1, ticks + 1):
        for i, S in enumerate(states):
            if S["status"] == RM.RUNNING and t > start[i]:
                if hold[i]:
                    yrows["held_ticks"][i] += 1
                else:
                    key = (int(robots["slot"][i]), FM.NONE if robots.get("seed_face") is None else int(robots["seed_face"][i]))
                    goal = None if goals is None else (goals[0][i], goals[1][i])
                    how[RM.one_tick(model, cfg, fields[key[0]], has[key], S, goal, dt, dist_tol, ang_tol)] += 1
                    had_tick[i, t - 1] = True
            trace[i, t - 1] = S["pos"]
        if t % check_stride:
            continue
        if t in skip_checks:
            hold = np.zeros(n, np.uint8)
            skipped.append(t)
        else:
            pos = np.array([S["pos"] for S in states], F32).reshape(n, 3)
            direction = np.array([S["dir"] for S in states], F32).reshape(n, 3)
            status = np.array([S["status"] for S in states], np.int32)
            hold, near, _ = check(rows, yrows, pos, direction, status, t <= start, flags, radius, ahead_cos, priority, t)
            pairs.append(int(near.sum()) // 2)
        held_at.append(hold.copy())
    out = dict(status=np.array([S["status"] for S in states], np.int32), ticks=np.array([S["ticks"] for S in states], np.uint32),
               pos=np.array([S["pos"] for S in states], F32).reshape(n, 3), dir=np.array([S["dir"] for S in states], F32).reshape(n, 3),
               face=np.array([S["face"] for S in states], np.uint32), travel=np.array([S["travel"] for S in states], np.float64),
               cost_integral=np.array([S["cost_integral"] for S in states], np.float64), min_goal_dist=np.array([S["min_goal_dist"] for S in states], F32),
               trace=trace, how=how, had_tick=had_tick, hold=hold, held_at=np.array(held_at, np.uint8).reshape(len(held_at), n), pairs=np.array(pairs, np.int64),
               **rows, **yrows)
    out["stats"] = stats(out, check_stride, skipped)
    out["sep_stats"] = None if skipped else SM.stats(out, check_stride)   # (separation_model.stats knows no skipped check)
    return out


def stats(out, check_stride, skipped=()):
    """what mnav_fleet_yield_stats tells, from the model's outputs"""
    held = out["held_at"].sum(axis=1).astype(np.int64)
    ran = [c for c in range(len(held)) if (c + 1) * check_stride not in skipped]
    best = max(ran, key=lambda c: (held[c], -c)) if ran else None
    return dict(robots_held=int((out["hold_checks"] > 0).sum()), held_ticks=int(out["held_ticks"].astype(np.int64).sum()),
                max_held=int(held[best]) if ran else 0, max_held_tick=(best + 1) * check_stride if ran else NONE, held_last=int(out["hold"].sum()),
                checks_run=len(ran), checks_skipped=len(held) - len(ran), first_skipped_tick=min(skipped) if len(skipped) else NONE)


def assert_same_yield(got, want, what=""):
    for k in YIELD_KEYS:
        g, w = np.asarray(got[k] if isinstance(got, dict) else getattr(got, k)), np.asarray(want[k])
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, k, np.nonzero(g != w)[0][:8], g[g != w][:4], w[g != w][:4])
