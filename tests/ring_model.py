"""The wait-for analysis of a yielding fleet rollout (mnav_fleet_rollout_rings) in Python / numpy, written from its
specification (include/mnav.h), NOT from mnav_fleet_ring.h.  What tests/test_ring_model.py (CPU, against the header compiled for
the host) and tests/test_gpu_fleet_rings.py (device) compare with.

analyse() walks the chain of every held robot with a visited set -- no doubling; run() is yield_model.run's tick-synchronous
loop with the analysis and the release behind yield_model.check."""
import numpy as np

from tests import follow_model as FM
from tests import rollout_model as RM
from tests import separation_model as SM
from tests import yield_model as YM

F32 = np.float32
NONE = SM.NONE
FREE, QUEUED, PARKED, RING_TAIL, RING_MEMBER = 0, 1, 2, 3, 4
RELEASE = 1
RING_KEYS = ("wait_class", "wait_anchor", "ring_checks", "first_ring_tick", "parked_checks", "released_checks")
COUNT_KEYS = ("queued", "parked", "tails", "members", "rings", "released")


def start_rrows(n):
    return dict(wait_class=np.zeros(n, np.uint8), wait_anchor=np.full(n, NONE, np.uint32), ring_checks=np.zeros(n, np.uint32),
                first_ring_tick=np.full(n, NONE, np.uint32), parked_checks=np.zeros(n, np.uint32), released_checks=np.zeros(n, np.uint32))


def analyse(hold0, blocker, mover, priority=None):
    """one check: (wait_class, anchor, leaders) of the graph w(i) = blocker[i] if hold0[i] else i.  leaders: the leader of every
    ring, sorted."""
    n = len(hold0)
    prio = [0] * n if priority is None else [int(p) for p in priority]
    cls, anchor, leaders = np.zeros(n, np.uint8), np.full(n, NONE, np.uint32), set()
    for i in range(n):
        if not hold0[i]:
            continue
        seen, order, at = {}, [], i
        while hold0[at] and at not in seen:
            seen[at] = len(order)
            order.append(at)
            at = int(blocker[at])
            assert at != order[-1] and 0 <= at < n
        if not hold0[at]:                                             # the root
            cls[i], anchor[i] = (QUEUED if mover[at] else PARKED), at
            continue
        ring = order[seen[at]:]                                       # the chain came back to `at`: the cycle from there on
        assert len(ring) >= 3
        leader = min(ring, key=lambda j: (prio[j], j))
        leaders.add(leader)
        cls[i], anchor[i] = (RING_MEMBER if i in ring else RING_TAIL), leader
    return cls, anchor, sorted(leaders)


def blockers(yields, d2):
    """b[i] of every robot that yields to somebody (the first minimum: ties to the smallest index), NONE elsewhere"""
    d2y = np.where(yields, d2, F32(np.inf))
    who = np.argmin(d2y, axis=1).astype(np.uint32)
    who[~yields.any(axis=1)] = NONE
    return who


def check(rows, yrows, rrows, pos, direction, status, waiting, flags, radius, ahead_cos, priority, tick, ring_flags):
    """one check at call tick `tick`: yield_model.check, then the analysis and the release.  Returns (hold, hold0, blocker,
    counts); rrows' wait_class / wait_anchor are this check's."""
    hold0, near, yields = YM.check(rows, yrows, pos, direction, status, waiting, flags, radius, ahead_cos, priority, tick)
    b = blockers(yields, SM.d2_matrix(pos))
    mover = (np.asarray(status) == RM.RUNNING) & ~np.asarray(waiting)
    cls, anchor, leaders = analyse(hold0, b, mover, priority)
    hold = hold0.copy()
    member = cls == RING_MEMBER
    rrows["wait_class"][:], rrows["wait_anchor"][:] = cls, anchor
    rrows["ring_checks"][member] += 1
    first = member & (rrows["first_ring_tick"] == NONE)
    rrows["first_ring_tick"][first] = tick
    rrows["parked_checks"][cls == PARKED] += 1
    released = 0
    if ring_flags & RELEASE:
        for i in leaders:
            hold[i] = 0
            rrows["released_checks"][i] += 1
        released = len(leaders)
    counts = dict(queued=int((cls == QUEUED).sum()), parked=int((cls == PARKED).sum()), tails=int((cls == RING_TAIL).sum()), members=int(member.sum()),
                  rings=len(leaders), released=released)
    return hold, hold0, b, counts


def run(model, cfg, fields, robots, goals, dt, ticks, dist_tol, ang_tol, start_tick, radius, check_stride, flags, ahead_cos, priority=None, hold_in=None,
        ring_flags=0, skip_checks=()):
    """The whole call: what yield_model.run returns (`held_at`: the flags every check left, after the release; `stats`: of
    those flags), RING_KEYS, `class_at` and `anchor_at` (checks, n), `counts` (one dict per check, zeros for a skipped one) and `ring_stats`
    (mnav_fleet_ring_stats)."""
    n = robots["pos"].shape[0]
    start = np.zeros(n, np.int64) if start_tick is None else np.asarray(start_tick, np.int64)
    states = [RM.start(robots["pos"][i], robots["dir"][i], robots["up"][i], robots["face_in"][i]) for i in range(n)]
    has = {}
    for i in range(n):
        key = (int(robots["slot"][i]), FM.NONE if robots.get("seed_face") is None else int(robots["seed_face"][i]))
        if key not in has:
            has[key] = FM.has_vector(model, fields[key[0]], key[1])
    hold = np.zeros(n, np.uint8) if hold_in is None else (np.asarray(hold_in) != 0).astype(np.uint8)
    rows, yrows, rrows = SM.start_rows(n), YM.start_yrows(n), start_rrows(n)
    trace, had_tick = np.zeros((n, ticks, 3), F32), np.zeros((n, ticks), bool)
    how = np.zeros(5, np.int64)
    held_at, class_at, anchor_at, counts, skipped = [], [], [], [], []
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
            rrows["wait_class"][:], rrows["wait_anchor"][:] = FREE, NONE
            counts.append(dict.fromkeys(COUNT_KEYS, 0))
            skipped.append(t)
        else:
            pos = np.array([S["pos"] for S in states], F32).reshape(n, 3)
            direction = np.array([S["dir"] for S in states], F32).reshape(n, 3)
            status = np.array([S["status"] for S in states], np.int32)
            hold, _, _, c = check(rows, yrows, rrows, pos, direction, status, t <= start, flags, radius, ahead_cos, priority, t, ring_flags)
            counts.append(c)
        held_at.append(hold.copy())
        class_at.append(rrows["wait_class"].copy())
        anchor_at.append(rrows["wait_anchor"].copy())
    out = dict(status=np.array([S["status"] for S in states], np.int32), ticks=np.array([S["ticks"] for S in states], np.uint32),
               pos=np.array([S["pos"] for S in states], F32).reshape(n, 3), dir=np.array([S["dir"] for S in states], F32).reshape(n, 3),
               face=np.array([S["face"] for S in states], np.uint32), travel=np.array([S["travel"] for S in states], np.float64),
               cost_integral=np.array([S["cost_integral"] for S in states], np.float64), min_goal_dist=np.array([S["min_goal_dist"] for S in states], F32),
               trace=trace, how=how, had_tick=had_tick, hold=hold, held_at=np.array(held_at, np.uint8).reshape(len(held_at), n),
               class_at=np.array(class_at, np.uint8).reshape(len(class_at), n),
               anchor_at=np.array(anchor_at, np.uint32).reshape(len(anchor_at), n), counts=counts, **rows, **yrows, **rrows)
    out["stats"] = YM.stats(out, check_stride, skipped)
    out["ring_stats"] = stats(out, check_stride, skipped)
    return out


def stats(out, check_stride, skipped=()):
    """what mnav_fleet_ring_stats tells, from the model's outputs"""
    counts = out["counts"]
    ran = [c for c in range(len(counts)) if (c + 1) * check_stride not in skipped]
    best = max(ran, key=lambda c: (counts[c]["rings"], -c)) if ran else None
    last = counts[-1] if counts else dict.fromkeys(COUNT_KEYS, 0)
    return dict(robots_ring=int((out["ring_checks"] > 0).sum()), rings=sum(counts[c]["rings"] for c in ran), max_rings=counts[best]["rings"] if ran else 0,
                max_rings_tick=(best + 1) * check_stride if ran else NONE, releases=sum(counts[c]["released"] for c in ran), members_last=last["members"],
                tails_last=last["tails"], parked_last=last["parked"], queued_last=last["queued"], rings_last=last["rings"], checks_run=len(ran),
                checks_skipped=len(counts) - len(ran), first_skipped_tick=min(skipped) if len(skipped) else NONE)


def ring_sizes(out, check):
    """the members of every ring at check `check`, by leader"""
    member = out["class_at"][check] == RING_MEMBER
    leaders, sizes = np.unique(out["anchor_at"][check][member], return_counts=True)
    return dict(zip(leaders.tolist(), sizes.tolist()))


def assert_same_rings(got, want, what=""):
    for k in RING_KEYS:
        g, w = np.asarray(got[k] if isinstance(got, dict) else getattr(got, k)), np.asarray(want[k])
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, k, np.nonzero(g != w)[0][:8], g[g != w][:4], w[g != w][:4])
