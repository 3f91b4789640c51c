"""The device rollout in Python / numpy, written from its specification (include/mnav.h, mnav_follow_rollout), NOT from
mnav_rollout.h: what tests/test_rollout_model.py (CPU, against the header compiled for the host) and
tests/test_gpu_rollout.py (device) compare with.  One tick of a RUNNING robot is follow_model.tick (the reference's
computeVelocityCommands), then isGoalReached (mesh_controller.cpp:172-177), then the unicycle of
follow_model.unicycle_step pinned to float trigonometry; numpy float32 / float64 scalars in the stated order.  cosf, sinf
and acosf are the host libm's own through ctypes, not the product's restatements."""
import ctypes as C

import numpy as np

from tests import follow_model as FM

F32, F64 = np.float32, np.float64
RUNNING, REACHED, OUT_OF_MAP, NO_FIELD = 0, 1, 2, 3

for _name in ("cosf", "sinf"):
    getattr(FM._libm, _name).restype = C.c_float
    getattr(FM._libm, _name).argtypes = [C.c_float]


def start(pos, d, up, face):
    return dict(pos=FM.vec(pos), dir=FM.vec(d), up=FM.vec(up), face=int(face), status=RUNNING, ticks=0, travel=F64(0), cost_integral=F64(0),
                min_goal_dist=F32(np.inf))


def goal_test(S, goal_pos, goal_dir, dist_tol, ang_tol):
    """step 4: isGoalReached on the position and heading this tick set; updates min_goal_dist"""
    gd = FM.length(FM.sub(FM.vec(goal_pos), S["pos"]))
    ang = F32(FM._libm.acosf(float(FM.dot(FM.vec(goal_dir), S["dir"]))))
    S["min_goal_dist"] = gd if gd < S["min_goal_dist"] else S["min_goal_dist"]
    return bool(gd <= F32(dist_tol) and ang <= F32(ang_tol))


def advance(S, lin, ang, cost, dt):
    """step 6: the unicycle, position in double stored as float32, heading by Rodrigues' formula in float32"""
    dt = F64(dt)
    step = F64(lin) * dt
    S["travel"] = F64(S["travel"] + step)
    S["cost_integral"] = F64(S["cost_integral"] + F64(F32(cost)) * dt)
    d, up = S["dir"], S["up"]
    S["pos"] = [F32(F64(S["pos"][k]) + F64(d[k]) * step) for k in range(3)]
    th = F32(F64(ang) * dt)
    c, s = F32(FM._libm.cosf(float(th))), F32(FM._libm.sinf(float(th)))
    k = FM.cross(up, d)
    h = F32(FM.dot(up, d) * F32(F32(1) - c))
    dn = FM.add(FM.add(FM.scale(d, c), FM.scale(k, s)), FM.scale(up, h))
    S["dir"] = FM.div(dn, FM.length(dn))


def one_tick(model, cfg, vecmap, has, S, goal, dt, dist_tol, ang_tol):
    """one tick of a RUNNING robot; goal: (goal_pos, goal_dir) or None.  Returns the tick's `how`."""
    R = FM.tick(model, cfg, vecmap, has, S["pos"], S["dir"], S["up"], S["face"])
    S["ticks"] += 1
    if R["code"] == FM.OUT_OF_MAP:
        S["status"], S["face"] = OUT_OF_MAP, FM.NONE
        return R["how"]
    S["pos"], S["face"] = FM.vec(R["pos"]), int(R["face"])
    with np.errstate(all="ignore"):
        if goal is not None and goal_test(S, goal[0], goal[1], dist_tol, ang_tol):
            S["status"] = REACHED
            return R["how"]
        if R["code"] == FM.NO_FIELD:
            S["status"] = NO_FIELD
            return R["how"]
        advance(S, R["cmd"][0], R["cmd"][1], R["cost"], dt)
    return R["how"]


KEYS = ("status", "ticks", "pos", "dir", "face", "travel", "cost_integral", "min_goal_dist")


def run(model, cfg, fields, robots, goals, dt, ticks, dist_tol=0.0, ang_tol=0.0, trace_stride=0):
    """`ticks` ticks of every robot of `robots` (dict of arrays as for follow_model.tick_batch); goals: (goal_pos (n, 3),
    goal_dir (n, 3)) or None.  Returns a dict of arrays (KEYS, `trace` (n, ticks // trace_stride, 3) or None, `how` = ticks
    by how (5 counters))."""
    n = robots["pos"].shape[0]
    states = [start(robots["pos"][i], robots["dir"][i], robots["up"][i], robots["face_in"][i]) for i in range(n)]
    rows = ticks // trace_stride if trace_stride else 0
    trace = np.zeros((n, rows, 3), F32) if trace_stride else None
    how = np.zeros(5, np.int64)
    cache = {}
    for i, S in enumerate(states):
        s = int(robots["slot"][i])
        sf = FM.NONE if robots.get("seed_face") is None else int(robots["seed_face"][i])
        if (s, sf) not in cache:
            cache[(s, sf)] = FM.has_vector(model, fields[s], sf)
        goal = None if goals is None else (goals[0][i], goals[1][i])
        for t in range(1, ticks + 1):
            if S["status"] == RUNNING:
                how[one_tick(model, cfg, fields[s], cache[(s, sf)], S, goal, dt, dist_tol, ang_tol)] += 1
            if trace_stride and t % trace_stride == 0:
                trace[i, t // trace_stride - 1] = S["pos"]
    out = dict(status=np.array([S["status"] for S in states], np.int32), ticks=np.array([S["ticks"] for S in states], np.uint32),
               pos=np.array([S["pos"] for S in states], F32).reshape(n, 3), dir=np.array([S["dir"] for S in states], F32).reshape(n, 3),
               face=np.array([S["face"] for S in states], np.uint32), travel=np.array([S["travel"] for S in states], F64),
               cost_integral=np.array([S["cost_integral"] for S in states], F64),
               min_goal_dist=np.array([S["min_goal_dist"] for S in states], F32), trace=trace, how=how)
    return out


def assert_same(got, want, what="", keys=KEYS + ("trace",)):
    """every comparison exact: integers equal, floats and doubles by their bits, any NaN equals any NaN"""
    for k in keys:
        g, w = got[k] if isinstance(got, dict) else getattr(got, k), want[k]
        if w is None:
            assert g is None, (what, k)
            continue
        g, w = np.asarray(g), np.asarray(w)
        if not FM.same_bits(g.astype(w.dtype) if g.dtype.kind != "f" else g, w):
            bad = np.nonzero((g != w).reshape(g.shape[0], -1).any(axis=1))[0]
            raise AssertionError((what, k, bad[:8], g[bad[:3]], w[bad[:3]]))


def assert_every_outcome(want, what=""):
    """conditions on the MODEL's output: all four statuses (so a robot is still RUNNING at the end), a goal reached after the
    first tick, and ticks resolved with no face yet (how 1), by staying (2) and by a neighbour search (3)"""
    st = set(want["status"].tolist())
    assert st == {RUNNING, REACHED, OUT_OF_MAP, NO_FIELD}, (what, np.bincount(want["status"], minlength=4))
    assert ((want["status"] == REACHED) & (want["ticks"] > 1)).any(), what
    assert want["how"][1] > 0 and want["how"][2] > 0 and want["how"][3] > 0, (what, want["how"])
