"""The sampled rollout in Python / numpy, written from its specification (include/mnav.h, mnav_follow_sample), NOT from
mnav_sample.h: what tests/test_sample_model.py (CPU, against the header compiled for the host) and tests/test_gpu_sample.py
(device) compare with.  Built on tests/rollout_model.py and tests/follow_model.py: one tick of a RUNNING row is
follow_model.tick, then the rollout's steps with the three differences of the specification -- the potential and the lethal
flag after step 3, the candidate's command in step 6, the score at the end.  Tick-synchronous semantics (rows are
independent, so row after row gives the same); numpy float32 / float64 scalars in the stated order; the host libm's
trigonometry as in rollout_model."""
import numpy as np

from tests import follow_model as FM
from tests import rollout_model as RM

F32, F64 = np.float32, np.float64
NONE = FM.NONE
PICKS = ("best_k", "best_score", "best_cmd", "n_feasible")
ROWS = ("status", "ticks", "score", "potential", "lethal", "cost_integral", "travel", "pos")
SAMPLE_DEFAULTS = dict(w_potential=1.0, w_cost=0.0, w_time=0.0, lethal_cost=1.0)


def command(gain, bias, x, cap):
    """difference b: u = gain * x; a bias that is not zero is added; the follower's saturation"""
    with np.errstate(all="ignore"):
        u = F64(gain) * F64(x)
        if bias != 0:
            u = F64(u + F64(bias))
        return u if u < F64(cap) else F64(cap)


def potential(model, d, face, b):
    """difference a: d[v0]*b0 + d[v1]*b1 + d[v2]*b2 in float32, left to right"""
    vs = model.faces[face]
    with np.errstate(all="ignore"):
        return F32(F32(F32(F32(d[vs[0]]) * F32(b[0])) + F32(F32(d[vs[1]]) * F32(b[1]))) + F32(F32(d[vs[2]]) * F32(b[2])))


def start(pos, d, up, face):
    S = RM.start(pos, d, up, face)
    S.update(pot=F32(np.inf), lethal=0, cmd0=None)
    return S


def after_tick(model, cfg, R, d, S, cand, goal, dt, dist_tol, ang_tol, lethal_cost):
    """steps 2 to 6 (and the count of step 1) of a RUNNING row whose tick gave R"""
    S["ticks"] += 1
    if R["code"] == FM.OUT_OF_MAP:
        S["status"], S["face"] = RM.OUT_OF_MAP, NONE
        return
    S["pos"], S["face"] = FM.vec(R["pos"]), int(R["face"])
    S["pot"] = potential(model, d, S["face"], R["bary"])
    if R["code"] == FM.OK and not (F32(R["cost"]) < F32(lethal_cost)):
        S["lethal"] = 1
    with np.errstate(all="ignore"):
        if goal is not None and RM.goal_test(S, goal[0], goal[1], dist_tol, ang_tol):
            S["status"] = RM.REACHED
            return
        if R["code"] == FM.NO_FIELD:
            S["status"] = RM.NO_FIELD
            return
        lin = command(cand[0], cand[1], R["cmd"][0], cfg["max_lin_velocity"])
        ang = command(cand[2], cand[3], R["cmd"][1], cfg["max_ang_velocity"])
        if S["cmd0"] is None:
            S["cmd0"] = (lin, ang)
        RM.advance(S, lin, ang, R["cost"], dt)


def score(S, sample, dt):
    """difference c: J in double, left to right"""
    with np.errstate(all="ignore"):
        return F64(F64(F64(sample["w_potential"]) * F64(S["pot"]) + F64(sample["w_cost"]) * F64(S["cost_integral"])) +
                   F64(sample["w_time"]) * F64(F64(S["ticks"]) * F64(dt)))


def feasible(status, lethal, J):
    return bool(status in (RM.RUNNING, RM.REACHED) and not lethal and np.isfinite(J))


def pick(status, lethal, J, cmd0):
    """the feasible row with the smallest (J, k) among a robot's K rows: J by <, ties (-0 against +0 is one) to the smaller k"""
    best, count = None, 0
    for k in range(len(J)):
        if not feasible(int(status[k]), int(lethal[k]), J[k]):
            continue
        count += 1
        if best is None or J[k] < J[best]:
            best = k
    if best is None:
        return NONE, F64(np.inf), (F64(0), F64(0)), 0
    return best, F64(J[best]), (F64(cmd0[best][0]), F64(cmd0[best][1])), count


def run(model, cfg, fields, pots, robots, goals, table, dt, ticks, dist_tol=0.0, ang_tol=0.0, sample=None):
    """`ticks` ticks of the n * K rows of `robots` (dict of arrays as for rollout_model.run) under the (K, 4) table;
    fields[s] / pots[s]: vector map and potential of plan s.  Returns a dict: ROWS as (n, K) arrays (pos (n, K, 3)), cmd0
    (n, K, 2), PICKS per robot, and `how` = row-ticks by how (5 counters).  A tick of a state that was seen before -- every
    row's first -- is taken from a cache: follow_model.tick is a function of (field, position, heading, up, face); and a
    robot's row under a candidate that stands in the table twice is computed once."""
    sample = dict(SAMPLE_DEFAULTS, **(sample or {}))
    table = np.asarray(table, F64).reshape(-1, 4)
    n, K = robots["pos"].shape[0], table.shape[0]
    out = dict(status=np.zeros((n, K), np.int32), ticks=np.zeros((n, K), np.uint32), score=np.zeros((n, K), F64), potential=np.zeros((n, K), F32),
               lethal=np.zeros((n, K), np.uint8), cost_integral=np.zeros((n, K), F64), travel=np.zeros((n, K), F64), pos=np.zeros((n, K, 3), F32),
               cmd0=np.zeros((n, K, 2), F64), best_k=np.zeros(n, np.uint32), best_score=np.zeros(n, F64), best_cmd=np.zeros((n, 2), F64),
               n_feasible=np.zeros(n, np.uint32), how=np.zeros(5, np.int64))
    has_cache, tick_cache = {}, {}
    for i in range(n):
        s = int(robots["slot"][i])
        sf = NONE if robots.get("seed_face") is None else int(robots["seed_face"][i])
        if (s, sf) not in has_cache:
            has_cache[(s, sf)] = FM.has_vector(model, fields[s], sf)
        goal = None if goals is None else (goals[0][i], goals[1][i])
        rows = {}                                                         # a robot's rows under one candidate are one row
        for k in range(K):
            if table[k].tobytes() not in rows:
                S, how = start(robots["pos"][i], robots["dir"][i], robots["up"][i], robots["face_in"][i]), np.zeros(5, np.int64)
                for _ in range(ticks):
                    if S["status"] != RM.RUNNING:
                        break
                    key = (s, sf, np.asarray(S["pos"], F32).tobytes(), np.asarray(S["dir"], F32).tobytes(), np.asarray(S["up"], F32).tobytes(), S["face"])
                    if key not in tick_cache:
                        tick_cache[key] = FM.tick(model, cfg, fields[s], has_cache[(s, sf)], S["pos"], S["dir"], S["up"], S["face"])
                    R = tick_cache[key]
                    how[R["how"]] += 1
                    after_tick(model, cfg, R, pots[s], S, table[k], goal, dt, dist_tol, ang_tol, sample["lethal_cost"])
                rows[table[k].tobytes()] = (S, how)
            S, how = rows[table[k].tobytes()]
            out["how"] += how
            out["status"][i, k], out["ticks"][i, k], out["score"][i, k] = S["status"], S["ticks"], score(S, sample, dt)
            out["potential"][i, k], out["lethal"][i, k] = S["pot"], S["lethal"]
            out["cost_integral"][i, k], out["travel"][i, k], out["pos"][i, k] = S["cost_integral"], S["travel"], S["pos"]
            out["cmd0"][i, k] = (0.0, 0.0) if S["cmd0"] is None else S["cmd0"]
        out["best_k"][i], out["best_score"][i], out["best_cmd"][i], out["n_feasible"][i] = pick(out["status"][i], out["lethal"][i], out["score"][i], out["cmd0"][i])
    return out


def stats(want):
    """the counts mnav_sample_stats reports, folded from a run's output"""
    st = np.bincount(want["status"].reshape(-1), minlength=4)
    feas = [feasible(int(s), int(le), J) for s, le, J in zip(want["status"].reshape(-1), want["lethal"].reshape(-1), want["score"].reshape(-1))]
    return dict(running=int(st[0]), reached=int(st[1]), out_of_map=int(st[2]), no_field=int(st[3]), lethal_rows=int(want["lethal"].sum()),
                feasible_rows=int(sum(feas)), robots_without_pick=int((want["best_k"] == NONE).sum()), row_ticks=int(want["ticks"].sum()),
                stayed=int(want["how"][2]), neighbour=int(want["how"][3]), **{"global": int(want["how"][1] + want["how"][4])})


def assert_same(got, want, what="", keys=PICKS + ROWS):
    """every comparison exact: integers equal, floats and doubles by their bits, any NaN equals any NaN"""
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if not FM.same_bits(g.astype(w.dtype) if g.dtype.kind != "f" else g, w):
            bad = np.argwhere((g != w) & ~((g != g) & (w != w)))
            raise AssertionError((what, k, bad[:8].tolist(), [g[tuple(b)] for b in bad[:3]], [w[tuple(b)] for b in bad[:3]]))


def assert_every_branch(want, what=""):
    """conditions on the MODEL's output: a row in every final status, a lethal row, a robot without a feasible row, a robot
    whose pick is not candidate 0, and a robot with two rows tied in J"""
    st = set(want["status"].reshape(-1).tolist())
    assert st == {RM.RUNNING, RM.REACHED, RM.OUT_OF_MAP, RM.NO_FIELD}, (what, np.bincount(want["status"].reshape(-1), minlength=4))
    assert want["lethal"].any(), what
    assert (want["best_k"] == NONE).any() and (want["n_feasible"] == 0).any(), what
    assert ((want["best_k"] != NONE) & (want["best_k"] != 0)).any(), what
    tied = False
    for i in range(want["score"].shape[0]):
        J = want["score"][i][np.isfinite(want["score"][i])]
        tied = tied or np.unique(J).size < J.size
    assert tied, what
