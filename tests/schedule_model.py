"""The rule of mnav_fleet_schedule (include/mnav.h) in numpy, on top of tests/fleet_model.py and
tests/timed_traffic_model.py: the robots, the contributor rule and the float32 window arithmetic are those of the timed call;
a schedule gives every contributor the smallest delay (whole windows) whose visits all lie inside the horizon and fit under
`capacity`, round by round -- probe, claim, decide, commit -- on the committed cells.  The robots' visits are kept as one flat
list (CSR), every round works on the open robots' slices of it at once.  tests/test_fleet_schedule_model.py pins the header's
host mirror against this file, tests/test_gpu_schedule.py the device."""
from __future__ import annotations

import numpy as np

from tests import fleet_model as FM
from tests import timed_traffic_model as XM
from tests import traffic_model as TM

NONE = FM.NONE
F = np.float32
ST_NONE, COMMITTED, NO_SLOT, OPEN = 0, 1, 2, 3
SEED_FREE = 1
BYTES_PER_CELL = 20                                       # cell, holder, tentative count (4 each), tentative holder (8)


def depart_at(depart, d, tau):
    """depart_d: one float32 multiply, then one float32 add (d = 0 gives depart bit for bit)"""
    with np.errstate(over="ignore"):
        return (np.asarray(depart, F) + (np.asarray(d).astype(F) * F(tau)).astype(F)).astype(F)


def refused(state: XM.Cells, n, weights, depart, pace, B, tau, capacity, max_delay, flags, accumulate) -> bool:
    if XM.refused(state, n, weights, depart, pace, B, tau, accumulate):
        return True
    return capacity < 1 or max_delay >= B or (flags & ~SEED_FREE) != 0


class Visits:
    """the visits of the contributors as one flat list: robot i owns [off[i], off[i + 1]), from its vertex down to the seed"""

    def __init__(self, fields, slots, vtx, run, on):
        n = len(slots)
        off = run["offsets"].astype(np.int64)
        self.cnt = np.zeros(n, np.int64)
        us, ds = [], []
        for i in np.flatnonzero(on):
            path = np.concatenate(([int(vtx[i])], run["ids"][off[i]:off[i + 1]][::-1])).astype(np.int64)
            self.cnt[i] = path.size
            us.append(path)
            ds.append(np.asarray(fields[int(slots[i])].dist, F)[path])
        self.off = np.concatenate(([0], np.cumsum(self.cnt))).astype(np.int64)
        self.u = np.concatenate(us) if us else np.zeros(0, np.int64)
        self.d = np.concatenate(ds) if ds else np.zeros(0, F)
        self.last = np.zeros(self.u.size, bool)
        self.last[self.off[1:][self.cnt > 0] - 1] = True                   # the visit on the seed

    def of(self, robots):
        """(flat visit index, position in `robots`) of every visit of the given robots"""
        m = self.cnt[robots]
        loc = np.repeat(np.arange(robots.size), m)
        within = np.arange(int(m.sum())) - np.repeat(np.cumsum(m) - m, m)
        return self.off[robots][loc] + within, loc


def schedule(state: XM.Cells, fields, slots, vtx, weights=None, depart=None, pace=None, key=None, B=64, tau=1.0, capacity=1, max_delay=0, max_rounds=0,
             flags=0, accumulate=False, run=None):
    """one mnav_fleet_schedule call on `state`.  Returns None (state untouched) where the call refuses, else the call's
    outputs, the per-round (claimed, won) list and the statistics.  run: FM.run(fields, V, slots, vtx) when the caller has it."""
    n, V = len(slots), state.V
    if refused(state, n, weights, depart, pace, B, tau, capacity, max_delay, flags, accumulate):
        return None
    with np.errstate(over="ignore", under="ignore"):
        tf = np.float64(tau).astype(F)
    w = (np.ones(n, np.uint32) if weights is None else np.asarray(weights, np.uint32)).astype(np.int64)
    dep = np.zeros(n, F) if depart is None else np.asarray(depart, F)
    pc = np.ones(n, F) if pace is None else np.asarray(pace, F)
    ky = np.arange(n, dtype=np.uint32) if key is None else np.asarray(key, np.uint32)
    r = FM.run(fields, V, slots, vtx) if run is None else run
    on = TM.contributes(r["codes"], r["potential"]) & (w > 0)
    P = r["potential"].astype(F)
    vs = Visits(fields, slots, vtx, r, on)
    constrained = ~vs.last if flags & SEED_FREE else np.ones(vs.u.size, bool)
    if accumulate and state.cell is not None:
        cell, holder, T = state.cell.astype(np.int64).ravel(), state.holder.copy().ravel(), state.T
    else:
        cell, holder, T = np.zeros(V * B, np.int64), np.full(V * B, NONE, np.uint32), 0
    status = np.where(on, OPEN, ST_NONE).astype(np.uint32)
    cur, rnd = np.zeros(n, np.int64), np.full(n, NONE, np.uint32)

    def cells_of(robots):
        """(visit, position in robots, robot, in the horizon, cell index) of the robots' visits at their current delays"""
        vis, loc = vs.of(robots)
        who = robots[loc]
        t = XM.visit_time(P[who], vs.d[vis], depart_at(dep[robots], cur[robots], tf)[loc], pc[who])
        inside, k = XM.window_of(t, tf, B)
        return vis, loc, who, inside, vs.u[vis] * B + k.astype(np.int64)

    rounds = []
    while (status == OPEN).any() and (max_rounds == 0 or len(rounds) < max_rounds):
        # probe: the smallest delay from cur on that fits the cells as they stand; all open robots step together
        pend = np.flatnonzero(status == OPEN)
        while pend.size:
            vis, loc, who, inside, c = cells_of(pend)
            full = constrained[vis] & inside & (cell[c] + w[who] > capacity)
            beyond = np.bincount(loc[~inside], minlength=pend.size) > 0
            heavy = w[pend] > capacity
            fit = ~beyond & ~heavy & ~(np.bincount(loc[full], minlength=pend.size) > 0)
            dead = ~fit & (beyond | heavy | (cur[pend] >= max_delay))         # beyond the horizon: every larger delay is too
            status[pend[dead]] = NO_SLOT
            pend = pend[~fit & ~dead]
            cur[pend] += 1
        # claim: tentative counts and the tentative holder (key, index) of every constrained visit
        claim = np.flatnonzero(status == OPEN)
        vis, loc, who, inside, c = cells_of(claim)
        assert inside.all()
        con = constrained[vis]
        ticket = (ky[who].astype(np.uint64) << np.uint64(32)) | who.astype(np.uint64)
        tent, th = np.zeros(V * B, np.int64), np.full(V * B, np.iinfo(np.uint64).max, np.uint64)
        np.add.at(tent, c[con], w[who[con]])
        np.minimum.at(th, c[con], ticket[con])
        # decide: every constrained visit is uncontended, or the robot holds it
        lose = con & (cell[c] + tent[c] > capacity) & (th[c] != ticket)
        lost = np.bincount(loc[lose], minlength=claim.size) > 0
        # commit: ALL visits of the winners
        m = ~lost[loc]
        np.add.at(cell, c[m], w[who[m]])
        np.minimum.at(holder, c[m], ky[who[m]])
        win = claim[~lost]
        status[win], rnd[win] = COMMITTED, len(rounds) + 1
        T += int(w[win].sum())
        rounds.append((int(claim.size), int(win.size)))
        assert win.size > 0 or claim.size == 0                                # progress
    assert cell.max(initial=0) <= XM.MAX_TOTAL
    state.cell, state.holder = cell.astype(np.uint32).reshape(V, B), holder.reshape(V, B)
    state.B, state.tau, state.T = B, tf, T
    done = status == COMMITTED
    delay = np.where(done, cur, NONE).astype(np.uint32)
    depart_out = np.where(done, depart_at(dep, cur, tf), F(np.inf)).astype(F)
    return dict(codes=r["codes"], potential=r["potential"], status=status, delay=delay, depart_out=depart_out, round=rnd, per_round=rounds,
                contributing=int(on.sum()), committed=int(done.sum()), no_slot=int((status == NO_SLOT).sum()), open=int((status == OPEN).sum()),
                rounds=len(rounds), delayed=int((done & (cur > 0)).sum()), max_delay_used=int(cur[done].max(initial=0)),
                claims=sum(a for a, _ in rounds), committed_visits=int(vs.cnt[done].sum()), weight=int(w[done].sum()),
                # what mnav_timed_traffic_stats says afterwards
                timed=dict(contributing=int(done.sum()), adds=int(vs.cnt[done].sum()), beyond_horizon=0, total_weight=T,
                           occupied_cells=int((state.cell > 0).sum()), over_cells=int((state.cell > np.uint32(min(capacity, NONE))).sum()),
                           largest_cell=int(state.cell.max(initial=0)), yielding=0, windows=B))
