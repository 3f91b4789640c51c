"""The rules of mnav_fleet_costs and mnav_fleet_assign (include/mnav.h) in numpy.

pair / matrix: the pair rule, i.e. rules 1 to 6 of tests/fleet_model.py without the walk of the chain.  nearest: the
feasible minima with their tie rule.  quantise, auction: the assignment exactly as the device runs it (the synchronous
auction with its eps schedule), with the phases and rounds it takes.  exact: an independent O(N^3) Hungarian solver on
the same padded problem, for (size, sum of q).  tests/test_dispatch_model.py pins these against each other and the
header's host mirror against them; tests/test_gpu_dispatch.py pins the device against them."""
from __future__ import annotations

import numpy as np

from tests import fleet_model as FM
from tests.fleet_model import BEYOND_FIELD, INF, INVALID_GOAL, NO_PATH_FOUND, NONE, SUCCESS

I64MAX = np.iinfo(np.int64).max


def wave_ran_out(f: FM.Field) -> bool:
    """no vertex holds a finite value at or above the cut: every vertex the wave reached was expanded"""
    cut = FM.cut_of(f.dist, f.target, f.offset)
    return (not cut < INF) or not (np.isfinite(f.dist) & (f.dist >= cut)).any()


def pair(f: FM.Field, V: int, v: int):
    """(code, potential) of a robot on vertex v for the column of field f: fleet_model.classify without the walk"""
    if v >= V:
        return INVALID_GOAL, INF                                        # rule 1
    if f.dist is None:
        return f.code, INF                                              # rule 2
    if v == f.seed:
        return SUCCESS, np.float32(0)                                   # rule 3
    d = np.float32(f.dist[v])
    cut = FM.cut_of(f.dist, f.target, f.offset)
    if d < cut or v == f.target:                                        # rule 4: no walk
        return (NO_PATH_FOUND if int(f.pred[v]) == v else SUCCESS), d
    if not d < INF and wave_ran_out(f):
        return NO_PATH_FOUND, INF                                       # rule 5
    return BEYOND_FIELD, INF                                            # rule 6


def matrix(fields, V: int, vtx):
    """codes (n x m uint8) and potentials (n x m float32) of robots on vtx over the columns `fields`: pair(), a column at a time"""
    vtx = np.asarray(vtx, np.int64)
    n, m = vtx.size, len(fields)
    codes, pot = np.full((n, m), INVALID_GOAL, np.uint8), np.full((n, m), INF, np.float32)
    inside = vtx < V
    vc = np.where(inside, vtx, 0)
    for j, f in enumerate(fields):
        if f.dist is None:
            codes[inside, j] = f.code
            continue
        d, p = f.dist[vc].astype(np.float32), f.pred[vc].astype(np.int64)
        cut = FM.cut_of(f.dist, f.target, f.offset)
        seed = inside & (vc == f.seed)
        four = inside & ~seed & ((d < cut) | (vc == f.target))
        rest = inside & ~seed & ~four
        code = np.full(n, BEYOND_FIELD, np.uint8)
        if wave_ran_out(f):
            code[~(d < INF)] = NO_PATH_FOUND
        codes[rest, j] = code[rest]
        codes[four, j] = np.where(p[four] == vc[four], NO_PATH_FOUND, SUCCESS)
        pot[four, j] = d[four]
        codes[seed, j], pot[seed, j] = SUCCESS, 0
    return codes, pot


def feasible_of(codes, pot):
    return (codes == SUCCESS) & np.isfinite(pot)


def counts(codes):
    """pairs served / beyond the field / without a path / invalid"""
    c = [int((codes == SUCCESS).sum()), int((codes == BEYOND_FIELD).sum()), int((codes == NO_PATH_FOUND).sum())]
    return c + [codes.size - sum(c)]


def nearest(codes, pot):
    """(nearest_slot per robot, nearest_robot per column): the smallest feasible potential, ties to the smallest index"""
    masked = np.where(feasible_of(codes, pot), pot, INF)
    ns = np.where(np.isfinite(masked).any(axis=1), masked.argmin(axis=1), NONE).astype(np.uint32)
    nr = np.where(np.isfinite(masked).any(axis=0), masked.argmin(axis=0), NONE).astype(np.uint32)
    return ns, nr


def quantise(pot, feasible, quantum: float):
    """q = floor(potential / quantum + 0.5) in double over the feasible pairs, -1 elsewhere"""
    x = np.floor(np.where(feasible, pot, 0).astype(np.float64) / np.float64(quantum) + 0.5)
    return np.where(feasible, x, -1).astype(np.int64)


def padded(q, feasible):
    """the N x N costs (unscaled): q, M = N q_max + 1 for an infeasible real pair, 0 with a dummy row or column"""
    n, m = q.shape
    N = max(n, m)
    qmax = int(q[feasible].max()) if feasible.any() else 0
    M = N * qmax + 1
    cost = np.zeros((N, N), np.int64)
    cost[:n, :m] = np.where(feasible, q, M)
    return cost, N, M


def result_of(mine, q, feasible):
    """dict(col_of_robot (n; NONE: unassigned), size, total_q) of bidder -> column over the padded problem"""
    n, m = q.shape
    col = np.full(n, NONE, np.uint32)
    for i in range(n):
        j = int(mine[i])
        if j < m and feasible[i, j]:
            col[i] = j
    got = col != NONE
    return dict(col_of_robot=col, size=int(got.sum()), total_q=int(q[np.flatnonzero(got), col[got].astype(np.int64)].sum()))


def auction(q, feasible, max_rounds: int | None = None):
    """The synchronous auction of mnav_fleet_assign: dict(col_of_robot, size, total_q, phases, rounds, bids), or None when
    max_rounds is reached.  Costs scaled by N + 1; eps from max(1, C / 2) by / 8 down to 1, prices kept across phases; a
    round: every unassigned bidder bids price + (second - best) + eps on its best column (ties: smallest column), every
    column takes its highest bid (ties: smallest bidder) and evicts its owner."""
    cost, N, M = padded(q, feasible)
    cost = cost * (N + 1)
    eps = max(1, int(cost.max()) // 2)
    price = np.zeros(N, np.int64)
    owner, mine = np.full(N, -1, np.int64), np.full(N, -1, np.int64)
    phases, rounds, bids = 1, 0, 0
    while True:
        un = np.flatnonzero(mine < 0)
        w = cost[un] + price[None, :]
        ar = np.arange(un.size)
        j1 = w.argmin(axis=1)                                           # the first minimum: ties to the smallest column
        w1 = w[ar, j1]
        w[ar, j1] = I64MAX
        w2 = w.min(axis=1)
        bid = price[j1] + np.where(w2 == I64MAX, 0, w2 - w1) + eps
        assert (bid < 2 ** 62).all()
        bids += un.size
        order = np.lexsort((un, -bid, j1))                              # by column, then the highest bid, then the smallest bidder
        first = np.ones(order.size, bool)
        first[1:] = j1[order][1:] != j1[order][:-1]
        win = order[first]
        cols, who = j1[win], un[win]
        old = owner[cols]
        mine[old[old >= 0]] = -1
        owner[cols], mine[who], price[cols] = who, cols, bid[win]
        rounds += 1
        if not (mine < 0).any():
            if eps == 1:
                break
            eps, phases = max(1, eps // 8), phases + 1
            owner[:], mine[:] = -1, -1
        if max_rounds is not None and rounds >= max_rounds:
            return None
    out = result_of(mine, q, feasible)
    out.update(phases=phases, rounds=rounds, bids=bids, mine=mine.astype(np.uint32))
    return out


def exact(q, feasible):
    """(size, total_q) of a maximum-size, then minimum-sum assignment: the O(N^3) Hungarian method (shortest augmenting
    paths with potentials) on the padded costs, independent of the auction"""
    cost, N, M = padded(q, feasible)
    u, v = np.zeros(N + 1, np.int64), np.zeros(N + 1, np.int64)
    p, way = np.zeros(N + 1, np.int64), np.zeros(N + 1, np.int64)       # p[j]: the row of column j (1-based, 0: none)
    for i in range(1, N + 1):
        p[0] = i
        j0 = 0
        minv = np.full(N + 1, I64MAX, np.int64)
        used = np.zeros(N + 1, bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            cur = cost[i0 - 1] - u[i0] - v[1:]
            free = ~used[1:]
            better = free & (cur < minv[1:])
            minv[1:][better] = cur[better]
            way[1:][better] = j0
            cand = np.where(free, minv[1:], I64MAX)
            j1 = int(cand.argmin()) + 1
            delta = cand[j1 - 1]
            u[p[used]] += delta
            v[used] -= delta
            minv[1:][free] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    n, m = q.shape
    size = total = 0
    for j in range(1, m + 1):
        i = int(p[j]) - 1
        if i < n and feasible[i, j - 1]:
            size, total = size + 1, total + int(q[i, j - 1])
    return size, total
