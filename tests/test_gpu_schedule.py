"""GPU: the fleet schedule (mnav_fleet_schedule, mnav_schedule_stats).  Every comparison is exact:
statuses, delays, rounds, cells and holders are integers, departures and potentials are compared by bits.

Per robot status, delay, committed departure and round, the cells, holders, peaks, windows and both sets of statistics equal
tests/schedule_model.py (which tests/test_fleet_schedule_model.py pins on the CPU) over the shapes that reach every path of
the probe; without the model, no cell exceeds the capacity and a replay of the committed robots through
mnav_fleet_timed_traffic at their new departures gives the same cells with nothing over and nobody yielding; schedules on
top of reservations; round limits, chunking and both ways of cleaning give the same bits; the hot spot of one plan; refusals
touch nothing; the layer prices the schedule's peaks.

The conditions on the model's values (at least 40 % of the contributors committed, some NO_SLOT, some delay above 0, at least
3 rounds; a committed delay of 64 or more with 100 windows) are asserted from 257 robots on wherever the scenario can meet
them: 257 robots (162 contributors) in 100 windows all find a slot, so that pair has no NO_SLOT and no delay of 64 -- the 1200
robots of the same shape have both -- and 860 contributors do not fit 37 windows of capacity 1 (202 commit), where the 257
robots of that shape commit 117 of 162.

Shapes: the world of tests/test_gpu_fleet.py -- terrain(48) = 2304 vertices, 8 plans -- and up to 1200 robots where the
model is in the loop, 3000 on one plan for the committed rounds of the stagger scenario."""
import ctypes as C

import numpy as np
import pytest

from mesh_navigation_amd import capi
from tests import fleet_model as FM
from tests import schedule_model as SM
from tests import timed_traffic_model as XM
from tests import traffic_model as TM
from tests.fleet_model import bits
from tests.test_fleet_schedule_model import COUNTS, STAGGER_SCHEDULE, timing
from tests.test_gpu_fleet import LIMIT, OFFSET, World, make_ctx, robots
from tests.test_gpu_timed_traffic import OUTPUTS as TT_OUTPUTS, STATS as TT_STATS, same_cells, same_snapshot, snapshot
from tests.test_gpu_traffic import FAR
from tests.test_timed_traffic_model import STAGGER_FREE, STAGGER_ROBOTS, STAGGER_WINDOWS, largest_potential

pytestmark = pytest.mark.gpu
SENTINEL = 0xDEADBEEF
F = np.float32
SIZES = (1, 63, 64, 65, 257, 1200)
TIMED_STATS = ("contributing", "adds", "beyond_horizon", "total_weight", "occupied_cells", "over_cells", "largest_cell", "yielding", "windows")
# windows, max_delay, capacity, weights 1 .. 3, flags: each the smallest shape that reaches a distinct path of the probe
SHAPES = {"B37": (37, 36, 1, False, 0),                   # masked lanes, B not a power of two
          "B100": (100, 99, 1, False, 0),                 # a second block of 64 candidates
          "cap3": (64, 20, 3, True, 0),
          "cap2_heavy": (64, 63, 2, True, 0),             # w > capacity is NO_SLOT at once
          "seed_free": (64, 63, 1, False, SM.SEED_FREE)}


@pytest.fixture(scope="module")
def world():
    return World()


_runs = {}


def run_of(W, fields, offset, n, seed=5):
    """robots(W, fields, n, seed) and FM.run over them, computed once per (offset, n, seed)"""
    key = (W.version, offset, n, seed)
    if key not in _runs:
        sl, vt = robots(W, fields, n, seed)
        _runs[key] = (sl, vt, FM.run(fields, W.V, sl, vt))
    return _runs[key]


def check_schedule(ctx, W, fields, slots, vtx, where, state, run=None, **kw):
    """one fleet_schedule call against the model on `state`: outputs, cells, holders, peaks, windows, both statistics"""
    got = ctx.fleet_schedule(slots, vtx, **kw)
    want = SM.schedule(state, fields, slots, vtx, kw.get("weights"), kw.get("depart"), kw.get("pace"), kw.get("key"), kw.get("windows", 64), kw.get("tau", 1.0),
                       kw.get("capacity", 1), kw.get("max_delay", 0), kw.get("max_rounds", 0), kw.get("flags", 0), kw.get("accumulate", False), run=run)
    assert want is not None, where
    assert np.array_equal(got["vertex"], vtx) and np.array_equal(got["codes"], want["codes"]) and np.array_equal(bits(got["potential"]), bits(want["potential"])), where
    for k in ("status", "delay", "round"):
        assert np.array_equal(got[k], want[k]), (where, k, np.flatnonzero(got[k] != want[k])[:8], got[k][got[k] != want[k]][:8], want[k][got[k] != want[k]][:8])
    assert np.array_equal(bits(got["depart"]), bits(want["depart_out"])), where
    same_cells(ctx, state, where)
    st, ts = ctx.schedule_stats(), ctx.timed_traffic_stats()
    print(where, "n", len(slots), {k: st[k] for k in COUNTS}, "ms kernels %.3f total %.3f" % (st["ms_kernels"], st["ms_total"]))
    assert {k: st[k] for k in COUNTS} == {k: want[k] for k in COUNTS}, (where, st, {k: want[k] for k in COUNTS})
    assert {k: ts[k] for k in TIMED_STATS} == want["timed"], (where, ts, want["timed"])
    return want, got


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_device_equals_the_model(world, shape):
    W = world
    B, max_delay, capacity, weighted, flags = SHAPES[shape]
    ctx = make_ctx(W)
    try:
        ctx.plan_dijkstra_batch(W.seeds, W.targets, FAR, LIMIT)
        fields = W.fields(offset=FAR)
        state = XM.Cells(W.V)
        for n in SIZES:
            sl, vt, run = run_of(W, fields, FAR, n)
            depart, pace, key, tau = timing(n, fields, 11 * n + B)
            w = np.random.default_rng(n).integers(1, 4, n).astype(np.uint32) if weighted else None
            ctx.fleet_paths(sl, vt)
            ctx.fleet_traffic(sl, vt)
            fs, cs = ctx.fleet_stats(), ctx.traffic_stats()                   # of those two calls: a schedule moves neither
            want, _ = check_schedule(ctx, W, fields, sl, vt, (shape, n), state, run, weights=w, depart=depart, pace=pace, key=key, windows=B, tau=tau, capacity=capacity,
                                     max_delay=max_delay, flags=flags)
            assert ctx.fleet_stats() == fs and ctx.traffic_stats() == cs, (shape, n)
            if n >= 257:                                                      # conditions on the MODEL's values
                assert want["delayed"] > 0 and want["rounds"] >= 3, (shape, n, want["per_round"])
                if (shape, n) != ("B100", 257):                               # (162 contributors in 100 windows all find a slot inside the horizon)
                    assert want["no_slot"] > 0, (shape, n)
                if (shape, n) != ("B37", 1200):                               # (860 contributors do not fit 37 windows: 202 do)
                    assert 5 * want["committed"] >= 2 * want["contributing"], (shape, n, want["committed"], want["contributing"])
                if shape == "B100" and n == 1200:
                    assert want["max_delay_used"] >= 64, want["max_delay_used"]
                if shape == "cap2_heavy":
                    heavy = (w == 3) & (want["status"] != SM.ST_NONE)
                    assert heavy.any() and (want["status"][heavy] == SM.NO_SLOT).all()
                if not flags:
                    assert int(state.cell.max()) <= capacity
    finally:
        ctx.close()


def test_capacity_holds_and_the_replay_counts_the_same_cells(world):
    """without the model: no cell above capacity, and the committed robots at their new departures ARE the cells"""
    W = world
    ctx = make_ctx(W)
    try:
        ctx.plan_dijkstra_batch(W.seeds, W.targets, FAR, LIMIT)
        fields = W.fields(offset=FAR)
        for n, capacity, weighted in ((1200, 1, False), (1000, 3, True)):
            sl, vt = robots(W, fields, n, 21)
            depart, pace, key, tau = timing(n, fields, 3 + n)
            w = np.random.default_rng(n).integers(1, 4, n).astype(np.uint32) if weighted else np.ones(n, np.uint32)
            got = ctx.fleet_schedule(sl, vt, weights=w, depart=depart, pace=pace, key=key, windows=64, tau=tau, capacity=capacity, max_delay=63)
            d, ts, ss = ctx.timed_traffic_download(), ctx.timed_traffic_stats(), ctx.schedule_stats()
            done = got["status"] == capi.SCHEDULE_COMMITTED
            assert int(d["cells"].max()) <= capacity and ts["over_cells"] == 0 and ts["largest_cell"] <= capacity, (n, capacity)
            assert ss["committed"] == int(done.sum()) > n // 5 and ss["no_slot"] > 0 and ss["open"] == 0 and ss["delayed"] == int((got["delay"][done] > 0).sum()) > 0
            assert np.isinf(got["depart"][~done]).all() and (got["delay"][~done] == capi.NONE).all()
            replay = ctx.fleet_timed_traffic(sl, vt, weights=np.where(done, w, 0).astype(np.uint32), depart=np.where(done, got["depart"], 0).astype(F), pace=pace, key=key,
                                             windows=64, tau=tau, free_count=capacity)
            d2, ts2 = ctx.timed_traffic_download(), ctx.timed_traffic_stats()
            assert all(np.array_equal(d[k], d2[k]) for k in ("cells", "holders", "peak", "window")), (n, capacity)
            assert ts2["beyond_horizon"] == 0 and ts2["over_cells"] == 0 and ts2["yielding"] == 0 and not replay["yield_hops"].any()
            assert {k: ts2[k] for k in TIMED_STATS} == {k: ts[k] for k in TIMED_STATS}, (ts, ts2)
    finally:
        ctx.close()


def test_reservations_of_earlier_calls(world):
    """a second schedule on top of a first; a schedule on top of a timed count that already has cells above capacity"""
    W = world
    ctx = make_ctx(W)
    try:
        ctx.plan_dijkstra_batch(W.seeds, W.targets, FAR, LIMIT)
        fields = W.fields(offset=FAR)
        n = 1000
        sl, vt, _ = run_of(W, fields, FAR, n, 8)
        depart, pace, key, tau = timing(n, fields, 14)
        kw = dict(windows=64, tau=tau, capacity=2, max_delay=40)
        a, b = slice(0, 437), slice(437, n)
        state = XM.Cells(W.V)
        first, _ = check_schedule(ctx, W, fields, sl[a], vt[a], "first half", state, depart=depart[a], pace=pace[a], key=key[a], **kw)
        second, _ = check_schedule(ctx, W, fields, sl[b], vt[b], "second half", state, depart=depart[b], pace=pace[b], key=key[b], accumulate=True, **kw)
        assert int(state.cell.max()) <= 2 and second["timed"]["total_weight"] == first["committed"] + second["committed"] and second["delayed"] > 0
        # (two halves are NOT required to equal one call over the whole fleet: the first half never sees the second)
        state = XM.Cells(W.V)
        t = ctx.fleet_timed_traffic(sl[a], vt[a], depart=depart[a], pace=pace[a], key=key[a], windows=64, tau=tau, free_count=2)
        XM.timed(state, fields, sl[a], vt[a], None, depart[a], pace[a], key[a], 64, tau, 2)
        over = ctx.timed_traffic_stats()["over_cells"]
        assert over > 0 and t["codes"].size == 437
        before = state.cell.copy()
        on_top, _ = check_schedule(ctx, W, fields, sl[b], vt[b], "on a count", state, depart=depart[b], pace=pace[b], key=key[b], accumulate=True, **kw)
        grown = state.cell > before
        assert on_top["committed"] > 50 and int(state.cell[grown].max()) <= 2 and on_top["timed"]["over_cells"] == over      # blocked cells stay as they were
    finally:
        ctx.close()


def test_round_limits_chunks_and_cleaning(world):
    W = world
    ctx = make_ctx(W)
    try:
        ctx.plan_dijkstra_batch(W.seeds, W.targets, FAR, LIMIT)
        fields = W.fields(offset=FAR)
        n = 1200
        sl, vt, run = run_of(W, fields, FAR, n)
        depart, pace, key, tau = timing(n, fields, 19)
        kw = dict(depart=depart, pace=pace, key=key, windows=64, tau=tau, capacity=1, max_delay=63)
        full, got = check_schedule(ctx, W, fields, sl, vt, "default", XM.Cells(W.V), run, **kw)
        cells = ctx.timed_traffic_download()
        assert full["rounds"] > 10 and full["open"] == 0                      # more rounds than the default chunk
        for limit in (1, 2):
            want, _ = check_schedule(ctx, W, fields, sl, vt, ("max_rounds", limit), XM.Cells(W.V), run, max_rounds=limit, **kw)
            assert want["open"] > 0 and want["rounds"] == limit and want["per_round"] == full["per_round"][:limit]
        for option, value in (("schedule_chunk_rounds", 1), ("schedule_chunk_rounds", 5), ("schedule_clean_fill", 1), ("schedule_clean_fill", 0)):
            ctx.set_option(option, value)
            again = ctx.fleet_schedule(sl, vt, **kw)
            ctx.set_option(option, None)
            d = ctx.timed_traffic_download()
            assert all(np.array_equal(bits(again[k]) if again[k].dtype == F else again[k], bits(got[k]) if got[k].dtype == F else got[k]) for k in got), (option, value)
            assert all(np.array_equal(d[k], cells[k]) for k in cells), (option, value)
            assert {k: ctx.schedule_stats()[k] for k in COUNTS} == {k: full[k] for k in COUNTS}, (option, value)
    finally:
        ctx.close()


@pytest.mark.parametrize("flags", [0, SM.SEED_FREE])
def test_hot_spot(world, flags):
    """1000 robots on ONE plan: every contributor's last visit lands on the seed -- the same-address case of all four atomics"""
    W = world
    ctx = make_ctx(W)
    try:
        ctx.plan_dijkstra_batch(W.seeds, W.targets, FAR, LIMIT)
        fields = W.fields(offset=FAR)
        vt = np.random.default_rng(3).integers(0, W.V, 1000).astype(np.uint32)
        sl = np.zeros(1000, np.uint32)
        tau = float(F(largest_potential(fields[:1]) / 48))
        key = np.random.default_rng(4).integers(0, 300, 1000).astype(np.uint32)
        state = XM.Cells(W.V)
        want, _ = check_schedule(ctx, W, fields, sl, vt, ("hot spot", flags), state, key=key, windows=64, tau=tau, capacity=1, max_delay=63, flags=flags)
        seed = fields[0].seed
        assert want["contributing"] > 900 and want["committed"] == int(state.cell[seed].astype(np.uint64).sum())
        assert (int(state.cell[seed].max()) > 1) == bool(flags) and want["no_slot"] > 0
    finally:
        ctx.close()


def test_the_committed_rounds_of_the_stagger_scenario(world):
    """the rounds of tests/test_fleet_schedule_model.py::test_the_stagger_scenario_through_the_schedule on the device: round by
    round (max_rounds = 1, 2, ...) the claims and commits are the committed figures"""
    W = world
    ctx = make_ctx(W)
    try:
        ctx.plan_dijkstra_batch(W.seeds, W.targets, FAR, LIMIT)
        fields = W.fields(offset=FAR)
        vt = np.random.default_rng(3).integers(0, W.V, STAGGER_ROBOTS).astype(np.uint32)
        sl = np.zeros(STAGGER_ROBOTS, np.uint32)
        tau = float(F(largest_potential(fields[:1]) / 48))
        for flags, (figures, per_round) in STAGGER_SCHEDULE.items():
            seen, claims, committed = [], 0, 0
            for limit in range(1, len(per_round) + 1):
                ctx.fleet_schedule(sl, vt, windows=STAGGER_WINDOWS, tau=tau, capacity=STAGGER_FREE, max_delay=STAGGER_WINDOWS - 1, max_rounds=limit, flags=flags)
                st = ctx.schedule_stats()
                seen.append((st["claims"] - claims, st["committed"] - committed))
                claims, committed = st["claims"], st["committed"]
                assert st["rounds"] == limit
            assert tuple(seen) == per_round and (st["contributing"], st["committed"], st["no_slot"], st["rounds"]) == figures and st["open"] == 0, (flags, seen, st)
            cells = ctx.timed_traffic_download()["cells"].copy()
            if flags:
                cells[fields[0].seed] = 0
            assert int(cells.max()) <= STAGGER_FREE
    finally:
        ctx.close()


def raw_schedule(ctx, slots, vtx, weights=None, depart=None, pace=None, key=None, windows=64, tau=1.0, capacity=1, max_delay=0, max_rounds=0, flags=0, accumulate=False):
    """the C call with sentinel-filled outputs: (rc, outputs untouched)"""
    n = len(slots)
    sl, vt = (np.ascontiguousarray(a, np.uint32) for a in (slots, vtx))
    w, ky = (None if a is None else np.ascontiguousarray(a, np.uint32) for a in (weights, key))
    dp, pc = (None if a is None else np.ascontiguousarray(a, np.float32) for a in (depart, pace))
    ints = [np.full(n, SENTINEL, np.uint32) for _ in range(5)]
    pot, out = np.full(n, np.nan, np.float32), np.full(n, np.nan, np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = ctx._L.mnav_fleet_schedule(ctx._h, n, p(sl), p(vt), None, p(w), p(dp), p(pc), p(ky), int(windows), float(tau), int(capacity), int(max_delay), int(max_rounds),
                                    int(flags), 1 if accumulate else 0, p(ints[0]), p(ints[1]), p(pot), p(ints[2]), p(ints[3]), p(out), p(ints[4]))
    return rc, all((a == SENTINEL).all() for a in ints) and np.isnan(pot).all() and np.isnan(out).all()


def test_refusals_touch_nothing(world):
    W = world
    ctx = make_ctx(W)
    old = W.costs
    try:
        one = np.zeros(1, np.uint32)
        rc, clean = raw_schedule(ctx, one, W.targets[:1])                    # no plan yet
        assert rc == -1 and clean and ctx.schedule_stats()["rounds"] == 0 and ctx.timed_traffic_stats()["windows"] == 0
        seeds, targets = W.seeds[:6], W.targets[:6].copy()
        ctx.plan_dijkstra_batch(seeds, targets, OFFSET, LIMIT)
        fields = W.fields(targets)[:6]
        n = 300
        sl, vt = robots(W, fields, n, 8)
        depart, pace, key, tau = timing(n, fields, 2)
        kw = dict(depart=depart, pace=pace, key=key, windows=64, tau=tau, capacity=1, max_delay=63)
        state = XM.Cells(W.V)
        check_schedule(ctx, W, fields, sl, vt, "start", state, **kw)
        snap, stats = snapshot(ctx), ctx.schedule_stats()
        assert snap[1]["total_weight"] > 20

        def refused(what, **over):
            args = dict(kw)
            args.update(over)
            slots, vtx = args.pop("slots", sl), args.pop("vtx", vt)
            for acc in (False, True) if "accumulate" not in over else (over["accumulate"],):
                args["accumulate"] = acc
                rc, clean = raw_schedule(ctx, slots, vtx, **args)
                assert rc == -1 and clean and what in ctx._err() and same_snapshot(ctx, snap) and ctx.schedule_stats() == stats, (over.keys(), acc, rc, ctx._err())

        def bad(like, at, value):
            a = like.copy()
            a[at] = value
            return a
        refused("capacity must be at least 1", capacity=0)
        for md in (64, 2 ** 31):
            refused("max_delay must be below windows", max_delay=md)
        for fl in (2, 3, 2 ** 31):
            refused("unknown flag bit", flags=fl)
        # the timed call's refusals
        for B in (0, 1025):
            refused("windows out of range", windows=B, max_delay=0)
        for t in (0.0, np.nan, np.inf, 1e39):
            refused("tau must be finite and positive", tau=t)
        refused("departure time", depart=bad(depart, n - 1, -1.0))
        refused("pace", pace=bad(pace, 0, 0.0))
        for r in (dict(windows=63, max_delay=20), dict(tau=2 * tau)):
            refused("differ from the cells' configuration", accumulate=True, **r)
        refused("total weight does not fit the counters", weights=np.full(n, 2 ** 31, np.uint32))
        refused("slot out of range", slots=np.full(n, 8, np.uint32))
        ctx.set_option("timed_traffic_max_mb", 0)                              # the memory cap: cells, holders and the tentative arrays
        refused("timed_traffic_max_mb")
        ctx.set_option("timed_traffic_max_mb", SM.BYTES_PER_CELL * W.V * 64 / 1048576.0)      # exactly what 64 windows take
        refused("timed_traffic_max_mb", windows=65, accumulate=False)
        check_schedule(ctx, W, fields, sl[:50], vt[:50], "at the cap", state, depart=depart[:50], pace=pace[:50], key=key[:50], windows=64, tau=tau, capacity=1, max_delay=63,
                       accumulate=True)
        ctx.set_option("timed_traffic_max_mb", None)
        # stale fields until the per-plan replan has run
        snap, stats = snapshot(ctx), ctx.schedule_stats()
        ids = np.array([W.mesh.vertex_at(0.5, 0.5), W.mesh.vertex_at(0.52, 0.5), int(targets[0])], np.uint32)
        ids = ids[~np.isin(ids, seeds)]
        W.change_costs(ctx, ids, 0.45)
        refused("costs changed")
        ctx.replan_dijkstra_each(None, OFFSET, want_pred=True)
        fields = W.fields(targets)[:6]
        want, _ = check_schedule(ctx, W, fields, sl, vt, "after the replan", XM.Cells(W.V), **kw)
        assert want["committed"] > 50
        # n = 0: with accumulate nothing happens, without it the cells start over
        ctx.fleet_schedule(np.zeros(0, np.uint32), np.zeros(0, np.uint32), windows=64, tau=tau, accumulate=True)
        assert ctx.timed_traffic_stats()["total_weight"] == want["timed"]["total_weight"]
        ctx.fleet_schedule(np.zeros(0, np.uint32), np.zeros(0, np.uint32), windows=64, tau=tau)
        d = ctx.timed_traffic_download()
        assert not d["cells"].any() and (d["holders"] == FM.NONE).all() and not d["peak"].any() and ctx.timed_traffic_stats()["total_weight"] == 0
        assert ctx.schedule_stats()["contributing"] == 0 and ctx.schedule_stats()["rounds"] == 0
    finally:
        ctx.close()
        if W.costs is not old:
            W.costs = old
            W.weights = W.om.edge_weights(W.case.edge_dist, W.costs, 1.0)
            W.version += 1


def test_the_layer_prices_the_schedule(world):
    W = world
    ctx = make_ctx(W)
    try:
        ctx.plan_dijkstra_batch(W.seeds, W.targets, FAR, LIMIT)
        fields = W.fields(offset=FAR)
        n = 1200
        sl, vt, run = run_of(W, fields, FAR, n)
        depart, pace, key, tau = timing(n, fields, 23)
        w = np.random.default_rng(5).integers(1, 4, n).astype(np.uint32)
        state = XM.Cells(W.V)
        check_schedule(ctx, W, fields, sl, vt, "layer", state, run, weights=w, depart=depart, pace=pace, key=key, windows=64, tau=tau, capacity=3, max_delay=63, flags=SM.SEED_FREE)
        peak = state.peak
        assert peak.max() > 3                                                  # the seeds' arrivals are counted
        for free_count, gain, cap in ((0, 1.0, np.inf), (1, 0.125, 1.0), (3, 0.3, 9.0)):
            ctx.layer_timed_traffic(3, free_count, gain, cap)
            cost, lethal = ctx.layer_download(3)
            assert np.array_equal(bits(cost), bits(TM.cost(peak, free_count, gain, cap))) and not lethal.any(), (free_count, gain, cap)
    finally:
        ctx.close()


def test_the_occupancy_calls_grow_the_buffers_the_next_one_uses(world):
    """mnav_fleet_traffic, mnav_fleet_timed_traffic and mnav_fleet_schedule share the fleet scratch, the per-robot weight /
    depart / pace / key arrays and the cells, and each call grows what the next one then uses.  Ten calls whose arguments do
    not depend on where they stand -- traffic with 3 robots; timed traffic with 200 robots in 70 windows (past 64: the peak
    pass's lanes per vertex saturate); a schedule of 1 robot in 5 windows (the cells are made anew); a schedule of 200 robots
    in 70 windows with all four per-robot arrays; timed traffic accumulated on top; traffic with 200 weighted robots; a
    schedule of 300 robots (a second block of kFleetBlock = 256); n = 0 without accumulate to each of the three -- on a fresh
    context in this order, on a second fresh context in the opposite order and on the first once more in the opposite order.
    Every output of a call by its bits, its counts or cells, holders, peaks and windows and every statistic but the times
    are the same in the three runs; the accumulating call, whose cells depend on the schedule before it (200 robots going
    up, 300 coming down), equals the model on the model's cells of that schedule; no call moves fleet_stats() or the
    statistics of an entry point whose state it does not write."""
    W = world
    fields = W.fields(offset=FAR)
    tau = timing(1, fields, 0)[3]
    none = np.zeros(0, np.uint32)

    def fleet(n, seed):
        sl, vt, run = run_of(W, fields, FAR, n, seed)
        depart, pace, key, _ = timing(n, fields, seed)
        w = np.random.default_rng(seed).integers(1, 4, n).astype(np.uint32)
        return sl, vt, run, dict(weights=w, depart=depart, pace=pace, key=key)

    r3, r1, ra, rb, rc, rd, re = fleet(3, 41), fleet(1, 42), fleet(200, 43), fleet(200, 44), fleet(200, 45), fleet(200, 46), fleet(300, 47)
    calls = [("traffic", r3, dict()),
             ("timed", ra, dict(weights=ra[3]["weights"], windows=70, tau=tau, free_count=1)),
             ("schedule", r1, dict(windows=5, tau=tau, capacity=1, max_delay=4)),
             ("schedule", rb, dict(rb[3], windows=70, tau=tau, capacity=3, max_delay=40)),
             ("timed", rc, dict(rc[3], windows=70, tau=tau, free_count=3, accumulate=True)),
             ("traffic", rd, dict(weights=rd[3]["weights"])),
             ("schedule", re, dict(re[3], windows=70, tau=tau, capacity=2, max_delay=69)),
             ("traffic", (none, none, None, {}), dict()),
             ("timed", (none, none, None, {}), dict(windows=70, tau=tau)),
             ("schedule", (none, none, None, {}), dict(windows=70, tau=tau))]
    ON_TOP = 4

    def fresh():
        ctx = make_ctx(W)
        ctx.plan_dijkstra_batch(W.seeds, W.targets, FAR, LIMIT)
        return ctx

    def plain(stats):
        return {k: v for k, v in stats.items() if not k.startswith("ms_")}

    def run(ctx, order):
        seen = {}
        for k in order:
            kind, (sl, vt, _, _), kw = calls[k]
            fs, others = ctx.fleet_stats(), (ctx.traffic_stats(), ctx.timed_traffic_stats(), ctx.schedule_stats())
            if kind == "traffic":
                out = ctx.fleet_traffic(sl, vt, **kw)
                state = dict(counts=ctx.traffic_download(), traffic=plain(ctx.traffic_stats()))
                assert (ctx.timed_traffic_stats(), ctx.schedule_stats()) == others[1:], (order, k)
            else:
                out = ctx.fleet_timed_traffic(sl, vt, **kw) if kind == "timed" else ctx.fleet_schedule(sl, vt, **kw)
                state = dict(ctx.timed_traffic_download(), timed=plain(ctx.timed_traffic_stats()), schedule=plain(ctx.schedule_stats()) if kind == "schedule" else {})
                assert ctx.traffic_stats() == others[0] and (kind == "schedule" or ctx.schedule_stats() == others[2]), (order, k)
            assert ctx.fleet_stats() == fs, (order, k)
            seen[k] = (out, state)
        return seen

    def same(a, b):
        return a == b if isinstance(a, dict) else a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))

    def assert_same_calls(a, b, what):
        for k in range(len(calls)):
            if k != ON_TOP:
                for x, y in zip(a[k], b[k]):
                    assert x.keys() == y.keys() and all(same(x[f], y[f]) for f in x), (what, k, [f for f in x if not same(x[f], y[f])])

    def assert_on_top(got, before, where):
        """the accumulating call against the model: on the cells the model's schedule `before` leaves"""
        _, (sl, vt, r, _), kw = calls[before]
        cells = XM.Cells(W.V)
        assert SM.schedule(cells, fields, sl, vt, kw["weights"], kw["depart"], kw["pace"], kw["key"], 70, tau, kw["capacity"], kw["max_delay"], run=r) is not None
        _, (sl, vt, r, _), kw = calls[ON_TOP]
        want = XM.timed(cells, fields, sl, vt, kw["weights"], kw["depart"], kw["pace"], kw["key"], 70, tau, kw["free_count"], True, run=r)
        out, state = got
        assert np.array_equal(out["vertex"], vt) and all(np.array_equal(out[f], want[f]) for f in TT_OUTPUTS if f != "vertex"), where
        assert np.array_equal(bits(out["potential"]), bits(want["potential"])) and np.array_equal(bits(out["first_yield_time"]), bits(want["first_yield_time"])), where
        assert np.array_equal(state["cells"], cells.cell) and np.array_equal(state["holders"], cells.holder), where
        assert np.array_equal(state["peak"], cells.peak) and np.array_equal(state["window"], cells.window), where
        assert {f: state["timed"][f] for f in TT_STATS} == {f: want[f] for f in TT_STATS} and want["contributing"] > 50 and want["over_cells"] > 0, (where, state["timed"])

    up_order, down_order = tuple(range(len(calls))), tuple(reversed(range(len(calls))))
    a, b = fresh(), fresh()
    try:
        up = run(a, up_order)
        down = run(b, down_order)
        assert_same_calls(up, down, "each call grows what the next uses, up / down")
        a.fleet_paths(r3[0], r3[1])                                   # fleet_stats() tells of a call: the occupancy calls put it back
        assert a.fleet_stats()["served"] + a.fleet_stats()["beyond_field"] + a.fleet_stats()["no_path"] + a.fleet_stats()["invalid"] == 3
        again = run(a, down_order)
        assert_same_calls(up, again, "over the capacities left")
        assert_on_top(up[ON_TOP], 3, "on the 200-robot schedule")
        assert_on_top(down[ON_TOP], 6, "on the 300-robot schedule")
        for x, y in zip(down[ON_TOP], again[ON_TOP]):
            assert all(same(x[f], y[f]) for f in x), "on the 300-robot schedule, again"
        # what the calls were: the schedules commit and delay, the n = 0 calls leave nothing
        assert up[3][1]["schedule"]["committed"] > 50 and up[3][1]["schedule"]["delayed"] > 0 and up[6][1]["schedule"]["committed"] > 50
        assert up[1][1]["timed"]["windows"] == 70 and up[2][1]["timed"]["windows"] == 5 and up[5][1]["traffic"]["contributing"] > 50
        assert not up[7][1]["counts"].any() and not up[8][1]["cells"].any() and not up[9][1]["cells"].any() and up[9][1]["cells"].shape == (W.V, 70)
    finally:
        a.close()
        b.close()
