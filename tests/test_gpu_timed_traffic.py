"""GPU: timed fleet traffic (mnav_fleet_timed_traffic, mnav_timed_traffic_download, mnav_timed_traffic_stats,
mnav_layer_timed_traffic, mnav_map_timed_traffic).  Every comparison is exact: cells, holders and
the report are integers, times, potentials and costs are compared by bits.

Cells, holders, peaks, windows, every per-robot output and every statistic equal tests/timed_traffic_model.py (which
tests/test_timed_traffic_model.py pins on the CPU); with a horizon that holds everything the sum over the windows is what
mnav_fleet_traffic counts for the same robots in the same context, and neither mnav_fleet_stats nor mnav_traffic_stats
moves.  The layer equals the traffic cost rule on the peaks, the graph update equals tests/map_model.py fed with those
costs, one round of plan -> timed traffic -> map update -> replan ends on the oracle's fresh plans, and the stagger loop
runs the rounds of the CPU test.

Shapes: the world of tests/test_gpu_fleet.py -- terrain(48) = 2304 vertices, 8 plans of which one has seed == target and
one a target out of range -- and up to 3000 robots, 1 to 100 windows."""
import ctypes as C

import numpy as np
import pytest

from mesh_navigation_amd import capi
from tests import fleet_model as FM
from tests import map_model as MM
from tests import timed_traffic_model as XM
from tests import traffic_model as TM
from tests.fleet_model import bits
from tests.test_gpu_fleet import LIMIT, OFFSET, World, make_ctx, robots
from tests.test_gpu_traffic import CONTRIBUTORS, FAR, NODES, oracle_fields, same_map
from tests.test_timed_traffic_model import (STAGGER, STAGGER_FREE, STAGGER_ROBOTS, STAGGER_WINDOWS, largest_potential, stagger, timing)

pytestmark = pytest.mark.gpu
SENTINEL = 0xDEADBEEF
F = np.float32
SIZES = (1, 63, 64, 65, 255, 256, 257, 3000)
OUTPUTS = ("codes", "vertex", "conflict_hops", "yield_hops", "first_yield_vertex", "first_yield_window")
STATS = ("contributing", "adds", "beyond_horizon", "total_weight", "occupied_cells", "over_cells", "largest_cell", "yielding", "windows")


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


def same_cells(ctx, state, where):
    d = ctx.timed_traffic_download()
    assert d["cells"].dtype == np.uint32 and d["cells"].shape == (state.V, state.B), (where, d["cells"].shape)
    assert np.array_equal(d["cells"], state.cell), (where, np.argwhere(d["cells"] != state.cell)[:8])
    assert np.array_equal(d["holders"], state.holder), (where, np.argwhere(d["holders"] != state.holder)[:8])
    assert np.array_equal(d["peak"], state.peak) and np.array_equal(d["window"], state.window), where
    return d


def check_timed(ctx, W, fields, slots, vtx, where, state, run=None, **kw):
    """one fleet_timed_traffic call against the model on `state`: outputs, cells, holders, peaks, windows, statistics"""
    t = ctx.fleet_timed_traffic(slots, vtx, **kw)
    want = XM.timed(state, fields, slots, vtx, kw.get("weights"), kw.get("depart"), kw.get("pace"), kw.get("key"), kw.get("windows", 64), kw.get("tau", 1.0),
                    kw.get("free_count", 0), kw.get("accumulate", False), run=run)
    assert want is not None, where
    assert np.array_equal(t["vertex"], vtx), where
    for k in OUTPUTS:
        if k != "vertex":
            assert np.array_equal(t[k], want[k]), (where, k, np.flatnonzero(t[k] != want[k])[:8])
    assert np.array_equal(bits(t["potential"]), bits(want["potential"])) and np.array_equal(bits(t["first_yield_time"]), bits(want["first_yield_time"])), where
    same_cells(ctx, state, where)
    st = ctx.timed_traffic_stats()
    print(where, "n", len(slots), {k: st[k] for k in STATS}, "ms kernels %.3f total %.3f" % (st["ms_kernels"], st["ms_total"]))
    assert {k: st[k] for k in STATS} == {k: want[k] for k in STATS}, (where, st, {k: want[k] for k in STATS})
    return want


@pytest.mark.parametrize("B", [1, 3, 64, 100])
@pytest.mark.parametrize("offset", [OFFSET, FAR], ids=["offset_0.3", "offset_far"])
def test_cells_equal_the_model(world, offset, B):
    W = world
    ctx = make_ctx(W)
    try:
        d = ctx.timed_traffic_download()                                     # nothing after upload_mesh
        assert not d["peak"].any() and (d["window"] == FM.NONE).all() and d["cells"].shape == (W.V, 0) and ctx.timed_traffic_stats()["total_weight"] == 0
        ctx.plan_dijkstra_batch(W.seeds, W.targets, offset, LIMIT)
        if offset == FAR:
            ctx.set_option("timed_peak_blocks", 3)                           # the peak pass strides: 3 blocks over 2304 vertices
        fields = W.fields(offset=offset)
        top = largest_potential(fields)
        state = XM.Cells(W.V)
        for n in SIZES:
            sl, vt, run = run_of(W, fields, offset, n)
            depart, pace, key, tau = timing(n, fields, B, 11 * n + B)
            ctx.fleet_paths(sl, vt)
            ctx.fleet_traffic(sl, vt)
            fs, ts, c = ctx.fleet_stats(), ctx.traffic_stats(), ctx.traffic_download()
            want = check_timed(ctx, W, fields, sl, vt, (offset, B, n), state, run, depart=depart, pace=pace, key=key, windows=B, tau=tau, free_count=n % 3)
            if n >= 64:
                assert 5 * want["contributing"] >= 2 * n, (n, want["contributing"])                  # at least 40 % contribute
                assert want["adds"] > 0 and want["beyond_horizon"] > 0, (n, want)
            if n in CONTRIBUTORS[offset]:
                assert want["contributing"] == CONTRIBUTORS[offset][n], (n, want["contributing"])
            # a horizon that holds everything: the windows sum to the counts of mnav_fleet_traffic
            wide = check_timed(ctx, W, fields, sl, vt, (offset, B, n, "wide"), state, run, depart=depart, pace=pace, key=key, windows=B, tau=2.0 * top / B)
            assert wide["beyond_horizon"] == 0 and np.array_equal(state.cell.astype(np.uint64).sum(axis=1), c), (offset, B, n)
            assert ctx.fleet_stats() == fs and ctx.traffic_stats() == ts and np.array_equal(ctx.traffic_download(), c), (offset, B, n)
    finally:
        ctx.close()


def test_hot_spot(world):
    """3000 robots of one plan: every contributor's last visit lands on the seed -- the same-address case of both atomics;
    then two seeds in one wave, one robot, and a robot on the seed"""
    W = world
    ctx = make_ctx(W)
    try:
        ctx.plan_dijkstra_batch(W.seeds, W.targets, FAR, LIMIT)
        fields = W.fields(offset=FAR)
        vt = np.random.default_rng(3).integers(0, W.V, 3000).astype(np.uint32)
        sl = np.zeros(3000, np.uint32)
        top = largest_potential(fields[:1])
        key = np.random.default_rng(4).permutation(3000).astype(np.uint32) + 7
        state = XM.Cells(W.V)
        for B, tau in ((1, 3e38), (64, top / 60), (3, top)):                  # one window: every robot in the seed's one cell
            want = check_timed(ctx, W, fields, sl, vt, ("hot spot", B), state, key=key, windows=B, tau=tau, free_count=1)
            seed = fields[0].seed
            assert want["contributing"] == 2946 == int(state.cell[seed].astype(np.uint64).sum()) and want["beyond_horizon"] == 0, want
            assert int(state.holder[seed].min()) == int(key[want["codes"] == FM.SUCCESS].min())
            if B == 1:
                assert want["largest_cell"] == 2946 and want["yielding"] == 2945                      # everybody but the smallest key
        sl[1::2] = 1
        check_timed(ctx, W, fields, sl[:200], vt[:200], "two seeds", state, windows=64, tau=top / 60)
        one = check_timed(ctx, W, fields, sl[:1], np.array([fields[0].target], np.uint32), "one robot", state, windows=64, tau=top / 60)
        assert one["contributing"] == 1 and one["adds"] > 1 and one["yielding"] == 0
        on_seed = check_timed(ctx, W, fields, sl[:1], np.array([fields[0].seed], np.uint32), "on the seed", state, depart=np.array([5.5 * top / 60], F), windows=64, tau=top / 60)
        assert on_seed["adds"] == 1 and state.cell[fields[0].seed, 5] == 1 and int(state.cell.astype(np.uint64).sum()) == 1
    finally:
        ctx.close()


def raw_timed(ctx, slots, vtx, weights=None, depart=None, pace=None, key=None, windows=64, tau=1.0, free_count=0, accumulate=False):
    """the C call with sentinel-filled outputs: (rc, outputs untouched)"""
    n = len(slots)
    sl, vt = (np.ascontiguousarray(a, np.uint32) for a in (slots, vtx))
    w, ky = (None if a is None else np.ascontiguousarray(a, np.uint32) for a in (weights, key))
    dp, pc = (None if a is None else np.ascontiguousarray(a, np.float32) for a in (depart, pace))
    ints = [np.full(n, SENTINEL, np.uint32) for _ in range(6)]
    pot, ft = np.full(n, np.nan, np.float32), np.full(n, np.nan, np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = ctx._L.mnav_fleet_timed_traffic(ctx._h, n, p(sl), p(vt), None, p(w), p(dp), p(pc), p(ky), int(windows), float(tau), int(free_count), 1 if accumulate else 0,
                                         p(ints[0]), p(ints[1]), p(pot), p(ints[2]), p(ints[3]), p(ints[4]), p(ints[5]), p(ft))
    return rc, all((a == SENTINEL).all() for a in ints) and np.isnan(pot).all() and np.isnan(ft).all()


def snapshot(ctx):
    d = ctx.timed_traffic_download()
    return d, ctx.timed_traffic_stats()


def same_snapshot(ctx, snap):
    d, st = snapshot(ctx)
    return st == snap[1] and all(np.array_equal(d[k], snap[0][k]) for k in ("peak", "window", "cells", "holders"))


def test_weights_accumulate_and_positions(world):
    W = world
    ctx = make_ctx(W)
    try:
        ctx.plan_dijkstra_batch(W.seeds, W.targets, OFFSET, LIMIT)
        fields = W.fields()
        n = 1000
        sl, vt, run = run_of(W, fields, OFFSET, n, 8)
        w = np.random.default_rng(12).integers(0, 6, n).astype(np.uint32)
        depart, pace, key, tau = timing(n, fields, 64, 21)
        kw = dict(windows=64, tau=tau, free_count=2)
        state = XM.Cells(W.V)
        whole = check_timed(ctx, W, fields, sl, vt, "weights", state, run, weights=w, depart=depart, pace=pace, key=key, **kw)
        d_whole = ctx.timed_traffic_download()
        assert whole["contributing"] > 300 and (w == 0).sum() > 100 and whole["total_weight"] > whole["contributing"] and whole["yielding"] > 0
        # two halves, the second on top of the first, equal the one call; the second half's report is the whole call's
        state = XM.Cells(W.V)
        a, b = slice(0, 437), slice(437, n)
        check_timed(ctx, W, fields, sl[a], vt[a], "first half", state, weights=w[a], depart=depart[a], pace=pace[a], key=key[a], **kw)
        second = check_timed(ctx, W, fields, sl[b], vt[b], "second half", state, weights=w[b], depart=depart[b], pace=pace[b], key=key[b], accumulate=True, **kw)
        d = ctx.timed_traffic_download()
        assert all(np.array_equal(d[k], d_whole[k]) for k in d) and second["total_weight"] == whole["total_weight"]
        assert np.array_equal(second["yield_hops"], whole["yield_hops"][b]) and np.array_equal(second["conflict_hops"], whole["conflict_hops"][b])
        # zero weights: classified, nothing added; n = 0 starts the cells over
        zero = check_timed(ctx, W, fields, sl, vt, "zero weights", state, run, weights=np.zeros(n, np.uint32), accumulate=True, **kw)
        assert zero["contributing"] == 0 and zero["adds"] == 0 and np.array_equal(ctx.timed_traffic_download()["cells"], d_whole["cells"])
        ctx.fleet_timed_traffic(np.zeros(0, np.uint32), np.zeros(0, np.uint32), **kw)
        d = ctx.timed_traffic_download()
        assert not d["cells"].any() and (d["holders"] == FM.NONE).all() and not d["peak"].any() and (d["window"] == FM.NONE).all()
        assert ctx.timed_traffic_stats()["total_weight"] == 0
        # positions: the cells of the located vertices
        rng = np.random.default_rng(3)
        m = 300
        slots = (np.arange(m) % 6).astype(np.uint32)
        v = rng.integers(0, W.V, m)
        pos = (W.mesh.xyz[v] + rng.uniform(-0.04, 0.04, (m, 3)).astype(np.float32) * np.array([1, 1, 0.2], np.float32)).astype(np.float32)
        nearest = np.array([W.om.nearest_vertex(q) for q in pos], np.uint32)
        assert ctx.locate_stats()["built"] == 0
        fs = ctx.fleet_stats()
        t = ctx.fleet_timed_traffic(slots, None, pos, depart=depart[:m], pace=pace[:m], key=key[:m], **kw)
        assert ctx.timed_traffic_stats()["built_index"] == 1 and ctx.locate_stats()["built"] == 1 and ctx.fleet_stats() == fs
        assert np.array_equal(t["vertex"], nearest)
        by_pos = ctx.timed_traffic_download()
        state = XM.Cells(W.V)
        want = check_timed(ctx, W, fields, slots, nearest, "by vertex", state, depart=depart[:m], pace=pace[:m], key=key[:m], **kw)
        assert ctx.timed_traffic_stats()["built_index"] == 0 and want["contributing"] > 100
        assert all(np.array_equal(by_pos[k], state_k) for k, state_k in (("cells", state.cell), ("holders", state.holder), ("peak", state.peak), ("window", state.window)))
        for k in OUTPUTS:
            if k != "vertex":
                assert np.array_equal(t[k], want[k]), k
    finally:
        ctx.close()


def test_refusals_touch_nothing(world):
    W = world
    ctx = make_ctx(W)
    try:
        one = np.zeros(1, np.uint32)
        rc, clean = raw_timed(ctx, one, W.targets[:1])                       # no plan yet
        assert rc == -1 and clean and ctx.timed_traffic_stats()["windows"] == 0
        ctx.plan_dijkstra_batch(W.seeds, W.targets, OFFSET, LIMIT)
        fields = W.fields()
        n = 300
        sl, vt, run = run_of(W, fields, OFFSET, n, 8)
        depart, pace, key, tau = timing(n, fields, 64, 2)
        state = XM.Cells(W.V)
        check_timed(ctx, W, fields, sl, vt, "start", state, run, depart=depart, pace=pace, key=key, windows=64, tau=tau, free_count=1)
        snap = snapshot(ctx)
        assert snap[1]["total_weight"] > 100

        def refused(what, **kw):
            args = dict(depart=depart, pace=pace, key=key, windows=64, tau=tau)
            args.update(kw)
            slots, vtx = args.pop("slots", sl), args.pop("vtx", vt)
            for acc in (False, True) if "accumulate" not in kw else (kw["accumulate"],):
                args["accumulate"] = acc
                rc, clean = raw_timed(ctx, slots, vtx, **args)
                assert rc == -1 and clean and what in ctx._err() and same_snapshot(ctx, snap), (kw.keys(), acc, rc, ctx._err())

        def bad(like, at, value):
            a = like.copy()
            a[at] = value
            return a
        for B in (0, 1025, 2 ** 31):
            refused("windows out of range", windows=B)
        for t in (0.0, -1.0, np.nan, np.inf, 1e-50, 1e39):
            refused("tau must be finite and positive", tau=t)
        for x in (np.nan, -1.0, np.inf):
            refused("departure time", depart=bad(depart, n - 1, x))
        for x in (0.0, -1.0, np.nan, np.inf):
            refused("pace", pace=bad(pace, 0, x))
        for kw in (dict(windows=63), dict(windows=1), dict(tau=2 * tau), dict(tau=float(np.nextafter(F(tau), F(0))))):
            refused("differ from the cells' configuration", accumulate=True, **kw)
        two = np.array([2 ** 31, 2 ** 31], np.uint32)
        sl2, vt2 = np.zeros(2, np.uint32), np.array([fields[0].seed, fields[0].target], np.uint32)
        refused("total weight does not fit the counters", slots=sl2, vtx=vt2, weights=two, depart=None, pace=None, key=None)
        refused("total weight does not fit the counters", slots=sl2[:1], vtx=vt2[:1], weights=np.array([2 ** 32 - 1], np.uint32), depart=None, pace=None, key=None,
                accumulate=True)
        refused("slot out of range", slots=np.array([8], np.uint32), vtx=vt2[:1], depart=None, pace=None, key=None)
        ctx.set_option("timed_traffic_max_mb", 0)                              # the memory cap
        refused("timed_traffic_max_mb")
        ctx.set_option("timed_traffic_max_mb", 8.0 * W.V * 64 / 1048576.0)    # exactly the cells and holders of 64 windows
        refused("timed_traffic_max_mb", windows=65, accumulate=False)
        check_timed(ctx, W, fields, sl, vt, "at the cap", state, run, depart=depart, pace=pace, key=key, windows=64, tau=tau, free_count=1, accumulate=True)
        ctx.set_option("timed_traffic_max_mb", None)
        # another configuration without accumulate reallocates
        check_timed(ctx, W, fields, sl, vt, "new windows", state, run, depart=depart, pace=pace, key=key, windows=7, tau=3 * tau)
        big = ctx.fleet_timed_traffic(sl2[:1], vt2[:1], weights=np.array([2 ** 32 - 1], np.uint32), windows=2, tau=1.0)
        d, st = snapshot(ctx)
        assert big["codes"][0] == FM.SUCCESS and int(d["cells"][fields[0].seed, 0]) == 2 ** 32 - 1 == st["largest_cell"] == st["total_weight"] == int(d["peak"][fields[0].seed])
    finally:
        ctx.close()


def test_stale_fields_are_refused_until_the_replan(world):
    W = world
    ctx = make_ctx(W)
    old = W.costs
    try:
        seeds, targets = W.seeds[:6], W.targets[:6].copy()
        ctx.plan_dijkstra_batch(seeds, targets, OFFSET, LIMIT)
        fields = W.fields(targets)[:6]
        sl, vt = robots(W, fields, 400, 33)
        depart, pace, key, tau = timing(400, fields, 16, 3)
        kw = dict(depart=depart, pace=pace, key=key, windows=16, tau=tau, free_count=1)
        state = XM.Cells(W.V)
        check_timed(ctx, W, fields, sl, vt, "before", state, **kw)
        snap = snapshot(ctx)
        ids = np.array([W.mesh.vertex_at(0.5, 0.5), W.mesh.vertex_at(0.52, 0.5), int(targets[0])], np.uint32)
        ids = ids[~np.isin(ids, seeds)]
        W.change_costs(ctx, ids, 0.45)
        for acc in (False, True):
            rc, clean = raw_timed(ctx, sl, vt, accumulate=acc, **kw)
            assert rc == -1 and clean and "costs changed" in ctx._err() and same_snapshot(ctx, snap), (acc, ctx._err())
        ctx.replan_dijkstra_each(None, OFFSET, want_pred=True)
        fields = W.fields(targets)[:6]
        want = check_timed(ctx, W, fields, sl, vt, "after the replan", state, **kw)
        assert want["contributing"] > 100
    finally:
        ctx.close()
        if W.costs is not old:
            W.costs = old
            W.weights = W.om.edge_weights(W.case.edge_dist, W.costs, 1.0)
            W.version += 1


def test_the_layer(world):
    """layer_timed_traffic: the traffic cost rule on the peaks, and its change list"""
    W = world
    ctx = make_ctx(W)
    try:
        with pytest.raises(RuntimeError):
            ctx.layer_timed_traffic(64)
        for bad in (dict(gain=-1.0), dict(gain=np.inf), dict(gain=np.nan), dict(cap=-0.5), dict(cap=np.nan)):
            with pytest.raises(RuntimeError):
                ctx.layer_timed_traffic(3, **bad)
        first = ctx.layer_timed_traffic(3, 0, 1.0, np.inf)                    # no cells yet: zero costs, a fresh slot lists every vertex
        assert np.array_equal(first["changed"], np.arange(W.V)) and not ctx.layer_download(3)[0].any()
        ctx.plan_dijkstra_batch(W.seeds, W.targets, FAR, LIMIT)
        fields = W.fields(offset=FAR)
        state = XM.Cells(W.V)
        sl, vt, run = run_of(W, fields, FAR, 3000)
        depart, pace, key, tau = timing(3000, fields, 64, 6)
        check_timed(ctx, W, fields, sl, vt, "layer", state, run, depart=depart, pace=pace, key=key, windows=64, tau=tau)
        peak = state.peak
        assert peak.max() > 8
        old_cost, old_lethal = ctx.layer_download(3)
        for free_count, gain, cap in ((0, 1.0, np.inf), (2, 0.125, 1.0), (2, 0.125, 1.0), (3, 0.3, 4 * np.float32(0.3)), (400, 1.0, 9.0), (1, 0.0, 3.0)):
            got = ctx.layer_timed_traffic(3, free_count, gain, cap)
            want = TM.cost(peak, free_count, gain, cap)
            cost, lethal = ctx.layer_download(3)
            assert np.array_equal(bits(cost), bits(want)) and not lethal.any(), (free_count, gain, cap)
            assert np.array_equal(got["changed"], TM.changed(old_cost, old_lethal, want, False)), (free_count, gain, cap, got["changed"].size)
            print("timed layer", free_count, gain, cap, "changed", got["changed"].size, "max", float(want.max()))
            old_cost, old_lethal = cost, lethal
        # a slot that held lethal flags and another layer's costs: the flags go, and every difference is listed
        other = np.random.default_rng(1).random(W.V).astype(np.float32)
        other[::3] = TM.cost(peak, 2, 0.125, 1.0)[::3]
        flags = (np.arange(W.V) % 7 == 0).astype(np.uint8)
        ctx.layer_upload(4, other, flags)
        got = ctx.layer_timed_traffic(4, 2, 0.125, 1.0)
        want = TM.cost(peak, 2, 0.125, 1.0)
        cost, lethal = ctx.layer_download(4)
        assert np.array_equal(bits(cost), bits(want)) and not lethal.any()
        assert np.array_equal(got["changed"], TM.changed(other, flags, want, False)) and W.V // 2 < got["changed"].size < W.V
        # the untimed layer of the same context still reads the untimed counts (none here)
        ctx.layer_traffic(5, 0, 1.0, np.inf)
        assert not ctx.layer_download(5)[0].any()
    finally:
        ctx.close()


def start_graph(W):
    """a static cost layer and the timed traffic layer under a COMBINE_AVG, edge_cost_factor 1; the model of the same graph"""
    ctx = capi.MnavContext(0)
    ctx.upload_mesh(W.mesh.xyz, W.mesh.faces, W.mesh.edges, W.case.vn)
    ctx.set_resident_outputs(True)
    ctx.layer_upload(0, W.costs)
    ctx.layer_timed_traffic(1)                                                # no cells: zero costs
    ctx.map_configure(NODES, 2, 1.0, W.invalid)
    ctx.map_compute()
    model = MM.MapModel(W.om, W.case.edge_dist, NODES, 2, 1.0, W.invalid)
    model.set_input(0, W.costs)
    model.set_input(1, np.zeros(W.V, np.float32))
    model.compute()
    return ctx, model


def test_map_timed_traffic_and_one_closed_round(world):
    """plan -> fleet_timed_traffic -> map_timed_traffic -> (stale: refused) -> replan_dijkstra_each: the graph's state is the
    model's after the update and every plan ends on the oracle's fresh plan on the downloaded costs"""
    W = world
    ctx, model = start_graph(W)
    try:
        vc, w = same_map(ctx, model, "compute")
        seeds, targets = W.seeds[:6], W.targets[:6]
        limit = 1.0                                                          # (COMBINE_AVG with weights 1, 1 adds the layers: a seed's static cost <= 0.8 plus the cap stays below it)
        ctx.plan_dijkstra_batch(seeds, targets, FAR, limit, want_fields=True)
        fields, plans = oracle_fields(W, vc, w, seeds, targets, FAR, limit)
        n = 3000
        sl, vt = (np.arange(n) % 6).astype(np.uint32), np.random.default_rng(41).integers(0, W.V, n).astype(np.uint32)
        depart, pace, key, _ = timing(n, fields, 64, 8)
        tau = 1.5 * largest_potential(fields) / 64
        state = XM.Cells(W.V)
        want = check_timed(ctx, W, fields, sl, vt, "graph", state, depart=depart, pace=pace, key=key, windows=64, tau=tau, free_count=3)
        assert want["contributing"] > 2000 and want["over_cells"] > 0
        with pytest.raises(RuntimeError):
            ctx.map_timed_traffic(1, 0, -1.0, 1.0)                          # an argument error leaves the graph usable
        with pytest.raises(RuntimeError):
            ctx.map_timed_traffic(2, 0, 1.0, 1.0)                           # a derived node
        same_map(ctx, model, "after the refusals")
        vc0 = vc
        new = TM.cost(state.peak, 3, 0.01, 0.15)
        ids = TM.changed(model.cost[1], model.lethal[1], new, False)
        D = model.update_layer(1, ids, new[ids])
        got = ctx.map_timed_traffic(1, 3, 0.01, 0.15)
        vc, w = same_map(ctx, model, "map_timed_traffic")
        assert np.array_equal(got["changed"], D) and D.size > 0, (got["changed"].size, D.size)
        assert np.array_equal(got["changed"], np.flatnonzero(bits(vc0) != bits(vc)))                  # D: the host diff of the vertex costs
        assert got["stats"]["default_changed"] == D.size and got["stats"]["waves"] == 0
        with pytest.raises(RuntimeError, match="costs changed"):
            ctx.fleet_timed_traffic(sl[:4], vt[:4], windows=64, tau=tau, accumulate=True)
        same_cells(ctx, state, "after the stale refusal")
        b = ctx.replan_dijkstra_each(None, FAR, want_dist=True, want_pred=True)
        fields, plans = oracle_fields(W, vc, w, seeds, targets, FAR, limit)
        for k, r in enumerate(plans):
            assert b["codes"][k] == r.code and np.array_equal(b["pred"][k], r.pred) and np.array_equal(bits(b["dist"][k]), bits(r.dist)), ("end", k)
            assert np.array_equal(b["paths"][k], r.path), ("end", k)
        check_timed(ctx, W, fields, sl, vt, "second count", state, depart=depart, pace=pace, key=key, windows=64, tau=tau, free_count=3)
    finally:
        ctx.close()


def test_stagger_loop(world):
    """the rounds of tests/test_timed_traffic_model.py::test_stagger_loop on the device: every round equals the model and the committed figures"""
    W = world
    ctx = make_ctx(W)
    try:
        ctx.plan_dijkstra_batch(W.seeds, W.targets, FAR, LIMIT)
        fields = W.fields(offset=FAR)
        vt = np.random.default_rng(3).integers(0, W.V, STAGGER_ROBOTS).astype(np.uint32)
        sl = np.zeros(STAGGER_ROBOTS, np.uint32)
        tau = float(F(largest_potential(fields[:1]) / 48))
        run = FM.run(fields, W.V, sl, vt)
        state = XM.Cells(W.V)
        seen = []

        def call(depart):
            want = check_timed(ctx, W, fields, sl, vt, ("stagger", len(seen)), state, run, depart=depart, windows=STAGGER_WINDOWS, tau=tau, free_count=STAGGER_FREE)
            seen.append((want["over_cells"], want["yielding"]))
            return want                                                       # (the device's yield_hops are the model's: checked)
        for _ in stagger(call, tau):
            pass
        assert tuple(seen) == STAGGER and seen[-1][1] < seen[0][1], seen
    finally:
        ctx.close()
