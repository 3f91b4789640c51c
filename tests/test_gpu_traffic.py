"""GPU: fleet traffic (mnav_fleet_traffic, mnav_traffic_download, mnav_traffic_stats, mnav_layer_traffic,
mnav_map_traffic).  Every comparison is exact: counts are integers, costs are compared by bits.

The counts equal tests/traffic_model.py (which tests/test_traffic_model.py pins on the CPU) AND the histogram of one
mnav_fleet_paths call over the same robots in the same context; codes, vertices and potentials are that call's bits and
mnav_fleet_stats keeps its values.  The layer equals the model's cost rule, the graph update equals tests/map_model.py fed
with the model's traffic costs, and two rounds of plan -> traffic -> map update -> replan end on the oracle's fresh plans.

Shapes: the world of tests/test_gpu_fleet.py -- terrain(48) = 2304 vertices, 8 plans of which one has seed == target and
one a target out of range -- and up to 3000 robots."""
import ctypes as C

import numpy as np
import pytest

from mesh_navigation_amd import capi
from tests import fleet_model as FM
from tests import map_model as MM
from tests import traffic_model as TM
from tests.fleet_model import bits
from tests.test_gpu_fleet import LIMIT, OFFSET, World, make_ctx, robots

pytestmark = pytest.mark.gpu
SENTINEL = 0xDEADBEEF
FAR = 1e9                                                                    # an offset beyond every field: the waves run out
SIZES = (1, 63, 64, 65, 255, 256, 257, 3000)
# tests/traffic_model.py on this world with robots(W, fields, n, 5): contributors per n, and the outcomes at n = 3000
CONTRIBUTORS = {OFFSET: {64: 31, 257: 109, 3000: 1529}, FAR: {64: 36, 257: 162, 3000: 2188}}


@pytest.fixture(scope="module")
def world():
    return World()


def check_traffic(ctx, W, fields, slots, vtx, where, weights=None, accumulate=False, state=None):
    """fleet_paths, then fleet_traffic over the same robots: outputs, fleet_stats, counts and statistics; returns the model's dict"""
    state = TM.Counts(W.V) if state is None else state
    p = ctx.fleet_paths(slots, vtx)
    fs = ctx.fleet_stats()
    t = ctx.fleet_traffic(slots, vtx, weights=weights, accumulate=accumulate)
    assert ctx.fleet_stats() == fs, where                                   # no statistic of another entry point moves
    for k in ("codes", "vertex"):
        assert np.array_equal(t[k], p[k]), (where, k)
    assert np.array_equal(bits(t["potential"]), bits(p["potential"])), where
    want = TM.traffic(state, fields, slots, vtx, weights, accumulate)
    assert np.array_equal(t["codes"], want["codes"]) and np.array_equal(bits(t["potential"]), bits(want["potential"])), where
    c = ctx.traffic_download()
    assert c.dtype == np.uint32 and np.array_equal(c, state.c), (where, np.flatnonzero(c != state.c)[:8])
    if weights is None and not accumulate:
        # the histogram of the downloaded paths: only contributors have ids (a served robot of a seed == target plan has none)
        on = TM.contributes(p["codes"], p["potential"])
        hist = np.bincount(p["ids"], minlength=W.V) + np.bincount(np.asarray(vtx)[on], minlength=W.V)
        assert np.array_equal(c, hist.astype(np.uint32)), where
        assert int(c.astype(np.uint64).sum()) == p["total"] + int(on.sum()) == want["adds"], where
    st = ctx.traffic_stats()
    print(where, "n", len(slots), {k: st[k] for k in st if not k.startswith("ms")}, "ms kernels %.3f total %.3f" % (st["ms_kernels"], st["ms_total"]))
    assert {k: st[k] for k in ("contributing", "adds", "total_weight", "occupied", "peak")} == {k: want[k] for k in ("contributing", "adds", "total_weight", "occupied", "peak")}, (where, st, want)
    return want


@pytest.mark.parametrize("offset", [OFFSET, FAR], ids=["offset_0.3", "offset_far"])
def test_counts_equal_the_model_and_the_histogram_of_fleet_paths(world, offset):
    W = world
    ctx = make_ctx(W)
    try:
        assert not ctx.traffic_download().any() and ctx.traffic_stats()["total_weight"] == 0      # zero after upload_mesh
        ctx.plan_dijkstra_batch(W.seeds, W.targets, offset, LIMIT)
        assert "k_plan_async" in ctx.last_engine(), ctx.last_engine()
        fields = W.fields(offset=offset)
        seen = {}
        for n in SIZES:
            sl, vt = robots(W, fields, n, 5)
            want = check_traffic(ctx, W, fields, sl, vt, (offset, n))
            if n >= 64:
                assert 5 * want["contributing"] >= 2 * n, (n, want["contributing"])              # at least 40 % contribute
            if n in CONTRIBUTORS[offset]:
                assert want["contributing"] == CONTRIBUTORS[offset][n], (n, want["contributing"])
            for c in want["codes"]:
                seen[int(c)] = seen.get(int(c), 0) + (n == 3000)
        if offset == OFFSET:
            assert seen[FM.BEYOND_FIELD] == 723 and seen[FM.INVALID_GOAL] == 382, seen
        else:
            assert seen[FM.NO_PATH_FOUND] == 58 and FM.BEYOND_FIELD not in seen, seen
    finally:
        ctx.close()


def test_hot_spot(world):
    """3000 robots of one plan: every contributor's last add lands on the seed -- the same-address case of every aggregation
    path, with one add per wave and with one add per lane"""
    W = world
    ctx = make_ctx(W)
    try:
        ctx.plan_dijkstra_batch(W.seeds, W.targets, FAR, LIMIT)
        fields = W.fields(offset=FAR)
        vt = np.random.default_rng(3).integers(0, W.V, 3000).astype(np.uint32)
        sl = np.zeros(3000, np.uint32)
        for combine in (None, 0, 1):
            ctx.set_option("traffic_combine", combine)
            want = check_traffic(ctx, W, fields, sl, vt, ("hot spot", combine))
            c = ctx.traffic_download()
            assert want["contributing"] == 2946 == int(c[fields[0].seed]) == want["peak"] and want["occupied"] == 1998, want
        # a wave whose contributors end on two seeds, and a single contributor
        sl[1::2] = 1
        check_traffic(ctx, W, fields, sl[:200], vt[:200], "two seeds")
        check_traffic(ctx, W, fields, sl[:1], np.array([fields[0].target], np.uint32), "one robot")
    finally:
        ctx.close()


def raw_traffic(ctx, slots, vtx, weights, accumulate):
    """the C call with sentinel-filled outputs: (rc, outputs untouched)"""
    n = len(slots)
    sl, vt, w = (np.ascontiguousarray(a, np.uint32) for a in (slots, vtx, weights))
    code, vout, pot = np.full(n, SENTINEL, np.uint32), np.full(n, SENTINEL, np.uint32), np.full(n, np.nan, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = ctx._L.mnav_fleet_traffic(ctx._h, n, p(sl), p(vt), None, p(w), 1 if accumulate else 0, p(code), p(vout), p(pot))
    return rc, (code == SENTINEL).all() and (vout == SENTINEL).all() and np.isnan(pot).all()


def test_weights_refusals_and_positions(world):
    W = world
    ctx = make_ctx(W)
    try:
        with pytest.raises(RuntimeError):
            ctx.fleet_traffic(np.zeros(1, np.uint32), W.targets[:1])        # no plan yet
        ctx.plan_dijkstra_batch(W.seeds, W.targets, OFFSET, LIMIT)
        fields = W.fields()
        n = 1000
        sl, vt = robots(W, fields, n, 8)
        w = np.random.default_rng(12).integers(0, 6, n).astype(np.uint32)
        whole = check_traffic(ctx, W, fields, sl, vt, "weights", weights=w)
        c_whole = ctx.traffic_download()
        assert whole["contributing"] > 300 and (w == 0).sum() > 100 and whole["total_weight"] > whole["contributing"]
        # two halves, the second on top of the first, equal the one call
        state = TM.Counts(W.V)
        check_traffic(ctx, W, fields, sl[:437], vt[:437], "first half", weights=w[:437], state=state)
        halves = check_traffic(ctx, W, fields, sl[437:], vt[437:], "second half", weights=w[437:], accumulate=True, state=state)
        assert np.array_equal(ctx.traffic_download(), c_whole) and halves["total_weight"] == whole["total_weight"]
        # zero weights: classified, nothing added; n = 0 starts the counts over
        zero = check_traffic(ctx, W, fields, sl, vt, "zero weights", weights=np.zeros(n, np.uint32), accumulate=True, state=state)
        assert zero["contributing"] == 0 and zero["adds"] == 0 and np.array_equal(ctx.traffic_download(), c_whole)
        # the weights that do not fit: refused, and nothing is touched
        st0 = ctx.traffic_stats()
        two = np.array([2 ** 31, 2 ** 31], np.uint32)
        sl2, vt2 = np.zeros(2, np.uint32), np.array([fields[0].seed, fields[0].target], np.uint32)
        for acc in (False, True):
            rc, untouched = raw_traffic(ctx, sl2, vt2, two, acc)
            assert rc == -1 and untouched and "total weight does not fit the counters" in ctx._err(), (acc, rc, ctx._err())
            assert np.array_equal(ctx.traffic_download(), c_whole) and ctx.traffic_stats() == st0
        rc, untouched = raw_traffic(ctx, sl2[:1], vt2[:1], np.array([2 ** 32 - 1], np.uint32), True)      # fits alone, not on top of T
        assert rc == -1 and untouched and np.array_equal(ctx.traffic_download(), c_whole) and ctx.traffic_stats() == st0
        rc, untouched = raw_traffic(ctx, np.array([8], np.uint32), vt2[:1], np.ones(1, np.uint32), False)  # a slot that is no plan
        assert rc == -1 and untouched and np.array_equal(ctx.traffic_download(), c_whole) and ctx.traffic_stats() == st0
        big = ctx.fleet_traffic(sl2[:1], vt2[:1], weights=np.array([2 ** 32 - 1], np.uint32))
        assert big["codes"][0] == FM.SUCCESS and int(ctx.traffic_download()[fields[0].seed]) == 2 ** 32 - 1 == ctx.traffic_stats()["peak"] == ctx.traffic_stats()["total_weight"]
        ctx.fleet_traffic(np.zeros(0, np.uint32), np.zeros(0, np.uint32))
        assert not ctx.traffic_download().any() and ctx.traffic_stats()["total_weight"] == 0
        # positions: the counts of the located vertices
        rng = np.random.default_rng(3)
        m = 300
        slots = (np.arange(m) % 6).astype(np.uint32)
        v = rng.integers(0, W.V, m)
        pos = (W.mesh.xyz[v] + rng.uniform(-0.04, 0.04, (m, 3)).astype(np.float32) * np.array([1, 1, 0.2], np.float32)).astype(np.float32)
        nearest = np.array([W.om.nearest_vertex(q) for q in pos], np.uint32)
        assert ctx.locate_stats()["built"] == 0
        fs = ctx.fleet_stats()
        t = ctx.fleet_traffic(slots, None, pos)
        assert ctx.traffic_stats()["built_index"] == 1 and ctx.locate_stats()["built"] == 1 and ctx.fleet_stats() == fs
        assert np.array_equal(t["vertex"], nearest)
        state = TM.Counts(W.V)
        want = TM.traffic(state, fields, slots, nearest)
        assert np.array_equal(ctx.traffic_download(), state.c) and want["contributing"] > 100 and np.array_equal(t["codes"], want["codes"])
        ctx.fleet_traffic(slots, None, pos, accumulate=True)
        assert ctx.traffic_stats()["built_index"] == 0 and np.array_equal(ctx.traffic_download(), 2 * state.c)
        # a cost-changing call makes the fields stale: refused like mnav_fleet_paths, counts untouched
        ctx.update_costs(np.array([W.targets[0]], np.uint32), np.array([W.costs[int(W.targets[0])]], np.float32))
        rc, untouched = raw_traffic(ctx, sl2, vt2, np.ones(2, np.uint32), False)
        assert rc == -1 and untouched and "costs changed" in ctx._err() and np.array_equal(ctx.traffic_download(), 2 * state.c)
    finally:
        ctx.close()


def many_plans(W, n):
    """n plans on the world's map (seeds and targets among the traversable vertices) with the oracle's fields"""
    rng = np.random.default_rng(31)
    ok = np.flatnonzero((W.costs <= LIMIT) & (W.invalid == 0))
    pick = rng.choice(ok, 2 * n, replace=False).astype(np.uint32)
    seeds, targets = pick[:n], pick[n:]
    fields = []
    for s, g in zip(seeds, targets):
        r = W.fresh(s, g, OFFSET)
        fields.append(FM.Field(r.dist, r.pred, int(s), int(g), OFFSET))
    return seeds, targets, fields


@pytest.mark.parametrize("source", ["async", "tiled", "tile_batch_170", "replan_each"])
def test_fields_of_every_engine_that_leaves_predecessors(world, source):
    W = world
    ctx = make_ctx(W)
    old = W.costs
    try:
        if source == "tile_batch_170":
            seeds, targets, fields = many_plans(W, 170)
            ctx.set_dijkstra_engine("tile_batch")
            assert ctx.plan_dijkstra_batch(seeds, targets, OFFSET, LIMIT)["rc"] == 0 and "k_tb" in ctx.last_engine(), ctx.last_engine()
        elif source == "replan_each":
            seeds, targets = W.seeds[:6], W.targets[:6].copy()
            ctx.plan_dijkstra_batch(seeds, targets, OFFSET, LIMIT)
            ids = np.array([W.mesh.vertex_at(0.5, 0.5), W.mesh.vertex_at(0.52, 0.5), int(targets[0])], np.uint32)
            ids = ids[~np.isin(ids, seeds)]
            W.change_costs(ctx, ids, 0.45)
            with pytest.raises(RuntimeError):
                ctx.fleet_traffic(np.zeros(1, np.uint32), targets[:1])      # stale until the replan
            b = ctx.replan_dijkstra_each(None, OFFSET, want_pred=True)
            print("replan each", {k: v for k, v in b["each"].items() if k not in ("levels", "classes")})
            fields = W.fields(targets)[:6]
            assert all(np.array_equal(b["pred"][k], fields[k].pred) for k in range(6))
        else:
            if source == "tiled":
                ctx.set_dijkstra_engine("tiled")
            ctx.plan_dijkstra_batch(W.seeds, W.targets, OFFSET, LIMIT)
            assert {"tiled": "k_tile_round", "async": "k_plan_async"}[source] in ctx.last_engine(), ctx.last_engine()
            fields = W.fields()
        for n in (max(65, len(fields) + 87), 3000):                          # (robots() wants room for one special robot per plan)
            sl, vt = robots(W, fields, n, 20 + n)
            want = check_traffic(ctx, W, fields, sl, vt, (source, n))
        assert want["contributing"] >= 1000 and want["peak"] >= 10, want
    finally:
        ctx.close()
        if W.costs is not old:
            W.costs = old
            W.weights = W.om.edge_weights(W.case.edge_dist, W.costs, 1.0)
            W.version += 1


def test_the_layer(world):
    """layer_traffic: costs and change list against a fresh slot and against a slot holding another count's layer"""
    W = world
    ctx = make_ctx(W)
    try:
        with pytest.raises(RuntimeError):
            ctx.layer_traffic(64)
        for bad in (dict(gain=-1.0), dict(gain=np.inf), dict(gain=np.nan), dict(cap=-0.5), dict(cap=np.nan)):
            with pytest.raises(RuntimeError):
                ctx.layer_traffic(3, **bad)
        first = ctx.layer_traffic(3, 0, 1.0, np.inf)                          # no counts yet: zero costs, a fresh slot lists every vertex
        assert np.array_equal(first["changed"], np.arange(W.V)) and not ctx.layer_download(3)[0].any()
        ctx.plan_dijkstra_batch(W.seeds, W.targets, FAR, LIMIT)
        fields = W.fields(offset=FAR)
        state = TM.Counts(W.V)
        sl, vt = robots(W, fields, 3000, 5)
        ctx.fleet_traffic(sl, vt)
        TM.traffic(state, fields, sl, vt)
        old_cost, old_lethal = ctx.layer_download(3)
        for free_count, gain, cap in ((0, 1.0, np.inf), (2, 0.125, 1.0), (2, 0.125, 1.0), (5, 0.3, 40 * np.float32(0.3)), (400, 1.0, 9.0), (1, 0.0, 3.0)):
            got = ctx.layer_traffic(3, free_count, gain, cap)
            want = TM.cost(state.c, free_count, gain, cap)
            cost, lethal = ctx.layer_download(3)
            assert np.array_equal(bits(cost), bits(want)) and not lethal.any(), (free_count, gain, cap)
            assert np.array_equal(got["changed"], TM.changed(old_cost, old_lethal, want, False)), (free_count, gain, cap, got["changed"].size)
            print("layer", free_count, gain, cap, "changed", got["changed"].size, "max", float(want.max()), "at the cap", int((want == np.float32(cap)).sum()))
            old_cost, old_lethal = cost, lethal
        # a slot that held lethal flags and another layer's costs: the flags go, and every difference is listed
        other = np.random.default_rng(1).random(W.V).astype(np.float32)
        other[::3] = TM.cost(state.c, 2, 0.125, 1.0)[::3]
        flags = (np.arange(W.V) % 7 == 0).astype(np.uint8)
        ctx.layer_upload(4, other, flags)
        got = ctx.layer_traffic(4, 2, 0.125, 1.0)
        want = TM.cost(state.c, 2, 0.125, 1.0)
        cost, lethal = ctx.layer_download(4)
        assert np.array_equal(bits(cost), bits(want)) and not lethal.any()
        assert np.array_equal(got["changed"], TM.changed(other, flags, want, False)) and W.V // 2 < got["changed"].size < W.V
        # a second count's layer over the first one's
        sl, vt = robots(W, fields, 700, 6)
        ctx.fleet_traffic(sl, vt)
        TM.traffic(state, fields, sl, vt)
        got = ctx.layer_traffic(4, 2, 0.125, 1.0)
        new = TM.cost(state.c, 2, 0.125, 1.0)
        assert np.array_equal(bits(ctx.layer_download(4)[0]), bits(new)) and np.array_equal(got["changed"], TM.changed(want, lethal, new, False))
        assert 0 < got["changed"].size < W.V
    finally:
        ctx.close()


NODES = [dict(layer=0, kind="input"), dict(layer=1, kind="input"), dict(layer=2, kind="avg", inputs=[0, 1], weights=[1.0, 1.0])]


def start_graph(W):
    """a static cost layer and the traffic layer under a COMBINE_AVG, edge_cost_factor 1; the model of the same graph"""
    ctx = capi.MnavContext(0)
    ctx.upload_mesh(W.mesh.xyz, W.mesh.faces, W.mesh.edges, W.case.vn)
    ctx.set_resident_outputs(True)
    ctx.layer_upload(0, W.costs)
    ctx.layer_traffic(1)                                                      # no counts: zero costs
    ctx.map_configure(NODES, 2, 1.0, W.invalid)
    ctx.map_compute()
    model = MM.MapModel(W.om, W.case.edge_dist, NODES, 2, 1.0, W.invalid)
    model.set_input(0, W.costs)
    model.set_input(1, np.zeros(W.V, np.float32))
    model.compute()
    return ctx, model


def same_map(ctx, model, where):
    for slot in (0, 1, 2):
        cost, lethal = ctx.layer_download(slot)
        assert np.array_equal(bits(cost), bits(model.cost[slot])) and np.array_equal(lethal != 0, model.lethal[slot] != 0), (where, slot)
    vc, w = ctx.download_costs()
    assert np.array_equal(bits(vc), bits(model.vertex_costs)) and np.array_equal(bits(w), bits(model.edge_weights)), where
    return vc, w


def map_traffic_step(ctx, model, state, free_count, gain, cap, where):
    """map_traffic on the device, update_layer with the model's traffic costs on the model: layers, costs, weights and D"""
    vc0, _ = ctx.download_costs()
    new = TM.cost(state.c, free_count, gain, cap)
    ids = TM.changed(model.cost[1], model.lethal[1], new, False)
    D = model.update_layer(1, ids, new[ids])
    got = ctx.map_traffic(1, free_count, gain, cap)
    vc, w = same_map(ctx, model, where)
    assert np.array_equal(got["changed"], D), (where, got["changed"].size, D.size)
    assert np.array_equal(got["changed"], np.flatnonzero(bits(vc0) != bits(vc))), where          # D: the host diff of the vertex costs
    assert got["stats"]["default_changed"] == D.size and got["stats"]["waves"] == 0
    print(where, "traffic layer changed", ids.size, "D", D.size, "edges reweighted", got["stats"]["edges_reweighted"])
    return vc, w


def oracle_fields(W, vc, w, seeds, targets, offset, limit):
    out, plans = [], []
    for s, g in zip(seeds, targets):
        r = W.om.dijkstra(w, vc, int(s), int(g), offset, limit, W.invalid)
        plans.append(r)
        out.append(FM.Field(r.dist, r.pred, int(s), int(g), offset))
    return out, plans


def test_map_traffic_and_the_closed_loop(world):
    """Two rounds of plan -> fleet_traffic -> map_traffic -> (fleet_paths refused as stale) -> replan_dijkstra_each: the
    graph's state is the model's after every update, every plan equals the oracle's fresh plan on the downloaded costs,
    and the counts of the second round are the model's on those fields."""
    W = world
    ctx, model = start_graph(W)
    try:
        vc, w = same_map(ctx, model, "compute")
        seeds, targets = W.seeds[:6], W.targets[:6]
        limit = 1.0                                                          # (COMBINE_AVG with weights 1, 1 adds the layers: a seed's static cost <= 0.8 plus the cap stays below it)
        b = ctx.plan_dijkstra_batch(seeds, targets, FAR, limit, want_fields=True)
        state = TM.Counts(W.V)
        rng = np.random.default_rng(41)
        n = 3000
        sl, vt = (np.arange(n) % 6).astype(np.uint32), rng.integers(0, W.V, n).astype(np.uint32)
        peaks = []
        for rnd in range(2):
            fields, plans = oracle_fields(W, vc, w, seeds, targets, FAR, limit)
            for k, r in enumerate(plans):                                    # every plan: the oracle's fresh plan on the downloaded costs
                assert b["codes"][k] == r.code and np.array_equal(b["pred"][k], r.pred) and np.array_equal(bits(b["dist"][k]), bits(r.dist)), (rnd, k)
                assert np.array_equal(b["paths"][k], r.path), (rnd, k)
            ctx.fleet_traffic(sl, vt)
            want = TM.traffic(state, fields, sl, vt)
            c = ctx.traffic_download()
            st = ctx.traffic_stats()
            assert np.array_equal(c, state.c) and int(c.astype(np.uint64).sum()) == want["adds"] == st["adds"] and st["peak"] == want["peak"], rnd
            assert want["contributing"] > 2000 and all(r.code == FM.SUCCESS for r in plans), rnd
            peaks.append(want["peak"])
            if rnd == 0:
                # an argument error leaves the graph usable and the slot as it was
                with pytest.raises(RuntimeError):
                    ctx.map_traffic(1, 0, -1.0, 1.0)
                with pytest.raises(RuntimeError):
                    ctx.map_traffic(2, 0, 1.0, 1.0)                          # a derived node
                same_map(ctx, model, "after the refusals")
            vc, w = map_traffic_step(ctx, model, state, 20, 0.004, 0.15, ("map_traffic", rnd))
            with pytest.raises(RuntimeError, match="costs changed"):
                ctx.fleet_paths(sl[:4], vt[:4])
            with pytest.raises(RuntimeError, match="costs changed"):
                ctx.fleet_traffic(sl[:4], vt[:4], accumulate=True)
            assert np.array_equal(ctx.traffic_download(), state.c)
            b = ctx.replan_dijkstra_each(None, FAR, want_dist=True, want_pred=True)
            print("round", rnd, "peak", want["peak"], "occupied", want["occupied"], "classes", list(b["each"]["classes"]) if b["each"]["classes"] is not None else None,
                  "whole fresh", b["each"]["whole_fresh"])
        fields, plans = oracle_fields(W, vc, w, seeds, targets, FAR, limit)
        for k, r in enumerate(plans):
            assert b["codes"][k] == r.code and np.array_equal(b["pred"][k], r.pred) and np.array_equal(bits(b["dist"][k]), bits(r.dist)), ("end", k)
            assert np.array_equal(b["paths"][k], r.path), ("end", k)
        p = ctx.fleet_paths(sl, vt)                                          # the replan made the fields the map's again
        assert np.array_equal(p["codes"], FM.run(fields, W.V, sl, vt)["codes"])
        print("peaks of the two rounds (reported, not asserted: spreading depends on the terrain)", peaks)
    finally:
        ctx.close()
