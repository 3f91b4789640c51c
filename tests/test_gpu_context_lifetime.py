"""GPU: ONE context across meshes that grow and shrink (mnav_upload_mesh keeps the context).

Every subsystem has its own tests, almost all of them in a fresh context on one mesh.  Here the four worlds of
tests/lifetime_world.py follow each other in one context, S -> L -> T -> H -> S under tile_size 64 and S -> L -> S with
tile_size 128 for L, and at every stop check_stop() runs the planners on every engine, the CVP batch on the wide kernel with
its back-tracking, every layer and a layer graph, the pose lookup, the follower and a rollout, every fleet call and the
three replans -- against the oracle and the numpy models each subsystem's own test uses, with those tests' own helpers.
The long-lived context must ALSO give, bit for bit, what a fresh context gives for the same mesh: that catches state that
leaks from one mesh into the next even where model and kernel agree.  A stale V-, F-, E- or tile-count-sized buffer is
silent on a smaller mesh and an out-of-bounds write on a larger one, so every quantity both grows and shrinks.

Then: what every reader of resident outputs answers between a new mesh and its next plan (refused, outputs untouched), in
both directions, and three batch sizes in a row on one mesh (200, 1, 65 plans): the robot-side calls see exactly the
plans of the last call.

Every comparison is exact (integers equal, floats by their bits); the follower and the rollout run under the
configuration and tolerances of tests/test_gpu_rollout.py.  The conditions on the inputs that keep a stop from passing
vacuously are lifetime_world.input_conditions(): computed from the models alone, asserted below."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from mesh_navigation_amd import capi
from tests import clearance_model as CM
from tests import dispatch_model as DM
from tests import fleet_model as FM
from tests import follow_model as FOL
from tests import lifetime_world as LW
from tests import locate_model as LM
from tests import map_model as MM
from tests import obstacle_model as OM
from tests import rollout_model as RM
from tests import timed_traffic_model as XM
from tests import traffic_model as TM
from tests.fleet_model import bits
from tests.lifetime_world import LIMIT, OFFSET, world
from tests.test_gpu_clearance_layer import check_layer, clearance_case
from tests.test_gpu_dispatch import QUANTUM, check_matrix, raw_assign, raw_costs
from tests.test_gpu_edge_cases import centroid, face_of
from tests.test_gpu_fleet import check_paths, check_walks, raw_paths, walk_robots
from tests.test_gpu_fleet_plans import check_plans, goal_positions
from tests.test_gpu_nbhd_layers import check as check_nbhd
from tests.test_gpu_obstacle_layer import check as check_obstacle
from tests.test_gpu_planners import assert_cvp_close, assert_dijkstra_equal
from tests.test_gpu_tile_batch import popped
from tests.test_gpu_timed_traffic import check_timed, raw_timed
from tests.test_gpu_traffic import check_traffic, raw_traffic
from tests.test_rollout_model import ANG_TOL, DIST_TOL, DT
from tests.test_timed_traffic_model import timing

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEF
ENGINES = [("tiled", None, "k_tile_round"), ("band", None, "k_step"), ("tile_batch", 0, "k_tb_solve_q"), ("tile_batch", 1, "k_tbv_solve"),
           ("async", None, "k_plan_async")]
GRAPH = [dict(layer=6, kind="avg", inputs=[1, 4], weights=[0.75, 0.5]), dict(layer=1, kind="inflation", inputs=[5], inflation_radius=0.3, inscribed_radius=0.15),
         dict(layer=5, kind="max", inputs=[0, 2]), dict(layer=0, kind="input"), dict(layer=2, kind="input"), dict(layer=4, kind="input")]   # graph (c) of tests/map_model.py
ROLLOUT_TICKS = 8
CVP_LIMIT = 1.0                                   # (under the worlds' cost limit of 0.8 hardly a face at a seed lets the CVP wave start)
ASSIGN_ROBOTS = 130                               # the auction's model takes seconds beyond that


def u(a):
    """an array as unsigned words: what `exact` means"""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def keep(out, key, *arrays):
    assert key not in out, key
    out[key] = [u(np.asarray(a)).copy() for a in arrays]


def same_outputs(a, b, where):
    """every exact output of two runs of check_stop, bit for bit"""
    assert list(a) == list(b), (where, [k for k in a if k not in b], [k for k in b if k not in a])
    for k in a:
        assert len(a[k]) == len(b[k]), (where, k)
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert x.shape == y.shape and np.array_equal(x, y), (where, k, i)


# -- the CPU side of a stop, computed once per world ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def vector_maps(W):
    """the oracle's vector map of every running plan (computeVectorMap on its predecessors)"""
    return [W.om.dijkstra_vector_map(W.fresh(W.seeds[k], W.targets[k]).pred) for k in W.running]


@functools.lru_cache(maxsize=None)
def cvp_plans(W):
    """a CVP plan per Dijkstra plan of the world: the wave starts at the centroid of a face at the seed vertex and runs to a
    face at the target vertex (an id out of range becomes a face out of range); with the oracle's result, and its walk back
    from the target face's centroid, for the plans whose faces exist"""
    m = W.mesh
    n = len(W.seeds)
    sp, tp = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    sf, tf = np.full(n, m.F + 1, np.uint32), np.full(n, m.F + 1, np.uint32)
    refs, walks, codes = [], [], []
    for k, (s, t) in enumerate(zip(W.seeds, W.targets)):
        if s < W.V:
            sf[k] = face_of(m, int(s))
            sp[k] = centroid(m, int(sf[k]))
        if t < W.V:
            tf[k] = face_of(m, int(t))
            tp[k] = centroid(m, int(tf[k]))
        if sf[k] < m.F and tf[k] < m.F:
            r = W.om.cvp(W.case.weights, W.costs0, W.case.vn, sp[k], int(sf[k]), int(tf[k]), OFFSET, CVP_LIMIT, W.invalid)
            refs.append(r)
            walks.append(W.om.cvp_backtrack(r.vecmap, r.has_vec, sp[k], int(sf[k]), tp[k], int(tf[k]), step_width=0.15) if r.code == 0 else None)
            codes.append(r.code)
        else:
            refs.append(None)
            walks.append(None)
            codes.append(capi.INVALID_START if sf[k] >= m.F else capi.INVALID_GOAL)
    return sp, sf, tp, tf, refs, walks, np.array(codes, np.uint32)


@functools.lru_cache(maxsize=None)
def locate_queries(W):
    pts = np.concatenate([LM.surface_points(W.mesh, 160, 31)[0],
                          W.mesh.xyz[np.random.default_rng(32).integers(0, W.V, 40)] + np.float32([0.013, -0.021, 0.04])]).astype(np.float32)
    return pts, LM.oracle_locate(W.om, pts)


@functools.lru_cache(maxsize=None)
def follower_wants(W):
    """one tick and ROLLOUT_TICKS ticks of the world's follower robots in the models, over the oracle's vector maps"""
    robots, goals = W.follow_robots
    cfg = FOL.config()
    fields = vector_maps(W)
    tick = FOL.tick_batch(W.follow_model, cfg, fields, robots)
    roll = RM.run(W.follow_model, cfg, dict(enumerate(fields)), robots, goals, DT, ROLLOUT_TICKS, DIST_TOL, ANG_TOL, trace_stride=1)
    return cfg, tick, roll


@functools.lru_cache(maxsize=None)
def auction_wants(W, vtx, plans):
    """the model's matrix, its auction and the exact optimum for the robots on `vtx` over the plans (seed, target) in order"""
    fields = [FM.Field(None, None, s, t, OFFSET, FM.plan_code(s, t, W.V)) if s == t or max(s, t) >= W.V else
              FM.Field(W.fresh(s, t).dist, W.fresh(s, t).pred, s, t, OFFSET) for s, t in plans]
    codes, pot = DM.matrix(fields, W.V, np.array(vtx, np.uint32))
    feasible = DM.feasible_of(codes, pot)
    q = DM.quantise(pot, feasible, QUANTUM)
    return pot, feasible, DM.auction(q, feasible), DM.exact(q, feasible)


@functools.lru_cache(maxsize=None)
def conditions(W):
    return LW.input_conditions(W)


def assert_conditions(W):
    """a stop that meets none of its branches passes vacuously: the counts of lifetime_world.input_conditions()"""
    c = conditions(W)
    print(W.name, "tile", W.tile_size, "input conditions", c)
    assert c["plans"] == W.n_plans and c["robots"] == W.n_robots and c["success"] >= 1 and c["rewound"] >= 1, c
    if W.name == "T":
        return c
    assert c["rejected"] >= 1 and 5 * c["contributing"] >= 2 * c["robots"] and c["beyond_field"] >= 1 and c["no_path"] >= 1, c
    assert min(c["over_cells"].values()) >= 1 and c["obstacle_lethal"] >= 1 and c["graph_changed"] >= 1, c
    return c


# -- the calls of a stop ------------------------------------------------------------------------------------------------
def dijkstra_calls(ctx, W, tag, out):
    fields, codes = W.fields(), W.plan_codes()
    maps = vector_maps(W)
    for engine, kernel, name in ENGINES:
        where = (tag, engine, kernel)
        ctx.set_dijkstra_engine(engine)
        ctx.set_option("tb_kernel", kernel)
        b = ctx.plan_dijkstra_batch(W.seeds, W.targets, OFFSET, LIMIT, want_fields=True)
        assert name in ctx.last_engine(), (where, ctx.last_engine())
        assert np.array_equal(b["codes"], codes), (where, b["codes"], codes)
        for k, f in enumerate(fields):
            if f.dist is None:
                assert len(b["paths"][k]) == 0 and not ctx.device_output(k, 0), (where, k)
                continue
            assert_dijkstra_equal(SimpleNamespace(code=int(b["codes"][k]), dist=b["dist"][k], pred=b["pred"][k], path=b["paths"][k]), W.fresh(f.seed, f.target))
            vm = ctx.download_output("vecmap", k)
            assert np.array_equal(bits(vm), bits(maps[k])), (where, k)
            keep(out, "dijkstra %s %s plan %d" % (engine, kernel, k), b["dist"][k], b["pred"][k], b["paths"][k], vm)
        keep(out, "dijkstra %s %s" % (engine, kernel), b["codes"], b["path_len"])
    ctx.set_option("tb_kernel", None)
    ctx.set_dijkstra_engine("auto")
    # paths only: no finalize pass, nothing V-sized handed out but the popped potential
    ctx.set_resident_outputs(False)
    b = ctx.plan_dijkstra_batch(W.seeds, W.targets, OFFSET, LIMIT, want_fields=False)
    ctx.set_resident_outputs(True)
    assert np.array_equal(b["codes"], codes), (tag, "paths only")
    for k, f in enumerate(fields):
        assert not ctx.device_output(k, 0) and not ctx.device_output(k, 1), (tag, k)
        if f.dist is None:
            assert len(b["paths"][k]) == 0
            continue
        ref = W.fresh(f.seed, f.target)
        assert np.array_equal(b["paths"][k], ref.path), (tag, "paths only", k)
        pot = ctx.download_output("popped", k)
        if ref.code == 0:
            full = W.fresh(f.seed, f.target, np.inf).dist
            m = popped(full, f.target, OFFSET)
            assert np.array_equal(bits(pot[m]), bits(full[m])) and np.isinf(pot[~m]).all(), (tag, "popped", k)
        keep(out, "paths only plan %d" % k, b["paths"][k], pot)


def cvp_calls(ctx, W, tag, out):
    sp, sf, tp, tf, refs, walks, codes = cvp_plans(W)
    ctx.set_option("cvp_wide", 1)                                             # the wide step kernel at these plan counts (auto takes it from 32 plans on)
    b = ctx.plan_cvp_batch(sp, sf, tf, OFFSET, CVP_LIMIT, want_fields=True, want_vecmap=True)
    ctx.set_option("cvp_wide", None)
    assert np.array_equal(b["codes"], codes), (tag, b["codes"], codes)
    got = ctx.backtrack_cvp_batch(sp, sf, tp, tf, step_width=0.15)
    for k, r in enumerate(refs):
        st, pos, face = got[k]
        if r is None:
            assert (st, len(face)) == (0, 0), (tag, k)
            continue
        assert_cvp_close(SimpleNamespace(code=int(b["codes"][k]), dist=b["dist"][k], pred=b["pred"][k]), r)
        assert np.array_equal(bits(b["vecmap"][k]), bits((r.vecmap * r.has_vec[:, None]).astype(np.float32))), (tag, "cvp vector map", k)
        if walks[k] is not None:
            rc, ppos, pface = walks[k]
            assert (st == 1) == (rc == 0) and np.array_equal(face, pface) and np.array_equal(bits(pos), bits(ppos)), (tag, "walk", k)
        keep(out, "cvp plan %d" % k, b["dist"][k], b["pred"][k], b["vecmap"][k], np.int32(st), pos, face)


def vector_field(ctx, layer, W, vec, where):
    """the vector field of an inflation layer against the oracle's; returns the has-entry flags.  None: the wave met a vertex
    of more than 15 neighbours and kept no field (include/mnav.h) -- on a mesh that has such a vertex only."""
    try:
        dv, has = ctx.layer_vectors(layer)
    except RuntimeError as e:
        assert "more than 15 neighbours" in str(e) and int(W.deg.max()) > 15, (where, str(e), int(W.deg.max()))
        return None
    same = (bits(dv).reshape(-1, 3) == bits(vec).reshape(-1, 3)).all(axis=1) | (np.isnan(dv).any(axis=1) & np.isnan(vec).any(axis=1))
    same |= (has == 0) & (vec == 0).all(axis=1)                                # no entry in the reference's map
    assert same.all(), (where, layer, int((~same).sum()))
    return has


def graph_state(ctx, model, W, where):
    """same_state of tests/test_gpu_layer_graph.py: every layer slot, the inflation distances and (where the mesh allows
    them) vector fields, the resident vertex costs and edge weights"""
    for slot in model.order:
        infl = model.nodes[slot]["kind"] == "inflation"
        got = ctx.layer_download(slot, distances=infl)
        assert np.array_equal(bits(got[0]), bits(model.cost[slot])), (where, slot, int((bits(got[0]) != bits(model.cost[slot])).sum()))
        assert np.array_equal(got[1] != 0, model.lethal[slot] != 0), (where, slot)
        if infl:
            assert np.array_equal(bits(got[2]), bits(model.dist[slot])), (where, slot)
            vector_field(ctx, slot, W, model.vec[slot], where)
    vc, w = ctx.download_costs()
    assert np.array_equal(bits(vc), bits(model.vertex_costs)) and np.array_equal(bits(w), bits(model.edge_weights)), where


def layer_calls(ctx, W, tag, out):
    m, L, nrm = W.mesh, W.layer_inputs, W.case.vn
    # inflation with its vector field (the wave works in plan slot 0)
    ctx.layer_upload(0, W.costs0, L["lethal"])
    ctx.layer_inflation(1, 0)
    cost, dist, vec = W.om.inflation(L["lethal"], W.case.edge_dist)
    c, le, d = ctx.layer_download(1, distances=True)
    assert np.array_equal(bits(d), bits(dist)) and np.array_equal(bits(c), bits(cost)) and np.array_equal(le, L["lethal"]), tag
    got = vector_field(ctx, 1, W, vec, tag)
    keep(out, "inflation vectors", np.uint8(got is not None), *([] if got is None else [got]))
    keep(out, "inflation", c, le, d)
    # obstacle, clearance, border, height difference / roughness / ridge
    obs = check_obstacle(ctx, 2, m, L["cloud"])
    keep(out, "obstacle", *ctx.layer_download(2))
    clr, _ = clearance_case(ctx, m, nrm, layer=8)
    keep(out, "clearance", clr, *ctx.layer_download(8))
    check_layer(ctx, 9, ctx.layer_border(9), CM.border_layer(m.V, m.edges, m.faces))
    keep(out, "border", *ctx.layer_download(9))
    check_nbhd(ctx, m, nrm, 0.3, layer=10)
    keep(out, "ridge", *ctx.layer_download(10))
    # a layer graph over the uploaded layer, the obstacle layer and a third input; one obstacle update, one map_update_layer
    ctx.layer_upload(4, L["third"])
    model = MM.MapModel(W.om, W.case.edge_dist, GRAPH, 6, 1.0, W.invalid)
    model.set_input(0, W.costs0, L["lethal"])
    model.set_input(2, obs["cost"], obs["lethal"])
    model.set_input(4, L["third"])
    ctx.map_configure(GRAPH, 6, 1.0, W.invalid)
    ctx.map_compute()
    model.compute()
    graph_state(ctx, model, W, (tag, "compute"))
    a = ctx.map_obstacle(2, L["cloud2"])
    want = OM.obstacle_layer(m.xyz, m.faces, L["cloud2"], old_lethal=obs["lethal"])
    c2, le2 = ctx.layer_download(2)
    assert np.array_equal(le2, want["lethal"]) and np.array_equal(bits(c2), bits(want["cost"])), (tag, "map_obstacle")
    D = model.replace_layer(2, c2, le2, want["changed"])
    assert np.array_equal(a["changed"], D), (tag, "map_obstacle", a["changed"].size, D.size)
    graph_state(ctx, model, W, (tag, "map_obstacle"))
    D2 = model.update_layer(0, L["ids"], L["upd_cost"], L["upd_lethal"])
    b = ctx.map_update_layer(0, L["ids"], L["upd_cost"], L["upd_lethal"])
    assert np.array_equal(b["changed"], D2), (tag, "map_update_layer", b["changed"].size, D2.size)
    graph_state(ctx, model, W, (tag, "map_update_layer"))
    if W.name != "T":
        assert obs["lethal"].any() and D.size >= 1, (tag, int(obs["lethal"].sum()), D.size)
    keep(out, "graph", a["changed"], b["changed"], *ctx.download_costs())
    W.upload_costs(ctx)                                                       # the world's own costs again, for the calls that follow


def locate_calls(ctx, W, tag, out):
    pts, want = locate_queries(W)
    got = ctx.locate(pts)
    LM.assert_same(got, want, (tag, "locate"))
    keep(out, "locate", got["vertex"], got["face"], got["bary"], got["dist"])


def follower_calls(ctx, W, tag, out):
    cfg, tick, roll = follower_wants(W)
    robots, goals = W.follow_robots
    r = W.running
    b = ctx.plan_dijkstra_batch(W.seeds[r], W.targets[r], OFFSET, LIMIT)
    assert np.array_equal(b["codes"], W.plan_codes()[r]), tag
    for k, vm in enumerate(vector_maps(W)):
        assert np.array_equal(bits(ctx.download_output("vecmap", k)), bits(vm)), (tag, "vector map", k)   # what the models read
    o = ctx.follow(robots["pos"], robots["dir"], robots["up"], robots["face_in"], robots["slot"], None, capi.FollowConfig(**cfg))
    got = {k: getattr(o, k) for k in ("code", "how", "face", "bary", "pos", "mesh_dir", "cost", "cmd")}
    FOL.assert_same(got, tick, (tag, "follow"))
    keep(out, "follow", *[got[k] for k in sorted(got)])
    ro = capi.RolloutConfig(dt=DT, dist_tolerance=DIST_TOL, angle_tolerance=ANG_TOL, ticks=ROLLOUT_TICKS, trace_stride=1)
    g = ctx.rollout(robots["pos"], robots["dir"], robots["up"], robots["face_in"], robots["slot"], None, goals[0], goals[1], capi.FollowConfig(**cfg), ro)
    assert not g.cancelled
    RM.assert_same(g, roll, (tag, "rollout"))
    keep(out, "rollout", *[getattr(g, k) for k in RM.KEYS], g.trace)
    print(tag, "follow how", np.bincount(tick["how"], minlength=5), "rollout status", np.bincount(roll["status"], minlength=4))


def assignment(ctx, W, fields, vtx, where, out):
    """fleet_assign over all plans: a valid assignment, the optimum of the exact solver and the model's auction bit for bit
    (the checks of tests/test_gpu_dispatch.py)"""
    n, m = len(vtx), len(fields)
    pot, feasible, want, best = auction_wants(W, tuple(int(v) for v in vtx), tuple((f.seed, f.target) for f in fields))
    got = ctx.fleet_assign(vtx, slots=None, m=m, quantum=QUANTUM)
    st = ctx.dispatch_stats()
    sor, ros = got["slot_of_robot"], got["robot_of_slot"]
    has = sor != FM.NONE
    col_of = np.full(n, FM.NONE, np.uint32)
    for j in range(m):
        if ros[j] != FM.NONE:
            assert sor[ros[j]] == j, (where, j)
            col_of[ros[j]] = j
    assert int((ros != FM.NONE).sum()) == int(has.sum()) == got["assigned"] and all(feasible[i, int(col_of[i])] for i in np.flatnonzero(has)), where
    assert np.array_equal(bits(got["potential"]), bits(np.where(has, pot[np.arange(n), np.where(has, col_of, 0)], np.inf).astype(np.float32))), where
    assert (got["assigned"], got["total_q"]) == best, (where, got["assigned"], got["total_q"], best)
    assert np.array_equal(col_of, want["col_of_robot"]), where
    assert (st["phases"], st["rounds"], st["bids"], st["assigned"]) == (want["phases"], want["rounds"], want["bids"], want["size"]), (where, st)
    keep(out, "assign", sor, ros, got["potential"], np.int64(got["total_q"]))


def fleet_calls(ctx, W, tag, out):
    fields = W.fields()
    sl, vt = W.robots()
    n = len(sl)
    b = ctx.plan_dijkstra_batch(W.seeds, W.targets, OFFSET, LIMIT)
    assert np.array_equal(b["codes"], W.plan_codes()), tag
    # paths
    want, _ = check_paths(ctx, W, fields, sl, vt, (tag, "paths"))
    p = ctx.fleet_paths(sl, vt)
    keep(out, "fleet paths", p["codes"], p["path_len"], p["offsets"], p["ids"], p["potential"])
    if W.name != "T":
        assert want["counts"][1] >= 1 and want["counts"][2] >= 1, (tag, want["counts"])      # MNAV_BEYOND_FIELD and no path
    # walks over the vector maps of the plans that ran
    maps = [None] * len(fields)
    for k, vm in zip(W.running, vector_maps(W)):
        maps[k] = (vm, (vm != 0).any(axis=1).astype(np.uint8))
    sf = np.array([face_of(W.mesh, int(s)) for s in W.seeds], np.uint32)
    sp = np.stack([centroid(W.mesh, int(f)) for f in sf])
    pos, face = walk_robots(W, np.random.default_rng(9), n)
    w = ctx.fleet_walks(sl, sp, sf, pos, face, step_width=0.15, walk_cap=512)
    tally = check_walks(w, W, maps, sp, sf, sl, pos, face, 0.15, 512, (tag, "walks"))
    keep(out, "fleet walks", w["status"], w["path_len"], w["offsets"], w["faces"], w["positions"])
    # plans
    start = (W.mesh.xyz[np.minimum(vt, W.V - 1)] + np.random.default_rng(10).uniform(-0.03, 0.03, (n, 3)).astype(np.float32) * np.float32([1, 1, 0.2])).astype(np.float32)
    goal = goal_positions(W, fields)
    check_plans(ctx, W, W.case.vn, fields, sl, vt, start, goal, (tag, "plans"), fresh=10)
    pl = ctx.fleet_plans(sl, start, goal, vt)
    keep(out, "fleet plans", pl["codes"], pl["path_len"], pl["offsets"], pl["cost"], pl["poses"])
    # dispatch
    codes, pot, _ = check_matrix(ctx, W, fields, vt, None, (tag, "costs"))
    keep(out, "fleet costs", codes, pot)
    assignment(ctx, W, fields, vt[:ASSIGN_ROBOTS], (tag, "assign"), out)
    # traffic, timed traffic with 5 and then 70 windows, the traffic layer
    tr = check_traffic(ctx, W, fields, sl, vt, (tag, "traffic"))
    counts = ctx.traffic_download()
    keep(out, "traffic", counts)
    state = XM.Cells(W.V)
    run = FM.run(fields, W.V, sl, vt)
    for B in (5, 70):
        depart, pace, key, tau = timing(n, fields, B, 11 * n + B)
        tt = check_timed(ctx, W, fields, sl, vt, (tag, "timed", B), state, run, depart=depart, pace=pace, key=key, windows=B, tau=tau, free_count=1)
        d = ctx.timed_traffic_download()
        keep(out, "timed %d" % B, d["cells"], d["holders"], d["peak"], d["window"])
        if W.name != "T":
            assert tt["over_cells"] >= 1, (tag, B, tt)
    if W.name != "T":
        assert 5 * tr["contributing"] >= 2 * n, (tag, tr["contributing"], n)
    got = ctx.layer_traffic(12, 1, 0.125, 1.0)
    cost, lethal = ctx.layer_download(12)
    assert np.array_equal(bits(cost), bits(TM.cost(counts, 1, 0.125, 1.0))) and not lethal.any(), (tag, "layer_traffic")
    assert np.array_equal(got["changed"], np.arange(W.V)), (tag, "layer_traffic")         # a fresh slot lists every vertex
    keep(out, "traffic layer", cost)
    print(tag, "fleet", want["counts"], "walk statuses", tally, "contributing", tr["contributing"], "of", n)


def replan_calls(ctx, W, tag, out):
    """update_costs on 10 vertices in three steps, each followed by one of the replans; the plans are those that reach the
    device (a plan that never does makes every replan plan the whole call afresh: reason 3)"""
    r = W.running
    seeds, targets = W.seeds[r], W.targets[r]
    ctx.set_option("replan_fresh_below", 0)                                   # the repair at every level (the policy has tests of its own)
    try:
        b = ctx.plan_dijkstra_batch(seeds, targets, OFFSET, LIMIT)
        assert "k_plan_async" in ctx.last_engine(), (tag, ctx.last_engine())
        for step, (ids, call) in enumerate(zip(W.cost_changes, ("replan", "each", "warm"))):
            W.change_costs(ctx, ids, 0.45, "ABC"[: step + 1])
            if call == "warm":
                ctx.set_option("replan_repair_engine", 5)
            a = (ctx.replan_dijkstra_each if call == "each" else ctx.replan_dijkstra)(None, OFFSET, want_dist=True, want_pred=True)
            ctx.set_option("replan_repair_engine", None)
            rp = a["replan"]
            print(tag, call, {k: v for k, v in rp.items() if k != "levels"}, None if call != "each" else {k: v for k, v in a["each"].items() if k not in ("levels", "classes")})
            assert rp["log_len"] == len(ids), (tag, call, rp)
            if call != "each":
                assert rp["reason"] == 0, (tag, call, rp)                         # repaired, not planned afresh
            if call == "warm":
                assert a["warm"]["plans"] == len(r) and a["warm"]["fallback"] == 0, (tag, a["warm"])
            for k in range(len(r)):
                ref = W.fresh(seeds[k], targets[k])
                assert_dijkstra_equal(SimpleNamespace(code=int(a["codes"][k]), dist=a["dist"][k], pred=a["pred"][k], path=a["paths"][k]), ref)
            keep(out, "replan %s" % call, a["codes"], a["dist"], a["pred"], a["path_len"])
    finally:
        ctx.set_option("replan_fresh_below", None)
        ctx.set_option("replan_repair_engine", None)
        W.restore_costs()


def check_stop(ctx, W, tag):
    """Everything a stop runs on the mesh of W, uploaded here into ctx (fresh, or holding another mesh and its state).
    Returns the exact outputs, by name, and the device bytes at the end."""
    assert_conditions(W)
    out = {}
    W.upload(ctx)
    ctx.set_resident_outputs(True)
    dijkstra_calls(ctx, W, tag, out)
    cvp_calls(ctx, W, tag, out)
    layer_calls(ctx, W, tag, out)
    locate_calls(ctx, W, tag, out)
    follower_calls(ctx, W, tag, out)
    fleet_calls(ctx, W, tag, out)
    replan_calls(ctx, W, tag, out)
    return out, ctx.device_bytes()


# -- a fresh context per mesh, and the sequences -----------------------------------------------------------------------
_fresh = {}


def fresh_stop(factory, name, tile):
    """check_stop of the world on a context of its own, run once"""
    if (name, tile) not in _fresh:
        ctx = factory()
        try:
            _fresh[(name, tile)] = check_stop(ctx, world(name, tile), ("fresh", name, tile))
        finally:
            ctx.close()
    return _fresh[(name, tile)]


@pytest.mark.parametrize("name,tile", [("S", 64), ("L", 64), ("T", 64), ("H", 64), ("L", 128)])
def test_a_fresh_context_meets_every_check(gpu_ctx_factory, name, tile):
    out, nbytes = fresh_stop(gpu_ctx_factory, name, tile)
    assert len(out) > 30 and nbytes > 0


def run_sequence(factory, stops):
    ctx = factory()
    first = None
    try:
        for i, (name, tile) in enumerate(stops):
            tag = ("stop %d" % i, name, tile)
            got, nbytes = check_stop(ctx, world(name, tile), tag)
            want, want_bytes = fresh_stop(factory, name, tile)
            same_outputs(got, want, tag)                                       # nothing of the meshes before leaks into this one
            assert nbytes == want_bytes, (tag, nbytes, want_bytes)
            if i == 0:
                first = (got, nbytes)
        same_outputs(got, first[0], "the last stop against the first")
        assert nbytes == first[1], (nbytes, first[1])
    finally:
        ctx.close()


def test_one_context_across_S_L_T_H_S(gpu_ctx_factory):
    run_sequence(gpu_ctx_factory, [("S", 64), ("L", 64), ("T", 64), ("H", 64), ("S", 64)])


def test_one_context_across_tile_sizes(gpu_ctx_factory):
    """tile_size is read at upload: the tile tables change shape under the same context"""
    run_sequence(gpu_ctx_factory, [("S", 64), ("L", 128), ("S", 64)])


# -- refusals between a mesh and its next plan -------------------------------------------------------------------------
def p_(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def raw_download(ctx, slot, what, V):
    """mnav_download_output into a sentinel-filled buffer: (rc, untouched)"""
    buf = np.full(3 * V + 1, SENTINEL, np.uint32)
    rc = ctx._L.mnav_download_output(ctx._h, int(slot), int(what), p_(buf))
    return rc, bool((buf == SENTINEL).all())


def raw_follow(ctx, robots, rollout):
    n = robots["pos"].shape[0]
    code, cmd = np.full(n, -7, np.int32), np.full((n, 2), -7.0)
    cfg = capi.FollowConfig()
    args = [ctx._h, n, p_(robots["pos"]), p_(robots["dir"]), p_(robots["up"]), p_(robots["face_in"]), p_(robots["slot"]), None]
    if rollout:
        ro = capi.RolloutConfig(dt=DT, dist_tolerance=DIST_TOL, angle_tolerance=ANG_TOL, ticks=2, trace_stride=0)
        status, pos = np.full(n, -7, np.int32), np.full((n, 3), -7.0, np.float32)
        rc = ctx._L.mnav_follow_rollout(*args, None, None, C.byref(cfg), C.byref(ro), p_(status), None, p_(pos), None, None, None, None, None, None)
        return rc, bool((status == -7).all() and (pos == -7.0).all())
    rc = ctx._L.mnav_follow_batch(*args, C.byref(cfg), p_(code), None, None, None, None, None, p_(cmd), None)
    return rc, bool((code == -7).all() and (cmd == -7.0).all())


def raw_walks(ctx, W, slots, n_plans, plans):
    """mnav_fleet_walks / mnav_fleet_plans with sentinel-filled per-robot outputs"""
    n = len(slots)
    sf = np.resize(np.array([face_of(W.mesh, int(s)) for s in W.seeds if s < W.V], np.uint32), n_plans)      # (n_plans rows, whatever the world's own count)
    sp = np.stack([centroid(W.mesh, int(f)) for f in sf])
    pos = np.ascontiguousarray(W.mesh.xyz[np.arange(n) % W.V], np.float32)
    status, lens = np.full(n, SENTINEL, np.uint32), np.full(n, SENTINEL, np.uint32)
    tot = C.c_uint64(SENTINEL)
    if plans:
        goal = np.ascontiguousarray(sp)
        vtx = (np.arange(n) % W.V).astype(np.uint32)
        rc = ctx._L.mnav_fleet_plans(ctx._h, n, p_(slots), p_(vtx), p_(pos), n_plans, p_(goal), p_(status), None, None, p_(lens), None, None, None, 0, C.byref(tot))
    else:
        rc = ctx._L.mnav_fleet_walks(ctx._h, n, p_(slots), n_plans, p_(sp), p_(sf), p_(pos), None, 0.15, -1, 64, p_(status), None, p_(lens), None, None, None, 0, C.byref(tot))
    return rc, bool((status == SENTINEL).all() and (lens == SENTINEL).all() and tot.value == SENTINEL)


def refusals_after_a_new_mesh(ctx, old, new):
    """every reader of resident outputs, between upload_mesh of `new` (with its costs) and the next plan call; `old`: the
    world whose plans ran last.  Every call returns its error code with mnav_last_error set and touches no output."""
    n_old, V = len(old.seeds), new.V
    robots, _ = new.follow_robots
    robots = {k: (None if v is None else np.ascontiguousarray(v[:2])) for k, v in robots.items()}
    robots["slot"] = np.zeros(2, np.uint32)
    sl, vt = np.zeros(2, np.uint32), new.ok[:2].astype(np.uint32)
    refused = []

    def no(what, rc, untouched, bad=-1):
        assert rc == bad and untouched and ctx._err(), (what, rc, untouched, ctx._err())
        refused.append((what, ctx._err()))

    for slot in (0, n_old - 1, n_old + 3):
        for what, name in enumerate(("dist", "pred", "direction", "cutface", "vecmap", "popped")):
            assert what == 5 or not ctx.device_output(slot, what), (slot, name)
            no(("download", name, slot), *raw_download(ctx, slot, what, V))
    out3 = np.full(3, -7.0, np.float32)
    rc = ctx._L.mnav_vector_at(ctx._h, 0, p_(new.mesh.faces[0].astype(np.uint32)), p_(np.float32([0.3, 0.3, 0.4])), p_(out3))
    no("vector_at", rc, bool((out3 == -7.0).all()))
    sp, sf, tp, tf = cvp_plans(new)[:4]
    pos, face, cnt, st = np.full((1, 8, 3), -7.0, np.float32), np.full((1, 8), SENTINEL, np.uint32), np.full(1, SENTINEL, np.uint32), np.full(1, -7, np.int32)
    rc = ctx._L.mnav_backtrack_cvp_batch(ctx._h, 1, p_(sp[:1]), p_(sf[:1]), p_(tp[:1]), p_(tf[:1]), 0.15, -1, 8, p_(pos), p_(face), p_(cnt), p_(st))
    no("backtrack_cvp_batch", rc, bool((pos == -7.0).all() and (face == SENTINEL).all() and cnt[0] == SENTINEL and st[0] == -7))
    no("follow", *raw_follow(ctx, robots, False))
    no("follow_rollout", *raw_follow(ctx, robots, True))
    no("fleet_paths", *raw_paths(ctx, sl, vt))
    no("fleet_walks", *raw_walks(ctx, new, sl, n_old, False))                  # (as found: the robot-side calls still see the old plan count)
    no("fleet_plans", *raw_walks(ctx, new, sl, n_old, True))
    no("fleet_costs", *raw_costs(ctx, vt, None, n_old))
    no("fleet_assign", *raw_assign(ctx, vt, None, n_old, QUANTUM))
    no("fleet_traffic", *raw_traffic(ctx, sl, vt, np.ones(2, np.uint32), False))
    no("fleet_timed_traffic", *raw_timed(ctx, sl, vt))
    for name in ("map_traffic", "map_timed_traffic"):                          # the graph went with the mesh
        ch, nc = np.full(V, SENTINEL, np.uint32), C.c_uint32(SENTINEL)
        rc = getattr(ctx._L, "mnav_" + name)(ctx._h, 0, 0, 1.0, np.inf, p_(ch), C.byref(nc))
        no(name, rc, bool((ch == SENTINEL).all() and nc.value == SENTINEL))
    for name in ("mnav_replan_dijkstra_batch", "mnav_replan_dijkstra_each"):
        for targets in (None, np.zeros(n_old, np.uint32)):
            codes, lens = np.full(n_old, SENTINEL, np.uint32), np.full(n_old, SENTINEL, np.uint32)
            rc = getattr(ctx._L, name)(ctx._h, n_old, p_(targets), OFFSET, p_(codes), None, None, None, 0, p_(lens))
            no((name, targets is not None), rc, bool((codes == SENTINEL).all() and (lens == SENTINEL).all()), bad=capi.INTERNAL_ERROR)
    return refused


def refusals_after_a_cvp_call_and_a_new_mesh(ctx, old, new):
    """the same between a CVP batch on `old` and the next plan on `new`: the readers that work on CVP fields"""
    n_old = len(old.seeds)
    refused = []

    def no(what, rc, untouched):
        assert rc == -1 and untouched and ctx._err(), (what, rc, untouched, ctx._err())
        refused.append((what, ctx._err()))

    for what, name in enumerate(("dist", "pred", "direction", "cutface", "vecmap", "popped")):
        assert what == 5 or not ctx.device_output(0, what), name
        no(("download", name, 0), *raw_download(ctx, 0, what, new.V))
    valid = (cvp_plans(new)[1] < new.mesh.F) & (cvp_plans(new)[3] < new.mesh.F)
    sp, sf, tp, tf = (np.ascontiguousarray(np.resize(a, (n_old,) + a.shape[1:])) for a in (x[valid] for x in cvp_plans(new)[:4]))
    pos, face = np.full((n_old, 8, 3), -7.0, np.float32), np.full((n_old, 8), SENTINEL, np.uint32)
    cnt, st = np.full(n_old, SENTINEL, np.uint32), np.full(n_old, -7, np.int32)
    rc = ctx._L.mnav_backtrack_cvp_batch(ctx._h, n_old, p_(sp), p_(sf), p_(tp), p_(tf), 0.15, -1, 8, p_(pos), p_(face), p_(cnt), p_(st))
    no("backtrack_cvp_batch", rc, bool((pos == -7.0).all() and (face == SENTINEL).all() and (cnt == SENTINEL).all() and (st == -7).all()))
    robots = {k: (None if v is None else np.ascontiguousarray(v[:2])) for k, v in new.follow_robots[0].items()}
    robots["slot"] = np.zeros(2, np.uint32)
    no("follow", *raw_follow(ctx, robots, False))
    no("follow_rollout", *raw_follow(ctx, robots, True))
    no("fleet_walks", *raw_walks(ctx, new, np.zeros(2, np.uint32), n_old, False))
    return refused


def fresh_context_statistics(ctx):
    return dict(layer=ctx.obstacle_stats(), nbhd=ctx.neighbourhood_stats(), clearance=ctx.clearance_stats(), map=ctx.map_stats(), locate=ctx.locate_stats(),
                replan=ctx.replan_stats(), each=ctx.replan_each_stats(), warm=ctx.replan_warm_stats(), traffic=ctx.traffic_stats(), timed=ctx.timed_traffic_stats())


def resident_everything(ctx, W):
    """a finalized batch with vector maps, then what fills the per-mesh state a new mesh has to drop"""
    ctx.set_resident_outputs(True)
    b = ctx.plan_dijkstra_batch(W.seeds, W.targets, OFFSET, LIMIT, want_fields=True)
    assert np.array_equal(b["codes"], W.plan_codes())
    sl, vt = W.robots()
    ctx.fleet_traffic(sl, vt)
    ctx.fleet_timed_traffic(sl, vt, windows=5, tau=1.0)
    ctx.locate(locate_queries(W)[0])
    ctx.layer_obstacle(2, W.layer_inputs["cloud"])
    assert ctx.traffic_download().any() and ctx.device_output(0, 0) and ctx.device_output(0, 4) and "k_" in ctx.last_engine()
    assert ctx.download_output("popped", 0).shape == (W.V,)


@pytest.mark.parametrize("first,second", [("L", "S"), ("S", "L")])
def test_refusals_between_a_mesh_and_its_next_plan(gpu_ctx_factory, first, second):
    old, new = world(first), world(second)
    blank = gpu_ctx_factory()
    new.upload(blank)
    want_stats = fresh_context_statistics(blank)
    ctx = gpu_ctx_factory()
    try:
        old.upload(ctx)
        ctx.set_resident_outputs(True)
        sp, sf, tp, tf, _, _, codes = cvp_plans(old)
        assert np.array_equal(ctx.plan_cvp_batch(sp, sf, tf, OFFSET, CVP_LIMIT)["codes"], codes) and ctx.device_output(int(np.flatnonzero(codes == 0)[0]), 4)
        new.upload(ctx)
        refused = refusals_after_a_cvp_call_and_a_new_mesh(ctx, old, new)
        assert "not a Dijkstra plan" in refused[5][1] and all("not resident" in text for _, text in refused[:5] + refused[6:]), refused
        # a paths-only batch of the tile-batch engine keeps its distances in the engine's buffers, not in plan slots
        old.upload(ctx)
        ctx.set_resident_outputs(False)
        ctx.set_dijkstra_engine("tile_batch")
        b = ctx.plan_dijkstra_batch(old.seeds, old.targets, OFFSET, LIMIT)
        ctx.set_dijkstra_engine("auto")
        assert "k_tb" in ctx.last_engine() and np.array_equal(b["codes"], old.plan_codes()) and ctx.download_output("popped", 0).shape == (old.V,)
        ctx.vector_at(old.mesh.faces[0], np.float32([0.3, 0.3, 0.4]))          # (served from the blocked distances: runs)
        new.upload(ctx)
        for slot in (0, len(old.seeds) + 3):
            rc, untouched = raw_download(ctx, slot, 5, new.V)
            assert rc == -1 and untouched and "output not resident" in ctx._err(), (slot, rc, untouched, ctx._err())
        out3 = np.full(3, -7.0, np.float32)
        rc = ctx._L.mnav_vector_at(ctx._h, 0, p_(new.mesh.faces[0].astype(np.uint32)), p_(np.float32([0.3, 0.3, 0.4])), p_(out3))
        assert rc == -1 and (out3 == -7.0).all() and "not resident" in ctx._err(), (rc, out3, ctx._err())
        old.upload(ctx)
        resident_everything(ctx, old)
        new.upload(ctx)
        refused = refusals_after_a_new_mesh(ctx, old, new)
        for what, text in refused:
            print(what, "->", text)
        for name in ("download", ):
            assert all("output not resident" in text for what, text in refused if what[0] == name), refused
        # the traffic layers are no readers of plan outputs: no counts since the mesh, so a layer of zeros, as in a fresh context
        for call, layer in ((ctx.layer_traffic, 3), (ctx.layer_timed_traffic, 4)):
            got = call(layer, 0, 1.0, np.inf)
            cost, lethal = ctx.layer_download(layer)
            assert np.array_equal(got["changed"], np.arange(new.V)) and not cost.any() and not lethal.any(), layer
        c = ctx.traffic_download()
        assert c.shape == (new.V,) and not c.any()
        d = ctx.timed_traffic_download()
        assert d["cells"].shape == (new.V, 0) and not d["peak"].any() and (d["window"] == FM.NONE).all()
        got_stats = fresh_context_statistics(ctx)
        for k in want_stats:
            a, b = ({x: v for x, v in s.items() if not x.startswith("ms")} for s in (got_stats[k], want_stats[k]))
            assert str(a) == str(b), (k, a, b)
        assert ctx.last_engine() == "none"                                     # -1 after a new mesh: the engine named was the old mesh's
        # one plan on the new mesh, and every call of a stop works and equals the fresh context
        got, nbytes = check_stop(ctx, new, ("after", first, second))
        want, want_bytes = fresh_stop(gpu_ctx_factory, second, 64)
        same_outputs(got, want, (first, second))
        assert nbytes == want_bytes
    finally:
        ctx.close()
        blank.close()


# -- plan-count edges inside one mesh -------------------------------------------------------------------------------------
def test_the_robot_side_calls_see_the_plans_of_the_last_call(gpu_ctx_factory):
    """200 plans, then 1, then 65 on L through `auto`: after each call every robot-side call refers to exactly its plans, a
    slot index >= the last n is refused although the device slot still exists, and the outputs equal a fresh context's"""
    W = world("L")
    rng = np.random.default_rng(41)
    pick = rng.choice(W.ok, 400, replace=False).astype(np.uint32)
    seeds, targets = pick[:200], pick[200:]
    ctx = gpu_ctx_factory()
    try:
        W.upload(ctx)
        ctx.set_resident_outputs(True)
        robots, _ = W.follow_robots
        two = {k: (None if v is None else np.ascontiguousarray(v[:2])) for k, v in robots.items()}
        for n in (200, 1, 65):
            b = ctx.plan_dijkstra_batch(seeds[:n], targets[:n], OFFSET, LIMIT)
            fields = []
            for k in range(n):
                r = W.fresh(seeds[k], targets[k])
                assert b["codes"][k] == r.code and np.array_equal(b["paths"][k], r.path), (n, k)
                fields.append(FM.Field(r.dist, r.pred, int(seeds[k]), int(targets[k]), OFFSET))
            m = 4 * n + 3
            sl = (np.arange(m) % n).astype(np.uint32)
            vt = rng.integers(0, W.V, m).astype(np.uint32)
            got = {}
            check_paths(ctx, W, fields, sl, vt, ("plans", n))
            check_traffic(ctx, W, fields, sl, vt, ("traffic", n))
            check_timed(ctx, W, fields, sl, vt, ("timed", n), XM.Cells(W.V), windows=5, tau=1.0, free_count=1)
            check_matrix(ctx, W, fields, vt[:40], None, ("costs", n))
            assignment(ctx, W, fields, vt[:40], ("assign", n), got)
            r = min(100, m)                                                  # robots of the plans and the walks
            start = (W.mesh.xyz[vt[:r]] + np.float32([0.01, -0.02, 0.004])).astype(np.float32)
            check_plans(ctx, W, W.case.vn, fields, sl[:r], vt[:r], start, goal_positions(W, fields), ("fleet plans", n), fresh=5)
            wsf = np.array([face_of(W.mesh, int(s)) for s in seeds[:n]], np.uint32)
            wsp = np.stack([centroid(W.mesh, int(f)) for f in wsf])
            wpos, wface = walk_robots(W, np.random.default_rng(9), r)
            w = ctx.fleet_walks(sl[:r], wsp, wsf, wpos, wface, step_width=0.15, walk_cap=512)
            vms = {int(k): W.om.dijkstra_vector_map(fields[int(k)].pred) for k in np.unique(sl[:r])}
            check_walks(w, W, [None if k not in vms else (vms[k], (vms[k] != 0).any(axis=1).astype(np.uint8)) for k in range(n)], wsp, wsf, sl[:r], wpos, wface, 0.15, 512,
                        ("fleet walks", n))
            o = ctx.follow(robots["pos"], robots["dir"], robots["up"], robots["face_in"], (np.arange(W.n_robots) % n).astype(np.uint32), None, capi.FollowConfig(**FOL.config()))
            maps = [ctx.download_output("vecmap", k) for k in range(min(n, 3))]
            for k in range(min(n, 3)):
                assert np.array_equal(bits(maps[k]), bits(W.om.dijkstra_vector_map(fields[k].pred))), (n, k)
            # a slot >= n: refused, outputs untouched, although device slot n exists since the batch of 200
            bad = np.array([0, n], np.uint32)
            for what, (rc, untouched) in (("paths", raw_paths(ctx, bad, vt[:2])), ("traffic", raw_traffic(ctx, bad, vt[:2], np.ones(2, np.uint32), True)),
                                           ("timed", raw_timed(ctx, bad, vt[:2], windows=5, accumulate=True)), ("costs", raw_costs(ctx, vt[:2], bad, 2)),
                                           ("assign", raw_assign(ctx, vt[:2], bad, 2, QUANTUM)),
                                           ("follow", raw_follow(ctx, dict(two, slot=bad), False)), ("rollout", raw_follow(ctx, dict(two, slot=bad), True)),
                                           ("walks", raw_walks(ctx, W, bad, n, False)), ("plans", raw_walks(ctx, W, bad, n, True))):
                assert rc == -1 and untouched and "slot" in ctx._err(), (n, what, rc, untouched, ctx._err())
            for what in (0, 1, 4):
                assert not ctx.device_output(n, what) and raw_download(ctx, n, what, W.V) == (-1, True), (n, what)
            # ... and a fresh context with this batch alone gives the same bits
            other = gpu_ctx_factory()
            try:
                W.upload(other)
                other.set_resident_outputs(True)
                other.plan_dijkstra_batch(seeds[:n], targets[:n], OFFSET, LIMIT)
                for k in range(min(n, 3)):
                    for w in ("dist", "pred", "vecmap"):
                        assert np.array_equal(u(ctx.download_output(w, k)), u(other.download_output(w, k))), (n, k, w)
                a, c = ctx.fleet_paths(sl, vt), other.fleet_paths(sl, vt)
                assert all(np.array_equal(u(a[k]), u(c[k])) for k in ("codes", "path_len", "offsets", "ids", "potential")), n
                o2 = other.follow(robots["pos"], robots["dir"], robots["up"], robots["face_in"], (np.arange(W.n_robots) % n).astype(np.uint32), None, capi.FollowConfig(**FOL.config()))
                assert all(FOL.same_bits(getattr(o, k), getattr(o2, k)) for k in ("code", "how", "face", "bary", "pos", "mesh_dir", "cost", "cmd")), n
            finally:
                other.close()
    finally:
        ctx.close()
