"""GPU: fleet plans (mnav_upload_face_normals, mnav_fleet_plans, mnav_fleet_walk_plans).

Plans: every robot's code, vertex, potential, pose count, offset, poses and cost equal tests/plans_model.py (the paths of
tests/fleet_model.py posed by OracleMesh.dijkstra_poses) and, for served robots, the poses of a fresh plan of the CPU
oracle, over the fields left by the tile rounds, the tile-batch engine and a replan after a cost update.  Walk plans:
OracleMesh.cvp_backtrack + OracleMesh.cvp_poses.  Everything bit for bit (doubles through view(np.uint64)); a NaN matches
any NaN, and outside the degenerate test there is none.

Shapes: terrain(48) = 2304 vertices, 8 plans, up to 3 * 256 + 41 robots."""
import ctypes as C

import numpy as np
import pytest

from mesh_navigation_amd import capi, meshgen
from mesh_navigation_amd.planner import DijkstraMeshPlanner
from oracle import oracle as O
from tests import fleet_model as FM
from tests import plans_model as PM
from tests.common import Case
from tests.fleet_model import bits
from tests.test_gpu_fleet import LIMIT, OFFSET, SENTINEL, Plain, World, check_walks, make_ctx, seed_ends, walk_robots

pytestmark = pytest.mark.gpu
COUNTS = (0, 1, 65, 3 * 256 + 41)


@pytest.fixture(scope="module")
def world():
    return World()


def goal_positions(W, fields):
    return np.array([W.mesh.xyz[min(f.seed, W.V - 1)] + np.array([0.023, 0.011, 0.004], np.float32) for f in fields], np.float32)


def robots(W, fields, n, seed):
    """n robots spread over the plans: random vertices, the special ones of every plan; every third robot stands on its
    plan's seed or on no vertex, so rows without poses sit between the others; positions near the vertices"""
    rng = np.random.default_rng(seed)
    slots = (np.arange(n) % len(fields)).astype(np.uint32)
    vtx = rng.integers(0, W.V, n).astype(np.uint32)
    if n >= 64:
        free, k = [i for i in range(n) if i % 3], 0                         # (robot 0, 3, 6, ... belong to the loop below)
        for s, f in enumerate(fields):
            special = [f.target, W.V, FM.NONE] + ([] if f.dist is None else list(FM.robots_of(f, W.V, rng, 0)))
            for v in special[:6]:
                if k < len(free):
                    slots[free[k]], vtx[free[k]] = s, min(int(v), FM.NONE)
                    k += 1
        for i in range(0, n, 3):
            vtx[i] = fields[int(slots[i])].seed if (i // 3) % 2 else W.V + 1
    on = np.minimum(vtx, W.V - 1)
    start = (W.mesh.xyz[on] + rng.uniform(-0.03, 0.03, (n, 3)).astype(np.float32) * np.array([1, 1, 0.2], np.float32)).astype(np.float32)
    return slots, vtx, start


def check_plans(ctx, W, vn, fields, slots, vtx, start, goal, where, from_positions=False, fresh=40):
    out = ctx.fleet_plans(slots, start, goal, None if from_positions else vtx)
    stats = ctx.fleet_stats()
    n = len(slots)
    assert np.array_equal(out["vertex"], vtx), where
    want = PM.run(W.om, vn, fields, W.V, slots, vtx, start, goal)
    total = int(want["offsets"][n])
    nan = PM.same(out, want, where)
    print(where, "n", n, "served / beyond / no path / invalid", want["counts"], "poses", total, "NaN poses", nan,
          "ms kernels %.3f total %.3f" % (stats["ms_kernels"], stats["ms_total"]))
    assert out["rc"] == 0 and out["total"] == total == out["poses"].shape[0], (where, out["rc"], out["total"], total)
    if n:
        assert [stats[k] for k in ("served", "beyond_field", "no_path", "invalid")] == want["counts"] and stats["entries"] == total, (where, stats)
    # ... and, whatever the model says: a served robot has the poses and the cost of a fresh plan of the oracle
    checked = 0
    for i in range(n):
        f, v = fields[int(slots[i])], int(vtx[i])
        if checked >= fresh or f.dist is None or v >= W.V or int(out["codes"][i]) != FM.SUCCESS or v == f.seed:
            continue
        r = W.fresh(f.seed, v, f.offset)
        poses, cost = W.om.dijkstra_poses(vn, r.path, start[i], goal[int(slots[i])])
        lo = int(out["offsets"][i])
        PM.same_poses(out["poses"][lo: lo + int(out["path_len"][i])], poses, (where, i))
        assert PM.bits64(out["cost"][i]) == PM.bits64(cost), (where, i)
        checked += 1
    return want, nan, checked


@pytest.mark.parametrize("source", ["tiled", "tile_batch"])
def test_plans_equal_the_model_and_the_oracle(world, source):
    W = world
    ctx = make_ctx(W)
    try:
        ctx.set_dijkstra_engine(source)
        ctx.plan_dijkstra_batch(W.seeds, W.targets, OFFSET, LIMIT)
        assert {"tiled": "k_tile_round", "tile_batch": "k_tb"}[source] in ctx.last_engine(), ctx.last_engine()
        fields = W.fields()
        goal = goal_positions(W, fields)
        nans = 0
        for n in COUNTS:
            sl, vt, st = robots(W, fields, n, 10 + n)
            want, nan, checked = check_plans(ctx, W, W.case.vn, fields, sl, vt, st, goal, (source, n))
            nans += nan
        assert nans == 0                                                    # no NaN pose among random robots
        ln = want["path_len"]
        assert want["counts"][0] >= 100 and want["counts"][1] >= 50 and want["counts"][3] >= 20 and checked >= 30, (want["counts"], checked)
        assert ((ln[1:-1] == 0) & (ln[:-2] > 0) & (ln[2:] > 0)).sum() >= 20   # rows without poses between rows with poses
    finally:
        ctx.close()


def test_plans_after_a_replan(world):
    W = world
    ctx = make_ctx(W)
    seeds, targets = W.seeds[:6], W.targets[:6].copy()
    old = W.costs
    try:
        ctx.set_option("replan_fresh_below", 0)
        ctx.plan_dijkstra_batch(seeds, targets, OFFSET, LIMIT)
        ids = np.array([W.mesh.vertex_at(0.5, 0.5), W.mesh.vertex_at(0.52, 0.5), int(targets[0])], np.uint32)
        ids = ids[~np.isin(ids, seeds)]
        W.change_costs(ctx, ids, 0.45)
        moved = W.mesh.vertex_at(0.3, 0.7)
        if moved != seeds[1]:
            targets[1] = moved
        b = ctx.replan_dijkstra(targets, OFFSET)
        assert b["replan"]["reason"] == 0 and b["replan"]["log_len"] == ids.size
        fields = W.fields(targets)
        goal = goal_positions(W, fields)
        for n in (65, 3 * 256 + 41):
            sl, vt, st = robots(W, fields, n, 40 + n)
            want, nan, checked = check_plans(ctx, W, W.case.vn, fields, sl, vt, st, goal, ("replan", n))
            assert nan == 0
        assert want["counts"][0] >= 100 and checked >= 30
    finally:
        ctx.close()
        W.costs = old
        W.weights = W.om.edge_weights(W.case.edge_dist, W.costs, 1.0)
        W.version += 1


def test_plans_from_positions_and_the_sizing_protocol(world):
    W = world
    ctx = make_ctx(W)
    try:
        ctx.plan_dijkstra_batch(W.seeds, W.targets, OFFSET, LIMIT)
        fields = W.fields()
        goal = goal_positions(W, fields)
        rng = np.random.default_rng(3)
        n = 300
        slots = (np.arange(n) % 6).astype(np.uint32)
        v = rng.integers(0, W.V, n)
        pos = (W.mesh.xyz[v] + rng.uniform(-0.04, 0.04, (n, 3)).astype(np.float32) * np.array([1, 1, 0.2], np.float32)).astype(np.float32)
        nearest = np.array([W.om.nearest_vertex(p) for p in pos], np.uint32)
        want, nan, _ = check_plans(ctx, W, W.case.vn, fields, slots, nearest, pos, goal, "positions", from_positions=True)
        assert nan == 0
        total = int(want["offsets"][n])
        assert total > 100
        # the two-call protocol, by hand: too small a buffer leaves it untouched, reports the size and gives every per-robot output
        L, h = ctx._L, ctx._h
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        for cap, rc_want in ((total - 1, 1), (total, 0)):
            codes, lens, off, cost, tot = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64), np.full(n, -1.0), C.c_uint64(0)
            poses = np.full((total, 7), -7.0, np.float64)
            rc = L.mnav_fleet_plans(h, n, p(slots), p(nearest), p(pos), len(fields), p(goal), p(codes), None, None, p(lens), p(off), p(cost), p(poses), cap, C.byref(tot))
            assert rc == rc_want and tot.value == total, (cap, rc, tot.value)
            assert np.array_equal(codes, want["codes"]) and np.array_equal(lens, want["path_len"]) and np.array_equal(off, want["offsets"])
            assert np.array_equal(PM.bits64(cost), PM.bits64(want["cost"]))
            if rc:
                assert (poses == -7.0).all()
            else:
                PM.same_poses(poses, want["poses"], "cap = total")
        assert L.mnav_fleet_plans(h, 0, *([None] * 3), 0, *([None] * 8), 0, None) == 0      # n = 0 does nothing
    finally:
        ctx.close()


def test_random_normals_take_every_branch_of_the_quaternion(world):
    W = world
    v = np.random.default_rng(5).normal(size=(W.V, 3))
    vn = (v / np.linalg.norm(v, axis=1)[:, None]).astype(np.float32)
    ctx = capi.MnavContext(0)
    try:
        ctx.upload_mesh(W.mesh.xyz, W.mesh.faces, W.mesh.edges, vn)
        ctx.compute_edge_weights(W.costs, W.case.edge_dist, 1.0, W.invalid)
        ctx.set_resident_outputs(True)
        ctx.plan_dijkstra_batch(W.seeds, W.targets, OFFSET, LIMIT)
        fields = W.fields()
        sl, vt, st = robots(W, fields, 257, 77)
        want, nan, _ = check_plans(ctx, W, vn, fields, sl, vt, st, goal_positions(W, fields), "random normals")
        taken = PM.quat_branch(want["poses"])
        print("branches told from the oracle's poses (trace > 0, xx, yy, zz):", taken)
        assert nan == 0 and all(b > 0 for b in taken), taken
    finally:
        ctx.close()


def test_degenerate_first_poses_are_nan_with_exact_position_and_length():
    """a flat mesh (every normal is +-z): a robot 0.5 above xyz[pred[v]] looks along the normal, a robot on xyz[pred[v]]
    looks nowhere -- two NaN quaternions, positions exact, 0.5 and 0 added to the costs"""
    case = Case(meshgen.terrain(48, 0.1, 6, amplitude=0.0))
    mesh, om = case.mesh, case.om
    assert (case.vn[:, :2] == 0).all()
    seed, target = mesh.vertex_at(0.3, 0.35), mesh.vertex_at(0.7, 0.6)
    ref = om.dijkstra(case.weights, case.costs, seed, target, 1e9)
    field = FM.Field(ref.dist, ref.pred, seed, target, 1e9)
    vt = np.array([target, mesh.vertex_at(0.6, 0.2), mesh.vertex_at(0.2, 0.8)], np.uint32)
    first = mesh.xyz[ref.pred[vt]]
    start = np.array([mesh.xyz[target] + np.array([0.01, 0.02, 0.0], np.float32), first[1] + np.array([0, 0, 0.5], np.float32), first[2]], np.float32)
    goal = (mesh.xyz[[seed]] + np.array([0.023, 0.011, 0.0], np.float32)).astype(np.float32)
    with capi.MnavContext(0) as ctx:
        case.upload(ctx)
        ctx.set_resident_outputs(True)
        assert ctx.plan_dijkstra(seed, target, 1e9).code == 0
        out = ctx.fleet_plans(np.zeros(3, np.uint32), start, goal, vt)
    want = PM.run(om, case.vn, [field], mesh.V, np.zeros(3, np.uint32), vt, start, goal)
    assert PM.same(out, want, "degenerate") == 2                            # exactly two NaN poses
    nan = np.isnan(out["poses"]).any(axis=1)
    o = out["offsets"].astype(np.int64)
    assert list(np.flatnonzero(nan)) == [o[1], o[2]] and np.isnan(out["poses"][nan][:, 3:]).all()
    assert np.array_equal(out["poses"][nan][:, :3], start[1:].astype(np.float64))
    for i, length in ((1, 0.5), (2, 0.0)):                                   # what the NaN pose adds to the cost (the cost itself: PM.same above)
        pose0, step = O.pose_from_position(start[i], first[i], case.vn[int(ref.pred[vt[i]])])
        assert step == np.float32(length) and np.isnan(pose0[3:]).all(), (i, step)
        assert out["cost"][i] >= length and out["path_len"][i] == len(om.dijkstra(case.weights, case.costs, seed, int(vt[i]), 1e9).path) + 1


def raw_plans(ctx, slots, vtx, start, goal, n_plans):
    """the C call with sentinel-filled outputs: (rc, whether every output is untouched)"""
    n = len(slots)
    sl, vt = np.ascontiguousarray(slots, np.uint32), np.ascontiguousarray(vtx, np.uint32)
    code, vout, lens = (np.full(n, SENTINEL, np.uint32) for _ in range(3))
    pot, off, cost, poses = np.full(n, np.nan, np.float32), np.full(n + 1, SENTINEL, np.uint64), np.full(n, -7.0), np.full((64, 7), -7.0)
    tot = C.c_uint64(SENTINEL)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = ctx._L.mnav_fleet_plans(ctx._h, n, p(sl), p(vt), p(start), n_plans, p(goal), p(code), p(vout), p(pot), p(lens), p(off), p(cost), p(poses), 64, C.byref(tot))
    untouched = all((a == SENTINEL).all() for a in (code, vout, lens, off)) and np.isnan(pot).all() and (cost == -7.0).all() and (poses == -7.0).all() and tot.value == SENTINEL
    return rc, untouched


def test_refusals_touch_nothing(world):
    W = world
    seeds, targets = W.seeds[:3], W.targets[:3]
    sl, vt = np.zeros(4, np.uint32), np.array(list(targets) + [5], np.uint32)
    start = W.mesh.xyz[vt].copy()
    goal = W.mesh.xyz[seeds].copy()
    ctx = capi.MnavContext(0)
    try:
        def refused(what, start=start, goal=goal, n_plans=3):
            rc, untouched = raw_plans(ctx, sl, vt, start, goal, n_plans)
            assert rc == -1 and untouched and ctx._err(), (what, rc, untouched, ctx._err())
            print(what, "->", ctx._err())

        ctx.upload_mesh(W.mesh.xyz, W.mesh.faces, W.mesh.edges, None)       # a mesh without vertex normals
        ctx.compute_edge_weights(W.costs, W.case.edge_dist, 1.0, W.invalid)
        ctx.set_resident_outputs(True)
        ctx.plan_dijkstra_batch(seeds, targets, OFFSET, LIMIT)
        assert ctx.fleet_paths(sl, vt)["rc"] == 0                          # (the paths need no normals)
        refused("no vertex normals")
        with pytest.raises(RuntimeError):
            ctx.upload_face_normals(W.case.fn[:-1])                         # the wrong F
        with pytest.raises(RuntimeError):
            ctx.fleet_walk_plans(sl, W.mesh.xyz[seeds], np.zeros(3, np.uint32), np.zeros((3, 7)), start, step_width=0.2, walk_cap=64)   # no face normals
        W.upload(ctx)
        refused("no plan yet")
        ctx.plan_dijkstra_batch(seeds, targets, OFFSET, LIMIT)
        keep = [(ctx.download_output("dist", k), ctx.download_output("pred", k)) for k in range(3)]
        assert ctx.fleet_plans(sl, start, goal, vt)["rc"] == 0
        refused("null start_pos", start=None)
        refused("null goal_pos", goal=None)
        refused("the wrong n_plans", n_plans=2)
        sl[3] = 3
        refused("a slot that is not a plan of the last call")
        sl[3] = 0
        ctx.update_costs(np.array([targets[0]], np.uint32), np.array([W.costs[int(targets[0])]], np.float32))
        refused("a stale field after update_costs")
        for k in range(3):
            for x, y in zip(keep[k], (ctx.download_output("dist", k), ctx.download_output("pred", k))):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), k
        ctx.replan_dijkstra(None, OFFSET)
        assert ctx.fleet_plans(sl, start, goal, vt)["rc"] == 0               # the replan makes the fields the map's again
    finally:
        ctx.close()


@pytest.mark.parametrize("planner", ["cvp", "dijkstra"])
def test_walk_plans_equal_the_oracle(planner):
    W = Plain(meshgen.terrain(48, 0.1, 6))
    rng = np.random.default_rng(9)
    goals = [W.mesh.vertex_at(0.3, 0.35), W.mesh.vertex_at(0.7, 0.6), W.mesh.vertex_at(0.25, 0.7), W.mesh.vertex_at(0.6, 0.3)]
    robots_v = [W.mesh.vertex_at(0.75, 0.8), W.mesh.vertex_at(0.2, 0.25), W.mesh.vertex_at(0.8, 0.3), W.mesh.vertex_at(0.3, 0.8)]
    sp, sf = seed_ends(W, goals)
    tp, tf = seed_ends(W, robots_v)
    goal_pose = np.concatenate([sp.astype(np.float64), np.array([[0, 0, np.sin(0.1 * k), np.cos(0.1 * k)] for k in range(4)])], axis=1)
    with capi.MnavContext(0) as ctx:
        W.case.upload(ctx)
        ctx.upload_face_normals(W.case.fn)
        ctx.set_resident_outputs(True)
        if planner == "cvp":
            b = ctx.plan_cvp_batch(sp, sf, tf, 1e9)
            refs = [W.om.cvp(W.case.weights, W.case.costs, W.case.vn, sp[k], int(sf[k]), int(tf[k]), 1e9) for k in range(4)]
            assert list(b["codes"]) == [r.code for r in refs] == [0] * 4
            maps = [(r.vecmap, r.has_vec) for r in refs]
        else:
            ctx.plan_dijkstra_batch(goals, robots_v, 1e9)
            refs = [W.om.dijkstra(W.case.weights, W.case.costs, goals[k], robots_v[k], 1e9) for k in range(4)]
            vms = [W.om.dijkstra_vector_map(r.pred) for r in refs]
            maps = [(vm, (vm != 0).any(axis=1).astype(np.uint8)) for vm in vms]
        n = 64                                                                # 4 plans x 16 robots
        slots = (np.arange(n) % 4).astype(np.uint32)
        pos, face = walk_robots(W, rng, n)
        pos[5] = W.mesh.xyz[0] + np.array([-3.0, -3.0, 0.0], np.float32)      # beside the mesh: no face, no poses
        face[5] = capi.NONE
        kw = dict(step_width=0.15, walk_cap=4096)
        walks = ctx.fleet_walks(slots, sp, sf, pos, face, **kw)
        check_walks(walks, W, maps, sp, sf, slots, pos, face, 0.15, 4096, planner)    # the rows are the oracle's ...
        rows = [(walks["positions"][int(walks["offsets"][i]): int(walks["offsets"][i + 1])], walks["faces"][int(walks["offsets"][i]): int(walks["offsets"][i + 1])])
                for i in range(n)]
        want = PM.walk_run(W.om, W.case.fn, rows, slots, goal_pose)                     # ... and their poses OracleMesh.cvp_poses
        out = ctx.fleet_walk_plans(slots, sp, sf, goal_pose, pos, face, **kw)
        st = ctx.fleet_stats()

        def same(o, where):
            for k in ("status", "start_face", "path_len", "offsets"):
                assert np.array_equal(o[k], walks[k]), (where, k)
            assert np.array_equal(o["path_len"], want["path_len"]) and np.array_equal(o["offsets"], want["offsets"]), where
            assert np.array_equal(PM.bits64(o["cost"]), PM.bits64(want["cost"])), where
            assert PM.same_poses(o["poses"], want["poses"], where) == 0

        same(out, planner)
        failed = int(((walks["status"] != 1) & (walks["path_len"] > 0)).sum())
        print(planner, "poses", out["total"], "reached", int((walks["status"] == 1).sum()), "partial rows", failed, st)
        assert out["rc"] == 0 and out["total"] == walks["total"] == st["entries"] and st["chunks"] == 1 and (walks["status"] == 1).sum() >= 10
        ends = out["offsets"][1:][out["path_len"] > 0].astype(np.int64) - 1
        assert np.array_equal(PM.bits64(out["poses"][ends]), PM.bits64(goal_pose[slots[out["path_len"] > 0]]))   # the goal pose verbatim
        ctx.set_option("fleet_scratch_mb", 1)                               # rows of 4096 entries take 64 KiB: 16 rows per MiB, 4 chunks
        chunked = ctx.fleet_walk_plans(slots, sp, sf, goal_pose, pos, face, **kw)
        assert ctx.fleet_stats()["chunks"] == 4 and ctx.fleet_stats()["entries"] == out["total"]
        ctx.set_option("fleet_scratch_mb", None)
        same(chunked, planner + " chunked")
        # a walk_cap that is hit: the partial rows are posed too
        w16 = ctx.fleet_walks(slots, sp, sf, pos, face, step_width=0.05, walk_cap=16)
        rows16 = [(w16["positions"][int(w16["offsets"][i]): int(w16["offsets"][i + 1])], w16["faces"][int(w16["offsets"][i]): int(w16["offsets"][i + 1])]) for i in range(n)]
        want16 = PM.walk_run(W.om, W.case.fn, rows16, slots, goal_pose)
        out16 = ctx.fleet_walk_plans(slots, sp, sf, goal_pose, pos, face, step_width=0.05, walk_cap=16)
        assert ((out16["status"] == 0) & (out16["path_len"] == 16)).sum() >= 10
        assert np.array_equal(out16["offsets"], want16["offsets"]) and np.array_equal(PM.bits64(out16["cost"]), PM.bits64(want16["cost"]))
        assert PM.same_poses(out16["poses"], want16["poses"], "cap 16") == 0
        small = ctx.fleet_walk_plans(slots, sp, sf, goal_pose, pos, face, poses_cap=out["total"] - 1, **kw)
        assert small["rc"] == 1 and small["total"] == out["total"] and small["poses"] is None and np.array_equal(PM.bits64(small["cost"]), PM.bits64(want["cost"]))
        with pytest.raises(RuntimeError):
            ctx.fleet_walk_plans(slots, sp, sf, None, pos, face, **kw)       # no goal poses


def test_other_entry_points_are_left_alone(world):
    W = world
    ctx = make_ctx(W)
    try:
        seeds, targets = W.seeds[:4], W.targets[:4]
        ctx.plan_dijkstra_batch(seeds, targets, OFFSET, LIMIT)
        ctx.upload_face_normals(W.case.fn)
        n = 64
        rng = np.random.default_rng(2)
        slots = (np.arange(n) % 4).astype(np.uint32)
        v = rng.integers(0, W.V, n)
        pos = (W.mesh.xyz[v] + np.array([0.031, 0.017, 0.0], np.float32)).astype(np.float32)
        heading = np.tile(np.array([1, 0, 0], np.float32), (n, 1))
        up = np.tile(np.array([0, 0, 1], np.float32), (n, 1))
        sp, sf = seed_ends(W, seeds)
        goal_pose = np.concatenate([sp.astype(np.float64), np.tile([0.0, 0, 0, 1], (4, 1))], axis=1)

        def others():
            f = ctx.follow(pos, heading, up, np.full(n, capi.NONE, np.uint32), slots)
            fs = ctx.follow_stats()
            d = [ctx.download_output(w, k) for k in range(4) for w in ("dist", "pred", "vecmap")]
            p = ctx.fleet_paths(slots, None, pos)
            w = ctx.fleet_walks(slots, sp, sf, pos, None, step_width=0.2, walk_cap=256)
            return f, {k: fs[k] for k in fs if not k.startswith("ms")}, d, p, w

        ctx.locate(pos[:1])                                                 # (the lookup index exists: no call below builds it)
        f0, fs0, d0, p0, w0 = others()
        a = ctx.fleet_plans(slots, pos, sp, None)
        c = ctx.fleet_walk_plans(slots, sp, sf, goal_pose, pos, None, step_width=0.2, walk_cap=256)
        assert a["rc"] == 0 and c["rc"] == 0 and a["total"] > 100 and c["total"] > 100
        assert np.array_equal(a["codes"], p0["codes"]) and np.array_equal(bits(a["potential"]), bits(p0["potential"])) and np.array_equal(a["vertex"], p0["vertex"])
        assert np.array_equal(c["status"], w0["status"]) and np.array_equal(c["path_len"], w0["path_len"])
        f1, fs1, d1, p1, w1 = others()
        for k in capi.FollowOut.__dataclass_fields__:
            assert np.array_equal(getattr(f0, k).view(np.uint8), getattr(f1, k).view(np.uint8)), k
        assert fs0 == fs1
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(d0, d1))
        for k in ("codes", "vertex", "potential", "path_len", "offsets", "ids"):
            assert np.array_equal(p0[k].view(np.uint8), p1[k].view(np.uint8)), k
        for k in ("status", "start_face", "path_len", "offsets", "positions", "faces"):
            assert np.array_equal(w0[k].view(np.uint8), w1[k].view(np.uint8)), k
        r = ctx.replan_dijkstra(None, OFFSET, want_dist=True, want_pred=True)   # the plan outputs of the recorded call
        assert r["replan"]["reason"] == 0 and r["replan"]["log_len"] == 0
        assert all(np.array_equal(r["pred"][k], d0[3 * k + 1]) and np.array_equal(bits(r["dist"][k]), bits(d0[3 * k])) for k in range(4))
        W.upload(ctx)                                                       # mnav_upload_mesh drops the face normals
        ctx.plan_dijkstra_batch(seeds, targets, OFFSET, LIMIT)
        with pytest.raises(RuntimeError, match="face normals"):
            ctx.fleet_walk_plans(slots, sp, sf, goal_pose, pos, None, step_width=0.2, walk_cap=256)
    finally:
        ctx.close()


def test_adapter_fleet_plans_equal_make_plan():
    """DijkstraMeshPlanner::makeFleetPlans for 32 start poses against 32 makePlan calls through the same adapter (the host
    pose loop of mnav_planner_host.hpp): codes, poses and costs bit for bit, MNAV_BEYOND_FIELD robots excluded"""
    case = Case(meshgen.terrain(48, 0.1, 6))
    m = case.mesh
    mm = dict(xyz=m.xyz, faces=m.faces, edges=m.edges, vertex_normals=case.vn, face_normals=case.fn, vertex_costs=case.costs, edge_weights=case.weights, invalid=None)
    pose = lambda p: np.array([p[0], p[1], p[2], 0, 0, 0, 1], np.float64)
    robot = m.xyz[m.vertex_at(0.85, 0.8)] + np.array([0.031, 0.017, 0.05], np.float32)
    goal = m.xyz[m.vertex_at(0.12, 0.2)] + np.array([0.023, 0.011, 0.02], np.float32)
    rng = np.random.default_rng(8)
    # starts inside the first plan's cut: between the goal and the robot (the wave from the goal has passed them)
    t = rng.uniform(0.05, 0.8, 32)[:, None]
    starts = (goal[None] * (1 - t) + robot[None] * t + rng.uniform(-0.2, 0.2, (32, 3)) * np.array([1, 1, 0])).astype(np.float32)
    starts[:, 2] = [m.xyz[case.om.nearest_vertex(p)][2] + 0.03 for p in starts]
    start_poses = np.array([pose(p) for p in starts])
    fleet, single = DijkstraMeshPlanner(), DijkstraMeshPlanner()
    try:
        assert fleet.initialize("dijkstra_mesh_planner", mm) and single.initialize("dijkstra_mesh_planner", mm)
        code, plan, cost, _ = fleet.makePlan(pose(robot), pose(goal))
        assert code == 0 and len(plan) > 10
        rc, codes, plans, costs, msg = fleet.makeFleetPlans(start_poses)
        assert rc == 0, msg
        beyond = codes == capi.BEYOND_FIELD
        print("adapter: beyond the field", int(beyond.sum()), "of 32; poses", sum(len(p) for p in plans))
        assert beyond.sum() <= 8                                            # at most a quarter
        for i in np.flatnonzero(~beyond):
            c1, p1, k1, _ = single.makePlan(start_poses[i], pose(goal))
            assert c1 == codes[i], (i, c1, codes[i])
            assert PM.same_poses(plans[i], p1, ("adapter", i)) == 0 and PM.bits64(costs[i]) == PM.bits64(k1), i
        # the plan's own robot out of its own field
        rc, codes, plans, costs, _ = fleet.makeFleetPlans(pose(robot)[None])
        assert rc == 0 and codes[0] == 0 and PM.same_poses(plans[0], plan, "own") == 0 and PM.bits64(costs[0]) == PM.bits64(cost)
    finally:
        fleet.close()
        single.close()
