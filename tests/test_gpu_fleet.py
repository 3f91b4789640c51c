"""GPU: fleet paths and fleet walks (mnav_fleet_paths, mnav_fleet_walks, mnav_fleet_stats).

Paths: every robot's code, ids, potential and offset equal a fresh plan of the CPU oracle from the plan's seed to the
robot's vertex (same offset, cost_limit and invalid mask), or the MNAV_BEYOND_FIELD of tests/fleet_model.py (which
tests/test_fleet_model.py pins on the CPU), over the fields left by the tile rounds, the asynchronous engine, the
tile-batch engine and a replan after a cost update.  Walks: statuses, faces and position bits equal
OracleMesh.cvp_backtrack on the oracle's field.

Shapes: terrain(48) = 2304 vertices (terrain(44) = 1936 for the inflation walk), 8 plans, up to 3000 robots."""
import ctypes as C

import numpy as np
import pytest

from mesh_navigation_amd import capi, meshgen
from oracle import oracle as O
from tests import fleet_model as FM
from tests.common import Case
from tests.fleet_model import bits

pytestmark = pytest.mark.gpu
LIMIT, OFFSET = 0.8, 0.3
SENTINEL = 0xDEADBEEF


class World:
    """terrain(48) with random costs (some above the limit), computed weights and an invalid mask; 6 plans that run, one
    whose seed is its target and one with a target id out of range"""

    def __init__(self):
        self.mesh = meshgen.terrain(48, 0.1, 6)
        V = self.V = self.mesh.V
        rng = np.random.default_rng(17)
        self.costs = rng.random(V).astype(np.float32)
        self.invalid = (rng.random(V) < 0.02).astype(np.uint8)
        self.case = Case(self.mesh, self.costs, 1.0, self.invalid)
        self.om = self.case.om
        self.weights = self.case.weights
        ok = np.flatnonzero((self.costs <= LIMIT) & (self.invalid == 0))
        pick = rng.choice(ok, 13, replace=False)
        self.seeds = np.array(list(pick[:6]) + [pick[12], pick[11]], np.uint32)
        self.targets = np.array(list(pick[6:12]) + [pick[12], V + 5], np.uint32)
        self.version = 0
        self._fresh = {}

    def upload(self, ctx):
        ctx.upload_mesh(self.mesh.xyz, self.mesh.faces, self.mesh.edges, self.case.vn)
        ctx.compute_edge_weights(self.costs, self.case.edge_dist, 1.0, self.invalid)

    def change_costs(self, ctx, ids, value):
        """mnav_update_costs on the context and on the model's state"""
        self.costs = self.costs.copy()
        self.costs[ids] = value
        self.weights = self.om.edge_weights(self.case.edge_dist, self.costs, 1.0)
        self.version += 1
        ctx.update_costs(np.asarray(ids, np.uint32), np.full(len(ids), value, np.float32))

    def fresh(self, seed, v, offset=OFFSET):
        """the oracle's plan from seed to v on the present costs, computed once"""
        key = (self.version, int(seed), int(v), offset)
        if key not in self._fresh:
            self._fresh[key] = self.om.dijkstra(self.weights, self.costs, int(seed), int(v), offset, LIMIT, self.invalid)
        return self._fresh[key]

    def fields(self, targets=None, offset=OFFSET):
        """the plans of the batch as the model sees them (the oracle's fields of the plans that run)"""
        t = self.targets if targets is None else targets
        out = []
        for s, g in zip(self.seeds, t):
            code = FM.plan_code(int(s), int(g), self.V)
            if code != FM.SUCCESS or s == g:
                out.append(FM.Field(None, None, int(s), int(g), offset, code))
            else:
                r = self.fresh(s, g, offset)
                out.append(FM.Field(r.dist, r.pred, int(s), int(g), offset))
        return out


@pytest.fixture(scope="module")
def world():
    return World()


def make_ctx(W):
    ctx = capi.MnavContext(0)
    W.upload(ctx)
    ctx.set_resident_outputs(True)
    return ctx


def robots(W, fields, n, seed):
    """n robots spread over the plans: random vertices, plus every plan's seed, target, ring and far vertices and ids out
    of range when there is room for them"""
    rng = np.random.default_rng(seed)
    slots = (np.arange(n) % len(fields)).astype(np.uint32)
    vtx = rng.integers(0, W.V, n).astype(np.uint32)
    if n >= 64:
        k = 0
        for s, f in enumerate(fields):
            special = [f.seed, f.target, W.V, FM.NONE] + ([] if f.dist is None else list(FM.robots_of(f, W.V, rng, 0)))
            for v in special[: max(1, (n // 2) // len(fields))]:
                slots[k], vtx[k] = s, min(int(v), FM.NONE)
                k += 1
    return slots, vtx


def check_paths(ctx, W, fields, slots, vtx, where, start_pos=None, want_vertex=None):
    out = ctx.fleet_paths(slots, None if start_pos is not None else vtx, start_pos)
    stats = ctx.fleet_stats()
    n = len(slots)
    if want_vertex is not None:
        assert np.array_equal(out["vertex"], want_vertex), where
        vtx = want_vertex
    else:
        assert np.array_equal(out["vertex"], vtx), where
    want = FM.run(fields, W.V, slots, vtx)
    print(where, "n", n, "served / beyond / no path / invalid", want["counts"], "ids", want["ids"].size, "ms kernels %.3f total %.3f" % (stats["ms_kernels"], stats["ms_total"]))
    assert out["rc"] == 0 and out["total"] == want["ids"].size, (where, out["rc"], out["total"])
    assert np.array_equal(out["codes"], want["codes"]), (where, np.flatnonzero(out["codes"] != want["codes"])[:8])
    assert np.array_equal(out["path_len"], want["path_len"]) and np.array_equal(out["offsets"], want["offsets"]), where
    assert np.array_equal(out["ids"], want["ids"]), where
    assert np.array_equal(bits(out["potential"]), bits(want["potential"])), where
    assert [stats[k] for k in ("served", "beyond_field", "no_path", "invalid")] == want["counts"] and stats["entries"] == want["ids"].size, (where, stats)
    # ... and, whatever the model says: a served robot has the fresh plan's code, path and potential
    checked = 0
    for i in range(n):
        f, v, code = fields[int(slots[i])], int(vtx[i]), int(out["codes"][i])
        if f.dist is None or v >= W.V or code == FM.BEYOND_FIELD:
            continue
        r = W.fresh(f.seed, v, f.offset)
        assert code == r.code, (where, i, code, r.code)
        lo = int(out["offsets"][i])
        assert np.array_equal(out["ids"][lo: lo + int(out["path_len"][i])], r.path), (where, i)
        if v != f.seed:
            assert bits(out["potential"][i]) == bits(r.dist[v]), (where, i)
        checked += 1
    return want, checked


@pytest.mark.parametrize("source", ["tiled", "async", "tile_batch"])
def test_paths_equal_fresh_plans(world, source):
    W = world
    ctx = make_ctx(W)
    try:
        ctx.set_dijkstra_engine(source)
        b = ctx.plan_dijkstra_batch(W.seeds, W.targets, OFFSET, LIMIT, want_fields=True)
        assert {"tiled": "k_tile_round", "async": "k_plan_async", "tile_batch": "k_tb"}[source] in ctx.last_engine(), ctx.last_engine()
        fields = W.fields()
        assert list(b["codes"][6:]) == [FM.SUCCESS, FM.INVALID_GOAL]
        for k in range(6):
            assert np.array_equal(b["pred"][k], fields[k].pred) and np.array_equal(bits(b["dist"][k]), bits(fields[k].dist)), (source, k)
        for n in (1, 64, 65, 3000):
            sl, vt = robots(W, fields, n, 10 + n)
            want, checked = check_paths(ctx, W, fields, sl, vt, (source, n))
        served, beyond, no_path, invalid = want["counts"]
        assert served >= 100 and beyond >= 100 and invalid >= 20 and checked >= 1000, (want["counts"], checked)   # many robots per plan, every rule
    finally:
        ctx.close()


def test_paths_after_a_replan(world):
    """mnav_update_costs makes the fields stale (refused), mnav_replan_dijkstra_batch makes them the map's again"""
    W = world
    ctx = make_ctx(W)
    seeds, targets = W.seeds[:6], W.targets[:6].copy()                     # (a plan that never reaches the device makes a replan plan afresh)
    old = W.costs
    try:
        ctx.set_option("replan_fresh_below", 0)
        ctx.plan_dijkstra_batch(seeds, targets, OFFSET, LIMIT)
        ids = np.array([W.mesh.vertex_at(0.5, 0.5), W.mesh.vertex_at(0.52, 0.5), int(targets[0])], np.uint32)
        ids = ids[~np.isin(ids, seeds)]
        W.change_costs(ctx, ids, 0.45)
        with pytest.raises(RuntimeError):
            ctx.fleet_paths(np.zeros(1, np.uint32), targets[:1])
        moved = W.mesh.vertex_at(0.3, 0.7)
        if moved != seeds[1]:
            targets[1] = moved
        b = ctx.replan_dijkstra(targets, OFFSET, want_dist=True, want_pred=True)
        print("replan", {k: v for k, v in b["replan"].items() if k != "levels"})
        assert b["replan"]["reason"] == 0 and b["replan"]["log_len"] == ids.size
        fields = W.fields(targets)
        assert all(np.array_equal(b["pred"][k], fields[k].pred) for k in range(6))
        for n in (1, 65, 3000):
            sl, vt = robots(W, fields, n, 40 + n)
            want, checked = check_paths(ctx, W, fields, sl, vt, ("replan", n))
        assert want["counts"][0] >= 100 and want["counts"][1] >= 100 and checked >= 1000
    finally:
        ctx.close()
        W.costs = old
        W.weights = W.om.edge_weights(W.case.edge_dist, W.costs, 1.0)
        W.version += 1


def test_a_wave_that_ran_out_leaves_nobody_beyond_the_field(world):
    """offset 1e9: the cut is finite, but no reached vertex lies at or above it -- rule 5 through k_fleet_open: the
    robots on vertices the wave cannot reach get the fresh plan's MNAV_NO_PATH_FOUND"""
    W = world
    ctx = make_ctx(W)
    try:
        seeds, targets = W.seeds[:6], W.targets[:6].copy()
        targets[5] = np.flatnonzero(W.invalid)[0]                           # a robot vertex no wave reaches: that plan's cut is +inf
        b = ctx.plan_dijkstra_batch(seeds, targets, 1e9, LIMIT)
        assert list(b["codes"]) == [0] * 5 + [FM.NO_PATH_FOUND]
        fields = W.fields(targets, 1e9)
        for n in (65, 3000):
            sl, vt = robots(W, fields, n, 70 + n)
            want, checked = check_paths(ctx, W, fields, sl, vt, ("ran out", n))
        served, beyond, no_path, invalid = want["counts"]
        assert beyond == 0 and no_path >= 20 and served >= 2000, want["counts"]
    finally:
        ctx.close()


def test_paths_from_positions_and_the_sizing_protocol(world):
    W = world
    ctx = make_ctx(W)
    try:
        ctx.plan_dijkstra_batch(W.seeds, W.targets, OFFSET, LIMIT, want_fields=False)          # (resident outputs: not a paths-only call)
        fields = W.fields()
        rng = np.random.default_rng(3)
        n = 300
        slots = (np.arange(n) % 6).astype(np.uint32)
        v = rng.integers(0, W.V, n)
        pos = (W.mesh.xyz[v] + rng.uniform(-0.04, 0.04, (n, 3)).astype(np.float32) * np.array([1, 1, 0.2], np.float32)).astype(np.float32)
        nearest = np.array([W.om.nearest_vertex(p) for p in pos], np.uint32)
        assert ctx.locate_stats()["built"] == 0
        one = ctx.fleet_paths(slots[:1], None, pos[:1], ids_cap=W.V)          # (one C call: the first with positions builds the lookup index)
        assert one["rc"] == 0 and ctx.fleet_stats()["built_index"] == 1 and ctx.locate_stats()["built"] == 1
        check_paths(ctx, W, fields, slots, None, "positions", start_pos=pos, want_vertex=nearest)
        check_paths(ctx, W, fields, slots[:65], None, "positions 65", start_pos=pos[:65], want_vertex=nearest[:65])
        assert ctx.fleet_stats()["built_index"] == 0
        # the two-call protocol, by hand: too small a buffer leaves it untouched and reports the size
        full = ctx.fleet_paths(slots, nearest)
        total = full["total"]
        assert total > 100
        L, h = ctx._L, ctx._h
        codes, lens, off, tot = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64), C.c_uint64(0)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        for cap, ids in ((total - 1, np.full(total, SENTINEL, np.uint32)), (0, None)):
            rc = L.mnav_fleet_paths(h, n, p(slots), p(nearest), None, p(codes), None, None, p(lens), p(off), None if ids is None else p(ids), cap, C.byref(tot))
            assert rc == 1 and tot.value == total and (ids is None or (ids == SENTINEL).all())
            assert np.array_equal(codes, full["codes"]) and np.array_equal(lens, full["path_len"]) and np.array_equal(off, full["offsets"])
        ids = np.full(total + 7, SENTINEL, np.uint32)
        assert L.mnav_fleet_paths(h, n, p(slots), p(nearest), None, None, None, None, None, None, p(ids), total + 7, None) == 0
        assert np.array_equal(ids[:total], full["ids"]) and (ids[total:] == SENTINEL).all()
        assert L.mnav_fleet_paths(h, 0, None, None, None, None, None, None, None, None, None, 0, None) == 0   # n = 0 does nothing
    finally:
        ctx.close()


def raw_paths(ctx, slots, vtx):
    """the C call with sentinel-filled outputs: (rc, every output array)"""
    n = len(slots)
    sl, vt = np.ascontiguousarray(slots, np.uint32), np.ascontiguousarray(vtx, np.uint32)
    outs = [np.full(n, SENTINEL, np.uint32) for _ in range(3)] + [np.full(n, np.nan, np.float32), np.full(n + 1, SENTINEL, np.uint64), np.full(64, SENTINEL, np.uint32)]
    code, vout, lens, pot, off, ids = outs
    tot = C.c_uint64(SENTINEL)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = ctx._L.mnav_fleet_paths(ctx._h, n, p(sl), p(vt), None, p(code), p(vout), p(pot), p(lens), p(off), p(ids), 64, C.byref(tot))
    untouched = all((a == SENTINEL).all() for a in (code, vout, lens, off, ids)) and np.isnan(pot).all() and tot.value == SENTINEL
    return rc, untouched


def test_refusals_touch_nothing(world):
    W = world
    ctx = make_ctx(W)
    try:
        seeds, targets = W.seeds[:3], W.targets[:3]
        sl, vt = np.zeros(4, np.uint32), np.array(list(targets) + [5], np.uint32)

        def refused(what):
            rc, untouched = raw_paths(ctx, sl, vt)
            assert rc == -1 and untouched and ctx._err(), (what, rc, untouched, ctx._err())
            print(what, "->", ctx._err())

        refused("no plan yet")
        # resident fields, then the refusals that leave them as they are
        a = ctx.plan_dijkstra_batch(seeds, targets, OFFSET, LIMIT, want_fields=True)
        keep = [(ctx.download_output("dist", k), ctx.download_output("pred", k), ctx.download_output("vecmap", k)) for k in range(3)]
        ok = ctx.fleet_paths(sl, vt)
        assert ok["rc"] == 0 and ok["codes"][0] == FM.SUCCESS
        sl[3] = 3
        refused("a slot that is not a plan of the last call")
        sl[3] = 0
        with pytest.raises(RuntimeError):
            ctx.fleet_paths(sl)                                              # neither vertices nor positions
        W_costs = W.costs[int(targets[0])]
        ctx.update_costs(np.array([targets[0]], np.uint32), np.array([W_costs], np.float32))   # (the same value: the map stays, the log does not)
        refused("update_costs without a replan")
        for k in range(3):
            for x, y in zip(keep[k], (ctx.download_output("dist", k), ctx.download_output("pred", k), ctx.download_output("vecmap", k))):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), k
        r = ctx.replan_dijkstra(None, OFFSET)
        assert ctx.fleet_paths(sl, vt)["rc"] == 0                            # the replan makes the fields the map's again
        # a paths-only batch: no predecessors are resident
        ctx.set_resident_outputs(False)
        ctx.plan_dijkstra_batch(seeds, targets, OFFSET, LIMIT, want_fields=False)
        assert not ctx.device_output(0, 1)
        refused("after a paths-only batch")
        ctx.set_resident_outputs(True)
        # a CVP call
        goal = W.mesh.xyz[int(seeds[0])] + np.array([0.02, 0.03, 0.0], np.float32)
        gf, _ = W.om.containing_face(goal)
        tf, _ = W.om.containing_face(W.mesh.xyz[int(targets[0])] + np.array([0.02, 0.03, 0.0], np.float32))
        ctx.plan_cvp_batch([goal], [gf], [tf], OFFSET, LIMIT)
        cvp = ctx.download_output("dist", 0)
        refused("after a CVP call")
        assert np.array_equal(ctx.download_output("dist", 0).view(np.uint32), cvp.view(np.uint32))
    finally:
        ctx.close()


# -- walks ------------------------------------------------------------------------------------------------------------
class Plain:
    """a mesh with uniform costs: the walks are about the field, not the costs"""

    def __init__(self, mesh):
        self.mesh, self.V = mesh, mesh.V
        self.case = Case(mesh)
        self.om = self.case.om


def walk_robots(W, rng, n):
    """start positions as the back-tracking tests make them: a vertex plus a small in-plane offset, with its face"""
    v = rng.integers(0, W.V, n)
    pos = (W.mesh.xyz[v] + np.array([0.031, 0.017, 0.0], np.float32)).astype(np.float32)
    face = np.array([W.om.containing_face(p)[0] for p in pos], np.int64)
    face = np.where((face >= 0) & (face < W.mesh.F), face, capi.NONE).astype(np.uint32)
    return pos, face


def check_walks(out, W, maps, seed_pos, seed_faces, slots, pos, face, sw, cap, where, inflation_field=None):
    n = len(slots)
    assert np.array_equal(out["start_face"], face), where
    tally = {}
    for i in range(n):
        lo, m, st = int(out["offsets"][i]), int(out["path_len"][i]), int(out["status"][i])
        tally[st] = tally.get(st, 0) + 1
        assert int(out["offsets"][i + 1]) == lo + m
        if face[i] == capi.NONE:
            assert (st, m) == (capi.WALK_NO_FACE, 0), (where, i)
            continue
        s = int(slots[i])
        if maps[s] is None:
            assert (st, m) == (0, 0), (where, i)
            continue
        vm, hv = maps[s]
        rc, ppos, pface = W.om.cvp_backtrack(vm, hv, seed_pos[s], int(seed_faces[s]), pos[i], int(face[i]), step_width=sw, cap=cap, inflation_field=inflation_field)
        assert (st == 1) == (rc == 0), (where, i, st, rc)
        assert np.array_equal(out["faces"][lo: lo + m], pface), (where, i)
        assert np.array_equal(out["positions"][lo: lo + m].view(np.uint32), ppos.view(np.uint32)), (where, i)
    assert int(out["offsets"][n]) == out["total"] == len(out["faces"])
    return tally


def seed_ends(W, vertices):
    sp = (W.mesh.xyz[np.asarray(vertices, np.int64)] + np.array([0.023, 0.011, 0.0], np.float32)).astype(np.float32)
    sf = np.array([W.om.containing_face(p)[0] for p in sp], np.uint32)
    return sp, sf


@pytest.mark.parametrize("planner", ["cvp", "dijkstra"])
def test_walks_equal_the_oracle(planner):
    W = Plain(meshgen.terrain(48, 0.1, 6))
    rng = np.random.default_rng(9)
    goals = [W.mesh.vertex_at(0.3, 0.35), W.mesh.vertex_at(0.7, 0.6)]
    robots_v = [W.mesh.vertex_at(0.75, 0.8), W.mesh.vertex_at(0.2, 0.25)]
    sp, sf = seed_ends(W, goals)
    tp, tf = seed_ends(W, robots_v)
    with capi.MnavContext(0) as ctx:
        W.case.upload(ctx)
        ctx.set_resident_outputs(True)
        if planner == "cvp":
            b = ctx.plan_cvp_batch(sp, sf, tf, OFFSET)
            refs = [W.om.cvp(W.case.weights, W.case.costs, W.case.vn, sp[k], int(sf[k]), int(tf[k]), OFFSET) for k in range(2)]
            assert list(b["codes"]) == [r.code for r in refs] == [0, 0]
            maps = [(r.vecmap, r.has_vec) for r in refs]
        else:
            b = ctx.plan_dijkstra_batch(goals, robots_v, OFFSET)
            refs = [W.om.dijkstra(W.case.weights, W.case.costs, goals[k], robots_v[k], OFFSET) for k in range(2)]
            vms = [W.om.dijkstra_vector_map(r.pred) for r in refs]
            maps = [(vm, (vm != 0).any(axis=1).astype(np.uint8)) for vm in vms]
        n = 80                                                                # 40 robots per plan
        slots = (np.arange(n) % 2).astype(np.uint32)
        pos, face = walk_robots(W, rng, n)
        pos[5] = W.mesh.xyz[0] + np.array([-3.0, -3.0, 0.0], np.float32)      # beside the mesh: no face
        face[5] = capi.NONE
        assert (face != capi.NONE).sum() >= 60
        before = [ctx.download_output("vecmap", k) for k in range(2)]
        out = ctx.fleet_walks(slots, sp, sf, pos, face, step_width=0.15, walk_cap=4096)
        st = ctx.fleet_stats()
        tally = check_walks(out, W, maps, sp, sf, slots, pos, face, 0.15, 4096, planner)
        print(planner, "statuses", tally, "entries", out["total"], st)
        no_face = int((face == capi.NONE).sum())                            # robot 5, and the starts whose offset left the mesh at its border
        assert tally.get(1, 0) >= 10 and tally.get(capi.WALK_NO_FACE, 0) == no_face >= 1 and out["status"][5] == capi.WALK_NO_FACE and st["chunks"] == 1
        assert (st["served"], st["invalid"], st["entries"]) == (tally.get(1, 0), no_face, out["total"]) and st["served"] + st["no_path"] + st["invalid"] == n
        # the faces found on the device (the rule of mnav_locate) instead of given ones
        out_l = ctx.fleet_walks(slots, sp, sf, pos, None, step_width=0.15, walk_cap=4096)
        for k in ("status", "start_face", "path_len", "offsets", "faces"):
            assert np.array_equal(out_l[k], out[k]), k
        assert np.array_equal(out_l["positions"].view(np.uint32), out["positions"].view(np.uint32))
        # at least three chunks give the same output (rows of 4096 entries take 64 KiB: 16 rows per MiB)
        ctx.set_option("fleet_scratch_mb", 1)
        out_c = ctx.fleet_walks(slots, sp, sf, pos, face, step_width=0.15, walk_cap=4096)
        assert ctx.fleet_stats()["chunks"] == 5
        ctx.set_option("fleet_scratch_mb", None)
        for k in ("status", "start_face", "path_len", "offsets", "faces"):
            assert np.array_equal(out_c[k], out[k]), k
        assert np.array_equal(out_c["positions"].view(np.uint32), out["positions"].view(np.uint32))
        # a walk_cap of 16 that is hit: status 0 with the 16 entries walked, as the oracle's guard
        out16 = ctx.fleet_walks(slots, sp, sf, pos, face, step_width=0.05, walk_cap=16)
        t16 = check_walks(out16, W, maps, sp, sf, slots, pos, face, 0.05, 16, planner + " cap 16")
        assert (out16["path_len"] == 16).sum() >= 10 and t16.get(0, 0) >= 10, t16
        # the sizing protocol: too small a buffer reports the size
        small = ctx.fleet_walks(slots, sp, sf, pos, face, step_width=0.15, walk_cap=4096, entries_cap=out["total"] - 1)
        assert small["rc"] == 1 and small["total"] == out["total"] and small["positions"] is None and np.array_equal(small["path_len"], out["path_len"])
        # refusals
        for bad in (dict(walk_cap=1), dict(step_width=0.0), dict(inflation_layer=0)):
            with pytest.raises(RuntimeError):
                ctx.fleet_walks(slots, sp, sf, pos, face, **{**dict(step_width=0.15, walk_cap=64), **bad})
        with pytest.raises(RuntimeError):
            ctx.fleet_walks(slots + 1, sp, sf, pos, face, step_width=0.15, walk_cap=64)      # slot 2 of 2 plans
        with pytest.raises(RuntimeError):
            ctx.fleet_walks(slots[:4], sp[:1], sf[:1], pos[:4], face[:4], step_width=0.15, walk_cap=64)   # n_plans differs from the last call
        for k in range(2):
            assert np.array_equal(ctx.download_output("vecmap", k).view(np.uint32), before[k].view(np.uint32))
        if planner == "cvp":
            # one robot per plan at the plan's own target: the call agrees with backtrack_cvp_batch
            old = ctx.backtrack_cvp_batch(sp, sf, tp, tf, step_width=0.15)
            one = ctx.fleet_walks([0, 1], sp, sf, tp, tf, step_width=0.15, walk_cap=4096)
            for k, (st_k, pos_k, face_k) in enumerate(old):
                lo, m = int(one["offsets"][k]), int(one["path_len"][k])
                assert st_k == one["status"][k] and m == len(face_k) > 0
                assert np.array_equal(one["faces"][lo: lo + m], face_k) and np.array_equal(one["positions"][lo: lo + m].view(np.uint32), pos_k.view(np.uint32))


def test_walks_with_the_device_built_inflation_layer():
    """the set-up of tests/test_gpu_backtrack.py: a corridor between two lethal walls, the inflation layer computed on the device"""
    mesh = meshgen.terrain(44, 0.1, 12, amplitude=0.3)
    N = mesh.N
    lethal = np.zeros(mesh.V, np.uint8)
    i, j = np.meshgrid(np.arange(N), np.arange(N))
    lethal[(((j == 18) | (j == 25)) & (i > 3) & (i < N - 4)).ravel()] = 1
    W = Plain(mesh)
    case = W.case
    cfg = O.InflationCfg.defaults()
    icost, idist, ivec = case.om.inflation(lethal, case.edge_dist, cfg)
    goal = mesh.xyz[21 * N + 6] + np.array([0.02, 0.03, 0.0], np.float32)
    sf, _ = case.om.containing_face(goal)
    starts = np.array([mesh.xyz[22 * N + N - 8 - 3 * k] + np.array([0.03, 0.01, 0.0], np.float32) for k in range(6)], np.float32)
    faces = np.array([case.om.containing_face(p)[0] for p in starts], np.uint32)
    with capi.MnavContext(0) as ctx:
        ctx.upload_mesh(mesh.xyz, mesh.faces, mesh.edges, case.vn)
        ctx.layer_upload(0, np.zeros(mesh.V, np.float32), lethal)
        ctx.layer_inflation(1, 0)
        ctx.combine_layers([1], [1.0], mode="max", edge_cost_factor=1.0)
        vc, w = ctx.download_costs()
        ctx.set_resident_outputs(True)
        out = ctx.plan_cvp(goal, sf, int(faces[0]), want_fields=False, want_vecmap=False)
        got = ctx.fleet_walks(np.zeros(6, np.uint32), [goal], [sf], starts, faces, step_width=0.2, inflation_layer=1, walk_cap=4096)
    ref = case.om.cvp(w, vc, case.vn, goal, sf, int(faces[0]))
    assert out.code == ref.code == 0
    field = (np.where(np.isfinite(idist), idist, 0).astype(np.float32), ivec, cfg, True)
    tally = check_walks(got, W, [(ref.vecmap, ref.has_vec)], np.array([goal]), [sf], np.zeros(6, np.uint32), starts, faces, 0.2, 4096, "inflation", inflation_field=field)
    assert tally.get(1, 0) >= 1 and got["total"] > 10, tally


def test_other_entry_points_are_left_alone(world):
    W = world
    ctx = make_ctx(W)
    try:
        seeds, targets = W.seeds[:4], W.targets[:4]
        ctx.plan_dijkstra_batch(seeds, targets, OFFSET, LIMIT)
        n = 64
        rng = np.random.default_rng(2)
        slots = (np.arange(n) % 4).astype(np.uint32)
        v = rng.integers(0, W.V, n)
        pos = (W.mesh.xyz[v] + np.array([0.031, 0.017, 0.0], np.float32)).astype(np.float32)
        heading = np.tile(np.array([1, 0, 0], np.float32), (n, 1))
        up = np.tile(np.array([0, 0, 1], np.float32), (n, 1))

        def others():
            f = ctx.follow(pos, heading, up, np.full(n, capi.NONE, np.uint32), slots)
            fs = ctx.follow_stats()
            d = [ctx.download_output(w, k) for k in range(4) for w in ("dist", "pred", "vecmap")]
            return f, {k: fs[k] for k in fs if not k.startswith("ms")}, d

        ctx.locate(pos[:1])                                                 # (the lookup index exists: neither follower call builds it)
        f0, fs0, d0 = others()
        sp, sf = seed_ends(W, seeds)
        p = ctx.fleet_paths(slots, None, pos)
        w = ctx.fleet_walks(slots, sp, sf, pos, None, step_width=0.2, walk_cap=256)
        assert p["rc"] == 0 and w["rc"] == 0 and (p["codes"] == FM.SUCCESS).any() and (w["status"] == 1).any()
        f1, fs1, d1 = others()
        for k in capi.FollowOut.__dataclass_fields__:
            a, b = getattr(f0, k), getattr(f1, k)
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), k
        assert fs0 == fs1
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(d0, d1))
        # a replan after the fleet calls is the replan it would have been: the log is empty, the fields are kept
        r = ctx.replan_dijkstra(None, OFFSET, want_dist=True, want_pred=True)
        assert r["replan"]["reason"] == 0 and r["replan"]["log_len"] == 0
        assert all(np.array_equal(r["pred"][k], d0[3 * k + 1]) and np.array_equal(bits(r["dist"][k]), bits(d0[3 * k])) for k in range(4))
    finally:
        ctx.close()
