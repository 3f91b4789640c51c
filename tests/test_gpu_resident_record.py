"""What a caller sees of the outputs the last plan call left on the device, state by state: the rows of the table in
tests/test_resident_record.py (the record of csrc/mnav_resident.h on the CPU), seen from outside through the C ABI.  Per state:
which of dist / pred / vector map mnav_device_output hands out per plan, whether mnav_download_output serves them, whether the
follower and the fleet calls run or refuse and with which words, the reason of a replan, mnav_last_engine.

Only the Python API of capi.py is used, so the file runs unchanged against a library built before the record existed: its
expectations were read off that code and passed against it first.

Shapes: terrain(24) = 576 vertices (2 tiles), 3 Dijkstra plans, 2 CVP plans, 4 robots: nothing here depends on the size."""
import numpy as np
import pytest

from mesh_navigation_amd import capi, meshgen
from tests.common import Case

pytestmark = pytest.mark.gpu

OFFSET = 0.3
T3, F3 = (True, True, True), (False, False, False)
NOT_RESIDENT = "not a Dijkstra call or replan whose fields are resident"


class World:
    def __init__(self):
        self.mesh = m = meshgen.terrain(24, 0.1, 6)
        self.case = Case(m)
        at = m.vertex_at
        self.seeds = np.array([at(0.2, 0.2), at(0.8, 0.3), at(0.5, 0.8)], np.uint32)        # the goals: where the waves start
        self.targets = np.array([at(0.8, 0.8), at(0.2, 0.7), at(0.4, 0.2)], np.uint32)      # the robots of the plan call
        shift = np.array([0.02, 0.03, 0.0], np.float32)
        self.seed_pos = (m.xyz[self.seeds] + shift).astype(np.float32)
        self.seed_faces = np.array([self.case.om.containing_face(p)[0] for p in self.seed_pos], np.uint32)
        self.robot_pos = (m.xyz[self.targets] + shift).astype(np.float32)
        self.robot_faces = np.array([self.case.om.containing_face(p)[0] for p in self.robot_pos], np.uint32)
        assert (self.seed_faces < m.F).all() and (self.robot_faces < m.F).all()
        # 4 robots: one per plan on its plan's robot vertex, one more on plan 0
        self.slots = np.array([0, 1, 2, 0], np.uint32)
        self.vtx = np.array(list(self.targets) + [at(0.6, 0.6)], np.uint32)
        self.pos = (m.xyz[self.vtx] + shift).astype(np.float32)

    def context(self):
        ctx = capi.MnavContext(0)
        self.case.upload(ctx)
        return ctx


@pytest.fixture(scope="module")
def world():
    return World()


def seen(ctx, n):
    """per caller plan: does mnav_device_output hand out (dist, pred, vector map)?"""
    got = [tuple(bool(ctx.device_output(i, w)) for w in (0, 1, 4)) for i in range(n)]
    print("device_output", got, "engine", ctx.last_engine())
    return got


def refusal(call):
    """the words a call refuses with; None when it runs"""
    try:
        call()
    except RuntimeError as e:
        return str(e)
    return None


def downloads(ctx, slot):
    """which of dist, pred, vecmap, popped mnav_download_output serves for a plan"""
    return tuple(refusal(lambda: ctx.download_output(w, slot)) is None for w in ("dist", "pred", "vecmap", "popped"))


def follow(ctx, W, slots):
    n = len(slots)
    heading = np.tile(np.array([1, 0, 0], np.float32), (n, 1))
    up = np.tile(np.array([0, 0, 1], np.float32), (n, 1))
    return ctx.follow(W.pos[:n], heading, up, np.full(n, capi.NONE, np.uint32), slots)


def robot_calls(ctx, W, n_plans=3):
    """refusal (or None) of follow, fleet_paths, fleet_walks, fleet_costs for the 4 robots over n_plans plans"""
    got = dict(follow=refusal(lambda: follow(ctx, W, W.slots)),
               paths=refusal(lambda: ctx.fleet_paths(W.slots, W.vtx)),
               walks=refusal(lambda: ctx.fleet_walks(W.slots, W.seed_pos[:n_plans], W.seed_faces[:n_plans], W.pos, None, step_width=0.15, walk_cap=256)),
               costs=refusal(lambda: ctx.fleet_costs(W.vtx, m=n_plans)))
    print("robot calls", got)
    return got


def plan(ctx, W, fields, engine="auto", resident=True):
    ctx.set_resident_outputs(resident)
    ctx.set_dijkstra_engine(engine)
    out = ctx.plan_dijkstra_batch(W.seeds, W.targets, OFFSET, want_fields=fields)
    ctx.set_dijkstra_engine("auto")
    assert out["rc"] == 0 and list(out["codes"]) == [0, 0, 0]
    return out


def same_as_fresh(ctx, W, a, vecmaps):
    """the outputs of a replan and what it left on the device, bit for bit those of a fresh plan on a second context"""
    B = W.context()
    try:
        b = plan(B, W, True, resident=vecmaps)
        assert np.array_equal(a["codes"], b["codes"]) and np.array_equal(a["path_len"], b["path_len"])
        assert all(np.array_equal(a["paths"][i], b["paths"][i]) for i in range(3))
        assert np.array_equal(a["dist"].view(np.uint32), b["dist"].view(np.uint32)) and np.array_equal(a["pred"], b["pred"])
        for i in range(3):
            for w in ("dist", "pred") + (("vecmap",) if vecmaps else ()):
                assert np.array_equal(ctx.download_output(w, i).view(np.uint32), B.download_output(w, i).view(np.uint32)), (w, i)
    finally:
        B.close()


def replan(ctx):
    return ctx.replan_dijkstra(None, OFFSET, want_dist=True, want_pred=True)


def test_a_finalized_call_leaves_everything(world):
    W = world
    with W.context() as ctx:
        assert seen(ctx, 3) == [F3] * 3 and ctx.last_engine() == "none"      # before the first call
        assert "not a Dijkstra call" in robot_calls(ctx, W)["paths"]
        plan(ctx, W, True)
        assert "k_plan_async" in ctx.last_engine()
        assert seen(ctx, 4) == [T3] * 3 + [F3]                               # (plan 3 is not a plan of the call)
        assert all(downloads(ctx, i) == (True, True, True, True) for i in range(3))
        assert downloads(ctx, 3) == (False, False, False, False)
        assert robot_calls(ctx, W) == dict(follow=None, paths=None, walks=None, costs=None)
        a = replan(ctx)
        assert a["replan"]["reason"] == 0 and seen(ctx, 3) == [T3] * 3
        same_as_fresh(ctx, W, a, True)
        # a call that was not asked for vector maps hands out none, not an earlier call's either
        plan(ctx, W, True, resident=False)
        assert seen(ctx, 3) == [(True, True, False)] * 3 and downloads(ctx, 0) == (True, True, False, True)
        r = robot_calls(ctx, W)
        assert "vector map of slot 0 not resident" in r["follow"] and "vector map of slot 0 not resident" in r["walks"]
        assert r["paths"] is None and r["costs"] is None


@pytest.mark.parametrize("engine,name,reason", [("tiled", "k_tile_round", 0), ("tile_batch", "k_tb", 1)])
def test_a_paths_only_call_leaves_paths(world, engine, name, reason):
    """No dist, pred or vector map is handed out; the popped potential is served.  The tile rounds leave a field a replan
    rewinds (reason 0), the tile-batch engine without its finalize pass does not (reason 1)."""
    W = world
    with W.context() as ctx:
        plan(ctx, W, False, engine=engine, resident=False)
        assert name in ctx.last_engine(), ctx.last_engine()
        assert seen(ctx, 3) == [F3] * 3
        assert all(downloads(ctx, i) == (False, False, False, True) for i in range(3))
        assert "output not resident" in refusal(lambda: ctx.download_output("dist", 0))
        r = robot_calls(ctx, W)
        assert "vector map of slot 0 not resident" in r["follow"] and "vector map of slot 0 not resident" in r["walks"]
        assert "predecessors of slot 0 not resident" in r["paths"] and "predecessors of slot 0 not resident" in r["costs"]
        a = replan(ctx)
        assert a["replan"]["reason"] == reason, a["replan"]
        assert seen(ctx, 3) == [(True, True, False)] * 3                     # a replan always finalizes; nobody asked for vector maps
        same_as_fresh(ctx, W, a, False)
        assert robot_calls(ctx, W)["paths"] is None


def test_an_inflation_wave_hides_the_outputs_and_a_replan_brings_them_back(world):
    W = world
    with W.context() as ctx:
        ctx.set_option("replan_fresh_below", 0)
        plan(ctx, W, True)
        lethal = np.zeros(W.mesh.V, np.uint8)
        lethal[W.mesh.vertex_at(0.5, 0.5)] = 1
        ctx.layer_upload(0, W.case.costs, lethal)
        ctx.layer_inflation(1, 0)                                            # the wave works in plan slot 0
        assert seen(ctx, 3) == [F3] * 3
        assert all(downloads(ctx, 0)[k] is False for k in range(4))
        assert "k_plan_async" in ctx.last_engine()                           # (the call is still the last Dijkstra call)
        # as found: the robot-side calls see ONE plan, and that one without a vector map
        assert "slot out of range" in refusal(lambda: follow(ctx, W, W.slots))
        assert "vector map of slot 0 not resident" in refusal(lambda: follow(ctx, W, np.zeros(2, np.uint32)))
        r = robot_calls(ctx, W)
        assert "n_plans differs from the last plan call" in r["walks"]
        assert "slot out of range" in refusal(lambda: ctx.fleet_walks(W.slots, W.seed_pos[:1], W.seed_faces[:1], W.pos, None, step_width=0.15, walk_cap=256))
        assert NOT_RESIDENT in r["paths"] and NOT_RESIDENT in r["costs"]
        a = replan(ctx)
        assert a["replan"]["reason"] == 0 and a["replan"]["log_len"] == 0, a["replan"]
        assert "k_tile_round" in ctx.last_engine()
        assert seen(ctx, 3) == [T3] * 3
        same_as_fresh(ctx, W, a, True)
        assert robot_calls(ctx, W) == dict(follow=None, paths=None, walks=None, costs=None)


def test_a_cvp_call_takes_the_outputs_and_keeps_the_recorded_call(world):
    W = world
    with W.context() as ctx:
        plan(ctx, W, True)
        c = ctx.plan_cvp_batch(W.seed_pos[:2], W.seed_faces[:2], W.robot_faces[:2], OFFSET)
        assert list(c["codes"]) == [0, 0]
        assert seen(ctx, 3) == [T3, T3, F3] and ctx.last_engine() == "none"
        assert downloads(ctx, 0) == (True, True, True, False)
        assert "not a Dijkstra plan" in refusal(lambda: ctx.download_output("popped", 0))
        r = robot_calls(ctx, W, n_plans=2)
        assert "slot out of range" in r["follow"] and "slot out of range" in r["walks"]      # robot 2 follows plan 2 of 2
        assert refusal(lambda: follow(ctx, W, np.array([0, 1], np.uint32))) is None          # the follower works on CVP fields
        assert NOT_RESIDENT in r["paths"] and NOT_RESIDENT in r["costs"]
        a = replan(ctx)                                                      # as found: the recorded Dijkstra call survived
        assert a["replan"]["reason"] == 1 and seen(ctx, 3) == [T3] * 3
        same_as_fresh(ctx, W, a, True)


def test_changed_costs_stop_the_fleet_calls_until_a_replan(world):
    W = world
    with W.context() as ctx:
        plan(ctx, W, True)
        ctx.upload_costs(W.case.costs, W.case.weights)
        assert seen(ctx, 3) == [T3] * 3 and downloads(ctx, 1) == (True, True, True, True)
        r = robot_calls(ctx, W)
        assert "the costs changed since the plan" in r["paths"] and "the costs changed since the plan" in r["costs"]
        assert r["follow"] is None and r["walks"] is None                    # (the follower and the walks read vector maps, whatever the log says)
        a = replan(ctx)
        assert a["replan"]["reason"] == 2 and seen(ctx, 3) == [T3] * 3
        same_as_fresh(ctx, W, a, True)
        assert robot_calls(ctx, W)["paths"] is None


def test_a_new_mesh_drops_the_recorded_call(world):
    W = world
    with W.context() as ctx:
        plan(ctx, W, True)
        W.case.upload(ctx)
        assert seen(ctx, 3) == [F3] * 3
        assert "no Dijkstra call" in refusal(lambda: replan(ctx))
        r = robot_calls(ctx, W)
        assert NOT_RESIDENT in r["paths"] and "vector map of slot 0 not resident" in r["follow"]   # (as found: the robot-side calls still see 3 plans)
        plan(ctx, W, True)
        assert seen(ctx, 3) == [T3] * 3 and replan(ctx)["replan"]["reason"] == 0
