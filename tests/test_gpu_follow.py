"""The vector-field follower on the device (mnav_follow_batch, mnav_follow_stats) against tests/follow_model.py, the
Python restatement of mesh_controller.cpp with the oracle's pinned pieces and the host libm's acosf: every query family
over the resident fields of a tile-batch Dijkstra batch, an asynchronous-engine batch, a single Dijkstra plan and a CVP
batch; 200 ticks of 256 unicycles; the lazy index build; the adapter's MeshController; errors.  Every comparison is
exact: codes, faces and `how` equal, floats and doubles by their bits (any NaN equals any NaN)."""
import ctypes as C

import numpy as np
import pytest

from mesh_navigation_amd import capi, meshgen
from tests import follow_model as FM
from tests import locate_model as LM
from tests.common import Case

pytestmark = pytest.mark.gpu

MESHES = {
    "terrain": lambda: meshgen.terrain(96, 0.1, 6, amplitude=0.6),
    "holes": lambda: meshgen.punched(72, 0.1, 4, drop=0.12),
    "hub": lambda: meshgen.fan_field(spokes=40, rings=6, seed=1),
}
SATURATING = FM.config(max_lin_velocity=0.8, max_ang_velocity=0.3, ang_vel_factor=4.0, lin_vel_factor=5.0, max_angle=45.0,
                       max_search_radius=0.15, max_search_distance=0.1)
N_PLANS = 6


def make_case(name):
    mesh = MESHES[name]()
    costs = np.random.default_rng(11).uniform(0.0, 0.8, mesh.V).astype(np.float32)
    return Case(mesh, costs, edge_cost_factor=1.0)


def plan_fields(ctx, case, kind):
    """runs the plans of `kind`, leaves their vector maps resident; returns (the fields as the model reads them, seed faces)"""
    mesh = case.mesh
    goal_f, robot_f = FM.plan_ends(mesh, N_PLANS)
    seeds, targets = mesh.faces[goal_f, 0], mesh.faces[robot_f, 0]
    ctx.set_resident_outputs(True)
    if kind == "cvp":
        goal_pos = mesh.xyz[mesh.faces[goal_f, 1]]                    # on a vertex of the seed face: its entry is the zero vector
        r = ctx.plan_cvp_batch(goal_pos, goal_f, robot_f, goal_dist_offset=0.05)
        assert (r["codes"] == capi.SUCCESS).all(), r["codes"]
        n, seed_faces = N_PLANS, goal_f
    elif kind == "single":
        out = ctx.plan_dijkstra(int(seeds[0]), int(targets[0]), goal_dist_offset=0.05, want_fields=False)
        assert out.code == capi.SUCCESS
        n, seed_faces = 1, np.array([FM.NONE], np.uint32)
    else:
        ctx.set_dijkstra_engine({"tile_batch": "tile_batch", "async": "async"}[kind])
        r = ctx.plan_dijkstra_batch(seeds, targets, goal_dist_offset=0.05)
        assert (r["codes"] == capi.SUCCESS).all(), r["codes"]
        assert ("tile-batch" in ctx.last_engine()) == (kind == "tile_batch") and ("async" in ctx.last_engine()) == (kind == "async")
        n, seed_faces = N_PLANS, np.full(N_PLANS, FM.NONE, np.uint32)
    return [ctx.download_output("vecmap", s) for s in range(n)], seed_faces


def device_tick(ctx, cfg, robots, seed_faces=True):
    o = ctx.follow(robots["pos"], robots["dir"], robots["up"], robots["face_in"], robots["slot"],
                   robots["seed_face"] if seed_faces and robots.get("seed_face") is not None else None, capi.FollowConfig(**cfg))
    return {k: getattr(o, k) for k in ("code", "how", "face", "bary", "pos", "mesh_dir", "cost", "cmd")}


def check_stats(ctx, want):
    st = ctx.follow_stats()
    assert st["stayed"] == (want["how"] == 2).sum() and st["neighbour"] == (want["how"] == 3).sum()
    assert st["global"] == ((want["how"] == 1) | (want["how"] == 4)).sum()
    assert st["lost"] == (want["code"] == FM.OUT_OF_MAP).sum() and st["no_field"] == (want["code"] == FM.NO_FIELD).sum()
    return st


@pytest.mark.parametrize("kind,name", [("tile_batch", "terrain"), ("async", "holes"), ("single", "hub"), ("cvp", "terrain"), ("cvp", "hub")])
def test_device_equals_the_model_on_every_family(gpu_ctx_factory, kind, name):
    case = make_case(name)
    ctx = gpu_ctx_factory()
    case.upload(ctx)
    fields, seed_faces = plan_fields(ctx, case, kind)
    model = FM.Model(case.mesh, case.om, case.costs)
    for cfg_name, cfg, per_family in (("default", FM.config(), 456), ("saturating", SATURATING, 40)):
        robots, fam = FM.make_robots(model, len(fields), seed_faces, 700 + len(name), per_family=per_family)    # 9 x 456 = 4104 robots
        robots = FM.set_angles(model, cfg, fields, robots, fam)
        use_seed = kind == "cvp"
        want = FM.tick_batch(model, cfg, fields, robots if use_seed else dict(robots, seed_face=None))
        got = device_tick(ctx, cfg, robots, seed_faces=use_seed)
        print(kind, name, cfg_name, "how:", np.bincount(want["how"], minlength=5), "code:", np.bincount(want["code"], minlength=3), ctx.follow_stats())
        FM.assert_same(got, want, (kind, name, cfg_name))
        check_stats(ctx, want)
        FM.assert_every_branch(want, fam, cfg, (kind, name, cfg_name))
        if cfg_name == "saturating":
            ok = want["code"] == FM.OK
            assert (want["cmd"][ok, 0] == cfg["max_lin_velocity"]).any() and (want["cmd"][ok, 1] == cfg["max_ang_velocity"]).any()
    assert robots["pos"].shape[0] >= 9 * 40 and np.unique(robots["slot"]).size == len(fields)


def test_two_hundred_ticks_of_256_unicycles(gpu_ctx_factory):
    case = make_case("terrain")
    ctx = gpu_ctx_factory()
    case.upload(ctx)
    fields, seed_faces = plan_fields(ctx, case, "cvp")
    model = FM.Model(case.mesh, case.om, case.costs)
    cfg = FM.config(max_lin_velocity=0.6, max_angle=60.0, max_ang_velocity=1.0)
    n, dt = 256, 0.1
    rng = np.random.default_rng(9)
    _, robot_f = FM.plan_ends(case.mesh, N_PLANS)
    slot = (np.arange(n) % N_PLANS).astype(np.uint32)
    cen = case.mesh.xyz[case.mesh.faces].astype(np.float64).mean(axis=1)
    pos = (cen[robot_f[slot]] + rng.normal(0, 0.3, (n, 3)) * np.array([1, 1, 0.05])).astype(np.float32)    # around their plan's robot face
    a = rng.uniform(0, 2 * np.pi, n)
    d = np.stack([np.cos(a), np.sin(a), np.zeros(n)], axis=1).astype(np.float32)
    up = np.tile(np.array([0, 0, 1], np.float32), (n, 1))
    face = np.full(n, FM.NONE, np.uint32)
    hows, n_ok = np.zeros(5, np.int64), 0
    for t in range(200):
        robots = dict(pos=pos, dir=d, up=up, face_in=face, slot=slot, seed_face=seed_faces[slot])
        want = FM.tick_batch(model, cfg, fields, robots)
        FM.assert_same(device_tick(ctx, cfg, robots), want, ("tick", t))
        hows += np.bincount(want["how"], minlength=5)
        ok = want["code"] == FM.OK
        n_ok += int(ok.sum())
        face = want["face"].copy()                                    # NONE after a tick that lost the mesh: the next one searches again
        for i in range(n):
            lin, ang = (want["cmd"][i, 0], want["cmd"][i, 1]) if ok[i] else (0.3, 0.4)      # no command: the robot coasts on a curve
            pos[i], d[i] = FM.unicycle_step(want["pos"][i], d[i], up[i], lin, ang, dt)
    print("ticks by how:", hows, "OK ticks:", n_ok)
    assert n_ok >= 100 * n and hows[1] >= n and hows[2] > 0 and hows[3] > 0


def test_the_index_is_built_only_when_a_robot_needs_a_global_search(gpu_ctx_factory):
    case = make_case("terrain")
    ctx = gpu_ctx_factory()
    case.upload(ctx)
    fields, seed_faces = plan_fields(ctx, case, "tile_batch")
    model = FM.Model(case.mesh, case.om, case.costs)
    rng = np.random.default_rng(4)
    n = 2048
    f = rng.integers(0, model.F, n)
    robots = dict(pos=FM.face_points(model, f, rng).astype(np.float32), dir=np.tile(np.array([1, 0, 0], np.float32), (n, 1)),
                  up=np.tile(np.array([0, 0, 1], np.float32), (n, 1)), face_in=f.astype(np.uint32), slot=(np.arange(n) % N_PLANS).astype(np.uint32),
                  seed_face=None)
    cfg = FM.config()
    want = FM.tick_batch(model, cfg, fields, robots)
    assert (want["how"] == 2).all()
    FM.assert_same(device_tick(ctx, cfg, robots), want, "all stay")
    st = check_stats(ctx, want)
    assert st["built_index"] == 0 and st["neighbour"] == 0 and st["global"] == 0 and st["stayed"] == n
    robots["pos"][17] = FM.face_points(model, np.array([(f[17] + model.F // 2) % model.F]), rng)[0]     # one robot is teleported across the mesh
    want = FM.tick_batch(model, cfg, fields, robots)
    assert want["how"][17] == 4
    FM.assert_same(device_tick(ctx, cfg, robots), want, "one teleported")
    st = check_stats(ctx, want)
    assert st["built_index"] == 1 and st["global"] == 1
    assert ctx.locate_stats()["built"] == 1                           # the lookup reports the build as its own ...
    ctx.locate(robots["pos"][:8])
    assert ctx.locate_stats()["built"] == 0                           # ... and does not build again
    FM.assert_same(device_tick(ctx, cfg, robots), want, "again")
    assert ctx.follow_stats()["built_index"] == 0


def test_errors_null_outputs_and_empty_batches(gpu_ctx_factory):
    case = make_case("terrain")
    model = FM.Model(case.mesh, case.om, case.costs)
    rng = np.random.default_rng(6)
    n = 64
    f = rng.integers(0, model.F, n)
    robots = dict(pos=FM.face_points(model, f, rng).astype(np.float32), dir=np.tile(np.array([0, 1, 0], np.float32), (n, 1)),
                  up=np.tile(np.array([0, 0, 1], np.float32), (n, 1)), face_in=f.astype(np.uint32), slot=np.zeros(n, np.uint32), seed_face=None)
    cfg = FM.config()
    ctx = gpu_ctx_factory()
    with pytest.raises(RuntimeError, match="mnav_upload_mesh"):
        device_tick(ctx, cfg, robots)
    ctx.upload_mesh(case.mesh.xyz, case.mesh.faces, case.mesh.edges, case.vn)
    with pytest.raises(RuntimeError, match="mnav_upload_costs"):
        device_tick(ctx, cfg, robots)
    case.upload(ctx)
    with pytest.raises(RuntimeError, match="slot out of range"):    # nothing planned yet
        device_tick(ctx, cfg, robots)
    empty = ctx.follow(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), np.zeros(0))
    assert empty.code.shape == (0,) and empty.cmd.shape == (0, 2)     # n == 0 does nothing
    # a paths-only batch of the tile-batch engine: mnav_vector_at serves it, the follower refuses it and touches nothing
    goal_f, robot_f = FM.plan_ends(case.mesh, N_PLANS)
    seeds, targets = case.mesh.faces[goal_f, 0], case.mesh.faces[robot_f, 0]
    ctx.set_dijkstra_engine("tile_batch")
    ctx.plan_dijkstra_batch(seeds, targets)
    assert ctx.vector_at(case.mesh.faces[robot_f[0]], np.array([0.3, 0.3, 0.4], np.float32), 0) is not None
    sentinel = dict(code=np.full(n, -7, np.int32), cmd=np.full((n, 2), -7.0))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    c = capi.FollowConfig()
    call = lambda cfgp, slots, face_in: ctx._L.mnav_follow_batch(ctx._h, n, p(robots["pos"]), p(robots["dir"]), p(robots["up"]), p(face_in), p(slots), None,
                                                                    cfgp, p(sentinel["code"]), None, None, None, None, None, p(sentinel["cmd"]), None)
    assert call(C.byref(c), robots["slot"], robots["face_in"]) == -1 and "not resident" in ctx._err()
    assert (sentinel["code"] == -7).all() and (sentinel["cmd"] == -7.0).all()
    # resident fields from here on
    fields, _ = plan_fields(ctx, case, "async")
    want = FM.tick_batch(model, cfg, fields, robots)
    dist0 = ctx.download_output("vecmap", 1)
    assert call(C.byref(c), np.full(n, N_PLANS, np.uint32), robots["face_in"]) == -1 and "slot out of range" in ctx._err()
    bad_face = robots["face_in"].copy()
    bad_face[5] = model.F
    assert call(C.byref(c), robots["slot"], bad_face) == -1 and "face id out of range" in ctx._err()
    for field, value in (("max_search_radius", 0.0), ("max_search_radius", float("nan")), ("max_search_distance", -1.0),
                         ("max_search_distance", float("inf"))):
        bad = capi.FollowConfig(**{field: value})
        assert call(C.byref(bad), robots["slot"], robots["face_in"]) == -1 and field in ctx._err(), (field, value)
    assert call(None, robots["slot"], robots["face_in"]) == -1 and "null" in ctx._err()
    assert (sentinel["code"] == -7).all() and (sentinel["cmd"] == -7.0).all()
    # NULL outputs: only what was asked for comes back
    assert call(C.byref(c), robots["slot"], robots["face_in"]) == 0
    assert np.array_equal(sentinel["code"], want["code"]) and FM.same_bits(sentinel["cmd"], want["cmd"])
    only = ctx.follow(robots["pos"], robots["dir"], robots["up"], robots["face_in"], robots["slot"], outputs=("cmd",))
    assert only.code is None and only.face is None and FM.same_bits(only.cmd, want["cmd"])
    none = ctx.follow(robots["pos"], robots["dir"], robots["up"], robots["face_in"], robots["slot"], outputs=())
    assert all(getattr(none, k) is None for k in ("code", "face", "bary", "pos", "mesh_dir", "cost", "cmd", "how"))
    FM.assert_same(device_tick(ctx, cfg, robots), want, "all outputs")
    # the call changed no plan output and no planner statistic
    assert np.array_equal(LM.bits(ctx.download_output("vecmap", 1)), LM.bits(dist0))
    s0 = ctx.stats()
    device_tick(ctx, cfg, robots)
    assert ctx.stats() == s0


# -- the adapter's MeshController --------------------------------------------------------------------------------------
def mesh_map_of(case):
    return dict(xyz=case.mesh.xyz, faces=case.mesh.faces, edges=case.mesh.edges, vertex_normals=case.vn, face_normals=case.fn,
                vertex_costs=case.costs, edge_weights=case.weights, invalid=case.invalid)


def pose_of(p, yaw):
    return np.array([p[0], p[1], p[2], 0.0, 0.0, np.sin(0.5 * yaw), np.cos(0.5 * yaw)], np.float64)


OUTCOME = {FM.OK: 0, FM.OUT_OF_MAP: 1, FM.NO_FIELD: 2}               # MeshController::Outcome SUCCESS / OUT_OF_MAP / FAILURE


def goal_reached_model(goal_pos, goal_dir, robot_pos, robot_dir, dist_tol, angle_tol):
    """mesh_controller.cpp:172-177"""
    goal_distance = FM.length(FM.sub(FM.vec(goal_pos), FM.vec(robot_pos)))
    angle = FM.F32(FM._libm.acosf(float(FM.dot(FM.vec(goal_dir), FM.vec(robot_dir)))))
    return bool(goal_distance <= FM.F32(dist_tol) and angle <= FM.F32(angle_tol))


def drive(ctl, model, cfg, field, has, start, yaw, goal_pose, ticks, dt):
    """ticks of the adapter's controller against the model, the unicycle integrated here; returns the smallest goal distance"""
    from mesh_navigation_amd.planner import MeshController
    goal_pos, goal_dir = goal_pose[:3].astype(np.float32), MeshController.direction(goal_pose, 0)
    pos, face, closest, n_ok = np.asarray(start, np.float32), FM.NONE, np.inf, 0
    for t in range(ticks):
        pose = pose_of(pos, yaw)
        d, up = MeshController.direction(pose, 0), MeshController.direction(pose, 2)
        assert abs(d[0] - np.cos(yaw)) < 1e-6 and abs(d[1] - np.sin(yaw)) < 1e-6 and np.allclose(up, [0, 0, 1], atol=1e-7)
        want = FM.tick(model, cfg, field, has, pos, d, up, face)
        code, cmd, face_out, pos_out, msg = ctl.computeVelocityCommands(pose)
        assert code == OUTCOME[want["code"]], (t, code, want["code"], msg)
        if want["code"] == FM.OUT_OF_MAP:
            assert face_out == face and FM.same_bits(pos_out, pos)     # nothing is kept from a tick that lost the map
        else:
            assert face_out == want["face"] and FM.same_bits(pos_out, np.asarray(want["pos"], np.float32)), (t, face_out, want["face"])
            face, pos = face_out, pos_out
        if want["code"] == FM.OK:
            assert FM.same_bits(cmd, want["cmd"]), (t, cmd, want["cmd"])
            n_ok += 1
        for tol in ((0.25, 4.0), (0.25, 0.6), (5.0, 0.3)):
            assert ctl.isGoalReached(*tol) == goal_reached_model(goal_pos, goal_dir, pos, d, *tol), (t, tol)
        closest = min(closest, float(np.linalg.norm(pos.astype(np.float64) - goal_pos)))
        if ctl.isGoalReached(0.25, 4.0):
            break
        lin, ang = (cmd[0], cmd[1]) if want["code"] == FM.OK else (0.0, 0.0)
        pos = (pos.astype(np.float64) + d.astype(np.float64) * lin * dt).astype(np.float32)
        yaw += ang * dt
    return closest, n_ok, t


def test_the_adapters_controller_follows_the_field_its_planner_left_on_the_device():
    from mesh_navigation_amd.planner import CVPMeshPlanner, DijkstraMeshPlanner, MeshController
    case = make_case("terrain")
    m = case.mesh
    model = FM.Model(m, case.om, case.costs)
    robot = m.xyz[m.vertex_at(0.7, 0.65)] + np.array([0.031, 0.017, 0.02], np.float32)
    goal = m.xyz[m.vertex_at(0.4, 0.35)] + np.array([0.023, 0.011, 0.01], np.float32)
    goal_pose = pose_of(goal, 0.4)
    # Dijkstra, every parameter at its default: the field is NOT copied into the host map (no setVectorMap side effect)
    pl = DijkstraMeshPlanner()
    assert pl.initialize("dijkstra_mesh_planner", mesh_map_of(case))
    code, plan, cost, msg = pl.makePlan(pose_of(robot, 0.0), goal_pose)
    assert code == 0 and len(plan) > 5
    plan[-1] = goal_pose                                               # (the controller reads the goal off the plan's last pose)
    ref = case.om.dijkstra(case.weights, case.costs, case.om.nearest_vertex(goal), case.om.nearest_vertex(robot))
    field = case.om.dijkstra_vector_map(ref.pred)
    has = FM.has_vector(model, field, FM.NONE)
    ctl = MeshController()
    assert ctl.initialize("mesh_controller", pl)
    assert ctl.setPlan(plan)
    cfg = FM.config()
    face0, bary0 = model.search_containing_face(robot)
    assert pl.host_direction(face0, bary0) is None                     # what the reference's controller would read: nothing ...
    closest, n_ok, t = drive(ctl, model, cfg, field, has, robot, 2.5, goal_pose, 400, 0.2)    # ... the device controller drives to the goal
    print("Dijkstra field: closest approach", closest, "OK ticks", n_ok, "of", t + 1)
    assert n_ok >= 20 and closest <= 0.25 and ctl.isGoalReached(0.25, 4.0)
    assert pl.host_direction(face0, bary0) is None                     # still nothing V-sized on the host
    # cancel: the tick still computes, the outcome says CANCELED until the next setPlan
    ctl.cancel()
    assert ctl.computeVelocityCommands(pose_of(robot, 2.5))[0] == MeshController.CANCELED
    assert ctl.setPlan(plan) and ctl.computeVelocityCommands(pose_of(robot, 2.5))[0] == MeshController.SUCCESS
    # non-default parameters reach the device
    slow = MeshController()
    assert slow.initialize("mesh_controller", pl, dict(max_lin_velocity=0.2, max_angle=90.0, max_search_distance=0.2))
    assert slow.setPlan(plan)
    closest2, n_ok2, _ = drive(slow, model, FM.config(max_lin_velocity=0.2, max_angle=90.0, max_search_distance=0.2), field, has, robot, 2.5, goal_pose, 40, 0.2)
    assert n_ok2 >= 20
    assert np.array_equal(LM.bits(pl.fetch("vector_map")), LM.bits(field))   # the field the controller followed is the reference's
    assert pl.host_direction(face0, bary0) is not None                 # (fetching it is what puts it into the host map)
    # a replan on the same context while the controller ticks (get_path beside exe_path): the context's lock serialises
    # them; the same start and goal give the same field, so every tick returns the first tick's bits
    import threading
    assert ctl.setPlan(plan)
    first = ctl.computeVelocityCommands(pose_of(robot, 2.5))
    assert first[0] == MeshController.SUCCESS
    replans = []

    def replan():
        for _ in range(6):
            replans.append(pl.makePlan(pose_of(robot, 0.0), goal_pose)[0])

    th = threading.Thread(target=replan)
    th.start()
    ticks = 0
    while th.is_alive() or ticks < 50:
        assert ctl.setPlan(plan)                                       # (forget the face: every tick is the first tick again)
        again = ctl.computeVelocityCommands(pose_of(robot, 2.5))
        assert again[0] == first[0] and again[2] == first[2] and FM.same_bits(again[1], first[1]) and FM.same_bits(again[3], first[3]), (ticks, again)
        ticks += 1
    th.join()
    assert replans == [0] * 6
    # the planner goes first: the controller holds the context's handle, finds it withdrawn and refuses
    pl.close()
    code, _, _, _, msg = ctl.computeVelocityCommands(pose_of(robot, 2.5))
    assert code == MeshController.INTERNAL_ERROR and "gone" in msg
    assert not ctl.setPlan(plan)
    slow.close(); ctl.close()
    # CVP: the plan's seed face goes along
    pc = CVPMeshPlanner()
    assert pc.initialize("cvp_mesh_planner", mesh_map_of(case), dict(step_width=0.1))
    code, plan, cost, msg = pc.makePlan(pose_of(robot, 0.0), goal_pose)
    assert code == 0, msg
    sf, _ = case.om.containing_face(goal)
    tf, _ = case.om.containing_face(robot)
    cv = case.om.cvp(case.weights, case.costs, case.vn, goal, sf, tf)
    field = (cv.vecmap * cv.has_vec[:, None]).astype(np.float32)
    ctl = MeshController()
    assert ctl.initialize("mesh_controller", pc) and ctl.setPlan(plan, 0, sf)
    closest, n_ok, t = drive(ctl, model, cfg, field, FM.has_vector(model, field, sf), robot, 2.5, goal_pose, 60, 0.2)
    print("CVP field: closest approach", closest, "OK ticks", n_ok, "of", t + 1)
    assert n_ok >= 30
    ctl.close(); pc.close()
