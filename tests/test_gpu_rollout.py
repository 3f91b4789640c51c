"""The device rollout (mnav_follow_rollout, mnav_rollout_stats) against tests/rollout_model.py, the Python restatement of
its specification with the host libm's cosf, sinf and acosf, over the resident fields of a single Dijkstra plan, an 8-plan
batch of the asynchronous engine, a 168-plan batch of the tile-batch engine and a 4-plan CVP batch; against the loop of
mnav_follow_batch calls it replaces; resumed in two calls; the index build at the start; refusals; the cancel flag; and,
against the compiled host mirror, a fleet large enough for a second trip of the list passes' grid-stride loops.  Every
comparison is exact: integers equal, floats and doubles by their bits (any NaN equals any NaN)."""
import ctypes as C

import numpy as np
import pytest

from mesh_navigation_amd import capi, meshgen
from tests import follow_model as FM
from tests import locate_model as LM
from tests import rollout_model as RM
from tests.common import Case
from tests.test_rollout_model import ANG_TOL, DIST_TOL, DT, TICKS, Mirror, after_tick, build_shim, fleet, fresh_state

pytestmark = pytest.mark.gpu

MESHES = {"terrain": lambda: meshgen.terrain(64, 0.1, 6, amplitude=0.6), "holes": lambda: meshgen.punched(72, 0.1, 4, drop=0.12)}
KINDS = {"single": ("terrain", 1), "async": ("terrain", 8), "tile_batch": ("terrain", 168), "cvp": ("holes", 4)}    # mesh, plans
SATURATING = FM.config(max_lin_velocity=0.8, max_ang_velocity=0.3, ang_vel_factor=4.0, lin_vel_factor=5.0, max_angle=45.0,
                       max_search_radius=0.15, max_search_distance=0.1)


class World:
    """a context with the resident fields of one plan call, the model of its mesh and the fields as the model reads them
    (downloaded when a robot first uses them)"""

    def __init__(self, ctx, kind):
        name, self.n_plans = KINDS[kind]
        mesh = MESHES[name]()
        self.case = Case(mesh, np.random.default_rng(11).uniform(0.0, 0.8, mesh.V).astype(np.float32), edge_cost_factor=1.0)
        self.ctx, self.kind = ctx, kind
        self.case.upload(ctx)
        self.model = FM.Model(mesh, self.case.om, self.case.costs)
        goal_f, robot_f = FM.plan_ends(mesh, self.n_plans)
        seeds, targets = mesh.faces[goal_f, 0], mesh.faces[robot_f, 0]
        ctx.set_resident_outputs(True)
        self.seed_faces = np.full(self.n_plans, FM.NONE, np.uint32)
        if kind == "cvp":
            r = ctx.plan_cvp_batch(mesh.xyz[mesh.faces[goal_f, 1]], goal_f, robot_f, goal_dist_offset=0.05)
            assert (r["codes"] == capi.SUCCESS).all(), r["codes"]
            self.seed_faces = goal_f
        elif kind == "single":
            assert ctx.plan_dijkstra(int(seeds[0]), int(targets[0]), goal_dist_offset=0.05, want_fields=False).code == capi.SUCCESS
        else:
            ctx.set_dijkstra_engine(kind)
            r = ctx.plan_dijkstra_batch(seeds, targets, goal_dist_offset=0.05)
            assert (r["codes"] == capi.SUCCESS).all(), r["codes"]
            assert ("tile-batch" in ctx.last_engine()) == (kind == "tile_batch") and ("async" in ctx.last_engine()) == (kind == "async")
        self.fields = {}

    def fleet(self, seed, per_family, drivers, close=5):
        robots, goals = fleet(self.model, self.n_plans, self.seed_faces, seed, per_family, drivers, close)
        for s in np.unique(robots["slot"]):
            if int(s) not in self.fields:
                self.fields[int(s)] = self.ctx.download_output("vecmap", int(s))
        if self.kind != "cvp":
            robots["seed_face"] = None
        return robots, goals

    def model_run(self, cfg, robots, goals, ticks, trace_stride=1):
        return RM.run(self.model, cfg, self.fields, robots, goals, DT, ticks, DIST_TOL, ANG_TOL, trace_stride=trace_stride)

    def device_run(self, cfg, robots, goals, ticks, trace_stride=1, outputs=None):
        ro = capi.RolloutConfig(dt=DT, dist_tolerance=DIST_TOL, angle_tolerance=ANG_TOL, ticks=ticks, trace_stride=trace_stride)
        g = (None, None) if goals is None else goals
        return self.ctx.rollout(robots["pos"], robots["dir"], robots["up"], robots["face_in"], robots["slot"], robots.get("seed_face"), g[0], g[1],
                                capi.FollowConfig(**cfg), ro, outputs)


@pytest.fixture(scope="module")
def worlds(gpu_ctx_factory):
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = World(gpu_ctx_factory(), kind)
        return made[kind]

    return get


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory)


def check_stats(ctx, want, n):
    st = ctx.rollout_stats()
    assert [st[k] for k in ("running", "reached", "out_of_map", "no_field")] == np.bincount(want["status"], minlength=4).tolist(), st
    assert st["robot_ticks"] == int(want["ticks"].sum()) and st["stayed"] == want["how"][2] and st["neighbour"] == want["how"][3]
    assert st["global"] == want["how"][1] + want["how"][4] and st["ms_kernels"] > 0 and st["ms_total"] >= st["ms_kernels"]
    return st


# n = 65: one robot past a wave; 257: one past a workgroup of the stay pass; strides 1 and 7 (ticks % 7 != 0 at 120 and 8)
@pytest.mark.parametrize("kind,cfg_name,n,ticks,with_goals", [("async", "default", 65, TICKS, True), ("tile_batch", "saturating", 65, TICKS, True),
                                                              ("tile_batch", "default", 65, TICKS, False), ("cvp", "default", 65, TICKS, True),
                                                              ("cvp", "default", 257, 8, True), ("single", "default", 1, 1, True)])
def test_device_equals_the_model(worlds, kind, cfg_name, n, ticks, with_goals):
    w = worlds(kind)
    cfg = SATURATING if cfg_name == "saturating" else FM.config()
    if n == 1:
        robots, goals = w.fleet(40, 0, 1, close=1)
        robots = {k: (None if v is None else v[-1:]) for k, v in robots.items()}
        goals = (goals[0][-1:], goals[1][-1:])
    else:
        per_family = 3 if n == 65 else 9
        robots, goals = w.fleet(42 if kind == "cvp" else 40, per_family, n - 9 * per_family, close=5 if n == 65 else 40)
    assert robots["pos"].shape[0] == n and (n == 1 or np.unique(robots["slot"]).size == min(n - 9 * per_family, w.n_plans))    # several plans
    g = goals if with_goals else None
    want = w.model_run(cfg, robots, g, ticks)
    got = w.device_run(cfg, robots, g, ticks)
    st = w.ctx.rollout_stats()
    print(kind, cfg_name, n, ticks, "status:", np.bincount(want["status"], minlength=4), "how:", want["how"], st)
    assert not got.cancelled
    RM.assert_same(got, want, (kind, cfg_name, n, ticks))
    check_stats(w.ctx, want, n)
    if ticks >= 7:
        got7 = w.device_run(cfg, robots, g, ticks, trace_stride=7)
        assert got7.trace.shape == (n, ticks // 7, 3) and FM.same_bits(got7.trace, want["trace"][:, 6::7][:, : ticks // 7])
        RM.assert_same(got7, want, (kind, cfg_name, n, ticks, "stride 7"), keys=RM.KEYS)
    if n == 65 and with_goals:
        RM.assert_every_outcome(want, (kind, cfg_name))
    if n == 1:
        assert want["ticks"][0] == 1 and want["how"].sum() == 1


def test_equals_the_loop_of_calls_it_replaces(worlds, shim):
    w = worlds("async")
    cfg, T = FM.config(), 40
    robots, goals = w.fleet(40, 3, 38)
    n = robots["pos"].shape[0]
    S = fresh_state(robots)
    fc = capi.FollowConfig(**cfg)
    for t in range(T):
        o = w.ctx.follow(S["pos"], S["dir"], robots["up"], S["face"], robots["slot"], None, fc)
        after_tick(shim, S, robots["up"], goals, DT, DIST_TOL, ANG_TOL, dict(code=o.code, how=o.how, face=o.face, pos=o.pos, cost=o.cost, cmd=o.cmd))
    got = w.device_run(cfg, robots, goals, T, trace_stride=0)
    assert got.trace is None
    RM.assert_same(got, S, "40 calls", keys=RM.KEYS)
    assert len(set(S["status"].tolist())) >= 3 and (S["ticks"] == T).any() and ((S["ticks"] > 1) & (S["ticks"] < T)).any()


def big_fleet(model, seed=7, n_first=65537, n_moved=2049, n_stay=300):
    """65 537 robots without a face (one more than the 1 024 x 64 lanes of the global pass), 2 049 with a face that does not
    hold them (one more than the 2 048 workgroups of the search pass: three in four a face 5 to 30 cm away, the fourth one
    across the mesh) and 300 on their own face; every robot stands inside a random face.  A goal per robot: the middle of
    the mesh, heading +x."""
    rng = np.random.default_rng(seed)
    n = n_first + n_moved + n_stay
    cen = model.xyz[model.faces].astype(np.float64).mean(axis=1)
    f = rng.integers(0, model.F, n)
    given = f.astype(np.uint32)
    given[:n_first] = FM.NONE
    for j in range(n_first, n_first + n_moved):
        d = np.linalg.norm(cen - cen[f[j]], axis=1)
        given[j] = rng.choice(np.nonzero((d > 0.05) & (d < 0.3) if j % 4 else d > 0.95)[0])
    a = rng.uniform(0, 2 * np.pi, n)
    pos = FM.face_points(model, f, rng)
    k = n_first + n_moved                                            # those that may need searchContainingFace stand near a corner of their face: it looks
    pos[:k] = 0.75 * model.xyz[model.faces[f[:k], rng.integers(0, 3, k)]].astype(np.float64) + 0.25 * pos[:k]   # around the nearest vertex only
    robots = dict(pos=pos.astype(np.float32), dir=np.stack([np.cos(a), np.sin(a), np.zeros(n)], axis=1).astype(np.float32),
                  up=np.tile(np.array([0, 0, 1], np.float32), (n, 1)), face_in=given, slot=np.zeros(n, np.uint32), seed_face=None)
    mid = cen[int(np.argmin(np.linalg.norm(cen - cen.mean(axis=0), axis=1)))].astype(np.float32)
    return robots, (np.tile(mid, (n, 1)), np.tile(np.array([1, 0, 0], np.float32), (n, 1)))


def test_the_second_trip_of_the_list_passes(worlds, shim):
    """Both grid-stride loops of the shared passes go round twice in tick 1: the global pass of the rollout (1 024 workgroups
    of 64 lanes) and the search pass of either caller (2 048 workgroups).  The reference is the compiled host mirror (rol_run
    of mnav_rollout.h through tests/test_rollout_model.py): the per-robot Python model would take minutes."""
    w = worlds("single")
    cfg = FM.config()
    robots, goals = big_fleet(w.model)
    n = robots["pos"].shape[0]
    if 0 not in w.fields:
        w.fields[0] = w.ctx.download_output("vecmap", 0)
    mirror = Mirror(shim, w.model)
    tick1 = mirror.run(cfg, [w.fields[0]], robots, goals, DT, 1, DIST_TOL, ANG_TOL, trace_stride=1)
    want = mirror.run(cfg, [w.fields[0]], robots, goals, DT, 1, DIST_TOL, ANG_TOL, trace_stride=1, state=tick1)
    mirror.close()
    want["how"] = tick1["how"] + want["how"]
    want["trace"] = np.concatenate([tick1["trace"], want["trace"]], axis=1)
    print("tick 1 how:", tick1["how"], "both ticks:", want["how"], "status:", np.bincount(want["status"], minlength=4))
    assert tick1["how"][1] >= 65537 and tick1["how"][3] + tick1["how"][4] >= 2049 and tick1["how"][2] > 0
    got = w.device_run(cfg, robots, goals, 2)
    RM.assert_same(got, want, "2 ticks")
    check_stats(w.ctx, want, n)
    # the follower on the same fleet: one call and rol_after_tick on the host equal one tick of the rollout
    S = fresh_state(robots)
    o = w.ctx.follow(S["pos"], S["dir"], robots["up"], S["face"], robots["slot"], None, capi.FollowConfig(**cfg))
    fs = w.ctx.follow_stats()
    assert (fs["stayed"], fs["neighbour"], fs["global"]) == (tick1["how"][2], tick1["how"][3], tick1["how"][1] + tick1["how"][4]), fs
    after_tick(shim, S, robots["up"], goals, DT, DIST_TOL, ANG_TOL, dict(code=o.code, how=o.how, face=o.face, pos=o.pos, cost=o.cost, cmd=o.cmd))
    one = w.device_run(cfg, robots, goals, 1, trace_stride=0)
    RM.assert_same(one, S, "one call", keys=RM.KEYS)
    RM.assert_same(one, tick1, "one tick", keys=RM.KEYS)


def test_resume_and_a_call_that_spans_two_blocks(worlds):
    w = worlds("async")
    cfg = FM.config()
    robots, goals = w.fleet(40, 3, 38)
    whole = w.device_run(cfg, robots, goals, TICKS, trace_stride=0)
    a = w.device_run(cfg, robots, goals, 50, trace_stride=0)
    run = np.nonzero(a.status == RM.RUNNING)[0]
    stopped = np.nonzero(a.status != RM.RUNNING)[0]
    assert run.size >= 8 and stopped.size >= 8
    RM.assert_same({k: getattr(a, k)[stopped] for k in RM.KEYS}, {k: getattr(whole, k)[stopped] for k in RM.KEYS}, "stopped by tick 50", keys=RM.KEYS)
    # pos_out, dir_out, face_out of the RUNNING robots fed back: 50 + 70 = 120 in every state bit (travel and cost_integral
    # are sums of one call: not compared)
    sub = dict(pos=a.pos[run], dir=a.dir[run], up=robots["up"][run], face_in=a.face[run], slot=robots["slot"][run])
    b = w.device_run(cfg, sub, (goals[0][run], goals[1][run]), 70, trace_stride=0)
    for k in ("status", "pos", "dir", "face"):
        assert FM.same_bits(getattr(b, k), getattr(whole, k)[run]), k
    assert np.array_equal(a.ticks[run] + b.ticks, whole.ticks[run])
    assert FM.same_bits(np.minimum(a.min_goal_dist[run], b.min_goal_dist), whole.min_goal_dist[run])
    assert (b.status == RM.RUNNING).any() and (b.status != RM.RUNNING).any()
    # 300 ticks: two blocks of the tick loop (256 + 44)
    r16 = {k: (None if v is None else v[-16:]) for k, v in robots.items()}
    g16 = (goals[0][-16:].copy(), goals[1][-16:])
    g16[0][::2, 0] += 50.0                                            # half of them never arrive
    want = w.model_run(cfg, r16, g16, 300)
    got = w.device_run(cfg, r16, g16, 300)
    RM.assert_same(got, want, "300 ticks")
    check_stats(w.ctx, want, 16)
    assert (want["ticks"] == 300).any() and (want["ticks"] < 256).any()


def test_the_index_is_built_once_at_the_start(gpu_ctx_factory):
    w = World(gpu_ctx_factory(), "single")                           # a fresh upload: no index yet
    rng = np.random.default_rng(4)
    n = 300
    lit = np.nonzero((np.asarray(w.ctx.download_output("vecmap", 0)) != 0).any(axis=1)[w.model.faces].all(axis=1))[0]
    f = rng.choice(lit, n)
    robots = dict(pos=FM.face_points(w.model, f, rng).astype(np.float32), dir=np.tile(np.array([1, 0, 0], np.float32), (n, 1)),
                  up=np.tile(np.array([0, 0, 1], np.float32), (n, 1)), face_in=f.astype(np.uint32), slot=np.zeros(n, np.uint32), seed_face=None)
    w.fields[0] = w.ctx.download_output("vecmap", 0)
    cfg = FM.config(max_lin_velocity=0.02)                           # 5 mm a tick: nobody leaves its neighbourhood
    want = w.model_run(cfg, robots, None, 6)
    assert want["how"][1] == 0 and want["how"][4] == 0 and want["how"][2] > 0 and (want["status"] == RM.RUNNING).all()
    RM.assert_same(w.device_run(cfg, robots, None, 6), want, "first call")
    st = check_stats(w.ctx, want, n)
    assert st["built_index"] == 1 and st["global"] == 0               # built although no robot needed it: no look at the lists between ticks
    assert w.ctx.locate_stats()["built"] == 1                         # the lookup reports the build as its own ...
    RM.assert_same(w.device_run(cfg, robots, None, 6), want, "second call")
    assert w.ctx.rollout_stats()["built_index"] == 0                  # ... and nobody builds again
    w.ctx.locate(robots["pos"][:8])
    assert w.ctx.locate_stats()["built"] == 0


def test_refusals_touch_nothing(worlds):
    w = worlds("async")
    ctx, cfg = w.ctx, FM.config()
    robots, goals = w.fleet(40, 3, 38)
    n = robots["pos"].shape[0]
    before = ctx.follow(robots["pos"], robots["dir"], robots["up"], robots["face_in"], robots["slot"])
    field0, stats0, fstats0 = ctx.download_output("vecmap", 1), ctx.stats(), ctx.follow_stats()
    sentinel = dict(status=np.full(n, -7, np.int32), pos=np.full((n, 3), -7.0, np.float32), travel=np.full(n, -7.0), trace=np.full((n, 4, 3), -7.0, np.float32))
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(fc=None, ro=None, slots=robots["slot"], face_in=robots["face_in"], gp=goals[0], gd=goals[1], trace=sentinel["trace"], null_cfg=False, null_ro=False,
             pos=robots["pos"]):
        fc = fc if fc is not None else capi.FollowConfig(**cfg)
        ro = ro if ro is not None else capi.RolloutConfig(dt=DT, ticks=4, trace_stride=1)
        return ctx._L.mnav_follow_rollout(ctx._h, n, p(pos), p(robots["dir"]), p(robots["up"]), p(face_in), p(slots), None, p(gp), p(gd),
                                          None if null_cfg else C.byref(fc), None if null_ro else C.byref(ro), p(sentinel["status"]), None, p(sentinel["pos"]),
                                          None, None, p(sentinel["travel"]), None, None, p(trace))

    RC = capi.RolloutConfig
    bad_face = robots["face_in"].copy()
    bad_face[5] = w.model.F
    refusals = [
        (dict(pos=None), "null"), (dict(null_cfg=True), "null"), (dict(null_ro=True), "null"),
        (dict(slots=np.full(n, w.n_plans, np.uint32)), "slot out of range"), (dict(face_in=bad_face), "face id out of range"),
        (dict(fc=capi.FollowConfig(max_search_radius=0.0)), "max_search_radius"), (dict(fc=capi.FollowConfig(max_search_distance=float("inf"))), "max_search_distance"),
        (dict(ro=RC(dt=0.0, ticks=4)), "dt"), (dict(ro=RC(dt=-0.1, ticks=4)), "dt"), (dict(ro=RC(dt=float("nan"), ticks=4)), "dt"),
        (dict(ro=RC(dt=float("inf"), ticks=4)), "dt"),
        (dict(ro=RC(dt=DT, ticks=0)), "ticks"), (dict(ro=RC(dt=DT, ticks=100001)), "ticks"),
        (dict(ro=RC(dt=DT, ticks=4, trace_stride=1), trace=None), "trace_out"), (dict(ro=RC(dt=DT, ticks=4, trace_stride=5)), "trace_stride"),
        (dict(gd=None), "goal"), (dict(gp=None), "goal"),
        (dict(ro=RC(dt=DT, ticks=4, dist_tolerance=float("nan"))), "tolerance"), (dict(ro=RC(dt=DT, ticks=4, angle_tolerance=float("nan"))), "tolerance"),
        (dict(fc=capi.FollowConfig(max_ang_velocity=400.0)), "100"), (dict(fc=capi.FollowConfig(max_ang_velocity=100.0, ang_vel_factor=4.0)), "100"),
        (dict(fc=capi.FollowConfig(max_ang_velocity=0.5, ang_vel_factor=0.01), ro=RC(dt=200.0, ticks=4)), "100"),
    ]
    for kw, text in refusals:
        assert call(**kw) == -1 and text in ctx._err(), (kw, ctx._err())
        assert all((v == -7).all() for v in sentinel.values()), kw
    # the resident field, the planner's statistics and the follower's last outputs are what they were
    assert np.array_equal(LM.bits(ctx.download_output("vecmap", 1)), LM.bits(field0)) and ctx.stats() == stats0 and ctx.follow_stats() == fstats0
    after = ctx.follow(robots["pos"], robots["dir"], robots["up"], robots["face_in"], robots["slot"])
    FM.assert_same({k: getattr(after, k) for k in ("code", "how", "face", "bary", "pos", "mesh_dir", "cost", "cmd")},
                   {k: getattr(before, k) for k in ("code", "how", "face", "bary", "pos", "mesh_dir", "cost", "cmd")}, "follow after the refusals")
    # just inside the bound, NULL outputs, n = 0: served
    assert call(fc=capi.FollowConfig(max_ang_velocity=399.0)) == 0 and (sentinel["status"] != -7).all() and (sentinel["trace"] != -7.0).all()
    only = w.device_run(cfg, robots, goals, 4, trace_stride=0, outputs=("status",))
    assert only.pos is None and only.travel is None and only.trace is None and np.array_equal(only.status, w.model_run(cfg, robots, goals, 4)["status"])
    empty = ctx.rollout(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), np.zeros(0))
    assert empty.status.shape == (0,) and empty.pos.shape == (0, 3) and not empty.cancelled
    # a successful rollout changes no plan output and no statistic of the planner or the follower either
    assert np.array_equal(LM.bits(ctx.download_output("vecmap", 1)), LM.bits(field0)) and ctx.stats() == stats0
    fs = ctx.follow_stats()
    w.device_run(cfg, robots, goals, 4)
    assert ctx.follow_stats() == fs


def test_a_cancel_flag_set_before_the_call_is_cleared_at_entry(worlds):
    w = worlds("async")
    cfg = FM.config()
    robots, goals = w.fleet(40, 3, 38)
    want = w.device_run(cfg, robots, goals, 20)
    w.ctx.cancel()
    got = w.device_run(cfg, robots, goals, 20)
    assert not got.cancelled and (got.ticks == want.ticks).all() and got.ticks.max() == 20
    RM.assert_same(got, {k: getattr(want, k) for k in RM.KEYS + ("trace",)}, "after a stale cancel")
