"""The sampled rollout (mnav_follow_sample, mnav_sample_stats) against tests/sample_model.py, the Python restatement of its
specification, over the resident fields and potentials of a single Dijkstra plan, an 8-plan batch of the asynchronous
engine, a 168-plan batch of the tile-batch engine and a 4-plan CVP batch: n = 67 robots (one past a wave), K in {1, 5, 64,
130} (n * K no multiple of 256, K no multiple of 64), 1, 7 and 40 ticks, with and without goals, robots without a face,
robots that leave the mesh, vertex costs above lethal_cost in reach.  Also: candidate (1, 0, 1, 0) against
mnav_follow_rollout on the device; K = 130 and K = 64 with candidates that all differ, at 7 and 40 ticks with goals, against
the compiled host mirror, with the whole branch list; 300 ticks (two blocks of the tick loop); 40 x 64 rows that all need a
neighbour search at once, against the compiled host mirror (a second trip of the search pass's grid-stride loop); a table with one candidate
twice; NULL per-row outputs; two identical calls; the statistics; refusals; the rollout's statistics left alone; the cancel
flag.  Every comparison is exact: integers equal, floats and doubles by their bits (any NaN equals any NaN).

The branch list of the CPU test (every final status, a lethal row, a robot without a pick, a pick that is not candidate 0,
two rows tied in J) is asserted on the model's output where the case can meet it: a call of one tick reaches no goal and ties
all rows of a robot (J reads nothing a candidate has changed yet), a call without goals reaches none either, and K = 1 has
neither ties nor another pick -- those cases assert the rest of the list.

Not tested: "a slot whose potential is not resident".  No sequence of public calls reaches it today -- the follower's check
asks for the slot's vector map first, and the finalize pass that leaves a vector map resident leaves the potential too --
so the refusal is a guard in the driver, exercised by no test."""
import ctypes as C

import numpy as np
import pytest

from mesh_navigation_amd import capi
from tests import follow_model as FM
from tests import rollout_model as RM
from tests import sample_model as SM
from tests.test_follow_model import CONFIGS
from tests.test_gpu_rollout import SATURATING, World as RolloutWorld
from tests.test_rollout_model import ANG_TOL, DIST_TOL, DT
from tests.test_sample_model import Mirror, build_shim

pytestmark = pytest.mark.gpu

SAMPLE = dict(w_potential=1.0, w_cost=0.5, w_time=0.1, lethal_cost=0.7)      # the vertex costs are uniform in 0 .. 0.8
# follower, an arc to the left, follow but keep left, the arc again (two rows tied in J), straight ahead
TABLE5 = np.array([[1, 0, 1, 0], [0, 0.5, 0, 0.3], [1, 0, 1, 0.2], [0, 0.5, 0, 0.3], [0, 1.0, 0, 0]], np.float64)


def table(K, distinct, seed=3):
    """K candidates of which `distinct` differ (the others repeat them, shuffled): gains 0 / 0.5 / 1, small biases of either
    sign, some exactly zero; candidate 0 is the follower"""
    rng = np.random.default_rng(seed)
    t = np.stack([rng.choice([0.0, 0.5, 1.0], distinct), rng.choice([0.0, 0.0, 0.1, 0.4, -0.05], distinct), rng.choice([0.0, 1.0, 1.0, -0.5], distinct),
                  rng.choice([0.0, 0.0, 0.2, -0.2, 0.35], distinct)], axis=1)
    t[0] = [1, 0, 1, 0]
    idx = np.concatenate([np.arange(distinct), rng.integers(0, distinct, K - distinct)])
    idx[1:] = rng.permutation(idx[1:])
    return np.ascontiguousarray(t[idx], np.float64)


class World(RolloutWorld):
    """the rollout tests' world, with the potentials as the model reads them (downloaded when a robot first uses them)"""

    def __init__(self, ctx, kind):
        super().__init__(ctx, kind)
        self.pots = {}

    def fleet(self, seed, per_family, drivers, close=5):
        robots, goals = super().fleet(seed, per_family, drivers, close)
        for s in np.unique(robots["slot"]):
            if int(s) not in self.pots:
                self.pots[int(s)] = self.ctx.download_output("dist", int(s))
        return robots, goals

    def sample_model(self, cfg, robots, goals, tab, ticks, sample=SAMPLE):
        return SM.run(self.model, cfg, self.fields, self.pots, robots, goals, tab, DT, ticks, DIST_TOL, ANG_TOL, sample)

    def sample_device(self, cfg, robots, goals, tab, ticks, sample=SAMPLE, outputs=None):
        ro = capi.RolloutConfig(dt=DT, dist_tolerance=DIST_TOL, angle_tolerance=ANG_TOL, ticks=ticks, trace_stride=0)
        g = (None, None) if goals is None else goals
        return self.ctx.follow_sample(robots["pos"], robots["dir"], robots["up"], robots["face_in"], robots["slot"], tab, robots.get("seed_face"), g[0], g[1],
                                      capi.FollowConfig(**cfg), ro, capi.SampleConfig(**sample), outputs)


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


CASES = {   # kind: follower config, K, distinct candidates, ticks, with goals
    "single": ("default", 130, 130, 1, True),
    "async": ("default", 5, 5, 40, True),
    "tile_batch": ("saturating", 64, 16, 7, False),
    "cvp": ("default", 1, 1, 40, True),
}


@pytest.fixture(scope="module")
def case(worlds):
    """a case's world, inputs and model output, computed once and shared (nobody changes them)"""
    made = {}

    def get(kind):
        if kind not in made:
            w = worlds(kind)
            cfg_name, K, distinct, ticks, with_goals = CASES[kind]
            cfg = SATURATING if cfg_name == "saturating" else FM.config()
            robots, goals = w.fleet(42 if kind == "cvp" else 40, 3, 40)
            tab = TABLE5 if K == 5 else table(K, distinct)
            g = goals if with_goals else None
            made[kind] = (w, cfg, robots, g, tab, ticks, w.sample_model(cfg, robots, g, tab, ticks))
        return made[kind]

    return get


def check_stats(ctx, want):
    st = ctx.sample_stats()
    for k, v in SM.stats(want).items():
        assert st[k] == v, (k, st, v)
    assert st["ms_kernels"] > 0 and st["ms_total"] >= st["ms_kernels"] and st["ms_expand"] > 0 and st["ms_pick"] > 0
    return st


@pytest.mark.parametrize("kind", list(CASES))
def test_device_equals_the_model(case, kind):
    w, cfg, robots, goals, tab, ticks, want = case(kind)
    n, K = robots["pos"].shape[0], tab.shape[0]
    assert n == 67 and (n * K) % 256 != 0
    assert (robots["face_in"] == FM.NONE).any() and np.unique(robots["slot"]).size >= min(40, w.n_plans)
    got = w.sample_device(cfg, robots, goals, tab, ticks)
    status = np.bincount(want["status"].reshape(-1), minlength=4)
    print(kind, K, ticks, "status:", status, "lethal:", int(want["lethal"].sum()), "no pick:", int((want["best_k"] == SM.NONE).sum()), "best_k:", want["best_k"],
          "how:", want["how"], w.ctx.sample_stats())
    assert not got["cancelled"]
    SM.assert_same(got, want, (kind, K, ticks))
    check_stats(w.ctx, want)
    # what the model's output must reach (the module docstring has the exceptions)
    assert status[RM.RUNNING] and status[RM.OUT_OF_MAP] and status[RM.NO_FIELD] and (want["best_k"] == SM.NONE).any()
    assert want["how"][1] > 0 and want["how"][2] > 0 and want["how"][3] > 0
    if ticks > 1:
        assert want["lethal"].any()
    if ticks > 1 and goals is not None:
        assert status[RM.REACHED]
    if K > 1 and ticks > 1:
        assert ((want["best_k"] != SM.NONE) & (want["best_k"] != 0)).any()
    if K > 1 and ticks == 1:                                          # one tick: a robot's rows differ in nothing J reads, all tied, and k = 0 wins
        assert ((want["n_feasible"] == K) & (want["best_k"] == 0)).any()
    if kind == "async":
        SM.assert_every_branch(want, kind)


def distinct_table(K, seed, twice=()):
    """K candidates with continuous gains and biases, all different -- no two rows of a robot share a trajectory -- except that
    candidate b repeats candidate a for every (a, b) of `twice`; candidate 0 is the follower"""
    rng = np.random.default_rng(seed)
    t = np.stack([rng.uniform(0.0, 1.2, K), rng.uniform(-0.05, 0.5, K), rng.uniform(-0.5, 1.2, K), rng.uniform(-0.35, 0.35, K)], axis=1)
    t[0] = [1, 0, 1, 0]
    for a, b in twice:
        t[b] = t[a]
    assert np.unique(t, axis=0).shape[0] == K - len(twice)
    return np.ascontiguousarray(t, np.float64)


# K, ticks, table: 130 rows are three strides of the pick's lanes (candidate 129 repeats 70: a tie behind the first stride);
# 64 distinct candidates over 40 ticks
WIDE = {"130x7": ("async", 130, 7, dict(seed=21, twice=((70, 129),))), "64x40": ("cvp", 64, 40, dict(seed=22))}


@pytest.mark.parametrize("name", list(WIDE))
def test_wide_tables_with_distinct_scores(worlds, shim, name):
    """K = 130 and K = 64 with candidates that all differ, 7 and 40 ticks, with goals: the scores of a robot's rows differ from
    lane to lane and from stride to stride of k_sample_pick, and the whole branch list holds.  The reference is the compiled
    host mirror (smp_run of mnav_sample.h, which tests/test_sample_model.py holds to the model): the numpy model would take
    a minute for 8 710 rows; it checks the picks of the mirror's rows here."""
    kind, K, ticks, how = WIDE[name]
    w = worlds(kind)
    cfg = FM.config()
    robots, goals = w.fleet(42 if kind == "cvp" else 40, 3, 40)
    tab = distinct_table(K, **how)
    slots = np.unique(robots["slot"])
    compact = dict(robots, slot=np.searchsorted(slots, robots["slot"]).astype(np.uint32))
    mirror = Mirror(shim, w.model)
    want = mirror.sample(cfg, [w.fields[int(s)] for s in slots], [w.pots[int(s)] for s in slots], compact, goals, tab, DT, ticks, DIST_TOL, ANG_TOL, SAMPLE)
    mirror.close()
    for i in range(want["best_k"].shape[0]):                          # the model's pick over the mirror's rows
        k, J, cmd, cnt = SM.pick(want["status"][i], want["lethal"][i], want["score"][i], want["cmd0"][i])
        assert (k, cnt) == (int(want["best_k"][i]), int(want["n_feasible"][i])) and FM.same_bits(np.array([J, *cmd]), np.array([want["best_score"][i], *want["best_cmd"][i]]))
    got = w.sample_device(cfg, robots, goals, tab, ticks)
    print(name, "status:", np.bincount(want["status"].reshape(-1), minlength=4), "lethal:", int(want["lethal"].sum()), "best_k:", want["best_k"], "how:", want["how"])
    SM.assert_same(got, want, name)
    check_stats(w.ctx, want)
    SM.assert_every_branch(want, name)
    assert want["how"][1] > 0 and want["how"][2] > 0 and want["how"][3] > 0
    # picks in every stride of the lanes, and robots whose feasible rows all differ in J
    best = want["best_k"][want["best_k"] != SM.NONE]
    assert (best >= 64).any() or K == 64
    assert np.unique(best).size >= 6
    spread = [np.unique(want["score"][i][np.isfinite(want["score"][i])]).size for i in range(want["score"].shape[0])]
    assert max(spread) >= K - 2
    if K == 130:
        assert FM.same_bits(got["score"][:, 129], got["score"][:, 70]) and not (got["best_k"] == 129).any()


def test_the_follower_candidate_equals_the_rollout(case):
    """K = 1, candidate (1, 0, 1, 0): the rows are mnav_follow_rollout's robots, device against device"""
    w, cfg, robots, goals, tab, ticks, want = case("cvp")
    assert tab.tolist() == [[1.0, 0.0, 1.0, 0.0]]
    got = w.sample_device(cfg, robots, goals, tab, ticks)
    ref = w.device_run(cfg, robots, goals, ticks, trace_stride=0)
    for a, b in (("status", "status"), ("ticks", "ticks"), ("pos", "pos"), ("travel", "travel"), ("cost_integral", "cost_integral")):
        assert FM.same_bits(got[a][:, 0], getattr(ref, b)), a
    assert len(set(ref.status.tolist())) == 4 and (ref.ticks == ticks).any()


def test_three_hundred_ticks_span_two_blocks(worlds):
    w = worlds("async")
    cfg = FM.config()
    robots, goals = w.fleet(40, 0, 8, close=3)
    goals[0][::2, 0] += 50.0                                          # half of them never arrive
    tab = TABLE5[[0, 2, 4]]
    want = w.sample_model(cfg, robots, goals, tab, 300)
    got = w.sample_device(cfg, robots, goals, tab, 300)
    SM.assert_same(got, want, "300 ticks")
    check_stats(w.ctx, want)
    assert (want["ticks"] > 256).any() and (want["ticks"] < 256).any()


def test_the_second_trip_of_the_search_pass(worlds, shim):
    """40 robots x 64 candidates under slow_wide, every robot given a face a short way off the one it stands in: at tick 1 all
    2 560 rows need the neighbour search, more than the 2 048 workgroups of the search pass.  Against the compiled host mirror
    (smp_run of mnav_sample.h through tests/test_sample_model.py)."""
    w = worlds("single")
    cfg = CONFIGS["slow_wide"]
    rng = np.random.default_rng(5)
    m = w.model
    n = 40
    cen = m.xyz[m.faces].astype(np.float64).mean(axis=1)
    inner = np.nonzero(np.linalg.norm(cen[:, :2] - cen[:, :2].mean(axis=0), axis=1) < 1.5)[0]
    f = rng.choice(inner, n)
    given = np.array([rng.choice(np.nonzero((np.linalg.norm(cen - cen[j], axis=1) > 0.12) & (np.linalg.norm(cen - cen[j], axis=1) < 0.3))[0]) for j in f], np.uint32)
    a = rng.uniform(0, 2 * np.pi, n)
    robots = dict(pos=FM.face_points(m, f, rng).astype(np.float32), dir=np.stack([np.cos(a), np.sin(a), np.zeros(n)], axis=1).astype(np.float32),
                  up=np.tile(np.array([0, 0, 1], np.float32), (n, 1)), face_in=given, slot=np.zeros(n, np.uint32), seed_face=None)
    for name, store in (("vecmap", w.fields), ("dist", w.pots)):
        if 0 not in store:
            store[0] = w.ctx.download_output(name, 0)
    tab = table(64, 64, seed=9)
    mirror = Mirror(shim, m)
    tick1 = mirror.sample(cfg, [w.fields[0]], [w.pots[0]], robots, None, tab, DT, 1, sample=SAMPLE)
    want = mirror.sample(cfg, [w.fields[0]], [w.pots[0]], robots, None, tab, DT, 5, sample=SAMPLE)
    mirror.close()
    print("tick 1 how:", tick1["how"], "5 ticks:", want["how"], "status:", np.bincount(want["status"].reshape(-1), minlength=4))
    assert tick1["how"][3] + tick1["how"][4] == n * 64 > 2048 and tick1["how"][3] > 2048
    got = w.sample_device(cfg, robots, None, tab, 5)
    SM.assert_same(got, want, "40 x 64 rows")
    check_stats(w.ctx, want)


def test_a_candidate_that_stands_twice_is_picked_at_its_first_place(case):
    w, cfg, robots, goals, _, _, _ = case("async")
    spin = [0.0, 0.0, 0.0, 0.3]
    tab = np.array([spin] * 10, np.float64)
    tab[3] = tab[9] = [1, 0, 1, 0]                                    # the follower, twice, among candidates that turn on the spot
    tab[5] = [0.5, 0, 1, 0]
    got = w.sample_device(cfg, robots, goals, tab, 12)
    for k in SM.ROWS:
        assert FM.same_bits(got[k][:, 9], got[k][:, 3]), k
    assert not (got["best_k"] == 9).any() and (got["best_k"] == 3).any()
    tied = FM.same_bits(got["score"][:, 3], got["score"][:, 9]) and (got["n_feasible"] >= 2).any()
    assert tied


def test_null_row_outputs_and_identical_calls(case):
    w, cfg, robots, goals, tab, ticks, want = case("async")
    a = w.sample_device(cfg, robots, goals, tab, ticks)
    st = w.ctx.sample_stats()
    b = w.sample_device(cfg, robots, goals, tab, ticks)
    for k in SM.PICKS + SM.ROWS:                                      # two identical calls: identical bytes
        assert a[k].tobytes() == b[k].tobytes(), k
    st2 = w.ctx.sample_stats()
    assert {k: v for k, v in st.items() if not k.startswith("ms_")} == {k: v for k, v in st2.items() if not k.startswith("ms_")}
    only = w.sample_device(cfg, robots, goals, tab, ticks, outputs=SM.PICKS)
    assert all(only[k] is None for k in SM.ROWS)
    SM.assert_same(only, want, "picks only", keys=SM.PICKS)
    some = w.sample_device(cfg, robots, goals, tab, ticks, outputs=("best_k", "score", "lethal"))
    assert some["best_score"] is None and some["pos"] is None
    SM.assert_same(some, want, "three outputs", keys=("best_k", "score", "lethal"))
    empty = w.ctx.follow_sample(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), np.zeros(0), tab)
    assert empty["best_k"].shape == (0,) and empty["status"].shape == (0, 5) and not empty["cancelled"]


def test_refusals_touch_nothing(case):
    w, cfg, robots, goals, tab, ticks, want = case("async")
    ctx = w.ctx
    n = robots["pos"].shape[0]
    w.device_run(cfg, robots, goals, 4, trace_stride=0)
    rstats0, sstats0, field0 = ctx.rollout_stats(), ctx.sample_stats(), ctx.download_output("dist", 1)
    sentinel = dict(best_k=np.full(n, 0xABCDEF01, np.uint32), best_score=np.full(n, -7.0), status=np.full((n, tab.shape[0]), -7, np.int32))
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    RC, SC = capi.RolloutConfig, capi.SampleConfig

    def call(fc=None, ro=None, sa=None, slots=robots["slot"], face_in=robots["face_in"], gp=goals[0], gd=goals[1], tb=tab, K=None, null_cfg=False, null_ro=False,
             null_sa=False, pos=robots["pos"]):
        fc = fc if fc is not None else capi.FollowConfig(**cfg)
        ro = ro if ro is not None else RC(dt=DT, ticks=4)
        sa = sa if sa is not None else SC(**SAMPLE)
        return ctx._L.mnav_follow_sample(ctx._h, n, p(pos), p(robots["dir"]), p(robots["up"]), p(face_in), p(slots), None, p(gp), p(gd), None if null_cfg else C.byref(fc),
                                         None if null_ro else C.byref(ro), tab.shape[0] if K is None else K, p(tb), None if null_sa else C.byref(sa),
                                         p(sentinel["best_k"]), p(sentinel["best_score"]), None, None, p(sentinel["status"]), None, None, None, None, None, None, None)

    def with_entry(j, v):
        t = tab.copy()
        t.reshape(-1)[j] = v
        return t

    bad_face = robots["face_in"].copy()
    bad_face[5] = w.model.F
    inf, nan = float("inf"), float("nan")
    wide = tab.copy()
    wide[2] = [1, 0, 50.0, 0]                                          # 50 * 0.5 rad/s * 4 s = 100 rad
    refusals = [
        # every refusal of mnav_follow_rollout
        (dict(pos=None), "null"), (dict(null_cfg=True), "null"), (dict(null_ro=True), "null"),
        (dict(slots=np.full(n, w.n_plans, np.uint32)), "slot out of range"), (dict(face_in=bad_face), "face id out of range"),
        (dict(fc=capi.FollowConfig(max_search_radius=0.0)), "max_search_radius"), (dict(fc=capi.FollowConfig(max_search_distance=inf)), "max_search_distance"),
        (dict(ro=RC(dt=0.0, ticks=4)), "dt"), (dict(ro=RC(dt=nan, ticks=4)), "dt"), (dict(ro=RC(dt=DT, ticks=0)), "ticks"), (dict(ro=RC(dt=DT, ticks=100001)), "ticks"),
        (dict(gd=None), "goal"), (dict(gp=None), "goal"), (dict(ro=RC(dt=DT, ticks=4, dist_tolerance=nan)), "tolerance"),
        (dict(fc=capi.FollowConfig(max_ang_velocity=400.0)), "100"),
        # the call's own
        (dict(ro=RC(dt=DT, ticks=4, trace_stride=1)), "trace_stride"), (dict(ro=RC(dt=DT, ticks=4, trace_stride=5)), "trace_stride"),
        (dict(K=0), "no candidates"), (dict(tb=None), "no candidates"),
        (dict(tb=with_entry(0, inf)), "gain or bias"), (dict(tb=with_entry(5, nan)), "gain or bias"), (dict(tb=with_entry(18, -inf)), "gain or bias"),
        (dict(sa=SC(**dict(SAMPLE, w_potential=-1e-9))), "weight"), (dict(sa=SC(**dict(SAMPLE, w_cost=inf))), "weight"), (dict(sa=SC(**dict(SAMPLE, w_time=nan))), "weight"),
        (dict(sa=SC(**dict(SAMPLE, lethal_cost=nan))), "lethal_cost"), (dict(sa=SC(**dict(SAMPLE, flags=1))), "flags"), (dict(null_sa=True), "null"),
        (dict(K=(1 << 28) // n + 1), "2^28"),
        (dict(tb=wide, ro=RC(dt=4.0, ticks=4)), "100 rad"), (dict(tb=with_entry(7, -25.0), ro=RC(dt=4.0, ticks=4)), "100 rad"),
    ]
    for kw, text in refusals:
        assert call(**kw) == -1 and text in ctx._err(), (kw, ctx._err())
        assert (sentinel["best_k"] == 0xABCDEF01).all() and (sentinel["best_score"] == -7.0).all() and (sentinel["status"] == -7).all(), kw
        assert ctx.rollout_stats() == rstats0 and ctx.sample_stats() == sstats0, kw
    assert np.array_equal(ctx.download_output("dist", 1).view(np.uint32), field0.view(np.uint32))
    # just inside the bounds: served (lethal_cost = +inf, a weight of 0, 24.9 rad/s of bias at dt = 4)
    assert call(sa=SC(w_potential=0.0, w_cost=0.0, w_time=0.0, lethal_cost=inf)) == 0 and (sentinel["best_k"] != 0xABCDEF01).all() and (sentinel["status"] != -7).all()
    assert call(tb=with_entry(7, -24.4), ro=RC(dt=4.0, ticks=2)) == 0
    # a served call leaves the rollout's record alone and changes no plan output
    assert ctx.rollout_stats() == rstats0 and ctx.sample_stats() != sstats0
    assert np.array_equal(ctx.download_output("dist", 1).view(np.uint32), field0.view(np.uint32))


def test_a_call_after_a_rollout_leaves_its_statistics(case):
    w, cfg, robots, goals, tab, ticks, want = case("async")
    w.device_run(cfg, robots, goals, 9)
    rs, fs, ps = w.ctx.rollout_stats(), w.ctx.follow_stats(), w.ctx.stats()
    w.sample_device(cfg, robots, goals, tab, ticks)
    assert w.ctx.rollout_stats() == rs and w.ctx.follow_stats() == fs and w.ctx.stats() == ps and rs["robot_ticks"] > 0
    # ... and the rollout after it is what it was
    ref = w.model_run(cfg, robots, goals, 9)
    RM.assert_same(w.device_run(cfg, robots, goals, 9), ref, "rollout after a sampled rollout")


def test_a_cancel_set_before_the_call_ends_it(case):
    w, cfg, robots, goals, tab, ticks, want = case("async")
    n = robots["pos"].shape[0]
    w.ctx.cancel()
    ctx = w.ctx
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    best_k, status = np.full(n, 0xABCDEF01, np.uint32), np.full((n, tab.shape[0]), -7, np.int32)
    fc, ro, sa = capi.FollowConfig(**cfg), capi.RolloutConfig(dt=DT, dist_tolerance=DIST_TOL, angle_tolerance=ANG_TOL, ticks=ticks), capi.SampleConfig(**SAMPLE)
    rc = ctx._L.mnav_follow_sample(ctx._h, n, p(robots["pos"]), p(robots["dir"]), p(robots["up"]), p(robots["face_in"]), p(robots["slot"]), None, p(goals[0]), p(goals[1]),
                                   C.byref(fc), C.byref(ro), tab.shape[0], p(tab), C.byref(sa), p(best_k), None, None, None, p(status), None, None, None, None, None, None, None)
    assert rc == 1 and (best_k == 0xABCDEF01).all() and (status == -7).all()      # cancelled: no pick, no row
    st = ctx.sample_stats()
    assert (st["feasible_rows"], st["lethal_rows"], st["robots_without_pick"], st["row_ticks"]) == (0, 0, 0, 0)      # ended before its first tick
    # the call that honoured the flag took it down: the next one runs to its end
    got = w.sample_device(cfg, robots, goals, tab, ticks)
    assert not got["cancelled"]
    SM.assert_same(got, want, "after the cancelled call")
