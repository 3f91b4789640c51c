"""The yielding fleet rollout on the device (mnav_fleet_rollout_yield, mnav_fleet_yield_stats) against tests/yield_model.py,
the tick-synchronous O(n^2) numpy restatement of include/mnav.h: the state, the separation rows, the yield rows, the flags
after the last check and the statistics, every output by its bits, over converging fleets of 2, 65 and 257 robots for 260
ticks (a block of 256 ticks of the tick loop and 4) on the asynchronous engine's fields and on a CVP batch's; the guard; runs
repeated and at other cell scales; refusals; yield = NULL against mnav_fleet_rollout; the statistics records kept apart; and
a rollout resumed through hold_out and hold_in.  On the worlds of tests/test_gpu_rollout.py."""
import ctypes as C

import numpy as np
import pytest

from mesh_navigation_amd import capi
from tests import follow_model as FM
from tests import locate_model as LM
from tests import rollout_model as RM
from tests import separation_model as SM
from tests import yield_model as YM
from tests.test_gpu_fleet_rollout import fleet_run
from tests.test_gpu_rollout import World
from tests.test_rollout_model import ANG_TOL, DIST_TOL, DT
from tests.test_separation_model import converging_fleet, starts
from tests.test_yield_model import YieldMirror, build_shim

pytestmark = pytest.mark.gpu

F32 = np.float32
RADIUS, AHEAD_COS, TICKS = 0.3, 0.5, 260
STATE = RM.KEYS + ("trace",)


@pytest.fixture(scope="module")
def worlds(gpu_ctx_factory):
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = World(gpu_ctx_factory(), kind)
        return made[kind]

    return get


def priorities(n):
    """four classes, not in index order"""
    return ((np.arange(n) * 7 + 3) % 4).astype(np.uint32)


def yield_run(w, robots, goals, ticks, start_tick=None, separation=None, yield_config=None, priority=None, hold_in=None, trace_stride=1, outputs=None, cfg=None):
    ro = capi.RolloutConfig(dt=DT, dist_tolerance=DIST_TOL, angle_tolerance=ANG_TOL, ticks=ticks, trace_stride=trace_stride)
    g = (None, None) if goals is None else goals
    return w.ctx.fleet_rollout_yield(robots["pos"], robots["dir"], robots["up"], robots["face_in"], robots["slot"], robots.get("seed_face"), g[0], g[1],
                                     capi.FollowConfig(**(cfg or FM.config())), ro, start_tick, separation, yield_config, priority, hold_in, outputs)


def fleet_of(w, n):
    """converging_fleet on world w; the CVP world's robots carry their plans' seed faces"""
    robots, goals = converging_fleet(w, n)
    return robots, goals, starts(n)


@pytest.fixture(scope="module")
def model_runs(worlds):
    """the model's run of a fleet, computed once per case"""
    made = {}

    def get(kind, n, check_stride, flags, with_priority, ticks=TICKS, skip_checks=()):
        key = (kind, n, check_stride, flags, with_priority, ticks, skip_checks)
        if key not in made:
            w = worlds(kind)
            robots, goals, start = fleet_of(w, n)
            prio = priorities(n) if with_priority else None
            made[key] = (robots, goals, start, prio, YM.run(w.model, FM.config(), w.fields, robots, goals, DT, ticks, DIST_TOL, ANG_TOL, start, RADIUS, check_stride,
                                                           flags, AHEAD_COS, prio, skip_checks=skip_checks))
        return made[key]

    return get


def assert_equals_model(got, want, check_stride, what):
    RM.assert_same(got, want, (what, "state"), keys=RM.KEYS)
    assert FM.same_bits(got.trace, SM.thin(want["trace"], check_stride)), what
    SM.assert_same_rows(got, want, (what, "separation"))
    YM.assert_same_yield(got, want, (what, "yield"))


def check_stats(ctx, want):
    st = ctx.fleet_yield_stats()
    for k, v in want["stats"].items():
        assert st[k] == v, (k, st, want["stats"])
    assert 0 < st["ms_pair"] < st["ms_separation"] < st["ms_kernels"] <= st["ms_total"], st
    return st


# 2 robots; 65: one past a wave; 257: one past the stay pass's workgroup and the pair pass's; 260 ticks: checks in both blocks of
# the tick loop (stride 7: 252 and 259); the four presence flags at 65; with and without priorities; two kinds of fields
CASES = [("async", 2, 1, 3, False), ("async", 65, 1, 0, True), ("async", 65, 7, 1, False), ("async", 65, 7, 2, True), ("async", 65, 1, 3, False),
         ("async", 257, 7, 3, True), ("async", 257, 1, 0, False), ("cvp", 65, 7, 3, True), ("cvp", 65, 1, 0, False)]


@pytest.mark.parametrize("kind,n,check_stride,flags,with_priority", CASES)
def test_the_device_equals_the_model(worlds, model_runs, kind, n, check_stride, flags, with_priority):
    w = worlds(kind)
    robots, goals, start, prio, want = model_runs(kind, n, check_stride, flags, with_priority)
    print(kind, n, check_stride, flags, with_priority, "status:", np.bincount(want["status"], minlength=4), want["stats"], "pairs:", int(want["pairs"].sum()))
    # conditions on the MODEL's output: somebody is held, somebody never is; in a fleet robots are released again and reach
    assert want["stats"]["robots_held"] >= 1 and want["stats"]["held_ticks"] > 0 and (want["hold_checks"] == 0).any()
    if n >= 65:
        first = np.array([np.nonzero(want["held_at"][:, i])[0][0] if want["hold_checks"][i] else 10 ** 6 for i in range(n)])
        later = np.array([want["had_tick"][i, min((first[i] + 1) * check_stride, TICKS):].any() for i in range(n)])
        assert later.sum() >= 3 and len(set(want["held_ticks"].tolist())) >= 5
        if not flags & SM.REACHED_PRESENT:                            # (a robot that stays where it REACHED blocks the others' way to the shared goal)
            assert ((want["status"] == RM.REACHED) & (want["hold_checks"] > 0)).any()
    sep = capi.SeparationConfig(radius=RADIUS, check_stride=check_stride, flags=flags)
    got = yield_run(w, robots, goals, TICKS, start_tick=start, separation=sep, yield_config=capi.YieldConfig(ahead_cos=AHEAD_COS), priority=prio,
                    trace_stride=check_stride)
    assert not got.cancelled and not got.skipped
    assert_equals_model(got, want, check_stride, (kind, n, check_stride, flags))
    check_stats(w.ctx, want)


def test_head_on_the_priorities_decide_on_the_device(worlds):
    """two robots of one plan that face each other 0.2 m apart: the one without right of way is held, and swapping the
    priorities swaps who is (conditions on the model's output; the device equals the model both ways)"""
    w = worlds("async")
    robots, goals, _ = fleet_of(w, 2)
    robots = {k: (None if v is None else np.array(v)) for k, v in robots.items()}
    robots["pos"][1] = robots["pos"][0] + F32(0.2) * robots["dir"][0]
    robots["dir"][1] = -robots["dir"][0]
    sep = capi.SeparationConfig(radius=RADIUS, check_stride=1, flags=0)
    held = []
    for prio in (np.array([0, 1], np.uint32), np.array([1, 0], np.uint32), None):
        want = YM.run(w.model, FM.config(), w.fields, robots, goals, DT, 12, DIST_TOL, ANG_TOL, None, RADIUS, 1, 0, AHEAD_COS, prio)
        got = yield_run(w, robots, goals, 12, separation=sep, yield_config=capi.YieldConfig(ahead_cos=AHEAD_COS), priority=prio)
        assert_equals_model(got, want, 1, prio)
        held.append(want["held_at"][0].tolist())
    print("held at the first check:", held)
    assert held == [[0, 1], [1, 0], [0, 1]]


@pytest.fixture(scope="module")
def mirror(worlds, tmp_path_factory):
    """mnav_fleet_yield.h on the host over the asynchronous world's mesh: T, the guard's count of a check, is a property of
    the grid, which the model does not have"""
    w = worlds("async")
    m = YieldMirror(build_shim(tmp_path_factory), w.model)
    yield m
    m.close()


def test_the_guard_releases_everybody_at_a_skipped_check(worlds, model_runs, mirror):
    """65 robots, stride 7, 42 ticks.  The host mirror tells T of every check; a bound one below the largest T among the
    checks after the first skips that check (the mirror, run with the bound, tells which checks the bound skips in the run
    that results), and the model runs with exactly those checks skipped."""
    w = worlds("async")
    ctx, ticks, stride = w.ctx, 42, 7
    robots, goals, start, prio, served = model_runs("async", 65, stride, 3, True, ticks)
    fields = [w.fields[s] for s in range(w.n_plans)]
    T = mirror.run_yield(FM.config(), fields, robots, goals, ticks, start_tick=start, check_stride=stride, flags=3, priority=prio)["chk"][:, 0].astype(np.int64)
    k = 1 + int(np.argmax(T[1:]))
    bound = int(T[k]) - 1
    chk = mirror.run_yield(FM.config(), fields, robots, goals, ticks, start_tick=start, check_stride=stride, flags=3, priority=prio, max_tests=bound)["chk"]
    skipped = tuple(int(t) for t in (np.nonzero(chk[:, 3])[0] + 1) * stride)
    print("T:", T, "bound:", bound, "skipped:", skipped)
    assert skipped and len(skipped) < ticks // stride
    want = model_runs("async", 65, stride, 3, True, ticks, skipped)[4]
    c = skipped[0] // stride - 1
    assert served["held_at"][c].any() and not want["held_at"][c].any()           # the served run holds somebody there; skipped, nobody is held
    assert want["stats"]["held_ticks"] < served["stats"]["held_ticks"]
    sep, yc = capi.SeparationConfig(radius=RADIUS, check_stride=stride, flags=3), capi.YieldConfig(ahead_cos=AHEAD_COS)
    try:
        ctx.set_option("separation_max_tests", bound)
        got = yield_run(w, robots, goals, ticks, start_tick=start, separation=sep, yield_config=yc, priority=prio, trace_stride=stride)
        assert got.skipped and not got.cancelled
        assert_equals_model(got, want, stride, ("skipped", skipped))
        st = check_stats(ctx, want)
        assert (st["checks_skipped"], st["first_skipped_tick"]) == (len(skipped), skipped[0])
        ctx.set_option("separation_max_tests", None)
        got = yield_run(w, robots, goals, ticks, start_tick=start, separation=sep, yield_config=yc, priority=prio, trace_stride=stride)
        assert not got.skipped
        assert_equals_model(got, served, stride, "served")
        # every check skipped: nobody is ever held, the motion is the fleet rollout's
        ctx.set_option("separation_max_tests", 0)
        free = yield_run(w, robots, goals, ticks, start_tick=start, separation=sep, yield_config=yc, priority=prio, trace_stride=stride)
        late = fleet_run(w, FM.config(), robots, goals, ticks, start_tick=start, trace_stride=stride)
        assert free.skipped and not free.hold.any() and not free.held_ticks.any() and (free.first_hold_tick == SM.NONE).all()
        RM.assert_same(free, {k: getattr(late, k) for k in STATE}, "every check skipped")
    finally:
        ctx.set_option("separation_max_tests", None)


def test_two_runs_and_other_cell_scales_give_the_same_bits(worlds, model_runs):
    w = worlds("async")
    robots, goals, start, prio, want = model_runs("async", 65, 1, 3, False)
    sep, yc = capi.SeparationConfig(radius=RADIUS, check_stride=1, flags=3), capi.YieldConfig(ahead_cos=AHEAD_COS)
    try:
        for scale in (None, None, 1.0, 4.0):
            w.ctx.set_option("separation_cell_scale", scale)
            again = yield_run(w, robots, goals, TICKS, start_tick=start, separation=sep, yield_config=yc)
            assert_equals_model(again, want, 1, scale)
            check_stats(w.ctx, want)
    finally:
        w.ctx.set_option("separation_cell_scale", None)


def test_a_narrow_cone_and_a_wide_one(worlds):
    """ahead_cos is used: 0 and 0.9 give other runs, each the model's"""
    w = worlds("async")
    robots, goals, start = fleet_of(w, 65)
    sep = capi.SeparationConfig(radius=RADIUS, check_stride=7, flags=3)
    seen = []
    for c in (0.0, 0.9):
        want = YM.run(w.model, FM.config(), w.fields, robots, goals, DT, 70, DIST_TOL, ANG_TOL, start, RADIUS, 7, 3, c)
        got = yield_run(w, robots, goals, 70, start_tick=start, separation=sep, yield_config=capi.YieldConfig(ahead_cos=c), trace_stride=7)
        assert_equals_model(got, want, 7, c)
        seen.append(want["stats"]["held_ticks"])
    assert seen[0] > seen[1] > 0


def test_without_a_yield_config_it_is_the_fleet_rollout(worlds, model_runs):
    w = worlds("async")
    robots, goals, start, prio, _ = model_runs("async", 65, 7, 3, True)
    sep = capi.SeparationConfig(radius=RADIUS, check_stride=7, flags=3)
    for kw in (dict(start_tick=start, separation=sep, trace_stride=7), dict(separation=sep), dict(start_tick=start), dict()):
        want = fleet_run(w, FM.config(), robots, goals, TICKS, **kw)
        fs, rs = w.ctx.fleet_rollout_stats(), w.ctx.rollout_stats()
        got = yield_run(w, robots, goals, TICKS, **kw)
        RM.assert_same(got, {k: getattr(want, k) for k in STATE}, sorted(kw))
        if "separation" in kw:
            SM.assert_same_rows(got, {k: getattr(want, k) for k in SM.SEP_KEYS}, sorted(kw))
        else:
            assert got.near_checks is None
        assert got.hold is None and got.held_ticks is None and got.skipped == want.skipped
        ys = w.ctx.fleet_yield_stats()
        assert (ys["robots_held"], ys["held_ticks"], ys["max_held"], ys["held_last"], ys["ms_pair"]) == (0, 0, 0, 0, 0) and ys["ms_kernels"] > 0
        assert w.ctx.fleet_rollout_stats() == fs and w.ctx.rollout_stats() == rs           # the other entry points' records are left alone
    # a radius that finds nobody: the state and separation outputs of the call without the rule, the yield rows at their start
    tiny = capi.SeparationConfig(radius=1e-4, check_stride=7, flags=0)
    want = fleet_run(w, FM.config(), robots, goals, TICKS, start_tick=start, separation=tiny, trace_stride=7)
    got = yield_run(w, robots, goals, TICKS, start_tick=start, separation=tiny, yield_config=capi.YieldConfig(ahead_cos=AHEAD_COS), priority=prio, trace_stride=7)
    RM.assert_same(got, {k: getattr(want, k) for k in STATE}, "nobody near")
    SM.assert_same_rows(got, {k: getattr(want, k) for k in SM.SEP_KEYS}, "nobody near")
    assert (got.near_checks == 0).all()
    YM.assert_same_yield(got, dict(YM.start_yrows(65), hold=np.zeros(65, np.uint8)), "start values")


def test_the_statistics_records_are_kept_apart(worlds, model_runs):
    w = worlds("async")
    ctx = w.ctx
    robots, goals, start, prio, want = model_runs("async", 65, 7, 3, True)
    sep, yc = capi.SeparationConfig(radius=RADIUS, check_stride=7, flags=3), capi.YieldConfig(ahead_cos=AHEAD_COS)
    w.device_run(FM.config(), robots, goals, 5, trace_stride=0)
    fleet_run(w, FM.config(), robots, goals, 9, start_tick=start, separation=sep, trace_stride=0)
    rs, fs = ctx.rollout_stats(), ctx.fleet_rollout_stats()
    yield_run(w, robots, goals, TICKS, start_tick=start, separation=sep, yield_config=yc, priority=prio, trace_stride=0)
    ys = check_stats(ctx, want)
    assert ctx.rollout_stats() == rs and ctx.fleet_rollout_stats() == fs and rs["robot_ticks"] > 0 and fs["checks_run"] == 1
    # ... and the other way round
    w.device_run(FM.config(), robots, goals, 3, trace_stride=0)
    assert ctx.fleet_yield_stats() == ys and ctx.rollout_stats() != rs
    fleet_run(w, FM.config(), robots, goals, 14, start_tick=start, separation=sep, trace_stride=0)
    assert ctx.fleet_yield_stats() == ys and ctx.fleet_rollout_stats()["checks_run"] == 2


def test_refusals_touch_nothing(worlds):
    w = worlds("async")
    ctx = w.ctx
    robots, goals, start = fleet_of(w, 65)
    n = 65
    SC, YC, RC = capi.SeparationConfig, capi.YieldConfig, capi.RolloutConfig
    yield_run(w, robots, goals, 4, separation=SC(radius=RADIUS), yield_config=YC())
    field0, stats0, ys0, fs0, rs0 = ctx.download_output("vecmap", 1), ctx.stats(), ctx.fleet_yield_stats(), ctx.fleet_rollout_stats(), ctx.rollout_stats()
    sentinel = dict(status=np.full(n, -7, np.int32), pos=np.full((n, 3), -7.0, F32), trace=np.full((n, 4, 3), -7.0, F32), near_checks=np.full(n, 7, np.uint32),
                    hold=np.full(n, 7, np.uint8), hold_checks=np.full(n, 7, np.uint32), held_ticks=np.full(n, 7, np.uint32), first_hold_tick=np.full(n, 7, np.uint32),
                    first_hold_robot=np.full(n, 7, np.uint32))
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    prio, hold_in = priorities(n), np.zeros(n, np.uint8)

    def call(ro=None, sep=SC(radius=RADIUS), no_sep=False, yc=YC(), no_yield=False, pos=robots["pos"], priority=None, hin=None, outs=True, hold_out=True):
        ro = ro if ro is not None else RC(dt=DT, ticks=4, trace_stride=1)
        fc = capi.FollowConfig(**FM.config())
        y_outs = [p(sentinel[k]) if outs else None for k in ("hold_checks", "held_ticks", "first_hold_tick", "first_hold_robot")]
        return ctx._L.mnav_fleet_rollout_yield(ctx._h, n, p(pos), p(robots["dir"]), p(robots["up"]), p(robots["face_in"]), p(robots["slot"]), None, p(goals[0]), p(goals[1]),
                                               C.byref(fc), C.byref(ro), p(start), None if no_sep else C.byref(sep), p(sentinel["status"]), None, p(sentinel["pos"]),
                                               None, None, None, None, None, p(sentinel["trace"]), None if no_sep else p(sentinel["near_checks"]), None, None, None,
                                               None, None, None, None if no_yield else C.byref(yc), p(priority), p(hin), p(sentinel["hold"]) if hold_out else None, *y_outs)

    refusals = [
        # those of mnav_fleet_rollout
        (dict(pos=None), "null"), (dict(ro=RC(dt=0.0, ticks=4)), "dt"), (dict(ro=RC(dt=DT, ticks=4, trace_stride=5)), "trace_stride"),
        (dict(sep=SC(radius=0.0)), "radius"), (dict(sep=SC(radius=RADIUS, check_stride=5)), "check_stride"), (dict(sep=SC(radius=RADIUS, flags=4)), "flag"),
        # the rule's own
        (dict(no_sep=True), "without a separation"),
        (dict(yc=YC(ahead_cos=1.0)), "ahead_cos"), (dict(yc=YC(ahead_cos=-0.1)), "ahead_cos"), (dict(yc=YC(ahead_cos=float("nan"))), "ahead_cos"),
        (dict(yc=YC(ahead_cos=float("inf"))), "ahead_cos"), (dict(yc=YC(ahead_cos=1.0 - 1e-12)), "ahead_cos"), (dict(yc=YC(ahead_cos=2.0)), "ahead_cos"),
        (dict(yc=YC(flags=1)), "reserved"), (dict(yc=YC(flags=0x80000000)), "reserved"),
        (dict(no_yield=True), "without a yield config"), (dict(no_yield=True, outs=False), "without a yield config"),
        (dict(no_yield=True, outs=False, hold_out=False, priority=prio), "without a yield config"),
        (dict(no_yield=True, outs=False, hold_out=False, hin=hold_in), "without a yield config"),
    ]
    for kw, text in refusals:
        assert call(**kw) == -1 and text in ctx._err(), (kw, ctx._err())
        assert all((v == (-7 if v.dtype.kind in "if" and v.dtype != np.uint32 and v.dtype != np.uint8 else 7)).all() for v in sentinel.values()), kw
    assert np.array_equal(LM.bits(ctx.download_output("vecmap", 1)), LM.bits(field0)) and ctx.stats() == stats0
    assert ctx.fleet_yield_stats() == ys0 and ctx.fleet_rollout_stats() == fs0 and ctx.rollout_stats() == rs0
    # served: the largest cosine below 1, NULL outputs, yield = NULL with every yield pointer NULL, n = 0
    assert call(yc=YC(ahead_cos=float(np.nextafter(F32(1), F32(0))))) == 0 and (sentinel["status"] != -7).all() and (sentinel["hold"] <= 1).all()
    assert (sentinel["hold_checks"] <= 4).all() and (sentinel["held_ticks"] <= 4).all()
    assert call(outs=False, hold_out=False, priority=prio, hin=hold_in) == 0
    assert call(no_yield=True, outs=False, hold_out=False) == 0
    empty = ctx.fleet_rollout_yield(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), np.zeros(0), separation=SC(radius=RADIUS), yield_config=YC())
    assert empty.status.shape == (0,) and empty.hold.shape == (0,) and not empty.skipped
    only = yield_run(w, robots, goals, 4, separation=SC(radius=RADIUS), yield_config=YC(), trace_stride=0, outputs=("status", "held_ticks"))
    assert only.pos is None and only.hold is None and only.near_checks is None and only.held_ticks is not None and only.status is not None


def test_two_calls_through_hold_out_and_hold_in_equal_one(worlds, model_runs):
    """a + b ticks with a a multiple of the stride, presence flags 0.  Every robot that can still be present is fed back: the
    RUNNING ones, which the comparison is about, and the stranded ones, which strand again at their first tick where they
    stood.  A REACHED robot is not present under these flags and is left out."""
    w = worlds("async")
    stride, a, b = 7, 28, 42
    robots, goals, start, prio, _ = model_runs("async", 65, stride, 0, True)
    sep, yc = capi.SeparationConfig(radius=RADIUS, check_stride=stride, flags=0), capi.YieldConfig(ahead_cos=AHEAD_COS)
    whole = yield_run(w, robots, goals, a + b, start_tick=start, separation=sep, yield_config=yc, priority=prio, trace_stride=stride)
    first = yield_run(w, robots, goals, a, start_tick=start, separation=sep, yield_config=yc, priority=prio, trace_stride=stride)
    keep = np.nonzero(first.status != RM.REACHED)[0]
    run = first.status[keep] == RM.RUNNING
    assert first.hold[keep][run].any() and not first.hold[keep][run].all() and 0 < keep.size < 65
    sub = {k: (None if v is None else v[keep]) for k, v in robots.items()}
    sub.update(pos=first.pos[keep], dir=first.dir[keep], face_in=first.face[keep])
    left = np.maximum(start[keep].astype(np.int64) - a, 0).astype(np.uint32)
    second = yield_run(w, sub, (goals[0][keep], goals[1][keep]), b, start_tick=left, separation=sep, yield_config=yc, priority=prio[keep], hold_in=first.hold[keep],
                       trace_stride=stride)
    for k in ("status", "pos", "dir", "face", "hold"):
        assert FM.same_bits(getattr(second, k)[run], getattr(whole, k)[keep][run]), k
    for k in ("ticks", "held_ticks", "hold_checks"):
        assert np.array_equal((getattr(first, k)[keep] + getattr(second, k))[run], getattr(whole, k)[keep][run]), k
    assert FM.same_bits(np.concatenate([first.trace[keep], second.trace], axis=1)[run], whole.trace[keep][run])
    assert second.held_ticks[run].any() and (second.ticks[run] > 0).any()
    # without hold_in the second call is another run: the robots that were held drive until its first check
    loose = yield_run(w, sub, (goals[0][keep], goals[1][keep]), b, start_tick=left, separation=sep, yield_config=yc, priority=prio[keep], trace_stride=stride)
    assert not FM.same_bits(loose.trace[run], second.trace[run])
