"""The wait-for analysis on the device (mnav_fleet_rollout_rings, mnav_fleet_ring_stats) against tests/ring_model.py, which
walks every chain with a visited set: the state, the separation rows, the yield rows, the ring rows, the classes and anchors
of the last check and the statistics, every output by its bits.  One fleet of 177 robots -- a converging fleet of 65, a
triangle, a ring of 67 (it crosses a wave), a ring of 5 with a tail of 3 and a line of 33 behind a robot that waits and is kept
present -- for 260 ticks (a block of 256 ticks of the tick loop and 4) at check strides 1 and 7, with and without priorities,
with and without the release, on the asynchronous engine's fields and on a CVP batch's; one of a ring of 257 and a line of 130
(one past the pair pass's workgroup, depth 129, nine rounds of the doubling); the equivalences of the header; the guard;
refusals; the statistics records kept apart; and a rollout resumed through hold_out and hold_in.  On the worlds of
tests/test_gpu_rollout.py."""
import ctypes as C

import numpy as np
import pytest

from mesh_navigation_amd import capi
from tests import follow_model as FM
from tests import locate_model as LM
from tests import ring_model as RG
from tests import rollout_model as RM
from tests import separation_model as SM
from tests import yield_model as YM
from tests.test_gpu_fleet_rollout import fleet_run
from tests.test_gpu_fleet_yield import priorities, yield_run
from tests.test_gpu_rollout import World
from tests.test_ring_model import RingMirror, build_shim, circle, line, place, ring_with_tail
from tests.test_rollout_model import ANG_TOL, DIST_TOL, DT
from tests.test_separation_model import converging_fleet, starts

pytestmark = pytest.mark.gpu

F32 = np.float32
NONE = SM.NONE
# the mesh is a few metres wide: the structures are built at a spacing of 0.05 under a radius of 0.075 (the second robot ahead
# is 0.1 away).  Cosine 0.25: the next robot of a triangle with tangent headings sits exactly on the cone of cosine 0.5
RADIUS, SPACING, AHEAD_COS, TICKS = 0.075, 0.05, 0.25, 260
STATE = RM.KEYS + ("trace",)
SLOW = FM.config(max_lin_velocity=0.2)


@pytest.fixture(scope="module")
def worlds(gpu_ctx_factory):
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = World(gpu_ctx_factory(), kind)
        return made[kind]

    return get


def rings_run(w, robots, goals, ticks, start_tick=None, separation=None, yield_config=None, priority=None, hold_in=None, ring_config=None, trace_stride=1, outputs=None,
              cfg=None):
    ro = capi.RolloutConfig(dt=DT, dist_tolerance=DIST_TOL, angle_tolerance=ANG_TOL, ticks=ticks, trace_stride=trace_stride)
    g = (None, None) if goals is None else goals
    return w.ctx.fleet_rollout_rings(robots["pos"], robots["dir"], robots["up"], robots["face_in"], robots["slot"], robots.get("seed_face"), g[0], g[1],
                                     capi.FollowConfig(**(cfg or FM.config())), ro, start_tick, separation, yield_config, priority, hold_in, ring_config, outputs)


def settle(w, shapes, keep_off=None, with_seed=False, slot=0, in_field=True, holes=False):
    """every shape -- a function of an angle that gives xy points about the origin and headings -- moved to a spot of the mesh
    where all its points lie on faces (in_field: faces whose corners have vectors in the field of plan `slot`), the spots far
    from the mesh's middle first and 0.4 m from each other and from keep_off.  The angle is such that the first robot of a
    circle heads straight away from the middle, where the fields lead: released, it has to turn before it drives.  Robots on
    plan `slot`, on their faces (with_seed: with that plan's seed face, as the robots of a CVP world carry it; holes: the mesh
    has holes, and only the first two robots of a structure need a face: the others may start without one)"""
    model = w.model
    if in_field and slot not in w.fields:
        w.fields[slot] = w.ctx.download_output("vecmap", slot)
    xyz = model.xyz.astype(np.float64)
    lo, hi, mid = np.nanmin(xyz, axis=0), np.nanmax(xyz, axis=0), np.nanmean(xyz, axis=0)
    gx, gy = np.meshgrid(np.arange(lo[0] + 0.1, hi[0], 0.15), np.arange(lo[1] + 0.1, hi[1], 0.15))
    spots = np.stack([gx.reshape(-1), gy.reshape(-1)], axis=1)
    spots = spots[np.argsort(-np.linalg.norm(spots - mid[None, :2], axis=1), kind="stable")]
    taken = np.zeros((0, 2)) if keep_off is None else np.asarray(keep_off, np.float64)[:, :2]
    seed_face = w.seed_faces[slot] if with_seed else None
    parts = []
    for shape in shapes:
        for c in spots:
            pos, d = shape(np.arctan2(c[1] - mid[1], c[0] - mid[0]) - np.pi / 2)
            q = pos[:, :2].astype(np.float64) + c[None, :]
            if (q < lo[None, :2] + 0.05).any() or (q > hi[None, :2] - 0.05).any():
                continue
            if taken.shape[0] and np.min(np.linalg.norm(q[:, None, :] - taken[None, :, :], axis=2)) < 0.4:
                continue
            try:
                part = place(model, q, slot=slot, seed_face=seed_face, holes=holes)
            except AssertionError:
                continue
            on_face = part["face_in"] != FM.NONE
            if not on_face[:2].all():
                continue
            if in_field:
                v = np.asarray(w.fields[slot], np.float64)[model.faces[part["face_in"][on_face]]]
                if not (np.isfinite(v).all() and (np.abs(v).sum(axis=-1) > 0).all()):
                    continue
            parts.append(dict(part, dir=np.array(d, F32)))
            taken = np.concatenate([taken, q])
            break
        else:
            raise AssertionError("no spot on the mesh for a structure")
    return parts


def join(robots, goals, parts):
    n0 = robots["pos"].shape[0]
    out = {}
    for k in robots:
        out[k] = None if robots[k] is None else np.concatenate([np.asarray(robots[k])] + [np.asarray(p[k]).astype(np.asarray(robots[k]).dtype) for p in parts])
    m = out["pos"].shape[0] - n0
    return out, (np.concatenate([goals[0], np.tile(goals[0][:1], (m, 1))]), np.concatenate([goals[1], np.tile(goals[1][:1], (m, 1))]))


def mixed_fleet(w):
    """the converging fleet of 65 and four structures, every constructed robot held at the start but the head of the line,
    which has not departed.  Returns robots, goals, start ticks, hold_in and the index ranges of the structures"""
    robots, goals = converging_fleet(w, 65)
    shapes = [lambda a: circle(3, SPACING, phase=a), lambda a: circle(67, SPACING, phase=a), lambda a: ring_with_tail(5, 3, SPACING, phase=a), lambda a: line(34, SPACING)]
    on_mesh = np.isfinite(robots["pos"]).all(axis=1) & (np.abs(robots["pos"][:, :2]) < 50).all(axis=1)
    parts = settle(w, shapes, keep_off=robots["pos"][on_mesh], with_seed=robots.get("seed_face") is not None, slot=w.n_plans - 1, holes=w.kind == "cvp")
    robots, goals = join(robots, goals, parts)
    n = robots["pos"].shape[0]
    start = np.concatenate([starts(65), np.zeros(n - 65, np.uint32)])
    hold_in = np.concatenate([np.zeros(65, np.uint8), np.ones(n - 65, np.uint8)])
    start[n - 1], hold_in[n - 1] = 100000, 0                         # the head of the line waits for good: WAITING_PRESENT keeps it
    at = np.cumsum([65, 3, 67, 8, 34])
    return robots, goals, start, hold_in, dict(triangle=range(65, at[1]), ring67=range(at[1], at[2]), ring5=range(at[2], at[2] + 5), tail=range(at[2] + 5, at[3]),
                                               queue=range(at[3], n - 1), head=n - 1)


@pytest.fixture(scope="module")
def model_runs(worlds):
    fleets, made = {}, {}

    def get(kind, check_stride, with_priority, ring_flags, ticks=TICKS, skip_checks=()):
        w = worlds(kind)
        if kind not in fleets:
            fleets[kind] = mixed_fleet(w)
        robots, goals, start, hold_in, where = fleets[kind]
        key = (kind, check_stride, with_priority, ring_flags, ticks, skip_checks)
        prio = None
        if with_priority:                                             # four classes, and one robot of every ring before all others: not the first one
            prio = priorities(robots["pos"].shape[0]) + 1
            prio[[where[r][1] for r in ("triangle", "ring67", "ring5")]] = 0
        if key not in made:
            made[key] = RG.run(w.model, FM.config(), w.fields, robots, goals, DT, ticks, DIST_TOL, ANG_TOL, start, RADIUS, check_stride, SM.WAITING_PRESENT, AHEAD_COS,
                               prio, hold_in, ring_flags, skip_checks)
        return robots, goals, start, hold_in, where, prio, made[key]

    return get


def assert_equals_model(got, want, check_stride, what):
    RM.assert_same(got, want, (what, "state"), keys=RM.KEYS)
    assert FM.same_bits(got.trace, SM.thin(want["trace"], check_stride)), what
    SM.assert_same_rows(got, want, (what, "separation"))
    YM.assert_same_yield(got, want, (what, "yield"))
    RG.assert_same_rings(got, want, (what, "rings"))


def check_stats(ctx, want, launches_per_check=None):
    st = ctx.fleet_ring_stats()
    for k, v in want["ring_stats"].items():
        assert st[k] == v, (k, st, want["ring_stats"])
    assert 0 < st["ms_ring"] < st["ms_separation"] < st["ms_kernels"] <= st["ms_total"], st
    return st


CASES = [("async", s, p, f) for s in (1, 7) for p in (False, True) for f in (0, RG.RELEASE)] + [("cvp", 1, True, RG.RELEASE), ("cvp", 7, False, 0)]


@pytest.mark.parametrize("kind,check_stride,with_priority,ring_flags", CASES)
def test_the_device_equals_the_model(worlds, model_runs, kind, check_stride, with_priority, ring_flags):
    w = worlds(kind)
    robots, goals, start, hold_in, where, prio, want = model_runs(kind, check_stride, with_priority, ring_flags)
    n = robots["pos"].shape[0]
    first = RG.ring_sizes(want, 0)
    print(kind, check_stride, with_priority, ring_flags, "rings at the first check:", first, "first:", want["counts"][0], "last:", want["counts"][-1], want["ring_stats"],
          "released:", np.nonzero(want["released_checks"])[0], want["released_checks"][want["released_checks"] > 0])
    # conditions on the MODEL's output: the first check sees the structures as they were placed
    assert n == 177 and sorted(first.values()) == [3, 5, 67]                                   # a ring of exactly 3, one above 64 members
    assert all(want["class_at"][0][i] == RG.RING_MEMBER for r in ("triangle", "ring67", "ring5") for i in where[r])
    assert [want["class_at"][0][i] for i in where["tail"]] == [RG.RING_TAIL] * 3 and len({want["anchor_at"][0][i] for i in list(where["tail"]) + list(where["ring5"])}) == 1
    assert [want["class_at"][0][i] for i in where["queue"]] == [RG.PARKED] * 33 and {want["anchor_at"][0][i] for i in where["queue"]} == {where["head"]}
    assert (want["class_at"] == RG.QUEUED).any() and want["class_at"][0][where["head"]] == RG.FREE
    if ring_flags:
        assert (want["released_checks"] >= 2).any()                                            # a leader released at two checks or more
        assert len(RG.ring_sizes(want, -1)) < 3 and want["ring_stats"]["releases"] >= 3         # a ring that is absent at the last check
        led = np.nonzero(want["released_checks"])[0]
        assert all(want["had_tick"][i].any() for i in led)                                     # the released robots have ticks
    else:
        assert all((want["class_at"][:, i] == RG.RING_MEMBER).all() for r in ("triangle", "ring67", "ring5") for i in where[r])      # nothing resolves the rings
        assert want["ring_stats"]["releases"] == 0 and want["ring_stats"]["rings_last"] >= 3
    sep = capi.SeparationConfig(radius=RADIUS, check_stride=check_stride, flags=SM.WAITING_PRESENT)
    got = rings_run(w, robots, goals, TICKS, start_tick=start, separation=sep, yield_config=capi.YieldConfig(ahead_cos=AHEAD_COS), priority=prio, hold_in=hold_in,
                    ring_config=capi.RingConfig(flags=ring_flags), trace_stride=check_stride)
    assert not got.cancelled and not got.skipped
    assert_equals_model(got, want, check_stride, (kind, check_stride, with_priority, ring_flags))
    check_stats(w.ctx, want)
    if not ring_flags:                                                # flags 0: every other output is the yielding rollout's
        plain = yield_run(w, robots, goals, TICKS, start_tick=start, separation=sep, yield_config=capi.YieldConfig(ahead_cos=AHEAD_COS), priority=prio, hold_in=hold_in,
                          trace_stride=check_stride)
        for k in STATE + SM.SEP_KEYS + YM.YIELD_KEYS:
            assert FM.same_bits(getattr(got, k), getattr(plain, k)), k


def big_fleet(w):
    """a ring of 257 and a line of 130 (spacing 0.047: it has to fit the mesh) whose head waits and is kept present"""
    parts = settle(w, [lambda a: circle(257, SPACING, phase=a), lambda a: line(130, 0.047)], in_field=False)
    robots = {k: (None if parts[0][k] is None else np.concatenate([p[k] for p in parts])) for k in parts[0]}
    n = 387
    goal = np.nanmean(w.model.xyz.astype(np.float64), axis=0).astype(F32)
    start, hold_in = np.zeros(n, np.uint32), np.ones(n, np.uint8)
    start[n - 1], hold_in[n - 1] = 100000, 0                          # the head waits for good and is kept present: the line is parked behind it
    return robots, (np.tile(goal, (n, 1)), np.tile(np.array([1, 0, 0], F32), (n, 1))), start, hold_in


@pytest.mark.parametrize("ring_flags", [0, RG.RELEASE])
def test_a_ring_of_257_and_a_line_of_130(worlds, ring_flags):
    w = worlds("async")
    robots, goals, start, hold_in = big_fleet(w)
    if 0 not in w.fields:
        w.fields[0] = w.ctx.download_output("vecmap", 0)
    prio = priorities(387)
    want = RG.run(w.model, SLOW, w.fields, robots, goals, DT, 21, DIST_TOL, ANG_TOL, start, RADIUS, 1, SM.WAITING_PRESENT, AHEAD_COS, prio, hold_in, ring_flags)
    print(ring_flags, [c for c in want["counts"]][:8], want["ring_stats"])
    assert RG.ring_sizes(want, 0) == {int(np.lexsort((np.arange(257), prio[:257]))[0]): 257}     # one ring of 257, led by the smallest (priority, index)
    assert want["counts"][0]["parked"] == 129 and {want["anchor_at"][0][i] for i in range(257, 386)} == {386}      # depth 129
    assert (want["ring_checks"][:257] >= 1).all()
    if ring_flags:                                                    # (a leader that finds no field where it stands parks the other 256 behind it)
        assert want["ring_stats"]["releases"] >= 1 and want["had_tick"][: 257].any() and max(c["parked"] + c["queued"] for c in want["counts"]) >= 129
    else:
        assert all(c["parked"] == 129 and c["members"] == 257 for c in want["counts"])
    sep = capi.SeparationConfig(radius=RADIUS, check_stride=1, flags=SM.WAITING_PRESENT)
    got = rings_run(w, robots, goals, 21, start_tick=start, separation=sep, yield_config=capi.YieldConfig(ahead_cos=AHEAD_COS), priority=prio, hold_in=hold_in,
                    ring_config=capi.RingConfig(flags=ring_flags), cfg=SLOW)
    assert_equals_model(got, want, 1, ("big", ring_flags))
    check_stats(w.ctx, want)
    try:                                                              # rounds that return at once where the earlier ones cover the robots held: the same bits
        w.ctx.set_option("ring_early_exit", 1)
        again = rings_run(w, robots, goals, 21, start_tick=start, separation=sep, yield_config=capi.YieldConfig(ahead_cos=AHEAD_COS), priority=prio, hold_in=hold_in,
                          ring_config=capi.RingConfig(flags=ring_flags), cfg=SLOW)
        assert_equals_model(again, want, 1, ("big, early exit", ring_flags))
    finally:
        w.ctx.set_option("ring_early_exit", None)


def test_without_a_ring_config_it_is_the_yielding_rollout(worlds, model_runs):
    w = worlds("async")
    robots, goals, start, hold_in, where, prio, _ = model_runs("async", 7, True, 0)
    sep, yc = capi.SeparationConfig(radius=RADIUS, check_stride=7, flags=SM.WAITING_PRESENT), capi.YieldConfig(ahead_cos=AHEAD_COS)
    for kw in (dict(start_tick=start, separation=sep, yield_config=yc, priority=prio, hold_in=hold_in, trace_stride=7), dict(start_tick=start, separation=sep), dict()):
        want = yield_run(w, robots, goals, 70, **kw)
        ys, fs, rs = w.ctx.fleet_yield_stats(), w.ctx.fleet_rollout_stats(), w.ctx.rollout_stats()
        got = rings_run(w, robots, goals, 70, **kw)
        for k in STATE + (SM.SEP_KEYS if "separation" in kw else ()) + (YM.YIELD_KEYS if "yield_config" in kw else ()):
            assert FM.same_bits(getattr(got, k), getattr(want, k)), (sorted(kw), k)
        assert got.wait_class is None and got.ring_checks is None and got.skipped == want.skipped
        st = w.ctx.fleet_ring_stats()
        assert (st["robots_ring"], st["rings"], st["releases"], st["members_last"], st["ms_ring"]) == (0, 0, 0, 0, 0) and st["ms_kernels"] > 0
        assert w.ctx.fleet_yield_stats() == ys and w.ctx.fleet_rollout_stats() == fs and w.ctx.rollout_stats() == rs


def test_two_runs_and_other_cell_scales_give_the_same_bits(worlds, model_runs):
    w = worlds("async")
    robots, goals, start, hold_in, where, prio, want = model_runs("async", 7, True, RG.RELEASE)
    sep, yc = capi.SeparationConfig(radius=RADIUS, check_stride=7, flags=SM.WAITING_PRESENT), capi.YieldConfig(ahead_cos=AHEAD_COS)
    try:
        for scale, early in ((None, None), (None, 1), (1.0, None), (4.0, 1)):
            w.ctx.set_option("separation_cell_scale", scale)
            w.ctx.set_option("ring_early_exit", early)
            again = rings_run(w, robots, goals, TICKS, start_tick=start, separation=sep, yield_config=yc, priority=prio, hold_in=hold_in,
                              ring_config=capi.RingConfig(flags=RG.RELEASE), trace_stride=7)
            assert_equals_model(again, want, 7, (scale, early))
            check_stats(w.ctx, want)
    finally:
        w.ctx.set_option("separation_cell_scale", None)
        w.ctx.set_option("ring_early_exit", None)


@pytest.fixture(scope="module")
def mirror(worlds, tmp_path_factory):
    """mnav_fleet_ring.h on the host over the asynchronous world's mesh: T, the guard's count of a check, is a property of the
    grid, which the model does not have"""
    m = RingMirror(build_shim(tmp_path_factory), worlds("async").model)
    yield m
    m.close()


def test_the_guard_leaves_every_class_free_at_a_skipped_check(worlds, model_runs, mirror):
    """stride 7, 42 ticks, as the guard's test of the yielding rollout: a bound one below the largest T among the checks after
    the first; the mirror, run with the bound, tells which checks it skips, and the model runs with exactly those skipped"""
    w = worlds("async")
    ctx, ticks, stride = w.ctx, 42, 7
    robots, goals, start, hold_in, where, prio, served = model_runs("async", stride, True, RG.RELEASE, ticks)
    fields = [w.fields.get(s, w.fields[0]) for s in range(w.n_plans)]
    kw = dict(start_tick=start, radius=RADIUS, check_stride=stride, flags=SM.WAITING_PRESENT, ahead_cos=AHEAD_COS, priority=prio, hold_in=hold_in, ring_flags=RG.RELEASE)
    for s in np.unique(robots["slot"]):
        assert int(s) in w.fields
    T = mirror.run_rings(FM.config(), fields, robots, goals, ticks, **kw)["chk"][:, 0].astype(np.int64)
    k = 1 + int(np.argmax(T[1:]))
    bound = int(T[k]) - 1
    chk = mirror.run_rings(FM.config(), fields, robots, goals, ticks, max_tests=bound, **kw)["chk"]
    skipped = tuple(int(t) for t in (np.nonzero(chk[:, 3])[0] + 1) * stride)
    print("T:", T, "bound:", bound, "skipped:", skipped)
    assert skipped and len(skipped) < ticks // stride
    want = model_runs("async", stride, True, RG.RELEASE, ticks, skipped)[6]
    c = skipped[0] // stride - 1
    assert served["class_at"][c].any() and not want["class_at"][c].any() and (want["anchor_at"][c] == NONE).all()
    sep, yc = capi.SeparationConfig(radius=RADIUS, check_stride=stride, flags=SM.WAITING_PRESENT), capi.YieldConfig(ahead_cos=AHEAD_COS)
    try:
        ctx.set_option("separation_max_tests", bound)
        got = rings_run(w, robots, goals, ticks, start_tick=start, separation=sep, yield_config=yc, priority=prio, hold_in=hold_in,
                        ring_config=capi.RingConfig(flags=RG.RELEASE), trace_stride=stride)
        assert got.skipped and not got.cancelled
        assert_equals_model(got, want, stride, ("skipped", skipped))
        st = check_stats(ctx, want)
        assert (st["checks_skipped"], st["first_skipped_tick"]) == (len(skipped), skipped[0])
        ctx.set_option("separation_max_tests", 0)                     # every check skipped: FREE at the end, nothing counted
        free = rings_run(w, robots, goals, ticks, start_tick=start, separation=sep, yield_config=yc, priority=prio, hold_in=hold_in,
                         ring_config=capi.RingConfig(flags=RG.RELEASE), trace_stride=stride)
        assert free.skipped and not free.wait_class.any() and (free.wait_anchor == NONE).all() and not free.ring_checks.any() and not free.hold.any()
        st = ctx.fleet_ring_stats()
        assert (st["rings"], st["robots_ring"], st["checks_run"], st["checks_skipped"], st["members_last"]) == (0, 0, 0, ticks // stride, 0)
    finally:
        ctx.set_option("separation_max_tests", None)


def test_the_statistics_records_are_kept_apart(worlds, model_runs):
    w = worlds("async")
    ctx = w.ctx
    robots, goals, start, hold_in, where, prio, want = model_runs("async", 7, True, RG.RELEASE)
    sep, yc, rc = capi.SeparationConfig(radius=RADIUS, check_stride=7, flags=SM.WAITING_PRESENT), capi.YieldConfig(ahead_cos=AHEAD_COS), capi.RingConfig(flags=RG.RELEASE)
    w.device_run(FM.config(), robots, goals, 5, trace_stride=0)
    fleet_run(w, FM.config(), robots, goals, 9, start_tick=start, separation=sep, trace_stride=0)
    yield_run(w, robots, goals, 14, start_tick=start, separation=sep, yield_config=yc, priority=prio, hold_in=hold_in, trace_stride=0)
    rs, fs, ys = ctx.rollout_stats(), ctx.fleet_rollout_stats(), ctx.fleet_yield_stats()
    rings_run(w, robots, goals, TICKS, start_tick=start, separation=sep, yield_config=yc, priority=prio, hold_in=hold_in, ring_config=rc, trace_stride=0)
    gs = check_stats(ctx, want)
    assert ctx.rollout_stats() == rs and ctx.fleet_rollout_stats() == fs and ctx.fleet_yield_stats() == ys and ys["checks_run"] == 2 and ys["held_last"] > 0
    # ... and the other way round
    w.device_run(FM.config(), robots, goals, 3, trace_stride=0)
    fleet_run(w, FM.config(), robots, goals, 14, start_tick=start, separation=sep, trace_stride=0)
    yield_run(w, robots, goals, 21, start_tick=start, separation=sep, yield_config=yc, priority=prio, hold_in=hold_in, trace_stride=0)
    assert ctx.fleet_ring_stats() == gs and ctx.fleet_yield_stats()["checks_run"] == 3 and ctx.rollout_stats() != rs


def test_refusals_touch_nothing(worlds, model_runs):
    w = worlds("async")
    ctx = w.ctx
    robots, goals, start, hold_in, where, prio, _ = model_runs("async", 7, True, RG.RELEASE)
    n = robots["pos"].shape[0]
    SC, YC, GC, RC = capi.SeparationConfig, capi.YieldConfig, capi.RingConfig, capi.RolloutConfig
    rings_run(w, robots, goals, 4, separation=SC(radius=RADIUS), yield_config=YC(), ring_config=GC())
    field0, stats0 = ctx.download_output("vecmap", 1), ctx.stats()
    records0 = (ctx.fleet_ring_stats(), ctx.fleet_yield_stats(), ctx.fleet_rollout_stats(), ctx.rollout_stats())
    sentinel = dict(status=np.full(n, -7, np.int32), pos=np.full((n, 3), -7.0, F32), near_checks=np.full(n, 7, np.uint32), hold=np.full(n, 7, np.uint8),
                    hold_checks=np.full(n, 7, np.uint32), wait_class=np.full(n, 7, np.uint8), wait_anchor=np.full(n, 7, np.uint32), ring_checks=np.full(n, 7, np.uint32),
                    first_ring_tick=np.full(n, 7, np.uint32), parked_checks=np.full(n, 7, np.uint32), released_checks=np.full(n, 7, np.uint32))
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(ro=None, sep=SC(radius=RADIUS), no_sep=False, yc=YC(ahead_cos=AHEAD_COS), no_yield=False, gc=GC(), no_rings=False, outs=True, pos=robots["pos"]):
        ro = ro if ro is not None else RC(dt=DT, ticks=4, trace_stride=0)
        fc = capi.FollowConfig(**FM.config())
        r_outs = [p(sentinel[k]) if outs else None for k in capi.RING_OUTPUTS]
        return ctx._L.mnav_fleet_rollout_rings(ctx._h, n, p(pos), p(robots["dir"]), p(robots["up"]), p(robots["face_in"]), p(robots["slot"]), None, p(goals[0]), p(goals[1]),
                                               C.byref(fc), C.byref(ro), p(start), None if no_sep else C.byref(sep), p(sentinel["status"]), None, p(sentinel["pos"]),
                                               None, None, None, None, None, None, None if no_sep else p(sentinel["near_checks"]), None, None, None, None, None, None,
                                               None if no_yield else C.byref(yc), None, None, None if no_yield else p(sentinel["hold"]),
                                               None if no_yield else p(sentinel["hold_checks"]), None, None, None, None if no_rings else C.byref(gc), *r_outs)

    refusals = [
        # those of mnav_fleet_rollout_yield
        (dict(pos=None), "null"), (dict(ro=RC(dt=0.0, ticks=4)), "dt"), (dict(sep=SC(radius=0.0)), "radius"), (dict(sep=SC(radius=RADIUS, flags=4)), "flag"),
        (dict(yc=YC(ahead_cos=1.0)), "ahead_cos"), (dict(yc=YC(flags=1)), "reserved"), (dict(no_sep=True), "without a separation"),
        # the analysis' own
        (dict(no_yield=True), "without a yield config"), (dict(no_yield=True, no_sep=True, outs=False), "without a yield config"),
        (dict(gc=GC(flags=2)), "unknown ring flag"), (dict(gc=GC(flags=3)), "unknown ring flag"), (dict(gc=GC(flags=0x80000000)), "unknown ring flag"),
        (dict(no_rings=True), "without a ring config"),
    ]
    for kw, text in refusals:
        assert call(**kw) == -1 and text in ctx._err(), (kw, ctx._err())
        assert all((v == (-7 if v.dtype in (np.int32, np.float32) else 7)).all() for v in sentinel.values()), kw
    assert np.array_equal(LM.bits(ctx.download_output("vecmap", 1)), LM.bits(field0)) and ctx.stats() == stats0
    assert (ctx.fleet_ring_stats(), ctx.fleet_yield_stats(), ctx.fleet_rollout_stats(), ctx.rollout_stats()) == records0
    # served: both flags values, NULL outputs, rings = NULL with every ring pointer NULL, n = 0, a choice of outputs
    assert call(gc=GC(flags=1)) == 0 and (sentinel["status"] != -7).all() and (sentinel["wait_class"] <= 4).all() and (sentinel["ring_checks"] <= 4).all()
    assert call(outs=False) == 0 and call(no_rings=True, outs=False) == 0
    empty = ctx.fleet_rollout_rings(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), np.zeros(0), separation=SC(radius=RADIUS), yield_config=YC(),
                                    ring_config=GC())
    assert empty.status.shape == (0,) and empty.wait_class.shape == (0,) and not empty.skipped
    only = rings_run(w, robots, goals, 4, separation=SC(radius=RADIUS), yield_config=YC(), ring_config=GC(), trace_stride=0, outputs=("status", "wait_class", "held_ticks"))
    assert only.pos is None and only.hold is None and only.wait_anchor is None and only.wait_class is not None and only.held_ticks is not None and only.status is not None


def test_two_calls_through_hold_out_and_hold_in_equal_one(worlds, model_runs):
    """a + b ticks with a a multiple of the stride; every robot is fed back with its state, so every robot that can be present
    is (a robot that has stopped stops again at once where it stood; REACHED ones are not present under these flags)"""
    w = worlds("async")
    stride, a, b = 7, 28, 42
    robots, goals, start, hold_in, where, prio, _ = model_runs("async", stride, True, RG.RELEASE)
    sep, yc, rc = capi.SeparationConfig(radius=RADIUS, check_stride=stride, flags=SM.WAITING_PRESENT), capi.YieldConfig(ahead_cos=AHEAD_COS), capi.RingConfig(flags=RG.RELEASE)
    kw = dict(separation=sep, yield_config=yc, ring_config=rc, trace_stride=stride)
    whole = rings_run(w, robots, goals, a + b, start_tick=start, priority=prio, hold_in=hold_in, **kw)
    first = rings_run(w, robots, goals, a, start_tick=start, priority=prio, hold_in=hold_in, **kw)
    keep = np.nonzero(first.status != RM.REACHED)[0]
    run = first.status[keep] == RM.RUNNING
    assert first.hold[keep][run].any() and not first.hold[keep][run].all() and first.released_checks.any()
    sub = {k: (None if v is None else v[keep]) for k, v in robots.items()}
    sub.update(pos=first.pos[keep], dir=first.dir[keep], face_in=first.face[keep])
    left = np.maximum(start[keep].astype(np.int64) - a, 0).astype(np.uint32)
    second = rings_run(w, sub, (goals[0][keep], goals[1][keep]), b, start_tick=left, priority=prio[keep], hold_in=first.hold[keep], **kw)
    for k in ("status", "pos", "dir", "face", "hold", "wait_class"):
        assert FM.same_bits(getattr(second, k)[run], getattr(whole, k)[keep][run]), k
    back = np.full(robots["pos"].shape[0] + 1, NONE, np.uint32)     # the anchors of the second call are indices into its robots
    back[keep] = np.arange(keep.size)
    assert np.array_equal(second.wait_anchor[run], back[np.minimum(whole.wait_anchor[keep][run], back.size - 1)])
    for k in ("ticks", "held_ticks", "hold_checks", "ring_checks", "parked_checks", "released_checks"):
        assert np.array_equal((getattr(first, k)[keep] + getattr(second, k))[run], getattr(whole, k)[keep][run]), k
    assert FM.same_bits(np.concatenate([first.trace[keep], second.trace], axis=1)[run], whole.trace[keep][run])
    assert second.released_checks[run].any() and second.ring_checks[run].any()
