"""GPU: fleet dispatch (mnav_fleet_costs, mnav_fleet_assign, mnav_dispatch_stats).

Matrix: codes and potential bits of the n x m pairs equal ONE mnav_fleet_paths call over the same pairs and the model of
tests/dispatch_model.py on the oracle's fields; both nearest arrays equal numpy with the tie rule; over the fields left by
the tile rounds, the asynchronous engine, the tile-batch engine and a replan after a cost update.  Assignment: a valid
assignment with (size, sum of q) of the exact solver, and the assignment, phases, rounds and bids of the model's auction
bit for bit, whichever kernels run the rounds.

Shapes: the world of tests/test_gpu_fleet.py (terrain(48) = 2304 vertices, 8 plans), up to 257 robots; 257 full fields for
the assignments."""
import ctypes as C

import numpy as np
import pytest

from tests import dispatch_model as DM
from tests import fleet_model as FM
from tests.fleet_model import bits
from tests.test_gpu_fleet import LIMIT, OFFSET, World, make_ctx

pytestmark = pytest.mark.gpu
SENTINEL = 0xDEADBEEF
QUANTUM = 1e-3


@pytest.fixture(scope="module")
def world():
    W = World()
    W.targets = W.targets.copy()
    W.targets[4:6] = np.flatnonzero(W.invalid)[:2]    # plans 4 and 5 run and find no path: their cut is +inf, what they never reached has no path
    return W


def robots_of(W, fields, n):
    """n robot vertices chosen from the model, in rounds over the running plans: below the cut, on the tentative ring at or
    above it, never reached by the wave, with pred == self; then the plan's seed and target, an id >= V and MNAV_NONE"""
    rng = np.random.default_rng(23)
    groups = []
    for f in fields:
        if f.dist is None:
            continue
        cut = FM.cut_of(f.dist, f.target, f.offset)
        fin = np.isfinite(f.dist)
        ids = np.arange(W.V)
        below, ring, never = ids[fin & (f.dist < cut)], ids[fin & (f.dist >= cut)], ids[~fin]
        own = ids[(f.pred == ids) & (ids != f.seed)]
        special = np.array([f.seed, f.target, W.V + 1 + len(groups), FM.NONE], np.int64)
        groups.append([rng.permutation(g) for g in (below, below, below, ring, never, own)] + [special])
    out, k = [], 0
    while len(out) < n:
        for g in groups:
            for kind in g:
                if k < kind.size and len(out) < n:
                    out.append(int(kind[k]))
        k += 1
    return np.array(out, np.uint32)


def raw_costs(ctx, vtx, slots, m, pos=None):
    """the C call with sentinel-filled outputs: (rc, untouched)"""
    n = len(vtx) if vtx is not None else len(pos)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    code, pot = np.full((n, m), 0xEE, np.uint8), np.full((n, m), np.nan, np.float32)
    vout, ns, nr = np.full(n, SENTINEL, np.uint32), np.full(n, SENTINEL, np.uint32), np.full(m, SENTINEL, np.uint32)
    rc = ctx._L.mnav_fleet_costs(ctx._h, n, p(vtx), p(pos), m, p(slots), p(code), p(pot), p(vout), p(ns), p(nr))
    untouched = (code == 0xEE).all() and np.isnan(pot).all() and all((a == SENTINEL).all() for a in (vout, ns, nr))
    return rc, untouched


def raw_assign(ctx, vtx, slots, m, quantum):
    n = len(vtx)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    sor, ros, pot = np.full(n, SENTINEL, np.uint32), np.full(m, SENTINEL, np.uint32), np.full(n, np.nan, np.float32)
    a, tq, tp = C.c_uint32(SENTINEL), C.c_int64(SENTINEL), C.c_double(-7.0)
    rc = ctx._L.mnav_fleet_assign(ctx._h, n, p(vtx), None, m, p(slots), quantum, p(sor), p(ros), p(pot), C.byref(a), C.byref(tq), C.byref(tp))
    untouched = (sor == SENTINEL).all() and (ros == SENTINEL).all() and np.isnan(pot).all() and a.value == SENTINEL and tq.value == SENTINEL and tp.value == -7.0
    return rc, untouched


def check_matrix(ctx, W, fields, vtx, slots, where, start_pos=None):
    """fleet_costs over the columns `slots` (None: all plans) against one fleet_paths call over the pairs and the model"""
    cols = np.arange(len(fields), dtype=np.uint32) if slots is None else np.asarray(slots, np.uint32)
    n, m = len(vtx), len(cols)
    out = ctx.fleet_costs(None if start_pos is not None else vtx, start_pos, slots, m=m)
    st = ctx.dispatch_stats()
    assert np.array_equal(out["vertex"], vtx), where
    paths = ctx.fleet_paths(np.tile(cols, n), np.repeat(vtx, m), ids_cap=0)
    assert np.array_equal(out["codes"].ravel(), paths["codes"]), (where, np.flatnonzero(out["codes"].ravel() != paths["codes"])[:8])
    assert np.array_equal(bits(out["potential"]).ravel(), bits(paths["potential"])), where
    codes, pot = DM.matrix([fields[int(s)] for s in cols], W.V, vtx)
    assert np.array_equal(out["codes"], codes) and np.array_equal(bits(out["potential"]), bits(pot)), where
    ns, nr = DM.nearest(codes, pot)
    assert np.array_equal(out["nearest_slot"], ns) and np.array_equal(out["nearest_robot"], nr), where
    want = DM.counts(codes)
    assert [st[k] for k in ("served", "beyond_field", "no_path", "invalid")] == want and st["feasible"] == int(DM.feasible_of(codes, pot).sum()), (where, st, want)
    assert (st["assigned"], st["rounds"]) == (0, 0)
    return codes, pot, st


COLUMNS = {1: [3], 3: [4, 0, 6], 8: None}


@pytest.mark.parametrize("source", ["tiled", "async", "tile_batch"])
def test_matrix_equals_fleet_paths(world, source):
    W = world
    ctx = make_ctx(W)
    try:
        ctx.set_dijkstra_engine(source)
        b = ctx.plan_dijkstra_batch(W.seeds, W.targets, OFFSET, LIMIT)
        assert {"tiled": "k_tile_round", "async": "k_plan_async", "tile_batch": "k_tb"}[source] in ctx.last_engine(), ctx.last_engine()
        assert list(b["codes"][4:]) == [FM.NO_PATH_FOUND, FM.NO_PATH_FOUND, FM.SUCCESS, FM.INVALID_GOAL]
        fields = W.fields(W.targets)
        for n in (1, 63, 65, 257):
            vtx = robots_of(W, fields, n)
            for m, slots in COLUMNS.items():
                codes, pot, st = check_matrix(ctx, W, fields, vtx, slots, (source, n, m))
        # n = 257 over all plans: every outcome in at least 2 % of the pairs, a quarter of them feasible, and pairs that
        # wait for the look at their plan (never reached under a finite cut: the lazy rule-5 path)
        share = np.array(DM.counts(codes)) / codes.size
        feasible = DM.feasible_of(codes, pot).mean()
        marked = sum(int((~np.isfinite(f.dist[vtx[vtx < W.V]])).sum()) for f in fields if f.dist is not None and np.isfinite(FM.cut_of(f.dist, f.target, f.offset)))
        print(source, "shares served / beyond / no path / invalid", share, "feasible", feasible, "marked", marked, "ms", st["ms_costs"], st["ms_total"])
        assert (share >= 0.02).all() and feasible >= 0.25 and marked > 0, (share, feasible, marked)
    finally:
        ctx.close()


def test_matrix_after_a_wave_that_ran_out(world):
    """offset 1e9: finite cuts with nothing at or above them -- the lazy look turns the marked pairs into MNAV_NO_PATH_FOUND"""
    W = world
    ctx = make_ctx(W)
    try:
        ctx.plan_dijkstra_batch(W.seeds, W.targets, 1e9, LIMIT)
        fields = W.fields(W.targets, 1e9)
        for n, (m, slots) in ((65, (8, None)), (257, (3, [4, 0, 6])), (257, (8, None))):
            codes, pot, st = check_matrix(ctx, W, fields, robots_of(W, fields, n), slots, ("ran out", n, m))
        assert st["beyond_field"] == 0 and st["no_path"] >= 0.02 * codes.size
    finally:
        ctx.close()


def test_matrix_after_a_replan_and_from_positions(world):
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
        vtx = robots_of(W, W.fields(targets), 65)
        rc, untouched = raw_costs(ctx, vtx, None, 6)
        assert rc == -1 and untouched and "costs changed" in ctx._err(), ctx._err()
        b = ctx.replan_dijkstra(targets, OFFSET)
        assert b["replan"]["reason"] == 0 and b["replan"]["log_len"] == ids.size
        fields = W.fields(targets)
        for n, slots in ((65, None), (257, [5, 2, 0])):
            check_matrix(ctx, W, fields, robots_of(W, fields, n), slots, ("replan", n))
        # robots given by positions: the vertex by the rule of mnav_locate, the ids stay on the device
        rng = np.random.default_rng(3)
        v = rng.integers(0, W.V, 130)
        pos = (W.mesh.xyz[v] + rng.uniform(-0.04, 0.04, (130, 3)).astype(np.float32) * np.array([1, 1, 0.2], np.float32)).astype(np.float32)
        near = np.array([W.om.nearest_vertex(p) for p in pos], np.uint32)
        assert ctx.locate_stats()["built"] == 0
        check_matrix(ctx, W, fields, near, None, "positions", start_pos=pos)
        assert ctx.dispatch_stats()["built_index"] == 1 and ctx.locate_stats()["built"] == 1
        check_matrix(ctx, W, fields, near[:63], [1, 3], "positions 63", start_pos=pos[:63])
        assert ctx.dispatch_stats()["built_index"] == 0
        # nothing of the matrix's size has to leave the device
        small = ctx.fleet_costs(near, slots=None, m=6, want_matrix=False)
        assert small["codes"] is None and np.array_equal(small["nearest_slot"], DM.nearest(*DM.matrix(fields, W.V, near))[0])
    finally:
        ctx.close()
        W.costs = old
        W.weights = W.om.edge_weights(W.case.edge_dist, W.costs, 1.0)
        W.version += 1


def test_refusals_touch_nothing(world):
    W = world
    ctx = make_ctx(W)
    try:
        fields = W.fields(W.targets)
        vtx = robots_of(W, fields, 65)
        u32 = lambda *a: np.array(a, np.uint32)

        def refused(what, slots, m, vertices=vtx, text=None, quantum=None):
            before = ctx.dispatch_stats()
            rc, untouched = raw_costs(ctx, vertices, slots, m) if quantum is None else raw_assign(ctx, vertices, slots, m, quantum)
            assert rc == -1 and untouched and ctx._err(), (what, rc, untouched, ctx._err())
            assert text is None or text in ctx._err(), (what, ctx._err())
            assert ctx.dispatch_stats() == before, what
            print(what, "->", ctx._err())

        refused("no plan yet", None, 8)
        ctx.plan_dijkstra_batch(W.seeds, W.targets, OFFSET, LIMIT)
        ok = ctx.fleet_assign(vtx, slots=None, m=8, quantum=QUANTUM)
        assert ok["assigned"] > 0 and ctx.dispatch_stats()["rounds"] > 0
        refused("a slot that is not a plan of the last call", u32(0, 8), 2, text="slot")
        refused("a slot given twice", u32(2, 0, 2), 3, text="twice")
        refused("all plans, wrong count", None, 7, text="plan count")
        refused("no columns", u32(), 0)
        before = ctx.dispatch_stats()
        assert ctx._L.mnav_fleet_costs(ctx._h, 5, None, None, 8, None, None, None, None, None, None) == -1 and ctx.dispatch_stats() == before   # neither vertices nor positions
        ctx.set_option("dispatch_max_mb", 1e-4)                               # 104 bytes
        refused("a matrix above dispatch_max_mb", None, 8, text="dispatch_max_mb")
        ctx.set_option("dispatch_max_mb", None)
        for q in (0.0, -1.0, float("nan"), float("inf")):
            refused("quantum %r" % q, None, 8, quantum=q, text="quantum")
        refused("a cost above 2^31 - 1", None, 8, quantum=1e-12, text="2^31")
        many = np.resize(vtx[vtx < W.V], 7000).astype(np.uint32)             # N = 7000, q_max near 2^31: (N + 1) (N q_max + 1) >= 2^56
        reach = ctx.fleet_costs(many, slots=[0])["potential"]
        top = float(reach[np.isfinite(reach)].max())
        assert top > 0
        refused("quantum too fine", u32(0), 1, vertices=many, quantum=top / 2.0e9, text="quantum too fine for this fleet")
        ctx.set_option("dispatch_max_rounds", 3)
        refused("three rounds", None, 8, quantum=QUANTUM, text="dispatch_max_rounds")
        ctx.set_option("dispatch_max_rounds", None)
        assert ctx.fleet_assign(vtx, slots=None, m=8, quantum=QUANTUM)["assigned"] == ok["assigned"]
        # costs changed with no replan; a last call that is not a Dijkstra call
        ctx.update_costs(u32(W.targets[0]), np.array([W.costs[int(W.targets[0])]], np.float32))
        refused("update_costs without a replan", None, 8, text="costs changed")
        refused("update_costs without a replan (assign)", None, 8, quantum=QUANTUM, text="costs changed")
        ctx.replan_dijkstra(None, OFFSET)
        assert ctx.fleet_costs(vtx, slots=None, m=8)["codes"].shape == (65, 8)
        goal = W.mesh.xyz[int(W.seeds[0])] + np.array([0.02, 0.03, 0.0], np.float32)
        gf, _ = W.om.containing_face(goal)
        tf, _ = W.om.containing_face(W.mesh.xyz[int(W.targets[0])] + np.array([0.02, 0.03, 0.0], np.float32))
        ctx.plan_cvp_batch([goal], [gf], [tf], OFFSET, LIMIT)
        refused("after a CVP call", None, 1)
    finally:
        ctx.close()


def test_other_statistics_are_left_alone(world):
    W = world
    ctx = make_ctx(W)
    try:
        ctx.plan_dijkstra_batch(W.seeds, W.targets, OFFSET, LIMIT)
        fields = W.fields(W.targets)
        vtx = robots_of(W, fields, 65)
        ctx.locate(W.mesh.xyz[:1])
        ctx.fleet_paths(np.zeros(3, np.uint32), vtx[:3])
        before = (ctx.fleet_stats(), ctx.locate_stats(), ctx.stats())
        keep = [ctx.download_output(w, k) for k in range(6) for w in ("dist", "pred")]
        ctx.fleet_costs(vtx, slots=None, m=8)
        ctx.fleet_assign(None, W.mesh.xyz[vtx[vtx < W.V]], slots=None, m=8, quantum=QUANTUM)
        after = (ctx.fleet_stats(), ctx.locate_stats(), ctx.stats())
        assert before == after
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(keep, [ctx.download_output(w, k) for k in range(6) for w in ("dist", "pred")]))
    finally:
        ctx.close()


# -- assignment -------------------------------------------------------------------------------------------------------
class Fleet:
    """257 full fields (offset 1e9) on one context, and the cases that use them: (robot vertices, column slots)"""

    def __init__(self, W):
        self.W = W
        rng = np.random.default_rng(31)
        ok = np.flatnonzero((W.costs <= LIMIT) & (W.invalid == 0))
        pick = rng.choice(ok, 258, replace=False)
        self.seeds, target = pick[:257].astype(np.uint32), int(pick[257])
        self.ctx = make_ctx(W)
        b = self.ctx.plan_dijkstra_batch(self.seeds, np.full(257, target, np.uint32), 1e9, LIMIT, want_fields=True)
        self.fields = [FM.Field(b["dist"][k], b["pred"][k], int(self.seeds[k]), target, 1e9) for k in range(257)]
        lost = np.flatnonzero(W.invalid)[:5]                                  # robots no wave reaches: no feasible pair
        r257 = np.concatenate([rng.choice(ok, 252, replace=False), lost]).astype(np.uint32)
        r130 = np.concatenate([rng.choice(ok, 127, replace=False), lost[:3]]).astype(np.uint32)
        self.cases = {
            "257x130": (r257, np.arange(130, dtype=np.uint32)),
            "130x257": (r130, None),
            "64x64": (rng.choice(ok, 64, replace=False).astype(np.uint32), rng.permutation(257)[:64].astype(np.uint32)),
            "1x1": (r257[:1], np.array([200], np.uint32)),
            "equal rows": (np.concatenate([np.full(20, r257[7]), r257[:6]]).astype(np.uint32), np.arange(40, 64, dtype=np.uint32)),
            "no feasible pair": (np.concatenate([lost, [W.V + 2, FM.NONE]]).astype(np.uint32), np.arange(9, dtype=np.uint32)),
        }
        self._model = {}

    def model(self, name):
        """the model's matrix, auction and the exact optimum of a case, computed once"""
        if name not in self._model:
            vtx, slots = self.cases[name]
            cols = self.fields if slots is None else [self.fields[int(s)] for s in slots]
            codes, pot = DM.matrix(cols, self.W.V, vtx)
            feasible = DM.feasible_of(codes, pot)
            q = DM.quantise(pot, feasible, QUANTUM)
            self._model[name] = (codes, pot, feasible, q, DM.auction(q, feasible), DM.exact(q, feasible))
        return self._model[name]


@pytest.fixture(scope="module")
def fleet(world):
    F = Fleet(world)
    yield F
    F.ctx.close()


CASES = ["257x130", "130x257", "64x64", "1x1", "equal rows", "no feasible pair"]


@pytest.mark.parametrize("tail", ["wide", "default", "tail"])
@pytest.mark.parametrize("name", CASES)
def test_assignment_is_optimal_and_the_models(fleet, name, tail):
    F, ctx = fleet, fleet.ctx
    vtx, slots = F.cases[name]
    m = 257 if slots is None else len(slots)
    n, N = len(vtx), max(len(vtx), m)
    codes, pot, feasible, q, want, best = F.model(name)
    ctx.set_option("dispatch_tail_bidders", {"wide": 0, "default": None, "tail": N}[tail])
    try:
        out = ctx.fleet_assign(vtx, slots=slots, m=m, quantum=QUANTUM)
        st = ctx.dispatch_stats()
        again = ctx.fleet_assign(vtx, slots=slots, m=m, quantum=QUANTUM)
    finally:
        ctx.set_option("dispatch_tail_bidders", None)
    print(name, tail, "assigned", out["assigned"], "total q", out["total_q"], {k: st[k] for k in ("phases", "rounds", "tail_rounds", "bids", "ms_costs", "ms_assign", "ms_total")})
    col_slot = np.arange(m, dtype=np.uint32) if slots is None else slots
    sor, ros = out["slot_of_robot"], out["robot_of_slot"]
    got = sor != FM.NONE
    # a valid assignment over feasible pairs, consistent in both directions
    col_of = np.full(n, FM.NONE, np.uint32)
    for j in range(m):
        if ros[j] != FM.NONE:
            assert sor[ros[j]] == col_slot[j], (name, j)
            col_of[ros[j]] = j
    assert int((ros != FM.NONE).sum()) == int(got.sum()) == out["assigned"] and np.unique(sor[got]).size == out["assigned"]
    assert all(feasible[i, int(col_of[i])] for i in np.flatnonzero(got))
    assert np.array_equal(bits(out["potential"]), bits(np.where(got, pot[np.arange(n), np.where(got, col_of, 0)], np.inf).astype(np.float32)))
    assert out["total_q"] == int(q[np.flatnonzero(got), col_of[got].astype(np.int64)].sum())
    total = 0.0
    for x in out["potential"][got]:
        total += float(x)                                                    # the double sum in robot order
    assert out["total_potential"] == total
    # the optimum, and the model's auction bit for bit
    assert (out["assigned"], out["total_q"]) == best, (name, tail, out["assigned"], out["total_q"], best)
    assert np.array_equal(col_of, want["col_of_robot"]), (name, tail)
    assert (st["phases"], st["rounds"], st["bids"], st["assigned"]) == (want["phases"], want["rounds"], want["bids"], want["size"]), (name, tail, st, want["rounds"])
    assert st["feasible"] == int(feasible.sum()) and [st[k] for k in ("served", "beyond_field", "no_path", "invalid")] == DM.counts(codes)
    assert {"wide": st["tail_rounds"] == 0, "tail": st["tail_rounds"] == st["rounds"], "default": st["tail_rounds"] <= st["rounds"]}[tail], (tail, st)
    for k in out:
        a, b = np.asarray(out[k]), np.asarray(again[k])
        assert np.array_equal(a.view(np.uint8) if a.ndim else a, b.view(np.uint8) if b.ndim else b), (name, k)      # two calls, the same bits
    if name == "no feasible pair":
        assert out["assigned"] == 0 and not got.any()
    if name == "257x130" and tail == "default":
        assert 0 < st["tail_rounds"] < st["rounds"]                          # both kinds of round ran
        # end to end: the assigned robots' paths come out of the slots the assignment names
        p = ctx.fleet_paths(sor[got], vtx[got], ids_cap=0)
        assert (p["codes"] == FM.SUCCESS).all() and np.array_equal(bits(p["potential"]), bits(out["potential"][got]))


@pytest.mark.parametrize("name", ["257x130", "130x257"])
def test_nearest_over_several_tiles(fleet, name):
    """more than one tile of 64 in both directions: the tile minima of k_dispatch_costs and their combine (5 x 3 and 3 x 5 tiles)"""
    F, ctx = fleet, fleet.ctx
    vtx, slots = F.cases[name]
    m = 257 if slots is None else len(slots)
    codes, pot = F.model(name)[:2]
    out = ctx.fleet_costs(vtx, slots=slots, m=m)
    ns, nr = DM.nearest(codes, pot)
    assert np.array_equal(out["codes"], codes) and np.array_equal(bits(out["potential"]), bits(pot))
    assert np.array_equal(out["nearest_slot"], ns) and np.array_equal(out["nearest_robot"], nr)
    assert (ns >= 64).any() and (nr >= 64).any() and (ns == FM.NONE).any()      # minima beyond the first tile, and rows without a feasible pair
    # ties across tiles go to the smallest index: the same robot twice, the same column's field under two slots is not possible, so rows only
    twice = np.concatenate([vtx[100:101], vtx]).astype(np.uint32)
    again = ctx.fleet_costs(twice, slots=slots, m=m)
    c2, p2 = DM.matrix(F.fields if slots is None else [F.fields[int(s)] for s in slots], F.W.V, twice)
    assert np.array_equal(again["nearest_robot"], DM.nearest(c2, p2)[1]) and not (again["nearest_robot"] == 101).any()


def test_three_rounds_are_not_enough(fleet):
    ctx = fleet.ctx
    vtx, slots = fleet.cases["64x64"]
    ctx.set_option("dispatch_max_rounds", 3)
    try:
        rc, untouched = raw_assign(ctx, vtx, slots, 64, QUANTUM)
        assert rc == -1 and untouched and "dispatch_max_rounds" in ctx._err(), ctx._err()
    finally:
        ctx.set_option("dispatch_max_rounds", None)
