"""CPU: the per-plan replan rule (tests/replan_each_model.py) against OracleMesh.dijkstra on the new map --
every bit of dist, pred, the path and the code of every plan, whatever its class -- over the scenarios of the GPU tests, 240
random events, the four kinds of offset, a flat grid full of ties and vertex-cost changes across cost_limit at and just beyond
the cut.  The KEPT claim is what is at stake: a plan the rule keeps returns what it held, and that must be the fresh result."""
import numpy as np
import pytest

from tests import replan_each_model as E
from tests import replan_model as R
from tests.replan_model import bits

SCENARIOS = R.scenarios()


def check(W, old, seed, t0, off0, C, t1, off1, f, where, finalized=True):
    want = W.om.dijkstra(W.weights, W.costs, seed, t1, off1, R.LIMIT)
    cls, code, dist, pred, path, info = E.replan_each(W, old, seed, t0, off0, C, t1, off1, f, finalized)
    assert code == want.code, (where, cls)
    assert np.array_equal(bits(dist), bits(want.dist)), (where, cls, int((bits(dist) != bits(want.dist)).sum()))
    assert np.array_equal(pred, want.pred) and np.array_equal(path, want.path), (where, cls)
    return cls, want, info


@pytest.mark.parametrize("f", [E.F_DEFAULT, 0.0])
@pytest.mark.parametrize("sc", SCENARIOS, ids=[s.name for s in SCENARIOS])
def test_scenarios_of_the_batch_replan(sc, f):
    if len(sc.seeds) > 16:
        sc = R.Scenario(sc.name, sc.N, sc.tile, sc.computed, sc.seeds[::10], sc.targets[::10], sc.offset, sc.steps, sc.engine, sc.fields, sc.reason)
    W = R.World(sc.N, sc.computed)
    targets, offset = list(sc.targets), sc.offset
    old = [W.om.dijkstra(W.weights, W.costs, s, t, offset, R.LIMIT) for s, t in zip(sc.seeds, targets)]
    for k, st in enumerate(sc.steps):
        C = np.concatenate([W.apply(ev) for ev in st.events]) if st.events else np.zeros(0, np.uint32)
        new_t = list(st.targets) if st.targets is not None else targets
        for p, s in enumerate(sc.seeds):
            cls, old[p], _ = check(W, old[p], s, targets[p], offset, C, new_t[p], st.offset, f, (sc.name, k, p))
            assert not (f == 0.0 and cls == E.FRESH)
            if st.expect in ("partial", "all") and len(sc.seeds) == 1:
                assert cls != E.KEPT, (sc.name, k)
        targets, offset = new_t, st.offset


def mixed_steps():
    """the two steps of the mixed batch: (world after the step, logged ids, per-plan classes, old results, new results)"""
    seeds, targets, patch = E.mixed12()
    W = R.World(96, True)
    back = W.costs[patch].copy()
    old = [W.om.dijkstra(W.weights, W.costs, s, t, 0.3, R.LIMIT) for s, t in zip(seeds, targets)]
    out = []
    for k, ev in enumerate([("costs", patch, 1.5), ("costs", patch, back)]):
        C = W.apply(ev)
        cls = []
        for p, s in enumerate(seeds):
            c, old[p], _ = check(W, old[p], s, targets[p], 0.3, C, targets[p], 0.3, E.F_DEFAULT, ("mixed12", k, p))
            cls.append(c)
        out.append(cls)
    return out


def test_the_mixed_batch_holds_every_class_in_both_steps():
    for k, cls in enumerate(mixed_steps()):
        for c in (E.KEPT, E.REPAIRED, E.FRESH):
            assert cls.count(c) >= 2, (k, cls)


def test_the_batch_of_70_holds_every_class():
    seeds, targets, patch = E.batch70()
    W = R.World(48, True)
    old = [W.om.dijkstra(W.weights, W.costs, s, t, 0.3, R.LIMIT) for s, t in zip(seeds, targets)]
    C = W.apply(("costs", patch, 1.5))
    cls = [E.classify(48, old[p].dist, targets[p], 0.3, C, targets[p], 0.3)[0] for p in range(70)]
    assert min(cls.count(c) for c in (E.KEPT, E.REPAIRED, E.FRESH)) >= 5, [cls.count(c) for c in range(3)]
    assert cls.count(E.FRESH) > 4                                      # (more than the async_max_batch the GPU test sets)
    for p in range(0, 70, 5):
        check(W, old[p], seeds[p], targets[p], 0.3, C, targets[p], 0.3, E.F_DEFAULT, ("batch70", p))


@pytest.mark.parametrize("N,computed", [(32, True), (32, False), (48, True)])
def test_random_events(N, computed):
    """80 random events per mesh as in tests/test_replan_model.py -- patches over the limit, just under it and to zero, or edge
    weights scaled --, small patches and near robots so that fields end before the event, events next to the goal, moved and unmoved targets, the
    offsets 0.3, 0, negative and +inf, and a paths-only (not finalized) field now and then."""
    rng = np.random.default_rng(2000 + N + computed)
    seen = [0, 0, 0]
    for trial in range(80):
        W = R.World(N, computed)
        V = W.mesh.V
        s = int(rng.integers(V))
        if trial % 4 < 2:                                              # a robot near its goal: a small field
            x = int(np.clip(s % N + rng.integers(-5, 6), 0, N - 1)); y = int(np.clip(s // N + rng.integers(-5, 6), 0, N - 1))
            t = y * N + x
        else:
            t = int(rng.integers(V))
        if t == s:
            t = (s + 1) % V
        off = [0.3, 0.0, -0.2, np.inf][(trial // 2) % 4]
        old = W.om.dijkstra(W.weights, W.costs, s, t, off, R.LIMIT)
        patch = W.rect(rng.random(), rng.random(), int(rng.integers(0, 4)))
        if trial % 5 == 0:                                             # an event next to the goal: little of the field survives
            patch = np.array([(s + 2) % V, (s + 2 * N) % V], np.uint32)
        if computed or trial % 2:
            C = W.apply(("costs", patch, [1.5, 0.95, 0.0][trial % 3]))
        else:
            e = W.edges_at(patch)
            C = W.apply(("edges", e, W.weights[e] * R.f32([4.0, 0.2][(trial // 2) % 2])))
        t1 = t if trial % 8 else int(rng.integers(V))
        if t1 == s:
            t1 = (s + 1) % V
        off1 = off if trial % 16 != 5 else 0.1
        cls, _, _ = check(W, old, s, t, off, C, t1, off1, E.F_DEFAULT, (N, computed, trial), finalized=trial % 10 != 9)
        assert not (cls == E.KEPT and (t1 != t or off1 != off or trial % 10 == 9))
        seen[cls] += 1
    assert min(seen) >= 8, seen                                        # every class is exercised, KEPT included


@pytest.mark.parametrize("off", [0.0, 0.3, -0.2, np.inf])
def test_a_flat_grid_full_of_ties(off):
    """Equal potentials everywhere: at the target's value (the cut for offsets <= 0) sit many vertices, some expanded."""
    N = 24
    rng = np.random.default_rng(24)
    kept = 0
    for trial in range(24):
        W = E.FlatWorld(N)
        s = W.v(0.3, 0.3)
        t = s + (1 + trial % 6) + 7 * N                                # (a, b) cells from the goal: (b, a) has the same potential
        old = W.om.dijkstra(W.weights, W.costs, s, t, off, R.LIMIT)
        assert int((bits(old.dist) == bits(old.dist[t])).sum()) >= 2    # a tie at the target's value
        patch = W.rect(rng.random(), rng.random(), int(rng.integers(0, 3)))
        C = W.apply(("costs", patch, [1.5, 0.5][trial % 2]))
        cls, _, _ = check(W, old, s, t, off, C, t, off, E.F_DEFAULT, ("flat", off, trial))
        kept += cls == E.KEPT
    assert kept >= 3 or not np.isfinite(off)


@pytest.mark.parametrize("off", [0.0, 0.3, -0.2])
def test_cost_changes_across_the_limit_at_and_beyond_the_cut(off):
    """One vertex goes over cost_limit, then back: at the cut (an expanded source there stops expanding -- the plan is not
    KEPT, and keeping it would be wrong), next to expanded vertices, and with its whole one-ring beyond the cut (KEPT)."""
    for W in (E.FlatWorld(24), R.World(32, True)):
        s, t = W.v(0.3, 0.3), W.v(0.5, 0.55)
        base = W.om.dijkstra(W.weights, W.costs, s, t, off, R.LIMIT)
        cut = R.old_cut(base.dist, t, off)
        exp = R.O.product_expanded_sources(base.dist, t, off)[0]
        adj = R.adjacency(W.N)
        order = np.argsort(base.dist, kind="stable")
        at = [int(v) for v in order if base.dist[v] == cut and v != s]
        beyond = [int(v) for v in order if cut < base.dist[v] < np.inf]
        # (a finite value beyond the cut is a tentative one: it has an expanded neighbour.  The nearest vertices whose whole
        #  one-ring lies beyond the cut are the unreached ones next to those)
        ring_out = [v for v in range(W.mesh.V) if base.dist[v] > cut and all(base.dist[u] > cut for u, _ in adj[v])]
        ring_out = sorted(ring_out, key=lambda v: min(base.dist[u] for u, _ in adj[v]))
        assert not set(ring_out) & set(beyond) and np.isfinite(min(base.dist[u] for u, _ in adj[ring_out[0]]))
        picks = [("at", v) for v in at[:4]] + [("beyond", v) for v in beyond[:4]] + [("ring", v) for v in ring_out[:4]]
        assert ring_out and beyond
        wrong_if_kept = 0
        for kind, v in picks:
            c0 = W.costs[v].copy()
            old = base
            for val in (1.5, c0):                                      # over the limit, and back
                C = W.apply(("costs", [v], val))
                cls, new, _ = check(W, old, s, t, off, C, t, off, E.F_DEFAULT, (kind, v, float(val)))
                assert (cls == E.KEPT) == (kind == "ring"), (kind, v, cls)
                if kind == "at" and exp[v]:
                    wrong_if_kept += not np.array_equal(bits(new.dist), bits(old.dist))
                old = new
        if at and any(exp[v] for v in at[:4]) and isinstance(W, E.FlatWorld):
            assert wrong_if_kept > 0                                   # L == cut alone would have kept a field that changed
