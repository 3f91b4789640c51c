"""CPU: the replan rule (tests/replan_model.py) against OracleMesh.dijkstra on the new map -- every bit of
dist, pred, the path and the code -- over every scenario tests/test_gpu_replan.py runs and over random events.  The
conditions the GPU scenarios state (some but not all rewound, the level is the old cut, everything rewound) are asserted
here on the model alone, so a GPU test cannot pass by accident of its inputs."""
import numpy as np
import pytest

from tests import replan_model as R
from tests.replan_model import bits

SCENARIOS = R.scenarios()


def run_scenario(sc, check):
    """the oracle before and after every step, the model's replan in between; check(step index, per-plan infos)"""
    W = R.World(sc.N, sc.computed)
    om = W.om
    targets, offset = list(sc.targets), sc.offset
    old = [om.dijkstra(W.weights, W.costs, s, t, offset, R.LIMIT) for s, t in zip(sc.seeds, targets)]
    for k, st in enumerate(sc.steps):
        C = np.concatenate([W.apply(ev) for ev in st.events]) if st.events else np.zeros(0, np.uint32)
        new_t = list(st.targets) if st.targets is not None else targets
        infos = []
        for p, s in enumerate(sc.seeds):
            want = om.dijkstra(W.weights, W.costs, s, new_t[p], st.offset, R.LIMIT)
            code, dist, pred, path, info = R.replan(W, old[p].dist, s, targets[p], offset, C, new_t[p], st.offset)
            where = (sc.name, k, p)
            assert code == want.code == (st.codes[p] if st.codes else 0), where
            assert np.array_equal(bits(dist), bits(want.dist)), (where, int((bits(dist) != bits(want.dist)).sum()))
            assert np.array_equal(pred, want.pred), where
            assert np.array_equal(path, want.path), where
            info["old"], info["new_target_old_value"] = old[p].dist, old[p].dist[new_t[p]]
            infos.append(info)
            old[p] = want
        check(k, st, infos)
        targets, offset = new_t, st.offset


def stated_conditions(k, st, infos):
    rew, reached = sum(i["rewound"] for i in infos), sum(i["reached"] for i in infos)
    if st.expect == "partial":
        assert 0 < rew < reached, (k, rew, reached)
        assert any(i["level"] < i["cut_old"] for i in infos), k      # the event, not the old cut, set a level
    elif st.expect == "cut":
        for i in infos:
            assert bits(i["level"]) == bits(i["cut_old"]) and i["kept"] == int((i["old"] < i["cut_old"]).sum()), k
    elif st.expect == "all":
        assert all(i["kept"] == 1 and i["level"] == 0 for i in infos), k


@pytest.mark.parametrize("sc", SCENARIOS, ids=[s.name for s in SCENARIOS])
def test_scenarios_of_the_gpu_tests(sc):
    if len(sc.seeds) > 16:                                             # the 170-plan batches: the model on every tenth plan
        sc = R.Scenario(sc.name, sc.N, sc.tile, sc.computed, sc.seeds[::10], sc.targets[::10], sc.offset, sc.steps, sc.engine, sc.fields, sc.reason)
    run_scenario(sc, stated_conditions)


def test_the_target_scenario_moves_into_the_unreached_region():
    sc = next(s for s in SCENARIOS if s.name == "targets48")
    seen = []
    run_scenario(sc, lambda k, st, infos: seen.append(float(infos[0]["new_target_old_value"])))
    assert np.isfinite(seen[0]) and np.isinf(seen[2]) and np.isfinite(seen[3])      # nearer: reached before; the corner: never; the same again


@pytest.mark.parametrize("N,computed", [(32, True), (32, False), (48, True)])
def test_random_events(N, computed):
    """80 random events per mesh: patches set over the limit, just under it and to zero (or, on uploaded weights, edge
    weights scaled up and down), moved and unmoved targets, the four offsets"""
    rng = np.random.default_rng(1000 + N + computed)
    partial = 0
    for trial in range(80):
        W = R.World(N, computed)
        V = W.mesh.V
        s, t = int(rng.integers(V)), int(rng.integers(V))
        off = [0.3, 0.0, -0.2, 1e9][trial % 4]
        old = W.om.dijkstra(W.weights, W.costs, s, t, off, R.LIMIT)
        patch = W.rect(rng.random(), rng.random(), int(rng.integers(1, 5)))
        if computed or trial % 2:
            C = W.apply(("costs", patch, [1.5, 0.95, 0.0][trial % 3]))
        else:
            e = W.edges_at(patch)
            C = W.apply(("edges", e, W.weights[e] * R.f32([4.0, 0.2][(trial // 2) % 2])))
        t1 = t if trial % 2 else int(rng.integers(V))
        want = W.om.dijkstra(W.weights, W.costs, s, t1, off, R.LIMIT)
        code, dist, pred, path, info = R.replan(W, old.dist, s, t, off, C, t1, off)
        assert code == want.code, trial
        assert np.array_equal(bits(dist), bits(want.dist)) and np.array_equal(pred, want.pred) and np.array_equal(path, want.path), trial
        partial += 0 < info["rewound"] < info["reached"]
    assert partial >= 40                                               # most events rewind a part of the field
