"""CPU: what tests/test_gpu_replan_warm.py relies on, pinned with the numpy rule (tests/replan_model.py,
tests/replan_each_model.py) and the oracle, so that no GPU test passes by never entering the warm start: the class counts of
every scenario, REPAIRED plans whose fields are partly kept, a kept / unkept frontier longer than a tile of the tile-batch
engine (in cells: tests/replan_warm_model.py says why that crosses a tile boundary whatever the tiling), a plan whose level is
its cut, a plan with only its seed kept -- and that the rule's result from such a state is the oracle's fresh plan."""
import functools

import numpy as np
import pytest

from tests import replan_each_model as E
from tests import replan_model as R
from tests import replan_warm_model as WM
from tests.replan_model import bits

OFF = WM.OFF


def oracle_all(W, seeds, targets, offset=OFF):
    return [W.om.dijkstra(W.weights, W.costs, s, t, offset, R.LIMIT) for s, t in zip(seeds, targets)]


def facts_of(W, seeds, targets, ev, f, old=None):
    old = old or oracle_all(W, seeds, targets)
    C = W.apply(ev)
    facts = WM.plan_facts(W, old, seeds, targets, OFF, C, targets, OFF, f)
    return old, C, facts


def counts(facts):
    return tuple(sum(1 for x in facts if x[0] == c) for c in (E.KEPT, E.REPAIRED, E.FRESH))


def partly_kept(facts):
    """REPAIRED plans whose kept share of the reached vertices is neither 0 (the seed alone) nor 1"""
    return [p for p, (c, L, cut, kept, rew, reached, fr) in enumerate(facts) if c == E.REPAIRED and kept > 1 and rew > 0]


def longest_frontier(facts):
    return max([x[6] for x in facts if x[0] == E.REPAIRED] or [0])


def same_as_fresh(W, old, seed, target, C, where):
    """the rule from the kept part of the old field reaches the oracle's fresh plan on W's current state"""
    code, dist, pred, path, _ = R.replan(W, old.dist, seed, target, OFF, C, target, OFF)
    ref = W.om.dijkstra(W.weights, W.costs, seed, target, OFF, R.LIMIT)
    assert code == ref.code and np.array_equal(bits(dist), bits(ref.dist)) and np.array_equal(pred, ref.pred), where
    assert np.array_equal(path, ref.path), where


def test_batch70_without_the_fresh_class():
    seeds, targets, patch = E.batch70()
    W = R.World(48, True)
    old, C, facts = facts_of(W, seeds, targets, ("costs", patch, 1.5), 0.0)
    assert counts(facts) == (31, 39, 0)
    part = partly_kept(facts)
    assert len(part) >= 4 and longest_frontier(facts) > WM.TB_TILE[48]
    for p in part[:3]:
        same_as_fresh(W, old[p], seeds[p], targets[p], C, ("batch70", p))


def test_batch70_at_the_default_fraction():
    seeds, targets, patch = E.batch70()
    _, _, facts = facts_of(R.World(48, True), seeds, targets, ("costs", patch, 1.5), E.F_DEFAULT)
    assert counts(facts) == (31, 30, 9)
    assert len(partly_kept(facts)) >= 4 and longest_frontier(facts) > WM.TB_TILE[48]


def test_mixed12_laid_and_lifted():
    seeds, targets, patch = E.mixed12()
    W = R.World(96, True)
    back = W.costs[patch].copy()
    old = None
    for k, ev in enumerate([("costs", patch, 1.5), ("costs", patch, back)]):
        old, C, facts = facts_of(W, seeds, targets, ev, E.F_DEFAULT, old)
        assert counts(facts) == (4, 4, 4), (k, counts(facts))
        part = partly_kept(facts)
        assert len(part) == 4 and longest_frontier(facts) > WM.TB_TILE[96], (k, longest_frontier(facts))
        same_as_fresh(W, old[part[0]], seeds[part[0]], targets[part[0]], C, ("mixed12", k))
        old = oracle_all(W, seeds, targets)


def test_the_k_tbv_solve_batch_repairs_more_than_a_flag_block():
    seeds, targets, patch = WM.tbv_batch()
    _, _, facts = facts_of(R.World(160, True), seeds, targets, ("costs", patch, 1.5), 0.0)
    k, r, f = counts(facts)
    assert r > 64 and f == 0 and k + r == 96, (k, r, f)
    assert len(partly_kept(facts)) >= 4 and longest_frontier(facts) > WM.TB_TILE[160]


@functools.lru_cache(maxsize=None)
def batch_facts():
    """per scenario of WM.BATCH_SCENARIOS and step: (expect, the plans' facts without the FRESH class)"""
    out = {}
    by_name = {s.name: s for s in R.scenarios()}
    for name in WM.BATCH_SCENARIOS:
        sc = by_name[name]
        assert sc.reason == 0 and sc.fields, name
        W = R.World(sc.N, sc.computed)
        targets, offset = list(sc.targets), sc.offset
        old = oracle_all(W, sc.seeds, targets, offset)
        rows = []
        for st in sc.steps:
            C = [W.apply(ev) for ev in st.events]
            C = np.concatenate(C) if C else np.zeros(0, np.uint32)
            new_t = list(st.targets) if st.targets is not None else targets
            rows.append((st.expect, WM.plan_facts(W, old, sc.seeds, targets, offset, C, new_t, st.offset, 0.0)))
            old, targets, offset = oracle_all(W, sc.seeds, new_t, st.offset), new_t, st.offset
        out[name] = rows
    return out


def test_the_batch_scenarios_cover_the_edge_cases():
    rows = batch_facts()
    assert set(rows) == set(WM.BATCH_SCENARIOS)
    at_cut = seed_only = partial = 0
    for name, steps in rows.items():
        for expect, facts in steps:
            for c, L, cut, kept, rew, reached, fr in facts:
                at_cut += bits(L) == bits(cut); seed_only += kept == 1; partial += kept > 1 and rew > 0
                assert expect != "cut" or bits(L) == bits(cut), name
                assert expect != "all" or kept == 1, name
                assert expect != "partial" or 0 < rew < reached, name
    assert at_cut >= 1 and seed_only >= 1 and partial >= 4, (at_cut, seed_only, partial)
    # moved targets with no event: a target inside the kept part, whose new cut lies below kept values
    expect, facts = rows["targets48"][0]
    sc = next(x for x in R.scenarios() if x.name == "targets48")
    W = R.World(sc.N, sc.computed)
    d = oracle_all(W, sc.seeds, sc.targets, sc.offset)[0].dist
    L, moved = facts[0][1], sc.steps[0].targets[0]
    assert expect == "cut" and not sc.steps[0].events and d[moved] < L and int((d[moved] + sc.steps[0].offset < d)[d < L].sum()) > 0
    # the 170-plan batch spans the 64-plan flag block with partly kept fields and a frontier longer than a tile
    expect, facts = rows["batch170"][0]
    assert len(facts) == 170 and sum(1 for x in facts if x[3] > 1 and x[4] > 0) >= 4 and max(x[6] for x in facts) > WM.TB_TILE[48]


def test_the_policy_steps_repair_between_8_and_160_plans():
    """tests/test_gpu_replan_warm.py test_policy_fall_back_and_a_stale_cancel: four steps, the patch laid and lifted twice"""
    seeds, targets, patch = E.batch70()
    W = R.World(48, True)
    back = W.costs[patch].copy()
    old = None
    for k in range(4):
        old, _, facts = facts_of(W, seeds, targets, ("costs", patch, back if k % 2 else 1.5), 0.0, old)
        assert 8 <= counts(facts)[1] <= 160 and counts(facts)[2] == 0, (k, counts(facts))
        old = oracle_all(W, seeds, targets)
