"""CPU companion of tests/test_gpu_engine_knobs.py: the inputs of that file are FAIR.  For every (case, band width, offset) it runs on
the band steps, the CPU model of the device schedule (oracle/schedule_model.cpp: the product's own rules and band controller, executed
serially) ends with code 0 under the evaluation orders 0, 2 and 3, its verification sweep finds every vertex at its fixed point and no
walk-limit flag, it produces the oracle's bits, and it needs fewer steps than a context's step cap.  A device plan may therefore return
INTERNAL_ERROR in none of them: a refusal on the device is the device's own.  The combinations come from tests/engine_knob_cases.py,
the list the GPU file parametrises over."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import engine_knob_cases as K

ORDERS = (0, 2, 3)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_cvp(c, plan_sp, sf, tf, mult, offset, at):
    ref = c.om.cvp(c.weights, c.costs, c.vn, plan_sp, sf, tf, goal_dist_offset=offset, invalid=c.invalid)
    assert ref.code in (O.SUCCESS, O.NO_PATH_FOUND), (at, ref.code)
    sv = c.mesh.faces[sf]
    upd = ref.pred != np.arange(c.mesh.V)
    cap = K.max_steps(c)
    for order in ORDERS:
        mod = O.schedule_model(1, c.mesh.faces, c.mesh.edges, c.weights, c.costs, sv, ref.dist[sv], sf, c.mesh.faces[tf], offset=offset,
                               delta=K.model_delta(c, mult, True), order=order, invalid=c.invalid, max_steps=cap)
        assert mod["code"] == 0, (at, order, mod["code"])
        assert mod["verify_bad"] == 0 and mod["verify_flags"] == 0, (at, order, mod["verify_bad"], mod["verify_flags"])
        assert mod["steps"] < cap, (at, order, mod["steps"])
        assert np.array_equal(bits(mod["dist"]), bits(ref.dist)) and np.array_equal(mod["pred"], ref.pred), (at, order)
        assert np.array_equal(mod["cutface"][upd], ref.cutface[upd]), (at, order)
        assert np.array_equal(bits(mod["direction"][upd]), bits(ref.direction[upd])), (at, order)
        assert mod["goal_dist"] == ref.stats["goal_dist"], (at, order)


@pytest.mark.parametrize("combo", K.CVP_SINGLE, ids=K.ident)
def test_cvp_single_plans_are_fair(combo):
    name, k, mult, offset = combo
    c = K.case(name)
    p = K.cvp_plans(name)[k]
    check_cvp(c, p.seed_pos, p.sf, p.tf, mult, offset, combo)


@pytest.mark.parametrize("combo", K.CVP_BATCH + K.CVP_BATCH_SHAPE, ids=K.ident)
def test_cvp_batch_plans_are_fair(combo):
    name, mult, offset = combo
    c = K.case(name)
    sps, sfs, tfs = K.cvp_batch(name)
    ran = 0
    for k in range(len(sfs)):
        if sfs[k] >= c.mesh.F:                                         # INVALID_START: answered on the host, no step runs
            continue
        check_cvp(c, sps[k], int(sfs[k]), int(tfs[k]), mult, offset, combo + (k,))
        ran += 1
    assert 0 < ran < len(sfs)


@pytest.mark.parametrize("combo", K.DIJKSTRA_BAND, ids=K.ident)
def test_band_dijkstra_plans_are_fair(combo):
    """A negative offset never reaches the band steps of a Dijkstra plan: the engines run with the bound of offset 0 and the passes
    behind them apply the reference's expanded set (mnav.hip dijkstra_impl, mnav_eval.h goal_cut), and the band steps hand such a call
    to the tile rounds (tests/test_gpu_folded_meshes.py; the GPU file asserts the kernel by name).  The model has no such pass, so it
    is held to the oracle at the offset the engines run with, max(offset, 0)."""
    name, k, mult, offset = combo
    c = K.case(name)
    s, t, lim = K.dijkstra_plans(name)[k]
    asked = c.om.dijkstra(c.weights, c.costs, s, t, goal_dist_offset=offset, cost_limit=lim, invalid=c.invalid)
    assert asked.code == (O.NO_PATH_FOUND if K.unreachable(name, k) else O.SUCCESS), (combo, asked.code)
    offset = max(offset, 0.0)
    ref = c.om.dijkstra(c.weights, c.costs, s, t, goal_dist_offset=offset, cost_limit=lim, invalid=c.invalid)
    cap = K.max_steps(c)
    for order in ORDERS:
        mod = O.schedule_model(0, c.mesh.faces, c.mesh.edges, c.weights, c.costs, [s], [0.0], O.NONE, [t], offset=offset, cost_limit=lim,
                               delta=K.model_delta(c, mult, False), order=order, invalid=c.invalid, max_steps=cap)
        assert mod["code"] == 0, (combo, order, mod["code"])
        assert mod["verify_bad"] == 0 and mod["verify_flags"] == 0, (combo, order)
        assert mod["steps"] < cap, (combo, order, mod["steps"])
        assert np.array_equal(bits(mod["dist"]), bits(ref.dist)) and np.array_equal(mod["pred"], ref.pred), (combo, order)
        assert mod["goal_dist"] == ref.stats["goal_dist"], (combo, order)


@pytest.mark.parametrize("radius", K.RADII)
def test_inflation_waves_are_fair(radius):
    """the wave's band is its radius: the model of mnav_layer_inflation ends clean with the oracle's distances at each of them"""
    c = K.case("L")
    lethal = K.lethal_of("L")
    cfg = O.InflationCfg.defaults()
    cfg.inflation_radius = radius
    _, dist, _ = c.om.inflation(lethal, c.edge_dist, cfg)
    for order in ORDERS:
        mod = O.schedule_model_inflation(c.mesh.faces, c.mesh.edges, c.edge_dist, lethal, max_distance=radius, order=order,
                                         max_steps=K.max_steps(c))
        assert mod["code"] == 0 and mod["verify_bad"] == 0 and mod["verify_flags"] == 0, (radius, order, mod["code"])
        assert mod["steps"] < K.max_steps(c)
        assert np.array_equal(bits(mod["dist"]), bits(dist)), (radius, order)
