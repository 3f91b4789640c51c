"""The warm repair: the repaired plans of a replan call on the tile-batch engine, started from their rewound fields by k_tb_warm
(option replan_repair_engine = 5; include/mnav.h mnav_replan_warm_stats).  Comparisons are those of
tests/test_gpu_replan.py and tests/test_gpu_replan_each.py: context A replans, context B plans afresh on the same map, and
codes, path lengths, paths, dist, pred, the resident vector map of every plan and the settled count are compared bit for bit;
plan 0 also against the oracle; the kept / rewound counts against the numpy rule (keep_mask).  Every test also shows that the new
path ran: "k_tb_warm" in the engine string and the number of plans repaired warm equal to the model's.
tests/test_replan_warm_model.py pins, on the CPU, what these scenarios rely on: class counts, partly kept fields, frontiers
longer than a tile, a level at the cut, a field with only its seed kept.

Shapes: terrain(48) with tb_tile 64 (about 40 tiles), terrain(96) and terrain(160) at the default 120 rows per tile; 160 x 160 is
the smallest mesh on which k_tbv_solve is accepted."""
import numpy as np
import pytest

from mesh_navigation_amd import capi
from tests import replan_each_model as E
from tests import replan_model as R
from tests import replan_warm_model as WM
from tests.replan_model import bits
from tests.test_gpu_replan import same_as_oracle, same_outputs
from tests.test_gpu_replan_each import event, model, oracle_all, same_as_model

pytestmark = pytest.mark.gpu
OFF = WM.OFF
SCENARIOS = {s.name: s for s in R.scenarios()}


def pair(factory, N, tile, repair_engine=5):
    """the world on two contexts: A keeps its fields and replans (warm), B plans afresh"""
    W = R.World(N, True)
    A, B = factory(), factory()
    for c in (A, B):
        c.set_option("tb_tile", WM.TB_TILE[N])                         # (read when the engine's streams are built)
        W.upload(c, tile)
        c.set_resident_outputs(True)
        c.set_option("replan_each_fresh_share", 1)                     # every plan by its own class
    A.set_option("replan_repair_engine", repair_engine)
    return W, A, B


def ran_warm(A, a, plans, kernel=None):
    w = a["warm"]
    print({x: w[x] for x in w})
    assert "k_tb_warm" in A.last_engine(), A.last_engine()
    assert w["plans"] == plans and w["fallback"] == 0 and w["live"], w
    assert w["iterations"] > 0 and w["pairs_woken"] > 0 and w["words"] > 0 and w["ms_warm"] > 0.0 and w["ms_finalize"] > 0.0, w
    if kernel:
        assert w["kernel"] == kernel and kernel in A.last_engine(), (w, A.last_engine())


def each_step(W, A, B, seeds, targets, old, ev, f, where, n_fresh_engine=None):
    """one event, one per-plan replan on A, one fresh plan on B, every comparison; returns (a, model, the new oracle results)"""
    n = len(seeds)
    C = event(W, ev, A, B)
    m = model(W, old, seeds, targets, OFF, C, targets, OFF, f=f)
    a = A.replan_dijkstra_each(None, OFF, want_dist=True, want_pred=True)
    b = B.plan_dijkstra_batch(seeds, targets, OFF, want_fields=True)
    same_as_model(a, m, where)
    same_outputs(A, B, a, b, n, True, where)
    new = oracle_all(W, seeds, targets)
    same_as_oracle(a, new[0], where)
    assert list(a["codes"]) == [r.code for r in new], where
    assert a["each"]["log_len"] == C.size
    return a, m, new


def recorded_by_tile_batch(A, seeds, targets, kernel):
    A.set_option("tb_kernel", kernel)
    A.set_dijkstra_engine("tile_batch")
    assert A.plan_dijkstra_batch(seeds, targets, OFF, want_fields=True)["rc"] == 0
    assert ("k_tbv_solve" if kernel else "k_tb_solve_q") in A.last_engine(), A.last_engine()
    A.set_dijkstra_engine("auto")


def test_the_repaired_plans_of_a_tile_batch_call_run_warm(gpu_ctx_factory):
    """batch70 without the FRESH class: 39 REPAIRED plans warm on k_tb_solve_q, 31 KEPT ones served from the compacted arrays"""
    seeds, targets, patch = E.batch70()
    W, A, B = pair(gpu_ctx_factory, 48, 64)
    A.set_option("replan_fresh_below", 0)
    recorded_by_tile_batch(A, seeds, targets, 0)
    old = oracle_all(W, seeds, targets)
    a, m, _ = each_step(W, A, B, seeds, targets, old, ("costs", patch, 1.5), 0.0, "batch70 warm")
    nr = int((m[0] == E.REPAIRED).sum())
    assert nr >= 10 and int((m[0] == E.FRESH).sum()) == 0 and int((m[0] == E.KEPT).sum()) >= 5
    ran_warm(A, a, nr, "k_tb_solve_q")
    e = a["each"]
    assert e["fresh_engine"] is None and e["rounds"] == a["warm"]["iterations"] and e["tiles_woken"] == a["warm"]["pairs_woken"], e
    assert e["ms_rewind"] == a["warm"]["ms_warm"] and e["ms_finalize"] == a["warm"]["ms_finalize"], e
    A.close(); B.close()


def test_kept_warm_and_fresh_plans_in_one_call(gpu_ctx_factory):
    """the same batch at the default replan_fresh_below: KEPT plans, a warm REPAIRED sub-batch and a FRESH sub-batch (on the tile
    rounds: async_max_batch 4 keeps it off the asynchronous engine); the engine string shows both"""
    seeds, targets, patch = E.batch70()
    W, A, B = pair(gpu_ctx_factory, 48, 64)
    A.set_option("async_max_batch", 4)
    recorded_by_tile_batch(A, seeds, targets, 0)
    old = oracle_all(W, seeds, targets)
    a, m, _ = each_step(W, A, B, seeds, targets, old, ("costs", patch, 1.5), E.F_DEFAULT, "batch70 three classes")
    assert min(int((m[0] == c).sum()) for c in (E.KEPT, E.REPAIRED, E.FRESH)) >= 5
    ran_warm(A, a, int((m[0] == E.REPAIRED).sum()), "k_tb_solve_q")
    assert "k_tile_round" in A.last_engine() and "k_tile_round" in a["each"]["fresh_engine"], A.last_engine()
    A.close(); B.close()


def test_two_warm_replans_in_a_row_then_fleet_paths_and_a_follower_tick(gpu_ctx_factory):
    """mixed12 recorded by the asynchronous engine; the patch is laid and lifted: the second replan rewinds fields a warm repair
    (and, for the KEPT and FRESH plans, other paths) left.  Afterwards every slot serves mnav_fleet_paths and mnav_follow_batch."""
    seeds, targets, patch = E.mixed12()
    W, A, B = pair(gpu_ctx_factory, 96, None)
    n = len(seeds)
    assert A.plan_dijkstra_batch(seeds, targets, OFF, want_fields=True)["rc"] == 0 and "k_plan_async" in A.last_engine()
    old = oracle_all(W, seeds, targets)
    back = W.costs[patch].copy()
    for k, ev in enumerate([("costs", patch, 1.5), ("costs", patch, back)]):
        a, m, old = each_step(W, A, B, seeds, targets, old, ev, E.F_DEFAULT, ("mixed warm", k))
        for c in (E.KEPT, E.REPAIRED, E.FRESH):
            assert int((m[0] == c).sum()) >= 2, (k, list(m[0]))
        ran_warm(A, a, int((m[0] == E.REPAIRED).sum()))
        assert "k_plan_async" in A.last_engine() and "k_plan_async" in a["each"]["fresh_engine"], A.last_engine()
    slots = np.arange(n, dtype=np.uint32)
    fa, fb = A.fleet_paths(slots, targets), B.fleet_paths(slots, targets)
    assert list(fa["codes"]) == [0] * n
    for name in ("codes", "vertex", "path_len", "offsets", "ids"):
        assert np.array_equal(fa[name], fb[name]), name
    assert np.array_equal(bits(fa["potential"]), bits(fb["potential"]))
    for p in range(n):
        assert np.array_equal(fa["ids"][int(fa["offsets"][p]):int(fa["offsets"][p + 1])], old[p].path), p
    m_ = W.mesh
    rng = np.random.default_rng(12)
    at = rng.integers(0, m_.V, 48)
    pos = (m_.xyz[at] + rng.uniform(-0.03, 0.03, (48, 3))).astype(np.float32)
    d = np.tile(np.array([1.0, 0.0, 0.0], np.float32), (48, 1))
    up = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (48, 1))
    face = np.full(48, capi.NONE, np.uint32)
    fslots = (np.arange(48) % n).astype(np.uint32)
    ta, tb = A.follow(pos, d, up, face, fslots), B.follow(pos, d, up, face, fslots)
    assert (ta.code == 0).any()
    for name in ("code", "face", "bary", "pos", "mesh_dir", "cost", "cmd", "how"):
        x, y = getattr(ta, name), getattr(tb, name)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), name
    A.close(); B.close()


def test_the_warm_start_of_k_tbv_solve(gpu_ctx_factory):
    """terrain(160), 96 plans recorded by k_tbv_solve, no FRESH class: more than 64 REPAIRED plans, so the warm sub-batch spans
    two 64-plan flag blocks and fills whole waves of the register kernel"""
    seeds, targets, patch = WM.tbv_batch()
    W, A, B = pair(gpu_ctx_factory, 160, None)
    A.set_option("replan_fresh_below", 0)
    recorded_by_tile_batch(A, seeds, targets, 1)
    old = oracle_all(W, seeds, targets)
    a, m, _ = each_step(W, A, B, seeds, targets, old, ("costs", patch, 1.5), 0.0, "tbv warm")
    nr = int((m[0] == E.REPAIRED).sum())
    assert nr > 64
    ran_warm(A, a, nr, "k_tbv_solve")
    A.close(); B.close()


@pytest.mark.parametrize("name", WM.BATCH_SCENARIOS)
def test_the_batch_replan_runs_all_plans_warm(gpu_ctx_factory, name):
    """mnav_replan_dijkstra_batch over the reason-0 scenarios of tests/replan_model.py, every step of each: all n plans warm"""
    sc = SCENARIOS[name]
    W = R.World(sc.N, sc.computed)
    A, B = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (A, B):
        c.set_option("tb_tile", WM.TB_TILE[sc.N])
        W.upload(c, sc.tile)
        c.set_resident_outputs(sc.fields)
    A.set_option("replan_fresh_below", 0)
    A.set_option("replan_repair_engine", 5)
    n, seeds = len(sc.seeds), np.array(sc.seeds, np.uint32)
    targets, offset = list(sc.targets), sc.offset
    A.set_dijkstra_engine(sc.engine)
    assert A.plan_dijkstra_batch(seeds, targets, offset, want_fields=sc.fields)["rc"] == 0
    A.set_dijkstra_engine("auto")
    old = [W.om.dijkstra(W.weights, W.costs, s, t, offset, R.LIMIT) for s, t in zip(sc.seeds, targets)]
    for k, st in enumerate(sc.steps):
        where = (sc.name, k)
        C = []
        for ev in st.events:
            C.append(W.apply(ev))
            W.send(A, ev)
            W.send(B, ev)
        C = np.concatenate(C) if C else np.zeros(0, np.uint32)
        new_t = list(st.targets) if st.targets is not None else targets
        a = A.replan_dijkstra(None if st.targets is None else new_t, st.offset, want_dist=True, want_pred=True)
        b = B.plan_dijkstra_batch(seeds, new_t, st.offset, want_fields=True)
        rp = a["replan"]
        print(sc.name, k, {x: rp[x] for x in rp if x != "levels"})
        same_outputs(A, B, a, b, n, sc.fields, where)
        new = [W.om.dijkstra(W.weights, W.costs, s, t, st.offset, R.LIMIT) for s, t in zip(sc.seeds, new_t)]
        same_as_oracle(a, new[0], where)
        assert list(a["codes"]) == [r.code for r in new], where
        assert st.codes is None or list(a["codes"]) == st.codes, where
        assert rp["reason"] == 0 and rp["log_len"] == C.size, (where, rp)
        ran_warm(A, a, n)
        assert A.last_engine().startswith("k_tb_warm"), A.last_engine()
        kept = rew = 0
        for p in range(n):
            cut = R.old_cut(old[p].dist, targets[p], offset)
            L = R.level(sc.N, old[p].dist, C, cut)
            keep = R.keep_mask(old[p].dist, L, sc.seeds[p])
            assert bits(rp["levels"][p]) == bits(L), (where, p, rp["levels"][p], L)
            kept += int(keep.sum()); rew += int((~keep & np.isfinite(old[p].dist)).sum())
            if st.expect == "cut":
                assert bits(L) == bits(cut), (where, p)
            if st.expect == "all":
                assert int(keep.sum()) == 1, (where, p)
        assert rp["kept"] == kept and rp["rewound"] == rew, (where, rp["kept"], kept, rp["rewound"], rew)
        assert rp["rounds"] == a["warm"]["iterations"] and rp["tiles_woken"] == a["warm"]["pairs_woken"], rp
        old, targets, offset = new, new_t, st.offset
    A.close(); B.close()


def test_policy_fall_back_and_a_stale_cancel(gpu_ctx_factory):
    """With both options unset and 70 plans the repair is today's (the tile rounds), and with replan_repair_engine = 0 at any
    number; replan_warm_min_plans = 8 sends the automatic mode to the warm start; a stale mnav_cancel does not cancel it.  A
    recorded paths-only tile-batch call holds nothing to rewind: reason 1, whatever the option."""
    seeds, targets, patch = E.batch70()
    W, A, B = pair(gpu_ctx_factory, 48, 64, repair_engine=None)
    A.set_option("replan_fresh_below", 0)
    recorded_by_tile_batch(A, seeds, targets, 0)
    old = oracle_all(W, seeds, targets)
    back = W.costs[patch].copy()
    steps = [(None, None, False), (0, None, False), (None, 8, True), (None, 8, True)]
    for k, (engine, min_plans, warm) in enumerate(steps):
        A.set_option("replan_repair_engine", engine)
        A.set_option("replan_warm_min_plans", min_plans)
        if k == 3:
            A.cancel()                                                 # stale: cleared at entry
        a, m, old = each_step(W, A, B, seeds, targets, old, ("costs", patch, back if k % 2 else 1.5), 0.0, ("policy", k))
        nr = int((m[0] == E.REPAIRED).sum())
        assert a["rc"] == capi.SUCCESS and 8 <= nr <= 160
        if warm:
            ran_warm(A, a, nr)
        else:
            assert A.last_engine() == "k_tile_round (tile rounds)" and a["warm"]["plans"] == 0 and a["warm"]["fallback"] == 0, (A.last_engine(), a["warm"])
            assert a["each"]["rounds"] > 0 and a["each"]["tiles_woken"] > 0
    A.close(); B.close()
    sc = SCENARIOS["pathsonly_tile_batch"]
    W = R.World(sc.N, sc.computed)
    A, B = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (A, B):
        W.upload(c, sc.tile)
        c.set_resident_outputs(False)
    A.set_option("replan_repair_engine", 5)
    A.set_dijkstra_engine("tile_batch")
    assert A.plan_dijkstra_batch(sc.seeds, sc.targets, OFF, want_fields=False)["rc"] == 0
    A.set_dijkstra_engine("auto")
    for ev in sc.steps[0].events:
        event(W, ev, A, B)
    a = A.replan_dijkstra(None, OFF, want_dist=True, want_pred=True)
    b = B.plan_dijkstra_batch(sc.seeds, sc.targets, OFF, want_fields=True)
    assert a["replan"]["reason"] == 1 and a["warm"]["plans"] == 0 and "k_tb_warm" not in A.last_engine(), (a["replan"], a["warm"])
    same_outputs(A, B, a, b, len(sc.seeds), False, "paths only")
    A.close(); B.close()
