"""The replan plan by plan (mnav_replan_dijkstra_each, include/mnav.h).  Comparisons are those of
tests/test_gpu_replan.py: context A replans per plan, context B plans afresh on the same map, and codes, path lengths, paths,
dist, pred, the resident vector map of every plan and the settled count are compared bit for bit; the first plan of every
step also against the oracle.  Through mnav_replan_each_stats every step shows which path each plan took: the class array, the
rewind levels and the kept / rewound counts are those of the numpy rule in tests/replan_each_model.py, which
tests/test_replan_each_model.py pins on the CPU (the batches and the class counts each scenario needs included).

Shapes: terrain(48) with tile_size 64 and terrain(96) at the default tile, as in tests/test_gpu_replan.py."""
import functools

import numpy as np
import pytest

from mesh_navigation_amd import capi
from tests import replan_each_model as E
from tests import replan_model as R
from tests.replan_model import bits
from tests.test_gpu_replan import same_as_oracle, same_outputs

pytestmark = pytest.mark.gpu
OFF = 0.3


def pair(factory, N, tile, resident=True, n=2):
    W = R.World(N, True)
    ctxs = [factory() for _ in range(n)]
    for c in ctxs:
        W.upload(c, tile)
        c.set_resident_outputs(resident)
        c.set_option("replan_each_fresh_share", 1)                     # every plan by its own class (the share policy has a test of its own)
    return (W, *ctxs)


def oracle_all(W, seeds, targets, offset=OFF):
    return [W.om.dijkstra(W.weights, W.costs, s, t, offset, R.LIMIT) for s, t in zip(seeds, targets)]


def event(W, ev, *ctxs):
    C = W.apply(ev)
    for c in ctxs:
        W.send(c, ev)
    return C


def model(W, old, seeds, targets, offset, C, new_t, new_off, f=E.F_DEFAULT, finalized=True):
    """classes, levels and the kept / rewound totals of the REPAIRED plans, by the numpy rule on the old potentials"""
    cls, lv, kept, rew = [], [], 0, 0
    for p, s in enumerate(seeds):
        c, L, _ = E.classify(W.N, old[p].dist, targets[p], offset, C, new_t[p], new_off, f, finalized)
        cls.append(c); lv.append(L)
        if c == E.REPAIRED:
            keep = R.keep_mask(old[p].dist, L, s)
            kept += int(keep.sum()); rew += int((~keep & np.isfinite(old[p].dist)).sum())
    return np.array(cls, np.uint8), np.array(lv, np.float32), kept, rew


def same_as_model(a, m, where, rewound=True):
    e = a["each"]
    print(where, {x: e[x] for x in e if x not in ("levels", "classes")}, list(e["classes"]))
    cls, lv, kept, rew = m
    assert e["reason"] == 0 and not e["whole_fresh"], (where, e)
    assert np.array_equal(e["classes"], cls), (where, list(e["classes"]), list(cls))
    assert np.array_equal(bits(e["levels"]), bits(lv)), where
    assert (e["kept_plans"], e["repaired_plans"], e["fresh_plans"]) == tuple(int((cls == c).sum()) for c in (E.KEPT, E.REPAIRED, E.FRESH)), where
    assert e["kept"] == kept, (where, e["kept"], kept)
    if rewound:
        assert e["rewound"] == rew, (where, e["rewound"], rew)


@functools.lru_cache(maxsize=None)
def mixed():
    return E.mixed12()


def test_mixed_classes_and_the_fleet_paths_after_them(gpu_ctx_factory):
    """One blocked patch laid and lifted among 12 plans: every class at least twice in each step, every plan compared; the
    FRESH plans run as a batch of their own on the asynchronous engine; afterwards mnav_fleet_paths serves every slot."""
    seeds, targets, patch = mixed()
    W, A, B = pair(gpu_ctx_factory, 96, None)
    n = len(seeds)
    assert A.plan_dijkstra_batch(seeds, targets, OFF, want_fields=True)["rc"] == 0 and "k_plan_async" in A.last_engine()
    old = oracle_all(W, seeds, targets)
    back = W.costs[patch].copy()
    for k, ev in enumerate([("costs", patch, 1.5), ("costs", patch, back)]):
        C = event(W, ev, A, B)
        m = model(W, old, seeds, targets, OFF, C, targets, OFF)
        for c in (E.KEPT, E.REPAIRED, E.FRESH):
            assert int((m[0] == c).sum()) >= 2, (k, list(m[0]))
        a = A.replan_dijkstra_each(None, OFF, want_dist=True, want_pred=True)
        b = B.plan_dijkstra_batch(seeds, targets, OFF, want_fields=True)
        same_as_model(a, m, ("mixed", k))
        same_outputs(A, B, a, b, n, True, ("mixed", k))
        old = oracle_all(W, seeds, targets)
        same_as_oracle(a, old[0], ("mixed", k))
        assert list(a["codes"]) == [r.code for r in old]
        assert a["each"]["log_len"] == C.size and a["each"]["tiles_woken"] > 0 and a["each"]["rounds"] > 0
        assert "k_tile_round" in A.last_engine() and "k_plan_async" in A.last_engine(), A.last_engine()
        assert "k_plan_async" in a["each"]["fresh_engine"]
    slots = np.arange(n, dtype=np.uint32)
    fa, fb = A.fleet_paths(slots, targets), B.fleet_paths(slots, targets)
    assert list(fa["codes"]) == [0] * n                                # a KEPT slot is served like every other
    for name in ("codes", "vertex", "path_len", "offsets", "ids"):
        assert np.array_equal(fa[name], fb[name]), name
    assert np.array_equal(bits(fa["potential"]), bits(fb["potential"]))
    for p in range(n):
        assert np.array_equal(fa["ids"][int(fa["offsets"][p]):int(fa["offsets"][p + 1])], old[p].path), p
    A.close(); B.close()


def test_the_same_after_a_tile_batch_call(gpu_ctx_factory):
    """70 plans, across the 64-plan block of the tile-batch engine that planned them; async_max_batch 4 keeps the FRESH batch
    off the asynchronous engine."""
    seeds, targets, patch = E.batch70()
    W, A, B = pair(gpu_ctx_factory, 48, 64)
    A.set_option("async_max_batch", 4)
    A.set_dijkstra_engine("tile_batch")
    assert A.plan_dijkstra_batch(seeds, targets, OFF, want_fields=True)["rc"] == 0 and "k_tb" in A.last_engine()
    A.set_dijkstra_engine("auto")
    old = oracle_all(W, seeds, targets)
    C = event(W, ("costs", patch, 1.5), A, B)
    m = model(W, old, seeds, targets, OFF, C, targets, OFF)
    assert min(int((m[0] == c).sum()) for c in (E.KEPT, E.REPAIRED, E.FRESH)) >= 5 and int((m[0] == E.FRESH).sum()) > 4
    a = A.replan_dijkstra_each(None, OFF, want_dist=True, want_pred=True)
    b = B.plan_dijkstra_batch(seeds, targets, OFF, want_fields=True)
    same_as_model(a, m, "batch70")
    same_outputs(A, B, a, b, 70, True, "batch70")
    new = oracle_all(W, seeds, targets)
    same_as_oracle(a, new[0], "batch70")
    assert list(a["codes"]) == [r.code for r in new]
    assert "k_tile_round" in A.last_engine() and "k_plan_async" not in A.last_engine() and "k_tb" not in A.last_engine(), A.last_engine()
    assert "k_tile_round" in a["each"]["fresh_engine"]
    A.close(); B.close()


def test_all_kept(gpu_ctx_factory):
    """An event beyond every cut, same targets and offset: no plan runs anything, and nothing resident is written."""
    seeds, targets, patch = mixed()
    seeds, targets = seeds[0::3], targets[0::3]                        # the four goals whose fields end far from the patch
    W, A, B = pair(gpu_ctx_factory, 96, None)
    n = len(seeds)
    a0 = A.plan_dijkstra_batch(seeds, targets, OFF, want_fields=True)
    vm0 = [A.download_output("vecmap", p) for p in range(n)]
    old = oracle_all(W, seeds, targets)
    C = event(W, ("costs", patch, 1.5), A, B)
    m = model(W, old, seeds, targets, OFF, C, targets, OFF)
    assert list(m[0]) == [E.KEPT] * n
    a = A.replan_dijkstra_each(None, OFF, want_dist=True, want_pred=True)
    b = B.plan_dijkstra_batch(seeds, targets, OFF, want_fields=True)
    same_as_model(a, m, "all kept")
    e = a["each"]
    assert e["rewound"] == 0 and e["kept"] == 0 and e["rounds"] == 0 and e["tiles_woken"] == 0 and e["ms_finalize"] == 0.0 and e["ms_rounds"] == 0.0
    assert e["fresh_engine"] is None and "every plan kept" in A.last_engine()
    same_outputs(A, B, a, b, n, True, "all kept")
    same_outputs(A, A, a, a0, n, False, "all kept, the previous call")
    for p in range(n):
        assert np.array_equal(bits(A.download_output("vecmap", p)), bits(vm0[p])), p
    same_as_oracle(a, oracle_all(W, seeds[:1], targets[:1])[0], "all kept")
    a2 = A.replan_dijkstra_each(None, OFF, want_dist=True, want_pred=True)   # ... and again, with an empty log
    assert list(a2["each"]["classes"]) == [E.KEPT] * n and a2["each"]["log_len"] == 0
    same_outputs(A, B, a2, b, n, True, "all kept, twice")
    A.close(); B.close()


def test_a_paths_only_call_is_repaired_not_kept(gpu_ctx_factory):
    seeds, targets, patch = mixed()
    seeds, targets = seeds[0::3], targets[0::3]
    W, A, B = pair(gpu_ctx_factory, 96, None, resident=False)
    n = len(seeds)
    assert A.plan_dijkstra_batch(seeds, targets, OFF, want_fields=False)["rc"] == 0
    old = oracle_all(W, seeds, targets)
    C = event(W, ("costs", patch, 1.5), A, B)
    m = model(W, old, seeds, targets, OFF, C, targets, OFF, finalized=False)
    assert list(m[0]) == [E.REPAIRED] * n
    a = A.replan_dijkstra_each(None, OFF, want_dist=True, want_pred=True)
    b = B.plan_dijkstra_batch(seeds, targets, OFF, want_fields=True)
    same_as_model(a, m, "paths only", rewound=False)                   # (beyond the cut a paths-only field holds the engine's values)
    same_outputs(A, B, a, b, n, False, "paths only")
    same_as_oracle(a, oracle_all(W, seeds[:1], targets[:1])[0], "paths only")
    a = A.replan_dijkstra_each(None, OFF, want_dist=True, want_pred=True)   # the replan left finalized fields: now they are kept
    assert list(a["each"]["classes"]) == [E.KEPT] * n
    same_outputs(A, B, a, b, n, False, "paths only, then kept")
    A.close(); B.close()


def test_moved_targets_without_a_map_event(gpu_ctx_factory):
    """New robot vertices inside the old cut, on its last expanded vertex and in the unreached region: none is KEPT."""
    W, A, B = pair(gpu_ctx_factory, 48, 64)
    s = W.v(0.15, 0.5)
    seeds, targets = [s] * 3, [W.v(0.6, 0.5)] * 3
    assert A.plan_dijkstra_batch(seeds, targets, OFF, want_fields=True)["rc"] == 0
    old = oracle_all(W, seeds, targets)
    d = old[0].dist
    cut = R.old_cut(d, targets[0], OFF)
    at = int(np.flatnonzero(d <= cut)[np.argmax(d[d <= cut])])
    new_t = [W.v(0.3, 0.5), at, W.v(0.98, 0.98)]
    assert d[new_t[0]] < cut and d[at] <= cut and np.isinf(d[new_t[2]])
    none = np.zeros(0, np.uint32)
    m = model(W, old, seeds, targets, OFF, none, new_t, OFF)
    assert E.KEPT not in list(m[0])
    a = A.replan_dijkstra_each(new_t, OFF, want_dist=True, want_pred=True)
    b = B.plan_dijkstra_batch(seeds, new_t, OFF, want_fields=True)
    same_as_model(a, m, "targets")
    same_outputs(A, B, a, b, 3, True, "targets")
    same_as_oracle(a, oracle_all(W, seeds[:1], new_t[:1])[0], "targets")
    A.close(); B.close()


def test_without_the_fresh_class(gpu_ctx_factory):
    """replan_fresh_below = 0: no plan is FRESH, KEPT plans are still kept, the rest is the repair of
    mnav_replan_dijkstra_batch, which a third context runs."""
    seeds, targets, patch = mixed()
    W, A, B, D = pair(gpu_ctx_factory, 96, None, n=3)
    n = len(seeds)
    for c in (A, D):
        c.set_option("replan_fresh_below", 0)
        assert c.plan_dijkstra_batch(seeds, targets, OFF, want_fields=True)["rc"] == 0
    old = oracle_all(W, seeds, targets)
    C = event(W, ("costs", patch, 1.5), A, B, D)
    m = model(W, old, seeds, targets, OFF, C, targets, OFF, f=0.0)
    assert int((m[0] == E.FRESH).sum()) == 0 and int((m[0] == E.KEPT).sum()) >= 2 and int((m[0] == E.REPAIRED).sum()) >= 4
    a = A.replan_dijkstra_each(None, OFF, want_dist=True, want_pred=True)
    b = B.plan_dijkstra_batch(seeds, targets, OFF, want_fields=True)
    d = D.replan_dijkstra(None, OFF, want_dist=True, want_pred=True)
    assert d["replan"]["reason"] == 0
    same_as_model(a, m, "f = 0")
    assert a["each"]["fresh_engine"] is None and "k_tile_round" in A.last_engine() and "async" not in A.last_engine()
    same_outputs(A, B, a, b, n, True, "f = 0")
    same_outputs(A, D, a, d, n, True, "f = 0, the batch replan")
    A.close(); B.close(); D.close()


def test_the_share_policy_plans_the_whole_call_afresh(gpu_ctx_factory):
    seeds, targets, patch = mixed()
    W, A, B = pair(gpu_ctx_factory, 96, None)
    n = len(seeds)
    A.set_option("replan_each_fresh_share", 0)
    assert A.plan_dijkstra_batch(seeds, targets, OFF, want_fields=True)["rc"] == 0
    old = oracle_all(W, seeds, targets)
    C = event(W, ("costs", patch, 1.5), A, B)
    m = model(W, old, seeds, targets, OFF, C, targets, OFF)
    a = A.replan_dijkstra_each(None, OFF, want_dist=True, want_pred=True)
    b = B.plan_dijkstra_batch(seeds, targets, OFF, want_fields=True)
    e = a["each"]
    assert e["whole_fresh"] and e["reason"] == 4 and a["replan"]["reason"] == 4, e
    assert np.array_equal(e["classes"], m[0]) and e["fresh_plans"] >= 2 and e["kept"] == 0 and e["rewound"] == 0
    assert "k_plan_async" in A.last_engine() and "k_tile_round" not in A.last_engine()
    same_outputs(A, B, a, b, n, True, "share")
    A.set_option("replan_each_fresh_share", 1)                         # 1: never
    old = oracle_all(W, seeds, targets)
    C = event(W, ("costs", patch, 0.2), A, B)
    m = model(W, old, seeds, targets, OFF, C, targets, OFF)
    a = A.replan_dijkstra_each(None, OFF, want_dist=True, want_pred=True)
    b = B.plan_dijkstra_batch(seeds, targets, OFF, want_fields=True)
    same_as_model(a, m, "share 1")
    same_outputs(A, B, a, b, n, True, "share 1")
    A.close(); B.close()


def test_refusals_and_a_stale_cancel(gpu_ctx_factory):
    sc = next(s for s in R.scenarios() if s.name == "wall48")
    W, A, B = pair(gpu_ctx_factory, 48, 64)
    with pytest.raises(RuntimeError, match="no Dijkstra call"):
        A.replan_dijkstra_each([3], OFF)
    empty = gpu_ctx_factory()
    with pytest.raises(RuntimeError, match="mnav_upload_mesh"):
        empty.replan_dijkstra_each([3], OFF)
    A.plan_dijkstra_batch(sc.seeds, sc.targets, OFF, want_fields=True)
    with pytest.raises(RuntimeError, match="n differs"):
        A.replan_dijkstra_each([sc.targets[0]] * 2, OFF)
    with pytest.raises(RuntimeError, match="NaN"):
        A.replan_dijkstra_each(None, float("nan"))
    ev = sc.steps[0].events[0]
    C = event(W, ev, A, B)
    A.cancel()                                                         # stale: cleared at entry
    a = A.replan_dijkstra_each(None, OFF, want_dist=True, want_pred=True)
    b = B.plan_dijkstra_batch(sc.seeds, sc.targets, OFF, want_fields=True)
    assert a["rc"] == capi.SUCCESS and a["each"]["reason"] == 0 and a["each"]["log_len"] == C.size and a["each"]["rewound"] > 0
    same_outputs(A, B, a, b, 1, True, "after the refusals")
    for c in (A, B, empty):
        c.close()
