"""GPU: the schedule pass of the tile-batch engine with the carried minima reduced per workgroup in LDS (k_tb_sched, mnav_tb.h),
against the sequential oracle, bit for bit: return code, vertex path, potential and predecessors of EVERY plan.

  a. `meshgen.terrain(72, 0.1, 2)` -- 5184 vertices, about 45 tiles of 120: no multiple of any workgroup's tile count, so the last
     workgroup has waves without a tile that still have to reach its barriers -- with 161, 193, 257 and 1000 plans (the last block
     of 64 plans is partial, and the threads that send the workgroup's minima walk past the end of the array), on both solve
     kernels, and the same batches with `tb_sched_lds` = 0: both paths against the same oracle
     results, so against each other;
  b. 16 448 plans on `meshgen.terrain(24, 0.1, 2)`: their words do not fit the LDS of a workgroup, the batch has to take the
     global path by itself and still match (257 distinct plans, repeated: the oracle runs once per distinct plan);
  c. one per-plan replan after a cost change: the warm start (k_tb_warm) sets the pending values and feeds the same pass;
  d. a batch on the hub mesh of tests/test_gpu_tbv_parity.py on k_tb_solve_q (items of 16 plans), both paths.

Which path a batch took is read from the engine's trace line (option `trace`), which engine and kernel ran from `last_engine()`
and the call's statistics.  Iteration and item counts are not pinned: they depend on the schedule, the result does not."""
import functools

import numpy as np
import pytest

from mesh_navigation_amd import meshgen
from tests import replan_each_model as E
from tests.common import Case
from tests.test_gpu_replan_each import oracle_all
from tests.test_gpu_replan_warm import each_step, pair, ran_warm, recorded_by_tile_batch
from tests.test_gpu_tbv_parity import TBQ, TBV, assert_engine, hub_reference, open_ctx, setup

pytestmark = pytest.mark.gpu

OFFSET = 0.3
IN_LDS, IN_GLOBAL = "carried minima reduced in LDS", "carried minima in global memory"


class Batch:
    """`distinct` random plans on a terrain (seed != target) and the oracle's result of each."""

    def __init__(self, N, distinct):
        self.case = c = Case(meshgen.terrain(N, 0.1, 2))
        rng = np.random.default_rng(N)
        V = c.mesh.V
        self.seeds = rng.choice(V, distinct, replace=distinct > V).astype(np.uint32)
        self.targets = rng.choice(V, distinct, replace=distinct > V).astype(np.uint32)
        self.targets[distinct // 2:] = self.targets[0]                   # a common robot vertex, like the bench, and scattered ones
        same = self.seeds == self.targets
        self.seeds[same] = (self.seeds[same] + 1) % V
        refs = [c.om.dijkstra(c.weights, c.costs, int(s), int(t), goal_dist_offset=OFFSET) for s, t in zip(self.seeds, self.targets)]
        self.codes = np.array([r.code for r in refs], np.uint32)
        self.dist = np.stack([r.dist for r in refs]).view(np.uint32)
        self.pred = np.stack([r.pred for r in refs])
        self.paths = [r.path for r in refs]


@functools.lru_cache(maxsize=None)
def batch(N, distinct):
    return Batch(N, distinct)


def trace_lines(capfd):
    return [l for l in capfd.readouterr().err.splitlines() if "tile-batch:" in l]


def run_and_compare(ctx, capfd, B, n, want_path, want_kernel, tag):
    """plans k = 0 .. n - 1 are B's plan k mod len(B.seeds); every output of every plan against the oracle"""
    idx = np.arange(n) % B.seeds.size
    seeds, targets = B.seeds[idx], B.targets[idx]
    capfd.readouterr()
    b = ctx.plan_dijkstra_batch(seeds, targets, goal_dist_offset=OFFSET, want_fields=True)
    lines = trace_lines(capfd)
    assert_engine(ctx, want_kernel)
    assert b["rc"] == 0 and b["stats"]["n_plans"] == n and b["stats"]["launches"] == 1 and b["stats"]["steps"] > 0, (tag, b["stats"])
    assert len(lines) == 1 and want_path in lines[0], (tag, lines)
    assert np.array_equal(np.asarray(b["codes"], np.uint32), B.codes[idx]), tag
    assert np.array_equal(b["dist"].view(np.uint32), B.dist[idx]), tag
    assert np.array_equal(b["pred"], B.pred[idx]), tag
    for k in range(n):
        assert np.array_equal(b["paths"][k], B.paths[idx[k]]), (tag, k)


def terrain_ctx(gpu_ctx_factory, B):
    ctx = gpu_ctx_factory()
    ctx.set_option("trace", 1)
    B.case.upload(ctx)
    ctx.set_dijkstra_engine("tile_batch")
    return ctx


@pytest.mark.parametrize("n", [161, 193, 257, 1000])
def test_partial_plan_blocks_on_both_paths_and_both_solve_kernels(gpu_ctx_factory, capfd, n):
    B = batch(72, 1000)
    assert (B.codes == 0).sum() > 500
    ctx = terrain_ctx(gpu_ctx_factory, B)
    try:
        for lds, want_path in ((None, IN_LDS), (0, IN_GLOBAL)):
            ctx.set_option("tb_sched_lds", lds)
            for kernel, want in ((1, TBV), (0, TBQ)):
                ctx.set_option("tb_kernel", kernel)
                run_and_compare(ctx, capfd, B, n, want_path, want, (72, n, lds, want))
    finally:
        ctx.close()


def test_a_batch_beyond_the_lds_takes_the_global_path_by_itself(gpu_ctx_factory, capfd):
    B = batch(24, 257)
    n = 16448                                                            # 4 x 16 448 bytes of minima > 64 KB
    ctx = terrain_ctx(gpu_ctx_factory, B)
    try:
        run_and_compare(ctx, capfd, B, n, IN_GLOBAL, "k_tb", (24, n, "default"))
        ctx.set_option("tb_sched_lds", 1)                                # asking for it does not make it fit
        run_and_compare(ctx, capfd, B, n, IN_GLOBAL, "k_tb", (24, n, "asked for"))
    finally:
        ctx.close()


def test_a_warm_replan_feeds_the_lds_pass(gpu_ctx_factory, capfd):
    """batch70 of the replan tests recorded by the tile-batch engine, a cost patch, one per-plan replan: the repaired plans start
    warm (k_tb_warm) and run through the schedule pass at its defaults.  Every output against a fresh plan on a second context and
    against the oracle (each_step)."""
    seeds, targets, patch = E.batch70()
    W, A, B = pair(gpu_ctx_factory, 48, 64)
    try:
        A.set_option("replan_fresh_below", 0)
        A.set_option("trace", 1)
        recorded_by_tile_batch(A, seeds, targets, 0)
        old = oracle_all(W, seeds, targets)
        capfd.readouterr()
        a, m, _ = each_step(W, A, B, seeds, targets, old, ("costs", patch, 1.5), 0.0, "batch70 warm, minima in LDS")
        lines = trace_lines(capfd)
        nr = int((m[0] == E.REPAIRED).sum())
        assert nr >= 10
        ran_warm(A, a, nr, "k_tb_solve_q")
        assert len(lines) == 1 and IN_LDS in lines[0], lines
    finally:
        A.close(); B.close()


def test_the_hub_mesh_on_quarter_wave_items_on_both_paths(gpu_ctx_factory, capfd):
    su = setup("hub")
    n = 257
    seeds, targets = su.plans(n)
    refs = hub_reference()
    ctx = open_ctx(gpu_ctx_factory, su, tb_kernel=0, trace=1)
    ctx.set_resident_outputs(False)
    try:
        for lds, want_path in ((None, IN_LDS), (0, IN_GLOBAL)):
            ctx.set_option("tb_sched_lds", lds)
            capfd.readouterr()
            b = ctx.plan_dijkstra_batch(seeds, targets, goal_dist_offset=OFFSET, cost_limit=su.cost_limit, want_fields=True)
            lines = trace_lines(capfd)
            assert_engine(ctx, TBQ)
            assert b["stats"]["n_plans"] == n and b["stats"]["launches"] == 1 and b["stats"]["steps"] > 0, b["stats"]
            assert len(lines) == 1 and want_path in lines[0], lines
            for k, (ref, _) in enumerate(refs):
                at = ("hub", lds, k)
                assert b["codes"][k] == ref.code, at
                assert np.array_equal(b["paths"][k], ref.path), at
                assert np.array_equal(b["dist"][k].view(np.uint32), ref.dist.view(np.uint32)), at
                assert np.array_equal(b["pred"][k], ref.pred), at
    finally:
        ctx.close()
