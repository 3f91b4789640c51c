"""GPU: the schedule pass of the tile-batch engine (k_tb_sched, mnav_tb.h: one wave owns a tile for the iteration, reads the
tile's flag bytes 64 blocks at a time, walks the set blocks in ascending order and fills the tile's bucket from a running count)
against the sequential oracle, bit for bit, on the hub mesh of tests/test_gpu_tbv_parity.py:

  a. plan counts 1, 64, 65, 129 (one, one full, two and three blocks of 64 plans, the last one partial) and 4097 (65 blocks: the
     tile's flag row does not fit one 64-lane load, and its last chunk holds a single flag), on both solve kernels, with bands of
     1 and 4 tile widths (more or fewer carried values per block) and one solve wave per CU: fields and vector map of every plan
     (4097: of 16 sampled plans, and the return codes of all of them), then paths only with the popped potential;
  b. a per-plan replan after a cost change: the warm start (k_tb_warm) sets pending values and flags itself and feeds the same
     schedule pass.

The bucket order within a tile (ascending by plan now) is not observable: the fixed point does not depend on it.  The smallest
carried value per plan goes through 64 arrays (copy = tile mod 64) that k_tb_plan folds: the hub mesh has more tiles than copies
(16 384 vertices in tiles of 120), so copies are shared."""
import functools

import numpy as np
import pytest

from tests import replan_each_model as E
from tests.test_gpu_replan_each import oracle_all
from tests.test_gpu_replan_warm import each_step, pair, ran_warm, recorded_by_tile_batch
from tests.test_gpu_tbv_parity import (TBQ, TBV, assert_engine, assert_fields_equal_oracle, assert_paths_equal_oracle, hub_reference, open_ctx,
                                       sample_of, setup)

pytestmark = pytest.mark.gpu

OFFSET = 0.3
BIG = 4097


@functools.lru_cache(maxsize=1)
def big_batch():
    """4097 plans on the hub mesh: the 257 of the parity file, then random usable vertices; the oracle's code of every plan and
    its full result (with the vector map) for 16 sampled plans."""
    su = setup("hub")
    c = su.case
    rng = np.random.default_rng(4097)
    ok = np.flatnonzero((c.invalid == 0) & (c.costs <= su.cost_limit) & (su.deg > 0))
    seeds = np.concatenate([su.seeds, rng.choice(ok, BIG - su.seeds.size)]).astype(np.uint32)
    targets = np.concatenate([su.targets, rng.choice(ok, BIG - su.targets.size)]).astype(np.uint32)
    same = seeds == targets
    seeds[same] = ok[(np.searchsorted(ok, seeds[same]) + 1) % ok.size]
    assert not (seeds == targets).any()
    # the code of a plan: whether the wave from the seed reaches the target at all -- one oracle run per distinct seed would do,
    # but the plans are cheap at this size (16 384 vertices, the wave stops at the goal)
    full = [c.om.dijkstra(c.weights, c.costs, int(s), int(t), goal_dist_offset=OFFSET, cost_limit=su.cost_limit, invalid=c.invalid) for s, t in zip(seeds, targets)]
    codes = np.array([r.code for r in full], np.uint32)
    sample = sample_of(BIG, np.random.default_rng(11))
    refs = {k: (full[k], c.om.dijkstra_vector_map(full[k].pred)) for k in sample}
    return seeds, targets, codes, sample, refs


def plans_and_refs(n):
    su = setup("hub")
    if n == BIG:
        seeds, targets, codes, sample, refs = big_batch()
        return seeds, targets, codes, sample, refs
    seeds, targets = su.plans(n)
    refs = hub_reference()[:n]
    return seeds, targets, np.array([r.code for r, _ in refs], np.uint32), list(range(n)), dict(enumerate(refs))


@pytest.mark.parametrize("n", [1, 64, 65, 129, BIG])
def test_plan_counts_bands_and_both_solve_kernels_equal_the_oracle(gpu_ctx_factory, n):
    su = setup("hub")
    seeds, targets, codes, sample, refs = plans_and_refs(n)
    assert n < 64 or len(set(codes.tolist())) > 1                      # reachable and unreachable targets in one batch
    ctx = open_ctx(gpu_ctx_factory, su, tb_waves_per_cu=1)
    try:
        for band in (1, 4):
            ctx.set_option("tb_band_mult", band)
            for kernel, want in ((0, TBQ), (1, TBV)):
                ctx.set_option("tb_kernel", kernel)
                b = ctx.plan_dijkstra_batch(seeds, targets, goal_dist_offset=OFFSET, cost_limit=su.cost_limit, want_fields=True)
                assert_engine(ctx, want)
                assert b["stats"]["n_plans"] == n
                assert np.array_equal(np.asarray(b["codes"], np.uint32), codes), (n, band, want)
                assert_fields_equal_oracle(ctx, b, seeds, targets, refs, ("hub", n, band, want))
        # paths only: no finalize pass, the lazy walk and the popped potential straight from the blocked distances
        ctx.set_resident_outputs(False)
        cache = {}
        for kernel, want in ((0, TBQ), (1, TBV)):
            ctx.set_option("tb_kernel", kernel)
            b = ctx.plan_dijkstra_batch(seeds, targets, goal_dist_offset=OFFSET, cost_limit=su.cost_limit, want_fields=False)
            assert_engine(ctx, want)
            assert np.array_equal(np.asarray(b["codes"], np.uint32), codes), (n, want, "paths only")
            assert_paths_equal_oracle(su.case, ctx, b, seeds, targets, sample, OFFSET, su.cost_limit, ("hub", n, want, "paths only"), cache)
    finally:
        ctx.close()


def test_a_warm_replan_feeds_the_same_schedule_pass(gpu_ctx_factory):
    """batch70 of the replan tests, recorded by the tile-batch engine; a cost patch, then one per-plan replan: the repaired plans
    start warm and run through k_tb_sched with a band of 4 tile widths and one solve wave per CU.  Every output against a fresh
    plan on a second context and against the oracle (each_step)."""
    seeds, targets, patch = E.batch70()
    W, A, B = pair(gpu_ctx_factory, 48, 64)
    try:
        A.set_option("replan_fresh_below", 0)
        A.set_option("tb_band_mult", 4)
        A.set_option("tb_waves_per_cu", 1)
        recorded_by_tile_batch(A, seeds, targets, 0)
        old = oracle_all(W, seeds, targets)
        a, m, _ = each_step(W, A, B, seeds, targets, old, ("costs", patch, 1.5), 0.0, "batch70 warm, band 4")
        nr = int((m[0] == E.REPAIRED).sum())
        assert nr >= 10
        ran_warm(A, a, nr, "k_tb_solve_q")
    finally:
        A.close(); B.close()
