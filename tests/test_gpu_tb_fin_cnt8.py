"""The settled-vertex count of the tile-batch finalize pass (option tb_fin_cnt8): a byte per (tile, plan),
stored 64 at a time by the wave that walks the block of plans and summed per plan behind the pass, instead of an atomicAdd per
reached pair.  The count of a batch -- the vertices with a finite potential, over all its plans -- must equal the oracle's and
must not depend on the option, and no output bit may change.

Shapes: the batches A and B of tests/test_gpu_tb_fin_keep.py (terrain(96), about 80 tiles; B after A skips the stores of the pairs
that are unreached again, whose bytes must be 0) at plan counts around the 64-plan block and with fewer plans than the rows of the
byte array are long; the hub terrain of tests/test_gpu_tbv_parity.py under its cost limit (robots that cannot be reached, valence
above the finalize slots); the helicoidal ramp of tests/folded_meshes.py (slices beyond 256 slots).  Both solve kernels where the
tiling allows both."""
import numpy as np
import pytest

from mesh_navigation_amd import capi
from tests import folded_meshes as FM
from tests.test_gpu_tb_fin_keep import N, assert_same_fields, batch, fields, world

pytestmark = pytest.mark.gpu
KERNELS = ((1, "k_tbv_solve"), (0, "k_tb_solve_q"))


def finite(refs):
    return int(sum(np.isfinite(r.dist).sum() for r, _ in refs))


@pytest.mark.parametrize("n", [63, 64, 65, 130])
def test_the_count_equals_the_oracle_with_bytes_and_with_atomics(n):
    W = world()
    want_a, want_b = finite(W.ref_a[:n]), finite(W.ref_b[:n])
    got = {}
    with W.context() as ctx:
        for kernel, name in KERNELS:
            ctx.set_option("tb_kernel", kernel)
            for cnt8 in (1, 0):
                ctx.set_option("tb_fin_cnt8", cnt8)
                a = batch(ctx, W.seeds_a[:n], W.targets_a[:n])
                b = batch(ctx, W.seeds_b[:n], W.targets_b[:n])           # B after A: the pass skips the pairs that are unreached again
                assert name in ctx.last_engine(), ctx.last_engine()
                print(n, name, "tb_fin_cnt8", cnt8, "settled", a["stats"]["settled"], b["stats"]["settled"], "oracle", want_a, want_b,
                      ctx.tb_finalize_stats())
                assert a["stats"]["settled"] == want_a and b["stats"]["settled"] == want_b, (n, name, cnt8)
                got[(kernel, cnt8)] = fields(ctx, n)
    for k in got:
        assert_same_fields(got[k], got[(1, 0)], str(k))


def test_fewer_plans_than_the_rows_are_long():
    W = world()
    with W.context() as ctx:
        for cnt8 in (1, 0):
            ctx.set_option("tb_fin_cnt8", cnt8)
            a = batch(ctx, W.seeds_a, W.targets_a)                       # 130 plans: the rows of the byte array
            b = batch(ctx, W.seeds_b[:70], W.targets_b[:70])
            assert a["stats"]["settled"] == finite(W.ref_a) and b["stats"]["settled"] == finite(W.ref_b[:70]), cnt8


def test_the_hub_terrain_under_its_cost_limit():
    from tests.test_gpu_tbv_parity import hub_reference, setup
    su = setup("hub")
    seeds, targets = su.plans(200)
    want = finite(hub_reference()[:200])
    with capi.MnavContext(0) as ctx:
        su.case.upload(ctx)
        ctx.set_dijkstra_engine("tile_batch")
        ctx.set_resident_outputs(True)
        for kernel, name in KERNELS:
            ctx.set_option("tb_kernel", kernel)
            for cnt8 in (1, 0):
                ctx.set_option("tb_fin_cnt8", cnt8)
                b = ctx.plan_dijkstra_batch(seeds, targets, 0.3, cost_limit=su.cost_limit)
                assert name in ctx.last_engine(), ctx.last_engine()
                assert list(b["codes"]) == [r.code for r, _ in hub_reference()[:200]]   # (some robots cannot be reached)
                assert b["stats"]["settled"] == want, (name, cnt8, b["stats"]["settled"], want)


def test_the_ramp_with_slices_beyond_256_slots():
    c = FM.case("ramp")
    seeds, targets = FM.plan_pairs("ramp", 72)
    want = 0
    for s, t in zip(seeds, targets):
        want += int(np.isfinite(c.om.dijkstra(c.weights, c.costs, int(s), int(t), goal_dist_offset=0.3).dist).sum())
    with capi.MnavContext(0) as ctx:
        c.upload(ctx)
        ctx.set_dijkstra_engine("tile_batch")
        ctx.set_resident_outputs(True)
        for cnt8 in (1, 0):
            ctx.set_option("tb_fin_cnt8", cnt8)
            b = ctx.plan_dijkstra_batch(seeds, targets, 0.3)
            assert b["rc"] == 0 and "k_tb_solve_q" in ctx.last_engine(), ctx.last_engine()
            assert b["stats"]["settled"] == want, (cnt8, b["stats"]["settled"], want)
