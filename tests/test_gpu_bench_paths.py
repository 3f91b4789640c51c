"""GPU: the three paths `bench.py` runs that had no `-m gpu` test of their own (VERDICT r03 "missing" #3):

  (a) the tile-batch engine on the C4 mesh (10M vertices) with a batch large enough to take it (>= 1024 plans):
      vertex paths and popped potential of a sample against the oracle (dijkstra_mesh_planner.cpp:287-348, :358-373);
  (b) V-sized outputs of a 64-plan batch at C2 scale through the tile-batch engine's own finalize pass (`k_tb_finalize`):
      potential / predecessors / vector map bits of >= 8 plans against the oracle (:189-209, :293-300);
  (c) `mnav_cancel` during a large tile-batch run: every plan CANCELED (:287, :350-354), a later batch unaffected (:238).
"""
import threading
import time

import numpy as np
import pytest

from mesh_navigation_amd import capi, meshgen
from oracle import oracle as O
from tests.common import terrain_case

pytestmark = pytest.mark.gpu


def _popped(full, t, offset):
    dt = full[t]
    gd = np.float32(np.float64(dt) + offset) if np.isfinite(dt) else np.float32(np.inf)
    return full <= gd


class C4:
    """The 10M-vertex mesh of config C4, its oracle, one batch of 1024 plans and the oracle's answers to the plans the tests of this
    module sample: generated once per process."""

    def __init__(self):
        self.mesh = mesh = meshgen.terrain(3163, 0.1, 4)
        self.w = meshgen.edge_lengths(mesh)
        self.costs = np.zeros(mesh.V, np.float32)
        self.om = O.OracleMesh(mesh.xyz, mesh.faces)
        rng = np.random.default_rng(41)
        self.n = n = 1024
        self.seeds = rng.choice(mesh.V, n, replace=False).astype(np.uint32)
        self.targets = rng.choice(mesh.V, n, replace=False).astype(np.uint32)
        self.targets[: n // 2] = mesh.vertex_at(0.9, 0.9)             # the bench's common robot vertex and scattered ones
        self._refs = {}

    def oracle(self, k):
        """(the plan at offset 0.3, the full-field potential) of plan k"""
        if k not in self._refs:
            ref = self.om.dijkstra(self.w, self.costs, int(self.seeds[k]), int(self.targets[k]))
            full = self.om.dijkstra(self.w, self.costs, int(self.seeds[k]), int(self.targets[k]), goal_dist_offset=np.inf).dist
            self._refs[k] = (ref, full)
        return self._refs[k]

    def context(self, gpu_ctx_factory):
        ctx = gpu_ctx_factory()
        ctx.upload_mesh(self.mesh.xyz, self.mesh.faces, self.mesh.edges, None)
        ctx.upload_costs(self.costs, self.w)
        ctx.set_dijkstra_engine("tile_batch")
        return ctx


@pytest.fixture(scope="module")
def c4():
    return C4()


def test_c4_tile_batch_1024_plans_paths_and_popped_potential(gpu_ctx_factory, c4):
    mesh, n, seeds, targets = c4.mesh, c4.n, c4.seeds, c4.targets
    ctx = c4.context(gpu_ctx_factory)
    b = ctx.plan_dijkstra_batch(seeds, targets, want_fields=False, path_cap=32768)
    assert b["rc"] == 0 and (b["codes"] == 0).all()
    assert b["stats"]["n_plans"] == n
    for k in (0, 511, 777, 1023):
        ref, full = c4.oracle(k)
        assert ref.code == 0
        assert np.array_equal(b["paths"][k], ref.path), k
        pot = ctx.download_output("popped", k)
        m = _popped(full, int(targets[k]), 0.3)
        assert np.array_equal(pot[m].view(np.uint32), full[m].view(np.uint32)), k
        assert np.isinf(pot[~m]).all()
    # size-independent property over a spread of the plans: a path starts at the wave source and ends next to the robot
    # vertex (reference list order seed ... pred[target]), every hop is an edge of the grid mesh (meshgen: id = j * N + i,
    # cells split along v00 - v11)
    N = 3163
    for k in range(0, n, 37):
        p = b["paths"][k].astype(np.int64)
        assert p[0] == seeds[k]
        hops = np.abs(np.diff(np.concatenate([p, [int(targets[k])]])))
        assert np.isin(hops, (1, N, N + 1)).all(), k
    ctx.close()


def test_c4_register_resident_kernel_band_4(gpu_ctx_factory, c4):
    """The same batch on k_tbv_solve (`tb_kernel` 1): 1024 plans on ~92 600 tiles are 3.4 plans per tile and iteration, so the band is
    the 4 tile widths `auto` gives the C4 bench leg (4096 plans) -- at a quarter of its memory.  Paths and popped potential of the
    first and last plan and of the two either side of the first 64-plan boundary."""
    n, seeds, targets = c4.n, c4.seeds, c4.targets
    ctx = c4.context(gpu_ctx_factory)
    ctx.set_option("tb_kernel", 1)
    try:
        b = ctx.plan_dijkstra_batch(seeds, targets, want_fields=False, path_cap=32768)
        print("kernel that ran:", ctx.last_engine())
        assert "k_tbv_solve" in ctx.last_engine(), ctx.last_engine()
        assert b["rc"] == 0 and (b["codes"] == 0).all()
        assert b["stats"]["n_plans"] == n
        for k in (0, 63, 64, 1023):
            ref, full = c4.oracle(k)
            assert ref.code == 0
            assert np.array_equal(b["paths"][k], ref.path), k
            pot = ctx.download_output("popped", k)
            m = _popped(full, int(targets[k]), 0.3)
            assert np.array_equal(pot[m].view(np.uint32), full[m].view(np.uint32)), k
            assert np.isinf(pot[~m]).all()
    finally:
        ctx.close()


def test_c2_tile_batch_fields_and_vector_map_full_groups(gpu_ctx_factory):
    """64 plans with V-sized outputs on the 1M mesh, written by the tile-batch engine's finalize pass (`k_tb_finalize`: with this
    engine the V-sized outputs never go through `k_dij_finalize`): exactly one full plan range of 64."""
    case = terrain_case(1000, 2)
    ctx = gpu_ctx_factory()
    case.upload(ctx)
    ctx.set_dijkstra_engine("tile_batch")
    ctx.set_resident_outputs(True)                                    # the vector map of every plan stays on the device
    m = case.mesh
    rng = np.random.default_rng(29)
    n = 64
    seeds = rng.choice(m.V, n, replace=False).astype(np.uint32)
    targets = rng.choice(m.V, n, replace=False).astype(np.uint32)
    targets[:32] = m.vertex_at(0.9, 0.9)
    b = ctx.plan_dijkstra_batch(seeds, targets, want_fields=True, path_cap=16384)
    assert b["rc"] == 0 and (b["codes"] == 0).all()
    for k in (0, 7, 8, 15, 16, 31, 32, 40, 55, 63):                   # first / last lanes of several groups
        ref = case.om.dijkstra(case.weights, case.costs, int(seeds[k]), int(targets[k]))
        assert ref.code == 0
        assert np.array_equal(b["paths"][k], ref.path), k
        assert np.array_equal(b["dist"][k].view(np.uint32), ref.dist.view(np.uint32)), k
        assert np.array_equal(b["pred"][k], ref.pred), k
        vm = case.om.dijkstra_vector_map(ref.pred)                    # computeVectorMap :189-209
        got = ctx.download_output("vecmap", k)
        assert np.array_equal(got.view(np.uint32), vm.view(np.uint32)), k
    ctx.set_resident_outputs(False)
    ctx.close()


def test_cancel_stops_a_running_tile_batch(gpu_ctx_factory):
    case = terrain_case(1000, 2)
    ctx = gpu_ctx_factory()
    case.upload(ctx)
    ctx.set_dijkstra_engine("tile_batch")
    m = case.mesh
    rng = np.random.default_rng(13)
    n = 7168
    seeds = rng.choice(m.V, n, replace=False).astype(np.uint32)
    targets = np.full(n, m.vertex_at(0.5, 0.5), np.uint32)
    kw = dict(goal_dist_offset=float("inf"), want_fields=False, path_cap=4096, want_stats=False)
    full = ctx.plan_dijkstra_batch(seeds, targets, **kw)              # warm-up: builds the streams, allocates the batch
    assert full["rc"] == 0 and (full["codes"] == 0).all()
    t0 = time.perf_counter()
    full = ctx.plan_dijkstra_batch(seeds, targets, **kw)
    t_full = time.perf_counter() - t0
    ref_paths = [full["paths"][k].copy() for k in (0, 100, 7167)]
    out = {}
    th = threading.Thread(target=lambda: out.update(ctx.plan_dijkstra_batch(seeds, targets, **kw)))
    t0 = time.perf_counter()
    th.start()
    time.sleep(min(0.05, 0.25 * t_full))
    ctx.cancel()
    th.join(timeout=120)
    t_cancel = time.perf_counter() - t0
    assert not th.is_alive()
    assert out["rc"] == capi.CANCELED and (out["codes"] == capi.CANCELED).all(), (out["rc"], t_full, t_cancel)
    assert t_cancel < t_full, (t_cancel, t_full)
    st = ctx.stats()                                                  # must not touch the cancelled batch's freed / stale state
    assert st is not None
    again = ctx.plan_dijkstra_batch(seeds, targets, **kw)             # same size: the interrupted buffers are reused
    assert again["rc"] == 0 and (again["codes"] == 0).all()
    for k, p in zip((0, 100, 7167), ref_paths):
        assert np.array_equal(again["paths"][k], p)
    ctx.close()
