"""GPU: the two hot kernels of the tile-batch engine at the shapes they ship at -- k_tbv_solve (mnav_tbv.h: the tile's distances
in a window of VGPRs, three stream passes over V-layout blocks with continuation blocks for rows of more than six sources) and
k_tb_finalize (mnav_tb_finalize.h: potential with the reference's cut-off semantics, predecessors, vector map) -- against the
sequential oracle (dijkstra_mesh_planner.cpp:189-209, :287-373), bit for bit:

  a. irregular topology on both solve kernels: valence 4 / 8 everywhere (union-jack: half of all vertices have sources in finalize
     slots 6 and 7), hubs of valence 8 .. 40 (the overflow list) with face-less vertices, a flat union-jack full of equal
     potentials (the exact branch: several sources attaining the value), a punched mesh with two components, the valence-40 fan;
     offsets 0.3, 0, inf, -0.2, -inf; costs, a cost limit and invalid vertices; EVERY plan of a 200-plan batch: return code, vertex
     path, potential, predecessors, vector map;
  b. plan counts around the 64-plan blocks (lanes past the batch's end, finalize's partial last plan range);
  c. bands and residency: they change the schedule, never the result;
  d. the sizes `bench.py` runs, under `auto`: 1M vertices with 1024 / 4096 plans (V-sized outputs resident) and 7168 plans paths only,
     the 64 concurrent goals of config C5 on the asynchronous engine.  (The 10M mesh: tests/test_gpu_bench_paths.py.)

Every test asserts which kernel ran (`last_engine()`): a test that meant k_tbv_solve and got the other kernel fails.  The meshes of
(a) - (c) are asserted eligible for k_tbv_solve (<= 64 ghosts per tile) on the CPU model in tests/test_tb_model.py."""
import functools

import numpy as np
import pytest

from mesh_navigation_amd import meshgen
from tests.common import Case, terrain_case

pytestmark = pytest.mark.gpu

HUBS = [(20, 20, 1), (60, 30, 2), (40, 90, 3), (100, 100, 5), (64, 64, 1), (90, 40, 2)]
OFFSETS = (0.3, 0.0, float("inf"), -0.2, float("-inf"))
HUB_COST_LIMIT = 0.8
TBV, TBQ, ASYNC = "k_tbv_solve", "k_tb_solve_q", "k_plan_async"


def build_mesh(name):
    if name == "union_jack":
        return meshgen.union_jack(96, 0.1, 3, 0.5)
    if name == "hub":
        return meshgen.hub_terrain(128, HUBS, 0.1, 3)
    if name == "flat_union_jack":
        return meshgen.union_jack(48, 1.0, flat=True)
    if name == "punched":
        return meshgen.punched(96, 0.1, 5, drop=0.30, cut_column=60)
    if name == "fan":
        return meshgen.fan_field(40, 6, 1)
    raise KeyError(name)


class Setup:
    """A mesh, its oracle-side arrays and a fixed list of plans that visits the mesh's special vertices."""

    def __init__(self, name):
        self.name = name
        mesh = self.mesh = build_mesh(name)
        rng = np.random.default_rng(101)
        deg = self.deg = np.bincount(mesh.edges.ravel(), minlength=mesh.V)
        self.cost_limit = 1.0
        if name == "hub":
            N = mesh.N
            costs = rng.uniform(0.0, 1.2, mesh.V).astype(np.float32)
            inv = (rng.uniform(size=mesh.V) < 0.03).astype(np.uint8)
            self.hubs = np.array([cj * N + ci for ci, cj, _ in HUBS])
            near = np.unique(np.concatenate([mesh.edges[np.isin(mesh.edges, self.hubs).any(axis=1)].ravel(), self.hubs]))
            costs[near] = rng.uniform(0.0, 0.5, near.size).astype(np.float32)   # the hubs and their rings stay usable: paths run over them
            inv[near] = 0
            self.case = Case(mesh, costs, edge_cost_factor=1.0, invalid=inv)
            self.cost_limit = HUB_COST_LIMIT
            ok = np.flatnonzero((inv == 0) & (costs <= HUB_COST_LIMIT) & (deg > 0))
            ring = np.setdiff1d(near, self.hubs)
            special = np.concatenate([self.hubs, ring[:: max(1, ring.size // 24)], np.flatnonzero(deg == 0)[:6],
                                      np.flatnonzero(inv == 1)[:3], np.flatnonzero(costs > HUB_COST_LIMIT)[:3]])
        else:
            self.case = Case(mesh)
            ok = np.flatnonzero(deg > 0)
            special = np.concatenate([np.flatnonzero(deg == deg.max())[:8], np.flatnonzero(deg == 0)[:6]])
            if name == "punched":                                       # both components as sources and as targets
                col = np.arange(mesh.V) % mesh.N
                special = np.concatenate([special, ok[col[ok] > 60][:12]])
            if name == "flat_union_jack":                               # the centre: its potential field is eightfold symmetric, 8 vertices tie with any goal
                special = np.concatenate([special, [mesh.vertex_at(0.5, 0.5)] * 8])
        special = special.astype(np.uint32)
        n = 257                                                          # the longest batch of this file; the 200-plan tests take a prefix
        self.seeds = rng.choice(ok, n, replace=ok.size < n).astype(np.uint32)
        self.targets = rng.choice(ok, n, replace=ok.size < n).astype(np.uint32)
        ns = min(special.size, 60) & ~1
        self.seeds[10:10 + ns:2] = special[:ns:2]                        # special vertices as wave sources ...
        self.targets[11:11 + ns:2] = special[1:ns:2]                     # ... and as targets, in the plans between
        self.targets[100:160] = self.targets[100]                       # a common robot vertex, like the bench
        self.seeds[181] = self.seeds[180]                               # duplicate sources
        same = self.seeds == self.targets
        self.seeds[same] = ok[(np.searchsorted(ok, self.seeds[same]) + 1) % ok.size]    # no seed == target by accident (it changes the batch size)
        assert not (self.seeds == self.targets).any()

    def plans(self, n, with_seed_equals_target=False):
        s, t = self.seeds[:n].copy(), self.targets[:n].copy()
        if with_seed_equals_target:
            s[7] = t[7]
        return s, t

    def reference(self, seeds, targets, offset, want_vecmap=True):
        c = self.case
        out = []
        for s, t in zip(seeds, targets):
            ref = c.om.dijkstra(c.weights, c.costs, int(s), int(t), goal_dist_offset=offset, cost_limit=self.cost_limit, invalid=c.invalid)
            out.append((ref, c.om.dijkstra_vector_map(ref.pred) if want_vecmap else None))       # computeVectorMap :189-209
        return out


@functools.lru_cache(maxsize=None)
def setup(name):
    return Setup(name)


@functools.lru_cache(maxsize=1)
def hub_reference():
    """The 257 plans of the hub mesh at offset 0.3: shared by (b) and (c)."""
    su = setup("hub")
    return su.reference(su.seeds, su.targets, 0.3)


def popped(full, t, offset):
    dt = full[t]
    gd = np.float32(np.float64(dt) + offset) if np.isfinite(dt) else np.float32(np.inf)
    return full <= gd


def assert_engine(ctx, want):
    got = ctx.last_engine()
    print("kernel that ran:", got)
    assert want in got, (want, got)


def assert_fields_equal_oracle(ctx, b, seeds, targets, refs, tag):
    """Exact comparison of a batch that left its V-sized outputs on the device (resident outputs): code, path, potential and vector
    map bits, predecessors -- of the plans in `refs` (index -> (oracle result, oracle vector map))."""
    items = refs.items() if isinstance(refs, dict) else enumerate(refs)
    for k, (ref, vm) in items:
        at = (tag, k, int(seeds[k]), int(targets[k]))
        assert b["codes"][k] == ref.code, at
        assert np.array_equal(b["paths"][k], ref.path), at
        if seeds[k] == targets[k]:                                      # :252-255: SUCCESS right after clearing the maps; the plan never reaches the device
            assert ref.code == 0 and len(ref.path) == 0
            if b["dist"] is not None:
                assert np.isinf(b["dist"][k]).all() and np.array_equal(b["pred"][k], np.arange(ctx.V, dtype=np.uint32)), at
            continue
        dist = b["dist"][k] if b["dist"] is not None else ctx.download_output("dist", k)
        pred = b["pred"][k] if b["pred"] is not None else ctx.download_output("pred", k)
        assert np.array_equal(dist.view(np.uint32), ref.dist.view(np.uint32)), at
        assert np.array_equal(pred, ref.pred), at
        got = ctx.download_output("vecmap", k)
        assert np.array_equal(got.view(np.uint32), vm.view(np.uint32)), at


def assert_paths_equal_oracle(case, ctx, b, seeds, targets, sample, offset, cost_limit, tag, cache=None):
    """A paths-only batch: code and vertex path, and the popped potential (dist <= goal_dist exact, +inf elsewhere) as
    tests/test_gpu_tile_batch.py checks it.  `cache` keeps the oracle's results for a second batch of the same plans."""
    def oracle(k, off):
        key = (k, off)
        if cache is None or key not in cache:
            r = case.om.dijkstra(case.weights, case.costs, int(seeds[k]), int(targets[k]), goal_dist_offset=off, cost_limit=cost_limit, invalid=case.invalid)
            if cache is None:
                return r
            cache[key] = r
        return cache[key]

    for k in sample:
        at = (tag, k, int(seeds[k]), int(targets[k]))
        ref = oracle(k, offset)
        assert b["codes"][k] == ref.code, at
        assert np.array_equal(b["paths"][k], ref.path), at
        if ref.code == 0 and seeds[k] != targets[k]:
            full = oracle(k, np.inf).dist
            pot = ctx.download_output("popped", k)
            m = popped(full, int(targets[k]), offset)
            assert np.array_equal(pot[m].view(np.uint32), full[m].view(np.uint32)), at
            assert np.isinf(pot[~m]).all(), at


def open_ctx(gpu_ctx_factory, su, **options):
    ctx = gpu_ctx_factory()
    for k, v in options.items():
        ctx.set_option(k, v)
    su.case.upload(ctx)
    ctx.set_dijkstra_engine("tile_batch")
    ctx.set_resident_outputs(True)                                      # the vector map of every plan stays on the device
    return ctx


# ---------------------------------------------------------------------------------------------------------------- a. topology
@pytest.mark.parametrize("name", ["union_jack", "hub", "flat_union_jack", "punched", "fan"])
def test_irregular_topology_every_plan_on_both_solve_kernels(gpu_ctx_factory, name):
    su = setup(name)
    n = 200
    seeds, targets = su.plans(n, with_seed_equals_target=True)
    ctx = open_ctx(gpu_ctx_factory, su)
    try:
        for offset in OFFSETS:
            refs = su.reference(seeds, targets, offset)
            if offset == 0.3:                                           # the batch is not trivial: paths exist, and on the split meshes some do not
                codes = [r.code for r, _ in refs]
                assert codes.count(0) > n // 2
                assert name not in ("hub", "punched") or len(set(codes)) > 1
            for kernel, want in ((0, TBQ), (1, TBV)):
                ctx.set_option("tb_kernel", kernel)
                b = ctx.plan_dijkstra_batch(seeds, targets, goal_dist_offset=offset, cost_limit=su.cost_limit, want_fields=True)
                assert_engine(ctx, want)
                assert b["stats"]["n_plans"] == n - 1                   # (the seed == target plan is answered on the host)
                assert_fields_equal_oracle(ctx, b, seeds, targets, refs, (name, offset, want))
        # paths only (no finalize pass): the lazy path walk and the popped potential straight from the solve kernel's blocked distances
        ctx.set_resident_outputs(False)
        cache = {}
        for kernel, want in ((0, TBQ), (1, TBV)):
            ctx.set_option("tb_kernel", kernel)
            for offset in (0.3, float("inf")):
                b = ctx.plan_dijkstra_batch(seeds, targets, goal_dist_offset=offset, cost_limit=su.cost_limit, want_fields=False)
                assert_engine(ctx, want)
                assert_paths_equal_oracle(su.case, ctx, b, seeds, targets, range(n), offset, su.cost_limit, (name, offset, want, "paths only"), cache)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------------ b. plan counts
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 257])
def test_plan_count_edges_on_the_register_resident_kernel(gpu_ctx_factory, n):
    """Lanes past NP in the last 64-plan block of k_tbv_solve, and k_tb_finalize's plan ranges (64 plans each) with a partial last
    range: fields and vector map of every plan."""
    su = setup("hub")
    seeds, targets = su.plans(n)
    refs = hub_reference()[:n]
    ctx = open_ctx(gpu_ctx_factory, su, tb_kernel=1)
    try:
        b = ctx.plan_dijkstra_batch(seeds, targets, goal_dist_offset=0.3, cost_limit=su.cost_limit, want_fields=True)
        assert_engine(ctx, TBV)
        assert b["stats"]["n_plans"] == n
        assert_fields_equal_oracle(ctx, b, seeds, targets, refs, ("hub", n))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------- c. bands and residency
@pytest.mark.parametrize("waves_per_cu", [1, None])
def test_band_and_residency_change_the_schedule_never_the_result(gpu_ctx_factory, waves_per_cu):
    """tb_band_mult 1 / 2 / 4 / 6 (4 is what `auto` gives k_tbv_solve below 40 plans per tile and iteration: the whole 10M bench leg)
    and one wave per CU against the default residency, both kernels: all outputs equal the oracle's, so each other's."""
    su = setup("hub")
    n = 200
    seeds, targets = su.plans(n)
    refs = hub_reference()[:n]
    ctx = open_ctx(gpu_ctx_factory, su, **({} if waves_per_cu is None else {"tb_waves_per_cu": waves_per_cu}))
    try:
        for band in (1, 2, 4, 6):
            ctx.set_option("tb_band_mult", band)
            for kernel, want in ((0, TBQ), (1, TBV)):
                ctx.set_option("tb_kernel", kernel)
                b = ctx.plan_dijkstra_batch(seeds, targets, goal_dist_offset=0.3, cost_limit=su.cost_limit, want_fields=True)
                assert_engine(ctx, want)
                assert_fields_equal_oracle(ctx, b, seeds, targets, refs, ("hub", band, waves_per_cu, want))
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- d. the sizes that are benched
def sample_of(n, rng, count=16):
    """Plans 0 and 63 of the first, a middle and the last 64-plan block, and random ones.  (The engine orders a batch by the tile of
    the wave source, so a caller's index is not its lane: the random ones spread over lanes and blocks either way.)"""
    mid = (n // 128) * 64
    last = ((n - 1) // 64) * 64
    fixed = [0, 63, mid, mid + 63, last, n - 1]
    rest = [int(k) for k in rng.permutation(n) if k not in fixed][: count - len(fixed)]
    return fixed + rest


@pytest.mark.parametrize("n", [1024, 4096])
def test_c2_auto_resident_fields_of_large_batches(gpu_ctx_factory, n):
    """1M vertices under `auto`: 1024 plans (10.6 plans per tile and iteration: k_tbv_solve with band 4) and 4096 plans (42.6: the
    default band; 64 plan ranges in k_tb_finalize).  Potential, predecessors and vector map of every plan stay on the device;
    16 sampled plans are downloaded and compared."""
    case = terrain_case(1000, 2)
    m = case.mesh
    ctx = gpu_ctx_factory()
    try:
        case.upload(ctx)
        ctx.set_resident_outputs(True)
        rng = np.random.default_rng(1000 + n)
        seeds = rng.choice(m.V, n, replace=False).astype(np.uint32)
        targets = np.full(n, m.vertex_at(0.9, 0.9), np.uint32)
        targets[: n // 4] = rng.choice(m.V, n // 4, replace=False)       # not only the common robot vertex
        same = seeds == targets
        seeds[same] = (seeds[same] + 1) % m.V
        b = ctx.plan_dijkstra_batch(seeds, targets, goal_dist_offset=0.3, want_fields=False, path_cap=16384)
        assert_engine(ctx, TBV)
        assert b["rc"] == 0 and (b["codes"] == 0).all()
        assert b["stats"]["n_plans"] == n
        refs = {}
        for k in sample_of(n, rng):
            ref = case.om.dijkstra(case.weights, case.costs, int(seeds[k]), int(targets[k]))
            refs[k] = (ref, case.om.dijkstra_vector_map(ref.pred))
        assert_fields_equal_oracle(ctx, b, seeds, targets, refs, ("C2 auto", n))
    finally:
        ctx.close()


def test_c2_auto_7168_plans_paths_only_as_benched(gpu_ctx_factory):
    """The headline batch as `bench.py` issues it -- 7168 goals from rng(5), common robot vertex, offset 0.3, rows of 16384 -- without
    the resident fields (those need 234 GB: the benchmark's business, not the suite's)."""
    case = terrain_case(1000, 2)
    m = case.mesh
    n = 7168
    ctx = gpu_ctx_factory()
    try:
        case.upload(ctx)
        goals = np.random.default_rng(5).choice(m.V, size=n, replace=False).astype(np.uint32)
        robots = np.full(n, m.vertex_at(0.9, 0.9), np.uint32)
        b = ctx.plan_dijkstra_batch(goals, robots, goal_dist_offset=0.3, want_fields=False, path_cap=16384)
        assert_engine(ctx, TBV)
        assert b["rc"] == 0 and (b["codes"] == 0).all()
        assert_paths_equal_oracle(case, ctx, b, goals, robots, sample_of(n, np.random.default_rng(7)), 0.3, 1.0, "C2 7168")
    finally:
        ctx.close()


def test_c5_64_concurrent_goals_under_auto(gpu_ctx_factory):
    """Config C5 as BASELINE.md states it: the C2 mesh, 64 goals from rng(5), one batch under `auto` -- the asynchronous engine."""
    case = terrain_case(1000, 2)
    m = case.mesh
    ctx = gpu_ctx_factory()
    try:
        case.upload(ctx)
        robot = m.vertex_at(0.9, 0.9)
        goals = np.random.default_rng(5).choice(m.V, size=64, replace=False).astype(np.uint32)
        b = ctx.plan_dijkstra_batch(goals, np.full(64, robot, np.uint32), goal_dist_offset=0.3, want_fields=False, path_cap=16384)
        assert_engine(ctx, ASYNC)
        assert b["rc"] == 0
        for k in range(64):
            ref = case.om.dijkstra(case.weights, case.costs, int(goals[k]), robot)
            assert b["codes"][k] == ref.code == 0, k
            assert np.array_equal(b["paths"][k], ref.path), k
    finally:
        ctx.close()
