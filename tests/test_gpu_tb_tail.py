"""GPU: the tail of a Dijkstra batch (dijkstra_tail, mnav.hip) -- path walk, packed-path offsets computed on the device
(k_pack_offsets), k_pack_paths, and the clean-up of the tile-batch engine's other distance buffer launched behind the call's last
download instead of at the end of the call:

  a. back-to-back tile-batch calls with different goals on one context: the two distance buffers alternate, each call starts on
     the buffer cleaned behind the call before it while the host was still copying that call's paths out.  Every call equals the
     oracle, and a fourth call that repeats the first is bit-equal to it;
  b. a corridor mesh on which some paths are longer than the default path row and some are not, in one call: the offsets computed
     on the device serve the plans that fit, the call falls back to the host's sequence (second walk into exact rows, offsets
     from the host) for all of them.  Paths and lengths equal the oracle's."""
import numpy as np
import pytest

from mesh_navigation_amd import meshgen
from tests.common import Case
from tests.test_gpu_tbv_parity import TBV, assert_engine, assert_fields_equal_oracle, assert_paths_equal_oracle, hub_reference, open_ctx, setup

pytestmark = pytest.mark.gpu

OFFSET = 0.3


def outputs(ctx, b, n):
    return dict(codes=np.array(b["codes"]).copy(), paths=[np.array(p).copy() for p in b["paths"]],
                dist=np.stack([ctx.download_output("dist", k) for k in range(n)]), pred=np.stack([ctx.download_output("pred", k) for k in range(n)]),
                vecmap=np.stack([ctx.download_output("vecmap", k) for k in range(n)]))


def test_back_to_back_calls_alternate_the_distance_buffers_and_equal_the_oracle(gpu_ctx_factory):
    su = setup("hub")
    refs = hub_reference()
    n = 129
    windows = (slice(0, n), slice(128, 128 + n), slice(64, 64 + n), slice(0, n))   # three different sets of goals, then the first again
    ctx = open_ctx(gpu_ctx_factory, su, tb_kernel=1)
    try:
        first = None
        for call, w in enumerate(windows):
            seeds, targets = su.seeds[w], su.targets[w]
            b = ctx.plan_dijkstra_batch(seeds, targets, goal_dist_offset=OFFSET, cost_limit=su.cost_limit, want_fields=True)
            assert_engine(ctx, TBV)
            assert b["stats"]["n_plans"] == n
            assert_fields_equal_oracle(ctx, b, seeds, targets, refs[w], ("call", call))
            if call == 0:
                first = outputs(ctx, b, n)
            if call == 3:
                again = outputs(ctx, b, n)
                assert np.array_equal(again["codes"], first["codes"])
                assert all(np.array_equal(p, q) for p, q in zip(again["paths"], first["paths"]))
                for key in ("dist", "pred", "vecmap"):
                    assert np.array_equal(again[key].view(np.uint32), first[key].view(np.uint32)), key
        # the paths-only tail (k_tb_path) takes the same route: two more calls on the alternating buffers
        ctx.set_resident_outputs(False)
        for call, w in enumerate(windows[1:3]):
            seeds, targets = su.seeds[w], su.targets[w]
            b = ctx.plan_dijkstra_batch(seeds, targets, goal_dist_offset=OFFSET, cost_limit=su.cost_limit, want_fields=False)
            assert_engine(ctx, TBV)
            assert_paths_equal_oracle(su.case, ctx, b, seeds, targets, range(0, n, 8), OFFSET, su.cost_limit, ("paths-only call", call))
    finally:
        ctx.close()


def corridor(W, L, h, rng):
    ii, jj = np.meshgrid(np.arange(W), np.arange(L), indexing="xy")
    xyz = np.stack([ii.ravel() * h + rng.uniform(-0.02, 0.02, W * L), jj.ravel() * h + rng.uniform(-0.02, 0.02, W * L),
                    0.05 * np.sin(jj.ravel() * 0.01)], axis=1).astype(np.float32)
    f = []
    for j in range(L - 1):
        for i in range(W - 1):
            a = j * W + i
            f.append((a, a + 1, a + W + 1)); f.append((a, a + W + 1, a + W))
    return meshgen.from_faces(xyz, np.array(f, np.uint32))


def test_paths_that_overflow_the_default_row_and_paths_that_fit_in_one_call(gpu_ctx_factory):
    W, L = 4, 4000
    rng = np.random.default_rng(21)
    mesh = corridor(W, L, 0.1, rng)
    case = Case(mesh)
    row = int(min(16.0 * np.sqrt(mesh.V) + 1024.0, mesh.V))            # the default path row (mnav.hip, default_path_stride): 3047 ids
    n = 24
    seeds = rng.integers(0, W * 100, n).astype(np.uint32)              # near one end
    targets = (mesh.V - 1 - rng.integers(0, W * 100, n)).astype(np.uint32)   # near the other end: paths of ~3900 vertices ...
    targets[::3] = seeds[::3] + W * rng.integers(20, 600, targets[::3].size).astype(np.uint32)   # ... and every third plan a short one
    refs = [case.om.dijkstra(case.weights, case.costs, int(s), int(t)) for s, t in zip(seeds, targets)]
    lens = np.array([len(r.path) for r in refs])
    assert all(r.code == 0 for r in refs)
    assert (lens > row).sum() >= 8 and ((lens > 0) & (lens <= row)).sum() >= 4, (row, lens)   # both kinds, by the oracle alone
    ctx = gpu_ctx_factory()
    try:
        case.upload(ctx)
        for engine in ("tile_batch", "tiled", "async"):
            ctx.set_dijkstra_engine(engine)
            for fields in (False, True):
                b = ctx.plan_dijkstra_batch(seeds, targets, want_fields=fields)
                for k in range(n):
                    assert b["codes"][k] == 0, (engine, fields, k)
                    assert len(b["paths"][k]) == lens[k], (engine, fields, k, len(b["paths"][k]), lens[k])
                    assert np.array_equal(b["paths"][k], refs[k].path), (engine, fields, k)
        # a call in which every path fits, right behind one that fell back: the device's offsets again
        ctx.set_dijkstra_engine("tile_batch")
        short = np.flatnonzero(lens <= row)
        b = ctx.plan_dijkstra_batch(seeds[short], targets[short], want_fields=False)
        for i, k in enumerate(short):
            assert b["codes"][i] == 0 and np.array_equal(b["paths"][i], refs[k].path), k
    finally:
        ctx.close()
